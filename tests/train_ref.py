"""Float64 references for the training kernels (csrc/train.hip): the net of riser/nets/cnn.py at depth 1, kernel 3, `gap_fc` in a
few lines of torch (autograd), and the same forward and backward pass in numpy.  The numpy backward takes the max-pool
selectors and the ReLU gates as INPUTS, so that a backward kernel can be held to float64 given the device's own forward
decisions: that measures one kernel's rounding, not a decision fp32 may legitimately take the other way.

Arrays are position-major [B, T, C] as on the device; selectors are 0 / 1 per pooled element (1: conv row 2 j + 1 won), gates
are pooled value > 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

FRAGILE_EPS = 1e-5
DEFECTS = ("tie_to_odd", "odd_row_gradient", "taps_unflipped", "prev_read_neighbour", "bias_skips_last_pair")


def make_state(channels, seed, bias=None):
    """{reference key: float32 array}: uniform weights at 0.9 of the He bound, small biases (or the constant `bias`)"""
    rng = np.random.RandomState(seed)
    sd, c_in = {}, 1
    for i, c in enumerate(channels):
        a = 0.9 * np.sqrt(6.0 / (3 * c_in))
        sd[f"layers.{i}.0.weight"] = rng.uniform(-a, a, (c, c_in, 3)).astype(np.float32)
        sd[f"layers.{i}.0.bias"] = (rng.uniform(-0.05, 0.05, c) if bias is None else np.full(c, bias)).astype(np.float32)
        c_in = c
    a = np.sqrt(3.0 / c_in) * 2
    sd["classifier.2.weight"] = rng.uniform(-a, a, (2, c_in)).astype(np.float32)
    sd["classifier.2.bias"] = rng.uniform(-0.1, 0.1, 2).astype(np.float32)
    return sd


def make_batch(B, L, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((B, L)).astype(np.float32), rng.randint(0, 2, B).astype(np.int64)


def n_layers_of(sd):
    return sum(1 for k in sd if k.startswith("layers.") and k.endswith(".weight"))


def torch_loss_and_grads(sd, x, y, dtype=torch.float64):
    """the net in torch on the CPU -> (loss, {key: grad}, [dY_l per layer, position-major], logits); everything float64
    numpy whatever `dtype` the arithmetic ran in"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    h = torch.tensor(x, dtype=dtype).unsqueeze(1)
    pooled = []
    for i in range(n_layers_of(sd)):
        h = F.max_pool1d(F.relu(F.conv1d(h, p[f"layers.{i}.0.weight"], p[f"layers.{i}.0.bias"], padding=1)), 2, 2)
        h.retain_grad()
        pooled.append(h)
    logits = h.mean(2) @ p["classifier.2.weight"].T + p["classifier.2.bias"]
    loss = F.cross_entropy(logits, torch.tensor(y, dtype=torch.long))
    loss.backward()
    grads = {k: v.grad.double().numpy() for k, v in p.items()}
    dys = [t.grad.double().numpy().transpose(0, 2, 1) for t in pooled]
    return float(loss.detach()), grads, dys, logits.detach().double().numpy()


def forward64(sd, x, tie_to_odd=False):
    """float64 numpy forward -> dict(a=[inputs of every layer, then the last pooled rows] [B, T, C], z=[conv + bias rows],
    sel, gate, gap, logits)"""
    a = [np.asarray(x, np.float64)[:, :, None]]
    zs, sels, gates = [], [], []
    for i in range(n_layers_of(sd)):
        w, b = sd[f"layers.{i}.0.weight"].astype(np.float64), sd[f"layers.{i}.0.bias"].astype(np.float64)
        ap = np.pad(a[-1], ((0, 0), (1, 1), (0, 0)))
        T = a[-1].shape[1]
        z = sum(ap[:, k:k + T, :] @ w[:, :, k].T for k in range(3)) + b
        r = np.maximum(z, 0.0)
        Th = T >> 1
        r0, r1 = r[:, 0:2 * Th:2], r[:, 1:2 * Th:2]
        sel = (r1 >= r0) if tie_to_odd else (r1 > r0)       # torch: row 2 j wins unless row 2 j + 1 is strictly larger
        yl = np.where(sel, r1, r0)
        zs.append(z)
        sels.append(sel.astype(np.uint8))
        gates.append(yl > 0)
        a.append(yl)
    gap = a[-1].mean(1)
    logits = gap @ sd["classifier.2.weight"].astype(np.float64).T + sd["classifier.2.bias"].astype(np.float64)
    return dict(a=a, z=zs, sel=sels, gate=gates, gap=gap, logits=logits)


def loss64(logits, y):
    m = logits.max(1, keepdims=True)
    lse = (m + np.log(np.exp(logits - m).sum(1, keepdims=True)))[:, 0]
    return float(np.mean(lse - logits[np.arange(len(y)), y]))


def backward64(sd, fwd, y, sels=None, gates=None, defect=None):
    """float64 numpy backward on the activations of `fwd`, through the given selectors and gates (default: fwd's own) ->
    ({key: grad}, [dY_l per layer]).  `defect`: one of DEFECTS (but tie_to_odd, which is forward64's) planted on purpose."""
    sels = fwd["sel"] if sels is None else sels
    gates = fwd["gate"] if gates is None else gates
    n, B = n_layers_of(sd), len(y)
    logits = fwd["logits"]
    m = logits.max(1, keepdims=True)
    sm = np.exp(logits - m)
    sm /= sm.sum(1, keepdims=True)
    dl = (sm - np.eye(2)[y]) / B
    grads = {"classifier.2.weight": dl.T @ fwd["gap"], "classifier.2.bias": dl.sum(0)}
    T_last = fwd["a"][-1].shape[1]
    dy = np.repeat(((dl @ sd["classifier.2.weight"].astype(np.float64)) / T_last)[:, None, :], T_last, axis=1)
    dys = [None] * n
    for l in range(n - 1, -1, -1):
        dys[l] = dy
        w = sd[f"layers.{l}.0.weight"].astype(np.float64)
        a_in = fwd["a"][l]
        T, Th = a_in.shape[1], a_in.shape[1] >> 1
        g = dy * np.asarray(gates[l], bool)
        dz = np.zeros((B, T, w.shape[0]))
        dz[:, 0:2 * Th:2] = g * (np.asarray(sels[l]) == 0)
        dz[:, 1:2 * Th:2] = g * (np.asarray(sels[l]) == 1)
        if defect == "odd_row_gradient" and T & 1:
            dz[:, T - 1] = g[:, Th - 1]
        ap = np.pad(a_in, ((0, 0), (1, 1), (0, 0)))
        if defect == "prev_read_neighbour":                 # reads back to back: row -1 of read b is the last row of read b - 1
            ap[1:, 0] = a_in[:-1, T - 1]
        grads[f"layers.{l}.0.weight"] = np.stack([np.einsum("buo,bui->oi", dz, ap[:, k:k + T]) for k in range(3)], axis=2)
        grads[f"layers.{l}.0.bias"] = (dz[:, :2 * Th - 2] if defect == "bias_skips_last_pair" else dz).sum((0, 1))
        if l:
            zp = np.pad(dz, ((0, 0), (1, 1), (0, 0)))
            if defect == "taps_unflipped":
                dy = sum(zp[:, k:k + T] @ w[:, :, k] for k in range(3))
            else:
                dy = sum(zp[:, 2 - k:2 - k + T] @ w[:, :, k] for k in range(3))
    return grads, dys


def fragile(fwd):
    """per layer a bool [B, T >> 1, C]: pooled elements whose decision fp32 may legitimately take the other way - the two
    rows closer than FRAGILE_EPS max|z| of the layer, or the winner that close to zero - apart from exact ties"""
    out = []
    for z in fwd["z"]:
        Th = z.shape[1] >> 1
        z0, z1 = z[:, 0:2 * Th:2], z[:, 1:2 * Th:2]
        lim = FRAGILE_EPS * np.abs(z).max()
        d, win = np.abs(z0 - z1), np.maximum(z0, z1)
        out.append(((d <= lim) & (d != 0)) | ((np.abs(win) <= lim) & (win != 0)))
    return out


def gap_of(got, want):
    """largest absolute difference over a tensor, divided by the largest magnitude of the float64 tensor"""
    want = np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (scale if scale > 0 else 1.0))


def bars_of(sd, x, y, floor=1e-6):
    """per tensor four times the gap torch's own fp32 autograd shows against float64 on the same inputs, at least `floor`:
    the device sums in another order and the MFMA does not round as sequential FMAs do -> ({key: bar}, [bar of dY_l], bar of
    the loss, float64 (loss, grads, dys, logits))"""
    l64, g64, d64, lg64 = torch_loss_and_grads(sd, x, y, torch.float64)
    l32, g32, d32, _ = torch_loss_and_grads(sd, x, y, torch.float32)
    bars = {k: max(4 * gap_of(g32[k], g64[k]), floor) for k in g64}
    dbars = [max(4 * gap_of(a, b), floor) for a, b in zip(d32, d64)]
    return bars, dbars, max(4 * abs(l32 - l64) / abs(l64), floor), (l64, g64, d64, lg64)
