"""Float64 references for the training kernels (csrc/train.hip) at any depth and any odd kernel: the net of riser/nets/cnn.py -
n_layers x [depth x (Conv1d(k_i, 'same') + ReLU), MaxPool1d(2, 2)], `gap_fc` - in torch (autograd), and the same forward and
backward pass in numpy.  The numpy backward takes the decisions of the forward pass as INPUTS - per pooling conv the selectors
and the gates of the pooled rows, per inner conv (one that is not the last of its layer) the ReLU gate of every row - so that a
backward kernel can be held to float64 given the device's own forward decisions: that measures one kernel's rounding, not a
decision fp32 may legitimately take the other way.  The shipped class is the net at depth 1 with every kernel 3.

Convs are numbered j = layer * depth + d as on the device.  Arrays are position-major [B, T, C]; a pooling conv's buffers have
T >> 1 rows, an inner conv's all T.  Selectors are 0 / 1 per pooled element (1: conv row 2 j + 1 won), gates are value > 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

FRAGILE_EPS = 1e-5
# defects backward64 (tie_to_odd: forward64) plants on purpose: the shipped class's list and the generic family's
SHIPPED_DEFECTS = ("tie_to_odd", "odd_row_gradient", "taps_unflipped", "prev_read_neighbour", "bias_skips_last_pair")
GENERIC_DEFECTS = ("taps_unflipped", "half_width_1", "inner_gate_skipped", "selector_on_inner", "inner_odd_row_withheld",
                   "bias_per_tap_group")

# (channels, kernels, depth, B, L, seed) of the generic device tests; test_gtrain_cpu.py holds the seeds' fragile share down
CASES = {
    "depth2": ([3, 7, 18], [5, 3, 7], 2, 3, 100, 11),       # rows 100, 50, 25 (odd): the 4-channel pad, the 16-column tile edge
    "depth3": ([3, 7, 18], [5, 3, 7], 3, 3, 100, 13),       # an inner conv behind an inner conv
    "wider_than_read": ([4, 6], [3, 9], 2, 2, 6, 13),       # layer 1 has 3 rows: the taps reach past both ends
    "taps1": ([17, 33], [1, 1], 1, 2, 50, 14),              # one tap group of 1
    "taps5": ([17, 33], [5, 5], 1, 2, 50, 15),              # 3 + 2
    "taps7": ([17, 33], [7, 7], 1, 2, 50, 16),              # 3 + 3 + 1
    "slices": ([5, 17], [5, 5], 2, 2, 9002, 23),            # conv 0 contracts 18 004 positions: several slices, the last short
    "block": ([160, 130], [3, 7], 1, 2, 260, 32),           # conv 1: 160 channels a tap forward, 130 backward - two 128-blocks
}
SMALL = ("depth2", "depth3", "wider_than_read", "taps1", "taps5", "taps7")


def case_of(name, bias=None):
    channels, kernels, depth, B, L, seed = CASES[name]
    x, y = make_batch(B, L, seed + 100)
    return make_state(channels, kernels, depth, seed, bias), x, y


def constant_reads(B, L):
    return np.repeat(np.array([0.75, -1.25, 0.5], np.float32)[:B, None], L, axis=1), np.array([1, 0, 1])[:B]


def slice_plan(B, L, level, c_in, c_out, k):
    """csrc/train/plan.hpp's arithmetic: slices of about 256 positions, their partial tiles - (c_out c_in k + c_out) floats
    each - within 32 MiB, and no more slices than a grid's y extent"""
    positions = B * (L >> level)
    cap = max(1, (32 << 20) // ((c_out * c_in * k + c_out) * 4))
    n = max(1, min(-(-positions // 256), cap, 65535))
    s = -(-(-(-positions // n)) // 4) * 4
    return max(1, -(-positions // s)), s


def convs_of(channels, kernels, depth):
    c_in = 1
    for i, (c, k) in enumerate(zip(channels, kernels)):
        for _ in range(depth):
            yield i, c_in, c, k
            c_in = c


def special_cases():
    """the depth-2 net on constant reads: ("ties": nearly every pool pair an exact tie; "dead": bias -50, no unit alive)"""
    channels, kernels, depth = CASES["depth2"][:3]
    x, y = constant_reads(3, 100)
    yield "ties", make_state(channels, kernels, depth, 13), x, y
    yield "dead", make_state(channels, kernels, depth, 13, bias=-50.0), x, y


def conv_keys(sd):
    """[(key prefix, pools)] in launch order: layers.{i}.{2 d}, the last conv of every layer pools"""
    out, i = [], 0
    while f"layers.{i}.0.weight" in sd:
        d = 0
        while f"layers.{i}.{2 * d}.weight" in sd:
            d += 1
        out += [(f"layers.{i}.{2 * e}", e == d - 1) for e in range(d)]
        i += 1
    return out


def make_state(channels, kernels, depth, seed, bias=None):
    """{reference key: float32 array}: uniform weights at 0.9 of the He bound, small biases (or the constant `bias`)"""
    rng = np.random.RandomState(seed)
    sd, c_in = {}, 1
    for i, (c, k) in enumerate(zip(channels, kernels)):
        for d in range(depth):
            a = 0.9 * np.sqrt(6.0 / (k * c_in))
            sd[f"layers.{i}.{2 * d}.weight"] = rng.uniform(-a, a, (c, c_in, k)).astype(np.float32)
            sd[f"layers.{i}.{2 * d}.bias"] = (rng.uniform(-0.05, 0.05, c) if bias is None else np.full(c, bias)).astype(np.float32)
            c_in = c
    a = np.sqrt(3.0 / c_in) * 2
    sd["classifier.2.weight"] = rng.uniform(-a, a, (2, c_in)).astype(np.float32)
    sd["classifier.2.bias"] = rng.uniform(-0.1, 0.1, 2).astype(np.float32)
    return sd


def make_batch(B, L, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((B, L)).astype(np.float32), rng.randint(0, 2, B).astype(np.int64)


def torch_forward(p, x, dtype, keep=None):
    """logits of the net with the parameter tensors `p`; `keep` collects every conv's output buffer (inner: the ReLU rows,
    pooling: the pooled rows)"""
    h = torch.as_tensor(x, dtype=dtype).unsqueeze(1)
    for key, pools in conv_keys(p):
        w = p[key + ".weight"]
        h = F.relu(F.conv1d(h, w, p[key + ".bias"], padding=w.shape[2] // 2))
        if pools:
            h = F.max_pool1d(h, 2, 2)
        if keep is not None:
            h.retain_grad()
            keep.append(h)
    return h.mean(2) @ p["classifier.2.weight"].T + p["classifier.2.bias"]


def torch_loss_and_grads(sd, x, y, dtype=torch.float64):
    """-> (loss, {key: grad}, [gradient arriving at conv j's output buffer, position-major], logits); float64 numpy whatever
    `dtype` the arithmetic ran in"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    kept = []
    logits = torch_forward(p, x, dtype, kept)
    loss = F.cross_entropy(logits, torch.tensor(y, dtype=torch.long))
    loss.backward()
    grads = {k: v.grad.double().numpy() for k, v in p.items()}
    dys = [t.grad.double().numpy().transpose(0, 2, 1) for t in kept]
    return float(loss.detach()), grads, dys, logits.detach().double().numpy()


def forward64(sd, x, tie_to_odd=False):
    """float64 numpy forward -> dict(a=[input of every conv, then the last pooled rows], z=[conv + bias rows], sel (None for
    an inner conv), gate (of the output buffer's rows), gap, logits).  `tie_to_odd`: the defect of that name, planted in
    every pool."""
    a = [np.asarray(x, np.float64)[:, :, None]]
    zs, sels, gates = [], [], []
    for key, pools in conv_keys(sd):
        w, b = sd[key + ".weight"].astype(np.float64), sd[key + ".bias"].astype(np.float64)
        k = w.shape[2]
        h, T = k // 2, a[-1].shape[1]
        ap = np.pad(a[-1], ((0, 0), (h, h), (0, 0)))
        z = sum(ap[:, t:t + T, :] @ w[:, :, t].T for t in range(k)) + b
        r = np.maximum(z, 0.0)
        zs.append(z)
        if pools:
            Th = T >> 1
            r0, r1 = r[:, 0:2 * Th:2], r[:, 1:2 * Th:2]
            sel = (r1 >= r0) if tie_to_odd else (r1 > r0)   # torch: row 2 j wins unless row 2 j + 1 is strictly larger
            out = np.where(sel, r1, r0)
            sels.append(sel.astype(np.uint8))
        else:
            out = r
            sels.append(None)
        gates.append(out > 0)
        a.append(out)
    gap = a[-1].mean(1)
    logits = gap @ sd["classifier.2.weight"].astype(np.float64).T + sd["classifier.2.bias"].astype(np.float64)
    return dict(a=a, z=zs, sel=sels, gate=gates, gap=gap, logits=logits)


def loss64(logits, y):
    m = logits.max(1, keepdims=True)
    lse = (m + np.log(np.exp(logits - m).sum(1, keepdims=True)))[:, 0]
    return float(np.mean(lse - logits[np.arange(len(y)), y]))


def backward64(sd, fwd, y, sels=None, gates=None, defect=None):
    """float64 numpy backward on the activations of `fwd`, through the given selectors and gates (default: fwd's own) ->
    ({key: grad}, [gradient arriving at conv j's output buffer]).  `defect`: one of SHIPPED_DEFECTS (but tie_to_odd, which is
    forward64's) or GENERIC_DEFECTS planted on purpose."""
    sels = fwd["sel"] if sels is None else sels
    gates = fwd["gate"] if gates is None else gates
    convs, B = conv_keys(sd), len(y)
    logits = fwd["logits"]
    m = logits.max(1, keepdims=True)
    sm = np.exp(logits - m)
    sm /= sm.sum(1, keepdims=True)
    dl = (sm - np.eye(2)[y]) / B
    grads = {"classifier.2.weight": dl.T @ fwd["gap"], "classifier.2.bias": dl.sum(0)}
    T_last = fwd["a"][-1].shape[1]
    dy = np.repeat(((dl @ sd["classifier.2.weight"].astype(np.float64)) / T_last)[:, None, :], T_last, axis=1)
    dys = [None] * len(convs)
    for j in range(len(convs) - 1, -1, -1):
        key, pools = convs[j]
        dys[j] = dy
        w = sd[key + ".weight"].astype(np.float64)
        k = w.shape[2]
        h = 1 if (defect == "half_width_1" and k > 3) else k // 2
        a_in = fwd["a"][j]
        T, Th = a_in.shape[1], a_in.shape[1] >> 1
        gate = np.asarray(gates[j], bool)
        bias_rows = T
        if pools:
            g = dy * gate
            dz = np.zeros((B, T, w.shape[0]))
            dz[:, 0:2 * Th:2] = g * (np.asarray(sels[j]) == 0)
            dz[:, 1:2 * Th:2] = g * (np.asarray(sels[j]) == 1)
            if defect == "odd_row_gradient" and T & 1:
                dz[:, T - 1] = g[:, Th - 1]
            if defect == "bias_skips_last_pair":
                bias_rows = 2 * Th - 2
        else:
            dz = dy * (1.0 if defect == "inner_gate_skipped" else gate)
            if defect == "selector_on_inner":               # the inner conv treated as if a pool followed it
                r = fwd["a"][j + 1]
                odd_wins = r[:, 1:2 * Th:2] > r[:, 0:2 * Th:2]
                dz[:, 0:2 * Th:2] *= ~odd_wins
                dz[:, 1:2 * Th:2] *= odd_wins
            if defect == "inner_odd_row_withheld" and T & 1:
                dz[:, T - 1] = 0.0
        pad = max(h, k - 1 - h)
        ap = np.pad(a_in, ((0, 0), (pad, pad), (0, 0)))
        zp = np.pad(dz, ((0, 0), (pad, pad), (0, 0)))
        if defect == "prev_read_neighbour":                 # reads back to back: the rows in front of read b are read b - 1's last
            n = min(pad, T)
            ap[1:, pad - n:pad] = a_in[:-1, T - n:]
        # dW[.., t] pairs dz[u] with a[u + t - h]; dY_prev[u] takes W[.., t] dz[u + h - t]
        grads[key + ".weight"] = np.stack([np.einsum("buo,bui->oi", dz, ap[:, pad + t - h:pad + t - h + T]) for t in range(k)], axis=2)
        groups = -(-k // 3) if defect == "bias_per_tap_group" else 1
        grads[key + ".bias"] = groups * dz[:, :bias_rows].sum((0, 1))
        if j:
            if defect == "taps_unflipped" and k > 1:
                dy = sum(zp[:, pad + t - h:pad + t - h + T] @ w[:, :, t] for t in range(k))
            else:
                dy = sum(zp[:, pad + h - t:pad + h - t + T] @ w[:, :, t] for t in range(k))
    return grads, dys


def fragile(fwd):
    """per conv a bool array in the shape of its output buffer: elements whose decision fp32 may legitimately take the other
    way.  Pooling conv: the two rows closer than FRAGILE_EPS max|z| of the conv, or the winner that close to zero; inner conv:
    a z that close to zero.  Exact ties and exact zeros apart."""
    out = []
    for z, sel in zip(fwd["z"], fwd["sel"]):
        lim = FRAGILE_EPS * np.abs(z).max()
        if sel is None:
            out.append((np.abs(z) <= lim) & (z != 0))
            continue
        Th = z.shape[1] >> 1
        z0, z1 = z[:, 0:2 * Th:2], z[:, 1:2 * Th:2]
        d, win = np.abs(z0 - z1), np.maximum(z0, z1)
        out.append(((d <= lim) & (d != 0)) | ((np.abs(win) <= lim) & (win != 0)))
    return out


def fragile_share(fwd):
    frag = fragile(fwd)
    return sum(int(f.sum()) for f in frag) / sum(f.size for f in frag)


def gap_of(got, want):
    """largest absolute difference over a tensor, divided by the largest magnitude of the float64 tensor"""
    want = np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (scale if scale > 0 else 1.0))


def bars_of(sd, x, y, floor=1e-6):
    """per tensor four times the gap torch's own fp32 CPU autograd shows against float64 on the same inputs, at least `floor`:
    the device sums in another order and the MFMA does not round as sequential FMAs do -> ({key: bar}, [bar of conv j's
    incoming gradient], bar of the loss, bar of the logits, float64 (loss, grads, dys, logits))"""
    l64, g64, d64, lg64 = torch_loss_and_grads(sd, x, y, torch.float64)
    l32, g32, d32, lg32 = torch_loss_and_grads(sd, x, y, torch.float32)
    bars = {k: max(4 * gap_of(g32[k], g64[k]), floor) for k in g64}
    dbars = [max(4 * gap_of(a, b), floor) for a, b in zip(d32, d64)]
    return bars, dbars, max(4 * abs(l32 - l64) / abs(l64), floor), max(4 * gap_of(lg32, lg64), floor), (l64, g64, d64, lg64)


def torch_adam(sd, x, y, dtype, steps, lr):
    """`steps` of torch.optim.Adam on the net -> (losses, {key: float64 parameters})"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    losses = []
    for _ in range(steps):
        loss = F.cross_entropy(torch_forward(p, x, dtype), torch.tensor(y, dtype=torch.long))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach().double().numpy() for k, v in p.items()}
