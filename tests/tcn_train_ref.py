"""Float64 references for TCN training (csrc/tcn_train.hip): the dense net of riser/nets/tcn.py as a torch functional on the
weight-norm parameters (g, v, b) with autograd and the dropout masks applied as tensors; the same forward and backward pass in
numpy on the receptive cone of the last sample, whose backward takes the gates - value > 0 of a1, a2 and out of every block -
as INPUTS, so that the device's backward can be held to float64 given the device's own forward decisions; and the numpy mirror
of the dropout hash (include/riser_amd.h).

Cone arrays are position-major [B, rows, C]: row m of block i's input and a1 is position L-1 - d_i m, row m' of its a2 and out
is position L-1 - d_i base m'.  Tap j of a conv on those rows is the reference's tap k - 1 - j.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from train_ref import gap_of, loss64, make_batch  # noqa: F401  (shared with the ConvNet's reference)

FRAGILE_EPS = 1e-5
DEFECTS = ("bias_counts_rows_below_0", "residual_at_unstrided_row", "taps_unflipped", "stride_ignored", "dropout_scale_missing",
           "mask_keyed_on_p", "dv_without_projection", "dg_dropped", "unapplied_shortcut_gradient")
NETS = (("tcn.npz", "tcn_k3_b2"), ("tcn.npz", "tcn_k5_b3"), ("tcn_edges.npz", "tcn_f1_k2"), ("tcn_edges.npz", "tcn_f68"),
        ("tcn_edges.npz", "tcn_k5_l1"), ("tcn_edges.npz", "tcn_k2_b4"))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B_CASE = 5


def load_net(name):
    """(cfg dict, {key: float32 array}) of a golden net"""
    g = np.load(os.path.join(GOLDEN, dict((n, f) for f, n in NETS)[name]))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    pre = f"{name}.sd."
    return cfg, {k[len(pre):]: np.asarray(g[k]) for k in g.files if k.startswith(pre)}


def lengths_of(name, cfg):
    """the lengths of the device cases: below, at and above the receptive field; the net whose every window is clamped also at
    1500, the main net also at one sample and at k - 1"""
    rf = cfg["rf"]
    extra = {"tcn_k2_b4": [1500], "tcn_k3_b2": [1, cfg["kernel"] - 1]}.get(name, [])
    return extra + [rf // 2, rf, rf + 37]


def case_seed(name, L):
    return 1000 * [n for _, n in NETS].index(name) + L % 997


def applied(cfg, i):
    return (1 if i == 0 else cfg["n_filters"]) != cfg["n_filters"]


def device_keys(cfg):
    keys = []
    for i in range(cfg["n_layers"]):
        for j in (0, 1):
            keys += [f"layers.{i}.blocks.{j}.0.weight_g", f"layers.{i}.blocks.{j}.0.weight_v", f"layers.{i}.blocks.{j}.0.bias"]
        if applied(cfg, i):
            keys += [f"layers.{i}.shortcut.weight", f"layers.{i}.shortcut.bias"]
    return keys + ["linear.weight", "linear.bias"]


# ---- the dropout hash ----------------------------------------------------------------------------------------------------------

M32 = np.uint64(0xFFFFFFFF)


def mix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & M32
    h ^= h >> np.uint64(16)
    return h


def drop_key(seed, counter, conv):
    h = mix32((seed & 0xFFFFFFFF) + 0x9e3779b9)
    for word in ((seed >> 32) & 0xFFFFFFFF, counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, conv):
        h = mix32(h + np.uint64(word))
    return h


def drop_hash(key, read, q, ch):
    """broadcasts over read, q, ch"""
    h = mix32(key + np.asarray(read, np.uint64))
    h = mix32(h + (np.asarray(q, np.uint64) & M32))
    return mix32(h + np.asarray(ch, np.uint64))


def threshold(p):
    return int(np.floor(float(p) * 4294967296.0))


def scale_of(p):
    return float(np.float32(1.0 / (1.0 - p))) if threshold(p) else 1.0


def keep_mask(p, seed, counter, conv, B, q, C):
    """bool [B, len(q), C]: the elements of conv `conv` kept at the distances `q` from the end"""
    q = np.asarray(q, np.int64)
    if not threshold(p):
        return np.ones((B, len(q), C), bool)
    h = drop_hash(drop_key(seed, counter, conv), np.arange(B)[:, None, None], q[None, :, None], np.arange(C)[None, None, :])
    return h >= np.uint64(threshold(p))


# ---- the cone --------------------------------------------------------------------------------------------------------------------

def cone(cfg, L):
    """per block (rows in, rows of a1, rows out, dilation): riser_amd.tcn.windows' arithmetic"""
    n, k, base = cfg["n_layers"], cfg["kernel"], cfg["dilation"]
    need = [0] * (n + 1)
    need[n] = 1
    for i in range(n - 1, -1, -1):
        need[i] = min((need[i + 1] - 1) * base + 1 + 2 * (k - 1), -(-L // base ** i))
    return [(need[i], min((need[i + 1] - 1) * base + k, need[i]), need[i + 1], base ** i) for i in range(n)]


def masks_of(cfg, B, L, p, seed, counter, keyed_on_p=False):
    """per block (mask of a1 [B, R1, F], mask of a2 [B, Ro, F]) - None where p applies none.  keyed_on_p: the defect of that
    name, the hash fed the position instead of the distance from the end."""
    if not threshold(p):
        return None
    out = []
    for i, (_, r1, ro, d) in enumerate(cone(cfg, L)):
        q1, q2 = d * np.arange(r1), d * cfg["dilation"] * np.arange(ro)
        if keyed_on_p:
            q1, q2 = L - 1 - q1, L - 1 - q2
        out.append((keep_mask(p, seed, counter, 2 * i, B, q1, cfg["n_filters"]),
                    keep_mask(p, seed, counter, 2 * i + 1, B, q2, cfg["n_filters"])))
    return out


def dense_masks(cfg, B, L, p, seed, counter):
    """the same masks over all L positions, [B, F, L] per conv, for the dense torch net"""
    if not threshold(p):
        return None
    q = L - 1 - np.arange(L)
    return [tuple(keep_mask(p, seed, counter, 2 * i + j, B, q, cfg["n_filters"]).transpose(0, 2, 1) for j in (0, 1))
            for i in range(cfg["n_layers"])]


def fold64(sd, prefix):
    v = sd[prefix + ".weight_v"].astype(np.float64)
    g = sd[prefix + ".weight_g"].astype(np.float64).reshape(-1, 1, 1)
    return g * v / np.sqrt((v * v).sum((1, 2), keepdims=True))


def _taps(a, rows, stride, k):
    """[a[:, stride m + j] for j < k], m < rows, zero beyond the buffer"""
    ap = np.pad(a, ((0, 0), (0, max(0, stride * (rows - 1) + k - a.shape[1])), (0, 0)))
    return [ap[:, j:j + stride * (rows - 1) + 1:stride] for j in range(k)]


def forward64(sd, cfg, x, p=0.0, masks=None):
    """float64 cone forward -> dict(blocks=[dict(x, z1, a1, z2, a2, zo, out)], logits)"""
    x = np.asarray(x, np.float64)
    B, L = x.shape
    k, base, s = cfg["kernel"], cfg["dilation"], scale_of(p) if masks is not None else 1.0
    blocks = []
    h = x[:, ::-1][:, :cone(cfg, L)[0][0], None]
    for i, (rin, r1, ro, d) in enumerate(cone(cfg, L)):
        pre = f"layers.{i}"
        w1, w2 = fold64(sd, pre + ".blocks.0.0"), fold64(sd, pre + ".blocks.1.0")
        h = h[:, :rin]
        z1 = sum(t @ w1[:, :, k - 1 - j].T for j, t in enumerate(_taps(h, r1, 1, k))) + sd[pre + ".blocks.0.0.bias"].astype(np.float64)
        a1 = np.maximum(z1, 0.0) * (masks[i][0] * s if masks is not None else 1.0)
        z2 = sum(t @ w2[:, :, k - 1 - j].T for j, t in enumerate(_taps(a1, ro, base, k))) + sd[pre + ".blocks.1.0.bias"].astype(np.float64)
        a2 = np.maximum(z2, 0.0) * (masks[i][1] * s if masks is not None else 1.0)
        xs = _taps(h, ro, base, 1)[0]
        res = xs @ sd[pre + ".shortcut.weight"][:, :, 0].astype(np.float64).T + sd[pre + ".shortcut.bias"].astype(np.float64) \
            if applied(cfg, i) else xs
        zo = a2 + res
        blocks.append(dict(x=h, z1=z1, a1=a1, z2=z2, a2=a2, zo=zo, out=np.maximum(zo, 0.0)))
        h = blocks[-1]["out"]
    logits = h[:, 0] @ sd["linear.weight"].astype(np.float64).T + sd["linear.bias"].astype(np.float64)
    return dict(blocks=blocks, logits=logits)


def gates_of(fwd):
    """per block (a1 > 0, a2 > 0, out > 0): what the backward gates on"""
    return [(b["a1"] > 0, b["a2"] > 0, b["out"] > 0) for b in fwd["blocks"]]


def backward64(sd, cfg, fwd, y, p=0.0, gates=None, defect=None):
    """float64 cone backward on the activations of `fwd` through the given gates (default: fwd's own) -> ({key: grad},
    [gradient arriving at block i's out], [gradient arriving at block i's a1]).  `defect`: one of DEFECTS (but mask_keyed_on_p,
    which is masks_of's) planted on purpose."""
    gates = gates_of(fwd) if gates is None else gates
    k, base, B = cfg["kernel"], cfg["dilation"], len(y)
    s = 1.0 if defect == "dropout_scale_missing" else scale_of(p)
    logits = fwd["logits"]
    sm = np.exp(logits - logits.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    dl = (sm - np.eye(2)[y]) / B
    grads = {"linear.weight": dl.T @ fwd["blocks"][-1]["out"][:, 0], "linear.bias": dl.sum(0)}
    dout = (dl @ sd["linear.weight"].astype(np.float64))[:, None, :]
    douts, da1s = [None] * cfg["n_layers"], [None] * cfg["n_layers"]
    for i in range(cfg["n_layers"] - 1, -1, -1):
        pre, blk = f"layers.{i}", fwd["blocks"][i]
        g1, g2, go = (np.asarray(g, bool) for g in gates[i])
        rin, r1, ro = blk["x"].shape[1], blk["a1"].shape[1], blk["out"].shape[1]
        w1, w2 = fold64(sd, pre + ".blocks.0.0"), fold64(sd, pre + ".blocks.1.0")
        douts[i] = dout
        g = dout * go
        dz2 = g * g2 * s
        dw2 = np.stack([np.einsum("bmo,bmi->oi", dz2, t) for t in _taps(blk["a1"], ro, base, k)][::-1], axis=2)
        grads[pre + ".blocks.1.0.bias"] = dz2.sum((0, 1))
        xs = _taps(blk["x"], ro, base, 1)[0]
        if applied(cfg, i) or defect == "unapplied_shortcut_gradient":
            grads[pre + ".shortcut.weight"] = np.einsum("bmo,bmi->oi", g, xs)[:, :, None]
            grads[pre + ".shortcut.bias"] = g.sum((0, 1))
        # dA1 on every row the taps reach; the rows beyond r1 are positions below 0 and take no gradient
        stride = 1 if defect == "stride_ignored" else base
        full = max(stride * (ro - 1) + k, r1)
        da1 = np.zeros((B, full, w2.shape[1]))
        for j in range(k):
            tap = j if defect == "taps_unflipped" else k - 1 - j
            da1[:, j:j + stride * (ro - 1) + 1:stride] += dz2 @ w2[:, :, tap]
        below0, da1 = da1[:, r1:], da1[:, :r1]
        da1s[i] = da1
        dz1 = da1 * g1 * s
        dw1 = np.stack([np.einsum("bmo,bmi->oi", dz1, t) for t in _taps(blk["x"], r1, 1, k)][::-1], axis=2)
        grads[pre + ".blocks.0.0.bias"] = dz1.sum((0, 1))
        if defect == "bias_counts_rows_below_0":            # a row below 0 holds relu(bias) where it is not zeroed
            grads[pre + ".blocks.0.0.bias"] = grads[pre + ".blocks.0.0.bias"] + \
                (below0 * (sd[pre + ".blocks.0.0.bias"] > 0) * s).sum((0, 1))
        for j, dw in ((0, dw1), (1, dw2)):
            cp = f"{pre}.blocks.{j}.0"
            v = sd[cp + ".weight_v"].astype(np.float64)
            gg = sd[cp + ".weight_g"].astype(np.float64).reshape(-1, 1, 1)
            n2 = (v * v).sum((1, 2), keepdims=True)
            dot = (dw * v).sum((1, 2), keepdims=True)
            grads[cp + ".weight_g"] = np.zeros_like(gg) if defect == "dg_dropped" else dot / np.sqrt(n2)
            grads[cp + ".weight_v"] = (gg / np.sqrt(n2)) * (dw if defect == "dv_without_projection" else dw - dot * v / n2)
        if i == 0:
            break
        dx = np.zeros((B, rin + k, w1.shape[1]))
        for j in range(k):
            tap = j if defect == "taps_unflipped" else k - 1 - j
            dx[:, j:j + r1] += dz1 @ w1[:, :, tap]
        dx = dx[:, :rin]
        res = g @ sd[pre + ".shortcut.weight"][:, :, 0].astype(np.float64) if applied(cfg, i) else g
        if defect == "residual_at_unstrided_row":
            dx[:, :ro] += res
        else:
            dx[:, 0:base * (ro - 1) + 1:base] += res
        dout = dx
    return grads, douts, da1s


def fragile_share(fwd):
    """the share of nonzero pre-activations (z1, z2, a2 + res) within FRAGILE_EPS of their tensor's largest magnitude"""
    n = total = 0
    for b in fwd["blocks"]:
        for z in (b["z1"], b["z2"], b["zo"]):
            n += int(((np.abs(z) <= FRAGILE_EPS * np.abs(z).max()) & (z != 0)).sum())
            total += z.size
    return n / total


def fragile(fwd):
    """per block three bool arrays in the shapes of a1, a2 and out"""
    return [tuple((np.abs(z) <= FRAGILE_EPS * np.abs(z).max()) & (z != 0) for z in (b["z1"], b["z2"], b["zo"]))
            for b in fwd["blocks"]]


# ---- the dense net in torch ------------------------------------------------------------------------------------------------------

def torch_forward(p, cfg, x, dtype, drop=0.0, masks=None, keep=None, mids=None):
    """logits of the dense net on the parameter tensors `p`; `keep` collects every block's output, `mids` every a1"""
    k, base = cfg["kernel"], cfg["dilation"]
    s = scale_of(drop) if masks is not None else 1.0
    h = torch.as_tensor(x, dtype=dtype).unsqueeze(1)
    for i in range(cfg["n_layers"]):
        d, a = base ** i, h
        for j in (0, 1):
            cp = f"layers.{i}.blocks.{j}.0"
            w = torch._weight_norm(p[cp + ".weight_v"], p[cp + ".weight_g"], 0)
            a = F.relu(F.conv1d(F.pad(a, ((k - 1) * d, 0)), w, p[cp + ".bias"], dilation=d))
            if masks is not None:
                a = a * torch.as_tensor(masks[i][j], dtype=dtype) * s
            if j == 0 and mids is not None:
                a.retain_grad()
                mids.append(a)
        res = F.conv1d(h, p[f"layers.{i}.shortcut.weight"], p[f"layers.{i}.shortcut.bias"]) if applied(cfg, i) else h
        h = F.relu(a + res)
        if keep is not None:
            h.retain_grad()
            keep.append(h)
    return h[:, :, -1] @ p["linear.weight"].T + p["linear.bias"]


def torch_loss_and_grads(sd, cfg, x, y, dtype=torch.float64, drop=0.0, masks=None):
    """-> (loss, {key: grad, zeros where autograd gives none}, [gradient arriving at block i's out on the cone's rows],
    [the same at a1], logits); float64 numpy whatever `dtype` the arithmetic ran in.  masks: dense_masks'."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    kept, mids = [], []
    logits = torch_forward(p, cfg, x, dtype, drop, masks, kept, mids)
    loss = F.cross_entropy(logits, torch.tensor(np.asarray(y), dtype=torch.long))
    loss.backward()
    grads = {k: (v.grad.double().numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    L = np.asarray(x).shape[1]
    douts, da1s = [], []
    for (rin, r1, ro, d), t, m in zip(cone(cfg, L), kept, mids):
        douts.append(t.grad.double().numpy()[:, :, L - 1 - d * cfg["dilation"] * np.arange(ro)].transpose(0, 2, 1))
        da1s.append(m.grad.double().numpy()[:, :, L - 1 - d * np.arange(r1)].transpose(0, 2, 1))
    return float(loss.detach()), grads, douts, da1s, logits.detach().double().numpy()


def bars_of(sd, cfg, x, y, drop=0.0, masks=None, floor=1e-6):
    """per tensor four times the gap torch's own fp32 CPU autograd shows against float64 on the same inputs and masks, at least
    `floor` -> ({key: bar}, [bar of block i's incoming gradient], bar of the loss, bar of the logits, float64 (loss, grads,
    douts, da1s, logits))"""
    r64 = torch_loss_and_grads(sd, cfg, x, y, torch.float64, drop, masks)
    r32 = torch_loss_and_grads(sd, cfg, x, y, torch.float32, drop, masks)
    bars = {k: max(4 * gap_of(r32[1][k], r64[1][k]), floor) for k in r64[1]}
    dbars = [max(4 * gap_of(a, b), floor) for a, b in zip(r32[2], r64[2])]
    return bars, dbars, max(4 * abs(r32[0] - r64[0]) / abs(r64[0]), floor), max(4 * gap_of(r32[4], r64[4]), floor), r64


def torch_adam(sd, cfg, x, y, dtype, steps, lr, drop=0.0, masks_of_step=None):
    """`steps` of torch.optim.Adam on (g, v, b) of the dense net -> (losses, {key: float64 parameters})"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    losses = []
    for t in range(steps):
        masks = masks_of_step(t) if masks_of_step else None
        loss = F.cross_entropy(torch_forward(p, cfg, x, dtype, drop, masks), torch.tensor(np.asarray(y), dtype=torch.long))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach().double().numpy() for k, v in p.items()}
