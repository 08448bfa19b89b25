"""Float64 reference of the TCN / TCNBot forward, the strided-cone formulation the device computes (csrc/tcn.hip), its
split-precision emulation (csrc/tcn_x3.hip), mutants of both - bugs a kernel could plausibly have, which the tests must
be able to tell apart - and a mirror of the device's tile planner.  A plain module the TCN tests import."""
import numpy as np

from riser_amd import tcn as T


def dense_forward(blocks, fw, fb, x, clamp_len=None):
    """the reference's forward on the folded weights: every conv causal (left pad (k-1) d, no right side), ReLU after
    each, relu(convs + residual), Linear on the last position.  float64.  clamp_len=L caps every dilation at L: a tap at a
    dilation >= L reads only padding for a read of L samples, so the result is the same, and a net whose dilations outgrow
    any read has an exact forward without a pad of that size."""
    import torch
    import torch.nn.functional as F
    h = torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None, :]
    for b in blocks:
        d = b["dilation"] if clamp_len is None else min(b["dilation"], int(clamp_len))
        y = h
        for cv in b["convs"]:
            w = torch.from_numpy(cv["w"].astype(np.float64))
            pad = (cv["k"] - 1) * d if cv["causal"] else 0
            y = F.relu(F.conv1d(F.pad(y, (pad, 0)), w, torch.from_numpy(cv["b"].astype(np.float64)),
                                dilation=d if cv["causal"] else 1))
        if b["shortcut"] is not None:
            res = F.conv1d(h, torch.from_numpy(b["shortcut"][0].astype(np.float64))[:, :, None],
                           torch.from_numpy(b["shortcut"][1].astype(np.float64)))
        else:
            res = h
        h = F.relu(y + res)
    return (h[:, :, -1] @ torch.from_numpy(fw.astype(np.float64)).T + torch.from_numpy(fb.astype(np.float64))).numpy()


def bf16(v):
    """fp32 -> the fp32 value of its bf16 rounding, to nearest even (what v_cvt_pk_bf16_f32 and the host packer do)"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def split(v):
    v = np.asarray(v, dtype=np.float32)
    hi = bf16(v)
    return hi.astype(np.float64), bf16(v - hi).astype(np.float64)


def x3_matmul(a, w, mutant=None):
    """a [..., K] fp32 @ w [K, N] fp32 in split precision: hi*hi + lo*hi + hi*lo, accumulated in float64, rounded to fp32.
    mutant 'plain_bf16': hi*hi alone; 'no_cross': hi*hi + hi*lo (the lo*hi term missing)."""
    ah, al = split(a)
    wh, wl = split(w)
    if mutant == "plain_bf16":
        return (ah @ wh).astype(np.float32)
    if mutant == "no_cross":
        return (ah @ wh + ah @ wl).astype(np.float32)
    return (ah @ wh + al @ wh + ah @ wl).astype(np.float32)


# bugs a block kernel could have, selected by cone_forward(..., mutant=) / x3_cone_forward(..., mutant=):
#   relu_bias           a conv output below position 0 is relu(bias), not 0 (the per-conv zero padding missed)
#   unstrided_residual  the residual taken at input row q instead of q * base
#   drop_last_channel   every conv's last output channel never written (left 0)
#   read_offset         the read staged one sample off (position L-2 - m where L-1 - m is meant)
# and, in split precision only,
#   plain_bf16          hi*hi alone
#   no_cross            hi*hi + hi*lo: one cross term missing
MUTANTS = ("relu_bias", "unstrided_residual", "drop_last_channel", "read_offset")
X3_MUTANTS = MUTANTS + ("plain_bf16", "no_cross")


def _cone(blocks, fw, fb, x, ld, x3, mutant):
    ft = np.float32 if x3 else np.float64
    x = np.asarray(x, dtype=ft)
    B, L = x.shape
    need = T.windows(blocks, ld or L)
    m0 = np.arange(need[0])
    p0 = L - 2 - m0 if mutant == "read_offset" else L - 1 - m0
    cur = np.where(p0 >= 0, x[:, np.clip(p0, 0, None)], 0.0).astype(ft)[:, :, None]      # [B, need0, 1]
    for i, b in enumerate(blocks):
        d, r = b["dilation"], b["base"]
        n_out = need[i + 1]
        convs = b["convs"]
        jk = max(j for j, cv in enumerate(convs) if cv["k"] > 1)

        def valid(rows, stride):
            return (L - 1 - d * (np.arange(rows) * stride) >= 0)[None, :, None]

        def padded(a, rows):
            if a.shape[1] >= rows:
                return a[:, :rows]
            return np.concatenate([a, np.zeros((a.shape[0], rows - a.shape[1], a.shape[2]), ft)], axis=1)

        # rows of every conv's output: backwards from n_out strided outputs
        rows = [0] * len(convs)
        rows[-1] = n_out
        for j in range(len(convs) - 1, 0, -1):
            rows[j - 1] = (rows[j] - 1) * (r if j == jk else 1) + convs[j]["k"]
        y = cur
        for j, cv in enumerate(convs):
            w = cv["w"]                                                     # [co, ci, k]; tap t reads m + t
            k = cv["k"]
            step = r if j == jk else 1
            src = padded(y, (rows[j] - 1) * step + k)
            taps = [src[:, t: t + (rows[j] - 1) * step + 1: step] for t in range(k)]
            if x3:
                # K tap-major: one GEMM over the concatenated taps, as the device runs it
                wk = np.concatenate([w[:, :, k - 1 - t].T for t in range(k)], axis=0)
                out = x3_matmul(np.concatenate(taps, axis=2), wk, mutant)
            else:
                w = w.astype(np.float64)
                out = np.zeros((B, rows[j], w.shape[0]))
                for t in range(k):
                    out += taps[t] @ w[:, :, k - 1 - t].T
            bias = cv["b"].astype(ft)
            below = np.maximum(bias, ft(0)) if mutant == "relu_bias" else ft(0)
            y = np.where(valid(rows[j], r if j >= jk else 1), np.maximum(out + bias, ft(0)), below).astype(ft)
            if mutant == "drop_last_channel":
                y[:, :, -1] = 0
        xs = padded(cur, (n_out - 1) * r + 1)[:, ::r]
        if mutant == "unstrided_residual":
            xs = padded(cur, n_out)
        if b["shortcut"] is not None:
            sw, sb = b["shortcut"]
            res = x3_matmul(xs, sw.T, mutant) + sb if x3 else xs @ sw.astype(np.float64).T + sb
        else:
            res = xs
        cur = np.where(valid(n_out, r), np.maximum(y + res, ft(0)), ft(0)).astype(ft)
    return cur[:, 0].astype(np.float64) @ fw.astype(np.float64).T + fb


def cone_forward(blocks, fw, fb, x, ld=None, mutant=None):
    """the formulation of csrc/tcn.hip: block i holds positions L-1 - d_i m (m < windows()[i]) position-major, counting
    back from the last sample; every value at a position below 0 is exactly 0; inside a block the convs up to the last
    k-conv run dense over m, that conv and what follows it only at m = base * m'.  x: [B, L] (one length).  float64."""
    return _cone(blocks, fw, fb, x, ld, False, mutant)


def x3_cone_forward(blocks, fw, fb, x, ld=None, mutant=None):
    """the strided cone of csrc/tcn.hip / tcn_x3.hip with every conv - the shortcut too - in split precision and bias,
    ReLU and the residual add in fp32.  x: [B, L] fp32 (one length) -> logits float64 [B, 2]."""
    return _cone(blocks, fw, fb, x, ld, True, mutant)


# ------------------------------------------------------------------------------------------------ the tile planner
LDS_BUDGET = 64 * 1024


def _cp(c, n):
    return (c + n - 1) // n * n


def _lds_bytes(b, T, nb, x3):
    """LDS bytes of a tile of nb reads x T outputs of block b: plan_tile (fp32) / tcn_x3_plan (bf16x3)"""
    convs = b["convs"]
    jk = max(j for j, cv in enumerate(convs) if cv["k"] > 1)
    rows, need = [0] * len(convs), T
    for j in range(len(convs) - 1, -1, -1):
        rows[j] = need
        need = min(1 << 24, (need - 1) * (b["base"] if j == jk else 1) + convs[j]["k"])
    if x3:                                  # channels padded to 8; an odd number of 16-byte units per row; two bf16 planes
        def pitch(c):
            c8 = _cp(c, 8)
            return c8 + 8 if (c8 // 8) % 2 == 0 else c8
        floor, unit = 8, 4
    else:                                   # channels padded to 4; an odd number of float4 per row; fp32
        def pitch(c):
            c4 = _cp(c, 4)
            return c4 + 4 if (c4 // 4) % 2 == 0 else c4
        floor, unit = 4, 4
    rows_buf = [need, 0, 0]
    pitch_buf = [pitch(convs[0]["w"].shape[1]), floor, floor]
    for j in range(len(convs) - 1):
        dst = 1 + (j & 1)
        rows_buf[dst] = max(rows_buf[dst], rows[j])
        pitch_buf[dst] = max(pitch_buf[dst], pitch(convs[j]["w"].shape[0]))
    return unit * sum(nb * r * p for r, p in zip(rows_buf, pitch_buf))


def tile_regimes(blocks, B, ld, mode):
    """(out_rows, T, nb, tiles_pos) of every block as the forward launches it (mode 'f32' or 'bf16x3'): T output positions
    of nb reads per workgroup - T up to 64, cut while the tile outgrows the 64 KB LDS budget; several reads only where one
    read's outputs fit one tile."""
    x3 = mode == "bf16x3"
    need = T.windows(blocks, ld)
    out = []
    for i, b in enumerate(blocks):
        out_rows = need[i + 1]
        t = min(out_rows, 64)
        while t > 1 and _lds_bytes(b, t, 1, x3) > LDS_BUDGET:
            t -= 1
        nb = 1
        if t == out_rows:
            nb = max(1, min(B, 64 // t))
            while nb > 1 and _lds_bytes(b, t, nb, x3) > LDS_BUDGET:
                nb -= 1
        out.append((out_rows, t, nb, -(-out_rows // t)))
    return out
