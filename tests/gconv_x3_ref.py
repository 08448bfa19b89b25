"""Reference side of the generic ConvNet family's bf16x3 mode (csrc/gconv_x3.hip): an emulation of its arithmetic in numpy
that knows nothing of the device's tiles or K order, the bars the device is held to, and the arithmetic mutants the bars must
tell from the real thing.

The emulation: activations are fp32 between convs; a conv with c_in > 4 splits its activations and its weights into
hi = bf16(v), lo = bf16(v - hi) and sums hi*hi + lo*hi + hi*lo - in float64 (`E64`) or in float32 (`E32`, numpy's own
summation order) - rounds to fp32, adds the bias and applies the ReLU in fp32; a conv with c_in <= 4 stays on the fp32 kernel
and is taken as exact (float64, rounded to fp32); the head is float64.  The device is a third accumulation order: a 1-ulp
difference in an fp32 activation moves the bf16 rounding of `lo` for about 1 element in 128, so two correct implementations
differ from each other by up to 0.7 of their own gap to float64, and the device is held to float64, not to the emulation.

Bars: X3_BARS[name] = 4 x max(E64, E32), rounded up to one digit (gconv_ref.bar_of), where E64 / E32 are the emulations' gaps
(gconv_ref.gap) to gconv_ref.forward(float64) on the config's own 77-read ragged batch.  Nothing here comes from a device."""
from __future__ import annotations

import numpy as np

from tests import gconv_ref as R
from tests.tcn_ref import bf16

# gaps of the two emulations to float64 on every config's 77 reads (tests/test_gconv_x3_cpu.py recomputes them to two digits)
X3_E64 = {"d1_k5_c20_67": 1.22e-05, "d2_k5373": 6.51e-05, "d3_k3_c5": 1.67e-05, "d1_k1_c17": 2.62e-05, "d2_k9_c33": 3.90e-05,
          "d1_k19_c8": 2.47e-05, "d2_cin65": 9.10e-05, "d2_cin133": 4.75e-05, "d1_wide_337_505": 9.30e-05,
          "d1_k19_c272": 1.14e-05, "d1_six_layers": 6.26e-05}
X3_E32 = {"d1_k5_c20_67": 1.24e-05, "d2_k5373": 4.75e-05, "d3_k3_c5": 1.66e-05, "d1_k1_c17": 2.62e-05, "d2_k9_c33": 3.90e-05,
          "d1_k19_c8": 2.88e-05, "d2_cin65": 8.54e-05, "d2_cin133": 2.96e-05, "d1_wide_337_505": 9.23e-05,
          "d1_k19_c272": 1.14e-05, "d1_six_layers": 6.26e-05}
# The mode was specified with the bars of a draft of this emulation (it rounded at other places, and such a difference moves
# a gap by up to 0.7 of itself, see above).  The rule's bar of this emulation never goes beyond the draft's: where the two
# differ the tighter one holds.
DRAFT_BARS = {"d1_k5_c20_67": 5e-5, "d2_k5373": 4e-4, "d3_k3_c5": 8e-5, "d1_k1_c17": 2e-4, "d2_k9_c33": 2e-4, "d1_k19_c8": 2e-4,
              "d2_cin65": 3e-4, "d2_cin133": 5e-4, "d1_wide_337_505": 4e-4, "d1_k19_c272": 5e-5, "d1_six_layers": 3e-4}
X3_BARS = {name: min(R.bar_of(max(X3_E64[name], X3_E32[name])), DRAFT_BARS[name]) for name in R.CONFIGS}

# the three nets of tests/golden/convnet_variants.npz behind Model: the emulations' largest |probability - the reference's own|
# over the fixture's five reads, and the bar by the same rule
VARIANT_GAPS = {"depth2_k5373": {"E64": 1.63e-06, "E32": 1.58e-06}, "depth1_k7": {"E64": 9.36e-06, "E32": 9.81e-06},
                "depth3_k3": {"E64": 1.02e-06, "E32": 9.76e-07}}
VARIANT_BARS = {name: R.bar_of(max(v.values())) for name, v in VARIANT_GAPS.items()}

# arithmetic defects of the split: the bar is worth something only if each of them misses it by a wide margin
ARITH_MUTANTS = {
    "plain_bf16": "hi*hi alone: no lo halves",
    "no_lo_hi": "the lo*hi term (the activation's low half) dropped",
    "no_hi_lo": "the hi*lo term (the weight's low half) dropped",
}
MUTANT_MARGIN = 10.0           # every arithmetic mutant lies at least this many bars from float64

SIG_PAD = 64                   # the batch of tests/test_gconv.py: rows 64 samples longer than the longest read, NaN behind


def split(v, dtype):
    v = np.asarray(v, dtype=np.float32)
    hi = bf16(v)
    return hi.astype(dtype), bf16(v - hi).astype(dtype)


def x3_matmul(a, w, acc=np.float64, arith=None):
    """a [T, K] fp32 @ w [K, N] fp32 in split precision, the three partial products summed in `acc`, rounded to fp32"""
    ah, al = split(a, acc)
    wh, wl = split(w, acc)
    y = ah @ wh
    if arith != "plain_bf16":
        if arith != "no_lo_hi":
            y = y + al @ wh
        if arith != "no_hi_lo":
            y = y + ah @ wl
    return y.astype(np.float32)


def _conv(x, w, b, acc, arith, left=None, right=None):
    """x [T, ci] fp32 -> conv + bias, fp32 [T, co]; 'same' zero padding (left / right: rows that stand in for it, mutants)"""
    T, ci = x.shape
    co, _, k = w.shape
    pad = k // 2
    lp = np.zeros((pad, ci), np.float32) if left is None else np.asarray(left, np.float32)
    rp = np.zeros((pad, ci), np.float32) if right is None else np.asarray(right, np.float32)
    xp = np.concatenate([lp, x, rp], axis=0)
    cols = np.concatenate([xp[t: t + T] for t in range(k)], axis=1)                # [T, k * ci], tap-major
    wm = np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(k * ci, co)
    if ci <= 4:                # stays on the fp32 kernel in both modes: exact
        y = (cols.astype(np.float64) @ wm.astype(np.float64)).astype(np.float32)
    else:
        y = x3_matmul(cols, wm, acc, arith)
    return y + b.astype(np.float32)


def forward_one(prog, sig, acc=np.float64, arith=None, mutant=None, row=None, prev=None):
    """logits [2] (float64) of one read in the emulated bf16x3 mode.  arith: a key of ARITH_MUTANTS; mutant: a key of
    gconv_ref.DEVICE_MUTANTS, with the meaning it has in gconv_ref.forward_one."""
    depth = prog["depth"]
    x = np.asarray(sig, np.float32)[:, None]
    for i, cv in enumerate(prog["convs"]):
        w, b = cv["w"], cv["b"]
        k, d = w.shape[2], i % depth
        pad = k // 2
        left = right = None
        if i == 0 and pad:
            if mutant == "right_pad_reads_pitch":
                right = np.asarray(row, np.float32)[len(sig): len(sig) + pad, None]
            if mutant == "left_from_prev_read":
                left = np.asarray(prev, np.float32)[-pad:, None]
        if mutant == "drop_last_chunk":
            p = R.plan_conv(w.shape[1], w.shape[0], k)
            if p["n_chunks"] > 1 and w.shape[1] % p["kc"]:
                w = w.copy()
                w[:, w.shape[1] // p["kc"] * p["kc"]:, :] = 0
        y = _conv(x, w, np.zeros_like(b) if mutant == "relu_before_bias" else b, acc, arith, left, right)
        if mutant == "pad_channel_weighted" and w.shape[1] % 4 and w.shape[1] > 1:
            y = y + w[:, -1, :].sum(axis=1)
        y = np.maximum(y, np.float32(0))
        if mutant == "relu_before_bias":
            y = y + b.astype(np.float32)
        pool = d == depth - 1
        if mutant == "pool_after_nonlast" and depth > 1:
            pool = d == 0
        if pool:
            T = y.shape[0]
            if mutant == "pool_pairs_shifted":
                y = np.concatenate([y[:1], y])[: T // 2 * 2]
            if mutant == "pool_trailing_odd" and T % 2:
                y = np.concatenate([y, y[-1:]])
            T = y.shape[0]
            y = y[: T // 2 * 2].reshape(T // 2, 2, -1).max(axis=1)
        x = y.astype(np.float32)
    m = x.astype(np.float64).mean(axis=0)
    return prog["fc_w"].astype(np.float64) @ m + prog["fc_b"].astype(np.float64)


def forward(prog, rows, lens, acc=np.float64, arith=None, mutant=None):
    """logits [B, 2] of a ragged batch: read b = rows[b, :lens[b]]"""
    out = np.zeros((len(lens), 2), np.float64)
    for b, L in enumerate(lens):
        prev = rows[b - 1, : lens[b - 1]] if b else np.zeros(64, rows.dtype) + 1.5
        out[b] = forward_one(prog, rows[b, :L], acc, arith, mutant, row=rows[b], prev=prev)
    return out


def edge_batch(name):
    """the config's own 77-read ragged batch, as tests/test_gconv.py draws it: (lens, rows with NaN behind every read)"""
    cfg = R.CONFIGS[name]
    lens = R.edge_lengths(cfg, R.SEED[name])
    rng = np.random.default_rng(R.SEED[name] + 1)
    rows = np.full((len(lens), int(lens.max()) + SIG_PAD), np.nan, np.float32)
    for b, L in enumerate(lens):
        rows[b, :L] = rng.standard_normal(L).astype(np.float32)
    return lens, rows
