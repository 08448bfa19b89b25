"""Reference side of the generic ConvNet family (csrc/gconv.hip): the edge table, a float64 / float32 ragged forward in numpy
that knows nothing of the device's K order, a mirror of the device planner's index arithmetic (shape_tags), and defect mutants
of the forward that the tests must be able to tell from the real thing."""
from __future__ import annotations

import types

import numpy as np

# name -> config.  max_len caps the lengths a config is run at (the wide ones run short reads: their float64 reference is
# the cost); every config's reads share one batch of N_READS
N_READS = 77
CONFIGS = {
    "d1_k5_c20_67": dict(n_layers=4, depth=1, channels=[20, 30, 45, 67], kernels=[5, 5, 5, 5], max_len=16000),
    "d2_k5373": dict(n_layers=4, depth=2, channels=[6, 9, 14, 20], kernels=[5, 3, 7, 3], max_len=16000),
    "d3_k3_c5": dict(n_layers=3, depth=3, channels=[5, 10, 15], kernels=[3, 3, 3], max_len=16000),
    "d1_k1_c17": dict(n_layers=2, depth=1, channels=[17, 17], kernels=[1, 1], max_len=16000),
    "d2_k9_c33": dict(n_layers=2, depth=2, channels=[33, 33], kernels=[9, 9], max_len=16000),
    "d1_k19_c8": dict(n_layers=5, depth=1, channels=[8, 12, 8, 12, 8], kernels=[19, 19, 19, 19, 19], max_len=16000),
    "d2_cin65": dict(n_layers=3, depth=2, channels=[65, 65, 20], kernels=[3, 3, 3], max_len=8615),
    "d2_cin133": dict(n_layers=3, depth=2, channels=[16, 133, 129], kernels=[3, 3, 3], max_len=8615),
    "d1_wide_337_505": dict(n_layers=2, depth=1, channels=[337, 505], kernels=[5, 5], max_len=4097),
    "d1_k19_c272": dict(n_layers=2, depth=1, channels=[8, 272], kernels=[3, 19], max_len=4097),
    "d1_six_layers": dict(n_layers=6, depth=1, channels=[5, 6, 7, 8, 9, 10], kernels=[3, 3, 3, 3, 3, 3], max_len=16000),
}
SEED = {name: 8100 + i for i, name in enumerate(CONFIGS)}
# the configs tests/golden/gconv_edges.npz pins against the reference's own ConvNet (tools/make_golden.py: f2e)
GOLDEN_EDGES = ("d2_k5373", "d3_k3_c5", "d1_k1_c17", "d2_k9_c33", "d1_k19_c8", "d2_cin65")
GOLDEN_LENGTHS = ("min", "min+1", 1000, 2049)

ALL_TAGS = sorted(["shape0", "shape1", "shape2", "shape3", "shape4", "vec1", "vec4", "chunks1", "chunks2", "chunks3+",
                   "ragged_last_chunk", "col_blocks2+", "partial_col_block", "idle_wave", "lds_over_64k", "pool", "no_pool",
                   "halo0", "halo1", "halo2", "halo3", "halo4", "halo9"])

# Bars per config on max |device - float64| / max(1, |logit|), by the CNN-RNN's rule: 4 x the device's largest gap on the first
# MI355X run (GCONV_GAP, the line tests/test_gconv.py prints before it asserts; profiles/gconv_gpu_tests.txt), rounded up to
# one digit, not below BAR_FLOOR.  The rule holds only while the device's gap is of the order of numpy-fp32's own gap to
# float64 on the same 77 reads, which tests/test_gconv.py computes and asserts beside the bar.
BAR_FLOOR = 2e-7
GCONV_GAP = {"d1_k5_c20_67": 4.85e-07, "d2_k5373": 4.29e-06, "d3_k3_c5": 6.48e-07, "d1_k1_c17": 9.92e-07, "d2_k9_c33": 7.94e-07,
             "d1_k19_c8": 1.87e-06, "d2_cin65": 1.90e-06, "d2_cin133": 3.33e-06, "d1_wide_337_505": 6.28e-06,
             "d1_k19_c272": 4.91e-07, "d1_six_layers": 1.90e-06}
BARS = {"d1_k5_c20_67": 2e-06, "d2_k5373": 2e-05, "d3_k3_c5": 3e-06, "d1_k1_c17": 4e-06, "d2_k9_c33": 4e-06,
        "d1_k19_c8": 8e-06, "d2_cin65": 8e-06, "d2_cin133": 2e-05, "d1_wide_337_505": 3e-05, "d1_k19_c272": 2e-06,
        "d1_six_layers": 8e-06}


def cnn_config(cfg):
    return types.SimpleNamespace(n_layers=cfg["n_layers"], depth=cfg["depth"], channels=list(cfg["channels"]),
                                 kernels=list(cfg["kernels"]), n_classes=2, classifier="gap_fc")


def make_state_dict(cfg, seed):
    """He-scaled random weights under the reference's state-dict keys (riser/nets/cnn.py:52-65: layers.{i}.{2 d})"""
    rng = np.random.default_rng(seed)
    sd, c_in = {}, 1
    for i, co in enumerate(cfg["channels"]):
        k = cfg["kernels"][i]
        for d in range(cfg["depth"]):
            sd[f"layers.{i}.{2 * d}.weight"] = (rng.standard_normal((co, c_in, k)) * np.sqrt(2.0 / (k * c_in))).astype(np.float32)
            sd[f"layers.{i}.{2 * d}.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)
            c_in = co
    sd["classifier.2.weight"] = rng.standard_normal((2, c_in)).astype(np.float32)
    sd["classifier.2.bias"] = rng.standard_normal(2).astype(np.float32)
    return sd


# ---------------------------------------------------------------------------------------------- the device planner, mirrored
SHAPES = ((4, 1, 2), (4, 2, 2), (4, 4, 2), (1, 4, 1), (1, 4, 2))       # (row tiles, wave columns, column tiles per wave)
LDS_PREFER, LDS_MAX, DEEP_FROM = 52 * 1024, 160 * 1024, 256


def _rows(s):
    return 16 * SHAPES[s][0]


def _cols(s):
    return 16 * SHAPES[s][1] * SHAPES[s][2]


def _slab_pitch(kc):
    return kc + 4 if (kc // 4) % 2 == 0 else kc


def _lds(s, k, kc):
    return ((_rows(s) + k - 1) * _slab_pitch(kc) + _cols(s) * k * kc) * 4


def plan_conv(c_in, c_out, k):
    """csrc/gconv/plan.hpp: plan_conv, or None where it refuses"""
    vec = 1 if c_in <= 4 else 4
    kg, npad = 4 * vec, (c_out + 15) // 16 * 16
    cand = (4, 3) if npad > DEEP_FROM else (2, 1, 0)
    pick = None
    for i, s in enumerate(cand):
        if i + 1 < len(cand) and _cols(cand[i + 1]) >= npad:
            continue
        if _lds(s, k, kg) <= LDS_PREFER:
            pick = s
            break
    if pick is None:
        pick = cand[-1]
        if _lds(pick, k, kg) > LDS_MAX:
            return None
    cpad, kc = -(-c_in // kg) * kg, kg
    if vec == 4:
        for c in (64, 32):
            if c <= cpad and _lds(pick, k, c) <= LDS_PREFER:
                kc = c
                break
    return dict(shape=pick, rows=_rows(pick), cols=_cols(pick), vec=vec, kc=kc, n_chunks=-(-c_in // kc),
                lds_bytes=_lds(pick, k, kc))


def convs_of(cfg):
    """(c_in, c_out, k, pool) of every conv in launch order"""
    out, c_in = [], 1
    for i in range(cfg["n_layers"]):
        for d in range(cfg["depth"]):
            out.append((c_in, cfg["channels"][i], cfg["kernels"][i], d == cfg["depth"] - 1))
            c_in = cfg["channels"][i]
    return out


def shape_tags(cfg):
    tags = set()
    for c_in, c_out, k, pool in convs_of(cfg):
        p = plan_conv(c_in, c_out, k)
        tags.add(f"shape{p['shape']}")
        tags.add(f"vec{p['vec']}")
        tags.add({1: "chunks1", 2: "chunks2"}.get(p["n_chunks"], "chunks3+"))
        if p["n_chunks"] > 1 and c_in % p["kc"]:
            tags.add("ragged_last_chunk")
        ncb = -(-c_out // p["cols"])
        if ncb > 1:
            tags.add("col_blocks2+")
            if c_out % p["cols"]:
                tags.add("partial_col_block")
        wave_cols = 16 * SHAPES[p["shape"]][2]
        if (ncb - 1) * p["cols"] + (SHAPES[p["shape"]][1] - 1) * wave_cols >= c_out:
            tags.add("idle_wave")
        if p["lds_bytes"] > 64 * 1024:
            tags.add("lds_over_64k")
        tags.add("pool" if pool else "no_pool")
        tags.add(f"halo{k // 2}")
    return tags


def edge_lengths(cfg, seed):
    """N_READS lengths: the minimum, one more, an odd row count at every pool level, each tile-row boundary +-1 at layers 0
    and 1, 4096, 4097, 8615 and 16000 where max_len allows, the rest drawn at random"""
    n, cap = cfg["n_layers"], cfg["max_len"]
    lo = 1 << n
    convs = convs_of(cfg)
    r0 = plan_conv(*convs[0][:3])["rows"]
    r1 = plan_conv(*convs[cfg["depth"]][:3])["rows"]
    lens = [lo, lo + 1] + [(4 << n) + (1 << l) for l in range(n)]
    for r in (r0, 2 * r0, 2 * r1, 4 * r1):
        lens += [r - 1, r, r + 1, r + 2, r + 3]
    lens += [4096, 4097, 8615, 16000]
    lens = [L for L in lens if lo <= L <= cap]
    rng = np.random.default_rng(seed + 77)
    while len(lens) < N_READS:
        lens.append(int(rng.integers(lo, min(cap, 1500) + 1)))
    return np.array(lens[:N_READS], dtype=np.int32)


# ---------------------------------------------------------------------------------------------- the forward, in numpy
def _conv_same(x, w, b, dtype, left=None, right=None):
    """x [T, ci], w [co, ci, k] -> [T, co]: 'same' zero padding (left / right: rows that stand in for the padding, mutants)"""
    T, ci = x.shape
    co, _, k = w.shape
    pad = k // 2
    lp = np.zeros((pad, ci), dtype) if left is None else left
    rp = np.zeros((pad, ci), dtype) if right is None else right
    xp = np.concatenate([lp, x, rp], axis=0)
    cols = np.concatenate([xp[t: t + T] for t in range(k)], axis=1)                # [T, k * ci], tap-major
    wm = np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(k * ci, co).astype(dtype)
    return cols @ wm + b.astype(dtype)


def forward_one(prog, sig, dtype=np.float64, mutant=None, row=None, prev=None):
    """logits [2] of one read `sig` [L] (float64: the reference arithmetic).  mutant: a key of DEVICE_MUTANTS; row: the
    read's whole row of the batch (what lies behind the read), prev: the read before it in the batch."""
    depth = prog["depth"]
    x = np.asarray(sig, dtype)[:, None]
    for i, cv in enumerate(prog["convs"]):
        w, b = cv["w"], cv["b"]
        k, d = w.shape[2], i % depth
        pad = k // 2
        left = right = None
        if i == 0 and pad:
            if mutant == "right_pad_reads_pitch":
                right = np.asarray(row, dtype)[len(sig): len(sig) + pad, None]
            if mutant == "left_from_prev_read":
                left = np.asarray(prev, dtype)[-pad:, None]
        if mutant == "drop_last_chunk":
            p = plan_conv(w.shape[1], w.shape[0], k)
            if p["n_chunks"] > 1 and w.shape[1] % p["kc"]:
                w = w.copy()
                w[:, w.shape[1] // p["kc"] * p["kc"]:, :] = 0
        y = _conv_same(x, w, np.zeros_like(b) if mutant == "relu_before_bias" else b, dtype, left, right)
        if mutant == "pad_channel_weighted" and w.shape[1] % 4 and w.shape[1] > 1:
            y = y + w[:, -1, :].astype(dtype).sum(axis=1)              # a pad channel that reads 1 under the last channel's taps
        y = np.maximum(y, 0)
        if mutant == "relu_before_bias":
            y = y + b.astype(dtype)
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
        x = y
    m = x.mean(axis=0)
    return prog["fc_w"].astype(dtype) @ m + prog["fc_b"].astype(dtype)


def forward(prog, rows, lens, dtype=np.float64, mutant=None):
    """logits [B, 2] of a ragged batch: read b = rows[b, :lens[b]]"""
    out = np.zeros((len(lens), 2), dtype)
    for b, L in enumerate(lens):
        prev = rows[b - 1, : lens[b - 1]] if b else np.zeros(64, rows.dtype) + 1.5
        out[b] = forward_one(prog, rows[b, :L], dtype, mutant, row=rows[b], prev=prev)
    return out


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def gap(got, want):
    """the measure the bars are set in: max |got - want| / max(1, |want|)"""
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))))


def mutant_applies(name, cfg):
    if name == "drop_last_chunk":
        return "ragged_last_chunk" in shape_tags(cfg)
    if name == "pad_channel_weighted":
        return any(c_in % 4 and c_in > 1 for c_in, _, _, _ in convs_of(cfg))
    if name == "pool_after_nonlast":
        return cfg["depth"] > 1
    if name in ("right_pad_reads_pitch", "left_from_prev_read"):
        return cfg["kernels"][0] > 1
    return True


DEVICE_MUTANTS = {
    "right_pad_reads_pitch": "right padding reads the next rows of the pitch instead of zero",
    "left_from_prev_read": "left neighbour taken from the previous read",
    "pool_pairs_shifted": "pool pairs shifted by one",
    "pool_trailing_odd": "a trailing odd row pooled",
    "drop_last_chunk": "last partial chunk dropped",
    "pad_channel_weighted": "pad channel weighted",
    "relu_before_bias": "ReLU before the bias",
    "pool_after_nonlast": "pool fused after a non-last conv of a layer",
}


def bar_of(gap):
    """the rule: 4 x the measured gap, rounded up to one digit, not below BAR_FLOOR"""
    import math
    v = max(BAR_FLOOR, 4.0 * gap)
    e = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / e - 1e-9) * e
