"""Helpers of tests/test_gpu_f32_shapes.py and tests/test_gpu_f32_thin.py: the fp32 conv kernels' tile-shape tables and the
small-batch kernel's instantiations read out of the sources, a mirror of their LDS footprints, the sweep's nets and read
lengths (normalised rows and raw int16), and a float64 reference of ONE ConvNet layer (direct and as Winograd F(4,3)) with
deliberate defects (MUTANTS) that the sweep's tolerances must be able to see.  numpy only."""
import os
import re

import numpy as np

from oracle import riser_oracle as ro
from riser_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riser_amd", "csrc")

# family -> (source with the kShapes[] table, gemm_row_div of rs_layer_info, the hook that forces a shape, chunk sizes)
# chunk 0 = the direct kernel's run-time-chunk instantiation (layers below 16 input channels: chunks of 4, 8 or 12)
FAMILIES = {
    "direct": dict(src="conv_f32.hip", row_div=1, hook="RS_FORCE_SHAPE_F32", kcs=(0, 16, 20, 24)),
    "wino": dict(src="conv_wino.hip", row_div=2, hook="RS_FORCE_SHAPE_WINO", kcs=(16, 20, 24)),
    "wino4": dict(src="conv_wino4.hip", row_div=4, hook="RS_FORCE_SHAPE_WINO4", kcs=(16, 20)),
}
LDS_LIMIT = 160 * 1024
RT_KC_MAX = 12                        # the largest run-time chunk (plan_static_f32: below 16 padded input channels)


def parse_shapes(family):
    """[(wm, wn, mt, nt, kind)] of the family's kShapes[] initialiser, kind "" (RS_SHAPE), "D" (RS_SHAPE_D: also in the
    one-item-ahead form) or "4" (RS_SHAPE_4: four waves)"""
    with open(os.path.join(CSRC, FAMILIES[family]["src"])) as f:
        text = f.read()
    m = re.search(r"kShapes\[\]\s*=\s*\{(.*?)\n\};", text, re.S)
    assert m, family
    body = re.sub(r"//[^\n]*", "", m.group(1))
    out = [(int(a), int(b), int(c), int(d), k)
           for k, a, b, c, d in re.findall(r"RS_SHAPE(?:_(D|4))?\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", body)]
    assert len(out) == len(re.findall(r"RS_SHAPE", body)), family     # every entry of the table was understood
    return out


def tile(family, shape):
    """(bm, bn) as rs_layer_info reports them: bm in conv rows (x1 direct, x2 F(2,3), x4 F(4,3))"""
    wm, wn, mt, nt = shape[:4]
    return FAMILIES[family]["row_div"] * wm * 16 * mt, wn * 16 * nt


def lds_bytes_of_tile(family, bm, bn, kc):
    """the three lds_bytes() of the sources, from the reported tile"""
    u = bm // FAMILIES[family]["row_div"]            # row units of the tile: conv rows, pooled rows, groups of four
    if family == "direct":
        floats = (u + 2) + 3 * bn
    elif family == "wino":
        floats = 2 * (u + 1) + 4 * bn
    else:
        floats = 4 * (u + 1) + 6 * bn
    return 2 * floats * (kc + 2) * 4


def lds_bytes(family, shape, kc):
    return lds_bytes_of_tile(family, *tile(family, shape), kc)


def fits(family, shape, kc):
    """whether the launchers honour a forced shape at this chunk (one that does not fit is silently ignored)"""
    return lds_bytes(family, shape, kc) <= LDS_LIMIT


def instantiations(family):
    """every (family, (wm, wn, mt, nt), chunk, deep?) a launch can reach: the coverage target of the sweep"""
    out = set()
    for s in parse_shapes(family):
        for kc in FAMILIES[family]["kcs"]:
            if fits(family, s, kc or RT_KC_MAX):
                out.add((family, s[:4], kc, False))
                if s[4] == "D":
                    out.add((family, s[:4], kc, True))
    return out


# ------------------------------------------------------------------------------------------------ nets
NARROW = (7, 10, 27, 50, 21, 90)      # 7 / 10 input channels: run-time chunks of 8 / 12; 27: a ragged chunk of 16; c_out < 16
SEED = 2
_W4_ALL = lambda n: ",".join(str(i) for i in range(1, n))
_KC_ALL = lambda n, kc: ";".join(f"{i}:{kc}" for i in range(1, n))
# name -> (channels, dtype, env when the model is created, whether every table entry is forced onto it)
VARIANTS = {
    "ship_f32": (synth.CHANNELS, "f32", {}, True),
    "ship_f32w": (synth.CHANNELS, "f32w", {}, False),                     # the model of record: F(2,3) and F(4,3) mixed
    "ship_w2": (synth.CHANNELS, "f32w", {"RS_WINO4": "none"}, True),
    "ship_w4_kc16": (synth.CHANNELS, "f32w", {"RS_WINO4": _W4_ALL(12), "RS_PLAN_KC": _KC_ALL(12, 16)}, True),
    "ship_w4_kc20": (synth.CHANNELS, "f32w", {"RS_WINO4": _W4_ALL(12), "RS_PLAN_KC": _KC_ALL(12, 20)}, True),
    "narrow_f32": (NARROW, "f32", {}, True),
    "narrow_w2": (NARROW, "f32w", {"RS_WINO4": "none"}, True),
    "narrow_w4_kc16": (NARROW, "f32w", {"RS_WINO4": _W4_ALL(6), "RS_PLAN_KC": _KC_ALL(6, 16)}, True),
    "narrow_w4_kc20": (NARROW, "f32w", {"RS_WINO4": _W4_ALL(6), "RS_PLAN_KC": _KC_ALL(6, 20)}, True),
}
# The nets of tests/test_gpu_f32_thin.py (the fp32 streaming kernel K3s, conv_stream_f32.hip, and the small-batch kernel K3m,
# conv_small_f32.hip): the Winograd variants above, and 6-layer nets with NARROW's tail whose first two layers sit on the
# streaming kernel's edges.  conv_stream_f32_ok wants layer 1 as F(2,3) with cp_in == 20 (row_pitch: c0 rounded up to 4, so
# c0 = 17 .. 20), kc == 20 and nch == 1 (plan_static_wino at 20 padded channels: one chunk of 20 costs 21.5, two of 16 cost 35,
# one of 24 costs 25.5) and c1 <= 32; the F(4,3) forms leave layer 1 to F(2,3) and put layers 2-5 behind the streaming kernel.
_TAIL = NARROW[2:]
_W4_TAIL = ",".join(str(i) for i in range(2, 6))
THIN_VARIANTS = {v: VARIANTS[v] for v in ("ship_f32w", "ship_w2", "ship_w4_kc16", "ship_w4_kc20", "narrow_w2", "narrow_w4_kc16",
                                          "narrow_w4_kc20")}
THIN_VARIANTS.update({
    "stream_18_13": ((18, 13) + _TAIL, "f32w", {}, False),        # layer-0 lanes above the real channels; NT = 1, c_out < 16
    "stream_19_29": ((19, 29) + _TAIL, "f32w", {}, False),        # NT = 2 with a partial second sub-tile
    "stream_17_32": ((17, 32) + _TAIL, "f32w", {}, False),        # NT = 2, both sub-tiles whole
    "stream_18_13_w4_kc20": ((18, 13) + _TAIL, "f32w", {"RS_WINO4": _W4_TAIL, "RS_PLAN_KC": _KC_ALL(6, 20)}, False),
    "stream_19_29_w4_kc16": ((19, 29) + _TAIL, "f32w", {"RS_WINO4": _W4_TAIL, "RS_PLAN_KC": _KC_ALL(6, 16)}, False),
})
# the variants whose layer 1 the streaming kernel takes on the raw entry point (an F(4,3) layer 1 is not its packing; the
# narrow net's layer 1 has 8 padded input channels)
THIN_STREAMING = ("ship_f32w", "ship_w2") + tuple(v for v in THIN_VARIANTS if v.startswith("stream_"))


def parse_small_instantiations():
    """{(nc, kc, shared, nw)} of the conv_small_f32_kernel<...> instantiations that pick() of conv_small_f32.hip can return
    (template arguments left out take the kernel template's defaults)"""
    with open(os.path.join(CSRC, "conv_small_f32.hip")) as f:
        text = f.read()
    d = re.search(r"template\s*<int NC, int KC, bool SH = (true|false), int NW = (\d+)>\s*__global__", text)
    m = re.search(r"KernelFn pick\([^)]*\)\s*\{(.*?)\n\}", text, re.S)
    assert d and m
    body = re.sub(r"//[^\n]*", "", m.group(1))
    found = re.findall(r"conv_small_f32_kernel<\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(true|false)\s*(?:,\s*(\d+)\s*)?)?>", body)
    assert len(found) == len(re.findall(r"conv_small_f32_kernel\s*<", body))       # every instantiation was understood
    out = [(int(nc), int(kc), (sh or d.group(1)) == "true", int(nw or d.group(2))) for nc, kc, sh, nw in found]
    assert len(set(out)) == len(out)
    return set(out)


_SD = {}


def state_dict(channels):
    channels = tuple(channels)
    if channels not in _SD:
        _SD[channels] = synth.make_state_dict(SEED, channels)
    return _SD[channels]


def config(channels):
    return synth.Config(synth.CnnConfig(channels=list(channels), kernels=[3] * len(channels)))


# ------------------------------------------------------------------------------------------------ reads
N_READS = 77
MAX_LEN = 16000
LD = MAX_LEN + 123                    # row pitch of the ragged batch: NaNs fill every row behind its read


def sweep_lengths(n_layers):
    """77 read lengths by rule: the net's minimum and +1; per layer i four lengths whose row count entering the layer is
    0, 1, 2, 3 (mod 4); one below, at and one above a multiple of the fine (1024), coarse (4096) and F(4,3)-doubled (8192)
    block; 16000; seeded random lengths for the rest"""
    lo = 1 << n_layers
    fixed = [lo, lo + 1, MAX_LEN]
    for i in range(n_layers):
        for r in range(4):
            q = (lo >> i) + 1
            while q % 4 != r:
                q += 1
            n = (q << i) + ((1 << i) - 1) * 5 // 8            # low bits: odd row counts in the layers in front of i
            assert lo <= n <= MAX_LEN and (n >> i) % 4 == r
            fixed.append(n)
    for blk, k in ((1024, 5), (4096, 2), (8192, 1)):
        fixed += [k * blk - 1, k * blk, k * blk + 1]
    fixed = sorted(set(fixed))
    assert len(fixed) <= N_READS - 8
    rng = np.random.default_rng(20260105 + n_layers)
    return fixed + [int(v) for v in rng.integers(lo, MAX_LEN + 1, N_READS - len(fixed))]


_SIGNALS = []


def reads(n_layers):
    """the sweep's reads: read k is the last n_k samples of a normalised synthetic read of 16000 samples (fp32)"""
    if not _SIGNALS:
        for k in range(N_READS):
            s = synth.make_signals(20260104, 1, MAX_LEN, first_read=9100 + k)[0]
            _SIGNALS.append(ro.mad_normalise(s).astype(np.float32))
    return [_SIGNALS[k][MAX_LEN - n:] for k, n in enumerate(sweep_lengths(n_layers))]


_RAW = []
_RAW_NORM = {}


def raw_reads(n_layers):
    """the same 77 reads as raw int16 (the streaming kernel runs on the raw entry point only): read k is the last n_k samples of a
    synthetic read of 16000 samples.  Packed (preprocess.pack_reads) they lie back to back: the sample in front of a read is
    the last one of the read before it"""
    if not _RAW:
        for k in range(N_READS):
            _RAW.append(synth.make_signals(20260104, 1, MAX_LEN, first_read=9100 + k)[0])
    return [_RAW[k][MAX_LEN - n:] for k, n in enumerate(sweep_lengths(n_layers))]


def raw_normalised(n_layers):
    """what layer 0 reads of raw_reads: each read normalised on its own (the oracle's float64 rule), as fp32"""
    if n_layers not in _RAW_NORM:
        _RAW_NORM[n_layers] = [ro.mad_normalise(s).astype(np.float32) for s in raw_reads(n_layers)]
    return _RAW_NORM[n_layers]


# ------------------------------------------------------------------------------------------------ one layer in float64
_BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]], dtype=np.float64)
_G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
               [0, 0, 1]], dtype=np.float64)
_AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)

MUTANTS = ("drop_last_channel", "weigh_pad_channels", "wino4_tap_swap", "last_pair_not_pooled", "left_neighbour_of_previous_read",
           "drop_a_bias_of_the_last_tile")


def _conv_f43(xp, w):
    """the pre-activation conv rows as Winograd F(4,3): xp [C, L + 2] (zero column either side), w [N, C, 3] -> [N, L]"""
    C, L = xp.shape[0], xp.shape[1] - 2
    G4 = (L + 3) // 4
    d = np.zeros((C, 4 * G4 + 2))
    d[:, :L + 2] = xp
    idx = 4 * np.arange(G4)[:, None] + np.arange(6)[None, :]
    V = np.einsum("jk,cgk->jcg", _BT, d[:, idx])                 # [6, C, G]
    U = np.einsum("jk,nck->jnc", _G, w)                          # [6, N, C]
    return U, V, G4, L


def layer_f64(x, w, b, mutant=None, kc=16, prev_last=None, wino4=False):
    """Conv1d(k = 3, zero 'same' padding, bias) -> ReLU -> MaxPool(2, 2) of ONE read in float64: x [C_in, L] -> [C_out, L // 2].
    wino4: the conv evaluated as F(4,3) (the same numbers to round-off).  mutant: one deliberate defect;
    kc = the layer's channel chunk (what "padding channels" are), prev_last [C_in] = the last row of the read in front."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).copy()
    b = np.asarray(b, dtype=np.float64).copy()
    N, C, L = w.shape[0], x.shape[0], x.shape[1]
    xp = np.zeros((C, L + 2))
    xp[:, 1:L + 1] = x
    if mutant == "drop_last_channel":                           # the last real channel of the (ragged) last chunk
        w[:, C - 1, :] = 0
    elif mutant == "left_neighbour_of_previous_read":
        xp[:, 0] = prev_last
    if wino4 or mutant == "wino4_tap_swap":
        U, V, G4, L = _conv_f43(xp, w)
        if mutant == "wino4_tap_swap":                          # taps 3 and 4 of the last output channel change places
            U[[3, 4], N - 1] = U[[4, 3], N - 1]
        M = np.einsum("jnc,jcg->jng", U, V)
        y = np.einsum("ij,jng->ngi", _AT, M).reshape(N, 4 * G4)[:, :L]
    else:
        y = w[:, :, 0] @ xp[:, 0:L] + w[:, :, 1] @ xp[:, 1:L + 1] + w[:, :, 2] @ xp[:, 2:L + 2]
    if mutant == "weigh_pad_channels":                          # the zero-padded tail of the last chunk is not zero: its
        npad = -C % kc                                          # slots alias the first channels, counted a second time
        assert npad > 0
        j = min(npad, C)
        y = y + w[:, :j, 0] @ xp[:j, 0:L] + w[:, :j, 1] @ xp[:j, 1:L + 1] + w[:, :j, 2] @ xp[:j, 2:L + 2]
    if mutant == "drop_a_bias_of_the_last_tile":                # of the last 16-channel tile, the entry that weighs most
        t0 = 16 * ((N - 1) // 16)                               # among the channels that are not dead on this read
        live = ((y[t0:] + b[t0:, None]) > 0).any(axis=1)
        b[t0 + int(np.argmax(np.abs(b[t0:]) * live))] = 0
    y = np.maximum(y + b[:, None], 0)
    Lo = L // 2
    out = np.maximum(y[:, 0:2 * Lo:2], y[:, 1:2 * Lo:2])
    if mutant == "last_pair_not_pooled" and Lo:
        out[:, Lo - 1] = y[:, 2 * Lo - 2]
    return out


def layer_f64_reads(xs, w, b):
    """layer_f64 (no mutant) of several reads at once: xs [k] = [C_in, L_k] -> [k] = [C_out, L_k // 2].  The reads lie side by
    side with their zero columns between them, so every tap is ONE product and the weights are converted and read once
    (per read, the late layers of the shipped net spend their time there).  Equal to layer_f64 up to float64 round-off."""
    w = np.asarray(w, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    Ls = [int(x.shape[1]) for x in xs]
    starts = np.concatenate([[0], np.cumsum([L + 2 for L in Ls])]).astype(np.int64)
    xp = np.zeros((w.shape[1], int(starts[-1])))
    for s, x in zip(starts, xs):
        xp[:, s + 1:s + 1 + x.shape[1]] = x
    T = xp.shape[1] - 2
    y = w[:, :, 0] @ xp[:, 0:T] + w[:, :, 1] @ xp[:, 1:T + 1] + w[:, :, 2] @ xp[:, 2:T + 2]
    y = np.maximum(y + b[:, None], 0)
    out = []
    for s, L in zip(starts, Ls):                                    # column s + p of y: position p of the read
        Lo = L // 2
        out.append(np.maximum(y[:, s:s + 2 * Lo:2], y[:, s + 1:s + 2 * Lo:2]))
    return out


def forward_f64_reads(sd, xs):
    """float64 logits [k, 2] of the reads xs [k] = [L_k] through the whole net (the `gap_fc` head: mean over the positions,
    then the Linear layer), layer by layer with layer_f64_reads"""
    n_layers = sum(1 for k in sd if k.startswith("layers.") and k.endswith(".0.weight"))
    hs = [np.asarray(x, dtype=np.float64)[None, :] for x in xs]
    for i in range(n_layers):
        hs = layer_f64_reads(hs, sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"])
    feat = np.stack([h.mean(axis=1) for h in hs])
    return feat @ np.asarray(sd["classifier.2.weight"], dtype=np.float64).T + np.asarray(sd["classifier.2.bias"], dtype=np.float64)


def layer_inputs(sd, x, upto):
    """float64 inputs of layers 0 .. upto of one read x [L]: [x, layer 0's output, ...]"""
    h = np.asarray(x, dtype=np.float64)[None, :]
    out = [h]
    for i in range(upto):
        h = layer_f64(h, sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"])
        out.append(h)
    return out
