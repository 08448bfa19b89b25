"""Helpers of tests/test_gpu_h16_layers.py: decoders of the three row layouts a 16-bit ConvNet layer writes, the storage
roundings of the modes, a mirror of the plain modes' weight packing, the sweep's nets and reads, and deliberate defects
(MUTANTS) of the float64 layer of tests/convnet_ref.py that the sweep's bars must be able to see.  numpy only."""
import numpy as np

from oracle import riser_oracle as ro
from riser_amd import synth
from tests import convnet_ref as R
from tests.overflow_ref import hi_slots

MODES = ("bf16x3", "f16x3", "f16xf8", "f16", "bf16")
SPLIT_MODES = ("bf16x3", "f16x3", "f16xf8")
PLAIN_MODES = ("f16", "bf16")


def base16(mode):
    """the 16-bit storage type of a mode (convnet_pack.hpp: base16)"""
    return "bf16" if mode in ("bf16", "bf16x3") else "f16"


# ------------------------------------------------------------------------------------------------ storage roundings
def bits_to_f64(u16, mode):
    """values of 16-bit patterns in the mode's storage type"""
    u16 = np.ascontiguousarray(u16, dtype=np.uint16)
    if base16(mode) == "f16":
        return u16.view(np.float16).astype(np.float64)
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def bf16_bits(v):
    """fp32 -> bf16 bit patterns, round to nearest even: u += 0x7fff + ((u >> 16) & 1), u >> 16 (gconv/plan.hpp: bf16_rne)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFFFFFF)
    return (u >> np.uint64(16)).astype(np.uint16)


def f16_bits(v):
    """-> f16 bit patterns, round to nearest even (numpy's conversion; 65520 and beyond become inf)"""
    with np.errstate(over="ignore"):
        return np.asarray(v).astype(np.float16).view(np.uint16)


def round16(v, mode):
    """v rounded to nearest even to the mode's storage type, as float64 (bf16: through fp32, the value the device holds)"""
    v = np.asarray(v, dtype=np.float64)
    return bits_to_f64(f16_bits(v) if base16(mode) == "f16" else bf16_bits(v.astype(np.float32)), mode)


def split16(v, mode):
    """(hi, lo) of split precision: hi = round16(v), lo = round16(v - hi)"""
    v = np.asarray(v, dtype=np.float64)
    hi = round16(v, mode)
    return hi, round16(v - hi, mode)


def ulp16(v, mode):
    """spacing of the mode's storage type at |v| (the distance between the two neighbours that enclose it), subnormals included"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    mant, emin = (10, -14) if base16(mode) == "f16" else (7, -126)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.exp2(e - mant)


# ------------------------------------------------------------------------------------------------ row decoders
def e4m3(b):
    """values of OCP e4m3 bytes (bias 7, subnormals of 2^-9)"""
    b = np.asarray(b).astype(np.int32)
    s = np.where(b & 0x80, -1.0, 1.0)
    e = (b >> 3) & 0xF
    m = b & 7
    return s * np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))


def row_bytes(rows, cp):
    return rows * cp * 2


def f8_scale_offset(rows, cp):
    """byte offset of the E8M0 scale plane behind `rows` F8 rows of cp 16-bit slots: the next multiple of 256"""
    return (row_bytes(rows, cp) + 255) // 256 * 256


def f8_scale_stride(rows):
    return (rows + 3) // 4 * 4


def capture_bytes(rows, cp, rows_format):
    """size of a layer's output buffer (F8 rows: with the scale plane)"""
    if rows_format == 2:
        return f8_scale_offset(rows, cp) + (cp // 128) * f8_scale_stride(rows) * 4
    return row_bytes(rows, cp)


def decode_plain(raw, rows, cp, c_out, mode):
    """format 0, one half per channel -> float64 [rows, c_out]"""
    u = np.asarray(raw, dtype=np.uint8)[:row_bytes(rows, cp)].view(np.uint16).reshape(rows, cp)
    return bits_to_f64(u[:, hi_slots(0, c_out)], mode)


def decode_split(raw, rows, cp, c_out, mode):
    """format 1, 32-channel panels [hi x 32 | lo x 32] -> (hi, lo) float64 [rows, c_out]; the value is hi + lo, unscaled"""
    u = np.asarray(raw, dtype=np.uint8)[:row_bytes(rows, cp)].view(np.uint16).reshape(rows, cp)
    s = hi_slots(1, c_out)
    return bits_to_f64(u[:, s], mode), bits_to_f64(u[:, s + 32], mode)


def decode_f8(raw, rows, cp, c_out):
    """format 2 (conv_ring_f8.hip): per 64 channels hi16 x 64 (f16), then the F panel [hi8 c0-31 | lo8 c0-31 | hi8 c32-63 |
    lo8 c32-63] of e4m3 bytes; the scale plane [panel][row stride][4] = E8M0 bytes (s0, s0 - 11, s1, s1 - 11) behind the rows.
    -> (hi16, lo8, hi8, scales): float64 [rows, c_out] with the 8-bit halves already x 2^(s - 127), scales uint8 [rows, panels, 4].
    A consuming layer uses hi16 + lo8."""
    raw = np.asarray(raw, dtype=np.uint8)
    P = cp // 128
    body = raw[:row_bytes(rows, cp)].reshape(rows, P, 256)
    hi = body[:, :, :128].copy().view(np.float16).reshape(rows, P * 64).astype(np.float64)[:, :c_out]
    f = body[:, :, 128:].reshape(rows, P, 2, 2, 32)                  # [row][panel][half][hi8 / lo8][32]
    so, stride = f8_scale_offset(rows, cp), f8_scale_stride(rows)
    sc = raw[so:so + P * stride * 4].reshape(P, stride, 4)[:, :rows]
    sc = np.ascontiguousarray(np.transpose(sc, (1, 0, 2)))           # [row][panel][s0, s0 - 11, s1, s1 - 11]
    val = e4m3(f) * 2.0 ** (sc.reshape(rows, P, 2, 2).astype(np.float64)[..., None] - 127.0)
    hi8 = val[:, :, :, 0, :].reshape(rows, P * 64)[:, :c_out]
    lo8 = val[:, :, :, 1, :].reshape(rows, P * 64)[:, :c_out]
    return hi, lo8, hi8, sc


def decode_rows(raw, rows, cp, c_out, rows_format, mode):
    """the values a consuming layer reads, float64 [rows, c_out], in any of the three formats"""
    if rows_format == 0:
        return decode_plain(raw, rows, cp, c_out, mode)
    if rows_format == 1:
        hi, lo = decode_split(raw, rows, cp, c_out, mode)
        return hi + lo
    hi, lo8, _, _ = decode_f8(raw, rows, cp, c_out)
    return hi + lo8


def pad_slot_mask(rows_format, cp, c_out):
    """bool [2 cp]: the BYTES of a row that belong to no channel (format 1: hi and lo slots; format 2: the hi16 slots and both
    e4m3 bytes of the channels behind c_out - 1)"""
    used = np.zeros(2 * cp, dtype=bool)
    c = np.arange(c_out)
    s = hi_slots(rows_format, c_out)
    used[2 * s] = used[2 * s + 1] = True
    if rows_format == 1:
        used[2 * (s + 32)] = used[2 * (s + 32) + 1] = True
    elif rows_format == 2:
        b = (c >> 6) * 256 + 128 + ((c >> 5) & 1) * 64 + (c & 31)
        used[b] = used[b + 32] = True
    return ~used


def pad_row_mask(lens, bases, rows_per_block, shift):
    """bool [rows]: rows of the buffer that no read fills - behind a read's last valid row (len >> shift) inside its blocks"""
    mask = np.ones(int(bases[-1]) * rows_per_block, dtype=bool)
    for k, n in enumerate(lens):
        r0 = int(bases[k]) * rows_per_block
        mask[r0:r0 + (int(n) >> shift)] = False
    return mask


# ------------------------------------------------------------------------------------------------ weights
def weight_scale(w, mode):
    """2^k with max |w| 2^k in [8192, 16384) in the f16 family, 1 in the bf16 family (convnet_pack.hpp: weight_scale)"""
    if base16(mode) != "f16":
        return 1.0
    wmax = float(np.abs(np.asarray(w, dtype=np.float32)).max())
    if not (wmax > 0.0 and np.isfinite(wmax)):
        return 1.0
    return float(2.0 ** min(60, max(-60, 13 - int(np.floor(np.log2(wmax))))))


def plain_weights(w, mode):
    """the weights a plain 16-bit layer multiplies with, in float64: to_h16(w ws) / ws (PlainLayout::put, w_unscale)"""
    ws = weight_scale(w, mode)
    return round16(np.asarray(w, dtype=np.float32).astype(np.float64) * ws, mode) / ws


def split_weights(w, mode):
    """(hi, lo) of the split-precision packing in float64, unscaled: hi = to_h16(w ws), lo = to_h16(w ws - hi) (SplitLayout::put)"""
    ws = weight_scale(w, mode)
    hi, lo = split16(np.asarray(w, dtype=np.float32).astype(np.float64) * ws, mode)
    return hi / ws, lo / ws


def layer_weights(w, mode):
    """the weights of the float64 reference: the packed values in the plain modes, the original fp32 ones in the split modes
    (hi + lo differs from them by less than the arithmetic's own floor)"""
    return plain_weights(w, mode) if mode in PLAIN_MODES else np.asarray(w, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the planner's rules
def ring_tail(mode, c_in, f8_layer=False):
    """whether plan_h16 (convnet_pack.hpp) packs the layer's last panel as the merged tail slab"""
    panels = (c_in + 31) // 32
    return mode in SPLIT_MODES and not f8_layer and 1 <= c_in % 32 <= 8 and 3 <= panels <= 5


def f8_flags(mode, channels, min_cin):
    """f8[i], i = 0 .. n_layers: layer i can take part in a run of F8 rows (convnet_pack.hpp: f8_eligible, f8_layers).  Layer i
    reads F8 rows if f8[i - 1] and f8[i], writes them if f8[i] and f8[i + 1]"""
    n = len(channels)
    return [mode == "f16xf8" and 3 <= i < n and channels[i - 1] >= max(64, min_cin) for i in range(n + 1)]


def wres_fits(mode, c_in, cp_in, c_out):
    """conv_wres_h16.hip: pick_shape - 256-row tiles of all 2 .. 7 16-channel groups, the whole weight tensor in LDS"""
    n16 = (c_out + 15) // 16
    panels = (c_in + 31) // 32 if mode in SPLIT_MODES else (cp_in + 63) // 64
    lds = 2 * (256 + 8) * 128 + 3072 + panels * 3 * 16 * n16 * 128
    return 2 <= n16 <= 7 and lds <= 160 * 1024 and not ring_tail(mode, c_in)


def ring_tiles():
    """{(bm, bn)} of conv_ring_h16.hip's kShapes[], read out of the source"""
    import os
    import re
    with open(os.path.join(R.CSRC, "conv_ring_h16.hip")) as f:
        body = re.search(r"kShapes\[\]\s*=\s*\{(.*?)\n\};", f.read(), re.S).group(1)
    shapes = re.findall(r"RS_SHAPE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", re.sub(r"//[^\n]*", "", body))
    return {(int(wm) * 16 * int(mt), int(wn) * 16 * int(nt)) for wm, wn, mt, nt in shapes}


# ------------------------------------------------------------------------------------------------ nets and reads
F8_ENV = {"RS_F8_MIN_CIN": "64"}
# name -> (channels, env when the model is created, modes)
NETS = {
    "ship": (synth.CHANNELS, {}, MODES),
    "tail": ((20, 30, 65, 72, 104, 136, 73, 40, 48), {}, MODES),            # both sides of every tail-merge bound
    "wide6": ((20, 32, 32, 96, 130, 200), {}, MODES),
    "odd5": ((12, 24, 33, 40, 50), {}, MODES),
    "narrow3": ((8, 17, 48), {}, MODES),                                     # the streaming kernels' width classes
    "f8net": ((20, 30, 64, 70, 130, 200, 250, 96), F8_ENV, ("f16xf8", "f16x3")),   # partial 64-channel scale panels
}
CASES = [(mode, net) for net, spec in NETS.items() for mode in spec[2]]
SIG_SEED = 20260106
_READS = {}


def reads(n_layers):
    """[(int16 signal, normalised float64)] per length of convnet_ref.sweep_lengths: every read its own signal, normalised on
    its own"""
    if n_layers not in _READS:
        out = []
        for k, n in enumerate(R.sweep_lengths(n_layers)):
            s = synth.make_signals(SIG_SEED, 1, n, first_read=7300 + k)[0]
            out.append((s, np.asarray(ro.mad_normalise(s), dtype=np.float64)))
        _READS[n_layers] = out
    return _READS[n_layers]


# ------------------------------------------------------------------------------------------------ one layer in float64
LO_MUTANTS = ("x_lo_w_hi_missing", "x_hi_w_lo_missing", "output_lo_not_stored")        # split modes only
STRUCTURAL = ("drop_last_channel", "last_pair_not_pooled", "left_neighbour_of_previous_read")
MUTANTS = LO_MUTANTS[:2] + ("tail_taps_swapped",) + STRUCTURAL + LO_MUTANTS[2:]


def layer_f64(x, w, b, mode, mutant=None, prev_last=None):
    """convnet_ref.layer_f64 of ONE read, x [C_in, L] -> [C_out, L // 2], with the defects of the 16-bit kernels on top of its
    own.  A missing cross product is the layer of the stacked input [x; part of x] under the weights [w, -part of w] (a conv is
    linear in both); w: the weights the mode multiplies with (layer_weights)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if mutant is None or mutant in STRUCTURAL:
        return R.layer_f64(x, w, b, mutant=mutant, prev_last=prev_last)
    assert mutant in MUTANTS, mutant
    if mutant == "tail_taps_swapped":                           # the merged tail slab: K group kw = tap kw's 8 channel slots
        c0 = 32 * (w.shape[1] // 32)
        assert ring_tail(mode, w.shape[1]) and c0 < w.shape[1]
        w = w.copy()
        w[:, c0:, [0, 2]] = w[:, c0:, [2, 0]]
        return R.layer_f64(x, w, b)
    assert mode in SPLIT_MODES, (mutant, mode)
    if mutant == "output_lo_not_stored":
        return round16(R.layer_f64(x, w, b), mode)
    x_hi, x_lo = split16(x, mode)
    w_hi, w_lo = split_weights(w.astype(np.float32), mode)
    xm, wm = (x_lo, w_hi) if mutant == "x_lo_w_hi_missing" else (x_hi, w_lo)
    return R.layer_f64(np.concatenate([x, xm]), np.concatenate([w, -wm], axis=1), b)


def three_products(x, w, b, mode):
    """what the split-precision arithmetic can give at best, in float64: x_hi w_hi + x_lo w_hi + x_hi w_lo (the lo lo term
    dropped), bias, ReLU, pool; not yet stored (store, f8_store).  x [C_in, L] as decoded (hi + lo), w the fp32 weights"""
    x_hi, x_lo = split16(x, mode)
    w_hi, w_lo = split_weights(w, mode)
    return R.layer_f64(np.concatenate([x_hi, x_lo, x_hi]), np.concatenate([w_hi, w_hi, w_lo], axis=1), b)


def e4m3_round(a):
    """a rounded to nearest even to OCP e4m3 (4 significant bits, subnormals of 2^-9, saturating at 448), as float64: the value
    of convnet_pack.hpp's to_e4m3 and of the epilogue's conversion"""
    a = np.asarray(a, dtype=np.float64)
    m = np.abs(a)
    e = np.clip(np.floor(np.log2(np.where(m > 0, m, 1.0))), -6, 8)
    q = np.exp2(e - 3)
    return np.sign(a) * np.minimum(np.rint(m / q) * q, 448.0)


def f8_store(y):
    """a float64 activation [C, L] as an F8 row holds it for the next layer (conv_ring_f8.hip): hi = f16(y) and, per position and
    32 channels, lo8 = e4m3((y - hi) 2^(11 - e)) with e = the block maximum's exponent - 7 (its exponent field at least 1)"""
    y = np.asarray(y, dtype=np.float64)
    C, L = y.shape
    hi = round16(y, "f16")
    top = np.pad(hi, ((0, -C % 32), (0, 0))).reshape(-1, 32, L).max(axis=1)
    f = np.maximum(np.floor(np.log2(np.where(top > 0, top, 1.0))) + 15, 1) * (top > 0) + (top <= 0)
    e = np.repeat(f - 22, 32, axis=0)[:C]
    return hi + e4m3_round((y - hi) * np.exp2(11 - e)) * np.exp2(e - 11)


def f8_products(x_hi, x_hi8, x_lo8, w, b):
    """what the 8-bit kernel's arithmetic can give at best on F8 rows, before its output is stored: x_hi w_hi in f16 operands plus
    the cross terms as ONE e4m3 product, q(x_hi) q(w_lo) + q(x_lo) q(w_hi) (F8Layout: hi8 = e4m3(hi 2^-6), lo8 = e4m3(lo 2^5) of
    the scaled weights), bias, ReLU, pool - all sums in float64.  x_* [C_in, L] as decode_f8 returns them, w the fp32 weights"""
    ws = weight_scale(w, "f16xf8")
    wv = np.asarray(w, dtype=np.float32).astype(np.float64) * ws
    w_hi = round16(wv, "f16")
    w_hi8, w_lo8 = e4m3_round(w_hi * 2.0 ** -6) * 2.0 ** 6, e4m3_round((wv - w_hi) * 2.0 ** 5) * 2.0 ** -5
    return R.layer_f64(np.concatenate([x_hi, x_hi8, x_lo8]), np.concatenate([w_hi, w_lo8, w_hi8], axis=1) / ws, b)


def store(v, mode):
    """a float64 activation as the mode stores it: one rounding (plain), hi + lo (split)"""
    if mode in PLAIN_MODES:
        return round16(v, mode)
    hi, lo = split16(v, mode)
    return hi + lo


def layer_inputs(channels, mode, x, upto):
    """float64 inputs of layers 0 .. upto of one normalised read x [L] for a net in `mode`'s weights, each layer's output held
    in float64 (no storage rounding): what the mutant and liveness tests run on"""
    sd = R.state_dict(channels)
    h = np.asarray(x, dtype=np.float64)[None, :]
    out = [h]
    for i in range(upto):
        w = sd[f"layers.{i}.0.weight"]
        h = R.layer_f64(h, layer_weights(w, mode) if i else w, sd[f"layers.{i}.0.bias"])
        out.append(h)
    return out


KEYS = ("stream", "wres", "ring", "ring_tail", "thin", "f8")
# the modes a kernel class exists in
KEY_MODES = {"stream": MODES, "wres": MODES, "ring": MODES, "ring_tail": SPLIT_MODES, "thin": SPLIT_MODES, "f8": ("f16xf8",)}


def layer_classes(mode, channels, i, f8_min_cin=200):
    """the kernel classes that can run conv layer i >= 1 of a net in the planner's default forms (convnet_forward.hpp:
    select_kernel): F8 rows > streaming > thin (split precision, by the launch's size) > weights-resident > ring"""
    c_in, c_out = channels[i - 1], channels[i]
    f8 = f8_flags(mode, channels, f8_min_cin)
    if (f8[i - 1] and f8[i]) or (f8[i] and f8[i + 1]):
        return {"f8"}
    if i <= 2 and c_in <= 32 and c_out <= 48:
        return {"stream"}
    out = {"ring_tail"} if ring_tail(mode, c_in) else {"ring"}
    if wres_fits(mode, c_in, (c_in + 7) // 8 * 8, c_out):
        out.add("wres")
    if mode in SPLIT_MODES:
        out.add("thin")
    return out
