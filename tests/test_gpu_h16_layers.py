"""The five 16-bit modes of the ConvNet (bf16x3, f16x3, f16xf8, f16, bf16) held to float64 one layer at a time, on the kernels
of conv_stream_h16.hip, conv_wres_h16.hip, conv_ring_h16.hip, conv_thin_h16.hip and conv_ring_f8.hip.

Per (mode, net) of tests/h16_ref.py (the shipped net; `tail` on both sides of every tail-merge bound; `wide6`, `odd5`,
`narrow3`; `f8net` with partial 64-channel scale panels) on one ragged batch of 77 reads (convnet_ref.sweep_lengths, each read
its own signal, NaNs behind every read):
  float64     every conv layer i >= 1 of the planner's own model against conv -> bias -> ReLU -> MaxPool in float64 computed
              from the DECODED capture of the device's layer i - 1 (one kernel's error, not twelve layers' sum), every read,
              valid row and channel.  Split modes and F8 layers: max |got - ref| / max(1, max |ref|) per (mode, kernel that ran
              the layer).  Plain modes: elementwise |got - ref| <= ulp16(ref) / 2 + A max(1, max |ref|) - the device rounds
              once, to nearest even, an fp32 value within the accumulation error of ref; A is the one measured term.  Pad rows
              and pad channel slots hold zero bits, lo slots included.  Logits and probabilities against the float64 forward.
  same bits   on the nets no other test runs: the capture of every layer and the logits equal bit for bit under the default,
              RS_THIN_H16_ROWS=0 / =100000000, a forced ring shape with and without RS_H16_WRES=0 (the force makes the ring
              launch readable from rs_layer_info) and RS_NO_STREAM_H16=1; through classify_raw on the int16 reads
              under the default (one launch for layers 0 + 1 + 2), RS_NO_STREAM012=1 and RS_NO_STREAM_H16=1.
  coverage    every kernel class in every mode it exists in, and the channel edges of the packings, from rs_layer_info.
The bars are about four times the largest gap measured on an MI355X (below, next to each other;
profiles/h16_layers_gpu_tests.txt); on the CPU every mutant of h16_ref (a defect of the float64 layer) must miss by more than
ten times the bar of the layer class it hits."""
import contextlib
import re
import time

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import synth
from tests import convnet_ref as R
from tests import h16_ref as H

from conftest import hooked_model

# ---- split modes and F8 layers: device against float64 per layer, x max(1, max |reference|) of the layer and read, per
# (mode, kernel).  Measured on an MI355X over the whole sweep (every net, layer, read, row, channel), and the bar: about 4x,
# rounded up.  Beside them, on reads FLOOR_READS from the same inputs: the arithmetic's own floor (float64 sums of the three
# products hi hi + lo hi + hi lo, stored as hi + lo; F8 layers: the cross terms as one e4m3 product, and the lo half of an F8
# row kept to four bits) and numpy's fp32 conv.  bf16x3 sits at 1.0 - 1.5 x its floor.  f16x3's floor is 50 times lower and
# fp32 accumulation takes over: its kernels sit at 2.0 - 2.7 x numpy fp32 (the fp32 kernels: 1 - 2 x, test_gpu_f32_shapes.py);
# the thin kernel's 13 x floor is layer 11 of the shipped net, a sum of 3405 products.  The 8-bit kernel sits at 1.2 x ITS floor.
LAYER_GAP = {
    ("bf16x3", "stream"): 1.0e-5, ("bf16x3", "wres"): 1.1e-5, ("bf16x3", "ring"): 9.1e-6, ("bf16x3", "ring_tail"): 9.7e-6, ("bf16x3", "thin"): 1.1e-5,
    ("f16x3", "stream"): 4.7e-7, ("f16x3", "wres"): 5.5e-7, ("f16x3", "ring"): 7.0e-7, ("f16x3", "ring_tail"): 9.0e-7, ("f16x3", "thin"): 1.7e-6,
    ("f16xf8", "stream"): 4.7e-7, ("f16xf8", "wres"): 5.5e-7, ("f16xf8", "ring"): 6.6e-7, ("f16xf8", "ring_tail"): 9.0e-7, ("f16xf8", "thin"): 6.4e-7, ("f16xf8", "f8"): 2.1e-5,
}
LAYER_FLOOR = {
    ("bf16x3", "stream"): 8.7e-6, ("bf16x3", "wres"): 1.0e-5, ("bf16x3", "ring"): 6.6e-6, ("bf16x3", "ring_tail"): 7.6e-6, ("bf16x3", "thin"): 7.2e-6,
    ("f16x3", "stream"): 1.5e-7, ("f16x3", "wres"): 1.2e-7, ("f16x3", "ring"): 1.3e-7, ("f16x3", "ring_tail"): 1.3e-7, ("f16x3", "thin"): 1.3e-7,
    ("f16xf8", "stream"): 1.5e-7, ("f16xf8", "wres"): 1.2e-7, ("f16xf8", "ring"): 1.2e-7, ("f16xf8", "ring_tail"): 1.2e-7, ("f16xf8", "thin"): 1.2e-7, ("f16xf8", "f8"): 1.8e-5,
}
LAYER_NUMPY32 = {
    ("bf16x3", "stream"): 2.2e-7, ("bf16x3", "wres"): 2.5e-7, ("bf16x3", "ring"): 2.7e-7, ("bf16x3", "ring_tail"): 3.2e-7, ("bf16x3", "thin"): 9.9e-7,
    ("f16x3", "stream"): 1.8e-7, ("f16x3", "wres"): 2.1e-7, ("f16x3", "ring"): 3.1e-7, ("f16x3", "ring_tail"): 3.9e-7, ("f16x3", "thin"): 8.3e-7,
    ("f16xf8", "stream"): 1.8e-7, ("f16xf8", "wres"): 2.1e-7, ("f16xf8", "ring"): 3.1e-7, ("f16xf8", "ring_tail"): 3.9e-7, ("f16xf8", "thin"): 3.5e-7, ("f16xf8", "f8"): 7.8e-7,
}
LAYER_TOL = {
    ("bf16x3", "stream"): 5e-5, ("bf16x3", "wres"): 5e-5, ("bf16x3", "ring"): 4e-5, ("bf16x3", "ring_tail"): 4e-5, ("bf16x3", "thin"): 5e-5,
    ("f16x3", "stream"): 2e-6, ("f16x3", "wres"): 3e-6, ("f16x3", "ring"): 3e-6, ("f16x3", "ring_tail"): 4e-6, ("f16x3", "thin"): 7e-6,
    ("f16xf8", "stream"): 2e-6, ("f16xf8", "wres"): 3e-6, ("f16xf8", "ring"): 3e-6, ("f16xf8", "ring_tail"): 4e-6, ("f16xf8", "thin"): 3e-6, ("f16xf8", "f8"): 9e-5,
}
# ---- plain modes: A of |got - ref| <= ulp16(ref) / 2 + A max(1, max |ref|), the fp32 accumulation allowance: measured, bar
PLAIN_A_GAP = {
    ("f16", "stream_l1"): 2.0e-4, ("f16", "stream"): 7.4e-8, ("f16", "wres"): 1.1e-7, ("f16", "ring"): 5.0e-7,
    ("bf16", "stream_l1"): 6.8e-4, ("bf16", "stream"): 2.6e-8, ("bf16", "wres"): 6.3e-8, ("bf16", "ring"): 1.3e-7,
}
PLAIN_A_TOL = {
    ("f16", "stream_l1"): 9e-4, ("f16", "stream"): 3e-7, ("f16", "wres"): 5e-7, ("f16", "ring"): 2.1e-6,
    ("bf16", "stream_l1"): 3e-3, ("bf16", "stream"): 1.1e-7, ("bf16", "wres"): 3e-7, ("bf16", "ring"): 6e-7,
}
# ---- end to end per mode: logits x max(1, |logit|), probabilities absolute: measured, bar (the probabilities of the plain
# modes: never above their envelope of test_gpu_parity.H16_TOL)
E2E_GAP = {"bf16x3": {"logits": 3.0e-4, "probs": 3.8e-5}, "f16x3": {"logits": 2.0e-5, "probs": 3.0e-6},
           "f16xf8": {"logits": 8.6e-4, "probs": 1.2e-4}, "f16": {"logits": 2.5e-2, "probs": 6.7e-3}, "bf16": {"logits": 1.4e-1, "probs": 3.7e-2}}
E2E_TOL = {"bf16x3": {"logits": 1.2e-3, "probs": 2e-4}, "f16x3": {"logits": 8e-5, "probs": 1.3e-5},
           "f16xf8": {"logits": 4e-3, "probs": 5e-4}, "f16": {"logits": 1e-1, "probs": 2e-2}, "bf16": {"logits": 6e-1, "probs": 1.5e-1}}

# plain modes, layer 1: its input is layer 0's fp32 result rounded to storage while the reference rounds the float64 one; where
# the two roundings fall on different sides an input moves by ulp16(x) and an output by |w| ulp16(x) (measured: about 1e-4 in
# f16, 4e-4 in bf16, as 0.2 x 2^-9 and 0.2 x 2^-6 over a scale of 4 ... 8 predict).  Kept in a key of its own so that it does
# not widen the allowance of layer 2, which the same streaming kernel runs from the device's own rows.
STREAM_L1 = "stream_l1"
BASE_ENV = {"RS_TAIL_DEBUG": "1"}          # prints the thin-or-ring decision of every launch; changes none
THIN_ALL = {"RS_THIN_H16_ROWS": "100000000"}
# (mode, net, form): the planner's default form of every case, and the thin-launch kernel forced onto `tail` in the split modes
# (on 77 reads the planner itself takes it on few layers or none)
SWEEP = [(mode, net, "") for mode, net in H.CASES] + [(mode, "tail", "thin") for mode in H.SPLIT_MODES]
FLOOR_READS = (0, 1, 2, 40)                # the reads the three-product floor is computed on (3 x the reference's cost)

# mutants that an honest bar cannot see past by 10 x: (mutant, mode, net, layer) -> reason
MUTANTS_NOT_SEEN = {("drop_last_channel", "f16xf8", "f8net", 6): "channel 199 of layer 5 is dead under these weights (ReLU): nothing to drop"}
for _m in H.LO_MUTANTS:
    for _i in range(3, 8):
        MUTANTS_NOT_SEEN[(_m, "f16xf8", "f8net", _i)] = "the 8-bit cross terms keep four bits: the F8 bar is above a tenth of a lost lo half"


def _tol(mode, key):
    return (PLAIN_A_TOL if mode in H.PLAIN_MODES else LAYER_TOL)[(mode, key)]


# ------------------------------------------------------------------------------------------------ CPU: decoders
def _encode_split(v_hi, v_lo, cp, mode):
    """rows of 32-channel panels [hi x 32 | lo x 32] (rs_layer_info: rows_format 1), pad slots zero"""
    rows, C = v_hi.shape
    u = np.zeros((rows, cp), dtype=np.uint16)
    bits = H.f16_bits if H.base16(mode) == "f16" else H.bf16_bits
    for c in range(C):
        u[:, 64 * (c // 32) + c % 32] = bits(v_hi[:, c])
        u[:, 64 * (c // 32) + 32 + c % 32] = bits(v_lo[:, c])
    return u.view(np.uint8).reshape(-1)


def _to_e4m3(a):
    """nearest e4m3 byte of 0 <= a < 256 by table search (ties: the even mantissa)"""
    table = H.e4m3(np.arange(0x7F))
    a = np.asarray(a, dtype=np.float64)
    d = np.abs(a[..., None] - table)
    best = d.min(axis=-1, keepdims=True)
    cand = np.where(d == best, np.arange(0x7F), 1000)
    lo = cand.min(axis=-1)
    hi = np.where(d == best, np.arange(0x7F), -1).max(axis=-1)
    return np.where(lo % 2 == 0, lo, hi).astype(np.uint8)


def _encode_f8(v, cp):
    """F8 rows from conv_ring_f8.hip's description: per 64 channels hi16 x 64, then [hi8 c0-31 | lo8 c0-31 | hi8 c32-63 |
    lo8 c32-63]; per row and 32 channels e = floor(log2 max hi) - 7 (an all-zero or subnormal block: the exponent field 1),
    hi8 = e4m3(hi 2^-e), lo8 = e4m3((v - hi) 2^(11 - e)); scale plane [panel][stride][4] = (e + 127, e + 116) per block"""
    rows, C = v.shape
    P = cp // 128
    hi = v.astype(np.float16)
    lo = v - hi.astype(np.float64)
    body = np.zeros((rows, P, 256), dtype=np.uint8)
    stride = H.f8_scale_stride(rows)
    plane = np.zeros((P, stride, 4), dtype=np.uint8)
    for blk in range(2 * P):
        c0, c1 = 32 * blk, min(32 * blk + 32, C)
        p, h = blk // 2, blk % 2
        f = np.ones(rows, dtype=np.int64)                               # biased f16 exponent of the block maximum, at least 1
        if c1 > c0:
            top = hi[:, c0:c1].max(axis=1).view(np.uint16).astype(np.int64)
            f = np.maximum(top >> 10, 1)
            e = (f - 22).astype(np.float64)
            body[:, p, 64 * h:64 * h + 2 * (c1 - c0)] = hi[:, c0:c1].copy().view(np.uint8).reshape(rows, -1)
            body[:, p, 128 + 64 * h:128 + 64 * h + c1 - c0] = _to_e4m3(hi[:, c0:c1].astype(np.float64) * 2.0 ** -e[:, None])
            body[:, p, 160 + 64 * h:160 + 64 * h + c1 - c0] = _to_e4m3(np.abs(lo[:, c0:c1]) * 2.0 ** (11 - e[:, None])) | \
                np.where(lo[:, c0:c1] < 0, 0x80, 0).astype(np.uint8)
        plane[p, :rows, 2 * h] = f + 105
        plane[p, :rows, 2 * h + 1] = f + 94
    raw = np.zeros(H.capture_bytes(rows, cp, 2), dtype=np.uint8)
    raw[:rows * cp * 2] = body.reshape(-1)
    raw[H.f8_scale_offset(rows, cp):] = plane.reshape(-1)
    return raw


@pytest.mark.parametrize("mode", H.MODES)
def test_plain_and_split_decoders_invert_an_encoder(mode):
    rng = np.random.default_rng(11)
    for C in (1, 31, 32, 33, 70, 96):
        rows = 5
        v = np.abs(rng.standard_normal((rows, C))) * 3.0
        v[0, 0], v[1, C - 1] = 0.0, 60000.0 if H.base16(mode) == "f16" else 3.0e38
        if mode in H.PLAIN_MODES:
            cp = (C + 7) // 8 * 8
            u = np.zeros((rows, cp), dtype=np.uint16)
            u[:, :C] = (H.f16_bits if mode == "f16" else H.bf16_bits)(v)
            got = H.decode_rows(u.view(np.uint8).reshape(-1), rows, cp, C, 0, mode)
            assert np.array_equal(got, H.round16(v, mode))
            pad = H.pad_slot_mask(0, cp, C)
            assert pad.sum() == 2 * (cp - C) and not pad[:2 * C].any()
        else:
            cp = 64 * ((C + 31) // 32)
            hi, lo = H.split16(v, mode)
            raw = _encode_split(hi, lo, cp, mode)
            ghi, glo = H.decode_split(raw, rows, cp, C, mode)
            assert np.array_equal(ghi, hi) and np.array_equal(glo, lo)
            assert np.array_equal(H.decode_rows(raw, rows, cp, C, 1, mode), hi + lo)
            pad = H.pad_slot_mask(1, cp, C)
            assert pad.sum() == 2 * (cp - 2 * C)                                # hi AND lo slots of the ragged last panel
            body = raw.reshape(rows, 2 * cp)
            assert not body[:, pad].any() and body[:, ~pad].reshape(rows, -1).any()
            junk = body.copy()
            junk[:, pad] = 0xFF                                                 # the decoders never read a pad slot
            assert np.array_equal(H.decode_rows(junk.reshape(-1), rows, cp, C, 1, mode), hi + lo)


def test_f8_decoder_inverts_an_encoder():
    """ragged last 64-channel panel, a block whose maximum sits at both ends of [128, 256) after scaling, an all-zero block"""
    rng = np.random.default_rng(12)
    for C in (40, 64, 70, 130):
        rows = 6                                                                # the plane's row stride is 8
        cp = 128 * ((C + 63) // 64)
        v = np.abs(rng.standard_normal((rows, C))) * 2.0
        v[0, :32] = np.abs(rng.standard_normal(32)) * 0.5
        v[0, 3] = 4.0                                   # block maximum 2^2: scaled to 128, the low end
        v[1, :32] = np.abs(rng.standard_normal(32)) * 0.5
        v[1, 5] = 8.0 * (1 - 2.0 ** -11)                # the largest f16 below 2^3: scaled to just under 256
        v[2, :32] = 0.0                                 # an all-zero block
        raw = _encode_f8(v, cp)
        hi, lo8, hi8, sc = H.decode_f8(raw, rows, cp, C)
        assert sc.shape == (rows, cp // 128, 4)
        assert np.array_equal(hi, v.astype(np.float16).astype(np.float64))
        assert sc[0, 0, 0] == 127 + 2 - 7 and sc[1, 0, 0] == 127 + 2 - 7 and tuple(sc[2, 0, :2]) == (106, 95)
        assert np.array_equal(sc[..., 1], sc[..., 0] - 11) and np.array_equal(sc[..., 3], sc[..., 2] - 11)
        assert hi8[0, 3] == 4.0 and hi8[1, 5] == 8.0 and not hi8[2, :32].any() and not lo8[2, :32].any()
        # the block's largest value lands in [128, 256): hi8 keeps 4 bits of it, lo8 4 bits of a lo half below 2^-11 of it
        bmax = np.repeat(np.maximum(np.pad(hi, ((0, 0), (0, -C % 32))).reshape(rows, -1, 32).max(axis=2), 2.0 ** -14), 32, axis=1)[:, :C]
        assert (np.abs(hi8 - hi) <= bmax * 2.0 ** -4).all()
        assert (np.abs(lo8 - (v - hi)) <= bmax * 2.0 ** -15).all()
        assert np.array_equal(H.decode_rows(raw, rows, cp, C, 2, "f16xf8"), hi + lo8)
        assert np.array_equal(H.f8_store(v.T).T, hi + lo8)                      # the value-level mirror the F8 floor is built on
        assert np.array_equal(H.e4m3_round(H.e4m3(np.arange(0x7F))), H.e4m3(np.arange(0x7F))) and H.e4m3_round(500.0) == 448.0
        pad = H.pad_slot_mask(2, cp, C)
        assert pad.sum() == 2 * cp - 4 * C                                      # 2 bytes of hi16, one of hi8, one of lo8 per channel
        assert not raw[:rows * cp * 2].reshape(rows, -1)[:, pad].any()
        assert H.f8_scale_offset(rows, cp) % 256 == 0 and H.f8_scale_offset(3, 128) == 768 and H.f8_scale_offset(5, 128) == 1280
        assert raw.size == H.f8_scale_offset(rows, cp) + (cp // 128) * 8 * 4


def test_pad_row_mask():
    m = H.pad_row_mask([9, 4], np.array([0, 2, 3]), 4, 1)                       # rows per read: 4, 2 of blocks of 4 rows
    assert m.tolist() == [False] * 4 + [True] * 4 + [False] * 2 + [True] * 2


def test_roundings_and_ulp_on_hand_worked_values():
    f, b = "f16", "bf16"
    # f16: 11 significant bits.  2049 is a tie between 2048 and 2050: even is 2048; 2051 -> 2052
    assert H.round16(2049.0, f) == 2048.0 and H.round16(2051.0, f) == 2052.0 and H.round16(2049.0001, f) == 2050.0
    assert H.round16(65504.0, f) == 65504.0 and H.round16(65519.9, f) == 65504.0 and np.isinf(H.round16(65520.0, f))
    assert H.round16(2.0 ** -24, f) == 2.0 ** -24 and H.round16(2.0 ** -25, f) == 0.0 and H.round16(1.5 * 2.0 ** -24, f) == 2.0 ** -23
    # bf16: 8 significant bits.  257 is a tie between 256 and 258: 256; 259 -> 260
    assert H.round16(257.0, b) == 256.0 and H.round16(259.0, b) == 260.0 and H.round16(257.001, b) == 258.0
    assert H.round16(-1.00390625, b) == -1.0 and H.round16(1.01171875, b) == 1.015625          # 1 + 2^-8 (tie), 1 + 3 2^-8 (tie)
    assert H.bf16_bits(np.float32(1.0))[()] == 0x3F80 and H.bf16_bits(np.float32(3.0e38))[()] == 0x7F62
    assert H.round16(2.0 ** -133, b) == 2.0 ** -133 and H.round16(2.0 ** -127, b) == 2.0 ** -127    # subnormals of fp32's range
    hi, lo = H.split16(np.float64(np.float32(np.pi)), b)
    assert hi == 3.140625 and lo == H.round16(np.float64(np.float32(np.pi)) - 3.140625, b) and abs(hi + lo - np.pi) < 2.0 ** -15
    hi, lo = H.split16(1.0 + 2.0 ** -12, f)
    assert hi == 1.0 and lo == 2.0 ** -12
    assert H.ulp16(1.0, f) == 2.0 ** -10 and H.ulp16(1.999, f) == 2.0 ** -10 and H.ulp16(2.0, f) == 2.0 ** -9
    assert H.ulp16(65504.0, f) == 32.0 and H.ulp16(-3.0, f) == 2.0 ** -9
    assert H.ulp16(2.0 ** -14, f) == 2.0 ** -24 and H.ulp16(2.0 ** -20, f) == 2.0 ** -24 and H.ulp16(0.0, f) == 2.0 ** -24
    assert H.ulp16(1.0, b) == 2.0 ** -7 and H.ulp16(300.0, b) == 2.0 and H.ulp16(0.0, b) == 2.0 ** -133
    assert H.ulp16(np.array([0.75, 4.0]), b).tolist() == [2.0 ** -8, 2.0 ** -5]


def test_plain_weight_mirror_on_hand_worked_scales():
    w = np.array([0.3, -0.02, 0.1001], dtype=np.float32)
    # max |w| = 0.3 in [2^-2, 2^-1): 2^15 puts it at 9830.4, inside [8192, 16384)
    assert H.weight_scale(w, "f16") == 2.0 ** 15 and H.weight_scale(w, "f16x3") == 2.0 ** 15 and H.weight_scale(w, "f16xf8") == 2.0 ** 15
    assert H.weight_scale(w, "bf16") == 1.0 and H.weight_scale(w, "bf16x3") == 1.0
    assert H.weight_scale(np.array([0.25], np.float32), "f16") == 2.0 ** 15 and H.weight_scale(np.array([0.2499], np.float32), "f16") == 2.0 ** 16
    assert H.weight_scale(np.zeros(3, np.float32), "f16") == 1.0 and H.weight_scale(np.array([700.0], np.float32), "f16") == 2.0 ** 4
    # 0.3 x 2^15 = 9830.4 (fp32: 9830.400390625): f16 spacing 8 there -> 9832; -0.02 x 2^15 = -655.36: spacing 0.5 -> -655.5
    p = H.plain_weights(w, "f16")
    assert p[0] == 9832.0 / 2 ** 15 and p[1] == -655.5 / 2 ** 15
    assert np.array_equal(H.plain_weights(w, "bf16"), H.round16(w.astype(np.float64), "bf16"))
    assert H.plain_weights(w, "bf16")[0] == 0.30078125                          # 77 / 256
    hi, lo = H.split_weights(w, "f16x3")
    assert np.array_equal(hi, p) and np.abs(hi + lo - w.astype(np.float64)).max() < 2.0 ** -22 * 0.3
    assert np.array_equal(H.layer_weights(w, "bf16x3"), w.astype(np.float64))


def test_the_planner_mirror():
    ch = H.NETS["tail"][0]
    assert [H.ring_tail("bf16x3", c) for c in ch[2:8]] == [True, True, True, True, False, False]
    assert not H.ring_tail("f16", 65) and not H.ring_tail("f16x3", 33) and not H.ring_tail("f16x3", 161 + 32)
    assert H.f8_flags("f16xf8", H.NETS["f8net"][0], 64) == [False] * 3 + [True] * 5 + [False]
    assert H.f8_flags("f16xf8", synth.CHANNELS, 200) == [False] * 7 + [True] * 5 + [False]
    assert not any(H.f8_flags("f16x3", synth.CHANNELS, 64))
    # conv_wres_h16.hip: 2 (256 + 8) 128 + 3072 + panels 3 bn 128 <= 160 KB: 80 columns hold three panels, not four
    assert H.wres_fits("f16x3", 96, 96, 72) and not H.wres_fits("f16x3", 97, 104, 72) and not H.wres_fits("f16", 20, 24, 113)
    assert H.layer_classes("f16xf8", synth.CHANNELS, 7) == {"f8"} and H.layer_classes("f16x3", synth.CHANNELS, 7) == {"ring", "thin"}
    assert H.layer_classes("bf16", synth.CHANNELS, 1) == {"stream"} and H.layer_classes("bf16", synth.CHANNELS, 3) == {"ring", "wres"}
    assert len(SWEEP) == len(set(SWEEP)) == 5 * 5 + 2 + 3
    # the weights-resident tiles 256 x 16 n16, n16 = 2 .. 7: all but 256 x 64 are ring shapes too; the forced 128 x 128 is none of them
    assert [(256, 16 * n) in H.ring_tiles() for n in range(2, 8)] == [True, True, False, True, True, True]
    assert FORCED_TILE in H.ring_tiles() and FORCED_TILE[0] != 256 and {(64, 32), (512, 64)} <= H.ring_tiles()


def test_sweep_lengths_follow_the_rules_on_every_net():
    for net, (channels, _, _) in H.NETS.items():
        n = len(channels)
        lens = R.sweep_lengths(n)
        assert len(lens) == R.N_READS and min(lens) == 1 << n and max(lens) == R.MAX_LEN, net
        for i in range(n):
            assert {(v >> i) % 4 for v in lens} == {0, 1, 2, 3}, (net, i)
        assert [len(s) for s, _ in H.reads(n)] == lens and all(x.dtype == np.float64 for _, x in H.reads(n))


def test_layer_reference_wraps_the_oracle():
    ch = H.NETS["odd5"][0]
    sd = R.state_dict(ch)
    ins = H.layer_inputs(ch, "bf16x3", H.reads(5)[30][1], 4)
    for i in range(1, 5):
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        want = ro.conv_block(ins[i][None], w, b, acc=np.float64)[0]
        assert np.array_equal(H.layer_f64(ins[i], w, b, "bf16x3"), want), i
        # the three-product sum lacks lo lo (2^-16 of the product in bf16) and stores hi + lo (2^-17): at the arithmetic's floor
        gap = np.abs(H.store(H.three_products(H.store(ins[i], "bf16x3"), w, b, "bf16x3"), "bf16x3") - ro.conv_block(H.store(ins[i], "bf16x3")[None], w, b, acc=np.float64)[0]).max()
        assert 0 < gap < 1e-4 * max(1.0, np.abs(want).max()), (i, gap)


# net -> (the layers the mutants are put into, the reads they run on)
MUTANT_NETS = {"tail": (range(1, 9), (0, 2, 40)), "ship": (range(1, 6), (0, 1, 2)), "f8net": (range(3, 8), (0, 2, 40))}


@pytest.mark.parametrize("net", list(H.NETS))
def test_every_net_is_alive(net):
    """per layer the float64 reference has at least 25 % non-zero elements on a 6024-sample read, and the last input channel of
    every layer that drop_last_channel is used on (MUTANT_NETS) is not dead"""
    channels = H.NETS[net][0]
    n = len(channels)
    s = synth.make_signals(H.SIG_SEED, 1, 6024, first_read=7290)[0]
    ins = H.layer_inputs(channels, "bf16x3", ro.mad_normalise(s), n)
    for i in range(1, n + 1):
        assert (ins[i] != 0).mean() >= 0.25, (net, i - 1, float((ins[i] != 0).mean()))
        if net in MUTANT_NETS and i in MUTANT_NETS[net][0] and not any(k[0] == "drop_last_channel" and k[2:] == (net, i) for k in MUTANTS_NOT_SEEN):
            assert ins[i][-1].any(), (net, i)


# ------------------------------------------------------------------------------------------------ CPU: mutants at the bars


def _mutant_applies(mutant, mode, net, i):
    channels, env, modes = H.NETS[net]
    if mode not in modes or (net == "f8net" and mode != "f16xf8"):
        return False
    classes = H.layer_classes(mode, channels, i, int(env.get("RS_F8_MIN_CIN", 200)))
    if mutant in H.LO_MUTANTS:
        return mode in H.SPLIT_MODES
    if mutant == "tail_taps_swapped":
        return "ring_tail" in classes
    return True


@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("mutant", H.MUTANTS)
def test_mutants_are_caught_at_the_bars(mutant, mode):
    """each defect of the float64 layer, in every layer of `tail`, in layers 1-5 of the shipped net (and, f16xf8, in the F8 layers
    of `f8net`), misses the unmodified reference by more than ten times the mode's bar for the layer class it hits (the largest
    bar among the classes the planner can put the layer in).  Lo-half mutants: split modes only."""
    seen = 0
    for net, (layers, picks) in MUTANT_NETS.items():
        channels, env, _ = H.NETS[net]
        todo = [i for i in layers if _mutant_applies(mutant, mode, net, i) and (mutant, mode, net, i) not in MUTANTS_NOT_SEEN]
        if not todo:
            continue
        sd = R.state_dict(channels)
        rd = H.reads(len(channels))
        ins = [H.layer_inputs(channels, mode, rd[k][1], max(todo)) for k in picks]
        for i in todo:
            classes = H.layer_classes(mode, channels, i, int(env.get("RS_F8_MIN_CIN", 200)))
            if mutant == "tail_taps_swapped":
                classes = classes & {"ring_tail", "thin"}
            if mode in H.PLAIN_MODES and i == 1:
                classes = {STREAM_L1}
            bar = max(_tol(mode, key) for key in classes)
            w, b = H.layer_weights(sd[f"layers.{i}.0.weight"], mode), sd[f"layers.{i}.0.bias"]
            miss = 0.0
            for j, h in enumerate(ins):
                x = H.store(h[i], mode)
                ref = H.layer_f64(x, w, b, mode)
                bad = H.layer_f64(x, w, b, mode, mutant=mutant, prev_last=ins[j - 1][i][:, -1])
                scale = max(1.0, float(np.abs(ref).max()))
                if mode in H.PLAIN_MODES:                                     # in units of the elementwise bound
                    miss = max(miss, float((np.abs(bad - ref) / (H.ulp16(ref, mode) / 2 + bar * scale)).max()))
                else:
                    miss = max(miss, float(np.abs(bad - ref).max()) / scale / bar)
            assert miss > 10, (mutant, mode, net, i, sorted(classes), miss)
            seen += 1
    applies = mutant not in H.LO_MUTANTS + ("tail_taps_swapped",) or mode in H.SPLIT_MODES
    assert (seen > 0) == applies, (mutant, mode, seen)                        # at least one layer per (mutant, mode)


def test_the_bars_are_about_four_times_the_measured_gaps():
    for gaps, tols in ((LAYER_GAP, LAYER_TOL), (PLAIN_A_GAP, PLAIN_A_TOL)):
        assert set(gaps) == set(tols)
        for key, g in gaps.items():
            assert 3.9 * g <= tols[key] <= 5.5 * g, (key, g, tols[key])
    for mode in H.MODES:
        for what in ("logits", "probs"):
            g, t = E2E_GAP[mode][what], E2E_TOL[mode][what]
            assert 2.9 * g <= t <= 5.5 * g, (mode, what, g, t)           # below 4 x: the plain modes' probabilities, capped
    assert set(LAYER_FLOOR) == set(LAYER_NUMPY32) == set(LAYER_GAP)


def test_the_mutant_table_is_honest():
    for (mutant, mode, net, i), reason in MUTANTS_NOT_SEEN.items():
        assert mutant in H.MUTANTS and _mutant_applies(mutant, mode, net, i) and i in MUTANT_NETS[net][0] and reason
    for mode in H.MODES:
        keys = {k for k in H.KEYS if mode in H.KEY_MODES[k]} | ({STREAM_L1} if mode in H.PLAIN_MODES else set())
        table = PLAIN_A_TOL if mode in H.PLAIN_MODES else LAYER_TOL
        assert {k for m, k in table if m == mode} == keys, mode
    assert set(E2E_TOL) == set(H.MODES)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _model(mode, net, dev, extra=None):
    channels, env, _ = H.NETS[net]
    return hooked_model({**BASE_ENV, **env, **(extra or {})}, R.state_dict(channels), mode, dev, config=R.config(channels))


_BATCH = {}


def _batch(n_layers, dev):
    """the ragged batch as fp32 rows of LD floats, NaN behind every read, as packed int16 reads, and the lengths"""
    import torch
    from riser_amd.preprocess import pack_reads
    if n_layers not in _BATCH:
        rd = H.reads(n_layers)
        x = torch.full((R.N_READS, R.LD), float("nan"), dtype=torch.float32)
        for k, (_, xn) in enumerate(rd):
            x[k, :len(xn)] = torch.from_numpy(xn.astype(np.float32))
        _BATCH[n_layers] = (x.to(dev), pack_reads([s for s, _ in rd], dev), np.array([len(s) for s, _ in rd], dtype=np.int32))
    return _BATCH[n_layers]


def _forward(m, dev, capfd, layer=None, raw_reads=False):
    """(probs, logits, bytes of conv layer `layer`'s output buffer as the device laid it out, layers whose launch took the
    thin kernel) of the ragged batch through forward_batch, or through classify_raw on the int16 reads"""
    import torch
    x, packed, lens = _batch(m.n_layers, dev)
    cap = None
    if layer is not None:
        cap = torch.full((H.capture_bytes(*m.layer_rows(lens, layer)),), 0xA5, dtype=torch.uint8, device=dev)
    capfd.readouterr()
    with m.capture_layer(layer, cap) if layer is not None else contextlib.nullcontext():
        if raw_reads:
            probs, logits = m.classify_raw(*packed, return_logits=True)
        else:
            probs, logits = m.forward_batch(x, lens, return_logits=True)
        torch.cuda.synchronize(dev)
    err = capfd.readouterr().err
    thin = {int(i) for i, what in re.findall(r"\[thin-or-ring\] layer (\d+):[^\n]*-> (thin|ring)", err) if what == "thin"}
    return probs.cpu().numpy(), logits.cpu().numpy(), None if cap is None else cap.cpu().numpy(), thin


def _kernel_of(mode, info, i, thin, wres_on=True):
    """the kernel class that ran conv layer i.  READ from the device after the call: F8 (the row formats), streaming (its 16-row
    tile, which no other kernel has), thin (the launch's own thin-or-ring line, with its 64 x 32 tile), the merged tail (its K
    padding), and that the reported tile is the one the class can launch: 256 x all-columns for the weights-resident kernel, an
    entry of kShapes[] for the ring kernel.  MIRRORED from the planner's rules (h16_ref.wres_fits, wres_on): which of the
    weights-resident and the ring kernel ran a layer both admit - five of the six weights-resident tiles are ring shapes too, so
    rs_layer_info cannot tell them apart; test_every_form_keeps_the_bits reads that back with a forced ring shape."""
    li = info[i]
    n16 = (li["c_out"] + 15) // 16
    tile = (li["bm"], li["bn"])
    if li["rows_format"] == 2 or info[i - 1]["rows_format"] == 2:
        assert mode == "f16xf8" and i not in thin
        return "f8"
    if li["bm"] == 16:
        assert i <= 2 and li["bn"] == 16 * n16 and li["c_in"] <= 32 and li["c_out"] <= 48 and i not in thin
        return "stream"
    if i in thin:
        assert mode in H.SPLIT_MODES and tile == (64, 32)
        return "thin"
    if H.ring_tail(mode, li["c_in"]):
        assert li["k_pad"] == (3 * ((li["c_in"] + 31) // 32 - 1) + 1) * 32 and tile in H.ring_tiles(), (i, li)
        return "ring_tail"
    if wres_on and H.wres_fits(mode, li["c_in"], li["cp_in"], li["c_out"]):
        assert tile == (256, 16 * n16), (i, li)
        return "wres"
    assert tile in H.ring_tiles(), (i, li)                 # e.g. never the weights-resident 256 x 64, which is no ring shape
    return "ring"


_F64 = {}


def _f64_forward(channels):
    """float64 logits of the ragged batch from the fp32 signal rows the device gets"""
    channels = tuple(channels)
    if channels not in _F64:
        sd = R.state_dict(channels)
        _F64[channels] = np.concatenate([ro.convnet_forward(sd, x.astype(np.float32)[None], acc=np.float64)
                                         for _, x in H.reads(len(channels))])
    return _F64[channels]


_RESULTS = {}


def _case(case, dev, capfd):
    """the float64 sweep of one (mode, net, form), computed once: figures and findings, nothing asserted"""
    if case not in _RESULTS:
        try:
            _RESULTS[case] = _run_case(case, dev, capfd)
        except Exception as e:                                                # kept: the coverage test shows it again
            _RESULTS[case] = e
    if isinstance(_RESULTS[case], Exception):
        raise _RESULTS[case]
    return _RESULTS[case]


def _run_case(case, dev, capfd):
    mode, net, form = case
    channels = H.NETS[net][0]
    sd = R.state_dict(channels)
    rd = H.reads(len(channels))
    m = _model(mode, net, dev, THIN_ALL if form == "thin" else None)
    lens = _batch(m.n_layers, dev)[2]
    plain = mode in H.PLAIN_MODES
    gaps, floors, anchors, layers, bad_bits = {}, {}, {}, [], []
    prev = prev8 = None
    for i in range(1, m.n_layers):
        probs, logits, raw, thin = _forward(m, dev, capfd, i)
        info = m.layer_info()
        li = info[i]
        kernel = _kernel_of(mode, info, i, thin)
        key = STREAM_L1 if plain and i == 1 else kernel
        fmt, cp, C = li["rows_format"], li["cp_out"], li["c_out"]
        U, bases = li["block_samples"], m.block_bases(lens, i)
        assert list(np.diff(bases)) == [n // U + 1 for n in lens]
        P_out, P_in = U >> (i + 1), info[i - 1]["block_samples"] >> i
        bases_in = m.block_bases(lens, i - 1)
        rows = int(bases[-1]) * P_out
        got_all = H.decode_rows(raw, rows, cp, C, fmt, mode)
        layers.append(dict(layer=i, key=kernel, c_in=li["c_in"], c_out=C, f8_in=info[i - 1]["rows_format"] == 2, f8_out=fmt == 2,
                           tile=(li["bm"], li["bn"])))
        # ---- zero bits: the rows behind every read inside its blocks, and the slots of no channel (lo slots and e4m3 bytes too)
        body = raw[:H.row_bytes(rows, cp)].reshape(rows, 2 * cp)
        pad_rows = H.pad_row_mask(lens, bases, P_out, i + 1)
        if body[pad_rows].any():
            bad_bits.append((i, key, "pad rows", int(np.count_nonzero(body[pad_rows]))))
        if body[:, H.pad_slot_mask(fmt, cp, C)].any():
            bad_bits.append((i, key, "pad channel slots", int(np.count_nonzero(body[:, H.pad_slot_mask(fmt, cp, C)]))))
        if fmt == 2:
            # conv_ring_f8.hip:472,489: every block of every row gets the scale bytes (f + 105, f + 94), f the biased f16 exponent
            # of its maximum and at least 1 - a zero block (a pad row, a block behind the last channel) holds (106, 95), a valid
            # scale, never zero bits (:265: an E8M0 byte of 0xff would be a NaN times zero)
            sc = H.decode_f8(raw, rows, cp, C)[3].astype(np.int32)
            blocks = sc.reshape(rows, -1, 2)
            if not np.array_equal(blocks[..., 1], blocks[..., 0] - 11):
                bad_bits.append((i, key, "scale bytes: lo is not hi - 11", 0))
            if not (blocks[pad_rows] == (106, 95)).all():
                bad_bits.append((i, key, "scale bytes of pad rows", 0))
            if (-(-C // 32)) % 2 and not (blocks[:, -1] == (106, 95)).all():
                bad_bits.append((i, key, "scale bytes of the block behind the last channel", 0))
        # ---- float64 from the device's own input
        w32, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        w = H.layer_weights(w32, mode)
        for k, n in enumerate(lens):
            if i == 1:                      # from the fp32 signal row through layer 0 in float64, rounded to the mode's storage
                x0 = rd[k][1].astype(np.float32).astype(np.float64)
                x = H.store(R.layer_f64(x0[None], sd["layers.0.0.weight"], sd["layers.0.0.bias"]), mode)
            else:
                x = prev[bases_in[k] * P_in: bases_in[k] * P_in + (n >> i)].T
            ref = ro.conv_block(x[None], w, b, acc=np.float64)[0].T           # [L_out, C]
            L_out = ref.shape[0]
            assert L_out == n >> (i + 1)
            got = got_all[bases[k] * P_out: bases[k] * P_out + L_out]
            if not (np.isfinite(got).all() and np.isfinite(ref).all()):
                bad_bits.append((i, key, "a value of read %d or of its reference is not finite" % k, int(np.count_nonzero(~np.isfinite(got)))))
            scale = max(1.0, float(np.nanmax(np.abs(ref)))) if np.isfinite(ref).any() else 1.0
            err = np.abs(got - ref)
            err = np.where(np.isfinite(err), err, np.inf)                     # a NaN or inf anywhere is an infinite gap
            if plain:
                gap = max(0.0, float((err - H.ulp16(np.where(np.isfinite(ref), ref, 0.0), mode) / 2).max())) / scale
                floor = float(np.abs(H.round16(ref, mode) - ref).max()) / scale
            else:
                gap = float(err.max()) / scale
                floor = 0.0
                if k in FLOOR_READS:                                          # the arithmetic's own floor, and fp32 numpy's gap
                    if prev8 is not None:                                     # F8 rows in: the cross terms as one e4m3 product
                        r0, r1 = bases_in[k] * P_in, bases_in[k] * P_in + (n >> i)
                        y = H.f8_products(prev8[0][r0:r1].T, prev8[2][r0:r1].T, prev8[1][r0:r1].T, w32, b)
                    else:
                        y = H.three_products(x, w32, b, mode)
                    y = H.f8_store(y) if fmt == 2 else H.store(y, mode)
                    floor = float(np.abs(y.T - ref).max()) / scale
                    ref32 = ro.conv_block(x[None], w, b, acc=np.float32)[0].T
                    anchors[key] = max(anchors.get(key, 0.0), float(np.abs(ref32 - ref).max()) / scale)
            if not np.isfinite(gap):
                gap = float("inf")
            if gap > gaps.get(key, (-1.0,))[0]:
                r, c = np.unravel_index(int(np.argmax(err)), err.shape)
                gaps[key] = (gap, i, k, int(r), int(c))
            floors[key] = max(floors.get(key, 0.0), floor)
        prev = got_all
        prev8 = H.decode_f8(raw, rows, cp, C)[:3] if fmt == 2 else None
    m.close()
    f64 = _f64_forward(channels)
    dl = float((np.abs(logits - f64) / np.maximum(1.0, np.abs(f64))).max())
    dp = float(np.abs(probs - ro.softmax(f64)).max())
    return dict(gaps=gaps, floors=floors, anchors=anchors, layers=layers, bad_bits=bad_bits, logits=dl, probs=dp)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP, ids=["-".join(c).rstrip("-") for c in SWEEP])
def test_each_layer_against_float64_from_the_devices_own_input(dev, capfd, case):
    mode, net, form = case
    t0 = time.time()
    res = _case(case, dev, capfd)
    what = "A" if mode in H.PLAIN_MODES else "max|dev-f64|/scale"
    with capfd.disabled():
        for key in sorted(res["gaps"]):
            g, i, k, r, c = res["gaps"][key]
            print(f"\nH16_LAYERS {mode} {net}{'+' + form if form else ''} {key}: {what} {g:.3e} (layer {i} read {k} row {r} channel {c})  "
                  f"floor {res['floors'][key]:.3e}" + (f"  numpy fp32 {res['anchors'][key]:.3e}" if key in res["anchors"] else "")
                  + f"  bar {_tol(mode, key):.1e}", end="")
        print(f"\nH16_LAYERS {mode} {net}{'+' + form if form else ''} end to end: logits {res['logits']:.3e} probs {res['probs']:.3e}  "
              f"bars {E2E_TOL[mode]['logits']:.1e} {E2E_TOL[mode]['probs']:.1e}  kernels "
              + " ".join(f"{l['layer']}:{l['key']}" for l in res["layers"]) + f"  {time.time() - t0:.1f} s")
    assert not res["bad_bits"], (case, res["bad_bits"])
    for key, (g, *where) in res["gaps"].items():
        assert g < _tol(mode, key), (case, key, g, where)
    assert res["logits"] < E2E_TOL[mode]["logits"] and res["probs"] < E2E_TOL[mode]["probs"], (case, res["logits"], res["probs"])


# ---- the forms
# RS_H16_WRES=0 alone cannot be read back (five of the six weights-resident tiles are ring shapes too), so it comes with a ring
# shape forced onto every layer, 128 x 128, which the weights-resident kernel ignores: "ring_force" is that force alone (the
# weights-resident layers keep their 256 x all-columns tile), "wres_off" the two together (they now report 128 x 128)
FORCED_TILE = (128, 128)
RING_FORCE = {"RS_FORCE_SHAPE_RING": ";".join("%d:4,2,2,4" % i for i in range(1, 12))}
FORMS = {"thin_off": {"RS_THIN_H16_ROWS": "0"}, "thin_all": THIN_ALL, "ring_force": RING_FORCE,
         "wres_off": dict(RING_FORCE, RS_H16_WRES="0"), "no_stream": {"RS_NO_STREAM_H16": "1"}}
FORM_NETS = ("tail", "wide6", "odd5", "narrow3", "f8net")
FORM_CASES = [(mode, net) for mode, net in H.CASES if net in FORM_NETS]
_NO_THIN = "RS_THIN_H16_ROWS acts on split precision only (select_kernel: x3 &&)"
_ALL_STREAM = "every layer of narrow3 runs the streaming kernel: no tiled layer"
# (form, mode, net) a net has no layer for, with the reason.  (RS_NO_STREAM012 is not in rs_layer_info at all: both streaming
# forms report 16 x round_up(c_out, 16) tiles on layers 1 and 2; its bits are checked, its honouring cannot be read back.)
UNREACHABLE = {}
for _net in FORM_NETS:
    for _mode in H.PLAIN_MODES:
        if _mode in H.NETS[_net][2]:
            UNREACHABLE[("thin_off", _mode, _net)] = UNREACHABLE[("thin_all", _mode, _net)] = _NO_THIN
for _mode in H.SPLIT_MODES:
    UNREACHABLE[("thin_off", _mode, "narrow3")] = UNREACHABLE[("thin_all", _mode, "narrow3")] = _ALL_STREAM
for _mode in H.MODES:
    UNREACHABLE[("wres_off", _mode, "narrow3")] = UNREACHABLE[("ring_force", _mode, "narrow3")] = _ALL_STREAM


def _honoured(form, mode, info, kernels, kernels0):
    """the layers on which a force shows in rs_layer_info (kernels0: the default form's classes)"""
    layers = range(1, len(info))
    if form == "thin_all":
        return [i for i in layers if kernels[i] == "thin"]
    if form == "thin_off":                                                    # tiled split-precision layers, none of them thin
        assert "thin" not in kernels.values()
        return [i for i in layers if mode in H.SPLIT_MODES and kernels[i] in ("ring", "ring_tail", "wres")]
    tile = {i: (info[i]["bm"], info[i]["bn"]) for i in layers}
    if form == "ring_force":            # the ring kernels take the forced tile; the weights-resident kernel keeps its own
        assert all(tile[i] == (256, 16 * ((info[i]["c_out"] + 15) // 16)) for i in layers if kernels0[i] == "wres")
        return [i for i in layers if kernels0[i] == "wres" or (kernels[i] in ("ring", "ring_tail", "f8") and tile[i] == FORCED_TILE)]
    if form == "wres_off":              # the layers the weights-resident kernel ran now report the forced ring tile
        return [i for i in layers if kernels0[i] == "wres" and tile[i] == FORCED_TILE]
    return [i for i in layers if kernels0[i] == "stream" and kernels[i] != "stream" and info[i]["bm"] != 16]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,net", FORM_CASES)
def test_every_form_keeps_the_bits(dev, capfd, mode, net):
    n = len(H.NETS[net][0])

    def run(env, raw_reads=False, layers=None):
        m = _model(mode, net, dev, env)
        out, kernels = {}, {}
        for i in (layers if layers is not None else range(1, n)):
            probs, logits, raw, thin = _forward(m, dev, capfd, i, raw_reads)
            out[i] = raw
            if layers is None:
                kernels[i] = _kernel_of(mode, m.layer_info(), i, thin, wres_on=env.get("RS_H16_WRES") != "0")
        if not out:
            probs, logits, _, _ = _forward(m, dev, capfd, None, raw_reads)
        info = m.layer_info()
        m.close()
        return out, logits, info, kernels

    want, logits0, info0, kernels0 = run({})
    assert np.isfinite(logits0).all()
    for form, env in FORMS.items():
        got, logits, info, kernels = run(env)
        for i in want:
            assert np.array_equal(got[i], want[i]), (mode, net, form, "layer %d" % i)
        assert np.array_equal(logits, logits0), (mode, net, form)
        hon = _honoured(form, mode, info, kernels, kernels0)
        why = UNREACHABLE.get((form, mode, net))
        assert bool(hon) == (why is None), (mode, net, form, hon, why, kernels0, kernels)
    # the int16 reads through classify_raw: one launch for layers 0 + 1 + 2 (not taken while layer 1 or 2 is captured: layer 3;
    # narrow3 has no layer 3: its logits alone), two launches, and the tiled kernels
    layers = [3] if n > 3 else []
    for env in ({}, {"RS_NO_STREAM012": "1"}, {"RS_NO_STREAM_H16": "1"}):
        got, logits, _, _ = run(env, raw_reads=True, layers=layers)
        for i in layers:
            assert np.array_equal(got[i], want[i]), (mode, net, env, "classify_raw, layer %d" % i)
        assert np.array_equal(logits, logits0), (mode, net, env, "classify_raw")


def test_the_unreachable_table_names_real_cases():
    for (form, mode, net), why in UNREACHABLE.items():
        assert form in FORMS and (mode, net) in FORM_CASES and why


# ---- coverage
@pytest.mark.gpu
def test_the_sweep_covers_the_kernels_and_the_channel_edges(dev, capfd):
    ran = []                                                                  # (mode, layer record) over all cases
    for case in SWEEP:
        ran += [(case[0], l) for l in _case(case, dev, capfd)["layers"]]
    for key in H.KEYS:
        assert {m for m, l in ran if l["key"] == key} == set(H.KEY_MODES[key]), key
    split = [l for m, l in ran if m in H.SPLIT_MODES and l["key"] in ("ring", "ring_tail", "thin", "wres")]
    assert {l["c_in"] % 32 for l in split} >= {0, 1, 8, 9}
    tails = [l for l in split if H.ring_tail("f16x3", l["c_in"])]
    assert {l["key"] for l in tails} == {"ring_tail", "thin"}                  # both kernels that read the merged packing
    assert {(l["c_in"] + 31) // 32 for l in tails if l["key"] == "ring_tail"} == {3, 4, 5}       # conv_ring_h16.hip: TAIL
    assert {(l["c_in"] + 31) // 32 for l in tails if l["key"] == "thin"} == {3, 4, 5}            # conv_thin_h16.hip
    assert any(l["c_in"] % 32 <= 8 and l["c_in"] % 32 and (l["c_in"] + 31) // 32 == 2 for l in split if l not in tails)
    f8 = [l for m, l in ran if l["key"] == "f8" and l["c_in"] % 64 and l["c_out"] % 64]
    assert any(not l["f8_in"] and l["f8_out"] for l in f8), "first layer of a run"
    assert any(l["f8_in"] and l["f8_out"] for l in f8), "interior layer of a run"
    assert any(l["f8_in"] and not l["f8_out"] for l in f8), "last layer of a run"
