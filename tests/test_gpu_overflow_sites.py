"""The half-precision overflow flag (rs_model_saturated, Model.saturated()), held to the rows each of its seven sites stores.

The f16 / f16x3 / f16xf8 modes store activations as IEEE half; a value of 65520 or more becomes +inf and a later layer can turn it
into an ordinary-looking number.  Seven hand-written epilogues raise the model's sticky flag (DESIGN.md section 1 lists them).
Here every one of them is the LAST conv layer of a short net of the shipped class, so nothing downstream can repeat the flag, and
the oracle is the device's own output buffer (rs_debug_capture_layer), no tolerance involved:

  must raise       the captured output of the layer under test holds a non-finite hi half  ->  saturated() is True
  must stay quiet  its largest captured hi half, and that of every earlier layer, is below 65504 / 2  ->  saturated() is False

The last layer's weights and bias carry one power of two (the whole layer, or ONE output channel), chosen from a capture of the
unscaled net.  The input steers the overflow: quiet rows (0.05 x noise) with one loud window (3 x noise, 8 input rows of the
layer under test wide) at a chosen place.  rs_forward cases scale the window by powers of two up to the first capture with a
non-finite half ("raise") and back down to one below 65504 / 2 ("quiet") on ONE model.  rs_classify normalises every read itself
(median / MAD, values beyond 3.5 smoothed away), which fixes the window at about 2.6 x the background whatever its amplitude -
less than the factor 4 one power of two needs to put the window beyond 65520 and the background below 65504 / 2 - so those cases
keep ONE input and load the weights at two powers of two, one per side; their quiet rows are uniform noise of the same standard
deviation (a Gaussian's own tail reaches the +-3.5 the window is clipped to).  Before a "raise" is trusted every earlier
layer is captured on the same input and must be finite and 8 x below the limit, and every non-finite half must sit in the rows
(and, for one scaled channel, the channel) the window steers to: a window that failed to steer is a bug of this test.

Sites 2-6 test the packed word before the row mask, site 7 behind it.  The contract is on what is STORED, so a value that is
computed and masked off must not raise the flag; the windows at a read's end (an odd read's last rows, its dropped last input
row alone) are where it would.  No case shows it, so neither order is changed.

The 0 + 1 + 2 streaming launch (site 3) never writes layer 1's output and is not taken while layer 1 or 2 is captured: its
captures come from the same model in the two-launch form, which test_h16_streaming_layers_and_layer0_fold holds bit-identical;
the flag is then read behind a call without capture, which runs the one launch.

Every case prints an OVERFLOW_SITE line per window (pytest -s): site, mode, net, kernel tile, amplitude or scale, first inf."""
import contextlib
import math

import numpy as np
import pytest

from tests import overflow_ref as R

HALF_MAX = R.HALF_MAX
QUIET_BOUND = HALF_MAX / 2          # "must stay quiet" premise
EARLIER_BOUND = HALF_MAX / 8        # earlier layers on a raising input
# weight seeds (synth.make_state_dict): ReLU leaves some output channels of a random layer dead (never positive), and a dead
# channel cannot overflow whatever its scale; these seeds keep every channel channel_picks names alive in the layer under test
SEEDS = {(20, 30, 40): 1}
SEED = 11
NOISE_SEED = 3
NOISE_TRIES = 6                     # rs_classify cases: noise seeds tried per window until the unscaled capture can be steered

# (site, mode) pairs the issue's table asks for; test_every_site_and_mode_was_reached compares what ran with this
WANT = {(s, m) for s in (1, 2, 3, 4, 5) for m in ("f16", "f16x3")} | {(6, "f16x3"), (7, "f16xf8")}

_RING, _THIN_OFF = "RS_FORCE_SHAPE_RING", {"RS_THIN_H16_ROWS": "0"}
# id -> site, mode, channels, entry ("forward": rs_forward on fp32 rows, "raw": rs_classify on int16 reads), the layer under test,
# hooks, whether models with ONE scaled channel run as well
CASES = {}


def _case(cid, site, mode, channels, entry, layer, env=None, per_channel=False, **kw):
    CASES[cid] = dict(site=site, mode=mode, channels=tuple(channels), entry=entry, layer=layer, env=dict(env or {}),
                      per_channel=per_channel, **kw)


for _m in ("f16", "f16x3"):
    _case(f"site1-conv0-{_m}", 1, _m, (40, 24), "forward", 0, per_channel=True)
    _case(f"site2-layer1-{_m}", 2, _m, (20, 24), "forward", 1, per_channel=True)
    _case(f"site2-layer2-{_m}", 2, _m, (20, 30, 40), "forward", 2)
    _case(f"site2-folded-{_m}", 2, _m, (20, 24), "raw", 1)
    _case(f"site3-stream012-{_m}", 3, _m, (20, 30, 40), "raw", 2, per_channel=True)
    # the ring force names another tile than the weights-resident kernel's 256 x 48: that kernel ignores it, the ring kernel would not
    _case(f"site4-wres-{_m}", 4, _m, (20, 30, 40, 40), "forward", 3, dict(_THIN_OFF, **{_RING: "3:4,2,1,1"}), per_channel=True,
          tile=(256, 48))
    # 64 x 32 tiles on 40 channels: two tiles along the channels, the second partial
    _case(f"site5-ring-{_m}", 5, _m, (20, 30, 40, 40), "forward", 3, dict(_THIN_OFF, RS_H16_WRES="0", **{_RING: "3:4,2,1,1"}),
          per_channel=True, tile=(64, 32))
# split precision, merged tail panel (c_in % 32 in 1..8 behind 2-4 full panels) and the same packing un-merged
for _c, _kp in ((67, (7 * 32, 9 * 32)), (100, (10 * 32, 12 * 32))):
    _case(f"site5-tail{_c}-f16x3", 5, "f16x3", (20, 30, _c, 40), "forward", 3,
          dict(_THIN_OFF, RS_H16_WRES="0", **{_RING: "3:4,2,2,4"}), tile=(128, 128), k_pad=_kp[0])
    _case(f"site5-tail{_c}-unmerged-f16x3", 5, "f16x3", (20, 30, _c, 40), "forward", 3,
          dict(_THIN_OFF, RS_H16_WRES="0", RS_X3_TAIL="0", **{_RING: "3:4,2,2,4"}), tile=(128, 128), k_pad=_kp[1])
# the ring force names 128 x 128: a 64 x 32 tile is then the thin kernel's, not the ring table's own 64 x 32
_case("site6-thin-f16x3", 6, "f16x3", (20, 30, 40, 40), "forward", 3, {"RS_THIN_H16_ROWS": "100000000", _RING: "3:4,2,2,4"},
      per_channel=True, tile=(64, 32))
# RS_F8_MIN_CIN=64: layer 3 writes F8 rows, layer 4 reads them and writes half rows - the end of the run, isolated
_case("site7-f8-last-f16xf8", 7, "f16xf8", (20, 30, 64, 64, 40), "forward", 4, dict(_THIN_OFF, RS_F8_MIN_CIN="64"), per_channel=True)
# ... and the layer that WRITES F8 rows (premise from its own format-2 capture).  NOT isolated: layer 4 reads the inf and raises too
_case("site7-f8-rows-f16xf8", 7, "f16xf8", (20, 30, 64, 64, 40), "forward", 3, dict(_THIN_OFF, RS_F8_MIN_CIN="64"), raise_only=True)


# =====================================================================================================================
# CPU tests of the helpers
# =====================================================================================================================
def _half_bits(v):
    return np.asarray(v, dtype=np.float16).view(np.uint16)


def test_decoder_reads_the_hi_halves_of_every_row_format():
    """hand-built buffers: a non-finite hi half is found at its (read, row, channel); non-finite patterns in the lo halves, the
    e4m3 bytes and the pad slots behind the last channel are ignored"""
    inf, one = 0x7C00, int(_half_bits(1.0))
    bases, rpb = np.array([0, 2, 3]), 4                  # read 0: rows 0-7, read 1: rows 8-11
    # format 0: 40 channels in 48 slots
    b = np.full((12, 48), one, dtype=np.uint16)
    b[:, 40:] = 0xFFFF                                    # pad slots: ignored
    b[9, 39] = inf
    hi = R.decode_hi(b.reshape(-1), 0, 48, 40)
    assert hi.shape == (12, 40) and R.locate(hi, bases, rpb) == [(1, 1, 39)] and R.finite_max(hi) == 1.0
    # format 1: [hi x 32 | lo x 32] per panel, 40 channels = 2 panels
    b = np.full((12, 128), one, dtype=np.uint16)
    b[:, 32:64] = 0x7E00                                  # lo halves of panel 0 (NaN): ignored
    b[:, 96:] = 0xFC00                                    # lo halves of panel 1: ignored
    b[:, 64 + 8:96] = 0x7C00                              # hi slots of panel 1 behind channel 39: pad, ignored
    b[3, 5], b[3, 64 + 7], b[8, 64] = inf, 0x7C01, inf    # channels 5, 39 (a NaN) and 32
    hi = R.decode_hi(b.reshape(-1), 1, 128, 40)
    assert R.locate(hi, bases, rpb) == [(0, 3, 5), (0, 3, 39), (1, 0, 32)]
    # format 2: [hi16 x 64 | 64 slots of e4m3 bytes] per 64 channels, 70 channels = 2 groups
    b = np.full((12, 256), one, dtype=np.uint16)
    b[:, 64:128] = 0x7C7C
    b[:, 192:] = 0xFFFF                                   # e4m3 bytes: ignored
    b[:, 128 + 6:192] = inf                               # hi slots behind channel 69: ignored
    b[11, 63], b[0, 128 + 5] = inf, inf                   # channels 63 and 69
    hi = R.decode_hi(b.reshape(-1), 2, 256, 70)
    assert R.locate(hi, bases, rpb) == [(0, 0, 69), (1, 3, 63)]
    b[:] = int(_half_bits(30000.0))
    assert R.finite_max(R.decode_hi(b.reshape(-1), 2, 256, 70)) == 30000.0 and not R.nonfinite(R.decode_hi(b, 2, 256, 70)).any()


def test_the_devices_bit_test_mirrored():
    """(packed + 0x04000400) & 0x80008000 (csrc/common.hpp: f16_overflow_bits) over all 2^15 non-negative halves, in either half of
    the word: non-zero exactly for exponent field 31 (inf and NaN), the hit stays in its own half, and the low half never carries
    into the high one.  The test is only valid behind the ReLU, where the epilogues apply it: a half with its sign bit set trips it
    whatever its value (all negative finite halves and -0 do), except that -inf and negative NaNs in the LOW half (0xfc00 on)
    carry out of it - into the high half - and leave both bits clear."""
    h = np.arange(1 << 15, dtype=np.uint32)
    special = (h & R.EXP_MASK) == R.EXP_MASK
    assert special.sum() == 1024 and not special[int(_half_bits(65504.0))] and special[0x7C00]
    low, high = R.overflow_bits(h), R.overflow_bits(h << 16)
    assert np.array_equal(low != 0, special) and np.array_equal(high != 0, special)
    assert not (low & 0x80000000).any() and not (high & 0x8000).any()
    # next to the largest finite half in the other half of the word: still no carry, still its own bit only
    big = np.uint32(0x7BFF)
    assert np.array_equal(R.overflow_bits(h | (big << 16)) != 0, special)
    assert np.array_equal(R.overflow_bits((h << 16) | big) != 0, special)
    assert not (R.overflow_bits(h | (big << 16)) & 0x80000000).any()
    # sign bit set: negative finite halves (and -0) always trip it ...
    neg = np.arange(0x8000, 0xFC00, dtype=np.uint32)
    assert (R.overflow_bits(neg) == 0x8000).all() and (R.overflow_bits(neg << 16) == 0x80000000).all()
    # ... -inf / negative NaN do not: adding 0x0400 carries out of their half (from the low half into the high one) and clears
    # both bits - one more reason the epilogues test behind the ReLU only
    ninf = np.arange(0xFC00, 0x10000, dtype=np.uint32)
    assert (R.overflow_bits(ninf) == 0).all() and (R.overflow_bits(ninf << 16) == 0).all()


def test_window_builder():
    """the loud rows are where asked, everything else is quiet, NaN sits behind each read; the int16 form holds the same window"""
    lens = [300, 64, 177]
    base = R.noise(5, lens)
    s0, s1 = R.window_samples(2, 5, lens[2])
    assert (s0, s1) == (20, 52)
    assert R.window_samples(3, 20, 177) == (160, 177) and R.window_samples(3, -6, 16) == (0, 16)      # cut to the read
    x = R.float_batch(base, lens, 2, s0, s1, 4.0)
    assert x.shape == (3, 300 + R.PAD) and x.dtype == np.float32
    for b, n in enumerate(lens):
        assert np.isnan(x[b, n:]).all() and np.isfinite(x[b, :n]).all()
        loud = np.zeros(n, dtype=bool)
        if b == 2:
            loud[s0:s1] = True
        assert np.abs(x[b, :n][~loud]).max() < 0.05 * 6
        assert np.array_equal(x[b, :n][~loud], (0.05 * base[0][b][~loud]).astype(np.float32))
    assert np.array_equal(x[2, s0:s1], (4.0 * 3.0 * base[1][2][s0:s1]).astype(np.float32))
    assert np.abs(x[2, s0:s1]).std() > 10 * 0.05
    ubase = R.noise(5, lens, uniform=True)
    assert all(np.abs(q).max() <= math.sqrt(3) and abs(q.std() - 1) < 0.15 for q in ubase[0])
    reads = R.int16_reads(ubase, lens, 2, s0, s1, 1.0)
    assert [r.shape[0] for r in reads] == lens and all(r.dtype == np.int16 for r in reads)
    assert np.abs(reads[2][s0:s1]).max() > 20 * np.abs(np.delete(reads[2], np.s_[s0:s1])).max()
    assert all(np.abs(reads[b]).max() <= round(0.05 * math.sqrt(3) * 400) for b in (0, 1))
    assert R.covered_rows(0) == (-1, 4) and R.covered_rows(16) == (7, 12)
    assert R.channel_picks(40) == [0, 1, 38, 39, 22, 27] and R.channel_picks(24) == [0, 1, 22, 23]
    assert len(R.channel_picks(136)) == 12 and all(0 <= n < 136 for n in R.channel_picks(136))


# =====================================================================================================================
# GPU: one rig per case
# =====================================================================================================================
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _pow2_below(x: float) -> float:
    """largest power of two <= x"""
    return 2.0 ** math.floor(math.log2(x))


class Rig:
    """the nets, models and batches of one case, and the contract checks on them"""

    def __init__(self, cid, dev):
        from riser_amd import synth
        self.cid, self.dev = cid, dev
        self.__dict__.update(CASES[cid])
        self.n = len(self.channels)
        self.cfg = synth.Config(synth.CnnConfig(channels=list(self.channels), kernels=[3] * self.n))
        self.sd = synth.make_state_dict(SEEDS.get(self.channels, SEED), channels=self.channels)
        self.c_out = self.channels[self.layer]
        self.models = {}
        self.log = []
        # 9 reads between 2^n and 8615 samples; read 2 has an odd row count in every layer (all low bits set) with 3 mod 4 rows
        # entering the layer under test (the dropped last input row exists, and the row count behind the pool is odd too)
        i = self.layer
        rows_odd = ((5000 >> i) & ~3) | 3
        self.lens = [8615, 4097, ((rows_odd + 1) << i) - 1, 7777, 8191, 4096, (1 << self.n) + 1, 5000, 6023]
        self.lens_min = [1 << self.n]
        self._noise = {}
        self.noise, self.noise_min = self.noise_of(self.lens, 0), self.noise_of(self.lens_min, 0)

    def noise_of(self, lens, k):
        key = (len(lens), k)
        if key not in self._noise:
            self._noise[key] = R.noise(NOISE_SEED + 100 * k + len(lens), lens, uniform=self.entry == "raw")
        return self._noise[key]

    # ---- models -----------------------------------------------------------------------------------------------------
    def model(self, scale=1.0, channel=None):
        key = (float(scale), channel)
        if key not in self.models:
            from conftest import hooked_model
            sd = dict(self.sd)
            if scale != 1.0:
                w, b = (sd[f"layers.{self.layer}.0.{k}"].copy() for k in ("weight", "bias"))
                sel = slice(None) if channel is None else channel
                w[sel] *= np.float32(scale)
                b[sel] *= np.float32(scale)
                sd[f"layers.{self.layer}.0.weight"], sd[f"layers.{self.layer}.0.bias"] = w, b
                if self.layer + 1 < self.n and not self.__dict__.get("raise_only"):
                    # site 1 (layer 0 cannot be last): the next layer's weights on the scaled channels by 1 / scale, so that its own output keeps
                    # the size it has on the unscaled net (ReLU nets are positively homogeneous) and cannot overflow first
                    w1 = sd[f"layers.{self.layer + 1}.0.weight"].copy()
                    w1[:, sel] /= np.float32(scale)
                    sd[f"layers.{self.layer + 1}.0.weight"] = w1
            env = dict(self.env, RS_RANGE_CHECK="0")
            self.models[key] = hooked_model(env, sd, self.mode, self.dev, target=self.cid, config=self.cfg)
        return self.models[key]

    def close(self):
        for m in self.models.values():
            m.close()
        self.models = {}

    # ---- one library call -------------------------------------------------------------------------------------------
    def batch(self, lens, base, read, s0, s1, amplitude):
        import torch
        if self.entry == "forward":
            x = torch.from_numpy(R.float_batch(base, lens, read, s0, s1, amplitude)).to(self.dev)
            return ("forward", x, np.asarray(lens, dtype=np.int32))
        from riser_amd.preprocess import pack_reads
        return ("raw",) + pack_reads(R.int16_reads(base, lens, read, s0, s1, amplitude), self.dev)

    def run(self, m, batch, layer=None):
        """one call of the entry point under test -> (decoded hi halves of `layer`'s output or None, saturated())"""
        import torch
        lens = batch[2] if batch[0] == "forward" else batch[4]
        cap = None
        if layer is not None:
            rows, cp, fmt = m.layer_rows(lens, layer)
            cap = torch.zeros(rows * cp, dtype=torch.int16, device=self.dev)
        with m.capture_layer(layer, cap) if layer is not None else contextlib.nullcontext():
            if batch[0] == "forward":
                probs = m.forward_batch(batch[1], lens)
            else:
                probs = m.classify_raw(batch[1], batch[2], batch[3], lens)
        assert tuple(probs.shape) == (len(lens), 2)
        sat = m.saturated()
        assert not m.saturated()                                        # cleared by the read
        if cap is None:
            return None, sat
        return R.decode_hi(cap.cpu().numpy(), fmt, cp, m.channels[layer]), sat

    def layer0_oracle(self, m_key, lens, base, read, s0, s1, amplitude):
        """layer 0's output in fp32 (oracle.riser_oracle.conv_block) on the rows of a float batch, per read [C, L // 2]"""
        from oracle import riser_oracle as ro
        scale, channel = m_key
        w, b = self.sd["layers.0.0.weight"].copy(), self.sd["layers.0.0.bias"].copy()
        if self.layer == 0 and scale != 1.0:
            sel = slice(None) if channel is None else channel
            w[sel] *= np.float32(scale)
            b[sel] *= np.float32(scale)
        x = R.float_batch(base, lens, read, s0, s1, amplitude)
        return [ro.conv_block(x[k, : lens[k]][None, None, :], w, b, acc=np.float32)[0] for k in range(len(lens))]

    # ---- which kernel ran -------------------------------------------------------------------------------------------
    def confirm_kernel(self, m):
        """from rs_model_layer_info after a call without capture: the site's kernel ran the layer under test"""
        info = m.layer_info()
        li = info[self.layer]
        tile = (li["bm"], li["bn"])
        if self.site == 1:
            assert self.entry == "forward" and self.layer == 0        # rs_forward: layer 0 is its own launch (nothing folds it)
        elif self.site == 2:
            assert self.layer in (1, 2) and tile == (16, 16 * ((self.c_out + 15) // 16)), tile
            assert self.entry == "forward" or self.n == 2              # folded: rs_classify on a 2-layer net (no 0 + 1 + 2 launch)
        elif self.site == 3:
            # the one launch is taken on rs_classify for > 2 layers, c0 <= 32, 16 < c1 <= 32, c2 <= 48, both layers streaming
            assert self.entry == "raw" and self.n > 2 and self.layer == 2 and self.channels[0] <= 32
            assert 16 < self.channels[1] <= 32 and self.channels[2] <= 48 and "RS_NO_STREAM012" not in self.env
            assert all((info[k]["bm"], info[k]["bn"]) == (16, 16 * ((self.channels[k] + 15) // 16)) for k in (1, 2)), info
            assert (info[1]["block_samples"] >> 2) % 32 == 0
        elif self.site in (4, 5, 6):
            assert self.layer >= 3 and tile == self.tile, (tile, self.tile)
            if "k_pad" in self.__dict__:
                assert li["k_pad"] == self.k_pad, li
        elif self.site == 7:
            assert self.mode == "f16xf8" and info[2]["rows_format"] == 1 and info[3]["rows_format"] == 2 and info[4]["rows_format"] == 1
            assert tile[0] > 0
        return tile

    # ---- the contract on one window ---------------------------------------------------------------------------------
    def check_side(self, m, m_key, side, pos, batch, geom, amplitude, channel=None):
        """`side` "raise" or "quiet" on model m: premises from the captures (layer 0: the fp32 oracle), then the flag - behind
        the capturing calls and behind a call without capture"""
        lens, base, read, s0, s1, row0 = geom
        hi, sat = self.run(m, batch, self.layer) if self.layer else (None, self.run(m, batch)[1])
        flags = [sat]
        first = None
        if self.entry == "forward":
            l0 = self.layer0_oracle(m_key, lens, base, read, s0, s1, amplitude)
            l0max = max(float(v.max()) for v in l0)
        else:
            l0max = 0.0            # rs_classify: |normalised input| <= 3.5 but for a read's first and last sample; layer 0 is O(10)
        lo, hi_row = R.covered_rows(row0)
        if side == "raise":
            if self.layer == 0:
                assert l0max >= 2 * 65520.0, (self.cid, pos, l0max)
                where = [(k, int(r), int(c)) for k, v in enumerate(l0) for c, r in zip(*np.nonzero(v >= 65520.0))]
            else:
                assert l0max < EARLIER_BOUND, (self.cid, pos, l0max)
                where = R.locate(hi, m.block_bases(batch_lens(batch), self.layer), self.rows_per_block(m))
                assert where, (self.cid, pos, "no non-finite half in the capture")
            for (b, r, c) in where:                                     # the window steered the overflow
                assert b == read and lo <= r <= hi_row and r < lens[read] >> (self.layer + 1), (self.cid, pos, (b, r, c), (lo, hi_row))
                assert channel is None or c == channel, (self.cid, pos, (b, r, c), channel)
            first = where[0]
            for j in range(1, self.layer):                              # nothing upstream did the raising
                hj, sj = self.run(m, batch, j)
                assert not R.nonfinite(hj).any() and R.finite_max(hj) < EARLIER_BOUND, (self.cid, pos, j, R.finite_max(hj))
                flags.append(sj)
            flags.append(self.run(m, batch)[1])
            assert all(flags), f"{self.cid} {pos}: the layer's output overflowed and saturated() stayed False {flags}"
        else:
            peak = l0max if self.layer == 0 else R.finite_max(hi)
            assert self.layer == 0 or not R.nonfinite(hi).any()
            assert peak < QUIET_BOUND and l0max < QUIET_BOUND, (self.cid, pos, peak, l0max)
            for j in range(1, self.n if self.layer == 0 else self.layer):
                hj, sj = self.run(m, batch, j)
                assert not R.nonfinite(hj).any() and R.finite_max(hj) < QUIET_BOUND, (self.cid, pos, j, R.finite_max(hj))
                flags.append(sj)
            flags.append(self.run(m, batch)[1])
            assert not any(flags), (f"{self.cid} {pos}: nothing stored reaches {QUIET_BOUND:g} (largest {peak:.6g}) and "
                                    f"saturated() is True {flags}")
            first = peak
        return first

    def rows_per_block(self, m):
        return m.layer_info()[self.layer]["block_samples"] >> (self.layer + 1)

    def window_max(self, hi, m, lens, read, row0, channel=None):
        """(largest finite half inside the rows the window covers, largest outside them) of a decoded capture"""
        start = int(m.block_bases(lens, self.layer)[read]) * self.rows_per_block(m)
        lo, hi_row = R.covered_rows(row0)
        lo, hi_row = max(lo, 0), min(hi_row, (lens[read] >> (self.layer + 1)) - 1)
        v = hi.view(np.float16).astype(np.float32)
        if channel is not None:
            v = v[:, channel:channel + 1]
        inside = np.zeros(v.shape[0], dtype=bool)
        inside[start + lo:start + hi_row + 1] = True
        return float(v[inside].max()), float(v[~inside].max()) if (~inside).any() else 0.0

    def positions(self, tile_rows):
        """name -> (lens, noise, read, first input row of the window)"""
        i = self.layer
        rows = lambda k: self.lens[k] >> i                                                   # noqa: E731
        pos = {"first-row": (self.lens, self.noise, 0, 0),
               "odd-read-last-row": (self.lens, self.noise, 2, rows(2) - R.WINDOW_ROWS),
               "batch-last-row": (self.lens, self.noise, 8, rows(8) - R.WINDOW_ROWS),
               # only the odd read's dropped last input row is loud: the last stored row sees it through one tap, the row
               # behind the read's end - computed, then masked off - through two
               "dropped-odd-row": (self.lens, self.noise, 2, rows(2) - 1),
               "min-length-alone": (self.lens_min, self.noise_min, 0, 0),
               "below-tile-edge": (self.lens, self.noise, 0, tile_rows - R.WINDOW_ROWS),
               "above-tile-edge": (self.lens, self.noise, 0, tile_rows)}
        if self.entry == "raw":
            del pos["dropped-odd-row"]          # one row of samples clipped to +-3.5 cannot be singled out of a normalised read
        assert rows(2) % 4 == 3 and tile_rows + R.WINDOW_ROWS <= rows(0)
        return pos

    # ---- a window on the rs_forward path: one model, the amplitude walks ----------------------------------------------
    def forward_window(self, pos, geom, scale, channel=None):
        lens, base, read, row0 = geom
        s0, s1 = R.window_samples(self.layer, row0, lens[read])
        g = (lens, base, read, s0, s1, row0)
        m, key = self.model(scale, channel), (float(scale), channel)
        seen = {}

        def peak(a):                                    # (any non-finite, largest finite) of the layer under test at amplitude a
            if a not in seen:
                if self.layer == 0:
                    v = max(float(x.max()) for x in self.layer0_oracle(key, lens, base, read, s0, s1, a))
                    seen[a] = (v >= 2 * 65520.0, v)
                else:
                    h, _ = self.run(m, self.batch(lens, base, read, s0, s1, a), self.layer)
                    seen[a] = (bool(R.nonfinite(h).any()), R.finite_max(h))
            return seen[a]
        a = 1.0
        while peak(a)[0] and a > 2.0 ** -10:
            a /= 2
        while not peak(a)[0]:
            a *= 2
            assert a <= 2.0 ** 12, (self.cid, pos, "no overflow up to amplitude 4096", seen)
        q = a / 2
        while peak(q)[0] or peak(q)[1] >= QUIET_BOUND:
            q /= 2
            assert q > 2.0 ** -14, (self.cid, pos, seen)
        first = self.check_side(m, key, "raise", pos, self.batch(lens, base, read, s0, s1, a), g, a, channel)
        qmax = self.check_side(m, key, "quiet", pos, self.batch(lens, base, read, s0, s1, q), g, q, channel)
        self.note(pos, m, channel, f"scale 2^{int(math.log2(scale))} raise-amplitude {a:g} first-inf(read,row,ch) {first} "
                                   f"quiet-amplitude {q:g} quiet-max {qmax:.6g}")

    # ---- a window on the rs_classify path: one input, two scales -----------------------------------------------------
    def raw_steerable(self, geom, channel=None):
        """-> (geometry with the first noise seed, capture, raise scale, quiet scale) for which the UNSCALED capture shows a power
        of two that puts the window (of channel `channel`) beyond 65520 and every other row below it, or None.  Scaling the layer
        by a power of two is exact, and a captured half is within 2^-11 of the fp32 value it was rounded from."""
        lens, _, read, row0 = geom
        s0, s1 = R.window_samples(self.layer, row0, lens[read])
        m1 = self.model()
        for k in range(NOISE_TRIES):
            base = self.noise_of(lens, k)
            hi1, sat = self.run(m1, self.batch(lens, base, read, s0, s1, 1.0), self.layer)
            assert not sat and not R.nonfinite(hi1).any(), (self.cid, "the unscaled net raised the flag")
            inside, outside = self.window_max(hi1, m1, lens, read, row0, channel)
            everyone = self.window_max(hi1, m1, lens, read, row0)[0]
            if inside * 64 < everyone or inside <= 0:
                continue                                                    # the channel is (nearly) dead in this window
            up = 2.0 ** math.ceil(math.log2(65520.0 * 1.002 / inside))
            if up * outside < 65520.0 * 0.998:
                down = _pow2_below(QUIET_BOUND * 0.998 / max(inside, outside))
                return (lens, base, read, s0, s1, row0), up, down
        return None

    def raw_window(self, pos, steer, channel=None):
        g, up, down = steer
        lens, base, read, s0, s1, row0 = g
        batch = self.batch(lens, base, read, s0, s1, 1.0)
        first = self.check_side(self.model(up, channel), (up, channel), "raise", pos, batch, g, 1.0, channel)
        qmax = self.check_side(self.model(down, channel), (down, channel), "quiet", pos, batch, g, 1.0, channel)
        self.note(pos, self.model(up, channel), channel, f"raise-scale 2^{int(math.log2(up))} first-inf(read,row,ch) {first} "
                                                         f"quiet-scale 2^{int(math.log2(down))} quiet-max {qmax:.6g}")

    def note(self, pos, m, channel, text):
        li = m.layer_info()[self.layer]
        line = (f"OVERFLOW_SITE site {self.site} mode {self.mode} case {self.cid} net {'-'.join(map(str, self.channels))} "
                f"layer {self.layer} entry {self.entry} tile {li['bm']}x{li['bn']} rows_format {li['rows_format']} window {pos} "
                f"channel {'all' if channel is None else channel} {text}")
        self.log.append(line)
        print(line)

    # ---- the case ---------------------------------------------------------------------------------------------------
    def go(self):
        m1 = self.model()
        # the calibrated, unscaled net on the first window: the flag stays clear (NaN behind every fp32 row), and the capture
        # sets the layer's power of two
        lens, base = self.lens, self.noise
        s0, s1 = R.window_samples(self.layer, 0, lens[0])
        b1 = self.batch(lens, base, 0, s0, s1, 1.0)
        _, sat = self.run(m1, b1)
        assert not sat, (self.cid, "the unscaled net raised the flag")
        tile = self.confirm_kernel(m1)
        if self.site == 1:
            tile_rows = m1.layer_info()[0]["block_samples"]                # layer 0: a block edge of the packed layout instead
        else:
            tile_rows = tile[0]
        positions = self.positions(tile_rows)
        order = ("odd-read-last-row", "above-tile-edge", "batch-last-row", "first-row", "below-tile-edge")
        if self.entry == "raw":
            for pos, geom in positions.items():
                steer = self.raw_steerable(geom)
                assert steer is not None, (self.cid, pos, "no noise seed lets a power of two single out the window (test bug)")
                self.raw_window(pos, steer)
            for n in R.channel_picks(self.c_out) if self.per_channel else ():
                for pos in order:                                           # the first window that can be steered, in a fixed order
                    steer = self.raw_steerable(positions[pos], n)
                    if steer is not None:
                        break
                assert steer is not None, (self.cid, n, "channel is dead in every window (test bug)")
                self.raw_window(pos, steer, channel=n)
            self.confirm_kernel(m1)
            return (self.site, self.mode)
        caps = {}
        for pos, (ln, bs, read, row0) in positions.items():             # scale-1 captures of every window
            w0, w1 = R.window_samples(self.layer, row0, ln[read])
            if self.layer == 0:
                caps[pos] = self.layer0_oracle((1.0, None), ln, bs, read, w0, w1, 1.0)
                continue
            caps[pos], sat = self.run(m1, self.batch(ln, bs, read, w0, w1, 1.0), self.layer)
            assert not sat and not R.nonfinite(caps[pos]).any(), (self.cid, pos, "the unscaled net raised the flag")
            for j in range(1, self.layer):
                hj, sj = self.run(m1, self.batch(ln, bs, read, w0, w1, 1.0), j)
                assert not sj and R.finite_max(hj) < EARLIER_BOUND / 8, (self.cid, pos, j)
        if self.layer == 0:
            top = max(float(v.max()) for v in caps["first-row"])
        else:
            top = R.finite_max(caps["first-row"])
        scale = _pow2_below(HALF_MAX / 4 / top)                           # the whole layer: a quarter of the range at amplitude 1
        for pos, geom in positions.items():
            if self.__dict__.get("raise_only"):
                self.raise_only_window(pos, geom, scale)
            else:
                self.forward_window(pos, geom, scale)
        # ONE scaled output channel: a packed word holds channels (r & ~1, r | 1), a tile 16 or more
        for n in R.channel_picks(self.c_out) if self.per_channel else ():
            pos = self.pick_position(n, positions, caps, order)
            ln, bs, read, row0 = positions[pos]
            if self.layer == 0:
                top = max(float(v[n].max()) for v in caps[pos])
            else:
                top = self.window_max(caps[pos], m1, ln, read, row0, n)[0]
            self.forward_window(pos, positions[pos], _pow2_below(HALF_MAX / 4 / top), channel=n)
        self.confirm_kernel(self.model(scale))
        return (self.site, self.mode)

    def pick_position(self, n, positions, caps, order):
        """the window a one-channel model runs: the first, in a fixed order, where the UNSCALED capture shows channel n alive in
        the window (at least 1/64 of the layer's largest value there) - a choice made from the premise, never from the flag"""
        for pos in order:
            ln, bs, read, row0 = positions[pos]
            if self.layer == 0:
                lo, hi_row = R.covered_rows(row0)
                v = caps[pos][read][:, max(lo, 0):hi_row + 1]
                inside, everyone, outside = float(v[n].max()), float(v.max()), 0.0
            else:
                inside, outside = self.window_max(caps[pos], self.model(), ln, read, row0, n)
                everyone = self.window_max(caps[pos], self.model(), ln, read, row0)[0]
            if inside > 0 and inside * 64 >= everyone:
                return pos
        raise AssertionError(f"{self.cid}: channel {n} is dead in every window (test bug)")

    def raise_only_window(self, pos, geom, scale):
        lens, base, read, row0 = geom
        s0, s1 = R.window_samples(self.layer, row0, lens[read])
        m, key, a = self.model(scale), (float(scale), None), 1.0
        while not R.nonfinite(self.run(m, self.batch(lens, base, read, s0, s1, a), self.layer)[0]).any():
            a *= 2
            assert a <= 2.0 ** 12, (self.cid, pos)
        first = self.check_side(m, key, "raise", pos, self.batch(lens, base, read, s0, s1, a), (lens, base, read, s0, s1, row0), a)
        self.note(pos, m, None, f"scale 2^{int(math.log2(scale))} raise-amplitude {a:g} first-inf(read,row,ch) {first} (not isolated)")


def batch_lens(batch):
    return batch[2] if batch[0] == "forward" else batch[4]


class _Results:
    def __init__(self):
        self.done = {}

    def get(self, cid, dev):
        if cid not in self.done:
            rig = Rig(cid, dev)
            try:
                self.done[cid] = ("ok", rig.go())
            except BaseException as e:                     # kept: the final test reports the case instead of running it again
                self.done[cid] = ("failed", e)
                raise
            finally:
                rig.close()
        kind, val = self.done[cid]
        if kind == "failed":
            raise AssertionError(f"case {cid} failed earlier in this run: {val!r}")
        return val


@pytest.fixture(scope="module")
def results():
    return _Results()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_overflow_flag_follows_the_stored_rows(dev, results, cid):
    """one site in one mode (see the module's docstring): the windows on the whole layer scaled - the first pooled row of the
    first read, the last valid row of a read with an odd row count, that read's dropped last input row alone (rs_forward cases:
    the row behind the read's end, computed and masked off, sees it through two taps, the last stored row through one), the last
    valid row of the last read, a read of the minimum length alone, and both sides of a tile-row edge - raise and quiet, then up
    to 12 models with ONE output channel scaled, each on the first window (in a fixed order) in which the channel is alive.
    site1-*: layer 0 cannot be captured or be the last layer; its premise is oracle.riser_oracle.conv_block in fp32 on the same
    rows (at least 2 x 65520 somewhere for "raise", below 65504 / 2 everywhere for "quiet"), and layer 1 - its weights divided by
    the same power of two - reads the inf and can repeat the flag: the case still proves that an overflow of layer 0 never
    goes unreported, and that nothing is reported when it stays in range.  site7-f8-rows: not isolated either (see CASES)."""
    assert results.get(cid, dev) == (CASES[cid]["site"], CASES[cid]["mode"])


@pytest.mark.gpu
def test_every_site_and_mode_was_reached(dev, results):
    """the (site, mode) pairs the cases ran on - each confirmed from rs_model_layer_info behind its calls - are the table's"""
    ran = {results.get(cid, dev) for cid in sorted(CASES)}
    assert ran == WANT, (sorted(WANT - ran), sorted(ran - WANT))
