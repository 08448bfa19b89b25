"""numpy helpers of test_gpu_overflow_sites.py: decode a captured activation buffer of a half-precision mode, mirror the
device's overflow test on packed words, and build the batches whose one loud window steers where a layer overflows.

Nothing here touches the GPU: the tests hand these functions host copies of what rs_debug_capture_layer wrote."""
import numpy as np

HALF_MAX = 65504.0               # largest finite IEEE half; fp32 values of 65520 or more convert to +inf
EXP_MASK = 0x7C00                # exponent field of a half: all ones = inf or NaN
QUIET, LOUD = 0.05, 3.0          # standard deviations of the quiet rows and of the loud window at amplitude 1
WINDOW_ROWS = 8                  # width of the loud window in input rows of the layer under test
PAD = 64                         # floats behind the longest read in a row of the fp32 batches (all NaN)


# ---- the three row formats (rs_model_layer_info: rows_format) -------------------------------------------------------------
def hi_slots(rows_format: int, c_out: int) -> np.ndarray:
    """16-bit slot of a row that holds the hi half of channel c, for c in 0 .. c_out - 1.
    0: plain halves; 1: [hi x 32 | lo x 32] per 32-channel panel; 2: [hi16 x 64 | 64 slots of e4m3 bytes] per 64 channels"""
    c = np.arange(c_out)
    if rows_format == 0:
        return c
    if rows_format == 1:
        return (c >> 5) * 64 + (c & 31)
    if rows_format == 2:
        return (c >> 6) * 128 + (c & 63)
    raise ValueError(f"rows_format {rows_format}")


def decode_hi(buf, rows_format: int, cp: int, c_out: int) -> np.ndarray:
    """hi halves [rows, c_out] (uint16 bit patterns) of a captured buffer of rows x cp 16-bit slots; lo halves, e4m3 bytes and
    the pad slots behind channel c_out - 1 are left out"""
    u = np.asarray(buf).view(np.uint16).reshape(-1, cp)
    return u[:, hi_slots(rows_format, c_out)]


def nonfinite(hi: np.ndarray) -> np.ndarray:
    """mask of the halves with exponent field 31 (inf and NaN)"""
    return (hi & EXP_MASK) == EXP_MASK


def finite_max(hi: np.ndarray) -> float:
    """largest magnitude among the finite halves (0 if there are none)"""
    v = np.abs(hi.view(np.float16).astype(np.float32))
    v = v[np.isfinite(v)]
    return float(v.max()) if v.size else 0.0


def locate(hi: np.ndarray, bases, rows_per_block: int):
    """(read, pooled row within the read, channel) of every non-finite half of a decoded capture, in buffer order.  Read b's
    rows start at row bases[b] * rows_per_block of the buffer (Model.block_bases)."""
    start = np.asarray(bases[:-1], dtype=np.int64) * rows_per_block
    r, c = np.nonzero(nonfinite(hi))
    b = np.searchsorted(start, r, side="right") - 1
    return [(int(bb), int(rr - start[bb]), int(cc)) for bb, rr, cc in zip(b, r, c)]


# ---- the device's bit test (csrc/common.hpp: f16_overflow_bits) ------------------------------------------------------------
def overflow_bits(packed):
    """(packed + 0x04000400) & 0x80008000 on uint32 words of two halves, as the epilogues compute it"""
    p = np.asarray(packed, dtype=np.uint64)
    return ((p + np.uint64(0x04000400)) & np.uint64(0xFFFFFFFF) & np.uint64(0x80008000)).astype(np.uint32)


# ---- batches with one loud window --------------------------------------------------------------------------------------
def window_samples(layer: int, row0: int, length: int):
    """samples [s0, s1) of a read of `length` samples that input rows row0 .. row0 + 7 of conv layer `layer` cover (an input row
    of layer i is 2^i samples), cut to the read"""
    s0 = max(0, row0 << layer)
    s1 = min(length, (row0 + WINDOW_ROWS) << layer)
    if not 0 <= s0 < s1:
        raise ValueError(f"window at input row {row0} of layer {layer} misses a read of {length} samples")
    return s0, s1


def covered_rows(row0: int):
    """pooled rows [lo, hi] of the layer under test the window can reach: the rows its 8 input rows pool into, and one more on
    either side (the taps of layers 0 .. i together reach 1 + 1/2 + ... < 2 input rows of layer i beyond the window)"""
    return (row0 - 2) // 2, (row0 + WINDOW_ROWS + 1) // 2


def noise(seed: int, lens, uniform: bool = False):
    """(quiet, loud): per read one unit-variance array for the quiet rows (standard normal; `uniform`: uniform on +-sqrt(3)) and
    one standard-normal array for the window, fixed by the seed"""
    rng = np.random.default_rng(seed)
    if uniform:
        quiet = [rng.uniform(-1.0, 1.0, int(n)) * np.sqrt(3.0) for n in lens]
    else:
        quiet = [rng.standard_normal(int(n)) for n in lens]
    return quiet, [rng.standard_normal(int(n)) for n in lens]


def float_batch(base, lens, read: int, s0: int, s1: int, amplitude: float) -> np.ndarray:
    """fp32 rows [B, max(lens) + PAD]: 0.05 x the quiet noise everywhere, samples [s0, s1) of `read` replaced by amplitude x 3 x
    the loud noise, NaN behind every read (the library must never read it)"""
    quiet, loud = base
    x = np.full((len(lens), int(max(lens)) + PAD), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = QUIET * quiet[b]
    x[read, s0:s1] = amplitude * LOUD * loud[read][s0:s1]
    return x


def int16_reads(base, lens, read: int, s0: int, s1: int, amplitude: float, counts: float = 400.0):
    """the same batch as raw int16 reads (`counts` ADC counts per unit): the median / MAD normalisation of a read undoes its
    scale, so here the window's level RELATIVE to its read is all that `amplitude` sets"""
    quiet, loud = base
    out = []
    for b, n in enumerate(lens):
        v = QUIET * quiet[b]
        if b == read:
            v = v.copy()
            v[s0:s1] = amplitude * LOUD * loud[b][s0:s1]
        out.append(np.clip(np.rint(v * counts), -32768, 32767).astype(np.int16))
    return out


def channel_picks(c_out: int, limit: int = 12):
    """output channels to scale alone: 0, 1, c_out - 2, c_out - 1, and one even and one odd channel of every further 16-channel
    group (a packed word holds channels (r & ~1, r | 1): both parities matter)"""
    picks = [0, 1, c_out - 2, c_out - 1]
    for g in range(1, (c_out + 15) // 16):
        lo, hi = 16 * g, min(16 * g + 16, c_out)
        if hi == c_out:
            continue                                    # the last group is held by c_out - 2, c_out - 1
        picks += [lo + 4 + 2 * (g % 3), lo + 9 + 2 * (g % 2)]
    out = []
    for n in picks:
        if 0 <= n < c_out and n not in out:
            out.append(n)
    return out[:limit]
