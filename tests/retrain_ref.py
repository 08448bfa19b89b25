"""numpy mirror of the reference's retraining preprocessing (riser/retrain/preprocess.py:8-44) and the reads of
tests/golden/retrain.npz.  The rule itself is oracle.riser_oracle.mad_normalise_float without its zero-MAD guard, float32
throughout; float64 only in the pA scaling.  tests/test_retrain_cpu.py pins the mirror to the script's own answers, and it is
the yardstick for inputs larger than a fixture can hold."""
import zlib

import numpy as np

from oracle import riser_oracle as ro

F32 = np.float32


def pa(raw, offset, rng, digitisation):
    """the numpy expression pinned for get_raw_data(scale=True): float64 scalars, one rounding to float32"""
    scale = np.float64(rng) / np.float64(digitisation)
    return np.array(scale * (np.asarray(raw) + np.float64(offset)), dtype=np.float32)


def mad_normalise(x, lim):
    """-> (y float32 [n], median, mad): the script's mad_normalise on a float32 signal, no zero-MAD guard"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    med = F32(np.median(x))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = ro.mad_normalise_float(x, lim=lim, zero_mad_guard=False)
    return y, med, F32(np.median(np.abs(x - med)))


def prepare(signals_pa, cutoffs, lim):
    """-> per cutoff (rows float32 [N_c, cutoff], kept indices, stats float64 [N_c, 2]) of float32 pA reads"""
    out = []
    for n in cutoffs:
        kept = [i for i, s in enumerate(signals_pa) if len(s) >= n]
        res = [mad_normalise(signals_pa[i][:n], lim) for i in kept]
        rows = np.stack([r[0] for r in res]) if res else np.zeros((0, n), dtype=np.float32)
        stats = np.array([[r[1], r[2]] for r in res], dtype=np.float64).reshape(len(res), 2)
        out.append((rows, np.array(kept, dtype=np.int64), stats))
    return out


def same_bits(a, b):
    """bit for bit, NaN equal to NaN whatever its sign and payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    iv = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    jv = b.view(iv.dtype)
    return bool(np.array_equal(na, nb) and np.array_equal(iv[~na], jv[~nb]))


# ---- the fixture's reads: rebuilt from its seed, integers only ------------------------------------------------------------
CUTOFFS = (100, 150, 200)            # freq 50 at 2 / 3 / 4 s
# (outlier limit, cutoffs): every read at each; 3.3 is no float32 value
SETS = ((3.5, (100, 150, 200)), (2.0, (101,)), (3.3, (151,)))
NAMES = ("generic_260", "exact_200", "exact_150", "exact_100", "short_60", "between_120", "between_170", "all_equal",
         "zero_mad_mix", "outliers_0_1", "spike_at_each_cutoff_end", "runs", "run_of_66", "heavy_ties", "negative_pa",
         "mixed_sign", "generic_333")


def _noise(rng, n, centre=500):
    return (centre + rng.integers(-15, 16, size=(4, n)).sum(axis=0)).astype(np.int16)


def build_reads(seed):
    """-> (reads: list of int16 arrays, offset, range, digitisation: float64 [N]) in the order of NAMES"""
    rng = np.random.default_rng(int(seed))
    reads = [_noise(rng, n) for n in (260, 200, 150, 100, 60, 120, 170)]
    reads.append(np.full(200, 487, dtype=np.int16))                                   # all_equal
    z = np.full(230, 500, dtype=np.int16)                                             # zero_mad_mix: > half equal
    z[[0, 1, 2]] = (620, 640, 610)
    z[[3, 4]] = (380, 390)
    z[30:230:7] = _noise(rng, len(range(30, 230, 7)))
    z[[60, 61, 120, 199]] = (900, 100, 900, 100)
    reads.append(z)
    o = _noise(rng, 210)                                                              # outliers_0_1
    o[[0, 1]] = (2500, 2300)
    reads.append(o)
    s = _noise(rng, 260)                                                              # a spike at c - 1 for every cutoff c
    s[[99, 149, 199]] = (3000, -2000, 2800)
    s[[100, 150]] = (2900, 2700)                                                      # SETS' odd cutoffs: their last index
    reads.append(s)
    r = _noise(rng, 240)                                                              # runs: of 4, and across 100 and 150
    r[40:44] = (2000, -1500, 2200, 2100)
    r[97:104] = (1900, 2000, 2100, -900, 2300, 2400, 2500)
    r[148:153] = (-800, -900, 2600, 2700, -1000)
    reads.append(r)
    q = _noise(rng, 220)                                                              # run_of_66: 110 .. 175
    q[110:176] = (2000 + 37 * np.arange(66) % 500 * np.where(np.arange(66) % 3 == 0, -1, 1)).astype(np.int16)
    reads.append(q)
    reads.append(rng.choice(np.array([498, 499, 500, 501, 503], dtype=np.int16), size=205))     # heavy_ties
    reads.append(_noise(rng, 200))                                                    # negative_pa (by its offset)
    reads.append(_noise(rng, 215))                                                    # mixed_sign
    g = _noise(rng, 333)
    g[rng.integers(1, 332, size=9)] += rng.integers(300, 2000, size=9).astype(np.int16)
    reads.append(g)
    n = len(reads)
    offset = rng.integers(-20, 21, size=n).astype(np.float64)
    offset[NAMES.index("negative_pa")] = -900.0
    offset[NAMES.index("mixed_sign")] = -500.0
    rng_pa = (14000 + rng.integers(0, 1000, size=n)) / 10.0
    digitisation = np.full(n, 8192.0)
    assert n == len(NAMES)
    return reads, offset, rng_pa, digitisation


def reads_crc(reads):
    return zlib.crc32(b"".join(np.ascontiguousarray(r).tobytes() for r in reads))


def key(lim, cutoff):
    return f"y_{str(lim).replace('.', 'p')}_{cutoff}"


def write_tensor_inputs(g):
    """the two .npy contents the fixture's write_tensors case was recorded on: float32 [N, 100] and float64 [7, 100]"""
    pos = np.asarray(g[key(3.5, 100)])
    return pos, pos[::-1][:7].astype(np.float64) * 0.5
