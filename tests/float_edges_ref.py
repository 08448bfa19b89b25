"""The float signal kernels' VALUE edges, reference side: short reads of float16 / float32 / float64 that carry NaNs, infinities,
zeros of both signs, values next to overflow and underflow, subnormals and exact ties at the outlier limit, each at lengths that
straddle the radix select's wave and workgroup edges; the degenerate channel calibrations of the int16 retraining path; and what
every case must be for its name to be true, spelled with numpy (PROPERTIES).  The yardsticks are oracle.riser_oracle.mad_normalise
(the live rule) and tests.retrain_ref.mad_normalise (the retraining script's); tests/golden/float_edges.npz
(tools/make_golden_float_edges.py) pins both to the reference's own functions on exactly these reads.  All arithmetic is numpy's."""
import zlib
from typing import NamedTuple

import numpy as np

from oracle import riser_oracle as ro
from riser_amd.retrain import WORKGROUP_THREADS
from tests import retrain_ref as R
from tests.retrain_ref import same_bits            # noqa: F401  (the one NaN-aware bit comparison)
from tests.test_gpu_parity import SMALL_FLOAT_LENGTHS

SEED = 20261020
DTYPES = ("float16", "float32", "float64")
LIMITS = (3.5, 0.0)                                # the retraining rule's outlier_lim: the script's, and "everything but 0"
W = WORKGROUP_THREADS
LENGTHS = tuple(sorted(set(SMALL_FLOAT_LENGTHS) | {W - 1, W + 1}))
CLASSES = ("nan", "inf", "zero", "overflow", "underflow", "limit", "control")
ADC = np.array([455, 470, 485, 500, 515, 530, 560])          # seven levels: low-entropy reads, small fixtures


class Case(NamedTuple):
    name: str                                      # "<class>.<variant>.<n>"
    cls: str
    prop: str                                      # key of PROPERTIES
    x: np.ndarray


# ---- the oracles --------------------------------------------------------------------------------------------------------------
def live_oracle(x):
    with np.errstate(all="ignore"):
        return ro.mad_normalise(x)


def retrain_oracle(x, lim):
    """-> (y float32, median, mad)"""
    with np.errstate(all="ignore"):
        return R.mad_normalise(x, lim)


def stats(x):
    """numpy's own (median, MAD, denom, y before smoothing) of a read, in its dtype"""
    T = x.dtype.type
    with np.errstate(all="ignore"):
        med = np.median(x)
        dev = np.abs(x - med)
        mad = np.median(dev)
        denom = T(ro.SCALING_FACTOR) * mad
        return med, mad, denom, ((x - med) / denom).astype(x.dtype)


# ---- the sign of a zero median ---------------------------------------------------------------------------------------------
def _bits(v):
    v = np.asarray(v)
    return int(v.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]))


def zero_sign_free(x):
    """numpy's median or MAD of this read changes its bits (NaN apart) when the read is permuted: only the sign of a zero can, since
    np.partition holds -0.0 and +0.0 equal and leaves them in an order that depends on the input's.  The read itself, sorted both
    ways and eight fixed shuffles."""
    rng = np.random.default_rng(len(x))
    orders = [np.arange(len(x)), np.argsort(x, kind="stable"), np.argsort(x, kind="stable")[::-1]]
    orders += [rng.permutation(len(x)) for _ in range(8)]
    seen = set()
    with np.errstate(all="ignore"):
        for o in orders:
            med = np.median(x[o])
            mad = np.median(np.abs(x[o] - med))
            seen.add((np.isnan(med) or _bits(med), np.isnan(mad) or _bits(mad)))
    return len(seen) > 1


def mask_zero_sign(a):
    """a with every -0.0 made +0.0"""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[a == 0] = 0
    return a


# ---- builders -----------------------------------------------------------------------------------------------------------------
def nan_of(dtype, kind):
    """a NaN by its bits -> uint: "pos" / "neg" quiet, "payload" negative, signalling, with a payload"""
    fi = np.finfo(dtype)
    width = 8 * np.dtype(dtype).itemsize
    expo = ((1 << fi.nexp) - 1) << fi.nmant
    return {"pos": expo | 1 << (fi.nmant - 1), "neg": 1 << (width - 1) | expo | 1 << (fi.nmant - 1),
            "payload": 1 << (width - 1) | expo | 0x155}[kind]


def put_nan(x, i, kind):
    x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])[i] = nan_of(x.dtype, kind)


def base(rng, n, dtype):
    """a pA-like read on seven levels, mixed sign, MAD > 0 (two or three samples: all distinct)"""
    t = rng.choice(ADC, size=n, replace=n > len(ADC))
    return (t * 0.17548 - 80.0).astype(dtype)


def squiggle(rng, n, dtype):
    s = 500 + rng.integers(-15, 16, (4, n)).sum(0)
    if n > 8:
        s[0], s[n - 1] = 2500, -900
        s[n // 2: n // 2 + 3] = (2000, -1500, 2200)
    return (s * 0.17548 - 80.0).astype(dtype)


def around_zero(rng, n, mid, dtype):
    """the values `mid` in the middle of the sorted order, (n - len(mid)) / 2 quarters below and above, shuffled"""
    side = (n - len(mid)) // 2
    assert 2 * side + len(mid) == n
    lo = -(1 + rng.integers(0, 9, side)) * 0.25
    hi = (1 + rng.integers(0, 9, side)) * 0.25
    return rng.permutation(np.concatenate([lo, np.asarray(mid, dtype=np.float64), hi])).astype(dtype)


def mixed_zeros(rng, k):
    z = np.where(rng.integers(0, 2, k) == 1, -0.0, 0.0)
    if k >= 2:
        z[0], z[1] = -0.0, 0.0
    return z


def unit_read(rng, n, unit, dtype, spike=None):
    """odd n, median 0, MAD exactly `unit`: one 0, and on each side (n - 1) / 2 of unit / 2, unit, 2 unit with `unit` the
    middle deviation; `spike` replaces one + 2 unit (a deviation above the MAD stays above it)"""
    assert n % 2 == 1 and n >= 7
    h = (n - 1) // 2
    a = h // 3
    side = np.concatenate([np.full(a, 0.5), np.full(h - 2 * a, 1.0), np.full(a, 2.0)])
    x = np.concatenate([-side, [0.0], side]).astype(dtype) * dtype(unit)
    if spike is not None:
        x[-1] = spike
    p = rng.permutation(n)
    return x[p]


def limit_spikes(dtype):
    """(unit, lowest and highest x with x / (T(1.4826) * unit) == 3.5 exactly in T), searched over a few units"""
    T = np.dtype(dtype).type
    for unit in (1.0, 1.25, 1.5, 1.75, 0.75, 1.125, 1.375, 1.625, 1.875):
        d = T(ro.SCALING_FACTOR) * T(unit)
        x = T(3.5) * d
        for _ in range(8):
            x = np.nextafter(x, T(0))
        hits = []
        for _ in range(17):
            if T(x / d) == T(3.5):
                hits.append(x)
            x = np.nextafter(x, T(np.inf))
        if hits:
            return T(unit), hits[0], hits[-1]
    raise AssertionError(f"no exact tie at 3.5 in {dtype}")


def edge_cases(dtype, seed=SEED):
    """-> [Case]: every class at its lengths, the same for a given (dtype, seed)"""
    dt = np.dtype(dtype)
    T = dt.type
    fi = np.finfo(dt)
    rng = np.random.default_rng([int(seed), dt.itemsize])
    out = []

    def add(cls, variant, x, prop):
        x = np.ascontiguousarray(x, dtype=dt)
        out.append(Case(f"{cls}.{variant}.{len(x)}", cls, prop, x))

    # ---- NaN ----
    kinds = ("pos", "neg", "payload")
    k = 0
    for n in (2, 3, 64, 65, 257, W + 1, 1023):
        for where, i in (("first", 0), ("mid", n // 2), ("last", n - 1)):
            if where == "mid" and i in (0, n - 1):
                continue
            x = base(rng, n, dt)
            put_nan(x, i, kinds[k % 3])
            add("nan", f"{kinds[k % 3]}_{where}", x, "one_nan")
            k += 1
        k += 1                                                               # every kind meets every place
    for n in (63, 256):
        x = base(rng, n, dt)
        for j, i in enumerate(rng.choice(n, 5, replace=False)):
            put_nan(x, i, kinds[j % 3])
        add("nan", "several", x, "some_nan")
    x = base(rng, 64, dt)                                             # so many that a finite order statistic cannot be the middle
    for j, i in enumerate(rng.choice(64, 40, replace=False)):
        put_nan(x, i, kinds[j % 2])
    add("nan", "majority", x, "some_nan")
    for n in (3, 64):
        x = np.zeros(n, dtype=dt)
        for i in range(n):
            put_nan(x, i, kinds[i % 3])
        add("nan", "all", x, "all_nan")
    for n in (65, W):
        x = base(rng, n, dt)
        q = n // 3
        x[q: q + 4] = (400, -300, 420, 410)
        put_nan(x, q - 1, "pos")
        put_nan(x, q + 4, "payload")
        add("nan", "by_outliers", x, "some_nan")
    x = base(rng, 66, dt)
    x[7] = np.inf
    put_nan(x, 40, "neg")
    add("nan", "with_inf", x, "one_nan")

    # ---- +-inf ----
    for n in (3, 64, 65, 257):
        for variant, vals in (("pos", (np.inf,)), ("neg", (-np.inf,)), ("both", (np.inf, -np.inf))):
            for where in ("first", "mid", "last"):
                if n == 3 and (len(vals) == 2 or where != "first"):
                    continue                                             # three samples: one inf at most keeps the MAD finite
                x = base(rng, n, dt)
                i = {"first": 0, "mid": n // 2, "last": n - len(vals)}[where]
                x[i: i + len(vals)] = vals
                add("inf", f"{variant}_{where}", x, "inf_finite_stats")
    for n in (65, 256):
        x = base(rng, n, dt)
        q = n // 2
        x[q: q + 6] = (400, 410, np.inf, -np.inf, -300, 405)          # inside a run of finite outliers
        x[0: 2] = (np.inf, 390)                                          # :132 copies an outlier that is smoothed later
        x[n - 2:] = (-350, -np.inf)                                      # :134 copies the smoothed one
        add("inf", "in_runs", x, "inf_finite_stats")
    for n in (2, 3, 64, 65, W - 1, W + 1):
        for sign in (1, -1):
            x = base(rng, n, dt)
            x[rng.choice(n, n // 2 + (n % 2), replace=False)] = sign * np.inf          # the middle order statistic(s) infinite
            add("inf", f"median_{'pos' if sign > 0 else 'neg'}", x, "median_inf")
    for n in (2, 64):
        x = base(rng, n, dt)                                             # even n: (finite, +inf) in the middle
        x[rng.choice(n, n // 2, replace=False)] = np.inf
        add("inf", "median_half", x, "median_inf")
        x = np.full(n, np.inf, dtype=dt)                                 # (-inf, +inf) in the middle: their mean is NaN
        x[rng.choice(n, n // 2, replace=False)] = -np.inf
        add("inf", "median_cancels", x, "median_nan_no_nan")
    for n in (3, 65):
        x = np.full(n, np.inf, dtype=dt)                                 # a finite median among infinities: the MAD infinite
        x[: n // 2] = -np.inf
        x[n // 2] = 7.75
        add("inf", "mad_inf", rng.permutation(x), "mad_inf")
    add("inf", "alone", np.array([np.inf]), "median_inf")

    # ---- signed zeros ----
    for n in (63, 65, 257, W - 1):
        add("zero", "mid_mixed", around_zero(rng, n, mixed_zeros(rng, 3), dt), "median_zero_mixed")
    for n in (4, 64, 256, W):
        add("zero", "mid_mixed", around_zero(rng, n, mixed_zeros(rng, 2 if n == 4 else 4), dt), "median_zero_mixed")
    for n in (3, 65):
        add("zero", "mid_neg", around_zero(rng, n, [-0.0], dt), "median_neg_zero")
    add("zero", "mid_neg", around_zero(rng, 64, [-0.0, -0.0], dt), "median_neg_zero")
    add("zero", "mid_neg_pos", around_zero(rng, 64, [-0.0, 0.0], dt), "median_zero_mixed")
    x = around_zero(rng, 64, [-0.75, 0.75], dt)                          # -a + a: +0.0 whatever the order
    add("zero", "mid_cancels", x, "median_zero_no_zero")
    for n in (64, 257):
        x = np.abs(base(rng, n, dt)) + T(1)
        x[rng.choice(n, 6, replace=False)] = mixed_zeros(rng, 6)
        add("zero", "off_median", x, "zeros_off_median")
    for n in (2, 3, 64, 65, W + 1):
        add("zero", "all", rng.permutation(mixed_zeros(rng, n)).astype(dt), "all_zero_mixed")
    for n in (65, 256):
        x = base(rng, n, dt)
        idx = rng.choice(n, n // 2 + 3, replace=False)
        x[idx] = mixed_zeros(rng, len(idx))                              # more than half zeros: MAD 0 about a zero median
        add("zero", "zero_mad", x, "median_zero_mad_zero")

    # ---- overflow ----
    big = T(fi.max)
    for n in (2, 64, 256):
        h = n // 2 - 1
        x = np.concatenate([base(rng, h, dt), [T(0.75) * big, big], np.full(h, big)])
        add("overflow", "mean2", rng.permutation(x), "mean2_overflows")
    for n in (63, 65, 257):                                              # odd: no mean of two values of this size
        x = np.full(n, T(-0.9) * big, dtype=dt)                          # x - med beyond the largest finite value
        x[::4] = T(-0.9) * big * T(1 - 2.0 ** -6)
        x[1::4] = T(-0.9) * big * T(1 - 2.0 ** -5)
        x[rng.choice(n, 5, replace=False)] = big
        x[rng.choice(n, 2, replace=False)] = T(0.5) * big
        add("overflow", "sub", x, "sub_overflows")
    for n in (3, 64, 65):
        h = n // 2
        x = np.concatenate([np.full(h, T(-0.8) * big), [T(0)] * (n % 2), np.full(h, T(0.8) * big)]).astype(dt)
        if n > 3:
            x[0], x[-1] = T(-0.4) * big, T(0.4) * big
        # an even n: the two middle deviations are 0.8 max each, and their sum overflows before the product can
        add("overflow", "denom", rng.permutation(x), "denom_overflows" if n % 2 else "mad_mean2_overflows")
    tiny_unit = T(fi.smallest_normal) * T(4)
    x = unit_read(rng, 65, tiny_unit, T, spike=T(0.5) * big * tiny_unit * T(1.4826))
    add("overflow", "y_near_max", x, "y_near_max")
    x = unit_read(rng, 65, tiny_unit, T, spike=T(0.5) * big)
    add("overflow", "y", x, "y_overflows")

    # ---- underflow and subnormals ----
    sub = T(fi.smallest_subnormal)
    for n in (3, 64, 65, 256):
        t = rng.choice(ADC - 440, size=n, replace=n > len(ADC)) * np.where(rng.integers(0, 2, n) == 1, -1, 1)
        add("underflow", "all_subnormal", (t * np.float64(sub)).astype(dt), "all_subnormal")
    for n in (64, 257):
        t = rng.choice(np.array([0, 3, 5, 9, 11, 14, 20]), size=n)
        x = np.float64(fi.smallest_normal) + t * np.float64(sub)         # normal values one subnormal step apart: exact in T
        add("underflow", "mad_subnormal", x, "mad_subnormal")
    add("underflow", "denom_smallest", unit_read(rng, 65, sub, T), "denom_smallest_subnormal")
    add("underflow", "denom_smallest", unit_read(rng, 257, sub, T, spike=T(40) * sub), "denom_smallest_subnormal")
    for n in (65, 255):
        h = (n - 1) // 2
        far = T(2.0 ** (fi.maxexp // 2))
        near = T(fi.smallest_normal) * far * T(2.0 ** -3)                # near / (1.4826 far): a few units of the smallest subnormal
        side = np.concatenate([near * np.arange(1, 7).astype(dt), np.full(h - 6, far)])
        add("underflow", "y_subnormal", rng.permutation(np.concatenate([-side, [T(0)], side])), "y_subnormal")

    # ---- ties at the limit ----
    unit, x_lo, x_hi = limit_spikes(dt)
    for n, sign in ((65, 1), (257, -1)):
        for variant, spike in (("at", x_hi), ("above", np.nextafter(x_hi, T(np.inf))), ("below", np.nextafter(x_lo, T(0)))):
            x = unit_read(rng, n, unit, T, spike=spike)
            add("limit", f"{variant}_{'pos' if sign > 0 else 'neg'}", x * T(sign), f"limit_{variant}")

    # ---- control ----
    for n in (3, 64, 257, W + 1):
        add("control", "squiggle", squiggle(rng, n, dt), "plain")
    assert len({c.name for c in out}) == len(out)
    return out


def edge_reads(dtype, seed=SEED):
    """-> [(name, x)]"""
    return [(c.name, c.x) for c in edge_cases(dtype, seed)]


# ---- what a case must be for its name to be true ---------------------------------------------------------------------------------
def _p_limit(kind):
    def check(x):
        med, mad, denom, y = stats(x)
        T = x.dtype.type
        out = np.abs(y) > T(3.5)
        if med != 0 or not np.isfinite(y).all():
            return False
        i = int(np.argmax(np.abs(y)))
        moved = x.copy()
        if kind == "at":
            return bool(abs(y[i]) == T(3.5) and not out.any())
        # one ulp of x the other way and the same sample sits exactly at the limit, the median and the MAD unchanged
        moved[i] = np.nextafter(x[i], T(0) if kind == "above" else T(np.inf) * np.sign(x[i]))
        med2, mad2, _, y2 = stats(moved)
        same = _bits(med2) == _bits(med) and _bits(mad2) == _bits(mad) and abs(y2[i]) == T(3.5)
        return bool(same and (out.sum() == 1 and out[i] if kind == "above" else not out.any() and abs(y[i]) < T(3.5)))
    return check


def _zeros_mixed(x):
    z = x[x == 0]
    return bool(np.signbit(z).any() and not np.signbit(z).all())


def _p_mean2(x):
    v = np.sort(x)
    a, b = v[len(x) // 2 - 1], v[len(x) // 2]
    with np.errstate(all="ignore"):
        wide = bool(np.isfinite(a) and np.isfinite(b) and np.isinf(a + b))
        med = np.median(x)
    # float32 and float64 overflow with numpy; float16's float32 accumulator must not
    return wide and len(x) % 2 == 0 and (np.isfinite(med) if x.dtype == np.float16 else np.isinf(med))


def _fin(x):
    return bool(np.isfinite(x).all())


def _sub_overflows(x):
    with np.errstate(all="ignore"):
        return bool(np.isinf(x - np.median(x)).any())


PROPERTIES = {
    "one_nan": lambda x: int(np.isnan(x).sum()) == 1,
    "some_nan": lambda x: 1 < int(np.isnan(x).sum()) < len(x),
    "all_nan": lambda x: bool(np.isnan(x).all()),
    "inf_finite_stats": lambda x: bool(np.isinf(x).any() and not np.isnan(x).any() and np.isfinite(stats(x)[0])
                                       and np.isfinite(stats(x)[1]) and stats(x)[1] > 0),
    "median_inf": lambda x: bool(np.isinf(np.median(x)) and not np.isnan(x).any()),
    "median_nan_no_nan": lambda x: bool(np.isnan(stats(x)[0]) and not np.isnan(x).any()),
    "mad_inf": lambda x: bool(np.isfinite(stats(x)[0]) and np.isinf(stats(x)[1])),
    "median_zero_mixed": lambda x: bool(stats(x)[0] == 0 and stats(x)[1] > 0 and _zeros_mixed(x)
                                        and (np.sort(x)[[(len(x) - 1) // 2, len(x) // 2]] == 0).all()),
    "median_neg_zero": lambda x: bool(stats(x)[0] == 0 and stats(x)[1] > 0 and np.signbit(x[x == 0]).all()
                                      and (np.sort(x)[[(len(x) - 1) // 2, len(x) // 2]] == 0).all()),
    "median_zero_no_zero": lambda x: bool(stats(x)[0] == 0 and not (x == 0).any()),
    "zeros_off_median": lambda x: bool(stats(x)[0] != 0 and _zeros_mixed(x) and _fin(stats(x)[3])),
    "all_zero_mixed": lambda x: bool((x == 0).all() and (len(x) < 2 or _zeros_mixed(x)) and stats(x)[1] == 0),
    "median_zero_mad_zero": lambda x: bool(stats(x)[0] == 0 and stats(x)[1] == 0 and (x != 0).any() and _zeros_mixed(x)),
    "mean2_overflows": _p_mean2,
    "sub_overflows": lambda x: bool(_fin(x) and _fin(stats(x)[:2]) and _sub_overflows(x)),
    "denom_overflows": lambda x: bool(_fin(x) and _fin(stats(x)[:2]) and np.isinf(stats(x)[2])),
    "mad_mean2_overflows": lambda x: bool(_fin(x) and np.isfinite(stats(x)[0]) and np.isinf(stats(x)[2])
                                          and np.isfinite(stats(x)[1]) == (x.dtype == np.float16)),
    "y_near_max": lambda x: bool(_fin(stats(x)[3]) and np.abs(stats(x)[3]).max() > np.finfo(x.dtype).max / 4),
    "y_overflows": lambda x: bool(_fin(x) and _fin(stats(x)[:3]) and not _sub_overflows(x) and np.isinf(stats(x)[3]).any()),
    "all_subnormal": lambda x: bool((np.abs(x) < np.finfo(x.dtype).smallest_normal).all() and stats(x)[1] > 0),
    "mad_subnormal": lambda x: bool((np.abs(x) >= np.finfo(x.dtype).smallest_normal).all()
                                    and 0 < stats(x)[1] < np.finfo(x.dtype).smallest_normal),
    "denom_smallest_subnormal": lambda x: bool(stats(x)[1] == np.finfo(x.dtype).smallest_subnormal
                                               and stats(x)[2] == np.finfo(x.dtype).smallest_subnormal),
    "y_subnormal": lambda x: bool(((np.abs(stats(x)[3]) > 0) & (np.abs(stats(x)[3]) < np.finfo(x.dtype).smallest_normal)).any()
                                  and _fin(stats(x)[3])),
    "limit_at": _p_limit("at"),
    "limit_above": _p_limit("above"),
    "limit_below": _p_limit("below"),
    "plain": lambda x: bool(_fin(x) and _fin(live_oracle(x)) and live_oracle(x).dtype == x.dtype),
}


# ---- the int16 retraining path: degenerate calibrations ------------------------------------------------------------------------
CUTOFFS = (65, W + 1)                              # both prefixes of every int16 read keep what its calibration does to it


def int16_reads(seed=SEED):
    """three reads of W + 8 samples: about zero with exact zeros in both prefixes, about 500 with spikes, and five tied levels"""
    rng = np.random.default_rng([int(seed), 16])
    n = W + 8
    a = rng.integers(-15, 16, (4, n)).sum(0).astype(np.int16)
    a[[5, 64, 400]] = 0
    a[[20, 21, 300]] = (900, -800, 1000)
    b = (500 + rng.integers(-15, 16, (4, n)).sum(0)).astype(np.int16)
    b[[0, 1, 40, 64, 511, 512]] = (2500, 2300, -900, 2000, 2100, -1000)
    c = rng.choice(np.array([498, 499, 500, 501, 503], dtype=np.int16), size=n)
    return [a, b, c]


_DEGENERATE = (
    ("digitisation_0", (0.0, 1400.0, 0.0)),            # scale inf: +-inf, and NaN for a raw 0
    ("digitisation_0_offset", (100.0, 1400.0, 0.0)),   # no sample at 0: +-inf only
    ("range_0", (5.0, 0.0, 8192.0)),                   # every sample a zero (of its own sign): MAD 0
    ("offset_nan", (np.nan, 1400.0, 8192.0)),
    ("range_negative", (5.0, -1400.0, 8192.0)),
    ("scale_subnormal", (0.0, 8.192e-39, 8192.0)),     # pA = 1e-42 * raw: float32 subnormals out of a float64 product
    ("offset_huge", (1.0e9, 1400.0, 8192.0)),          # float32 keeps 16 pA steps at 1.7e8: a handful of ties
)
CALIBRATION_NAMES = tuple(n for n, _ in _DEGENERATE)


def degenerate_calibrations():
    """-> [(offset, range, digitisation)] for retrain_ref.pa, in the order of CALIBRATION_NAMES"""
    return [t for _, t in _DEGENERATE]


def calibrated(seed=SEED):
    """-> [(name, read index, pA float32 [W + 8])] of every int16 read under every degenerate calibration"""
    out = []
    with np.errstate(all="ignore"):
        for cname, (offset, rng, dig) in zip(CALIBRATION_NAMES, degenerate_calibrations()):
            for i, r in enumerate(int16_reads(seed)):
                out.append((f"{cname}.{i}", i, R.pa(r, offset, rng, dig)))
    return out


def _distinct(p):
    return len(np.unique(p[~np.isnan(p)]))


CALIBRATION_PROPERTIES = {
    "digitisation_0": lambda i, p: bool(np.isinf(p[~np.isnan(p)]).all() and np.isnan(p).any() == (i == 0)),
    "digitisation_0_offset": lambda i, p: bool(np.isinf(p).all()),
    "range_0": lambda i, p: bool((p == 0).all()),
    "offset_nan": lambda i, p: bool(np.isnan(p).all()),
    "range_negative": lambda i, p: bool(np.isfinite(p).all() and (p < 0).any()),
    "scale_subnormal": lambda i, p: bool((np.abs(p) < np.finfo(np.float32).smallest_normal).all() and _distinct(p) > 4),
    "offset_huge": lambda i, p: bool(np.isfinite(p).all() and 1 <= _distinct(p) <= 32),
}


def inputs_crc(seed=SEED):
    """one CRC over every float read of every dtype and the int16 reads"""
    crc = 0
    for dt in DTYPES:
        for c in edge_cases(dt, seed):
            crc = zlib.crc32(c.name.encode() + c.x.tobytes(), crc)
    for r in int16_reads(seed):
        crc = zlib.crc32(r.tobytes(), crc)
    return crc


def live_key(dtype, name):
    return f"live.{dtype}.{name}"


def retrain_key(name, lim, n=None):
    return f"retrain.{name}.{str(lim).replace('.', 'p')}" + (f".{n}" if n is not None else "")


def golden_groups(seed=SEED):
    """-> {group: [(key, samples), ...]}: the fixture keeps one concatenated array per group, in this order"""
    groups = {}
    for dt in DTYPES:
        groups[f"live.{dt}"] = [(live_key(dt, name), len(x)) for name, x in edge_reads(dt, seed)]
    f32 = [(name, x) for name, x in edge_reads("float32", seed) if len(x) >= 2]
    for lim in LIMITS:
        groups[f"retrain.{lim}"] = [(retrain_key(name, lim), len(x)) for name, x in f32]
        groups[f"retrain.cal.{lim}"] = [(retrain_key("cal." + name, lim, n), n) for name, _, _ in calibrated(seed) for n in CUTOFFS]
    return groups


def unpack(g):
    """the fixture -> {key: the reference's output for that case}; a row the reference returned as int64 zeros comes back so"""
    out = {}
    for group, keys in golden_groups(int(g["seed"])).items():
        flat, zeros = g[group + ".flat"], g[group + ".int64_zeros"]
        assert len(zeros) == len(keys)
        pos = 0
        for (k, n), z in zip(keys, zeros):
            if z:
                out[k] = np.zeros(n, dtype=np.int64)
            else:
                out[k] = flat[pos: pos + n]
                pos += n
        assert pos == len(flat), group
    return out
