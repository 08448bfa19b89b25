"""The value-edge table of the float signal kernels (tests/float_edges_ref.py) without a GPU: the builder still draws the reads the
fixture was recorded on, both numpy oracles give the reference's own bits and dtypes on them (tests/golden/float_edges.npz,
tools/make_golden_float_edges.py), every case is what its name says, and where numpy itself leaves the sign of a zero median
open.  tests/test_float_edges.py holds rs_normalise_float and rs_retrain_prepare to these oracles on these reads."""
import os

import numpy as np
import pytest

from tests import float_edges_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "float_edges.npz"))


@pytest.fixture(scope="module")
def want(g):
    return F.unpack(g)


@pytest.fixture(scope="module")
def cases():
    return {dt: F.edge_cases(dt) for dt in F.DTYPES}


def test_builder_regenerates_the_inputs(g):
    assert int(g["seed"]) == F.SEED and tuple(g["limits"].tolist()) == F.LIMITS and tuple(g["cutoffs"].tolist()) == F.CUTOFFS
    assert F.inputs_crc(int(g["seed"])) == int(g["inputs_crc"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "float_edges.npz")) < 64 * 1024


def test_same_bits_is_the_comparison_the_table_needs():
    for dt in F.DTYPES:
        a = np.array([1.5, -0.0, 0.0, np.inf], dtype=dt)
        nan = np.zeros(3, dtype=dt)
        for i, kind in enumerate(("pos", "neg", "payload")):
            F.put_nan(nan, i, kind)
        assert np.isnan(nan).all() and len(set(nan.tobytes()[i * nan.itemsize:(i + 1) * nan.itemsize] for i in range(3))) == 3
        assert F.same_bits(nan, nan[::-1]) and F.same_bits(a, a.copy())
        assert not F.same_bits(a, a[[0, 2, 1, 3]])                            # the sign of a zero counts
        assert not F.same_bits(a, np.array([1.5, -0.0, 0.0, np.nan], dtype=dt))
        assert not F.same_bits(a, a.astype(np.float64 if dt != "float64" else np.float32))
        assert F.same_bits(F.mask_zero_sign(a), F.mask_zero_sign(a[[0, 2, 1, 3]]))
    assert not F.same_bits(np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.float64))


def test_oracles_equal_the_reference(want, cases):
    bad = []
    for dt in F.DTYPES:
        for c in cases[dt]:
            w = want[F.live_key(dt, c.name)]
            got = F.live_oracle(c.x)
            if got.dtype != w.dtype or not F.same_bits(got, w):
                bad.append(("live", dt, c.name))
    for c in cases["float32"]:
        if len(c.x) < 2:
            continue
        for lim in F.LIMITS:
            y, med, mad = F.retrain_oracle(c.x, lim)
            if not F.same_bits(y, want[F.retrain_key(c.name, lim)]):
                bad.append(("retrain", lim, c.name))
            s_med, s_mad = F.stats(c.x)[:2]
            assert F.same_bits(med, np.float32(s_med)) and F.same_bits(mad, np.float32(s_mad)), c.name
    for name, _, pa in F.calibrated():
        for lim in F.LIMITS:
            for n in F.CUTOFFS:
                if not F.same_bits(F.retrain_oracle(pa[:n], lim)[0], want[F.retrain_key("cal." + name, lim, n)]):
                    bad.append(("retrain", lim, name, n))
    assert not bad, bad


def test_every_case_is_what_its_name_says(cases):
    for dt in F.DTYPES:
        cs = cases[dt]
        assert [c.name for c in cs] == [n for n, _ in F.edge_reads(dt)] and all(c.x.dtype == np.dtype(dt) for c in cs)
        assert {c.cls for c in cs} == set(F.CLASSES) and all(c.name.startswith(c.cls + ".") for c in cs)
        bad = [c.name for c in cs if not F.PROPERTIES[c.prop](c.x)]
        assert not bad, (dt, bad)
        lens = np.array([len(c.x) for c in cs])
        assert lens.max() <= 1100 and (lens <= 260).mean() > 0.75 and set(lens[lens > 1]) <= set(F.LENGTHS) | {4, 66, F.W}
        for cls in ("nan", "inf", "zero"):                               # both sides of a wave and of the retraining workgroup
            have = {len(c.x) for c in cs if c.cls == cls}
            assert have & {2, 3} and have & {63, 64} and 65 in have and have & {F.W - 1, F.W} and have & {F.W + 1, 1023}, cls
            assert {n % 2 for n in have} == {0, 1}
    # the same table for every dtype: one list of names
    assert [c.name for c in cases["float16"]] == [c.name for c in cases["float32"]] == [c.name for c in cases["float64"]]
    for name, i, pa in F.calibrated():
        assert pa.dtype == np.float32 and len(pa) >= F.CUTOFFS[-1]
        for n in F.CUTOFFS:                                              # both prefixes keep what the calibration does
            assert F.CALIBRATION_PROPERTIES[name.split(".")[0]](i, pa[:n]), (name, n)
    assert {n.split(".")[0] for n, _, _ in F.calibrated()} == set(F.CALIBRATION_PROPERTIES) == \
        set(F.CALIBRATION_NAMES)


def test_what_the_reference_answers(want, cases):
    """the contract in the reference's own rows: one NaN, an infinite median or an infinite MAD makes the whole row NaN; a zero MAD
    gives the live rule's int64 zeros and a NaN MAD does not; an infinity beside a finite median and MAD is smoothed away"""
    for dt in F.DTYPES:
        for c in cases[dt]:
            w = want[F.live_key(dt, c.name)]
            med, mad = F.stats(c.x)[:2]
            assert (w.dtype == np.int64) == bool(mad == 0), c.name
            assert w.dtype == (np.int64 if mad == 0 else c.x.dtype), c.name
            if c.cls == "nan" or c.prop in ("median_inf", "median_nan_no_nan"):
                assert np.isnan(med) or np.isinf(med), c.name
                assert np.isnan(mad) and w.dtype == c.x.dtype and np.isnan(w).all(), c.name
            if c.prop == "inf_finite_stats":
                assert np.isfinite(w[1:-1]).all() and np.isinf(c.x).any(), c.name      # :132 / :134 copy, unclipped
            if c.prop == "mad_inf":
                assert np.isnan(w).sum() == len(w) - 1 and (w == 0).sum() == 1, c.name
    for c in cases["float32"]:
        if c.prop in ("all_zero_mixed", "median_zero_mad_zero") and len(c.x) >= 2:
            w = want[F.retrain_key(c.name, 3.5)]                              # the retraining rule has no zero-MAD guard
            assert np.isnan(w[c.x == 0]).all(), c.name                        # 0 / 0; NaN is no outlier and stays


def test_numpy_leaves_the_sign_of_a_zero_median_to_nobody(cases):
    """np.median is np.mean of the middle value(s) and np.mean's sum starts from +0.0: a median that is a zero is +0.0 whatever the
    signs and the order of the zeros in the read.  A case whose median or MAD changes bits under a permutation would be compared
    with the sign of exact zeros masked (tests/test_float_edges.py); only the signed-zero class may hold such a case, and with
    this numpy none does - the device has to give +0.0 too."""
    for dt in F.DTYPES:
        free = [c for c in cases[dt] if F.zero_sign_free(c.x)]
        assert all(c.cls == "zero" for c in free), [c.name for c in free]
        zero_median = [c for c in cases[dt] if F.stats(c.x)[0] == 0]
        assert len(zero_median) >= 20 and any(c.prop == "median_neg_zero" for c in zero_median)
        for c in zero_median:
            if not F.zero_sign_free(c.x):
                med, mad = F.stats(c.x)[:2]
                assert not np.signbit(med) and not np.signbit(mad), c.name
