"""The retraining preprocessing (riser_amd/retrain.py, rs_retrain_prepare) without a GPU: the numpy mirror against the
reference scripts' own answers, what the fixture must contain to be worth testing against, the row maps, the balanced
tensor writer, the command line, and the C ABI's refusals (all of which happen before a device is touched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from riser_amd import _native as nv
from riser_amd import retrain as T
from tests import retrain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from riser_amd import build
    build.build()
    return nv.lib()


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "retrain.npz"))


@pytest.fixture(scope="module")
def cases(g):
    reads, offset, rng, dig = R.build_reads(int(g["seed"]))
    assert R.reads_crc(reads) == int(g["reads_crc"])                   # the generator still draws what the fixture was made of
    return reads, offset, rng, dig, [R.pa(*t) for t in zip(reads, offset, rng, dig)]


def _row(g, lim, cutoff, name):
    kept = g[R.key(lim, cutoff) + "_kept"].tolist()
    return g[R.key(lim, cutoff)][kept.index(R.NAMES.index(name))]


# ---- the mirror is the script's arithmetic ---------------------------------------------------------------------------------
def test_mirror_equals_reference(g, cases):
    sig = cases[4]
    assert [float(v) for v in g["limits"]] == [s[0] for s in R.SETS]
    for k, (lim, cutoffs) in enumerate(R.SETS):
        assert tuple(g[f"cutoffs_{k}"].tolist()) == cutoffs
        for n, (rows, kept, _) in zip(cutoffs, R.prepare(sig, cutoffs, lim)):
            assert g[R.key(lim, n)].dtype == np.float32 and g[R.key(lim, n)].shape == (len(kept), n)
            assert np.array_equal(kept, g[R.key(lim, n) + "_kept"]), (lim, n)
            assert R.same_bits(rows, g[R.key(lim, n)]), (lim, n)


def test_fixture_holds_every_quirk(g, cases):
    reads, offset, rng, dig, sig = cases
    assert R.SETS[0] == (3.5, R.CUTOFFS) and sorted(s[0] for s in R.SETS) == [2.0, 3.3, 3.5]
    assert float(np.float32(3.3)) != 3.3                                     # a limit that is no float32 value
    assert {n % 2 for _, cs in R.SETS for n in cs} == {0, 1}            # even and odd n
    lens = [len(r) for r in reads]
    c0, c1, c2 = R.CUTOFFS
    assert any(n < c0 for n in lens) and any(c0 < n < c1 for n in lens) and any(c1 < n < c2 for n in lens)
    assert all(c in lens for c in R.CUTOFFS) and any(n > c2 for n in lens)
    for c in R.CUTOFFS:
        assert g[R.key(3.5, c) + "_kept"].tolist() == [i for i, n in enumerate(lens) if n >= c]
        # all samples equal: 0 / 0 everywhere
        assert np.isnan(_row(g, 3.5, c, "all_equal")).all()
        # more than half equal plus spikes, one at index 0: NaN, inf and +-lim in one row
        z = _row(g, 3.5, c, "zero_mad_mix")
        assert np.isnan(z).any() and np.isinf(z).any() and (z == np.float32(3.5)).any() and (z == np.float32(-3.5)).any()
        assert np.isinf(z[0])
        assert R.mad_normalise(sig[R.NAMES.index("zero_mad_mix")][:c], 3.5)[2] == 0
        # outliers at 0 and 1: index 0 takes the unclipped y[1]
        assert abs(_row(g, 3.5, c, "outliers_0_1")[0]) > 3.5
    # no other row has a zero MAD, so NaN and inf come from the two reads built for it
    for lim, cs in R.SETS:
        for c in cs:
            bad = ~np.isfinite(g[R.key(lim, c)]).all(axis=1)
            assert set(g[R.key(lim, c) + "_kept"][bad].tolist()) == {R.NAMES.index("all_equal"), R.NAMES.index("zero_mad_mix")}

    def outliers(name, n, lim=3.5):
        x = sig[R.NAMES.index(name)][:n]
        med = np.median(x)
        y = (x - med) / (np.float32(1.4826) * np.median(np.abs(x - med)))
        return np.abs(y) > np.float32(lim)

    def runs(mask):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
        return list(zip(edges[::2], edges[1::2]))                       # [start, end)

    # a spike at index c - 1: the last element of one row, interior in the longer ones
    for c in R.CUTOFFS:
        assert outliers("spike_at_each_cutoff_end", c)[c - 1] and outliers("spike_at_each_cutoff_end", 260)[c - 1]
    assert outliers("spike_at_each_cutoff_end", 101, 2.0)[100] and outliers("spike_at_each_cutoff_end", 151, 3.3)[150]
    # a run of three or more, and runs across the 100 and 150 boundaries
    r200 = runs(outliers("runs", 200))
    assert any(e - s >= 3 for s, e in r200)
    assert any(s < 100 < e for s, e in r200) and any(s < 150 < e for s, e in r200)
    # a run longer than 64
    assert max(e - s for s, e in runs(outliers("run_of_66", 200))) > 64
    # heavy ties; negative and mixed-sign pA
    assert len(np.unique(sig[R.NAMES.index("heavy_ties")])) <= 5
    assert (sig[R.NAMES.index("negative_pa")] < 0).all()
    m = sig[R.NAMES.index("mixed_sign")]
    assert (m < 0).any() and (m > 0).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "retrain.npz")) < 64 * 1024


# ---- host side of prepare ----------------------------------------------------------------------------------------------------
def test_row_maps_and_kept_indices():
    lens = [8000, 7999, 16000, 12000, 11999, 20000, 2, 12001]
    rows, kept = T.row_maps(lens, [8000, 12000, 16000])
    assert rows.dtype == np.int64 and rows.shape == (3, 8)
    assert rows.tolist() == [[0, -1, 1, 2, 3, 4, -1, 5], [-1, -1, 0, 1, -1, 2, -1, 3], [-1, -1, 0, -1, -1, 1, -1, -1]]
    assert [k.tolist() for k in kept] == [[0, 2, 3, 4, 5, 7], [2, 3, 5, 7], [2, 5]]
    rows, kept = T.row_maps([5, 5], [6])
    assert rows.tolist() == [[-1, -1]] and kept[0].size == 0
    assert T.cutoffs_for(4, 3012) == [12048] and T.cutoffs_for([2, 3, 4], 4000) == [8000, 12000, 16000]
    for bad in ([], [100, 100], [150, 100], [1, 5], [5, 32769]):
        with pytest.raises(ValueError):
            T.check_cutoffs(bad)
    assert T.check_cutoffs([2, 32768]) == [2, 32768]


def test_prepare_without_reads_or_device():
    # nothing reaches the cutoff: the result is shaped (0, cutoff) and no device is needed
    res = T.prepare([np.zeros(50, dtype=np.int16)], [100, 150], calibration=np.array([[1.0, 0.2]]))
    assert [(r.cutoff, r.data.shape, r.data.dtype, r.kept.tolist()) for r in res] == \
        [(100, (0, 100), np.float32, []), (150, (0, 150), np.float32, [])]
    assert T.prepare([], [100])[0].data.shape == (0, 100)
    with pytest.raises(TypeError):
        T.prepare([np.zeros(200, dtype=np.float64)], [100])             # pA must be float32
    with pytest.raises(TypeError):
        T.prepare([np.zeros(200, dtype=np.int16)], [100])               # raw reads need a calibration
    with pytest.raises(ValueError):
        T.prepare([np.zeros(200, dtype=np.int16)], [100], calibration=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        T.prepare([np.zeros(200, dtype=np.float32)], [10, 20, 30, 40, 50])


def test_calibration_forms():
    off, rng, dig = np.array([3.0, -7.0]), np.array([1437.3, 1402.9]), np.array([8192.0, 2048.0])
    cal = T.as_calibration((off, rng, dig), 2)
    assert cal.dtype == np.float64 and np.array_equal(cal[:, 0], off) and np.array_equal(cal[:, 1], rng / dig)
    assert np.array_equal(T.as_calibration(cal, 2), cal)


# ---- write_tensors -------------------------------------------------------------------------------------------------------------
def test_write_tensors_against_the_script(g, tmp_path):
    pos, neg = R.write_tensor_inputs(g)
    assert pos.dtype == np.float32 and neg.dtype == np.float64 and len(pos) > len(neg) == 7
    p, n = T.write_tensors(pos, neg, str(tmp_path))
    for t, name, want in ((p, "positive.pt", g["wt_positive"]), (n, "negative.pt", g["wt_negative"])):
        back = torch.load(os.path.join(tmp_path, name), weights_only=True)
        assert back.dtype == torch.float32 and tuple(back.shape) == want.shape == (7, 100)
        assert R.same_bits(back.numpy(), want) and R.same_bits(t.numpy(), want)
    # the negative set is the longer one: it is cut
    p, n = T.write_tensors(neg, pos, str(tmp_path))
    assert tuple(p.shape) == tuple(n.shape) == (7, 100) and R.same_bits(n.numpy(), pos[:7])


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_command_line_parsing_and_file_names():
    a = T.parse_args(["preprocess", "2,3,4", "4000", "/data/run7/reads_a.npz", "--out-dir", "/tmp/o"])
    assert (a.command, a.n_secs, a.freq, a.cutoffs, a.name, a.outlier_lim) == \
        ("preprocess", [2, 3, 4], 4000, [8000, 12000, 16000], "reads_a", 3.5)
    assert T.output_paths(a.out_dir, a.name, a.cutoffs) == ["/tmp/o/reads_a_8000.npy", "/tmp/o/reads_a_12000.npy",
                                                            "/tmp/o/reads_a_16000.npy"]
    a = T.parse_args(["preprocess", "4", "3012", "x.npz", "--outlier-lim", "2.5"])
    assert (a.cutoffs, a.out_dir, a.outlier_lim, a.name) == ([12048], ".", 2.5, "x")
    a = T.parse_args(["write-tensors", "p.npy", "n.npy", "out"])
    assert (a.command, a.pos_npy, a.neg_npy, a.out_dir) == ("write-tensors", "p.npy", "n.npy", "out")
    for bad in (["preprocess", "2,2", "4000", "x.npz"], ["preprocess", "9", "4000", "x.npz"], ["preprocess", "x", "1", "x.npz"],
                ["preprocess", "2", "4000"], ["train"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_load_reads(tmp_path):
    flat = np.arange(10, dtype=np.int16)
    base = dict(flat=flat, lengths=np.array([4, 6]), read_ids=np.array(["a", "b"]), filename=np.array("f0"))
    np.savez(tmp_path / "raw.npz", offset=np.array([1.0, 2.0]), range=np.array([1400.0, 1500.0]),
             digitisation=np.array([8192.0, 8192.0]), **base)
    sig, cal, ids, fn = T.load_reads(str(tmp_path / "raw.npz"))
    assert [s.tolist() for s in sig] == [[0, 1, 2, 3], [4, 5, 6, 7, 8, 9]] and ids == ["a", "b"] and fn == "f0"
    assert cal.tolist() == [[1.0, 1400.0 / 8192.0], [2.0, 1500.0 / 8192.0]]
    np.savez(tmp_path / "nocal.npz", **base)
    with pytest.raises(ValueError):
        T.load_reads(str(tmp_path / "nocal.npz"))
    np.savez(tmp_path / "pa.npz", **{**base, "flat": flat.astype(np.float64)})
    sig, cal, _, _ = T.load_reads(str(tmp_path / "pa.npz"))
    assert cal is None and sig[1].dtype == np.float32


# ---- rs_retrain_prepare refuses before it touches a device -------------------------------------------------------------------
def test_refusals(lib):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def call(elem=2, B=2, cuts=(100, 150, 200), n_cut=None, lim=3.5, sig=p, off=p, ln=p, cal=p, rows=p, out="ok", null_cuts=False):
        arr = (C.c_int32 * max(len(cuts), 1))(*cuts)
        outs = None if out is None else (C.c_void_p * 4)(*([p] * 4 if out == "ok" else out))
        rc = lib.rs_retrain_prepare(sig, elem, off, ln, cal, B, None if null_cuts else arr, len(cuts) if n_cut is None else n_cut,
                                    lim, rows, outs, None, None)
        return rc, lib.rs_last_error()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == nv.RS_ERR_ARG and b"rs_retrain_prepare" in msg and word in msg, (kw, msg)

    for elem in (0, 1, 3, 8):
        refused(b"element size", elem=elem)
    refused(b"cutoffs", cuts=(), n_cut=0)
    refused(b"cutoffs", cuts=(10, 20, 30, 40, 50))
    refused(b"cutoffs", n_cut=-1)
    refused(b"cutoffs", null_cuts=True)
    refused(b"ascending", cuts=(100, 100))
    refused(b"ascending", cuts=(100, 150, 120))
    refused(b"outside", cuts=(1, 100))
    refused(b"outside", cuts=(0,))
    refused(b"outside", cuts=(-5, 100))
    refused(b"outside", cuts=(100, 32769))
    refused(b"negative B", B=-1)
    for lim in (-0.5, float("inf"), float("-inf"), float("nan")):
        refused(b"limit", lim=lim)
    for null in ("sig", "off", "ln", "rows"):
        refused(b"null", **{null: None})
    refused(b"null", out=None)
    refused(b"null output", out=[p, None, p, p])
    refused(b"calibration", cal=None)
    # float32 input needs no calibration; none of these launches (B == 0), null pointers and all
    assert call(elem=4, B=0, cal=None, sig=None, off=None, ln=None, rows=None, out=None)[0] == nv.RS_OK
    assert call(B=0, cuts=(2, 32768), lim=0.0)[0] == nv.RS_OK
    assert call(B=0, cuts=(100, 100))[0] == nv.RS_ERR_ARG               # an empty batch is still checked


# ---- header, export list and binding agree ---------------------------------------------------------------------------------------
def test_header_exports_binding_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "riser_amd.h")).read()
    assert "rs_retrain_prepare" in nv.SYMBOLS and hasattr(lib, "rs_retrain_prepare")
    decl = re.search(r"RS_API int rs_retrain_prepare\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == len(lib.rs_retrain_prepare.argtypes) == 13
    assert lib.rs_retrain_prepare.argtypes[8] is C.c_float and "float outlier_lim" in decl
    before = hdr[: hdr.index("RS_API int rs_retrain_prepare(")]
    assert before.rindex("rs_polya_coords(") < before.rindex("Added after ABI 2.9, rs_version unchanged")
    assert re.search(r"^\s*rs_\*;", open(os.path.join(ROOT, "riser_amd", "csrc", "exports.map")).read(), flags=re.M)
    from riser_amd import build
    assert "retrain_prep.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "riser_amd", "csrc", "retrain_prep.hip")).read()
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) == T.WORKGROUP_THREADS
    assert int(re.search(r"constexpr int kMaxCutoff = (\d+);", src).group(1)) == T.MAX_CUTOFF
    assert int(re.search(r"constexpr int kMaxCutoffs = (\d+);", src).group(1)) == T.MAX_CUTOFFS
    import riser_amd
    assert riser_amd.retrain is T
