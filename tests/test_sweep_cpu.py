"""The offline evaluation sweep (riser_amd/evaluate.py, rs_polya_coords) without a GPU: the numpy mirror of the window rule
against the reference's own answers, what the fixtures must contain to be worth testing against, the sweep's plan, its trim
and pair rules, the TSV lines, and the C ABI's refusals (all of which happen before a device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

from riser_amd import _native as nv
from riser_amd import evaluate as E
from tests import sweep_ref as R


@pytest.fixture(scope="module")
def lib():
    from riser_amd import build
    build.build()
    return nv.lib()


@pytest.fixture(scope="module")
def coords(golden_dir):
    return np.load(os.path.join(golden_dir, "polya_coords.npz"))


@pytest.fixture(scope="module")
def sweep_g(golden_dir):
    return np.load(os.path.join(golden_dir, "sweep.npz"))


# ---- the mirror is the reference's rule ----------------------------------------------------------------------------------
def test_mirror_equals_reference_on_every_read_and_row(coords):
    reads, neg = R.coords_reads(coords)
    assert len(reads) == 36 and coords["starts"].shape == (12, 36)
    for k, (res, thr) in enumerate(coords["rows"]):
        st, en = R.polya_coords_batch(reads, int(res), int(thr))
        assert np.array_equal(st, coords["starts"][k]) and np.array_equal(en, coords["ends"][k]), (res, thr)
    for k, (res, thr) in enumerate(coords["neg_rows"]):
        st, en = R.polya_coords_batch(neg, int(res), int(thr))
        assert np.array_equal(st, coords["neg_starts"][k]) and np.array_equal(en, coords["neg_ends"][k]), (res, thr)


def test_coords_fixture_holds_every_outcome(coords):
    rows = [tuple(int(v) for v in r) for r in coords["rows"]]
    assert rows == [(500, 20), (250, 20), (501, 20), (333, 12), (1000, 30), (64, 15), (7, 20), (2048, 25), (500, 60), (500, 5),
                    (1, 20), (4096, 40)]
    st, en = coords["starts"], coords["ends"]
    assert not ((st < 0) & (en >= 0)).any()                            # an end needs a start
    assert ((st >= 0) & (en > st)).any() and ((st >= 0) & (en < 0)).any() and ((st < 0) & (en < 0)).any()
    same = (st >= 0) & (st == en)
    assert same[rows.index((1000, 30))].any() and same[rows.index((500, 60))].any()
    for k, row in enumerate(rows):
        assert (en[k] >= 0).any() == (row not in ((1, 20), (4096, 40))), row
    counts = lambda k: (int(((st[k] >= 0) & (en[k] >= 0)).sum()), int(((st[k] >= 0) & (en[k] < 0)).sum()), int((st[k] < 0).sum()))
    assert counts(0) == (23, 1, 12) and counts(4) == (10, 1, 25) and counts(10) == (0, 33, 3) and counts(11) == (0, 1, 35)
    assert (coords["neg_starts"] >= 0).any() and (coords["neg_ends"] >= 0).any()


def test_sweep_fixture_holds_every_outcome(sweep_g):
    for kit, per_read in (("RNA002", [0, 0, 0, 0, 1, 1, 2, 1, 2, 3, 3, 3, 3, 3, 3, 3]),
                          ("RNA004", [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2])):
        probs, ends = sweep_g[f"{kit}_probs"], sweep_g[f"{kit}_ends"]
        K = len(sweep_g[f"{kit}_lengths"])
        n = (~np.isnan(probs[:, :, 0])).sum(axis=1)
        assert n.tolist() == per_read
        assert (n == 0).any() and ((n > 0) & (n < K)).any() and (n == K).any()
        assert int((ends < 0).sum()) == 4 and (ends > 0).any()         # both trim kinds
        assert np.array_equal(np.isnan(probs[:, :, 0]), np.isnan(probs[:, :, 1]))
        ok = ~np.isnan(probs[:, :, 0])
        assert np.abs(probs[ok].sum(axis=1) - 1).max() < 1e-6


# ---- plan, pairs, lines -----------------------------------------------------------------------------------------------
def test_sweep_plan(sweep_g):
    assert E.sweep_plan("RNA002") == {"sampling_hz": 3012, "lengths": [4096, 7108, 10120], "fixed_trim": 6481}
    assert E.sweep_plan("RNA004") == {"sampling_hz": 4000, "lengths": [4096, 8096], "fixed_trim": 4634}
    for kit in ("RNA002", "RNA004"):
        assert E.sweep_plan(kit)["lengths"] == sweep_g[f"{kit}_lengths"].tolist()
        assert E.sweep_plan(kit)["fixed_trim"] == int(sweep_g[f"{kit}_fixed_trim"])
    with pytest.raises(ValueError):
        E.sweep_plan("RNA999")


def test_pair_building():
    lengths, trim = [4096, 8096], 4634
    #        end found     start only    one short of L    exactly L      shorter than the trim   longer
    lens = [3001 + 8096, 4634 + 5000, 2501 + 4095, 2501 + 4096, 3000, 4634 + 9000]
    ends = [3000, -1, 2500, 2500, -1, -1]
    trims, valid = E.build_pairs(lens, ends, lengths, trim)
    assert trims.tolist() == [3001, 4634, 2501, 2501, 4634, 4634]
    assert valid.tolist() == [[True, True], [True, False], [False, False], [True, False], [False, False], [True, True]]
    want = R.pairs(lens, ends, lengths, trim)
    rn, rk = np.nonzero(valid)
    assert [(int(n), int(k), int(trims[n]), lengths[k]) for n, k in zip(rn, rk)] == want
    assert want == [(0, 0, 3001, 4096), (0, 1, 3001, 8096), (1, 0, 4634, 4096), (3, 0, 2501, 4096), (5, 0, 4634, 4096),
                    (5, 1, 4634, 8096)]
    # reads trimmed beforehand: neither the ends nor the fixed length are applied
    trims, valid = E.build_pairs(lens, ends, lengths, trim, already_trimmed=True)
    assert not trims.any() and valid[:, 0].tolist() == [True, True, True, True, False, True]
    assert R.pairs(lens, ends, lengths, trim, True)[0] == (0, 0, 0, 4096)


def test_lines():
    a, b = np.float32(0.1), np.float32(0.9)
    probs = np.full((3, 2, 2), np.nan, dtype=np.float32)
    probs[0] = [[a, b], [np.float32(0.25), np.float32(0.75)]]
    probs[1, 0] = [np.float32(1.0), np.float32(1e-8)]
    valid = ~np.isnan(probs[:, :, 0])
    res = E.SweepResult(np.array([1500, 2000, -1], dtype=np.int32), np.array([3000, -1, -1], dtype=np.int32), [4096, 8096],
                        probs, valid)
    lines = res.lines("m1", "ds", "f.fast5", ["r0", "r1", "r2"])
    assert lines[0] == "m1\tds\tf.fast5\tr0\t1500\t3000\t4096:0.10000000149011612,0.8999999761581421;8096:0.25,0.75\n"
    assert lines[1] == "m1\tds\tf.fast5\tr1\t2000\tNone\t4096:1.0,9.99999993922529e-09\n"
    assert lines[2] == "m1\tds\tf.fast5\tr2\tNone\tNone\t\n"
    assert all(len(ln.rstrip("\n").split("\t")) == 7 for ln in lines)
    res.already_trimmed = True
    assert res.lines("m1", "ds", "f", ["r0", "r1", "r2"])[2] == "m1\tds\tf\tr2\tboostnano\tboostnano\t\n"


# ---- rs_polya_coords refuses before it touches a device ---------------------------------------------------------------
def test_polya_coords_refusals(lib):
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    call = lambda B, max_len, res, ws=1 << 20, sig=p, off=p, ln=p, st=p, en=p, w=p: \
        lib.rs_polya_coords(sig, off, ln, B, max_len, res, 20, st, en, w, ws, None)
    for res in (0, 16385, -1):
        assert call(2, 10000, res) == nv.RS_ERR_ARG
        assert b"rs_polya_coords" in lib.rs_last_error() and b"resolution" in lib.rs_last_error()
    assert call(-1, 10000, 500) == nv.RS_ERR_ARG and b"rs_polya_coords" in lib.rs_last_error()
    assert call(2, -1, 500) == nv.RS_ERR_ARG
    for null in ("sig", "off", "ln", "st", "en", "w"):
        assert call(2, 10000, 500, **{null: None}) == nv.RS_ERR_ARG, null
        assert b"rs_polya_coords: null" in lib.rs_last_error()
    need = lib.rs_polya_coords_workspace_bytes(2, 10000, 500)
    assert need > 0
    assert call(2, 10000, 500, ws=need - 1) == nv.RS_ERR_WORKSPACE and b"rs_polya_coords" in lib.rs_last_error()
    assert call(2, 10000, 500, ws=0) == nv.RS_ERR_WORKSPACE
    # an empty batch is fine, null pointers and all
    assert lib.rs_polya_coords(None, None, None, 0, 0, 500, 20, None, None, None, 0, None) == nv.RS_OK
    assert lib.rs_polya_coords(None, None, None, 0, 0, 0, 20, None, None, None, 0, None) == nv.RS_ERR_ARG


def test_polya_coords_workspace_bytes_monotone(lib):
    f = lib.rs_polya_coords_workspace_bytes
    for res in (1, 7, 500, 16384):
        by_b = [f(B, 70000, res) for B in (1, 2, 3, 64, 1000)]
        ns = sorted({0, 1, res - 1, res, 2 * res, 70000, 200000})
        by_len = [f(16, n, res) for n in ns]
        assert by_b == sorted(by_b) and by_b[0] < by_b[-1] and by_len == sorted(by_len) and by_len[0] < by_len[-1]
        assert all(v >= 16 * (n // res) * 8 for v, n in zip(by_len, ns))
    assert f(0, 70000, 500) == 0 and f(4, 70000, 0) == 0 and f(4, 70000, 16385) == 0 and f(4, -1, 500) == 0
