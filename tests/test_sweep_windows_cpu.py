"""The window table of rs_polya_coords (csrc/polya_coords.hip: one (sum, 4 x MAD) per window) without a GPU: the exact integer
reference `window_table` of tests/sweep_ref.py against np.median in float64 and, through `scan_table`, against the reference
script's own answers; the numpy model of the device's two-level counting select against `window_table`; which of the select's
paths the designed windows of tests/sweep_ref.py reach at every resolution; and seven defects put into the model, each of which
the designed windows must notice at every resolution where it can show (tests/test_sweep_windows.py runs the same windows
through the kernel).  All comparisons are of integers: no tolerance anywhere."""
import os

import numpy as np
import pytest

from tests import sweep_ref as R

BIG = [r for r in R.RESOLUTIONS if r >= 4]
ODD = "an odd R has one middle rank (k0 == k1): "
# (mutant, R) -> why no window of R samples can show it; test_the_not_applicable_table_is_honest holds every entry to zero catches
NOT_APPLICABLE = {}
for _r in R.RESOLUTIONS:
    if _r % 2:
        NOT_APPLICABLE[("upper_at_k0", _r)] = ODD + "the upper middle is at k0"
        NOT_APPLICABLE[("straddle_ignored", _r)] = ODD + "nothing straddles"
        NOT_APPLICABLE[("parity_dropped", _r)] = ODD + "med2 is twice a sample, even"
        NOT_APPLICABLE[("med2_halved", _r)] = ODD + "med2 is twice a sample, med2 // 2 the median itself"
    if _r % 64 == 0:
        NOT_APPLICABLE[("sum_drops_partial_stride", _r)] = "R is a multiple of 64: no partial stride"
NOT_APPLICABLE[("bias_dropped", 1)] = "one sample is its own median in any order"
NOT_APPLICABLE[("bias_dropped", 2)] = "med2 is the sum of both samples in any order"
NOT_APPLICABLE[("med2_halved", 2)] = "both deviations are |a - b|; from med2 - 1 they are |a - b| - 1 and |a - b| + 1, the same sum"
NOT_APPLICABLE[("rank_not_rebased", 1)] = "the only rank is 0, inside its bin as well"

_cache = {}


def designed(res):
    """-> (names, windows [n, R] int16, the table of the windows, the unmutated model's answers and paths), once per R"""
    if res not in _cache:
        reads, names = R.designed_reads(res)
        wins = np.stack([r[w * res:(w + 1) * res] for r, nm in zip(reads, names) for w in range(len(nm))])
        flat = [n for nm in names for n in nm]
        assert wins.shape == (sum(R.designed_window_counts(res)), res) and len(flat) == wins.shape[0]
        assert [len(n) for n in names] == list(R.designed_window_counts(res)) and max(len(r) for r in reads) <= 4 * 16384
        assert res in (1, 16384) or all(len(r) % res for r in reads)   # ragged tails (4 x 16384 samples leave no room for one)
        table = np.stack(R.window_table(wins.reshape(-1), res), axis=1)
        model = [R.select_model(w) for w in wins]
        _cache[res] = (flat, wins, table, model)
    return _cache[res]


def random_windows(res, n=24):
    rng = np.random.default_rng([7, res])
    return np.concatenate([rng.integers(-32768, 32768, (n, res)), np.round(rng.normal(470, 25, (n, res))).astype(np.int64),
                           rng.integers(-3, 4, (n, res)), -32768 + rng.integers(0, 300, (n, res))]).astype(np.int16)


@pytest.mark.parametrize("res", R.RESOLUTIONS)
def test_window_table_is_np_median_in_float64(res):
    wins = np.concatenate([designed(res)[1], random_windows(res)])
    sums, med2, mad4 = R.window_table(wins.reshape(-1), res)
    assert sums.dtype == med2.dtype == mad4.dtype == np.int64 and sums.shape == (wins.shape[0],)
    med = np.median(wins.astype(np.float64), axis=1)
    mad = np.median(np.abs(wins.astype(np.float64) - med[:, None]), axis=1)
    assert np.array_equal(med2.astype(np.float64), 2 * med) and np.array_equal(mad4.astype(np.float64), 4 * mad)
    assert np.array_equal(sums, wins.astype(np.int64).sum(axis=1))
    assert not (mad4 & 1).any()                                        # the MAD comes in half steps only
    # a ragged tail shorter than R is no window
    tail = R.window_table(np.concatenate([wins.reshape(-1), wins[0, : res - 1]]), res)
    assert all(np.array_equal(a, b) for a, b in zip(tail, (sums, med2, mad4)))
    assert all(a.shape == (0,) for a in R.window_table(wins[0, : res - 1], res))


def test_the_alphabet_windows_are_all_there():
    for res in (1, 2, 3):
        wins = designed(res)[1]
        assert len({tuple(w) for w in wins.tolist()}) == len(R.ALPHABET) ** res
        assert set(np.unique(wins).tolist()) == set(R.ALPHABET)


def test_scan_of_the_table_reproduces_the_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "polya_coords.npz"))
    reads, neg = R.coords_reads(g)
    for group, rows, starts, ends in ((reads, g["rows"], g["starts"], g["ends"]), (neg, g["neg_rows"], g["neg_starts"], g["neg_ends"])):
        for k, (res, thr) in enumerate(rows):
            tables = [R.window_table(r, int(res)) for r in group]
            got = [R.scan_table(sums, mad4, int(res), int(thr)) for sums, _, mad4 in tables]
            assert [s for s, _ in got] == starts[k].tolist() and [e for _, e in got] == ends[k].tolist(), (res, thr)
    assert R.scan_table(np.zeros(0), np.zeros(0), 500, 20) == (-1, -1)


@pytest.mark.parametrize("res", R.RESOLUTIONS)
def test_select_model_equals_the_table(res):
    _, wins, table, model = designed(res)
    got = np.array([m[:3] for m in model], dtype=np.int64)
    assert np.array_equal(got, table), np.flatnonzero((got != table).any(axis=1))[:10]
    extra = random_windows(res, 3)
    assert np.array_equal(np.array([R.select_model(w)[:3] for w in extra]), np.stack(R.window_table(extra.reshape(-1), res), axis=1))
    for m in model:
        assert 0 <= m[3]["mad"]["hi0"] <= m[3]["mad"]["hi1"] <= 127    # |x - median| is below 2^15: the MAD select stays in bins 0 ... 127


@pytest.mark.parametrize("res", BIG)
def test_designed_windows_reach_every_path_of_the_select(res):
    names, _, _, model = designed(res)
    med = [m[3]["med"] for m in model]
    mad = [m[3]["mad"] for m in model]
    combos = {(a["straddle"], b["straddle"]) for a, b in zip(med, mad)}
    if res % 2:
        assert combos == {(False, False)}                              # one middle rank: nothing straddles, whatever the window
    else:
        assert combos == {(True, False), (False, True), (True, True), (False, False)}
        assert any(p["straddle"] and p["r0"] == p["n0"] - 1 and p["r1"] == 0 for p in mad)
    one_bin = [p for p in med if not p["straddle"]]
    assert any(p["r0"] == 0 for p in one_bin) and any(p["r1"] == p["n1"] - 1 for p in one_bin)
    assert any(p["r0"] == 0 and p["n0"] > 1 for p in one_bin) and any(p["r1"] == p["n1"] - 1 and p["n1"] > 1 for p in one_bin)
    assert any(p["hi0"] == 0 for p in med) and any(p["hi1"] == 255 for p in med)
    assert any(p["hi1"] == 127 for p in mad)                           # the highest bin the MAD select can choose
    assert len(set(names)) == min(len(names), len(R.FAMILIES))
    print(f"SELECT_PATHS R={res}: {len(model)} windows, median straddles {sum(p['straddle'] for p in med)}, "
          f"MAD straddles {sum(p['straddle'] for p in mad)}, both {sum(a['straddle'] and b['straddle'] for a, b in zip(med, mad))}, "
          f"median bins {min(p['hi0'] for p in med)} ... {max(p['hi1'] for p in med)}, MAD bins up to {max(p['hi1'] for p in mad)}")


def catches(mutant, res):
    """the designed windows whose (sum, 4 MAD) the defect changes: the two numbers the device's table holds, not med2"""
    _, wins, table, _ = designed(res)
    return sum(R.select_model(w, mutant)[:3:2] != (int(row[0]), int(row[2])) for w, row in zip(wins, table))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_designed_windows_catch_the_mutant(mutant):
    """a defect put into the model must move (sum, 4 MAD) of at least one designed window at every resolution where it
    can show at all; the counts are in profiles/sweep_windows_gpu_tests.txt"""
    for res in R.RESOLUTIONS:
        if (mutant, res) in NOT_APPLICABLE:
            continue
        n = catches(mutant, res)
        print(f"MUTANT_CATCH {mutant} R={res}: {n} of {designed(res)[1].shape[0]} designed windows")
        assert n >= 1, (mutant, res)


def test_the_not_applicable_table_is_honest():
    for (mutant, res), reason in NOT_APPLICABLE.items():
        assert mutant in R.MUTANTS and res in R.RESOLUTIONS and reason
        assert catches(mutant, res) == 0, (mutant, res)
        assert all(R.select_model(w, mutant)[:3] == R.select_model(w)[:3] for w in random_windows(res, 2)), (mutant, res)


@pytest.mark.parametrize("res, thr", sorted(R.RIDING))
def test_riding_reads_hold_every_outcome(res, thr):
    """what tests/test_sweep_windows.py asks of its threshold-riding reads, from the mirror alone"""
    reads, expected = R.riding_reads(res, thr)
    st, en = R.polya_coords_batch(reads, res, thr)
    n = len(reads)
    assert 3 * int((st >= 0).sum()) >= n and 4 * int((en >= 0).sum()) >= n and 10 * int(((st < 0) & (en < 0)).sum()) >= n
    for b, want in enumerate(expected):
        assert want is None or (int(st[b]), int(en[b])) == want, (b, want)
    _, _, mad4 = R.window_table(reads[0], res)
    h = 2 if res % 2 == 0 else 4
    assert set(mad4.tolist()) <= {4 * thr - h, 4 * thr, 4 * thr + h, 80, 80 + h}
    assert max(len(r) for r in reads) <= 4 * 16384 or res <= 500
    assert thr <= 20 or any(want is not None and want[0] == want[1] for want in expected)
    assert res > 256 or all(len(r) // res > 64 for r in reads) and any(len(r) // res > 128 for r in reads)
