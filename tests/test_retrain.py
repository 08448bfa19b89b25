"""The retraining preprocessing on the device: rs_retrain_prepare (csrc/retrain_prep.hip) against the reference script's own
answers (tests/golden/retrain.npz), the numpy mirror of tests/retrain_ref.py and the existing float kernel, and
riser_amd.retrain.prepare / the command line against one call.  Everything is bit for bit, NaN equal to NaN."""
import os

import numpy as np
import pytest
import torch

from riser_amd import retrain as T
from tests import retrain_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
BIG = (8000, 12000, 16000)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "retrain.npz"))
    reads, offset, rng, dig = R.build_reads(int(g["seed"]))
    assert R.reads_crc(reads) == int(g["reads_crc"])
    cal = T.as_calibration((offset, rng, dig), len(reads))
    return g, reads, cal, [R.pa(*t) for t in zip(reads, offset, rng, dig)]


def device_prepare(dev, reads, cal, cutoffs, lim, rows=None, lens=None):
    """rs_retrain_prepare on `reads` (int16 with `cal`, or float32 pA with cal None), every read at an ODD sample offset with
    +-32767 in front of and behind it; `rows` / `lens` in place of the natural row maps / true lengths.  Every output has one
    sentinel row behind its last row, and d_stats is sentinel-filled.  -> (outs [rows + 1, cutoff], stats [n_cut, B, 2], rows)"""
    dt = np.int16 if cal is not None else np.float32
    parts, offs, pos = [], [], 0
    for i, r in enumerate(reads):
        fill = 2 if pos % 2 == 1 else 1
        parts.append(np.full(fill, 32767 if i % 2 else -32767, dtype=dt))
        pos += fill
        offs.append(pos)
        parts.append(np.asarray(r, dtype=dt))
        pos += len(r)
    parts.append(np.full(3, 32767, dtype=dt))
    true_lens = np.array([len(r) for r in reads], dtype=np.int64)
    lens = true_lens if lens is None else np.asarray(lens, dtype=np.int64)
    assert (lens <= true_lens).all(), "the test itself would read out of bounds"
    if rows is None:
        rows = T.row_maps(lens, cutoffs)[0]
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    B = len(reads)
    assert rows.shape == (len(cutoffs), B)
    n_rows = [int(rows[c].max()) + 1 for c in range(len(cutoffs))]
    for c, n in enumerate(cutoffs):                                     # a row the kernel writes exists
        assert all(rows[c, b] < n_rows[c] for b in range(B))
    sig = torch.from_numpy(np.concatenate(parts)).to(dev)
    off = torch.from_numpy(np.array(offs, dtype=np.int64)).to(dev)
    ln = torch.from_numpy(lens.astype(np.int32)).to(dev)
    cal_d = torch.from_numpy(np.ascontiguousarray(cal, dtype=np.float64)).to(dev) if cal is not None else None
    rows_d = torch.from_numpy(rows).to(dev)
    outs = [torch.full((max(k, 0) + 1, n), SENTINEL, dtype=torch.float32, device=dev) for k, n in zip(n_rows, cutoffs)]
    stats = torch.full((len(cutoffs), B, 2), SENTINEL, dtype=torch.float64, device=dev)
    T.launch(sig, 2 if cal is not None else 4, off, ln, cal_d, B, list(cutoffs), lim, rows_d, outs, stats)
    torch.cuda.synchronize(dev)
    return [o.cpu().numpy() for o in outs], stats.cpu().numpy(), rows


def assert_rows(outs, stats, rows, want, what=""):
    """outs / stats of device_prepare against the mirror's (rows, kept, stats) per cutoff, under the natural row maps"""
    for c, (o, (w_rows, kept, w_stats)) in enumerate(zip(outs, want)):
        assert o.shape[0] == len(kept) + 1, (what, c)
        assert R.same_bits(o[:-1], w_rows), (what, c, np.flatnonzero([not R.same_bits(a, b) for a, b in zip(o[:-1], w_rows)]))
        assert (o[-1] == np.float32(SENTINEL)).all(), (what, c, "the row behind the output was written")
        skipped = np.ones(stats.shape[1], dtype=bool)
        skipped[kept] = False
        assert np.array_equal(stats[c, kept], w_stats), (what, c)
        assert (stats[c, skipped] == SENTINEL).all(), (what, c)


def noisy_reads(seed, lens, spikes=6, guard_from=None):
    """int16 reads (sums of uniform integers around 500) with a few spikes and runs of spikes; from sample guard_from[i] on
    read i is +-32767, so a kernel that reads a sample too many shifts a median."""
    rng = np.random.default_rng(seed)
    reads = []
    for i, n in enumerate(lens):
        r = (500 + rng.integers(-20, 21, size=(4, n)).sum(axis=0)).astype(np.int16)
        for p in rng.integers(0, n, size=min(spikes, n)):
            w = int(rng.integers(1, 6))
            r[p:p + w] = rng.integers(-3000, 3000, size=len(r[p:p + w]))
        if guard_from is not None:
            r[guard_from[i]:] = np.where(np.arange(n - guard_from[i]) % 2 == 0, 32767, -32767)
        reads.append(r)
    return reads


def calibration(seed, n):
    rng = np.random.default_rng(seed)
    return T.as_calibration((rng.integers(-30, 31, size=n).astype(np.float64), (13000 + rng.integers(0, 3000, size=n)) / 10.0,
                             np.full(n, 8192.0)), n)


def to_pa(reads, cal):
    return [np.array(s * (r + o), dtype=np.float32) for r, (o, s) in zip(reads, cal)]


@pytest.fixture(scope="module")
def ragged():
    """77 reads of 6000 .. 20000 samples at BIG; behind the longest cutoff that applies, and AT every cutoff index, +-32767"""
    rng = np.random.default_rng(20260111)
    lens = rng.integers(6000, 20001, size=77)
    lens[:6] = (8000, 7999, 12000, 16000, 16001, 11999)
    guard = [max([c for c in BIG if c <= n], default=0) for n in lens]
    reads = noisy_reads(11, lens, guard_from=guard)
    for r in reads:
        for c in BIG:
            if c < len(r):
                r[c] = 32767 if c % 16000 else -32767
    cal = calibration(12, len(reads))
    pa = to_pa(reads, cal)
    return reads, cal, pa, R.prepare(pa, BIG, 3.5)


# ---- the script's own answers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["int16", "float32"])
def test_fixtures(dev, golden, form):
    g, reads, cal, pa = golden
    for lim, cutoffs in R.SETS:
        outs, _, _ = device_prepare(dev, reads if form == "int16" else pa, cal if form == "int16" else None, cutoffs, lim)
        for n, o in zip(cutoffs, outs):
            want = g[R.key(lim, n)]
            assert o.shape[0] == want.shape[0] + 1
            bad = [R.NAMES[g[R.key(lim, n) + "_kept"][i]] for i in range(len(want)) if not R.same_bits(o[i], want[i])]
            assert not bad, (form, lim, n, bad)


# ---- the mirror, on what no fixture can hold -------------------------------------------------------------------------------------
def test_ragged_batch_equals_mirror_and_input_forms_agree(dev, ragged):
    reads, cal, pa, want = ragged
    assert [len(w[1]) for w in want] == [sum(len(r) >= c for r in reads) for c in BIG] and len(want[2][1]) < len(want[0][1]) < 77
    outs, stats, rows = device_prepare(dev, reads, cal, BIG, 3.5)
    assert_rows(outs, stats, rows, want, "int16")
    outs_f, stats_f, _ = device_prepare(dev, pa, None, BIG, 3.5)
    assert_rows(outs_f, stats_f, rows, want, "float32")
    for a, b in zip(outs, outs_f):
        assert R.same_bits(a, b)


@pytest.mark.parametrize("cutoffs", [(T.WORKGROUP_THREADS - 1, T.WORKGROUP_THREADS, T.WORKGROUP_THREADS + 1,
                                      4 * T.WORKGROUP_THREADS + 1), (2, 3, 4), (32768,)])
def test_thread_count_edges(dev, cutoffs):
    top = cutoffs[-1]
    lens = [top] if top == 32768 else [top + 5, top, cutoffs[0], cutoffs[1] if len(cutoffs) > 1 else top, 1, top + 100]
    reads = noisy_reads(sum(cutoffs), lens, spikes=4)
    if top == 4:
        reads[0][:] = (400, 900, 500, 510, 505, 400, 300, 200, 100)     # outliers at both ends of a tiny row
    cal = calibration(5, len(reads))
    for lim in (3.5, 1.0):
        outs, stats, rows = device_prepare(dev, reads, cal, cutoffs, lim)
        assert_rows(outs, stats, rows, R.prepare(to_pa(reads, cal), cutoffs, lim), (cutoffs, lim))


def test_solo_equals_batch_and_one_call_equals_three(dev, ragged):
    reads, cal, pa, want = ragged
    pick = [0, 2, 3, 4, 9, 30, 76]
    sub, sub_cal = [reads[i] for i in pick], cal[pick]
    batch, batch_stats, _ = device_prepare(dev, sub, sub_cal, BIG, 3.5)
    for c, n in enumerate(BIG):                                         # one three-cutoff call == three one-cutoff calls
        one, one_stats, _ = device_prepare(dev, sub, sub_cal, (n,), 3.5)
        assert R.same_bits(one[0], batch[c]) and np.array_equal(one_stats[0], batch_stats[c])
    taken = [0, 0, 0]
    for j, i in enumerate(pick):                                        # a read alone == the read in its batch
        solo, solo_stats, _ = device_prepare(dev, [reads[i]], cal[i:i + 1], BIG, 3.5)
        for c, n in enumerate(BIG):
            if len(reads[i]) >= n:
                assert R.same_bits(solo[c][0], batch[c][taken[c]]), (i, n)
                assert np.array_equal(solo_stats[c, 0], batch_stats[c, j])
                taken[c] += 1
            else:
                assert (solo[c] == np.float32(SENTINEL)).all() and (solo_stats[c] == SENTINEL).all()
    assert taken == [b.shape[0] - 1 for b in batch]


def test_rows_mapped_to_minus_one_are_skipped(dev, golden):
    g, reads, cal, pa = golden
    cutoffs, lim = R.SETS[0][1], 3.5
    lens = np.array([len(r) for r in reads])
    rows, kept = T.row_maps(lens, cutoffs)
    # drop every third read that would have a row and send the others to rows in REVERSE order
    new = np.full_like(rows, -1)
    where = []
    for c in range(len(cutoffs)):
        keep = [b for j, b in enumerate(kept[c]) if j % 3 != 1]
        new[c, keep] = np.arange(len(keep))[::-1]
        where.append(keep)
    outs, stats, _ = device_prepare(dev, reads, cal, cutoffs, lim, rows=new)
    for c, n in enumerate(cutoffs):
        want, full_kept = g[R.key(lim, n)], kept[c].tolist()
        assert outs[c].shape[0] == len(where[c]) + 1 and (outs[c][-1] == np.float32(SENTINEL)).all()
        for b in where[c]:
            assert R.same_bits(outs[c][new[c, b]], want[full_kept.index(b)]), (n, R.NAMES[b])
        skipped = np.setdiff1d(np.arange(len(reads)), where[c])
        assert (stats[c, skipped] == SENTINEL).all() and (stats[c, where[c]] != SENTINEL).all()
    # nothing mapped at all: nothing written
    outs, stats, _ = device_prepare(dev, reads, cal, cutoffs, lim, rows=np.full_like(rows, -1))
    assert all((o == np.float32(SENTINEL)).all() for o in outs) and (stats == SENTINEL).all()


# ---- the existing float kernel, wherever the two rules agree -----------------------------------------------------------------------
def test_cross_check_against_the_live_float_kernel(dev):
    from riser_amd.preprocess import Kit, SignalProcessor
    cutoffs = (1000, 1500, 2001)
    reads = noisy_reads(31, [2100] * 64, spikes=5)
    for i in (7, 50):                                                   # exactly 2 zero-MAD reads in 64: > half equal
        reads[i][np.arange(2100) % 5 != 0] = 500
    cal = calibration(32, 64)
    pa = to_pa(reads, cal)
    mads = np.array([[R.mad_normalise(p[:n], 3.5)[2] for p in pa] for n in cutoffs])
    assert ((mads == 0).sum(axis=1) == 2).all() and (mads[:, [7, 50]] == 0).all()
    outs, _, _ = device_prepare(dev, reads, cal, cutoffs, 3.5)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    for c, n in enumerate(cutoffs):
        live = proc.mad_normalise_float_batch([p[:n] for p in pa])
        took_part = 0
        for i in range(64):
            if mads[c, i] != 0:
                assert R.same_bits(outs[c][i], live[i]), (n, i)
                took_part += 1
            else:
                assert not live[i].any() and np.isnan(outs[c][i]).any()       # the two rules differ exactly here
        assert took_part == 62


# ---- prepare and the command line ---------------------------------------------------------------------------------------------------
def test_prepare_sub_batches_equal_one_call(dev, golden):
    g, reads, cal, pa = golden
    assert len(reads) == 17
    cutoffs = list(R.SETS[0][1])
    one = T.prepare(reads, cutoffs, cal, device=dev)
    for res in (T.prepare(reads, cutoffs, cal, device=dev, sub_batch=5), T.prepare(pa, cutoffs, device=dev, sub_batch=5)):
        for a, b in zip(one, res):
            assert a.cutoff == b.cutoff and np.array_equal(a.kept, b.kept) and R.same_bits(a.data, b.data)
    for r in one:
        assert R.same_bits(r.data, g[R.key(3.5, r.cutoff)]) and np.array_equal(r.kept, g[R.key(3.5, r.cutoff) + "_kept"])
    three = T.prepare(reads, cutoffs, (cal[:, 0], cal[:, 1] * 8192.0, np.full(17, 8192.0)), outlier_lim=3.3, device=dev)
    assert three[1].data.shape == (len(g[R.key(3.5, 150) + "_kept"]), 150)


def test_command_line(dev, golden, tmp_path, capsys):
    g, reads, cal, pa = golden
    _, offset, rng, dig = R.build_reads(int(g["seed"]))
    path = tmp_path / "set_a.npz"
    np.savez(path, flat=np.concatenate(reads), lengths=np.array([len(r) for r in reads]),
             read_ids=np.array([f"read{i}" for i in range(len(reads))]), filename=np.array("batch0"),
             offset=offset, range=rng, digitisation=dig)
    assert T.main(["preprocess", "2,3,4", "50", str(path), "--out-dir", str(tmp_path)]) == 0
    said = capsys.readouterr().out.splitlines()
    for n in R.CUTOFFS:
        got = np.load(tmp_path / f"set_a_{n}.npy")
        assert R.same_bits(got, g[R.key(3.5, n)])
        assert f"# of discarded reads (< {n} samples) in batch0: {17 - len(got)}" in said
    assert T.main(["preprocess", "3", "50", str(path), "--out-dir", str(tmp_path), "--outlier-lim", "2.0"]) == 0
    assert R.same_bits(np.load(tmp_path / "set_a_150.npy"), R.prepare(pa, [150], 2.0)[0][0])
