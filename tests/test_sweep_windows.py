"""The window table of rs_polya_coords on the device.  coords_windows_kernel (csrc/polya_coords.hip) writes one (sum, 4 x MAD)
per window into the caller's workspace and coords_scan_kernel turns the table into (start, end); the scan asks two things of a
MAD only, so tests/test_sweep.py sees a wrong table only where a window sits on a threshold.  Here the table itself is read
back and held to `window_table` of tests/sweep_ref.py - integers, no tolerance - on the designed windows that
tests/test_sweep_windows_cpu.py shows to reach every path of the kernel's select and to notice seven defects of it, at every
resolution where the launch changes form; and (start, end) to the mirror on reads whose windows ride the rule's thresholds."""
import numpy as np
import pytest
import torch

from riser_amd import _native as nv
from tests import sweep_ref as R
from tests.sweep_dev import device_scan

pytestmark = pytest.mark.gpu

PATTERN = 0xA5                                                         # no entry looks like it: |sum| <= 2^29
PATTERN_I32 = int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
SLACK = 256                                                            # bytes behind the workspace that must stay untouched


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def proc(dev):
    from riser_amd.preprocess import Kit, SignalProcessor
    return SignalProcessor(Kit.create_from_version("RNA004"), device=dev)


def exact_table(dev, reads, res, thr, lens=None, max_len=None):
    """one call on a workspace full of PATTERN -> (starts, ends, table): every window a read has equals `window_table`, every
    other entry and every byte behind rs_polya_coords_workspace_bytes still holds the pattern, and (start, end) is
    `scan_table` of the device's own row"""
    claimed = [len(r) for r in reads] if lens is None else [int(n) for n in lens]
    cut = max(max(claimed), 0) if max_len is None else int(max_len)
    need = int(nv.lib().rs_polya_coords_workspace_bytes(len(reads), cut, res))
    ws = torch.full((need + SLACK,), PATTERN, dtype=torch.uint8, device=dev)
    st, en, tab = device_scan(dev, reads, res, thr, lens=lens, max_len=cut, ws=ws, table=True)
    assert tab.shape == (len(reads), cut // res, 2)
    assert (ws[tab.size * 4:].cpu().numpy() == PATTERN).all(), "bytes behind the table were written"
    for b, r in enumerate(reads):
        sums, _, mad4 = R.window_table(r[: min(max(claimed[b], 0), cut)], res)
        nw = sums.shape[0]
        assert np.array_equal(tab[b, :nw, 0], sums), (res, b, np.flatnonzero(tab[b, :nw, 0] != sums)[:8])
        assert np.array_equal(tab[b, :nw, 1], mad4), (res, b, np.flatnonzero(tab[b, :nw, 1] != mad4)[:8])
        assert (tab[b, nw:] == PATTERN_I32).all(), (res, b, "an entry of a window the read does not have was written")
        assert (int(st[b]), int(en[b])) == R.scan_table(tab[b, :nw, 0], tab[b, :nw, 1], res, thr), (res, thr, b)
    return st, en, tab


@pytest.mark.parametrize("res", R.RESOLUTIONS)
def test_window_table_is_exact(dev, proc, res):
    reads, names = R.designed_reads(res)
    assert [len(n) for n in names] == list(R.designed_window_counts(res)) and max(len(r) for r in reads) <= 4 * 16384
    for thr in (20, 3):
        st, en, _ = exact_table(dev, reads, res, thr)
        wst, wen = R.polya_coords_batch(reads, res, thr)
        assert np.array_equal(st, wst) and np.array_equal(en, wen), (res, thr)
        if (res, thr) == (500, 20):
            assert np.array_equal(en, proc.get_polyA_end_batch(reads))     # the live detector, rs_polya_end


@pytest.mark.parametrize("res", [4, 65, 500, 3585])
def test_table_does_not_depend_on_the_batch(dev, res):
    reads, _ = R.designed_reads(res)
    _, _, batch = exact_table(dev, reads, res, 20)
    nws = [len(r) // res for r in reads]
    for b, r in enumerate(reads):
        _, _, alone = exact_table(dev, [r], res, 20)
        assert np.array_equal(alone[0, :nws[b]], batch[b, :nws[b]]), (res, b)
    _, _, rev = exact_table(dev, reads[::-1], res, 20)
    cut = 2 * res + res // 2                                           # mid-window: two windows of every read that has them
    _, _, short = exact_table(dev, reads, res, 20, max_len=cut)
    far = [len(r) * 10 if len(r) >= cut else len(r) for r in reads]    # a d_len beyond max_len is scanned as max_len
    assert any(n > len(r) for n, r in zip(far, reads))
    _, _, claimed = exact_table(dev, reads, res, 20, lens=far, max_len=cut)
    for b, nw in enumerate(nws):
        assert np.array_equal(rev[len(reads) - 1 - b, :nw], batch[b, :nw]), (res, b)
        assert np.array_equal(short[b, :min(nw, 2)], batch[b, :min(nw, 2)]), (res, b)
        assert np.array_equal(claimed[b], short[b]), (res, b)


@pytest.mark.parametrize("res, thr", sorted(R.RIDING))
def test_threshold_riding_windows(dev, proc, res, thr):
    reads, expected = R.riding_reads(res, thr)
    wst, wen = R.polya_coords_batch(reads, res, thr)
    n = len(reads)
    assert 3 * int((wst >= 0).sum()) >= n and 4 * int((wen >= 0).sum()) >= n and 10 * int(((wst < 0) & (wen < 0)).sum()) >= n
    for b, want in enumerate(expected):                                # a start in lane 63 that ends in lane 0 of the next trip
        assert want is None or (int(wst[b]), int(wen[b])) == want, (b, want)
    assert thr <= 20 or any(want is not None and want[0] == want[1] for want in expected)
    assert res > 256 or all(len(r) // res > 64 for r in reads) and any(len(r) // res > 128 for r in reads)
    st, en, _ = exact_table(dev, reads, res, thr)
    assert np.array_equal(st, wst) and np.array_equal(en, wen), (res, thr, np.flatnonzero((st != wst) | (en != wen))[:10])
    print(f"RIDING R={res} thr={thr}: {n} reads, {int((wst >= 0).sum())} with a start, {int((wen >= 0).sum())} with an end, "
          f"{int(((wst >= 0) & (wen // res // 64 != wst // res // 64) & (wen >= 0)).sum())} end in a later trip than they start")
    if (res, thr) == (500, 20):
        assert np.array_equal(en, proc.get_polyA_end_batch(reads))         # the live detector, rs_polya_end
