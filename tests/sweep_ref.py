"""Reference side of the offline evaluation sweep (riser_amd/evaluate.py, csrc/polya_coords.hip): own numpy mirrors of the two
rules the reference's script applies per read, so that the GPU tests can ask for cases no fixture holds.

  * `polya_coords`: the window rule of riser/test.py:80-117 in plain numpy / float64.  tests/test_sweep_cpu.py holds it equal
    to tests/golden/polya_coords.npz (the script's own answers) on every read and row: that pins the mirror to the reference.
  * `pairs`: the trim and the prefix lengths of riser/test.py:190-211.
"""
import numpy as np

from riser_amd import synth


def polya_coords(signal, resolution: int, mad_threshold: int):
    """-> (start, end), -1 for none.  Every window's numbers at once, then the two first-match picks: a window's conditions
    depend on the window and the 2 R samples before it only, and a start is never index 0 (the change of the first three
    windows is 0 or nan), so `not polyA_start` never re-opens one."""
    x = np.asarray(signal)
    R = int(resolution)
    nw = x.shape[0] // R
    if nw == 0:
        return -1, -1
    win = x[: nw * R].reshape(nw, R)
    med = np.median(win, axis=1)                                       # float64; an even R: the mean of the two middles
    mad = np.median(np.abs(win - med[:, None]), axis=1)
    sums = win.sum(axis=1, dtype=np.int64)
    mean = sums.astype(np.float64) / R
    rolling = mean.copy()
    if nw > 3:                                                         # i > 2 R, strictly
        rolling[3:] = (sums[1:-2] + sums[2:-1]).astype(np.float64) / (2 * R)
    with np.errstate(divide="ignore", invalid="ignore"):
        change = (mean - rolling) / rolling * 100
        is_start = (change > 20) & (mad <= mad_threshold)
    is_end = mad > 20                                                  # the script's literal, not the threshold
    s = np.flatnonzero(is_start)
    if s.size == 0:
        return -1, -1
    e = np.flatnonzero(is_end[s[0]:])
    return int(s[0]) * R, (int(s[0] + e[0]) * R if e.size else -1)


def polya_coords_batch(signals, resolution, mad_threshold):
    got = [polya_coords(s, resolution, mad_threshold) for s in signals]
    return (np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int32))


def pairs(read_lens, ends, lengths, fixed_trim, already_trimmed=False):
    """-> [(read, k, first sample, length)] in (read, length) order, read by read as the script goes."""
    out = []
    for n, (total, end) in enumerate(zip(read_lens, ends)):
        trim = 0 if already_trimmed else (int(end) + 1 if end > 0 else int(fixed_trim))
        left = max(int(total) - trim, 0)
        for k, L in enumerate(lengths):
            if left >= L:
                out.append((n, k, trim, int(L)))
    return out


# ---- the reads of the fixtures, rebuilt from their seeds ------------------------------------------------------------------
def coords_reads(g):
    """the 36 reads of tests/golden/polya_coords.npz and its group at negative levels"""
    seed, n = int(g["seed"]), int(g["n_reads"])
    reads = [synth.make_raw_read(seed, rid, 6000 + 523 * rid, rid % 4 != 3) for rid in range(n)]
    neg = [(r.astype(np.int32) - int(g["neg_shift"])).astype(np.int16) for r in reads]
    return reads + [s for _, s in synth.polya_edge_cases()], neg


def sweep_reads(g):
    seed, n = int(g["seed"]), int(g["n_reads"])
    return [synth.make_raw_read(seed, rid, 7000 + 911 * rid, rid % 4 != 3) for rid in range(n)]
