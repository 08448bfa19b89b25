"""Reference side of the offline evaluation sweep (riser_amd/evaluate.py, csrc/polya_coords.hip): own numpy mirrors of the two
rules the reference's script applies per read, so that the GPU tests can ask for cases no fixture holds.

  * `polya_coords`: the window rule of riser/test.py:80-117 in plain numpy / float64.  tests/test_sweep_cpu.py holds it equal
    to tests/golden/polya_coords.npz (the script's own answers) on every read and row: that pins the mirror to the reference.
  * `pairs`: the trim and the prefix lengths of riser/test.py:190-211.
  * `window_table` / `scan_table`: the (sum, twice the median, four times the MAD) of every window by sorting in int64, and the
    rule applied to such a table - what the device's window table is held to, entry by entry (tests/test_sweep_windows.py).
  * `select_model`: a numpy model of the device's two-level counting select that records the path a window takes and accepts
    defects (`MUTANTS`); `designed_reads` / `riding_reads`: the inputs built for that table, from a seed.
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
    return _scan(win.sum(axis=1, dtype=np.int64), mad, R, mad_threshold)


def _scan(sums, mad, R, mad_threshold):
    """the rule on every window's (sum, MAD in float64) at once"""
    nw = sums.shape[0]
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


# ---- the window table of csrc/polya_coords.hip, exactly ---------------------------------------------------------------------
def window_table(signal, R: int):
    """-> (sums, med2, mad4), int64 [len // R]: a window's sum, twice its median and four times its MAD, by sorting in int64.
    tests/test_sweep_windows_cpu.py holds it equal to np.median in float64 and, through `scan_table`, to the fixture."""
    x = np.asarray(signal).astype(np.int64)
    R = int(R)
    nw = x.shape[0] // R
    win = x[: nw * R].reshape(nw, R)
    s = np.sort(win, axis=1)
    med2 = s[:, (R - 1) // 2] + s[:, R // 2]
    d = np.sort(np.abs(2 * win - med2[:, None]), axis=1)
    mad4 = d[:, (R - 1) // 2] + d[:, R // 2]
    return win.sum(axis=1), med2, mad4


def scan_table(sums, mad4, R: int, thr: int):
    """-> (start, end) from a table: the rule of `polya_coords` in float64 and in its operation order (mad4 / 4 is exact)"""
    sums = np.asarray(sums, dtype=np.int64)
    if sums.shape[0] == 0:
        return -1, -1
    return _scan(sums, np.asarray(mad4, dtype=np.int64).astype(np.float64) * 0.25, int(R), thr)


# ---- a numpy model of the device's select, written from the header comment of csrc/polya_coords.hip ---------------------------
# Two levels of 256 bins: the histogram of a 16-bit key's high byte finds the bin that holds a rank, the histogram of the low
# byte inside that bin finds the key; the two middle ranks share the second histogram unless they straddle a high-byte bin.
# Keys: x + 32768 for the median, |2 x - med2| >> 1 for the MAD, whose parity is added back.  The model exists so that the
# tests can say which paths a window takes, and so that a defect can be put into it (`mutant`) to see whether the designed
# windows would notice the same defect in the kernel.
MUTANTS = ("upper_at_k0",                # the upper middle taken at rank k0
           "straddle_ignored",           # no third histogram: the second value's low byte is read from hi0's bin
           "parity_dropped",             # 4 MAD = 2 (e0 + e1), without med2's parity
           "bias_dropped",               # keys x & 0xffff: negatives sort above positives
           "med2_halved",                # the deviation taken from med2 // 2
           "rank_not_rebased",           # the low-byte histogram asked for the window's rank, not the rank inside the bin
           "sum_drops_partial_stride")   # the window sum without the last partial stride of 64 samples


def _find(hist, k):
    """rank k -> (bin, rank inside the bin, the bin's count); (-1, -1, 0) when fewer than k + 1 keys are counted"""
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, k, side="right"))
    if b >= len(hist):
        return -1, -1, 0
    return b, int(k - (cum[b] - hist[b])), int(hist[b])


def _select2(keys, k0, k1, mutant):
    """order statistics k0 <= k1 of `keys` -> (v0, v1, path)"""
    hist = np.bincount(keys >> 8, minlength=256)
    hi0, r0, n0 = _find(hist, k0)
    hi1, r1, n1 = _find(hist, k1)

    def low(hi, rank, k):
        h = np.bincount(keys[(keys >> 8) == hi] & 255, minlength=256)
        b = _find(h, k if mutant == "rank_not_rebased" else rank)[0]
        return -1 if b < 0 else (hi << 8) | b                          # no lane holds the rank: -1 comes out of the wave maximum

    v0 = low(hi0, r0, k0)
    if hi1 != hi0 and mutant == "straddle_ignored":
        v1 = (hi1 << 8) | (v0 & 255)
    else:
        v1 = low(hi1, r1, k1)
    return v0, v1, dict(straddle=hi1 != hi0, hi0=hi0, hi1=hi1, r0=r0, r1=r1, n0=n0, n1=n1)


def select_model(window, mutant=None):
    """one window -> (sum, med2, mad4, {"med": path, "mad": path}); path: straddle, the high bins hi0 / hi1 of the two middles,
    their ranks r0 / r1 inside those bins and the bins' counts n0 / n1"""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(window).astype(np.int64)
    R = x.shape[0]
    k0, k1 = (R - 1) // 2, R // 2
    if mutant == "upper_at_k0":
        k1 = k0
    total = int(x[: R // 64 * 64].sum() if mutant == "sum_drops_partial_stride" else x.sum())
    if mutant == "bias_dropped":
        u0, u1, med = _select2(x & 0xFFFF, k0, k1, mutant)
        med2 = sum(u - 65536 if u >= 32768 else u for u in (u0, u1))
    else:
        u0, u1, med = _select2(x + 32768, k0, k1, mutant)
        med2 = u0 + u1 - 65536
    centre = 2 * (med2 // 2) if mutant == "med2_halved" else med2
    e0, e1, mad = _select2(np.abs(2 * x - centre) >> 1, k0, k1, mutant)
    par = 0 if mutant == "parity_dropped" else centre & 1
    return total, int(med2), int(2 * (e0 + e1) + 2 * par), {"med": med, "mad": mad}


# ---- designed inputs, shared by tests/test_sweep_windows_cpu.py and tests/test_sweep_windows.py ----------------------------
RESOLUTIONS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 500, 3584, 3585, 16383, 16384)
ALPHABET = (-32768, -1, 0, 1, 32767)
DESIGN_SEED = 20261019


def _spread(rng, R, c_lo, c_hi, ts):
    """a window, as u = x + 32768, whose two middles are c_lo <= c_hi (one middle c_lo == c_hi for an odd R) and whose other
    samples lie at the distances `ts` beyond the nearer middle, half of them below and half above, shuffled.  With g = c_hi -
    c_lo the MAD key of a sample at distance t is t + (g >> 1), and the middles' own is g >> 1."""
    n_mid = 2 - R % 2
    half = (R - n_mid) // 2
    ts = np.asarray(ts, dtype=np.int64)
    assert ts.shape[0] == 2 * half and (n_mid == 2 or c_lo == c_hi) and 0 <= c_lo <= c_hi <= 65535
    up_only, down_only = ts > c_lo, ts > 65535 - c_hi
    assert not (up_only & down_only).any()
    free = np.flatnonzero(~up_only & ~down_only)
    rng.shuffle(free)
    n_down = half - int(down_only.sum())
    assert 0 <= n_down <= free.shape[0], (R, c_lo, c_hi)
    down = np.concatenate([np.flatnonzero(down_only), free[:n_down]])
    up = np.concatenate([np.flatnonzero(up_only), free[n_down:]])
    u = np.concatenate([c_lo - ts[down], np.array([c_lo, c_hi][:n_mid], dtype=np.int64), c_hi + ts[up]])
    assert u.shape[0] == R and u.min() >= 0 and u.max() <= 65535
    rng.shuffle(u)
    return (u - 32768).astype(np.int16)


def _ts(rng, R, T0, T1, top, tmin=0):
    """distances for `_spread` whose middle order statistics are T0 at rank k0 and T1 at rank k1 once the middles' own
    distance 0 is counted in (an odd R: the one middle rank holds T0; R = 4: rank k0 is a middle itself, rank k1 holds T1)"""
    assert tmin <= T0 <= T1 <= top
    if R % 2:
        m = (R - 1) // 2
        return np.concatenate([rng.integers(tmin, T0 + 1, m - 1), [T0], rng.integers(T0, top + 1, m)])
    m = R // 2
    low = np.concatenate([rng.integers(tmin, T0 + 1, m - 3), [T0]]) if m >= 3 else np.zeros(0, dtype=np.int64)
    return np.concatenate([low, [T1], rng.integers(T1, top + 1, 2 * m - 3 - low.shape[0])])


def _middles(R, boundary, i):
    """the two middles on either side of u = `boundary` (an odd R: the one middle below or at it, by turns)"""
    if R % 2:
        c = boundary - 1 + (i + (boundary > 32768)) % 2                # bins 0 and 255 in a family's first turn
        return c, c
    return boundary - 1, boundary


def _noise(i, n, level):
    x = synth.make_signals(DESIGN_SEED ^ 0x5A5A, 1, max(n, 1), first_read=i, spikes=False)[0, :n].astype(np.int64) - 500 + level
    return np.clip(x, -32768, 32767).astype(np.int16)


def _f_med_straddle(b):
    def f(rng, R, i):                                                  # the MAD's middles share bin 0
        T = int(rng.integers(5, 100))
        return _spread(rng, R, *_middles(R, 256 * b, i), _ts(rng, R, T, T, T + 100))
    return f


def _f_mad_straddle(c, j):
    def f(rng, R, i):                                                  # both middles at c: the median's share a bin
        T0, T1 = (256 * j - 1, 256 * j) if R % 2 == 0 else (256 * j - 1 + i % 2,) * 2
        return _spread(rng, R, c, c, _ts(rng, R, T0, T1, T1 + 500))
    return f


def _f_both(b, j):
    def f(rng, R, i):
        T0, T1 = (256 * j - 1, 256 * j) if R % 2 == 0 else (256 * j - 1 + i // 2 % 2,) * 2
        return _spread(rng, R, *_middles(R, 256 * b, i), _ts(rng, R, T0, T1, T1 + 500))
    return f


def _f_one_bin(c_lo, c_hi, last=False):
    def f(rng, R, i):                                                  # every other sample differs from the middles (tmin 1)
        T = int(rng.integers(5, 100))
        lo, hi = (c_lo, c_hi) if R % 2 == 0 else (c_hi, c_hi) if last else (c_lo, c_lo)
        return _spread(rng, R, lo, hi, _ts(rng, R, T, T, T + 100, tmin=1))
    return f


def _f_extremes(delta):
    def f(rng, R, i):                                                  # -32768 | 32767; an odd R: one sample in between
        n_lo = R // 2 + (delta if R % 2 == 0 else 0)
        x = np.concatenate([np.full(n_lo, -32768), np.full(R % 2, (0, -1)[i % 2]), np.full(R - n_lo - R % 2, 32767)])
        rng.shuffle(x)
        return x.astype(np.int16)
    return f


def _f_two_valued(delta):
    def f(rng, R, i):
        v = (-1, 255 - 32768, 500, -32768, 32766)[i % 5]               # the sign crossing, bins 0 | 1, one bin, both ends
        x = np.concatenate([np.full(R // 2 + delta, v), np.full(R - R // 2 - delta, v + 1)])
        rng.shuffle(x)
        return x.astype(np.int16)
    return f


def _f_sorted(step, descending):
    def f(rng, R, i):
        s = max(min(step, 65535 // R), 1)
        x = (-1, -32768, 100)[i % 3] + s * np.arange(R, dtype=np.int64)
        x = np.clip(x - (x.max() - 32767 if x.max() > 32767 else 0), -32768, 32767)
        return (x[::-1] if descending else x).astype(np.int16)
    return f


def _f_constant(rng, R, i):
    return np.full(R, (-32768, -1, 0, 777, 32767)[i % 5], dtype=np.int16)


def _f_ties(rng, R, i):
    level = (470, -20, 20000)[i % 3]
    return np.clip(np.round(rng.normal(level, 30, R) / 8) * 8, -32768, 32767).astype(np.int16)


def _f_uniform(rng, R, i):
    return rng.integers(-32768, 32768, R).astype(np.int16)


# by turns; the first eight are all that a resolution from 3584 on has room for (two reads of four windows)
FAMILIES = (
    ("median straddle 0|1", _f_med_straddle(1)), ("median straddle 254|255", _f_med_straddle(255)),
    ("MAD straddle 0|1", _f_mad_straddle(40000, 1)), ("both straddle, sign crossing", _f_both(128, 3)),
    ("one bin, first rank", _f_one_bin(256 * 77, 256 * 77 + 1)), ("one bin, last rank", _f_one_bin(256 * 200 + 254, 256 * 200 + 255, last=True)),
    ("extremes, even split", _f_extremes(0)), ("noise", lambda rng, R, i: _noise(i, R, (-3, 470, -300, 4000)[i % 4])),
    ("median straddle 127|128", _f_med_straddle(128)), ("MAD straddle 99|100", _f_mad_straddle(32768 + 3000, 100)),
    ("MAD straddle 2|3", _f_mad_straddle(20000, 3)), ("both straddle 49|50", _f_both(50, 1)), ("both straddle 199|200", _f_both(200, 40)),
    ("bin 255, first rank", _f_one_bin(65280, 65280)), ("bin 0, last rank", _f_one_bin(255, 255)),
    ("sign bin, first rank", _f_one_bin(32768, 32768)), ("constant", _f_constant),
    ("extremes, one fewer low", _f_extremes(-1)), ("extremes, one more low", _f_extremes(1)),
    ("two values, even split", _f_two_valued(0)), ("two values, one fewer low", _f_two_valued(-1)),
    ("two values, one more low", _f_two_valued(1)), ("ascending by 1", _f_sorted(1, False)), ("descending by 1", _f_sorted(1, True)),
    ("ascending by 3", _f_sorted(3, False)), ("descending, full range", _f_sorted(65535, True)),
    ("ascending, full range", _f_sorted(65535, False)), ("ties of 8 counts", _f_ties), ("uniform int16", _f_uniform),
)


def designed_windows(R: int, count: int):
    """-> [(family, int16 [R])], `count` of them: for R <= 3 every window over ALPHABET, by turns; else the families by turns,
    each turn with new draws and the next of a family's levels"""
    if R <= 3:
        grid = np.array(np.meshgrid(*[ALPHABET] * R, indexing="ij")).reshape(R, -1).T.astype(np.int16)
        return [("alphabet", grid[n % grid.shape[0]].copy()) for n in range(count)]
    rng = np.random.default_rng([DESIGN_SEED, R])
    out = []
    for n in range(count):
        name, f = FAMILIES[n % len(FAMILIES)]
        w = f(rng, R, n // len(FAMILIES))
        assert w.dtype == np.int16 and w.shape == (R,), name
        out.append((name, w))
    return out


def designed_window_counts(R: int):
    """windows per read: waves that leave a workgroup early (1, 3, 5), two and three trips of the scan loop (65, 130); from
    R = 3584 on two reads of four windows, 65 536 samples at most"""
    return (1, 3, 4, 5, 65, 130) if R <= 500 else (4, 4)


def designed_reads(R: int):
    """-> (reads, names): the designed windows concatenated into reads, each with a ragged tail shorter than R; names[b][w] is
    the family of read b's window w.  No read is longer than 65 536 samples: at R = 16384 there is no room for a tail."""
    counts = designed_window_counts(R)
    wins = designed_windows(R, sum(counts))
    assert R > 3 or sum(counts) >= len(ALPHABET) ** R
    rng = np.random.default_rng([DESIGN_SEED, R, 1])
    reads, names, at = [], [], 0
    for b, n in enumerate(counts):
        tail = rng.integers(-32768, 32768, min(1 + (7 * b + R // 2) % (R - 1) if R > 1 else 0, 65536 - n * R)).astype(np.int16)
        reads.append(np.concatenate([w for _, w in wins[at:at + n]] + [tail]))
        names.append([name for name, _ in wins[at:at + n]])
        at += n
    return reads, names


# ---- reads whose windows ride the rule's thresholds ---------------------------------------------------------------------------
RIDING = {(64, 12): 20261019, (255, 20): 20261020, (256, 40): 20261021, (500, 20): 20261022, (3585, 25): 20261023}


def _riding_window(rng, R, level, mad):
    """a window around `level` whose MAD is `mad` exactly (half steps for an even R, whole ones for an odd R); one even-R
    window in three has adjacent middles, so that med2 is odd and 4 MAD = 2 (T0 + T1) + 2 owes 2 to the parity term"""
    c = int(round(level)) + 32768
    if R % 2:
        return _spread(rng, R, c, c, _ts(rng, R, int(mad), int(mad), int(mad) + 60))
    g = int(rng.integers(0, 3) == 0)
    T0 = (int(2 * mad) - g) // 2
    T1 = int(2 * mad) - g - T0
    return _spread(rng, R, c, c + g, _ts(rng, R, T0, T1, T1 + 60))


def riding_reads(R: int, thr: int):
    """Reads whose every window has a MAD of thr - h, thr, thr + h, 20 or 20 + h (h = 0.5, or 1 for an odd R) and whose window
    levels step by factors around 1.20 against the 2 R before them, after a flat stretch of any length.  Three kinds: reads
    that cannot start (a rise always comes with a MAD above the threshold), reads that cannot end (no MAD above 20) and free
    ones.  For R <= 256, 70 ... 150 windows per read, and two reads with a start in window 63 / 127 that ends in the next one;
    where thr > 20 a read whose start ends in its own window.  -> (reads, expected): expected[b] is (start, end) or None."""
    rng = np.random.default_rng([RIDING[(R, thr)], R, thr])
    h = 0.5 if R % 2 == 0 else 1.0
    mads = (thr - h, thr, thr + h, 20.0, 20.0 + h)
    ups, others = (1.19, 1.21, 1.25), (1.0, 1.0, 0.9, 0.8)
    n_reads, nws = (48, (70, 100, 135, 150)) if R <= 256 else (96, tuple(range(4, 61))) if R == 500 else (48, tuple(range(4, 18)))
    reads, expected = [], []
    for b in range(n_reads):
        kind = ("none", "free", "no end", "free", "free")[b % 5]
        nw = int(rng.choice(nws))
        flat = int(rng.integers(0, nw - 3))
        level = float(rng.integers(300, 700))
        parts = []
        for w in range(nw):
            f = 1.0 if w < flat else float(rng.choice(ups + others))
            level = min(max(level * f, 150.0), 6000.0)
            pool = [m for m in mads if (kind != "none" or f <= 1.0 or m > thr) and (kind != "no end" or m <= 20.0)]
            parts.append(_riding_window(rng, R, level, float(rng.choice(pool))))
        parts.append(_riding_window(rng, R, level, 20.0)[: int(rng.integers(0, R))])      # a last partial window
        reads.append(np.concatenate(parts))
        expected.append(None)
    calm = min(thr, 20) - h
    if R <= 256:
        for at in (63, 127):
            parts = [_riding_window(rng, R, 400, 20.0 + h) for _ in range(at)]
            parts += [_riding_window(rng, R, 520, calm), _riding_window(rng, R, 520, 20.0 + h), _riding_window(rng, R, 520, calm)]
            reads.append(np.concatenate(parts))
            expected.append((at * R, (at + 1) * R))
    if thr > 20:
        at = 70 if R <= 256 else 5
        parts = [_riding_window(rng, R, 400, calm) for _ in range(at)] + [_riding_window(rng, R, 520, float(thr)) for _ in range(2)]
        reads.append(np.concatenate(parts))
        expected.append((at * R, at * R))
    return reads, expected
