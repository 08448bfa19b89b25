"""The float signal kernels at IEEE VALUE edges: rs_normalise_float (float16 / float32 / float64) and rs_retrain_prepare (float32
pA, and int16 under degenerate calibrations) on reads that carry NaNs, infinities, zeros of both signs, values next to overflow
and underflow, subnormals and exact ties at the outlier limit (tests/float_edges_ref.py), against numpy: the two oracles that
tests/test_float_edges_cpu.py pins to the reference's own answers.  Bit for bit, NaN equal to NaN; a case whose median numpy
itself gives either sign of zero (float_edges_ref.zero_sign_free - none with the numpy the fixture was made with) is compared
with the sign of exact zeros masked.  Every test prints one line per failing class before it asserts."""
import numpy as np
import pytest
import torch

from riser_amd import retrain as T
from tests import float_edges_ref as F
from tests import retrain_ref as R
from tests.test_retrain import SENTINEL, device_prepare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def proc(dev):
    from riser_amd.preprocess import Kit, SignalProcessor
    return SignalProcessor(Kit.create_from_version("RNA004"), device=dev)


def agree(x, got_row, got_stats, want_row, want_stats):
    """a device row and its (median, MAD) against the oracle's, the sign of exact zeros masked only where numpy leaves it open"""
    m = F.mask_zero_sign if F.zero_sign_free(x) else (lambda a: a)
    with np.errstate(invalid="ignore"):                                      # widening a signalling NaN
        want_stats = np.array(want_stats, dtype=np.float64)
    return F.same_bits(m(got_row), m(want_row)) and F.same_bits(m(np.asarray(got_stats, dtype=np.float64)), m(want_stats))


def report(what, bad):
    """one line per failing class, then the assertion"""
    by_cls = {}
    for name in bad:
        by_cls.setdefault(name.split(".")[0], []).append(name)
    for cls, names in by_cls.items():
        print(f"{what}: {cls}: {len(names)} failing: {' '.join(names)}")
    assert not bad, (what, sorted(by_cls))


# ---- rs_normalise_float -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.DTYPES)
def test_normalise_float_value_edges(proc, dt):
    cases = F.edge_cases(dt)
    outs, stats = proc.mad_normalise_float_batch([c.x for c in cases], return_stats=True)
    bad = []
    for c, o, st in zip(cases, outs, stats):
        want = F.live_oracle(c.x)
        if want.dtype == np.int64:                                           # a zero MAD: the batch surface keeps the dtype
            want = np.zeros(len(c.x), dtype=c.x.dtype)
        if not agree(c.x, o, st, want, F.stats(c.x)[:2]):
            bad.append(c.name)
    # bystanders: the finite reads get the rows they get in a batch of their own
    control = [i for i, c in enumerate(cases) if c.cls == "control"]
    alone, alone_stats = proc.mad_normalise_float_batch([cases[i].x for i in control], return_stats=True)
    for i, o, st in zip(control, alone, alone_stats):
        if not (F.same_bits(o, outs[i]) and F.same_bits(st, stats[i])):
            bad.append(cases[i].name + "(bystander)")
    report(f"rs_normalise_float {dt}", bad)


@pytest.mark.parametrize("dt", F.DTYPES)
def test_normalise_single_read_surface(proc, dt):
    """proc.mad_normalise on one case per class, a zero MAD and a NaN MAD: the reference's dtype rule - int64 zeros for MAD 0
    and NOT for MAD NaN"""
    cases = F.edge_cases(dt)
    pick = {c.cls: c for c in reversed(cases)}                               # the first of every class
    pick["mad 0"] = next(c for c in cases if c.prop == "median_zero_mad_zero")
    pick["mad nan"] = next(c for c in cases if c.prop == "median_inf")
    bad = []
    for what, c in pick.items():
        want = F.live_oracle(c.x)
        got = proc.mad_normalise(c.x.copy())
        m = F.mask_zero_sign if F.zero_sign_free(c.x) else (lambda a: a)
        assert want.dtype == (np.int64 if what == "mad 0" else c.x.dtype), what
        if got.dtype != want.dtype or not F.same_bits(m(got), m(want)):
            bad.append(c.name)
    report(f"mad_normalise {dt}", bad)


# ---- rs_retrain_prepare ---------------------------------------------------------------------------------------------------------------
def run_at_own_length(dev, reads, lim):
    """every float32 read at exactly its own length: T.MAX_CUTOFFS lengths per launch, all reads in every launch, a read mapped
    to a row only at the cutoff that is its length.  -> ([row], [(median, MAD)]) per read; the rows no read maps to, the row
    behind each output and the stats of unmapped reads must keep their sentinel."""
    lens = np.array([len(r) for r in reads])
    rows_out, stats_out = [None] * len(reads), [None] * len(reads)
    cuts_all = sorted(set(lens.tolist()))
    for k in range(0, len(cuts_all), T.MAX_CUTOFFS):
        cuts = cuts_all[k: k + T.MAX_CUTOFFS]
        rows = np.full((len(cuts), len(reads)), -1, dtype=np.int64)
        for c, n in enumerate(cuts):
            at = np.flatnonzero(lens == n)
            rows[c, at] = np.arange(len(at))
        outs, stats, _ = device_prepare(dev, reads, None, cuts, lim, rows=rows)
        for c, n in enumerate(cuts):
            assert (outs[c][-1] == np.float32(SENTINEL)).all(), (n, "the row behind the output was written")
            assert (stats[c][rows[c] < 0] == SENTINEL).all(), n
            for b in np.flatnonzero(rows[c] >= 0):
                rows_out[b], stats_out[b] = outs[c][rows[c, b]], stats[c, b]
    return rows_out, stats_out


@pytest.mark.parametrize("lim", F.LIMITS)
def test_retrain_prepare_value_edges_pa(dev, lim):
    cases = [c for c in F.edge_cases("float32") if len(c.x) >= 2]                # a cutoff is two samples at least
    got_rows, got_stats = run_at_own_length(dev, [c.x for c in cases], lim)
    bad = []
    for c, o, st in zip(cases, got_rows, got_stats):
        y, med, mad = F.retrain_oracle(c.x, lim)
        if not agree(c.x, o, st, y, (med, mad)):
            bad.append(c.name)
    control = [i for i, c in enumerate(cases) if c.cls == "control"]
    alone, alone_stats = run_at_own_length(dev, [cases[i].x for i in control], lim)
    for i, o, st in zip(control, alone, alone_stats):
        if not (F.same_bits(o, got_rows[i]) and F.same_bits(st, got_stats[i])):
            bad.append(cases[i].name + "(bystander)")
    report(f"rs_retrain_prepare pA, limit {lim}", bad)


@pytest.mark.parametrize("lim", F.LIMITS)
def test_retrain_prepare_degenerate_calibrations(dev, lim):
    """the int16 reads under every degenerate calibration, and under an ordinary one as bystanders, at both cutoffs"""
    raw = F.int16_reads()
    cals = list(zip(F.CALIBRATION_NAMES, F.degenerate_calibrations())) + [("control", (3.0, 1437.3, 8192.0))]
    names, reads, offset, rng, dig = [], [], [], [], []
    for cname, (o, r, d) in cals:
        for i, x in enumerate(raw):
            names.append(f"{cname}.{i}")
            reads.append(x)
            offset.append(o), rng.append(r), dig.append(d)
    with np.errstate(all="ignore"):
        cal = T.as_calibration((np.array(offset), np.array(rng), np.array(dig)), len(reads))
        pa = [R.pa(*t) for t in zip(reads, offset, rng, dig)]
        want = R.prepare(pa, F.CUTOFFS, lim)
    outs, stats, _ = device_prepare(dev, reads, cal, F.CUTOFFS, lim)
    bad = []
    for c, n in enumerate(F.CUTOFFS):
        w_rows, kept, w_stats = want[c]
        assert len(kept) == len(reads) and outs[c].shape[0] == len(reads) + 1 and (outs[c][-1] == np.float32(SENTINEL)).all()
        for b, name in enumerate(names):
            if not agree(pa[b][:n], outs[c][b], stats[c, b], w_rows[b], w_stats[b]):
                bad.append(f"{name}.{n}")
    k = len(raw)
    alone, alone_stats, _ = device_prepare(dev, reads[-k:], cal[-k:], F.CUTOFFS, lim)
    for c, n in enumerate(F.CUTOFFS):
        assert np.isfinite(alone[c][:-1]).all()
        if not (F.same_bits(alone[c][:-1], outs[c][-k - 1:-1]) and F.same_bits(alone_stats[c], stats[c, -k:])):
            bad.append(f"control.{n}(bystander)")
    report(f"rs_retrain_prepare int16, limit {lim}", bad)
