"""The offline evaluation sweep on the device: rs_polya_coords (csrc/polya_coords.hip) against the reference script's own answers
(tests/golden/polya_coords.npz), the live detector and the numpy mirror of tests/sweep_ref.py - exactly, no tolerance - and
riser_amd.evaluate.sweep against the script's pipeline (tests/golden/sweep.npz) and against solo calls, bit for bit."""
import os
import types

import numpy as np
import pytest
import torch

from riser_amd import _native as nv
from riser_amd import evaluate as E
from riser_amd import synth
from tests import sweep_ref as R
from tests.sweep_dev import assert_mirror, device_scan

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-3          # the project's bar for classify_raw against the reference (north_star, tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def proc(dev):
    from riser_amd.preprocess import Kit, SignalProcessor
    return SignalProcessor(Kit.create_from_version("RNA004"), device=dev)


@pytest.fixture(scope="module")
def coords(golden_dir):
    g = np.load(os.path.join(golden_dir, "polya_coords.npz"))
    reads, neg = R.coords_reads(g)
    return g, reads, neg


def _noisy(stream, n, level=470):
    return synth.make_signals(77 ^ 0x5A5A, 1, max(n, 1), first_read=stream, spikes=False)[0, :n].astype(np.int64) - 500 + level


def _i16(parts):
    return np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)


# ---- detector --------------------------------------------------------------------------------------------------------
def test_coords_equal_the_reference_on_every_read_and_row(proc, coords):
    g, reads, neg = coords
    for k, (res, thr) in enumerate(g["rows"]):
        st, en = proc.get_polyA_coords_batch(reads, int(res), int(thr))
        assert st.dtype == np.int32 and en.dtype == np.int32
        assert np.array_equal(st, g["starts"][k]) and np.array_equal(en, g["ends"][k]), (res, thr)
    for k, (res, thr) in enumerate(g["neg_rows"]):
        st, en = proc.get_polyA_coords_batch(neg, int(res), int(thr))
        assert np.array_equal(st, g["neg_starts"][k]) and np.array_equal(en, g["neg_ends"][k]), (res, thr)
    want = (int(g["starts"][0][0]), int(g["ends"][0][0]))
    assert proc.get_polyA_coords(reads[0], 500, 20) == tuple(None if v < 0 else v for v in want)
    assert proc.get_polyA_coords(reads[3], 500, 20) == (None, None)


def test_end_at_500_20_is_the_live_detector(proc, coords, golden_dir):
    g, reads, _ = coords
    _, en = proc.get_polyA_coords_batch(reads, 500, 20)
    assert np.array_equal(en, proc.get_polyA_end_batch(reads))
    live = np.load(os.path.join(golden_dir, "polya.npz"))
    cases = live["cases"]
    sigs = [synth.make_raw_read(int(s), int(rid), int(n), bool(p)) for s, rid, n, p, _ in cases]
    _, en = proc.get_polyA_coords_batch(sigs, 500, 20)
    assert np.array_equal(en, cases[:, 4].astype(np.int32))
    edge = [s for _, s in synth.polya_edge_cases()]
    _, en = proc.get_polyA_coords_batch(edge, 500, 20)
    assert np.array_equal(en, live["edge_ends"].astype(np.int32))


def test_small_and_largest_resolution(dev, coords):
    _, reads, _ = coords
    some = [reads[0], reads[3], reads[5], reads[24], reads[30]]
    for res, thr in ((2, 20), (3, 20), (2, 0), (3, 1)):
        assert_mirror(dev, some, res, thr)
    # 16384: a lone wave per workgroup, four windows in 70 000 samples, the rise in the only window that has a rolling mean
    long = _i16([_noisy(1, 49152), synth._quiet(77, 1, 70000 - 49152, 760)])
    st, en = assert_mirror(dev, [long, reads[2]], 16384, 20)
    assert st[0] == 49152 and en[0] == -1
    st, en = assert_mirror(dev, [long], 16384, 3)                      # the plateau's MAD is above 3: no start
    assert st[0] == -1


def test_extreme_samples(dev):
    rng = np.random.default_rng(5)
    read = _i16([20000 + rng.integers(-5, 6, 1700), np.full(1500, 32767), rng.integers(-32768, 32768, 1800),
                 np.full(1300, -32768), -32768 + rng.integers(0, 3, 900), rng.integers(-32768, 32768, 700)])
    full = rng.integers(-32768, 32768, 9000).astype(np.int16)
    two = np.where(rng.integers(0, 2, 7000) == 1, 32767, -32768).astype(np.int16)
    for res, thr in ((500, 20), (250, 20), (64, 40), (3, 20), (1000, 30), (4096, 20)):
        st, _ = assert_mirror(dev, [read, full, two, read[::-1].copy()], res, thr)
        if res == 500:
            assert st[0] == 1500                                       # 20000 -> 32767 is a 64 % rise on a flat window


def test_lengths_inside_a_batch(dev, coords):
    _, reads, _ = coords
    batch = [reads[0], reads[1][:499], reads[2], reads[4], reads[5], reads[6][:500]]
    lens = [len(batch[0]), 499, 0, -3, len(batch[4]), 500]
    st, en = assert_mirror(dev, batch, 500, 20, lens=lens)
    assert (st[1], en[1]) == (-1, -1) and (st[2], en[2]) == (-1, -1) and (st[3], en[3]) == (-1, -1) and st[0] > 0 and st[4] > 0
    # B = 1, every length all zero or negative, and a batch of windows shorter than every read
    assert_mirror(dev, [reads[0]], 500, 20)
    st, en = device_scan(dev, batch, 500, 20, lens=[0, -1, 0, -5, 0, 0])
    assert (st == -1).all() and (en == -1).all()
    # a d_len beyond max_len is scanned as max_len
    claimed = [len(r) for r in batch[:1]] + [499, 0, -3, len(batch[4]) * 10, 500]
    for cut in (3000, 3499, 1, 0):
        device_cut = assert_mirror(dev, batch, 500, 20, lens=[min(c, 2 ** 31 - 1) for c in claimed], max_len=cut)
        assert cut >= 3000 or (device_cut[0] == -1).all()


def test_a_long_read_among_short_ones_and_the_batch_reversed(dev, coords):
    _, reads, _ = coords
    long = _i16([_noisy(2, 150000), synth._quiet(77, 2, 3000, 760), _noisy(3, 47000, 520)])
    assert len(long) == 200000
    batch = [reads[0], reads[35], long, reads[1][:700], reads[7], reads[26]]
    for res, thr in ((500, 20), (333, 12)):
        st, en = assert_mirror(dev, batch, res, thr)
        assert st[2] >= 150000 - res and en[2] > st[2]
        rst, ren = device_scan(dev, batch[::-1], res, thr)
        assert np.array_equal(rst[::-1], st) and np.array_equal(ren[::-1], en)


def test_workspace_is_never_assumed_clean(dev, coords):
    g, reads, _ = coords
    small = [reads[0], reads[1], reads[9]]
    big_need = int(nv.lib().rs_polya_coords_workspace_bytes(len(reads), max(len(r) for r in reads), 250))
    ws = torch.full((big_need,), 0xFF, dtype=torch.uint8, device=dev)
    first = assert_mirror(dev, small, 500, 20, ws=ws)
    st, en = device_scan(dev, reads, 250, 20, ws=ws)                   # a larger call leaves its own table behind
    assert np.array_equal(st, g["starts"][1]) and np.array_equal(en, g["ends"][1])
    again = assert_mirror(dev, small, 500, 20, ws=ws)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    ws.fill_(0xFF)
    st, en = device_scan(dev, reads, 1000, 30, ws=ws)
    assert np.array_equal(st, g["starts"][4]) and np.array_equal(en, g["ends"][4])


# ---- sweep -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_g(golden_dir):
    g = np.load(os.path.join(golden_dir, "sweep.npz"))
    return g, R.sweep_reads(g)


@pytest.fixture(scope="module")
def shipped(dev, sweep_g):
    from riser_amd.model import Model
    m = Model(synth.make_state_dict(int(sweep_g[0]["weights_seed"])), synth.Config(), None, "mRNA", device=dev)
    yield m
    m.close()


@pytest.fixture(scope="module")
def tcn(dev):
    from riser_amd.model import Model
    cfg = dict(in_channels=1, n_filters=16, kernel=3, dilation=2, n_layers=6, dropout=0.0, n_classes=2)
    m = Model(synth.make_tcn_state_dict(11, cfg), types.SimpleNamespace(model="tcn", tcn=types.SimpleNamespace(**cfg)), None,
              "mRNA", device=dev)
    assert m.min_length <= 4096
    yield m
    m.close()


_results = {}


def run_sweep(model, reads, kit, tag):
    if (tag, kit) not in _results:
        _results[(tag, kit)] = E.sweep(model, reads, kit)
    return _results[(tag, kit)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_pairs_are_solo_calls(model, reads, res, kit):
    from riser_amd.preprocess import pack_reads
    plan = E.sweep_plan(kit)
    want = R.pairs([len(r) for r in reads], res.ends, plan["lengths"], plan["fixed_trim"], res.already_trimmed)
    assert [(n, k) for n, k, _, _ in want] == [(int(n), int(k)) for n, k in zip(*np.nonzero(res.valid))]
    assert np.array_equal(np.isnan(res.probs[:, :, 0]), ~res.valid) and np.array_equal(np.isnan(res.probs[:, :, 1]), ~res.valid)
    for n, k, first, L in want:
        sig, off, ln, lens = pack_reads([reads[n][first:first + L]], model.device)
        solo = model.classify_raw(sig, off, ln, lens).cpu().numpy()[0]
        assert np.array_equal(bits(solo), bits(res.probs[n, k])), (n, k)
    return len(want)


@pytest.mark.parametrize("kit", ["RNA002", "RNA004"])
def test_sweep_equals_the_reference_script(shipped, sweep_g, kit):
    g, reads = sweep_g
    res = run_sweep(shipped, reads, kit, "shipped")
    assert res.lengths == g[f"{kit}_lengths"].tolist() and res.probs.shape == (16, len(res.lengths), 2)
    assert res.starts.dtype == np.int32 and np.array_equal(res.starts, g[f"{kit}_starts"])
    assert np.array_equal(res.ends, g[f"{kit}_ends"])
    want = g[f"{kit}_probs"]
    assert np.array_equal(res.valid, ~np.isnan(want[:, :, 0]))
    gap = float(np.abs(res.probs[res.valid] - want[res.valid]).max())
    print(f"SWEEP_GAP {kit} {gap:.3e} over {int(res.valid.sum())} prefixes")
    assert gap < PROB_TOL


@pytest.mark.parametrize("kit", ["RNA002", "RNA004"])
def test_sweep_pairs_are_solo_calls_and_chunking_keeps_the_bits(shipped, sweep_g, kit):
    _, reads = sweep_g
    res = run_sweep(shipped, reads, kit, "shipped")
    assert assert_pairs_are_solo_calls(shipped, reads, res, kit) == {"RNA002": 28, "RNA004": 23}[kit]
    small = E.sweep(shipped, reads, kit, pairs_per_call=5)
    assert np.array_equal(bits(small.probs), bits(res.probs)) and np.array_equal(small.valid, res.valid)
    assert np.array_equal(small.ends, res.ends) and np.array_equal(small.starts, res.starts)


def test_sweep_with_a_generic_family_model(tcn, sweep_g):
    _, reads = sweep_g
    res = run_sweep(tcn, reads, "RNA002", "tcn")
    assert assert_pairs_are_solo_calls(tcn, reads, res, "RNA002") == 28
    small = E.sweep(tcn, reads, "RNA002", pairs_per_call=5)
    assert np.array_equal(bits(small.probs), bits(res.probs))


def test_already_trimmed_skips_the_scan_and_the_trim(shipped, sweep_g, monkeypatch):
    from riser_amd.preprocess import SignalProcessor
    _, reads = sweep_g

    def no_scan(*a, **k):
        raise AssertionError("reads trimmed beforehand are not scanned")
    monkeypatch.setattr(SignalProcessor, "polyA_coords_device", no_scan)
    res = E.sweep(shipped, reads, "RNA004", already_trimmed=True)
    assert (res.starts == -1).all() and (res.ends == -1).all() and res.already_trimmed
    assert np.array_equal(res.valid, np.array([[len(r) >= L for L in res.lengths] for r in reads]))
    assert assert_pairs_are_solo_calls(shipped, reads, res, "RNA004") == int(res.valid.sum()) and res.valid[0, 0]
    assert res.lines("m", "d", "f", ["r"] * 16)[0].split("\t")[4:6] == ["boostnano", "boostnano"]


def test_a_plan_length_below_the_minimum_is_refused_before_any_gpu_call():
    class Untouchable:
        min_length = 4097

        def __getattr__(self, name):
            raise AssertionError(f"the refusal comes before the model's {name} is used")
    with pytest.raises(ValueError, match="4096"):
        E.sweep(Untouchable(), [np.zeros(20000, dtype=np.int16)], "RNA004")


def test_lines_parse_back_to_the_device_probabilities(shipped, sweep_g):
    _, reads = sweep_g
    res = run_sweep(shipped, reads, "RNA002", "shipped")
    ids = [f"read-{i}" for i in range(16)]
    lines = res.lines("net", "set", "batch0.fast5", ids)
    assert len(lines) == 16
    for n, line in enumerate(lines):
        f = line.rstrip("\n").split("\t")
        assert len(f) == 7 and f[:4] == ["net", "set", "batch0.fast5", ids[n]]
        assert f[4] == ("None" if res.starts[n] < 0 else str(res.starts[n])) and f[5] == ("None" if res.ends[n] < 0 else str(res.ends[n]))
        preds = [p for p in f[6].split(";") if p]
        assert [int(p.split(":")[0]) for p in preds] == [L for k, L in enumerate(res.lengths) if res.valid[n, k]]
        for p in preds:
            k = res.lengths.index(int(p.split(":")[0]))
            pn, pp = (np.float32(float(v)) for v in p.split(":")[1].split(","))
            assert np.array_equal(bits([pn, pp]), bits(res.probs[n, k]))


def test_command_line_writes_the_scripts_file(shipped, sweep_g, tmp_path, capsys):
    g, reads = sweep_g
    seed = int(g["weights_seed"])
    (tmp_path / "cfg.yaml").write_text(
        "model: cnn\n\ncnn:\n  n_layers: 12\n  depth: 1\n  channels: [20,30,45,67,100,150,225,337,505,757,1135,1702]\n"
        "  kernels: [3,3,3,3,3,3,3,3,3,3,3,3]\n  n_classes: 2\n  classifier: gap_fc\n")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(seed).items()}, str(tmp_path / "net_v1.pth"))
    ids = [f"id-{i}" for i in range(len(reads))]
    np.savez(tmp_path / "set7.npz", flat=np.concatenate(reads), lengths=np.array([len(r) for r in reads]),
             read_ids=np.array(ids), filename=np.array("batch_0.fast5"))
    out = tmp_path / "out"
    out.mkdir()
    argv = [str(tmp_path / "set7.npz"), str(tmp_path / "net_v1.pth"), str(tmp_path / "cfg.yaml"), "RNA004", str(out), "N", "500", "20"]
    assert E.main(argv) == 0
    path = out / "batch_0.fast5_test_output.tsv"
    assert capsys.readouterr().out.strip() == str(path)
    want = run_sweep(shipped, reads, "RNA004", "shipped").lines("net_v1", "set7", "batch_0.fast5", ids)
    assert path.read_text() == "".join(want)
    with pytest.raises(SystemExit):
        E.main(argv[:6])                                               # N without RESOLUTION MAD_THRESHOLD
    with pytest.raises(ValueError):
        E.main(argv[:3] + ["RNA999"] + argv[4:])
