"""GPU checks of the control loop's host side (round 4): both traffic models a ReadUntil client can present (whole reads
re-sent, disjoint chunks under one id), the verified signal store, the C host loops against the eight-method duck type,
the sharded launcher on one GPU, and the contained length mismatch on every entry."""
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_path
from riser_amd import synth
from riser_amd.fake_client import FakeClient, FakeRead, PlainFakeClient

from test_gpu_more import _oracle_loop

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = logging.getLogger("ctl4")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _run(batches, models, proc, path, client_cls=FakeClient, signal_cache=True, mode="enrich"):
    from riser_amd.control import SequencerControl
    client = client_cls(batches)
    ctl = SequencerControl(client, models, proc, LOG, path, signal_cache=signal_cache)
    ctl.start(); ctl.target(mode, 0.5, 0.9); ctl.finish()
    rows = [ln.split(",", 1)[1] for ln in open(path + ".csv").read().strip().split("\n")[1:]]
    return rows, client.rejected, client.finished, ctl


def test_same_id_disjoint_chunks(dev, tmp_path):
    """a client that pops its cache delivers a read's NEXT chunk under the same id, not the read
    again (riser/client.py:44).  The signal store must not treat it as an extension of what its row holds: same CSV rows
    and client calls with the store on (C host loops and plain duck type), off, and as the oracle's per-read loop writes
    them; the store notices and stops trying."""
    from riser_amd import Kit, Model, SignalProcessor
    from riser_amd.replay import chunked_batches
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    models = [Model(synth.make_state_dict(s), synth.Config(), None, f"t{s}", device=dev) for s in (1, 2)]
    batches = chunked_batches(10, 192)
    # equal-length consecutive chunks are the dangerous case (nothing "new" to upload if the row were trusted): make sure
    # the script holds some
    same_len = sum(1 for b0, b1 in zip(batches, batches[1:]) for (c0, r0) in b0 for (c1, r1) in b1
                   if c0 == c1 and r0.id == r1.id and len(r0.raw_data) == len(r1.raw_data))
    assert same_len > 50
    runs = [_run(batches, models, proc, str(tmp_path / f"c{k}"), cls, cache)
            for k, (cls, cache) in enumerate(((FakeClient, True), (PlainFakeClient, True), (FakeClient, False)))]
    for r in runs[1:]:
        assert r[:3] == runs[0][:3]
    assert len(runs[0][0]) > 40
    store = runs[0][3]._store
    assert store.mismatches > 100 and store.delta_reads == 0 and store.auto_off and not store.resident
    cpu_models = {s: torch_path.TorchCpuModel(synth.make_state_dict(s)) for s in (1, 2)}
    want_rows, want_rej, want_fin = _oracle_loop(batches[:4], "RNA004", (1, 2), "enrich", 0.9, cpu_models)
    got = [r.split(",") for r in runs[0][0][: len(want_rows)]]
    assert len(got) == len(want_rows) > 15
    for g, w in zip(got, want_rows):
        assert (g[0], int(g[1]), int(g[2])) == w[:3]
        assert np.allclose([float(v) for v in g[4].split(";")], w[4], atol=1e-3)
    for m in models:
        m.close()


def test_store_verifies_the_overlap_not_the_id(dev, tmp_path):
    """a read that comes back under its id, LONGER, but with other samples where the row's tail was (a client that
    re-bases its buffer): caught by the overlap comparison and uploaded whole; a read that does extend its prefix takes
    the delta path.  Either way the rows equal the store-less run."""
    from riser_amd import Kit, Model, SignalProcessor
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    m = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", device=dev)
    a = synth.make_raw_read(9, 1, 20000, True)
    b = synth.make_raw_read(9, 2, 20000, True)
    shifted = np.concatenate([a[:9000], b[9000:16000]])            # same id, longer, different samples behind 9000
    shifted2 = np.concatenate([b[:12000], a[12000:17000]])         # differs everywhere the row's tail would be compared
    batches = [[(1, FakeRead("x", a[:12000])), (2, FakeRead("y", a[:12000]))],
               [(1, FakeRead("x", a[:15000])), (2, FakeRead("y", shifted2))],
               [(1, FakeRead("x", shifted)), (2, FakeRead("y", shifted2))]]
    on = _run(batches, [m], proc, str(tmp_path / "on"))
    off = _run(batches, [m], proc, str(tmp_path / "off"), signal_cache=False)
    assert on[:3] == off[:3] and len(on[0]) >= 4
    st = on[3]._store
    assert st.delta_reads == 2 and st.mismatches == 2            # x batch 1, y batch 2 extend; y batch 1, x batch 2 do not
    m.close()


def test_native_host_loops_equal_the_duck_type(dev, tmp_path):
    """whole-read traffic (scripted_batches): the C loops over read.raw_data (a client that declares raw_data_dtype) and
    the eight-method duck type give the same CSV TEXT (batch_start aside), the same client calls, the same PCIe bytes"""
    from riser_amd import Kit, Model, SignalProcessor
    from riser_amd.replay import scripted_batches
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    models = [Model(synth.make_state_dict(s), synth.Config(), None, t, device=dev) for s, t in ((1, "mRNA"), (3, "globin"))]
    batches = scripted_batches(6, 80)
    nat = _run(batches, models, proc, str(tmp_path / "n"))
    py = _run(batches, models, proc, str(tmp_path / "p"), PlainFakeClient)
    assert nat[:3] == py[:3] and len(nat[0]) > 150
    assert nat[3]._store.samples_uploaded == py[3]._store.samples_uploaded < 0.5 * nat[3]._store.samples_presented
    assert nat[3]._store.mismatches == 0 and nat[3]._store.delta_reads > 200
    # every phase of every assessed batch was timed, and the decision latency excludes the CSV rows
    ph = np.asarray(nat[3].batch_phases)
    assert ph.shape == (len(nat[3].batch_loop_times), 7) and (ph >= 0).all()
    assert all(a <= b for a, b in zip(nat[3].batch_latencies, nat[3].batch_loop_times))
    for m in models:
        m.close()


def test_polya_kernel_is_prefix_stable(dev):
    """the GPU detector (rs_polya_end) on prefixes of a read: an end found on a prefix is the end of the whole read
    (what makes the per-id cache's lifetime irrelevant to the CSV, riser/control.py:96-97)"""
    from riser_amd import Kit, SignalProcessor
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    reads, owner = [], []
    for rid in range(24):
        sig = synth.make_raw_read(31, rid, 26000, polya=(rid % 4 != 0))
        for n in (3000, 5200, 7777, 9000, 12500, 18001, 24000, 26000):
            reads.append(sig[:n])
            owner.append(rid)
    ends = proc.get_polyA_end_batch(reads)
    full = {rid: int(e) for rid, e, r in zip(owner, ends, reads) if len(r) == 26000}
    found = 0
    for rid, e, r in zip(owner, ends, reads):
        if e > 0:
            assert int(e) == full[rid], (rid, len(r))
            found += 1
    assert found > 60


def _launch(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, "-m", "riser_amd.launch", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("run_index", [5, 11])
def test_sharded_launch_two_ranks_one_gpu(tmp_path, golden_dir, run_index):
    """python -m riser_amd.launch --gpus 2 --share-gpus: two processes, each with its own client on its own channel range
    and its own models on the (shared) GPU.  The union of the ranks' CSV rows and reject / finish lists equals the
    single-rank run of the golden script - and the reference's own rows for that run (tests/golden/control.json)."""
    with open(os.path.join(golden_dir, "control.json")) as f:
        g = json.load(f)
    run = g["runs"][run_index]
    common = ["--channels", "22", "--replay-script", os.path.join(golden_dir, "control.json"), "--kit", g["kit"],
              "--mode", run["mode"], "--threshold", str(run["threshold"]), "--seeds", ",".join(map(str, run["seeds"])),
              "--duration-h", "1.0", "--share-gpus"]
    _launch(["--gpus", "1", "--out", str(tmp_path / "one"), *common])
    two = _launch(["--gpus", "2", "--out", str(tmp_path / "two"), *common])
    assert two["ranks"] == 2 and two["channel_ranges"] == [[1, 11], [12, 22]]

    def rows(path):
        return [ln.split(",", 1)[1] for ln in open(path).read().strip().split("\n")[1:]]
    single = rows(str(tmp_path / "one.rank0.csv"))
    parts = [rows(str(tmp_path / f"two.rank{r}.csv")) for r in range(2)]
    assert all(parts) and sorted(parts[0] + parts[1]) == sorted(single)
    assert all(int(ln.split(",")[1]) <= 11 for ln in parts[0]) and all(int(ln.split(",")[1]) >= 12 for ln in parts[1])
    # the reference's rows for this run: ids, channels, lengths, decisions; probabilities within the tolerance
    assert len(single) == len(run["rows"])
    for ln, want in zip(single, run["rows"]):
        p = ln.split(",")
        assert (p[0], int(p[1]), int(p[2]), p[3], p[7]) == (want["read_id"], want["channel"], want["sig_length"],
                                                            want["models"], want["decision"])
        assert np.allclose([float(v) for v in p[4].split(";")], want["prob_targets"], atol=1e-3)
    # reject / finish lists per batch: the ranks' lists together are the single run's (and the reference's)
    s1 = json.load(open(str(tmp_path / "one.summary.json")))["per_rank"][0]
    s2 = json.load(open(str(tmp_path / "two.summary.json")))["per_rank"]
    for key, ref in (("rejected_lists", run["rejected"]), ("finished_lists", run["finished"])):
        assert s1[key] == ref
        for b in range(len(ref)):
            both = s2[0][key][b] + s2[1][key][b]
            assert sorted(map(tuple, both)) == sorted(map(tuple, ref[b]))
    assert two["reads_assessed"] == len(single) and two["rejected"] == sum(len(x) for x in run["rejected"])


def test_launch_from_a_model_directory_in_the_reference_layout(tmp_path, golden_dir):
    """--model-dir DIR --targets ... --kit RNA004: DIR/{target}_config_{kit}_{pore}.yaml + DIR/{target}_model_{kit}_{pore}.pth
    as riser/riser.py:26-42 lays them out (the .pth read by torch.load as riser/model.py:19 does, the YAML's `cnn` section
    as config.cnn).  The synthetic weights of golden run 5 saved that way and launched on two ranks reproduce the
    reference's rows for that run."""
    import torch
    with open(os.path.join(golden_dir, "control.json")) as f:
        g = json.load(f)
    run = g["runs"][5]
    names = ("mRNA", "mtRNA", "globin")
    targets = [names[k % 3] for k in range(len(run["seeds"]))]
    mdir = tmp_path / "model"
    mdir.mkdir()
    pore = {"RNA002": "R9.4.1", "RNA004": "RP4"}[g["kit"]]
    yaml_text = ("model: cnn\nbatch_size: 32\nn_epochs: 30\nlearning_rate: 0.0001\n\ncnn:\n  n_layers: 12\n  depth: 1\n"
                 "  channels: [20,30,45,67,100,150,225,337,505,757,1135,1702]\n  kernels: [3,3,3,3,3,3,3,3,3,3,3,3]\n"
                 "  n_classes: 2\n  classifier: gap_fc # fc / gap_fc / gap\n")
    for t, seed in zip(targets, run["seeds"]):
        (mdir / f"{t}_config_{g['kit']}_{pore}.yaml").write_text(yaml_text)
        torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(int(seed)).items()},
                   str(mdir / f"{t}_model_{g['kit']}_{pore}.pth"))
    two = _launch(["--gpus", "2", "--share-gpus", "--channels", "22", "--replay-script", os.path.join(golden_dir, "control.json"),
                   "--kit", g["kit"], "--mode", run["mode"], "--threshold", str(run["threshold"]), "--duration-h", "1.0",
                   "--model-dir", str(mdir), "--targets", ",".join(targets), "--out", str(tmp_path / "md")])
    rows = []
    for r in range(2):
        rows += [ln.split(",", 1)[1] for ln in open(str(tmp_path / f"md.rank{r}.csv")).read().strip().split("\n")[1:]]
    assert two["ranks"] == 2 and len(rows) == len(run["rows"])
    want = {(w["read_id"], w["channel"], w["sig_length"]): w for w in run["rows"]}      # a read is re-assessed as it grows
    assert len(want) == len(run["rows"])
    for ln in rows:
        p = ln.split(",")
        w = want.pop((p[0], int(p[1]), int(p[2])))
        assert (p[3], p[7]) == (w["models"], w["decision"])
        assert np.allclose([float(v) for v in p[4].split(";")], w["prob_targets"], atol=1e-3)
    assert not want


def test_four_ranks_share_the_gpu_on_the_live_config(tmp_path):
    """The N-rank live path (`bench.py --config promethion_live --gpus N`, gloo, every rank on the one GPU of the box): what
    the 8-GPU run does per rank - own channel range, own client, own models, barriers around K batches, one JSON line.
    Four ranks, not eight: a GPU box admits at most six processes on its card and this test process is one of them (the
    8-rank shape itself is rehearsed on CPU, tests/test_bench_cpu.py, tests/test_host_cpu.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["RS_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--config", "promethion_live",
                        "--reads-per-gpu", "64", "--steps", "6", "--warmup", "2"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["steps"] == 6 and out["config"]["channels_per_rank"] == 64
    assert out["value"] > 0 and out["reads_received_per_s"] >= out["value"] and out["latency_samples"] == 6


def test_bench_dump_outputs_are_what_the_timed_step_returned(dev, tmp_path):
    """`bench.py --dump-outputs DIR`: the probabilities of the last timed step are those of the same seeded batch classified
    here; on the live config, the channels of the last timed batch's rejected / finished reads"""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    quiet = ["--no-latency", "--no-variants", "--no-control-loop", "--no-cpu-baseline"]
    runs = {"b64": ["--batch", "64", "--steps", "3", "--warmup", "1", *quiet],
            "live": ["--config", "promethion_live", "--reads-per-gpu", "64", "--steps", "3", "--warmup", "1"]}
    for name, args in runs.items():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs",
                            str(tmp_path / name)], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0
    got = np.load(tmp_path / "b64" / "probs.npy")
    sigs = synth.make_signals(20260103, 64, 16000)
    m = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype="f32w", device=dev)
    want = m.classify_raw(*pack_reads(list(sigs), dev)).cpu().numpy()
    m.close()
    assert got.dtype == np.float32 and got.shape == (64, 2)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    rejected, finished = (np.load(tmp_path / "live" / f"{k}.npy") for k in ("rejected", "finished"))
    assert rejected.dtype == finished.dtype == np.float64 and rejected.ndim == finished.ndim == 1
    assert set(rejected.tolist()) <= set(finished.tolist()) <= set(range(1, 65))


def test_bench_plain_run_prints_the_headline_and_full_adds_the_side_passes():
    """a plain `bench.py` prints the headline and the roofline of the HIP events inside the timed steps, nothing that needs
    work after them; `--full` adds the per-launch pass (slowest layer, stage times), the latency fields and the detail file"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    base = ["--gpus", "1", "--steps", "3", "--warmup", "1"]
    quiet = ["--no-latency", "--no-variants", "--no-control-loop", "--no-cpu-baseline"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", *quiet])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *base, *extra], cwd=ROOT, capture_output=True,
                           text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(got) == 1
        lines[name] = json.loads(got[0])
    for out in lines.values():
        assert out["unit"] == "chunks/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
        assert out["steps"] == 3 and abs(out["value"] - 512 / (out["ms_per_step"] * 1e-3)) / out["value"] < 1e-3
        assert out["roofline"]["achieved"] > 0 and 0 < out["roofline"]["frac"] < 1
    plain, full = lines["plain"], lines["full"]
    assert not {"p50_batch_latency_ms", "latency_samples", "detail_file", "cpu_baseline", "control_loop"} & set(plain)
    assert not {"slowest_layer", "normalise_ms", "sustained_value"} & set(plain["roofline"])
    assert full["latency_samples"] == 0 and "detail_file" in full
    assert full["roofline"]["slowest_layer"] in range(1, 12) and full["roofline"]["normalise_ms"] > 0


@pytest.mark.parametrize("dtype", ["f32w", "f32", "bf16x3"])
def test_length_mismatch_is_contained_on_every_path(dev, dtype):
    """host lengths that disagree with the device's - above AND below - on the fused path of every dtype
    (the fp32 direct mode runs the stand-alone layer-0 kernel, which indexes len[] through the block table) and on
    rs_forward: the reads whose lengths agree keep their bits, a read the plan had to drop is NaN, nothing faults"""
    from riser_amd import Kit, Model, SignalProcessor
    from riser_amd.preprocess import pack_reads
    lens = np.array([5000, 9000, 4500, 16000, 6000], dtype=np.int32)
    sigs = [synth.make_signals(20260103, 1, int(n), first_read=3500 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    m = Model(synth.make_state_dict(1), synth.Config(), None, "m", dtype=dtype, device=dev)
    good = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    # the host understates read 3 (4096 instead of 16000; Lmax drops to 9000, so the device sees 3 blocks where the host
    # counted 1): the reads in FRONT of it keep their bits, read 3 itself is computed on a wrong length (its result is
    # meaningless), and the table runs out for read 4, which is dropped -> NaN
    lied = lh.copy()
    lied[3] = 4096
    out = m.classify_raw(sig, off, ln, lied).cpu().numpy()
    assert np.array_equal(out[:3], good[:3]) and np.isnan(out[4]).all()
    # the host overstates read 1 (device 3 blocks, host 4): a tail of the table stays unused; every read keeps its bits
    lied = lh.copy()
    lied[1] = 16000
    out = m.classify_raw(sig, off, ln, lied).cpu().numpy()
    assert np.array_equal(out, good)
    # rs_forward (signals that arrive normalised) with the same two lies
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    x = proc.normalise_device(sig, off, ln, len(lens), 16000)
    gf = m.forward_batch(x, lh, lens_dev=ln).cpu().numpy()
    assert np.abs(gf - good).max() < 1e-5
    lied = lh.copy()
    lied[3] = 4096
    of = m.forward_batch(x, lied, lens_dev=ln).cpu().numpy()
    assert np.array_equal(of[:3], gf[:3]) and np.isnan(of[4]).all()
    lied = lh.copy()
    lied[1] = 16000
    assert np.array_equal(m.forward_batch(x, lied, lens_dev=ln).cpu().numpy(), gf)
    assert np.array_equal(m.classify_raw(sig, off, ln, lh).cpu().numpy(), good)
    m.close()


@pytest.mark.parametrize("dtype", ["f32w", "bf16x3"])
def test_ensemble_concurrent_equals_serial(dev, dtype):
    """rs_classify_ensemble with rs_ensemble_workspace_bytes() runs its forwards concurrently (model 0 on the caller's
    stream, the others on side streams); with the single-model workspace, or RS_ENSEMBLE_SERIAL, back to back.  Same bits
    and same decisions, at a live-sized batch and repeatedly (a race between the forks would show as a changed bit)."""
    import ctypes as C
    from conftest import hooked_model
    from riser_amd import _native as nv
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    specs = ((1, "mRNA"), (2, "mtRNA"), (3, "globin"))
    models = [Model(synth.make_state_dict(k), synth.Config(), None, t, dtype=dtype, device=dev) for k, t in specs]
    rng = np.random.default_rng(4)
    lens = rng.integers(4096, 8616, size=150).tolist()
    sigs = [synth.make_signals(20260103, 1, n, first_read=900 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    B = len(lens)
    dec = torch.empty(B, dtype=torch.uint8, device=dev)
    want = torch.stack([m.classify_raw(sig, off, ln, lh) for m in models])
    for _ in range(4):
        got = classify_raw_ensemble(models, sig, off, ln, lh, decision=dec, max_len=8615, threshold=0.9)
        assert torch.equal(got, want)
    dec_par = dec.clone()
    # the single-model workspace: the serial order through the same entry point
    L = nv.lib()
    hs = (C.c_void_p * 3)(*[m._h for m in models])
    small = max(L.rs_workspace_bytes(m._h, B, int(lh.max())) for m in models)
    assert small < L.rs_ensemble_workspace_bytes(hs, 3, B, int(lh.max()))
    ws = torch.empty(small, dtype=torch.uint8, device=dev)
    out = torch.empty((3, B, 2), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    nv.check(L.rs_classify_ensemble(hs, 3, sig.data_ptr(), off.data_ptr(), ln.data_ptr(), lh.ctypes.data, B, int(lh.min()),
                                    int(lh.max()), ws.data_ptr(), ws.numel(), out.data_ptr(), dec.data_ptr(), 8615, 0.9,
                                    nv.RS_ENRICH, st), "rs_classify_ensemble")
    assert torch.equal(out, want) and torch.equal(dec, dec_par)
    assert L.rs_classify_ensemble(hs, 3, sig.data_ptr(), off.data_ptr(), ln.data_ptr(), lh.ctypes.data, B, int(lh.min()),
                                  int(lh.max()), ws.data_ptr(), small - 4096, out.data_ptr(), None, 8615, 0.9, nv.RS_ENRICH,
                                  st) == -5                                      # RS_ERR_WORKSPACE
    serial = [hooked_model({"RS_ENSEMBLE_SERIAL": "1"}, synth.make_state_dict(k), dtype, dev, target=t) for k, t in specs]
    assert torch.equal(classify_raw_ensemble(serial, sig, off, ln, lh), want)
    for m in models + serial:
        m.close()


@pytest.mark.parametrize("traffic", ["whole", "chunks", "whole_no_store"])
def test_sliced_pipeline_equals_one_slice(dev, tmp_path, monkeypatch, traffic):
    """a PromethION-scale batch is assessed in slices pipelined over two streams (upload / poly(A) scan of slice k + 1 under
    the kernels of slice k): forced onto 150-channel batches (slices of ~16 reads) it writes the same rows and sends the
    same lists as the single-slice path, with the signal store, with a chunk client (store switched off mid-run) and without
    the store; reads longer than a store row (spill area) and duplicate channels in one batch included"""
    from riser_amd import Kit, Model, SignalProcessor
    from riser_amd.control import SequencerControl
    from riser_amd.replay import chunked_batches, scripted_batches
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    models = [Model(synth.make_state_dict(s), synth.Config(), None, f"t{s}", device=dev) for s in (1, 3)]
    batches = chunked_batches(9, 150) if traffic == "chunks" else scripted_batches(7, 150)
    long_read = FakeRead("long", synth.make_raw_read(5, 5, 40000, True))
    batches[2].append((3000, long_read))
    batches[3].append((3000, long_read))
    batches[4].append((7, FakeRead("dup-channel", synth.make_raw_read(5, 6, 15000, True))))     # channel 7 twice in one batch
    cache = traffic != "whole_no_store"
    one = _run(batches, models, proc, str(tmp_path / "one"), signal_cache=cache)
    monkeypatch.setattr(SequencerControl, "SLICE_READS", 16)
    many = _run(batches, models, proc, str(tmp_path / "many"), signal_cache=cache)
    assert many[:3] == one[:3] and len(one[0]) > (40 if traffic == "chunks" else 300)
    assert many[3]._side is not None and one[3]._side is None               # the pipeline really ran / really did not
    for m in models:
        m.close()


def test_random_traffic_stateful_paths_equal_the_plain_loop(dev, tmp_path):
    """Random ReadUntil traffic against the loop's STATE: 48 channels x 150 batches in which a read may grow by 0 ... 3000
    samples, pause (its channel missing from a batch), end (a new read, new id, takes the channel), come back under its id
    with OTHER samples (a re-based buffer), or shrink.  The signal store's rows, the verified delta path and the resumed
    poly(A) scans (control.py: row_have / row_tail / row_pa) must be invisible: same CSV rows and the same reject / finish
    calls, batch by batch, as the loop that uploads every read whole and scans it from its first sample
    (signal_cache=False); both also through the plain duck type."""
    from riser_amd import Kit, Model, SignalProcessor
    rng = np.random.default_rng(20260110)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    models = [Model(synth.make_state_dict(1), synth.Config(), None, "t1", dtype="bf16x3", device=dev)]
    C, NB = 48, 150
    serial = [0]

    def new_read():
        serial[0] += 1
        n = int(rng.integers(3000, 26000))
        return {"id": f"r{serial[0]}", "sig": synth.make_raw_read(31, serial[0], n, polya=bool(rng.random() < 0.75)),
                "seen": int(rng.integers(500, 3000))}

    chan = [new_read() for _ in range(C)]
    batches = []
    for b in range(NB):
        reads = []
        for c in range(C):
            r = chan[c]
            u = rng.random()
            if u < 0.06 or r["seen"] >= len(r["sig"]):
                chan[c] = r = new_read()                                    # the strand left: a new read in the pore
            elif u < 0.09:
                r["sig"] = synth.make_raw_read(37, serial[0] + 1000 + b, len(r["sig"]), polya=True)   # same id, other samples
            elif u < 0.12:
                r["seen"] = max(400, r["seen"] - int(rng.integers(1, 900)))  # shorter than last time
            elif u < 0.80:
                r["seen"] = min(len(r["sig"]), r["seen"] + int(rng.integers(0, 3000)))
            if rng.random() < 0.1:
                continue                                                    # not in this batch
            reads.append((c + 1, FakeRead(r["id"], r["sig"][: r["seen"]])))
        batches.append(reads)
    runs = [_run(batches, models, proc, str(tmp_path / f"f{k}"), cls, cache)
            for k, (cls, cache) in enumerate(((FakeClient, True), (FakeClient, False), (PlainFakeClient, True)))]
    assert len(runs[0][0]) > 300
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and r[2] == runs[0][2]
    store = runs[0][3]._store
    assert store.delta_reads > 1000 and store.mismatches > 20 and store.resident     # every path was taken
    for m in models:
        m.close()

