"""Further GPU checks: state-dict file loading, RNA002 kit control loop against the oracle,
cache behaviour, randomised property tests."""
import logging
import os

import numpy as np
import pytest
import torch

from oracle import riser_oracle as ro
from oracle import torch_path
from riser_amd import _native as nv
from riser_amd import synth
from riser_amd.fake_client import FakeClient, FakeRead

pytestmark = pytest.mark.gpu
SIG_SEED = 20260103


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def test_model_loads_pth_like_the_reference(dev, tmp_path):
    """riser/model.py:19 does torch.load(state); the same file must load here."""
    from riser_amd.model import Model
    sd = synth.make_state_dict(2)
    path = str(tmp_path / "mRNA_model_RNA004_RP4.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    log = logging.getLogger("x")
    m = Model(path, synth.Config(), log, "mRNA", device=dev)
    assert m.target == "mRNA" and m.logger is log and m.device.type == "cuda"
    x = ro.mad_normalise(synth.make_signals(SIG_SEED, 1, 6024, first_read=1)[0])
    assert np.abs(m.classify(x).cpu().numpy() - ro.classify(sd, x)).max() < 1e-3
    bad = dict(sd)
    bad["layers.3.0.weight"] = bad["layers.3.0.weight"][:, :10]
    with pytest.raises(ValueError):
        Model(bad, synth.Config(), log, "mRNA", device=dev)
    with pytest.raises(ValueError):                   # the reference exits on a classifier it does not know (cnn.py:39-41)
        Model(sd, synth.Config(synth.CnnConfig(classifier="softmax")), log, "mRNA", device=dev)
    for clf in ("gap", "fc"):                         # their configs need their own keys (classifier.0.* / classifier.1.*, .3.*)
        with pytest.raises(KeyError):
            Model(sd, synth.Config(synth.CnnConfig(classifier=clf)), log, "mRNA", device=dev)
    m.close()


def _oracle_loop(batches, kit, seeds, mode, thr, cache_models):
    """riser/control.py:31-97 restated with the oracle pieces -> (rows, rejected, finished)."""
    max_len, fixed = ro.kit_max_length(kit), ro.kit_fixed_trim_length(kit)
    cache, rows, rej_all, fin_all = {}, [], [], []
    for batch in batches:
        rej, acc, unc = [], [], []
        for ch, read in batch:
            sig = np.frombuffer(read.raw_data, np.int16)
            sig, trimmed = ro.trim_polya(sig, read.id, cache)
            if not trimmed:
                if len(sig) > fixed + max_len:
                    sig = sig[fixed:][:max_len]
                else:
                    continue
            else:
                if len(sig) < ro.MIN_INPUT_SIGNALS:
                    continue
                sig = sig[:max_len]
            x = ro.mad_normalise(sig)
            ps = [cache_models[s].classify(x).numpy() for s in seeds]
            d = ro.decide([p[1] for p in ps], [p[0] for p in ps], thr, mode, len(sig), max_len)
            rid = read.number if hasattr(read, "number") else read.id
            {"accept": acc, "reject": rej, "no_decision": unc}.get(d, []).append((ch, rid))
            rows.append((read.id, ch, len(sig), d, [float(p[1]) for p in ps]))
        rej_all.append(rej)
        fin_all.append(rej + acc + unc)
    return rows, rej_all, fin_all


@pytest.mark.parametrize("kit,seeds,mode", [("RNA002", (1,), "deplete"), ("RNA002", (2, 3), "enrich"),
                                            ("RNA004", (3,), "deplete")])
def test_control_loop_vs_oracle_loop(dev, tmp_path, kit, seeds, mode):
    from riser_amd import Kit, Model, SequencerControl, SignalProcessor
    rng = np.random.default_rng(hash((kit, seeds)) % 2**32)
    batches = []
    for b in range(3):
        reads = []
        for ch in range(1, 41):
            rid = b * 7 + ch
            n = int(rng.integers(3000, 26000))
            rd = FakeRead(f"id-{rid}", synth.make_raw_read(55, rid, n, polya=(rid % 4 != 0)),
                          number=(rid if rid % 2 else None))
            reads.append((ch, rd))
        batches.append(reads)
    cpu_models = {s: torch_path.TorchCpuModel(synth.make_state_dict(s)) for s in seeds}
    want_rows, want_rej, want_fin = _oracle_loop(batches, kit, seeds, mode, 0.9, cpu_models)
    models = [Model(synth.make_state_dict(s), synth.Config(), None, f"t{s}", device=dev) for s in seeds]
    proc = SignalProcessor(Kit.create_from_version(kit), device=dev)
    client = FakeClient(batches)
    out = str(tmp_path / "o")
    ctl = SequencerControl(client, models, proc, logging.getLogger("c"), out)
    ctl.start(); ctl.target(mode, 0.5, 0.9); ctl.finish()
    lines = open(out + ".csv").read().strip().split("\n")[1:]
    assert len(lines) == len(want_rows) > 20
    near = 0
    for ln, w in zip(lines, want_rows):
        p = ln.split(",")
        assert (p[1], int(p[2]), int(p[3])) == w[:3]
        got_p = [float(v) for v in p[5].split(";")]
        assert np.allclose(got_p, w[4], atol=1e-3)
        if any(abs(q - 0.9) < 1e-4 or abs(1 - q - 0.9) < 1e-4 for q in w[4]):
            near += 1                                   # a probability within 1e-4 of the threshold may flip
            continue
        assert p[8] == w[3], (p, w)
    assert near <= 1
    if near == 0:
        assert [[tuple(x) for x in b] for b in client.rejected] == want_rej
        assert [[tuple(x) for x in b] for b in client.finished] == want_fin
    for m in models:
        m.close()


def test_control_rejects_bad_mode_and_handles_empty_batches(dev, tmp_path):
    from riser_amd import Kit, Model, SequencerControl, SignalProcessor
    m = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", device=dev)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    short = FakeRead("s", synth.make_raw_read(1, 1, 3000, True))
    client = FakeClient([[], [(1, short)], []])
    ctl = SequencerControl(client, [m], proc, logging.getLogger("c"), str(tmp_path / "e"))
    with pytest.raises(ValueError):
        ctl.target("purify", 1.0, 0.9)
    ctl.target("enrich", 1.0, 0.9)
    assert client.rejected == [[], [], []] and client.finished == [[], [], []]
    assert open(str(tmp_path / "e.csv")).read().count("\n") == 1        # header only (the bad mode raised before the file was opened)
    m.close()


def test_polya_cache_is_used_and_bounded(dev):
    from riser_amd import Kit, SignalProcessor
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    sig = synth.make_raw_read(9, 2, 15000, True)
    cache = {}
    a, ok = proc.trim_polya(sig, "r", cache) if hasattr(proc, "trim_polya") else proc.trim_polyA(sig, "r", cache)
    assert ok and "r" in cache
    cache["r"] = 123                                       # a cached value is trusted, as in the reference
    b, ok2 = proc.trim_polyA(sig, "r", cache)
    assert ok2 and len(b) == len(sig) - 124


def test_random_batches_property(dev):
    """random lengths / offsets / batch sizes: every read's result equals its solo result bit for
    bit and the oracle within tolerance."""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    m = Model(synth.make_state_dict(3), synth.Config(), None, "g", device=dev)
    sd = synth.make_state_dict(3)
    rng = np.random.default_rng(2026)
    for trial in range(4):
        B = int(rng.integers(1, 40))
        lens = rng.integers(4096, 20000, B)
        sigs = [synth.make_signals(SIG_SEED + trial, 1, int(n) + 50, first_read=int(i))[0] for i, n in enumerate(lens)]
        sig, off, ln, lh = pack_reads(sigs, dev)
        trim = rng.integers(0, 50, B)
        off2 = off + torch.from_numpy(trim.astype(np.int64)).to(dev)
        ln2 = torch.from_numpy(lens.astype(np.int32)).to(dev)
        got = m.classify_raw(sig, off2, ln2, lens.astype(np.int32)).cpu().numpy()
        k = int(rng.integers(0, B))
        solo = m.classify_raw(sig, off2[k:k + 1].contiguous(), ln2[k:k + 1].contiguous(), lens[k:k + 1].astype(np.int32)).cpu().numpy()
        assert np.array_equal(solo[0], got[k])
        want = ro.classify_reads(sd, [sigs[k][trim[k]:trim[k] + lens[k]]])
        assert np.abs(got[k] - want[0]).max() < 1e-3
    m.close()


@pytest.mark.parametrize("dtype", ["f32w", "f16"])
def test_large_ragged_batch_tile_order(dev, dtype):
    """A few hundred reads of mixed lengths: the persistent tile walk runs with XCD blocks as gm x gn rectangles
    (rectangles may overhang the tile grid: invalid order indices are skipped) AND dead-tile elimination.  Every read
    must come out bit-identical to its result in a small batch (n-major order, grid below the CU count) and to the
    n-major order of the same large batch; a sample is checked against the oracle."""
    import os
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    sd = synth.make_state_dict(2)
    from conftest import hooked_model
    m = Model(sd, synth.Config(), None, "m", dtype=dtype, device=dev)
    m_nmajor = hooked_model({"RS_NO_RECT_ORDER": "1"}, sd, dtype, dev)
    rng = np.random.default_rng(77)
    for B in (437, 300):
        lens = rng.choice([4096, 6024, 8000, 8615, 12000, 16000], size=B).astype(np.int32)
        lens[0] = 16000
        sigs = [synth.make_signals(SIG_SEED, 1, int(n), first_read=2000 + i)[0] for i, n in enumerate(lens)]
        sig, off, ln, lh = pack_reads(sigs, dev)
        full = m.classify_raw(sig, off, ln, lh).cpu().numpy()
        assert np.array_equal(full, m_nmajor.classify_raw(sig, off, ln, lh).cpu().numpy())
        idx = np.sort(rng.choice(B, size=23, replace=False))
        tidx = torch.from_numpy(idx).to(dev)
        part = m.classify_raw(sig, off[tidx].contiguous(), ln[tidx].contiguous(), lh[idx]).cpu().numpy()
        assert np.array_equal(part, full[idx])
        pick = idx[:3]
        want = ro.classify_reads(sd, [sigs[k] for k in pick])
        assert np.abs(full[pick] - want).max() < (1e-3 if dtype == "f32w" else 2e-2)
    m.close()
    m_nmajor.close()


def test_autotune_keeps_results(dev):
    """rs_autotune (optional tile-shape tuning per batch geometry): fp32 results stay bit-identical whatever it
    picks; 16-bit results stay within 16-bit round-off (it may switch a layer to 64-channel panels); other batch
    geometries keep using the launch planner."""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    B = 160
    lens = np.full(B, 12000, dtype=np.int32)
    lens[::5] = 8000
    sigs = [synth.make_signals(SIG_SEED, 1, int(n), first_read=900 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    for dtype, tol in (("f32w", 0.0), ("f16", 5e-3)):
        m = Model(synth.make_state_dict(1), synth.Config(), None, "m", dtype=dtype, device=dev)
        before = m.classify_raw(sig, off, ln, lh).cpu().numpy()
        small = m.classify_raw(sig, off[:7].contiguous(), ln[:7].contiguous(), lh[:7]).cpu().numpy()
        changed = m.autotune(sig, off, ln, lh)
        assert changed >= 0
        after = m.classify_raw(sig, off, ln, lh).cpu().numpy()
        assert np.abs(after - before).max() <= tol, (dtype, changed)
        assert np.array_equal(after, m.classify_raw(sig, off, ln, lh).cpu().numpy())
        # another geometry is untouched by the tuned entries
        assert np.array_equal(small, m.classify_raw(sig, off[:7].contiguous(), ln[:7].contiguous(), lh[:7]).cpu().numpy())
        m.autotune(sig, off, ln, lh)                                           # re-tuning replaces, never accumulates
        assert np.abs(m.classify_raw(sig, off, ln, lh).cpu().numpy() - before).max() <= tol
        m.close()


def test_stream_classifier_matches_direct(dev):
    """host-resident reads streamed in sub-batches (copy/compute overlap) == one direct call."""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    from riser_amd.stream import StreamClassifier
    m = Model(synth.make_state_dict(1), synth.Config(), None, "m", device=dev)
    N, L = 300, 6024
    sigs = synth.make_signals(SIG_SEED, N, L)
    lens = np.full(N, L, dtype=np.int32)
    lens[::7] = 4500
    sc = StreamClassifier([m], sub_batch=64, max_len=L)
    got = sc.classify(sigs, lens)
    sig, off, ln, _ = pack_reads(list(sigs), dev)
    want = m.classify_raw(sig, off, torch.from_numpy(lens).to(dev), lens).cpu().numpy()
    assert got.shape == (1, N, 2) and np.array_equal(got[0], want)
    got2 = sc.classify(torch.from_numpy(sigs).pin_memory(), lens)          # pinned input path
    assert np.array_equal(got2[0], want)
    m.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16", "bf16x3", "f16x3"])
def test_h16_streaming_layers_and_layer0_fold(dev, dtype):
    """16-bit narrow layers: the per-wave streaming kernels - layers 0+1+2 in one launch (the default), layers 0+1
    and 2 as two launches (RS_NO_STREAM012), layers 1 and 2 behind the stand-alone layer-0 kernel - must reproduce
    the tiled 16-bit kernel bit for bit (same MFMA sequence, same roundings; layer 0 on the f32-input MFMA is the
    same fmaf chain), on full-length and mixed-length batches, and stay within the mode's tolerance of the oracle."""
    import os
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    sd = synth.make_state_dict(2)
    from conftest import hooked_model
    m = Model(sd, synth.Config(), None, "m", dtype=dtype, device=dev)
    m_tiled = hooked_model({"RS_NO_STREAM_H16": "1"}, sd, dtype, dev)
    m_two = hooked_model({"RS_NO_STREAM012": "1"}, sd, dtype, dev)
    tol = {"f16": 2e-2, "bf16": 1.5e-1, "bf16x3": 1e-3, "f16x3": 1e-3}[dtype]
    for lens in ([16000] * 6, [4096, 16000, 8615, 5000, 12001, 4097, 16383, 9999]):
        sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=300 + i)[0] for i, n in enumerate(lens)]
        sig, off, ln, lh = pack_reads(sigs, dev)
        xs = [ro.mad_normalise(s) for s in sigs]
        fused = m.classify_raw(sig, off, ln, lh).cpu().numpy()               # layer 0 folded into layer 1
        stream = m.classify_batch(xs).cpu().numpy()                          # conv0 kernel + streaming layers 1-2
        tiled = m_tiled.classify_raw(sig, off, ln, lh).cpu().numpy()     # conv0 kernel + tiled kernel everywhere
        two = m_two.classify_raw(sig, off, ln, lh).cpu().numpy()             # layers 0+1, then layer 2
        assert np.array_equal(fused, two), np.abs(fused - two).max()
        assert np.array_equal(fused, stream), np.abs(fused - stream).max()
        assert np.array_equal(fused, tiled), np.abs(fused - tiled).max()
        want = np.stack([ro.classify(sd, x) for x in xs])
        assert np.abs(fused - want).max() < tol
    m.close()
    m_tiled.close()
    m_two.close()


def test_config3_ensemble_split_precision_full_size(dev):
    """BASELINE config 3 at full size: the mRNA + mtRNA + globin stand-ins, 512 x 16000-sample chunks, one
    rs_classify_ensemble call on the 16-bit MFMA in split precision (bf16x3).  Against the ORACLE on all 512 reads of all
    three models: every probability within 1e-3, and every accept / reject / no-decision identical to the reference's
    rule (riser/control.py:75-82, oracle decide()) applied to the oracle's probabilities, in both modes; the same against
    the library's own fp32 ensemble; and the single call equals three rs_classify calls + rs_decide bit for bit."""
    from conftest import oracle_bench_batch
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    B, L = 512, 16000
    spec = ((1, "mRNA"), (2, "mtRNA"), (3, "globin"))
    x3 = [Model(synth.make_state_dict(k), synth.Config(), None, t, dtype="bf16x3", device=dev) for k, t in spec]
    f32 = [Model(synth.make_state_dict(k), synth.Config(), None, t, dtype="f32w", device=dev) for k, t in spec]
    sigs = synth.make_signals(SIG_SEED, B, L)
    sig, off, ln, lh = pack_reads(list(sigs), dev)
    for mode in (nv.RS_ENRICH, nv.RS_DEPLETE):
        dec = torch.empty(B, dtype=torch.uint8, device=dev)
        dec32 = torch.empty(B, dtype=torch.uint8, device=dev)
        p = classify_raw_ensemble(x3, sig, off, ln, lh, decision=dec, max_len=L, threshold=0.9, mode=mode)
        p32 = classify_raw_ensemble(f32, sig, off, ln, lh, decision=dec32, max_len=L, threshold=0.9, mode=mode)
        assert float((p - p32).abs().max()) < 1e-3
        assert torch.equal(dec, dec32), int((dec != dec32).sum())
        po = np.stack([oracle_bench_batch(k, "full") for k, _ in spec])                       # [3, 512, 2]
        for probs in (p, p32):
            assert np.abs(probs.cpu().numpy() - po).max() < 1e-3
        want_dec = [ro.decide(list(po[:, b, 1]), list(po[:, b, 0]), 0.9, "enrich" if mode == nv.RS_ENRICH else "deplete", L, L)
                    for b in range(B)]
        got_dec = [nv.DECISION_NAMES[int(d)] for d in dec.cpu().numpy()]
        assert got_dec == want_dec, sum(a != b for a, b in zip(got_dec, want_dec))
        assert torch.equal(p, torch.stack([m.classify_raw(sig, off, ln, lh) for m in x3]))
        counts = np.bincount(dec.cpu().numpy(), minlength=4)
        # a discriminating population: reads on both sides of the threshold (any model on-target: accepted when
        # enriching, rejected when depleting; the rest are at maximum length, so no "try again")
        decided = counts[nv.RS_ACCEPT if mode == nv.RS_ENRICH else nv.RS_REJECT]
        assert decided > 10 and B - decided > 10 and counts[nv.RS_TRY_AGAIN] == 0, counts
    for m in x3 + f32:
        m.close()


@pytest.mark.parametrize("dtype", ["f32w", "f16", "bf16x3"])
def test_classify_ensemble_entry(dev, dtype):
    """rs_classify_ensemble (normalise once, N forwards, decision on the device) == N x rs_classify + rs_decide."""
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    models = [Model(synth.make_state_dict(k), synth.Config(), None, t, dtype=dtype, device=dev)
              for k, t in ((1, "mRNA"), (2, "mtRNA"), (3, "globin"))]
    lens = [8615, 4096, 6000, 8615, 5123, 7777, 8000]
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=700 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    B = len(lens)
    for mode in (nv.RS_ENRICH, nv.RS_DEPLETE):
        dec = torch.empty(B, dtype=torch.uint8, device=dev)
        probs = classify_raw_ensemble(models, sig, off, ln, lh, decision=dec, max_len=8615, threshold=0.9, mode=mode)
        want = torch.stack([m.classify_raw(sig, off, ln, lh) for m in models])
        assert torch.equal(probs, want)
        dec2 = torch.empty(B, dtype=torch.uint8, device=dev)
        nv.check(nv.lib().rs_decide(want.contiguous().data_ptr(), 3, B, ln.data_ptr(), 8615, 0.9, mode, dec2.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
        assert torch.equal(dec, dec2)
    # argument checks
    with pytest.raises(nv.NativeError):
        other = Model(synth.make_state_dict(1), synth.Config(), None, "x", dtype="f16" if dtype == "f32w" else "f32w", device=dev)
        classify_raw_ensemble([models[0], other], sig, off, ln, lh)
    for m in models:
        m.close()


def test_oversized_batches_are_split(dev, monkeypatch):
    """batches beyond the 2 GiB buffer window of one library call are split by the host classes: force the
    split with a tiny limit and compare with the unsplit call (reads are independent: bit-identical)."""
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    m = Model(synth.make_state_dict(1), synth.Config(), None, "m", device=dev)
    assert 2000 < m.max_batch(16000) < 4000
    lens = [4096, 8615, 5000, 7000, 8000, 6024, 4100, 8192, 4500, 6666, 7777]
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=900 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    xs = [ro.mad_normalise(s) for s in sigs]
    want_raw = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    want_b, want_l = m.classify_batch(xs, return_logits=True)
    want_e = classify_raw_ensemble([m, m], sig, off, ln, lh).cpu().numpy()
    monkeypatch.setattr(Model, "max_batch", lambda self, lmax: 4)
    got_raw, got_rl = m.classify_raw(sig, off, ln, lh, return_logits=True)
    got_b, got_l = m.classify_batch(xs, return_logits=True)
    dec = torch.empty(len(lens), dtype=torch.uint8, device=dev)
    got_e = classify_raw_ensemble([m, m], sig, off, ln, lh, decision=dec, max_len=8615).cpu().numpy()
    assert np.array_equal(got_raw.cpu().numpy(), want_raw)
    assert torch.equal(got_b, want_b) and torch.equal(got_l, want_l) and torch.equal(got_rl, want_l)
    assert np.array_equal(got_e, want_e)
    m.close()


def test_gap_classifier_against_reference(dev, golden_dir):
    """`gap` head (riser/nets/cnn.py:34-38): batches of 3 reads against the reference's ConvNet.forward + softmax, on the
    shipped architecture (every dtype mode that claims 1e-3) and on a depth-2 net (generic conv program); Model.classify
    of ONE read raises what the reference raises."""
    from test_oracle_golden import _gap_cases
    from riser_amd.model import Model
    for name, cfg, sd, want, err in _gap_cases(golden_dir):
        config = synth.Config(synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"],
                                              classifier="gap"))
        for dt in (("f32w", "f32", "bf16x3", "f16x3") if cfg["depth"] == 1 else ("f32w",)):
            m = Model(sd, config, None, "x", dtype=dt, device=dev)
            for j, (L, probs) in enumerate(want.items()):
                sigs = synth.make_signals(SIG_SEED, 3, L, first_read=90 + 3 * j)
                got = m.classify_batch([ro.mad_normalise(s) for s in sigs]).cpu().numpy()
                assert np.abs(got - probs).max() < 1e-3, (name, dt, L)
                assert np.array_equal(got[:, 1] > 0.9, probs[:, 1] > 0.9)
            with pytest.raises(IndexError):
                m.classify(ro.mad_normalise(sigs[0]))
            m.close()


def test_fc_classifier_against_reference(dev, golden_dir):
    """`fc` head (riser/nets/cnn.py:22-27: Flatten -> Linear(67 * 753, 4096) -> ReLU -> Linear(4096, 2)) behind the 4-layer
    conv stack: Model.classify per read against the reference's own probabilities, the same reads batched (normalised
    and raw entry points, with a batch large enough to leave the split-K regime), both fp32 lowerings; a read of another
    length raises what the reference raises; through the C ABI without host lengths such a read comes back as NaN."""
    import json
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    g = np.load(os.path.join(golden_dir, "fc_head.npz"))
    sd = synth.make_fc_state_dict(1)
    config = synth.Config(synth.CnnConfig(channels=list(synth.FC_CHANNELS), kernels=[3] * 4, classifier="fc"))
    lens, want = g["lens"], g["probs"]
    sigs = [synth.make_signals(SIG_SEED, 1, int(L), first_read=120 + j)[0] for j, L in enumerate(lens)]
    xs = [ro.mad_normalise(s) for s in sigs]
    for dt in ("f32w", "f32"):
        m = Model(sd, config, None, "x", dtype=dt, device=dev)
        for j, x in enumerate(xs):
            one = m.classify(x).cpu().numpy()
            assert one.shape == (2,) and np.abs(one - want[j]).max() < 1e-3, (dt, j)
        got = m.classify_batch(xs).cpu().numpy()
        assert np.abs(got - want).max() < 1e-3 and np.array_equal(got[:, 1] > 0.9, want[:, 1] > 0.9)
        sig, off, ln, lh = pack_reads(sigs * 8, dev)                         # 40 reads: three 16-read tiles, fewer K splits
        raw = m.classify_raw(sig, off, ln, lh).cpu().numpy()
        assert np.abs(raw - np.tile(want, (8, 1))).max() < 1e-3
        assert np.array_equal(raw[:5], raw[35:])                             # the same read gives the same bits in any tile
        dec = torch.empty(len(lh), dtype=torch.uint8, device=dev)
        ens = classify_raw_ensemble([m], sig, off, ln, lh, decision=dec, max_len=12048).cpu().numpy()
        assert np.array_equal(ens[0], raw)
        for L, err in json.loads(str(g["errors"])).items():
            assert err == "RuntimeError"
            with pytest.raises(RuntimeError):
                m.classify(ro.mad_normalise(synth.make_signals(SIG_SEED, 1, int(L), first_read=130)[0]))
        # a caller of the C ABI that passes no host lengths: the odd read is NaN, its neighbours are untouched
        odd = sigs[:2] + [synth.make_signals(SIG_SEED, 1, 12064, first_read=130)[0]] + sigs[2:]
        sig, off, ln, lh = pack_reads(odd, dev)
        from riser_amd import _native as nv
        import ctypes as C
        Lb = nv.lib()
        ws = torch.empty(Lb.rs_workspace_bytes(m._h, len(odd), 12064), dtype=torch.uint8, device=dev)
        probs = torch.empty((len(odd), 2), dtype=torch.float32, device=dev)
        nv.check(Lb.rs_classify(m._h, sig.data_ptr(), off.data_ptr(), ln.data_ptr(), None, len(odd), 12048, 12064,
                                ws.data_ptr(), ws.numel(), probs.data_ptr(), None, None), "rs_classify")
        torch.cuda.synchronize()
        p = probs.cpu().numpy()
        assert np.isnan(p[2]).all() and np.abs(np.delete(p, 2, axis=0) - want).max() < 1e-3
        m.close()
    with pytest.raises(ValueError):
        Model(sd, config, None, "x", dtype="bf16x3", device=dev)


def test_split_precision_and_the_range_of_the_numbers(dev):
    """ReLU networks are positively homogeneous: scaling layer 5's weights and bias by s and layer 6's weights by 1 / s leaves
    the function unchanged, but moves layer 5's activations (and layer 6's weights) by s through the number formats.
    fp32 and bf16x3 (fp32's exponent range) must not care - held to the 1e-3 tolerance at s = 1e3 and 1e5.  f16x3 packs its
    weights with a power-of-two scale per layer (ConvLayerDev::w_unscale), so SMALL weights cost it nothing: held to 1e-4 at
    s = 1e3 (1.8e-3 before the scale); its activations must stay below 65504: at s = 1e5 it is merely
    required to stay finite."""
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    sigs = list(synth.make_signals(SIG_SEED, 24, 8000, first_read=500))
    sig, off, ln, lh = pack_reads(sigs, dev)
    base = synth.make_state_dict(1)
    ref = None
    for scale in (1.0, 1e3, 1e5):
        sd = dict(base)
        sd["layers.5.0.weight"] = base["layers.5.0.weight"] * np.float32(scale)
        sd["layers.5.0.bias"] = base["layers.5.0.bias"] * np.float32(scale)
        sd["layers.6.0.weight"] = base["layers.6.0.weight"] / np.float32(scale)
        for dt in ("f32w", "bf16x3", "f16x3"):
            m = Model(sd, synth.Config(), None, "m", dtype=dt, device=dev, range_check=False)
            p = m.classify_raw(sig, off, ln, lh).cpu().numpy()
            over = m.saturated()
            m.close()
            if ref is None:
                ref = p
            assert np.isfinite(p).all(), (dt, scale)
            assert over == (dt == "f16x3" and scale == 1e5), (dt, scale, over)        # the sticky flag of rs_model_saturated
            if dt != "f16x3" or scale <= 1e3:
                assert np.abs(p - ref).max() < (1e-4 if dt == "f16x3" else 1e-3), (dt, scale, float(np.abs(p - ref).max()))
                assert np.array_equal(p[:, 1] > 0.9, ref[:, 1] > 0.9), (dt, scale)


@pytest.mark.parametrize("dtype", ["f16x3", "f16xf8", "f16"])
def test_half_precision_overflow_fails_loudly(dev, dtype):
    """VERDICT round 5, item 2.  The half-precision modes cannot represent an activation beyond 65504; the reference's fp32 call
    (riser/model.py:22-28) can.  (a) Model() runs a synthetic sample through a new half-precision model and REFUSES weights whose
    activations come within x4 of that limit, naming the layer and the modes that do work; (b) loaded anyway (range_check=False),
    every epilogue checks its conversions: the launch still returns, `saturated()` is True (sticky, cleared by the read),
    `classify()` raises a RuntimeWarning and the control loop logs one per batch; (c) on the calibrated weights nothing fires;
    bf16x3 / fp32 never report (fp32's exponent range).  The scaled network is the SAME function (ReLU nets are positively
    homogeneous: layer 7 x s, layer 8 / s), so its fp32 result is the reference."""
    import logging
    import warnings
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    from riser_amd.replay import scripted_batches
    sigs = list(synth.make_signals(SIG_SEED, 24, 8000, first_read=900))
    sig, off, ln, lh = pack_reads(sigs, dev)
    base = synth.make_state_dict(1)
    ok = Model(base, synth.Config(), None, "m", dtype=dtype, device=dev)            # (c): passes the range check
    want = ok.classify_raw(sig, off, ln, lh).cpu().numpy()
    assert not ok.saturated()
    mx = ok.half_activation_maxima()
    assert len(mx) == 11 and all(0 < v < 65504 / 4 for v in mx)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ok.classify(ro.mad_normalise(sigs[0]))                                        # no warning on sane weights
    ok.close()
    layer = 7                                                                          # a layer of the 8-bit run in f16xf8
    s = np.float32(2.0 ** 14)
    sd = dict(base)
    sd[f"layers.{layer}.0.weight"] = base[f"layers.{layer}.0.weight"] * s
    sd[f"layers.{layer}.0.bias"] = base[f"layers.{layer}.0.bias"] * s
    sd[f"layers.{layer + 1}.0.weight"] = base[f"layers.{layer + 1}.0.weight"] / s
    with pytest.raises(ValueError, match=f"conv layer {layer} .* 'bf16x3'"):           # (a)
        Model(sd, synth.Config(), None, "big", dtype=dtype, device=dev)
    m = Model(sd, synth.Config(), None, "big", dtype=dtype, device=dev, range_check=False)          # (b)
    assert not m.saturated()
    p = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    assert p.shape == want.shape                                                      # the call itself returns
    assert m.saturated() and not m.saturated()                                        # sticky until read, then cleared
    with pytest.warns(RuntimeWarning, match="overflowed half precision"):
        m.classify(ro.mad_normalise(sigs[1]))
    assert not m.saturated()
    # the control loop: one warning per batch in the log, the batch still goes through
    records = []

    class Grab(logging.Handler):
        def emit(self, rec):
            records.append(rec.getMessage())
    log = logging.getLogger(f"sat_{dtype}")
    log.addHandler(Grab())
    log.setLevel(logging.INFO)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    from riser_amd.fake_client import FakeClient
    client = FakeClient(scripted_batches(3, 64))
    import tempfile, os
    with tempfile.TemporaryDirectory() as d:
        ctl = SequencerControl(client, [m], proc, log, os.path.join(d, "out"))
        ctl.start()
        ctl.target("enrich", 0.01, 0.9)
        ctl.finish()
    assert ctl.saturated_batches >= 1 and any("overflowed half precision" in r for r in records)
    m.close()
    f32 = Model(base, synth.Config(), None, "m", dtype="f32w", device=dev)            # fp32 on the unscaled weights
    ref = f32.classify_raw(sig, off, ln, lh).cpu().numpy()
    f32.close()
    for dt in ("bf16x3", "f32w"):                                                      # fp32's exponent range: never reported, right result
        r = Model(sd, synth.Config(), None, "big", dtype=dt, device=dev)
        pr = r.classify_raw(sig, off, ln, lh).cpu().numpy()
        assert not r.saturated() and np.abs(pr - ref).max() < 1e-3
        r.close()


def test_activation_range_check(dev):
    """riser_amd.rangecheck: per-layer activation maxima of the fp32 path on sample reads - the evidence for choosing f16x3
    (half precision's range) or bf16x3.  On the calibrated weights every layer is far inside 65504; with layer 5 scaled by
    1e5 (the same function: layer 6 undoes it) layer 5's maximum is 1e5 times larger and the verdict says bf16x3."""
    from riser_amd import rangecheck
    base = synth.make_state_dict(1)
    sigs = [synth.make_signals(SIG_SEED, 1, 6000 + 100 * i, first_read=700 + i)[0] for i in range(8)]
    mx = rangecheck.activation_range(base, signals=sigs, device=dev)
    assert len(mx) == 11 and all(0 < v < 5000 for v in mx)
    assert "safe" in rangecheck.verdict(mx)
    sd = dict(base)
    sd["layers.5.0.weight"] = base["layers.5.0.weight"] * np.float32(1e5)
    sd["layers.5.0.bias"] = base["layers.5.0.bias"] * np.float32(1e5)
    sd["layers.6.0.weight"] = base["layers.6.0.weight"] / np.float32(1e5)
    big = rangecheck.activation_range(sd, signals=sigs, device=dev)
    assert abs(big[4] / mx[4] / 1e5 - 1) < 1e-3 and abs(big[5] / mx[5] - 1) < 1e-3      # list index = layer - 1
    assert "bf16x3" in rangecheck.verdict(big) and big[4] > 65504


def test_integration_md_ctypes_stub_runs(dev, tmp_path):
    """the ctypes stub INTEGRATION.md section 2 shows a RISER maintainer (Model.__init__ / classify and mad_normalise bound straight
    to the C ABI) is executed as written - only the library path is filled in - and gives the oracle's probabilities and the
    reference's float64 normalisation"""
    import re
    from riser_amd import _native as nv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    sec = text[text.index("## 2. Bind the C ABI directly"):]
    code = re.search(r"```python\n(.*?)```", sec, re.S).group(1)
    assert 'C.CDLL("libriser_amd.so")' in code
    code = code.replace('C.CDLL("libriser_amd.so")', f'C.CDLL({nv.LIB_PATH!r})')
    ns = {}
    torch.cuda.set_device(dev)
    exec(compile(code, "INTEGRATION.md#2", "exec"), ns)
    sd = synth.make_state_dict(1)
    path = str(tmp_path / "mRNA.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    m = ns["Model"](path, synth.Config(), None, "mRNA")
    for first, L in ((3, 6024), (4, 16000), (5, 4096)):
        sig = synth.make_signals(SIG_SEED, 1, L, first_read=first)[0]
        x = ns["mad_normalise"](sig)
        assert x.dtype == np.float64 and np.array_equal(x, ro.mad_normalise(sig))
        p = m.classify(x)
        assert np.abs(p.cpu().numpy() - ro.classify(sd, x)).max() < 1e-3
    with pytest.raises(ValueError):
        ns["mad_normalise"](np.zeros(0, dtype=np.int16))


def test_fc_classifier_other_shapes_against_oracle(dev):
    """the `fc` head is not tied to 67 x 753 -> 4096 here: small nets, 1 ... 7 positions, hidden 64 / 192, batches of 1 ... 37
    reads (one to three 16-read tiles, 16 to 5 K splits) against the oracle's Flatten -> Linear -> ReLU -> Linear"""
    from riser_amd.model import Model
    rng = np.random.default_rng(20260106)
    for channels, positions, hidden in (([4, 6, 8, 10], 3, 64), ([20, 30, 45], 7, 192), ([5, 9], 1, 64)):
        n = len(channels)
        sd, c_in = {}, 1
        for i, co in enumerate(channels):
            sd[f"layers.{i}.0.weight"] = (rng.standard_normal((co, c_in, 3)) * np.sqrt(2.0 / (3 * c_in))).astype(np.float32)
            sd[f"layers.{i}.0.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)
            c_in = co
        F = c_in * positions
        sd["classifier.1.weight"] = (rng.standard_normal((hidden, F)) * np.sqrt(2.0 / F)).astype(np.float32)
        sd["classifier.1.bias"] = (rng.standard_normal(hidden) * 0.1).astype(np.float32)
        sd["classifier.3.weight"] = (rng.standard_normal((2, hidden)) * np.sqrt(2.0 / hidden)).astype(np.float32)
        sd["classifier.3.bias"] = (rng.standard_normal(2) * 0.1).astype(np.float32)
        config = synth.Config(synth.CnnConfig(channels=channels, kernels=[3] * n, classifier="fc"))
        m = Model(sd, config, None, "x", device=dev)
        for B in (1, 16, 17, 37):
            lens = rng.integers(positions << n, (positions + 1) << n, size=B)
            xs = [rng.standard_normal(int(L)).astype(np.float32) for L in lens]
            want = np.stack([ro.softmax(ro.convnet_forward(sd, x[None, :]))[0] for x in xs])
            got = m.classify_batch(xs).cpu().numpy()
            assert np.abs(got - want).max() < 1e-4, (channels, B)
        with pytest.raises(RuntimeError):
            m.classify(rng.standard_normal((positions + 1) << n).astype(np.float32))
        m.close()


def test_convnet_variants_against_reference(dev, golden_dir):
    """ConvNet configurations outside the shipped class - depth 2 / 3, kernels 5 and 7 (riser/nets/cnn.py:17,52-65) -
    run the generic MFMA conv program (csrc/seqnet.hip) behind the same Model surface: classify(signal), batched
    mixed-length calls and the fused raw-read entry, against the reference's own probabilities; the scalar conv kernel
    (RS_SEQ_SCALAR=1) must agree with the MFMA one to fp32 round-off; unsupported classifiers are refused."""
    import json
    from conftest import hooked_model
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    g = np.load(os.path.join(golden_dir, "convnet_variants.npz"))
    for name in ("depth2_k5373", "depth1_k7", "depth3_k3"):
        cfg = json.loads(str(g[f"{name}.cfg"]))
        sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
        config = synth.Config(synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"]))
        m = Model(sd, config, None, "x", device=dev)
        lens, want = g[f"{name}.lens"], g[f"{name}.probs"]
        sigs = [synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0] for j, L in enumerate(lens)]
        xs = [ro.mad_normalise(s) for s in sigs]
        for j, x in enumerate(xs):
            one = m.classify(x)
            assert one.shape == (2,) and np.abs(one.cpu().numpy() - want[j]).max() < 1e-3, (name, j)
        got = m.classify_batch(xs + xs[::-1]).cpu().numpy()                  # mixed lengths: grouped by length inside
        assert np.abs(got[: len(xs)] - want).max() < 1e-3 and np.array_equal(got[len(xs):], got[: len(xs)][::-1])
        sig, off, ln, lh = pack_reads(sigs, dev)
        assert np.abs(m.classify_raw(sig, off, ln, lh).cpu().numpy() - want).max() < 1e-3
        with pytest.raises(ValueError):
            m.classify(np.zeros((1 << cfg["n_layers"]) - 1))
        os.environ["RS_SEQ_SCALAR"] = "1"
        try:
            ms = Model(sd, config, None, "x", device=dev)
        finally:
            del os.environ["RS_SEQ_SCALAR"]
        assert np.abs(ms.classify_batch(xs).cpu().numpy() - got[: len(xs)]).max() < 1e-5
        ms.close()
        m.close()
    with pytest.raises(ValueError):                                           # even kernels: 'same' pads asymmetrically
        Model({}, synth.Config(synth.CnnConfig(channels=[4, 4], kernels=[4, 3])), None, "x", device=dev)


def test_promethion_per_gpu_shape(dev):
    """BASELINE config 4, the per-GPU share: 18 000 x 16000-sample chunks resident in HBM, walked in sub-batches
    (riser_amd.stream.classify_resident): (a) the population repeats 512 distinct signals, so read i must give exactly
    the bits of read i mod 512 wherever it sits in whichever sub-batch - and those 512 are ALL checked against the
    oracle; (b) bit identity with direct library calls on arbitrary sub-ranges."""
    from conftest import oracle_bench_batch
    from riser_amd.model import Model
    from riser_amd.stream import classify_resident
    sd = synth.make_state_dict(1)
    m = Model(sd, synth.Config(), None, "m", device=dev)
    N, L, SUB = 18000, 16000, 1024
    base = synth.make_signals(SIG_SEED, 512, L)
    idx = np.arange(N)
    sig = torch.from_numpy(np.ascontiguousarray(base[idx % 512].reshape(-1))).to(dev)
    probs = classify_resident([m], sig, N, L, None, SUB).cpu().numpy()
    # two sub-batches in flight on two HIP streams (per-stream workspaces): the same bits
    assert np.array_equal(probs, classify_resident([m], sig, N, L, None, SUB, streams=2).cpu().numpy())
    assert probs.shape == (1, N, 2) and np.isfinite(probs).all()
    p = probs[0]
    assert np.array_equal(p, p[idx % 512]), "a read's result depends on its position in the population"
    oracle = oracle_bench_batch(1, "full")
    assert np.abs(p[:512] - oracle).max() < 1e-4
    assert np.array_equal(p[:512, 1] > 0.9, oracle[:, 1] > 0.9)
    lo, hi = 5000, 5100                                                # straddles no sub-batch boundary ...
    off = torch.arange(lo, hi, dtype=torch.int64, device=dev) * L
    ln = torch.full((hi - lo,), L, dtype=torch.int32, device=dev)
    assert np.array_equal(m.classify_raw(sig, off, ln, np.full(hi - lo, L, np.int32)).cpu().numpy(), p[lo:hi])
    lo, hi = 17 * SUB - 40, 17 * SUB + 23                               # ... and one that does, ending at the ragged tail
    off = torch.arange(lo, hi, dtype=torch.int64, device=dev) * L
    ln = torch.full((hi - lo,), L, dtype=torch.int32, device=dev)
    assert np.array_equal(m.classify_raw(sig, off, ln, np.full(hi - lo, L, np.int32)).cpu().numpy(), p[lo:hi])
    m.close()


def test_classify_population_shards_by_read_id(dev):
    """riser_amd.dist.classify_population: each rank loads and classifies only the reads whose id hashes to it; the
    shards of a (simulated) 8-rank world partition the population and reproduce the single-rank result bit for bit."""
    from riser_amd import dist as rdist
    from riser_amd.model import Model
    m = Model(synth.make_state_dict(2), synth.Config(), None, "m", dtype="f16", device=dev)
    N, L = 700, 8000
    ids = [f"read-{i:05d}" for i in range(N)]
    base = synth.make_signals(SIG_SEED, 64, L, first_read=40)
    lens_all = np.where(np.arange(N) % 3 == 0, 6000, L).astype(np.int32)
    loads = []

    def load(ix):
        loads.append(np.asarray(ix))
        return base[np.asarray(ix) % 64], lens_all[ix]

    mine, probs, full = rdist.classify_population([m], ids, load, rank=0, world=1, sub_batch=256)
    assert mine.tolist() == list(range(N)) and np.array_equal(full[0], probs[0])
    seen = np.zeros(N, dtype=int)
    for r in range(8):
        ix, pr, _ = rdist.classify_population([m], ids, load, rank=r, world=8, sub_batch=64, gather=False)
        assert all(rdist.shard_of(ids[i], 8) == r for i in ix)
        assert np.array_equal(loads[-1], ix), "a rank must load only its own reads"
        seen[ix] += 1
        assert np.array_equal(pr[0], full[0][ix])
    assert (seen == 1).all()
    m.close()


@pytest.mark.parametrize("channels", [(12, 24, 33, 40, 50), (20, 30, 16, 70), (20, 32, 32, 96, 130, 200), (8, 17, 48)])
def test_other_channel_widths_all_modes(dev, channels):
    """ConvNets of the shipped class (depth 1, kernel 3, gap_fc) with OTHER channel widths: every width class of the
    streaming kernels (layer 1 with 17..32 channels, layer 2 with one, two or three 16-channel tiles, layer 0 below 20
    channels), the tiled kernels on odd widths, 3- to 6-layer nets; fp32, plain 16-bit and split precision against the
    oracle on a mixed-length batch (bf16 inside its own envelope, test_gpu_parity.H16_TOL; f16xf8 as planned and with every
    layer from 64 input channels on in the 8-bit form), and the one-launch streaming form against the two-launch one bit for bit."""
    from riser_amd.preprocess import pack_reads
    from conftest import hooked_model
    from test_gpu_parity import H16_TOL
    cfg = synth.Config(synth.CnnConfig(channels=list(channels), kernels=[3] * len(channels)))
    sd = synth.make_state_dict(7, channels=channels)
    lens = [4096, 8000, 5000, 8191, 4097, 6024, 7777]
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=700 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    want = ro.classify_reads(sd, sigs)
    for dtype, tol, env in (("f32w", 1e-4, {}), ("f32", 1e-4, {}), ("f16x3", 1e-3, {}), ("bf16x3", 1e-3, {}), ("f16", 3e-2, {}),
                            ("bf16", H16_TOL["bf16"], {}), ("f16xf8", 1e-3, {}), ("f16xf8", 1e-3, {"RS_F8_MIN_CIN": "64"})):
        m = hooked_model(env, sd, dtype, dev, config=cfg)
        got = m.classify_raw(sig, off, ln, lh).cpu().numpy()
        assert np.abs(got - want).max() < tol, (dtype, env, channels, np.abs(got - want).max())
        if dtype in ("f16x3", "bf16x3", "f16", "f16xf8"):
            m2 = hooked_model(dict(env, RS_NO_STREAM012="1"), sd, dtype, dev, config=cfg)
            assert np.array_equal(got, m2.classify_raw(sig, off, ln, lh).cpu().numpy()), (dtype, env, channels)
            m2.close()
        # batch composition: a sub-batch reproduces its rows bit for bit
        idx = torch.tensor([5, 0, 3], device=dev)
        part = m.classify_raw(sig, off[idx].contiguous(), ln[idx].contiguous(), lh[[5, 0, 3]]).cpu().numpy()
        assert np.array_equal(part, got[[5, 0, 3]]), (dtype, channels)
        m.close()


def test_control_loop_signal_store_and_scale(dev, tmp_path):
    """the device-resident signal store (a re-seen read uploads only its new samples) changes nothing but the PCIe
    bytes: the replay of AccumulatingCache traffic writes the same CSV, sends the same reject / finish lists with and
    without it; a depth-2 ConvNet (generic conv program) runs through the same loop; and an 18 000-channel batch
    (PromethION scale) goes through SequencerControl."""
    from riser_amd import Kit, Model, SequencerControl, SignalProcessor
    from riser_amd.replay import scripted_batches
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    models = [Model(synth.make_state_dict(s), synth.Config(), None, f"t{s}", device=dev) for s in (1, 2)]
    batches = scripted_batches(7, 96)
    # a read longer than a row of the store, a channel number beyond the first map, an id that changes mid-way
    long_read = FakeRead("long", synth.make_raw_read(5, 5, 40000, True))
    batches[2].append((3000, long_read))
    batches[3].append((3000, long_read))
    outs = []
    for k, cache in enumerate((True, False)):
        client = FakeClient(batches)
        ctl = SequencerControl(client, models, proc, logging.getLogger("c"), str(tmp_path / f"s{k}"), signal_cache=cache)
        ctl.reserve(128)
        ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
        rows = [ln.split(",", 1)[1] for ln in open(str(tmp_path / f"s{k}.csv")).read().strip().split("\n")[1:]]
        outs.append((rows, client.rejected, client.finished, ctl._store.samples_uploaded, ctl._store.samples_presented))
    assert outs[0][:3] == outs[1][:3] and len(outs[0][0]) > 200
    assert outs[1][3] == outs[1][4] and outs[0][3] < 0.45 * outs[0][4]          # most samples never cross PCIe twice
    # against the oracle's per-read loop (riser/control.py:31-97 restated): rows and lists
    cpu_models = {s: torch_path.TorchCpuModel(synth.make_state_dict(s)) for s in (1, 2)}
    want_rows, want_rej, want_fin = _oracle_loop(batches[:3], "RNA004", (1, 2), "enrich", 0.9, cpu_models)
    got = [r.split(",") for r in outs[0][0][: len(want_rows)]]
    for g, w in zip(got, want_rows):
        assert (g[0], int(g[1]), int(g[2])) == w[:3]
        assert np.allclose([float(v) for v in g[4].split(";")], w[4], atol=1e-3)
    for m in models:
        m.close()
    # a generic conv program (depth 2) in the loop: classify_raw_ensemble falls back to one call per model + rs_decide
    import json
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnet_variants.npz"))
    vcfg = json.loads(str(g["depth2_k5373.cfg"]))
    vsd = {k[len("depth2_k5373") + 4:]: g[k] for k in g.files if k.startswith("depth2_k5373.sd.")}
    cfg = synth.Config(synth.CnnConfig(channels=vcfg["channels"], kernels=vcfg["kernels"], depth=vcfg["depth"]))
    deep = Model(vsd, cfg, None, "deep", device=dev)
    with pytest.raises(ValueError):
        Model(vsd, cfg, None, "deep", dtype="f16", device=dev)            # the generic program is fp32 only
    with pytest.raises(NotImplementedError):
        deep.layer_info()
    client = FakeClient(batches[:2])
    ctl = SequencerControl(client, [deep], proc, logging.getLogger("c"), str(tmp_path / "deep"))
    ctl.start(); ctl.target("deplete", 0.5, 0.9); ctl.finish()
    assert open(str(tmp_path / "deep.csv")).read().count("\n") > 40
    deep.close()
    # PromethION scale: 18 000 channels in one ReadUntil batch
    m = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", device=dev)
    big = scripted_batches(2, 18000)
    client = FakeClient(big)
    ctl = SequencerControl(client, [m], proc, logging.getLogger("c"), str(tmp_path / "big"))
    ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
    n_rows = open(str(tmp_path / "big.csv")).read().count("\n") - 1
    assert n_rows > 10000 and len(client.finished) == 2
    m.close()


def test_f16xf8_cross_terms_on_the_8bit_mfma(dev, golden_dir):
    """RS_F16XF8 (csrc/conv_ring_f8.hip): split precision whose wide layers keep hi*hi on the f16 MFMA and evaluate the cross
    terms hi*lo + lo*hi as ONE block-scaled e4m3 product (v_mfma_scale_f32_16x16x128_f8f6f4; rows between those layers carry
    an E8M0 scale per row and 32 channels).  By default layers 7-11 of the shipped net; RS_F8_MIN_CIN=64 puts EVERY layer from
    4 on into that form (the run then crosses the fine -> coarse re-pack, whose scale plane moves with the rows).  Both against
    the reference's golden probabilities and the oracle within the 1e-3 tolerance, labels identical; and the properties that
    do not depend on size: a read's bits are those of the read alone, whatever the batch, its order, the layout (host lengths
    or not, one level or two), and thin launches (one read) agree with the batched row."""
    import os
    from conftest import hooked_model
    from riser_amd.preprocess import pack_reads
    net = np.load(os.path.join(golden_dir, "network.npz"))
    for env in ({}, {"RS_F8_MIN_CIN": "64"}):
        models, worst = {}, 0.0
        for seed, L, B, first in net["cases"]:
            tag = f"s{seed}_L{L}_B{B}_r{first}"
            seed = int(seed)
            if seed not in models:
                models[seed] = hooked_model(env, synth.make_state_dict(seed), "f16xf8", dev)
            sigs = synth.make_signals(int(net["sig_seed"][0]), int(B), int(L), first_read=int(first))
            sig, off, ln, lh = pack_reads(list(sigs), dev)
            got = models[seed].classify_raw(sig, off, ln, lh).cpu().numpy()
            want = net[f"{tag}.probs"]
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert np.isfinite(got).all() and err < 1e-3, (env, tag, err)
            assert np.array_equal(got[:, 1] > 0.9, want[:, 1] > 0.9), (env, tag)
        print(f"f16xf8 {env}: worst |dp| {worst:.2e} over the golden cases")
        assert worst < 5e-4, (env, worst)
        for m in models.values():
            m.close()
    # layout and batch invariance with every wide layer in the 8-bit form: lengths at the block edges of both levels
    sd = synth.make_state_dict(2)
    m = hooked_model({"RS_F8_MIN_CIN": "64"}, sd, "f16xf8", dev)
    one = hooked_model({"RS_F8_MIN_CIN": "64", "RS_ONE_LEVEL": "1"}, sd, "f16xf8", dev)
    info = m.layer_info()
    assert info[5]["cp_out"] == 128 * ((info[5]["c_out"] + 63) // 64) and info[11]["cp_out"] == 64 * ((info[11]["c_out"] + 31) // 32)
    lens = np.array([8615, 4096, 4097, 5119, 5120, 5121, 8191, 8192, 8193, 9215, 9216, 12287, 12288, 16000, 6024, 7168, 10240,
                     16383, 4607, 20000], dtype=np.int32)
    sigs = [synth.make_signals(SIG_SEED, 1, int(n), first_read=6100 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    got = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    want = ro.classify_reads(sd, sigs)
    assert np.abs(got - want).max() < 1e-3, float(np.abs(got - want).max())
    assert np.array_equal(got[:, 1] > 0.9, want[:, 1] > 0.9)
    assert np.array_equal(got, m.classify_raw(sig, off, ln, lh, packed=False).cpu().numpy())
    assert np.array_equal(got, one.classify_raw(sig, off, ln, lh).cpu().numpy())
    for idx in ([3], list(range(len(lens)))[::-1], [14, 0, 19, 7]):
        s2, o2, l2, h2 = pack_reads([sigs[i] for i in idx], dev)
        assert np.array_equal(m.classify_raw(s2, o2, l2, h2).cpu().numpy(), got[idx]), idx
    m.close()
    one.close()


@pytest.mark.parametrize("dtype", ["bf16x3", "f16x3"])
def test_merged_tail_panel_of_split_precision(dev, dtype):
    """round 6: a split-precision layer whose input ends in a panel of 1-8 channels behind 2-4 full ones runs that panel's three
    taps as ONE K step (conv_ring_h16.hip: TAIL; conv_thin_h16.hip).  A net whose layers sit on both sides of every
    eligibility bound - inputs of 65 (3 panels, 1 channel in the last), 72 (8), 104 (4 panels), 136 (5 panels), 73 (9: not
    merged), 40 (2 panels: not merged) - against the oracle; the thin-launch kernel, the ring kernel and every forced ring shape
    give the same bits; RS_X3_TAIL=0 (the un-merged order) stays within round-off of it; a sub-batch reproduces its rows."""
    from riser_amd.preprocess import pack_reads
    from conftest import hooked_model
    channels = (20, 30, 65, 72, 104, 136, 73, 40, 48)
    cfg = synth.Config(synth.CnnConfig(channels=list(channels), kernels=[3] * len(channels)))
    sd = synth.make_state_dict(11, channels=channels)
    rng = np.random.default_rng(5)
    lens = [int(n) for n in rng.integers(4096, 16001, size=37)] + [16000] * 3
    sigs = [synth.make_signals(SIG_SEED, 1, n, first_read=5200 + i)[0] for i, n in enumerate(lens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    want = ro.classify_reads(sd, sigs[:10])
    ring = hooked_model({"RS_THIN_H16_ROWS": "0"}, sd, dtype, dev, config=cfg)
    got = ring.classify_raw(sig, off, ln, lh, return_logits=True)
    assert np.abs(got[0][:10].cpu().numpy() - want).max() < 1e-3
    info = ring.layer_info()
    assert [info[i]["k_pad"] for i in (3, 4, 5, 6, 7, 8)] == [7 * 32, 7 * 32, 10 * 32, 13 * 32, 9 * 32, 6 * 32]   # merged: 3 (panels - 1) + 1 K steps
    for env in ({"RS_THIN_H16_ROWS": "100000000"}, {}, {"RS_THIN_H16_ROWS": "0", "RS_FORCE_SHAPE_RING": ";".join("%d:4,2,2,4" % i for i in range(3, 9))},
                {"RS_THIN_H16_ROWS": "0", "RS_FORCE_SHAPE_RING": ";".join("%d:8,1,2,7" % i for i in range(3, 9))}):
        m = hooked_model(env, sd, dtype, dev, config=cfg)
        g2 = m.classify_raw(sig, off, ln, lh, return_logits=True)
        assert torch.equal(g2[0], got[0]) and torch.equal(g2[1], got[1]), (dtype, env)
        m.close()
    plain = hooked_model({"RS_X3_TAIL": "0"}, sd, dtype, dev, config=cfg)
    assert [plain.layer_info()[i]["k_pad"] for i in (3, 4, 5, 6)] == [9 * 32, 9 * 32, 12 * 32, 15 * 32]
    p2 = plain.classify_raw(sig, off, ln, lh)
    assert 0 < float((p2 - got[0]).abs().max()) < 5e-4            # another summation order, the same arithmetic
    plain.close()
    idx = torch.tensor([7, 0, 39], device=dev)
    part = ring.classify_raw(sig, off[idx].contiguous(), ln[idx].contiguous(), lh[[7, 0, 39]])
    assert torch.equal(part, got[0][idx])
    ring.close()
