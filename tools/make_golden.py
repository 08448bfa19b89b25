#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ by running the REFERENCE itself.

Runs only in the build container (it imports /root/reference, which does not exist on
the GPU box and must never be copied).  The committed outputs are data: inputs (or the
integer seeds that rebuild them through riser_amd.synth) and the values the reference's
own code returned for them.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden.py

Reference entry points exercised:
  F1  SignalProcessor.mad_normalise          riser/preprocess.py:108-147  (F1b: float32 / float64 inputs)
  F2  Model.classify / ConvNet.forward        riser/model.py:22-28, riser/nets/cnn.py:43-65  (F2b: depth > 1 / odd kernels; F2c: `gap` head; F2d: `fc` head; F2e: edge configs of the generic family)
  F3  SequencerControl.target                 riser/control.py:11-124 (fake client)
  F4  SignalProcessor.get_polyA_end           riser/preprocess.py:42-79
  F5  ResNet.forward                          riser/nets/resnet.py  (F5b: edge configs of the launch-form sweep)
  F6  TCN.forward / TCNBot.forward            riser/nets/tcn.py, riser/nets/tcn_bot.py  (F6b: edge configs)
  F7  ConvRecNet.forward                      riser/nets/cnn_rnn.py  (F7b: edge configs of the shape sweep)
"""
import json
import logging
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# riser/nets/cnn.py:2 imports torchinfo (unused, not installed): stub it.
sys.modules.setdefault("torchinfo", types.SimpleNamespace(summary=None))
sys.path.insert(0, "/root/reference/riser")

import numpy as np          # noqa: E402
import torch                # noqa: E402

from model import Model                              # noqa: E402  (reference)
from preprocess import Kit, SignalProcessor          # noqa: E402  (reference)
from control import SequencerControl                 # noqa: E402  (reference)

from riser_amd import synth                          # noqa: E402
from riser_amd.fake_client import FakeClient, FakeRead   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIG_SEED = 20260103
LOG = logging.getLogger("golden")
LOG.addHandler(logging.NullHandler())


def ref_model(seed, target="mRNA"):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed).items()}
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(sd, f.name)
        path = f.name
    try:
        return Model(path, synth.Config(), LOG, target)
    finally:
        os.unlink(path)


# --------------------------------------------------------------------------------------
def f1_normalise():
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    cases = {}
    for L in (4096, 4097, 6024, 8615, 12048, 16000):
        cases[f"synth_{L}"] = synth.make_signals(SIG_SEED, 1, L, first_read=L % 97)[0]
    cases["synth_runs_16000"] = synth.make_signals(SIG_SEED, 1, 16000, first_read=16)[0]   # rid%16==0: forced runs
    base = synth.make_signals(SIG_SEED, 1, 5000, first_read=3, spikes=False)[0]

    def with_spikes(pos_val, src=base):
        s = src.copy()
        for p, v in pos_val:
            s[p] = v
        return s

    cases["out_first"] = with_spikes([(0, 2500)])
    cases["out_first_two"] = with_spikes([(0, 2500), (1, 2400)])
    cases["out_first_three_neg"] = with_spikes([(0, 0), (1, 5), (2, 2)])
    cases["out_last"] = with_spikes([(4999, 2500)])
    cases["out_last_two"] = with_spikes([(4998, 30), (4999, 2500)])
    cases["run3"] = with_spikes([(100, 1900), (101, 2000), (102, 1800)])
    cases["run4_mixed_sign"] = with_spikes([(200, 1900), (201, 10), (202, 1800), (203, 5)])
    cases["run5_then_gap_run2"] = with_spikes([(300 + k, 1500 + 37 * k) for k in range(5)] + [(306, 1700), (307, 20)])
    cases["long_run_64"] = with_spikes([(1000 + k, 1200 + (k * 53) % 700) for k in range(64)])
    cases["alternating"] = with_spikes([(2000 + 2 * k, 2000) for k in range(40)])
    cases["mad0_constant"] = np.full(4096, 512, dtype=np.int16)
    m = synth.make_signals(SIG_SEED, 1, 4100, first_read=5)[0]
    m[:2500] = 500
    cases["mad0_majority"] = m
    cases["even_half_median"] = np.array([1, 2, 3, 4, 5, 6, 7, 8, 100, -50] * 410, dtype=np.int16)
    cases["odd_len"] = np.array([3, -2, 7, 7, 1, 0, 9, 11, -30000, 30000, 4] * 373, dtype=np.int16)
    cases["negative_adc"] = (synth.make_signals(SIG_SEED, 1, 4500, first_read=9)[0].astype(np.int32) - 2600).astype(np.int16)
    cases["two_level"] = np.array(([100] * 7 + [900] * 6) * 400, dtype=np.int16)
    cases["tiny_len5"] = np.array([5, 1, 9, 3, 400], dtype=np.int16)
    cases["tiny_len2"] = np.array([5, 9], dtype=np.int16)

    out = {}
    names = []
    for name, sig in cases.items():
        y = proc.mad_normalise(sig.copy())
        med = np.median(sig)
        mad = np.median(np.abs(sig - med))
        names.append(name)
        out[f"{name}.sig"] = sig
        out[f"{name}.out"] = np.asarray(y)
        out[f"{name}.stats"] = np.array([med, mad], dtype=np.float64)
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "normalise.npz"), **out)
    print("F1:", len(names), "cases")


def f1b_normalise_float():
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    res, names = {}, []
    for name, x in synth.normalise_float_cases():
        y = np.asarray(proc.mad_normalise(x.copy()))
        names.append(name)
        res[f"{name}.out"] = y
    res["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "normalise_float.npz"), **res)
    print("F1b:", len(names), "float cases;", {n: str(res[f"{n}.out"].dtype) for n in names[:4]})


# --------------------------------------------------------------------------------------
def f2_network():
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    out = {}
    cases = []
    plan = [(1, L, 3, 100 + i) for i, L in enumerate((4096, 4097, 5000, 6024, 8000, 8615, 12000, 12048, 16000))]
    plan += [(2, 6024, 64, 0)]                       # BASELINE config 1 (RNA002 2 s, 64 chunks)
    plan += [(s, 16000, 8, 0) for s in (1, 2, 3)]    # ensemble stand-ins, RNA004 4 s
    plan += [(1, 16000, 32, 1000)]
    for seed, L, B, first in plan:
        tag = f"s{seed}_L{L}_B{B}_r{first}"
        m = ref_model(seed)
        sigs = synth.make_signals(SIG_SEED, B, L, first_read=first)
        probs = np.zeros((B, 2), np.float32)
        logits = np.zeros((B, 2), np.float32)
        for b in range(B):
            x = proc.mad_normalise(sigs[b].copy())
            probs[b] = m.classify(x).numpy()
            with torch.no_grad():
                logits[b] = m.model(torch.from_numpy(x).unsqueeze(0).float())[0].numpy()
        # per-layer statistics of read 0 for bisecting
        with torch.no_grad():
            h = torch.from_numpy(proc.mad_normalise(sigs[0].copy())).float()[None, None, :]
            stats = []
            for layer in m.model.layers:
                h = layer(h)
                flat = h.flatten().double()
                stats.append([float(flat.sum()), float(flat.abs().sum()), float(h[0, 0, 0]), float(h[0, -1, -1]),
                              float(h.shape[1]), float(h.shape[2])])
        out[f"{tag}.probs"] = probs
        out[f"{tag}.logits"] = logits
        out[f"{tag}.layer_stats"] = np.array(stats, dtype=np.float64)
        out[f"{tag}.sig_crc"] = np.array([int(sigs.astype(np.int64).sum()), int((sigs.astype(np.int64) ** 2).sum())], dtype=np.int64)
        cases.append([seed, L, B, first])
        print("F2:", tag, "p_on", np.round(probs[:4, 1], 4))
    out["cases"] = np.array(cases, dtype=np.int64)
    out["sig_seed"] = np.array([SIG_SEED], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "network.npz"), **out)


# --------------------------------------------------------------------------------------
def control_script():
    """(channel, read_id, rid, total_len, polya, number) per batch; RNA004 kit:
    max 8615, fixed trim 4633, fixed-trim trigger > 13248 (riser/preprocess.py:36-37,81-85)."""
    b0 = [
        (1, "r-polya-short", 0, 7000, True, None),       # trimmed but < 4096 left -> skipped (or not found)
        (2, "r-polya-mid", 1, 12000, True, None),        # trimmed, 4096 <= len < max
        (3, "r-polya-long", 2, 20000, True, 17),         # trimmed, > max -> cut to 8615
        (4, "r-nopolya-short", 3, 9000, False, None),    # not found, too short for fixed trim -> skipped
        (5, "r-nopolya-long", 4, 14000, False, None),    # not found, fixed trim + cut to max
        (6, "r-polya-mid2", 5, 11000, True, 23),
        (7, "r-polya-mid3", 6, 12500, True, None),
        (8, "r-nopolya-long2", 7, 15000, False, 99),
    ]
    b1 = [
        (1, "r-polya-short", 0, 11500, True, None),      # same read, more signal: cache hit, now assessable
        (2, "r-polya-mid", 1, 14000, True, None),
        (9, "r-polya-new", 8, 13000, True, None),
        (4, "r-nopolya-short", 3, 13249, False, None),   # just over the fixed-trim trigger
        (10, "r-edge-13248", 9, 13248, False, None),     # exactly at the trigger: not trimmed (strict >)
    ]
    b2 = [(11 + k, f"r-bulk-{k}", 20 + k, 10000 + 411 * k, k % 3 != 0, None) for k in range(12)]
    return [b0, b1, b2]


def build_batches(script, seed=77):
    batches = []
    for b in script:
        reads = []
        for ch, rid_s, rid, n, polya, number in b:
            reads.append((ch, FakeRead(rid_s, synth.make_raw_read(seed, rid, n, polya), number)))
        batches.append(reads)
    return batches


def f3_control():
    script = control_script()
    results = {"script": script, "raw_seed": 77, "kit": "RNA004", "runs": []}
    for mode in ("enrich", "deplete"):
        for seeds, thr in (((1,), 0.9), ((1,), 0.6), ((1,), 0.999), ((2,), 0.9), ((1, 2, 3), 0.9),
                           ((2, 3), 0.9), ((2, 3), 0.6)):
            if True:
                models = [ref_model(s, t) for s, t in zip(seeds, ("mRNA", "mtRNA", "globin"))]
                proc = SignalProcessor(Kit.create_from_version("RNA004"))
                client = FakeClient(build_batches(script))
                with tempfile.TemporaryDirectory() as d:
                    ctl = SequencerControl(client, models, proc, LOG, os.path.join(d, "out"))
                    ctl.start()
                    ctl.target(mode, 1.0, thr)
                    ctl.finish()
                    with open(os.path.join(d, "out.csv")) as f:
                        lines = f.read().strip().split("\n")
                rows = []
                for ln in lines[1:]:
                    p = ln.split(",")
                    rows.append({"read_id": p[1], "channel": int(p[2]), "sig_length": int(p[3]), "models": p[4],
                                 "prob_targets": [float(v) for v in p[5].split(";")], "threshold": float(p[6]),
                                 "mode": p[7], "decision": p[8]})
                results["runs"].append({"mode": mode, "seeds": list(seeds), "threshold": thr, "header": lines[0],
                                        "rows": rows, "rejected": client.rejected, "finished": client.finished,
                                        "warnings": client.warnings, "unblock": client.unblock_durations})
                print("F3:", mode, seeds, thr, [r["decision"] for r in rows])
    with open(os.path.join(OUT, "control.json"), "w") as f:
        json.dump(results, f, indent=1)


# --------------------------------------------------------------------------------------
def f2b_convnet_variants():
    """ConvNet configurations outside the shipped class (riser/nets/cnn.py:17,52-65): depth 2 and mixed odd kernels,
    through the reference's own Model.classify (one read at a time)."""
    rng = np.random.default_rng(20260104)
    cfgs = {"depth2_k5373": dict(n_layers=4, depth=2, channels=[6, 9, 14, 20], kernels=[5, 3, 7, 3]),
            "depth1_k7": dict(n_layers=5, depth=1, channels=[8, 12, 18, 27, 40], kernels=[7, 7, 7, 7, 7]),
            "depth3_k3": dict(n_layers=3, depth=3, channels=[5, 10, 15], kernels=[3, 3, 3])}
    out = {}
    for name, c in cfgs.items():
        cnn = synth.CnnConfig(channels=c["channels"], kernels=c["kernels"], depth=c["depth"])
        sd, c_in = {}, 1
        for i, co in enumerate(c["channels"]):
            ci = c_in
            for d in range(c["depth"]):
                k = c["kernels"][i]
                sd[f"layers.{i}.{2 * d}.weight"] = (rng.standard_normal((co, ci, k)) * np.sqrt(2.0 / (k * ci))).astype(np.float32)
                sd[f"layers.{i}.{2 * d}.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)
                ci = co
            c_in = co
        sd["classifier.2.weight"] = rng.standard_normal((2, c_in)).astype(np.float32)
        sd["classifier.2.bias"] = rng.standard_normal(2).astype(np.float32)
        with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
            torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, f.name)
            path = f.name
        try:
            m = Model(path, synth.Config(cnn), LOG, "x")
        finally:
            os.unlink(path)
        proc = SignalProcessor(Kit.create_from_version("RNA004"))
        lens = [1 << c["n_layers"], (1 << c["n_layers"]) + 1, 1000, 2049, 4096]
        probs = []
        for j, L in enumerate(lens):
            sig = synth.make_signals(SIG_SEED, 1, L, first_read=60 + j)[0]
            probs.append(m.classify(proc.mad_normalise(sig.copy())).numpy())
        out[f"{name}.cfg"] = np.array(json.dumps(c))
        out[f"{name}.lens"] = np.array(lens)
        out[f"{name}.probs"] = np.stack(probs)
        for k, v in sd.items():
            out[f"{name}.sd.{k}"] = v
        print("F2b:", name, np.stack(probs)[:, 1])
    np.savez_compressed(os.path.join(OUT, "convnet_variants.npz"), **out)


# --------------------------------------------------------------------------------------
def f2e_gconv_edges():
    """F2b at the edges of the generic family's shape arithmetic, on six configs of tests/gconv_ref.py (taken from there
    with their seeds, so the two cannot drift apart): kernels 1, 9 and 19, a 5-3-7-3 mix, depth 1 - 3, 17 / 33 / 65
    channels.  Logits of three synth reads per length from the reference's own ConvNet on the CPU; prints the largest gap
    to the float64 forward of tests/gconv_ref.py."""
    from nets.cnn import ConvNet
    from riser_amd import gconv as G
    from tests import gconv_ref as R
    out, worst = {}, 0.0
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    for name in R.GOLDEN_EDGES:
        cfg, seed = R.CONFIGS[name], R.SEED[name]
        cnn = R.cnn_config(cfg)
        net = ConvNet(cnn)
        sd = R.make_state_dict(cfg, seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net.eval()
        prog = G.build_gconv_program(sd, cnn)
        lo = G.min_length(prog)
        lens = [lo if L == "min" else lo + 1 if L == "min+1" else int(L) for L in R.GOLDEN_LENGTHS]
        for L in lens:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x)).numpy()
            out[f"{name}.L{L}.logits"] = logits
            worst = max(worst, R.gap(logits, R.forward(prog, x, [L] * 3)))
        out[f"{name}.cfg"] = np.array(json.dumps(dict(cfg, lengths=lens, seed=seed)))
        print("F2e:", name, "min", lo, "float64 gap so far %.2e" % worst)
    np.savez_compressed(os.path.join(OUT, "gconv_edges.npz"), **out)


# --------------------------------------------------------------------------------------
def f2c_gap_head():
    """The `gap` classifier (riser/nets/cnn.py:34-38: Conv1d(C, n_classes, 1) then AdaptiveAvgPool1d(1)) through the
    reference's ConvNet.forward on batches of 3 equal-length reads, softmax(dim=1) as riser/model.py:27 applies it.  The
    reference's own Model.classify cannot run this head: at batch 1 x.squeeze() (cnn.py:48-49) drops the batch dimension
    and softmax(dim=1) raises - recorded as `classify_error`."""
    rng = np.random.default_rng(20260105)
    out = {}
    cfgs = {"shipped_gap": dict(channels=list(synth.CHANNELS), kernels=list(synth.KERNELS), depth=1),
            "depth2_gap": dict(channels=[6, 9, 14, 20], kernels=[5, 3, 7, 3], depth=2)}
    for name, c in cfgs.items():
        cnn = synth.CnnConfig(channels=c["channels"], kernels=c["kernels"], depth=c["depth"], classifier="gap")
        if c["depth"] == 1:
            # the shipped architecture with the calibrated synthetic weights of seed 1 (riser_amd.synth: rebuilt from the
            # seed, not stored); its Linear head re-read as the 1 x 1 convolution of the `gap` classifier
            sd = dict(synth.make_state_dict(1))
            sd["classifier.0.weight"] = sd.pop("classifier.2.weight")[:, :, None].copy()
            sd["classifier.0.bias"] = sd.pop("classifier.2.bias")
            stored = {}
        else:
            sd, c_in = {}, 1
            for i, co in enumerate(c["channels"]):
                ci = c_in
                for d in range(c["depth"]):
                    k = c["kernels"][i]
                    sd[f"layers.{i}.{2 * d}.weight"] = (rng.standard_normal((co, ci, k)) * np.sqrt(2.0 / (k * ci))).astype(np.float32)
                    sd[f"layers.{i}.{2 * d}.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)
                    ci = co
                c_in = co
            sd["classifier.0.weight"] = rng.standard_normal((2, c_in, 1)).astype(np.float32)
            sd["classifier.0.bias"] = rng.standard_normal(2).astype(np.float32)
            stored = sd
        with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
            torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, f.name)
            path = f.name
        try:
            m = Model(path, synth.Config(cnn), LOG, "x")
        finally:
            os.unlink(path)
        proc = SignalProcessor(Kit.create_from_version("RNA004"))
        lens = [4096, 6024] if c["depth"] == 1 else [16, 1000, 2049]
        for j, L in enumerate(lens):
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=90 + 3 * j)
            X = torch.from_numpy(np.stack([proc.mad_normalise(x.copy()) for x in sigs])).to(dtype=torch.float)
            with torch.no_grad():
                out[f"{name}.L{L}.probs"] = torch.nn.functional.softmax(m.model(X), dim=1).numpy()
        try:
            m.classify(proc.mad_normalise(synth.make_signals(SIG_SEED, 1, lens[0], first_read=90)[0].copy()))
            err = ""
        except Exception as e:                                    # noqa: BLE001 - the type is the datum
            err = type(e).__name__
        out[f"{name}.classify_error"] = np.array(err)
        out[f"{name}.cfg"] = np.array(json.dumps(dict(c, lens=lens)))
        for k, v in stored.items():
            out[f"{name}.sd.{k}"] = v
        print("F2c:", name, err, out[f"{name}.L{lens[0]}.probs"][:, 1])
    np.savez_compressed(os.path.join(OUT, "gap_head.npz"), **out)


# --------------------------------------------------------------------------------------
def f2d_fc_head():
    """The `fc` classifier (riser/nets/cnn.py:22-27: Flatten -> Linear(67 * 753, 4096) -> ReLU -> Linear(4096, 2)) on the
    4-layer net it is hard-coded for, through the reference's Model.classify: reads of 12048 .. 12063 samples (753
    positions after four pools); any other length fails in the first Linear - the error type is recorded.  Weights:
    riser_amd.synth.make_fc_state_dict(1), rebuilt from the seed (826 MB, never stored)."""
    sd = synth.make_fc_state_dict(1)
    cnn = synth.CnnConfig(channels=list(synth.FC_CHANNELS), kernels=[3] * len(synth.FC_CHANNELS), classifier="fc")
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, f.name)
        path = f.name
    try:
        m = Model(path, synth.Config(cnn), LOG, "x")
    finally:
        os.unlink(path)
    proc = SignalProcessor(Kit.create_from_version("RNA002"))
    lens = [12048, 12048, 12050, 12063, 12048]
    probs = []
    for j, L in enumerate(lens):
        sig = synth.make_signals(SIG_SEED, 1, L, first_read=120 + j)[0]
        probs.append(m.classify(proc.mad_normalise(sig.copy())).numpy())
    errors = {}
    for L in (12047, 12064, 6024):
        try:
            m.classify(proc.mad_normalise(synth.make_signals(SIG_SEED, 1, L, first_read=130)[0].copy()))
            errors[str(L)] = ""
        except Exception as e:                                    # noqa: BLE001 - the type is the datum
            errors[str(L)] = type(e).__name__
    np.savez_compressed(os.path.join(OUT, "fc_head.npz"), lens=np.array(lens), probs=np.stack(probs),
                        errors=np.array(json.dumps(errors)))
    print("F2d:", np.stack(probs)[:, 1], errors)


# --------------------------------------------------------------------------------------
def f4_polya():
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    cases = []
    for rid in range(40):
        n = 6000 + 523 * rid
        polya = rid % 4 != 3
        sig = synth.make_raw_read(91, rid, n, polya)
        end = proc.get_polyA_end(sig)
        cases.append([91, rid, n, int(polya), -1 if end is None else int(end)])
    # corners of the window rule (riser_amd.synth.polya_edge_cases: a plateau that never ends, reads shorter than a
    # window, a rise inside the first 1000 samples where the rule is inert, a rolling mean of 0, reads beyond 65536
    # samples): the signals are rebuilt from integer hashes, the fixture keeps the reference's answers
    import warnings
    names, ends = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # x / 0 in the rolling-mean case
        for name, sig in synth.polya_edge_cases():
            end = proc.get_polyA_end(sig)
            names.append(name)
            ends.append(-1 if end is None else int(end))
    np.savez_compressed(os.path.join(OUT, "polya.npz"), cases=np.array(cases, dtype=np.int64),
                        edge_names=np.array(names), edge_ends=np.array(ends, dtype=np.int64))
    print("F4:", [c[4] for c in cases])
    print("F4 edge:", dict(zip(names, ends)))


# --------------------------------------------------------------------------------------
def f5_resnet():
    """reference ResNet (riser/nets/resnet.py) in eval mode with randomised weights AND BatchNorm
    running statistics (default mean 0 / var 1 would hide folding bugs)."""
    from nets.resnet import ResNet
    out = {}
    rng = np.random.default_rng(31337)
    cfgs = {"basic": dict(channels=[8, 12, 20], kernel=19, padding=5, stride=3, block="basic", n_layers=3,
                          blocks=[1, 2, 1], n_classes=2),
            "bottleneck": dict(channels=[16, 24, 32], kernel=7, padding=3, stride=2, block="bottleneck", n_layers=3,
                               blocks=[2, 1, 2], n_classes=2)}
    for name, cfg in cfgs.items():
        net = ResNet(types.SimpleNamespace(**cfg))
        sd = net.state_dict()
        new = {}
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                new[k] = v
            elif k.endswith("running_var"):
                new[k] = torch.from_numpy(rng.uniform(0.5, 2.0, v.shape).astype(np.float32))
            elif k.endswith("running_mean"):
                new[k] = torch.from_numpy((rng.standard_normal(v.shape) * 0.3).astype(np.float32))
            elif ".1.weight" in k and v.dim() == 1:                        # BN gamma
                new[k] = torch.from_numpy(rng.uniform(0.6, 1.4, v.shape).astype(np.float32))
            elif v.dim() == 1:                                             # biases / BN beta
                new[k] = torch.from_numpy((rng.standard_normal(v.shape) * 0.1).astype(np.float32))
            else:
                fan_in = v.shape[1] * (v.shape[2] if v.dim() == 3 else 1)
                new[k] = torch.from_numpy((rng.standard_normal(v.shape) * np.sqrt(1.5 / fan_in)).astype(np.float32))
        net.load_state_dict(new)
        net.eval()
        for L in (3000, 4097):
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=40)
            proc = SignalProcessor(Kit.create_from_version("RNA004"))
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x))
                probs = torch.softmax(logits, dim=1)
            out[f"{name}.L{L}.logits"] = logits.numpy()
            out[f"{name}.L{L}.probs"] = probs.numpy()
        for k, v in new.items():
            if not k.endswith("num_batches_tracked"):
                out[f"{name}.sd.{k}"] = v.numpy()
        out[f"{name}.cfg"] = np.array(json.dumps(cfg))
        print("F5:", name, out[f"{name}.L3000.probs"][:, 1])
    np.savez_compressed(os.path.join(OUT, "resnet.npz"), **out)


# edge configs of tests/test_resnet_shapes.py (same names, configs and weight seed): each one a launch form of csrc/seqnet.hip
_RB = lambda ch, bl, k, p, s, block="basic": dict(channels=ch, kernel=k, padding=p, stride=s, block=block, n_layers=len(ch),
                                                  blocks=bl, n_classes=2)
RESNET_EDGE_CFGS = {
    "s1_w8_np56": _RB([12, 56], [1, 2], 19, 5, 3),           # stem nt 1, an 8-wave block, compact column pitch 56 < 64
    "np40": _RB([44, 40], [1, 2], 9, 4, 2),                  # a 40-channel stage after a 44-channel one: pitch 40, not 48
    "bneck_nto123": _RB([16, 32, 48], [1, 1, 1], 19, 5, 3, "bottleneck"),    # NTM 1 with NTO 1, 2, 3
    "bneck_nto45": _RB([64, 66, 72], [1, 1, 1], 9, 4, 2, "bottleneck"),      # NTO 4, NTO 5 at NTM 1 and at NTM 2
    "wide_stem": _RB([96, 40], [1, 1], 7, 3, 2),             # a stem wider than 80: unfused stem, pool and stage
    "mixed": _RB([40, 36, 76], [1, 1, 1], 9, 4, 2),          # bf16x3 mixes split and fp32 blocks
}
RESNET_EDGE_SEED = 17


def f5b_resnet_edges():
    """reference ResNet (riser/nets/resnet.py) in eval mode on the edge configs of the launch-form sweep: logits and
    probabilities of three synth reads at the program's minimum length, one more, 4097 and 16000.  The weights are not
    stored: they are synth.make_resnet_state_dict(seed, cfg), loaded strictly into the reference's own module, and the cfg
    records the seed and synth.state_dict_sha16 of them."""
    from nets.resnet import ResNet
    from riser_amd.resnet import build_program
    out = {}
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    for name, cfg in RESNET_EDGE_CFGS.items():
        net = ResNet(types.SimpleNamespace(**cfg))
        sd = synth.make_resnet_state_dict(RESNET_EDGE_SEED, cfg)
        new = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        for k, v in net.state_dict().items():
            # the generator makes neither the BN counters nor the shortcut of a block that does not apply one (the reference
            # builds it anyway, resnet.py:21-24, and its forward skips it, :40-47): the module's own values for those
            if k not in new:
                assert k.endswith("num_batches_tracked") or ".shortcut." in k, k
                new[k] = v
        net.load_state_dict(new, strict=True)
        net.eval()
        mn = 1
        while True:                                         # the shortest read every conv and pool of the program accepts
            try:
                with torch.no_grad():
                    net(torch.zeros((1, mn)))
                break
            except RuntimeError:
                mn += 1
        lens = (mn, mn + 1, 4097, 16000)
        for L in lens:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=80)
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x))
                probs = torch.softmax(logits, dim=1)
            out[f"{name}.L{L}.logits"] = logits.numpy()
            out[f"{name}.L{L}.probs"] = probs.numpy()
        build_program(sd, types.SimpleNamespace(**cfg))     # the state dict is one the program builder reads
        out[f"{name}.cfg"] = np.array(json.dumps(dict(cfg, lengths=[int(v) for v in lens], seed=RESNET_EDGE_SEED,
                                                      sd_sha16=synth.state_dict_sha16(sd))))
        print("F5b:", name, "min", mn, out[f"{name}.L4097.probs"][:, 1])
    np.savez_compressed(os.path.join(OUT, "resnet_edges.npz"), **out)


TCN_CFGS = {
    # name: (bottleneck, config); n_filters 18 and 36 leave channel counts off the multiples of 4 (padding paths)
    "tcn_k3_b2": (False, dict(in_channels=1, n_filters=24, kernel=3, dilation=2, n_layers=5, dropout=0.2, n_classes=2)),
    "tcn_k5_b3": (False, dict(in_channels=1, n_filters=18, kernel=5, dilation=3, n_layers=4, dropout=0.2, n_classes=2)),
    "bot_k3": (True, dict(in_channels=1, n_filters=32, kernel=3, dilation=2, n_layers=5, dropout=0.2, n_classes=2)),
    "bot_k5": (True, dict(in_channels=1, n_filters=36, kernel=5, dilation=2, n_layers=4, dropout=0.2, n_classes=2)),
}


def tcn_lengths(rf):
    """below the receptive field, at it, one past it, and well above it"""
    return (max(2, rf // 3), rf, rf + 1, 4097, 12000)


def _tcn_golden(cfgs, seed, path, tag):
    """reference TCN / TCNBot (riser/nets/tcn.py, tcn_bot.py) in eval mode with randomised weights: weight_v, a weight_g
    that is not ||v|| (weight_norm's initial value would hide folding bugs), non-zero biases, every shortcut (used or not);
    logits and probabilities at tcn_lengths(rf) of three synth reads."""
    from nets.tcn import TCN
    from nets.tcn_bot import TCNBot
    out = {}
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    for name, (bot, cfg) in cfgs.items():
        net = (TCNBot if bot else TCN)(types.SimpleNamespace(**cfg))
        sd = net.state_dict()
        new = {}
        for k, v in sd.items():
            if k.endswith("weight_g"):
                new[k] = torch.from_numpy(rng.uniform(0.5, 1.5, v.shape).astype(np.float32))
            elif v.dim() == 1:                                              # biases
                new[k] = torch.from_numpy((rng.standard_normal(v.shape) * 0.1).astype(np.float32))
            else:                                                           # weight_v, shortcut and linear weights
                fan_in = int(np.prod(v.shape[1:]))
                new[k] = torch.from_numpy((rng.standard_normal(v.shape) * np.sqrt(1.0 / fan_in)).astype(np.float32))
        net.load_state_dict(new)
        net.eval()
        rf = net.get_receptive_field(cfg["kernel"], cfg["n_layers"]) if bot else \
            net.get_receptive_field(cfg["kernel"], cfg["n_layers"], cfg["dilation"])
        lens = tcn_lengths(rf)
        proc = SignalProcessor(Kit.create_from_version("RNA004"))
        for L in lens:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x))
                probs = torch.softmax(logits, dim=1)
            out[f"{name}.L{L}.logits"] = logits.numpy()
            out[f"{name}.L{L}.probs"] = probs.numpy()
        for k, v in new.items():
            out[f"{name}.sd.{k}"] = v.numpy()
        out[f"{name}.cfg"] = np.array(json.dumps(dict(cfg, model="tcn-bot" if bot else "tcn", rf=int(rf),
                                                      lengths=[int(v) for v in lens])))
        print(f"{tag}:", name, "RF", rf, out[f"{name}.L4097.probs"][:, 1])
    np.savez_compressed(os.path.join(OUT, path), **out)


def f6_tcn():
    _tcn_golden(TCN_CFGS, 4242, "tcn.npz", "F6")


TCN_EDGE_CFGS = {
    # the edges of the device's TCN program the configs above leave out (tests/test_tcn_shapes.py sweeps them on the GPU)
    "tcn_f1_k2": (False, dict(in_channels=1, n_filters=1, kernel=2, dilation=1, n_layers=3, dropout=0.2, n_classes=2)),
    "tcn_k5_l1": (False, dict(in_channels=1, n_filters=20, kernel=5, dilation=3, n_layers=1, dropout=0.2, n_classes=2)),
    "tcn_k2_b4": (False, dict(in_channels=1, n_filters=13, kernel=2, dilation=4, n_layers=7, dropout=0.2, n_classes=2)),
    "tcn_f68": (False, dict(in_channels=1, n_filters=68, kernel=3, dilation=2, n_layers=2, dropout=0.2, n_classes=2)),
    "bot_f4": (True, dict(in_channels=1, n_filters=4, kernel=3, dilation=2, n_layers=4, dropout=0.2, n_classes=2)),
    "bot_f22_k2": (True, dict(in_channels=1, n_filters=22, kernel=2, dilation=2, n_layers=6, dropout=0.2, n_classes=2)),
}


def f6b_tcn_edges():
    """F6 at the edges: one filter (identity residual in block 0), one layer, k 2, base 4, a partial second 64-column
    group (68 filters), TCNBot mid widths 1 and 5"""
    _tcn_golden(TCN_EDGE_CFGS, 4243, "tcn_edges.npz", "F6b")


CRNN_CFGS = {
    # LSTM and GRU, uni- and bidirectional, n_rec_layers 1 / 2 / 3 (1, 4 and 9 stacked layers), an even conv kernel, hidden
    # sizes off the multiples of 16 (17, 20) and above 128 (130: W_hh not register-resident on the device), one conv layer
    "lstm_bi_r2": dict(n_conv_layers=3, channels=[8, 16, 16], kernels=[5, 4, 3], cell="lstm", hidden=20, n_rec_layers=2,
                       bidirectional=True, dropout=0.2, n_classes=2),
    "gru_bi_r1_c1": dict(n_conv_layers=1, channels=[12], kernels=[6], cell="gru", hidden=17, n_rec_layers=1,
                         bidirectional=True, dropout=0.2, n_classes=2),
    "lstm_uni_r3": dict(n_conv_layers=2, channels=[16, 24], kernels=[7, 3], cell="lstm", hidden=24, n_rec_layers=3,
                        bidirectional=False, dropout=0.2, n_classes=2),
    "gru_uni_r2_h130": dict(n_conv_layers=2, channels=[8, 32], kernels=[3, 3], cell="gru", hidden=130, n_rec_layers=2,
                            bidirectional=False, dropout=0.2, n_classes=2),
    "lstm_bi_h130": dict(n_conv_layers=2, channels=[8, 16], kernels=[4, 5], cell="lstm", hidden=130, n_rec_layers=1,
                         bidirectional=True, dropout=0.2, n_classes=2),
    "gru_bi_r2": dict(n_conv_layers=3, channels=[8, 16, 32], kernels=[3, 5, 3], cell="gru", hidden=32, n_rec_layers=2,
                      bidirectional=True, dropout=0.2, n_classes=2),
}


CRNN_GAIN = 2.0        # synth.make_crnn_state_dict's gain for the fixture: every mutant of tests/crnn_ref.py shows


def crnn_min_length(kernels):
    need = 1
    for k in reversed(kernels):
        need = 2 * need + k - 1
    return need


def crnn_odd_pool_length(kernels, start):
    """the shortest length from `start` on where some max_pool drops an odd last sample"""
    L0 = start
    while True:
        L, odd = L0, False
        for k in kernels:
            odd |= (L - k + 1) % 2 == 1
            L = (L - k + 1) // 2
        if odd:
            return L0
        L0 += 1


def crnn_lengths(kernels):
    mn = crnn_min_length(kernels)
    return (mn, mn + 1, crnn_odd_pool_length(kernels, mn + 2), 4097, 12000)


def f7_crnn():
    """reference ConvRecNet (riser/nets/cnn_rnn.py) in eval mode with random weights and non-zero biases (b_ih and b_hh
    both); logits and probabilities at crnn_lengths of three synth reads.  The weights are not stored: they are
    synth.make_crnn_state_dict(seed, cfg) (the integer hash, the same on every platform), loaded strictly into the
    reference's own module, and the cfg records the seed and synth.state_dict_sha16 of them so that a test can rebuild them
    and tell when the generator has drifted."""
    from nets.cnn_rnn import ConvRecNet
    out = {}
    torch.manual_seed(4711)
    for n, (name, cfg) in enumerate(CRNN_CFGS.items()):
        net = ConvRecNet(types.SimpleNamespace(**cfg))
        seed = 4711 + n
        sd = synth.make_crnn_state_dict(seed, cfg, gain=CRNN_GAIN)
        new = {k: torch.from_numpy(v) for k, v in sd.items()}
        net.load_state_dict(new, strict=True)                          # the reference's own key set and shapes
        net.eval()
        lens = crnn_lengths(cfg["kernels"][: cfg["n_conv_layers"]])
        proc = SignalProcessor(Kit.create_from_version("RNA004"))
        for L in lens:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x))
                probs = torch.softmax(logits, dim=1)
            out[f"{name}.L{L}.logits"] = logits.numpy()
            out[f"{name}.L{L}.probs"] = probs.numpy()
        out[f"{name}.cfg"] = np.array(json.dumps(dict(cfg, model="cnn-rnn", min_length=int(lens[0]),
                                                      lengths=[int(v) for v in lens], seed=seed, gain=CRNN_GAIN,
                                                      sd_sha16=synth.state_dict_sha16(sd))))
        print("F7:", name, "min", lens[0], out[f"{name}.L4097.probs"][:, 1])
    np.savez_compressed(os.path.join(OUT, "crnn.npz"), **out)


def f7b_crnn_edges():
    """F7 at the edges of the device program's shape arithmetic, on six configs of tests/test_crnn_shapes.py (taken from
    there with their seeds, so the two cannot drift apart): taps 1 and 2, a 19-tap kernel over 8 channels, six conv layers,
    13 / 100 / 130 output channels, hidden 5, 129 and 320.  Logits and probabilities of three synth reads at the minimum
    length, one more, an odd-pool length and 4097; prints the largest gap to the float64 forward of tests/crnn_ref.py."""
    from nets.cnn_rnn import ConvRecNet
    from riser_amd import crnn as R
    from tests import crnn_ref
    from tests import test_crnn_shapes as S
    out, worst = {}, 0.0
    proc = SignalProcessor(Kit.create_from_version("RNA004"))
    for name in S.EDGES:
        cfg, seed = S.CONFIGS[name], S.SEED[name]
        net = ConvRecNet(types.SimpleNamespace(**cfg))
        sd = synth.make_crnn_state_dict(seed, cfg, gain=S.GAIN)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net.eval()
        prog = R.build_crnn_program(sd, types.SimpleNamespace(**cfg))
        lens = S.edge_lengths(prog)
        assert lens[0] == crnn_min_length(cfg["kernels"])
        for L in lens:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([proc.mad_normalise(s.copy()) for s in sigs]).astype(np.float32)
            with torch.no_grad():
                logits = net(torch.from_numpy(x))
                probs = torch.softmax(logits, dim=1)
            out[f"{name}.L{L}.logits"] = logits.numpy()
            out[f"{name}.L{L}.probs"] = probs.numpy()
            gap = float(np.abs(crnn_ref.forward(prog, x) - logits.numpy()).max())
            worst = max(worst, gap)
        out[f"{name}.cfg"] = np.array(json.dumps(dict(cfg, lengths=[int(v) for v in lens], seed=seed, gain=S.GAIN,
                                                      sd_sha16=synth.state_dict_sha16(sd))))
        print("F7b:", name, "min", lens[0], out[f"{name}.L4097.probs"][:, 1], "float64 gap so far %.2e" % worst)
    np.savez_compressed(os.path.join(OUT, "crnn_edges.npz"), **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["f1", "f2", "f3", "f4", "f5", "f6"]
    if "f1" in which:
        f1_normalise()
    if "f1b" in which or "f1" in which:
        f1b_normalise_float()
    if "f4" in which:
        f4_polya()
    if "f2" in which:
        f2_network()
    if "f2b" in which or "f2" in which:
        f2b_convnet_variants()
    if "f2c" in which or "f2" in which:
        f2c_gap_head()
    if "f2d" in which or "f2" in which:
        f2d_fc_head()
    if "f2e" in which:
        f2e_gconv_edges()
    if "f3" in which:
        f3_control()
    if "f5" in which:
        f5_resnet()
    if "f5b" in which:
        f5b_resnet_edges()
    if "f6" in which:
        f6_tcn()
    if "f6b" in which:
        f6b_tcn_edges()
    if "f7" in which:
        f7_crnn()
    if "f7b" in which:
        f7b_crnn_edges()
