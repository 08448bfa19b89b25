"""CNN-RNN (riser/nets/cnn_rnn.py, ConvRecNet): the host-side program and a float64 forward of it pinned to the
reference's own outputs (tests/golden/crnn.npz, CPU), and the device program (csrc/crnn.hip) behind `Model`."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import crnn as R
from riser_amd import synth
from tests import crnn_ref

NAMES = ["lstm_bi_r2", "gru_bi_r1_c1", "lstm_uni_r3", "gru_uni_r2_h130", "lstm_bi_h130", "gru_bi_r2"]
CFG_KEYS = ("n_conv_layers", "channels", "kernels", "cell", "hidden", "n_rec_layers", "bidirectional", "dropout", "n_classes")


def tol(ref):
    """the device's tolerance on a logit, relative above 1: 4x the largest gap measured on an MI355X over the eight configs of
    this file, rounded up (the fixtures against the reference and float64, the ragged sweeps, the 512-read bench batches).
    Measured, x max(1, |logit|): lstm_bi_r2 5.7e-8, gru_bi_r1_c1 2.8e-7, lstm_uni_r3 2.7e-8, gru_uni_r2_h130 4.0e-7,
    lstm_bi_h130 4.0e-7, gru_bi_r2 3.4e-7, bench_lstm 7.4e-8, bench_gru 2.8e-7"""
    return 2e-6 * np.maximum(1.0, np.abs(ref))


def held(tag, got, ref):
    """print the largest gap in units of max(1, |logit|), then hold every logit to tol()"""
    err = np.abs(got - ref)
    print(f"\nCRNN_GAP {tag} max|dev-ref|/scale {float((err / np.maximum(1.0, np.abs(ref))).max()):.3e}")
    assert (err <= tol(ref)).all(), (tag, float(err.max()))


def _load(golden_dir, name):
    """the fixture's outputs, its cfg and the weights it was made with: synth.make_crnn_state_dict(cfg seed), the same on
    every platform (the fixture stores their digest, not the weights)"""
    g = np.load(os.path.join(golden_dir, "crnn.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = synth.make_crnn_state_dict(cfg["seed"], {k: cfg[k] for k in CFG_KEYS}, gain=cfg["gain"])
    return g, cfg, sd


def _ns(cfg):
    return types.SimpleNamespace(**{k: cfg[k] for k in CFG_KEYS})


def _inputs(L):
    sigs = synth.make_signals(20260103, 3, L, first_read=60)
    return np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)


def _config(cfg):
    return types.SimpleNamespace(model="cnn-rnn", cnn_rnn=_ns(cfg))


def _bench(cell):
    cfg = synth.CRNN_BENCH_CFG if cell == "lstm" else synth.CRNN_GRU_BENCH_CFG
    return cfg, synth.make_crnn_state_dict(11 if cell == "lstm" else 12, cfg)


def odd_pool_length(prog, start):
    L0 = start
    while True:
        L, odd = L0, False
        for cv in prog["convs"]:
            odd |= (L - cv["k"] + 1) % 2 == 1
            L = (L - cv["k"] + 1) // 2
        if odd:
            return L0
        L0 += 1


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", NAMES)
def test_fixture_weights_rebuild_bit_for_bit(golden_dir, name):
    _, cfg, sd = _load(golden_dir, name)
    assert synth.state_dict_sha16(sd) == cfg["sd_sha16"]


@pytest.mark.parametrize("name", NAMES)
def test_float64_forward_matches_reference(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    assert len(prog["layers"]) == cfg["n_rec_layers"] ** 2
    for L in cfg["lengths"]:
        x = _inputs(L)
        lg = crnn_ref.forward(prog, x)
        assert np.abs(lg - g[f"{name}.L{L}.logits"]).max() < 1e-5, L
        # the last backward direction's one step is the full backward pass read at t = T - 1, exactly
        assert np.array_equal(lg, crnn_ref.forward(prog, x, one_step=False)), L


@pytest.mark.parametrize("name", NAMES)
def test_aligned_ragged_forward_equals_per_read_forwards(golden_dir, name):
    _, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    mn = R.min_length(prog)
    reads = [ro.mad_normalise(synth.make_signals(20260103, 1, n, first_read=80 + i)[0]).astype(np.float32)
             for i, n in enumerate((mn, mn + 1, odd_pool_length(prog, mn + 2), 900, 333, 2501))]
    want = np.concatenate([crnn_ref.forward(prog, r[None]) for r in reads])
    assert np.abs(crnn_ref.forward_ragged(prog, reads) - want).max() < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_mutants_miss_by_more_than_ten_tolerances(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    x = _inputs(4097)
    good = crnn_ref.forward(prog, x)
    applied = 0
    for mut in crnn_ref.MUTANTS:
        if not crnn_ref.mutant_applies(cfg, mut):
            continue
        applied += 1
        bad = crnn_ref.forward(prog, x, mutant=mut)
        assert (np.abs(bad - good) / tol(good)).max() > 10, mut
    assert applied >= 2


def test_every_mutant_applies_somewhere(golden_dir):
    cfgs = [_load(golden_dir, n)[1] for n in NAMES]
    for mut in crnn_ref.MUTANTS:
        assert any(crnn_ref.mutant_applies(c, mut) for c in cfgs), mut


@pytest.mark.parametrize("name", NAMES)
def test_steps_and_min_length_match_torch(golden_dir, name):
    import torch
    g, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    mn = R.min_length(prog)
    assert mn == cfg["min_length"]
    convs = [torch.nn.Sequential(torch.nn.Conv1d(cv["w"].shape[1], cv["w"].shape[0], cv["k"]), torch.nn.MaxPool1d(2, 2))
             for cv in prog["convs"]]

    def torch_steps(L):
        x = torch.zeros(1, 1, L)
        with torch.no_grad():
            for m in convs:
                x = m(x)
        return x.shape[2]

    with pytest.raises(RuntimeError):
        torch_steps(mn - 1)
    assert R.steps(prog, mn - 1) == 0
    for L in (mn, mn + 1, odd_pool_length(prog, mn + 2), 4097, 16000):
        assert R.steps(prog, L) == torch_steps(L) >= 1, L
    assert R.steps(prog, mn) == 1


def _sd_cfg(cell="lstm", bidir=True, n_rec=2):
    cfg = dict(n_conv_layers=2, channels=[8, 12], kernels=[3, 4], cell=cell, hidden=10, n_rec_layers=n_rec,
               bidirectional=bidir, dropout=0.0, n_classes=2)
    return synth.make_crnn_state_dict(3, cfg), cfg


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_build_program_reads_both_key_sets_and_flattens(cell):
    sd, cfg = _sd_cfg(cell)
    prog = R.build_crnn_program(sd, types.SimpleNamespace(**cfg))
    ng = 4 if cell == "lstm" else 3
    assert [lay["relu_after"] for lay in prog["layers"]] == [False, True, False, True]
    assert [lay["in_dim"] for lay in prog["layers"]] == [12, 20, 20, 20]
    assert all(lay["w_ih"][1].shape[0] == ng * 10 for lay in prog["layers"])
    assert np.array_equal(prog["layers"][3]["w_hh"][1], sd["rec_layers.1.weight_hh_l1_reverse"])
    assert prog["out_dim"] == 20 and prog["fc_w"].shape == (2, 20)
    assert R.min_length(prog) == 2 * (2 * 1 + 4 - 1) + 3 - 1
    assert R.program_macs(prog, 100) > 0


def test_build_program_refusals():
    sd, cfg = _sd_cfg("lstm")
    ns = types.SimpleNamespace
    bad_cfgs = [dict(cfg, cell="rnn"), dict(cfg, n_classes=3), dict(cfg, channels=[8]), dict(cfg, kernels=[3]),
                dict(cfg, channels=[8, 12, 99], n_conv_layers=2), dict(cfg, hidden=11), dict(cfg, kernels=[3, 5])]
    for c in bad_cfgs:
        with pytest.raises(ValueError):
            R.build_crnn_program(sd, ns(**c))
    no_rev = {k: v for k, v in sd.items() if k != "rec_layers.1.bias_hh_l0_reverse"}
    with pytest.raises(ValueError, match="_reverse"):
        R.build_crnn_program(no_rev, ns(**cfg))
    wrong = dict(sd, **{"linear.weight": np.zeros((2, 7), np.float32)})
    with pytest.raises(ValueError):
        R.build_crnn_program(wrong, ns(**cfg))
    # a GRU state dict under an LSTM config: every gate matrix has the wrong height
    sd_gru, _ = _sd_cfg("gru")
    with pytest.raises(ValueError):
        R.build_crnn_program(sd_gru, ns(**cfg))


CRNN_YAML = """model: cnn-rnn
batch_size: 32

cnn_rnn:
  n_conv_layers: 3
  channels: [8, 16, 16]
  kernels: [5, 4, 3]
  cell: lstm
  hidden: 20
  n_rec_layers: 2
  bidirectional: true
  dropout: 0.2
  n_classes: 2
"""


def _write_model_dir(tmp_path, golden_dir, name="lstm_bi_r2"):
    import torch
    g, cfg, sd = _load(golden_dir, name)
    d = tmp_path / "model"
    d.mkdir(exist_ok=True)
    (d / "mRNA_config_RNA004_RP4.yaml").write_text(CRNN_YAML)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(d / "mRNA_model_RNA004_RP4.pth"))
    return str(d), cfg, sd


@pytest.mark.parametrize("parser", ["yaml", "flat"])
def test_modeldir_reads_a_cnn_rnn_config(tmp_path, golden_dir, monkeypatch, parser):
    import builtins
    from riser_amd import modeldir
    d, cfg, _ = _write_model_dir(tmp_path, golden_dir)
    if parser == "flat":
        real = builtins.__import__

        def no_yaml(name, *a, **kw):
            if name == "yaml":
                raise ImportError(name)
            return real(name, *a, **kw)
        monkeypatch.setattr(builtins, "__import__", no_yaml)
    c = modeldir.get_config(os.path.join(d, "mRNA_config_RNA004_RP4.yaml"))
    assert c.model == "cnn-rnn" and not hasattr(c, "cnn")
    for k in CFG_KEYS:
        if k != "dropout":
            assert getattr(c.cnn_rnn, k) == cfg[k], k


def test_abi_2_9_symbols_and_null_handles():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    lib = nv.lib()
    for s in ("rs_crnn_create", "rs_crnn_destroy", "rs_crnn_min_length", "rs_crnn_steps", "rs_crnn_workspace_bytes",
              "rs_crnn_max_batch", "rs_crnn_forward_ragged"):
        assert s in nv.SYMBOLS and hasattr(lib, s), s
    assert lib.rs_version() == (2 << 16) | 9
    h = C.c_void_p()
    assert lib.rs_crnn_create(None, 1, None, 1, None, None, 2, 0, C.byref(h)) == nv.RS_ERR_ARG
    assert b"rs_crnn_create" in lib.rs_last_error()
    assert lib.rs_crnn_create(None, 1, None, 1, None, None, 2, 0, None) == nv.RS_ERR_ARG
    assert lib.rs_crnn_min_length(None) == nv.RS_ERR_ARG and b"rs_crnn_min_length" in lib.rs_last_error()
    assert lib.rs_crnn_steps(None, 100) == nv.RS_ERR_ARG and b"rs_crnn_steps" in lib.rs_last_error()
    assert lib.rs_crnn_forward_ragged(None, None, None, 1, 100, None, 0, None, None, None) == nv.RS_ERR_ARG
    assert b"rs_crnn_forward_ragged" in lib.rs_last_error()
    assert lib.rs_crnn_workspace_bytes(None, 1, 100) == 0 and lib.rs_crnn_max_batch(None, 100) == 0
    assert lib.rs_crnn_destroy(None) == nv.RS_OK
    # a cell other than LSTM / GRU, checked before any device is touched
    sd, cfg = _sd_cfg("lstm", bidir=False, n_rec=1)
    prog = R.build_crnn_program(sd, types.SimpleNamespace(**cfg))
    convs = (R._Conv * 2)(*[R._Conv(cv["w"].shape[1], cv["w"].shape[0], cv["k"], 0, cv["w"].ctypes.data,
                                    cv["b"].ctypes.data) for cv in prog["convs"]])
    lay = prog["layers"][0]
    layers = (R._Layer * 1)()
    layers[0].cell, layers[0].in_dim, layers[0].hidden, layers[0].relu_after = 2, lay["in_dim"], lay["hidden"], 1
    layers[0].w_ih[0], layers[0].w_hh[0] = lay["w_ih"][0].ctypes.data, lay["w_hh"][0].ctypes.data
    layers[0].b_ih[0], layers[0].b_hh[0] = lay["b_ih"][0].ctypes.data, lay["b_hh"][0].ctypes.data
    assert lib.rs_crnn_create(convs, 2, layers, 1, prog["fc_w"].ctypes.data, prog["fc_b"].ctypes.data, 10, 0,
                              C.byref(h)) == nv.RS_ERR_ARG
    assert b"rs_crnn_create" in lib.rs_last_error() and not h.value


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_model_matches_reference_and_float64(golden_dir, name):
    import torch
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    assert m.dtype == "f32" and m.min_length == cfg["min_length"]
    for L in cfg["lengths"]:
        x = _inputs(L)
        wl, wp = g[f"{name}.L{L}.logits"], g[f"{name}.L{L}.probs"]
        f64 = crnn_ref.forward(prog, x)
        probs, logits = m.classify_batch(x, return_logits=True)
        lg = logits.cpu().numpy()
        held(f"{name} L{L} reference", lg, wl)
        held(f"{name} L{L} float64", lg, f64)
        assert np.abs(probs.cpu().numpy() - wp).max() < 1e-5, L
        fb = m.forward_batch(torch.from_numpy(x).to(m.device), np.full(3, L, dtype=np.int32)).cpu().numpy()
        assert np.array_equal(fb, probs.cpu().numpy())
        for i in range(3):
            assert np.array_equal(m.classify(x[i]).cpu().numpy(), probs.cpu().numpy()[i]), (L, i)
    m.close()


def _sweep_lengths(mn, prog, rng, n=77):
    fixed = [mn, mn + 1, odd_pool_length(prog, mn + 2), 4096, 4097, 8615, 16000]
    return fixed + [int(v) for v in rng.integers(mn, 16001, n - len(fixed))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES + ["bench_lstm", "bench_gru"])
def test_ragged_sweep_against_float64_and_solo_runs(golden_dir, name):
    from riser_amd.model import Model
    if name.startswith("bench_"):
        cfg, sd = _bench(name[6:])
    else:
        _, cfg, sd = _load(golden_dir, name)
    prog = R.build_crnn_program(sd, _ns(cfg))
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    rng = np.random.default_rng(sum(name.encode()))
    lens = _sweep_lengths(m.min_length, prog, rng)
    sigs = [ro.mad_normalise(synth.make_signals(20260103, 1, n, first_read=300 + i)[0]).astype(np.float32)
            for i, n in enumerate(lens)]
    probs, logits = m.classify_batch(sigs, return_logits=True)
    logits = logits.cpu().numpy()
    want = crnn_ref.forward_ragged(prog, sigs)
    held(f"{name} ragged float64", logits, want)
    for i, s in enumerate(sigs):
        _, l1 = m.classify_batch([s], return_logits=True)
        assert np.array_equal(logits[i], l1.cpu().numpy()[0]), (name, i, lens[i])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_bench_net_512_raw_reads(cell):
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    cfg, sd = _bench(cell)
    prog = R.build_crnn_program(sd, _ns(cfg))
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    sigs = synth.make_signals(20260103, 512, 16000)
    sig, off, ln, lh = pack_reads(sigs, m.device)
    probs, logits = m.classify_raw(sig, off, ln, lh, return_logits=True)
    x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
    want = np.concatenate([crnn_ref.forward(prog, x[i:i + 128]) for i in range(0, 512, 128)])
    held(f"bench_{cell} 512 float64", logits.cpu().numpy(), want)
    m.close()


def _raw_reads(lens, first=700):
    return [synth.make_signals(20260103, 1, n, first_read=first + i)[0] for i, n in enumerate(lens)]


@pytest.mark.gpu
def test_classify_raw_normalises_the_whole_read(golden_dir):
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    g, cfg, sd = _load(golden_dir, "gru_bi_r2")
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    prog = R.build_crnn_program(sd, _ns(cfg))
    sigs = _raw_reads([4096, 5000, 8615, 300, 12000])
    sig, off, ln, lh = pack_reads(sigs, m.device)
    probs = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    for i, s in enumerate(sigs):
        x = ro.mad_normalise(s).astype(np.float32)
        want = ro.softmax(crnn_ref.forward(prog, x[None]))[0]
        assert np.abs(probs[i] - want).max() < 1e-5, i
    m.close()


@pytest.mark.gpu
def test_ensemble_of_two_crnns_decides_like_rs_decide(golden_dir):
    import torch
    from riser_amd import _native as nv
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    g1, c1, sd1 = _load(golden_dir, "lstm_bi_r2")
    g2, c2, sd2 = _load(golden_dir, "gru_bi_r2")
    dev = _dev()
    models = [Model(sd1, _config(c1), None, "a", device=dev), Model(sd2, _config(c2), None, "b", device=dev)]
    sigs = _raw_reads([4096, 5000, 8615, 300, 12000, 16000, 2000], first=900)
    sig, off, ln, lh = pack_reads(sigs, dev)
    dec = torch.empty(len(sigs), dtype=torch.uint8, device=dev)
    probs = classify_raw_ensemble(models, sig, off, ln, lh, decision=dec, max_len=12000, threshold=0.6)
    for k, m in enumerate(models):
        assert torch.equal(probs[k], m.classify_raw(sig, off, ln, lh))
    want = torch.empty_like(dec)
    p2 = probs.contiguous()
    nv.check(nv.lib().rs_decide(p2.data_ptr(), 2, len(sigs), ln.data_ptr(), 12000, 0.6, nv.RS_ENRICH, want.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    assert torch.equal(dec, want)
    for m in models:
        m.close()


@pytest.mark.gpu
def test_batch_beyond_max_batch_is_split(golden_dir, monkeypatch):
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, "lstm_bi_r2")
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    lens = [4097, 300, 16000, 125, 9000, 70, 12000]
    sigs = [ro.mad_normalise(s).astype(np.float32) for s in _raw_reads(lens, first=40)]
    whole = m.classify_batch(sigs).cpu().numpy()
    assert m.max_batch(16000) > len(sigs)
    monkeypatch.setattr(type(m._seq), "max_batch", lambda self, L: 3)
    split = m.classify_batch(sigs).cpu().numpy()
    assert np.array_equal(whole, split)
    m.close()


@pytest.mark.gpu
def test_get_models_and_sequencer_control_run_a_crnn(tmp_path, golden_dir):
    import logging
    import torch
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd import _native as nv
    from riser_amd.fake_client import FakeClient, FakeRead
    from riser_amd.modeldir import get_models
    d, cfg, sd = _write_model_dir(tmp_path, golden_dir)
    dev = _dev()
    (m,) = get_models(["mRNA"], logging.getLogger("t"), "RNA004", model_dir=d, device=dev)
    assert m._h is None and isinstance(m._seq, R.CRNNNet)
    rng = np.random.default_rng(12)
    batches = [[(ch, FakeRead(f"id-{b * 7 + ch}", synth.make_raw_read(56, b * 7 + ch, int(rng.integers(3000, 24000)),
                                                                      polya=((b * 7 + ch) % 4 != 0))))
                for ch in range(1, 25)] for b in range(2)]
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    out = str(tmp_path / "o")
    ctl = SequencerControl(FakeClient(batches), [m], proc, logging.getLogger("c"), out)
    ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
    lines = open(out + ".csv").read().strip().split("\n")
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) > 10
    names = {"try_again": nv.RS_TRY_AGAIN, "accept": nv.RS_ACCEPT, "reject": nv.RS_REJECT, "no_decision": nv.RS_NO_DECISION}
    p1 = np.array([[float(v) for v in r[5].split(";")] for r in rows], dtype=np.float32)
    probs = torch.from_numpy(np.stack([1 - p1[:, 0], p1[:, 0]], axis=1)[None].copy()).to(dev)
    lens = torch.tensor([int(r[3]) for r in rows], dtype=torch.int32, device=dev)
    dec = torch.empty(len(rows), dtype=torch.uint8, device=dev)
    nv.check(nv.lib().rs_decide(probs.data_ptr(), 1, len(rows), lens.data_ptr(), ro.kit_max_length("RNA004"), 0.9,
                                nv.RS_ENRICH, dec.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    for r, dk in zip(rows, dec.cpu().numpy()):
        q = float(r[5])
        if abs(q - 0.9) < 1e-4 or abs(1 - q - 0.9) < 1e-4:
            continue
        assert names[r[8]] == dk, r
    m.close()


@pytest.mark.gpu
def test_refuses_other_dtypes_and_short_reads(golden_dir):
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, "gru_bi_r1_c1")
    with pytest.raises(ValueError, match="f32"):
        Model(sd, _config(cfg), None, "mRNA", dtype="bf16x3", device=_dev())
    # a config without `model` and without `cnn` selects the net from its `cnn_rnn` section
    m = Model(sd, types.SimpleNamespace(cnn_rnn=_ns(cfg)), None, "mRNA", device=_dev())
    mn = m.min_length
    with pytest.raises(ValueError, match="shorter than the network minimum"):
        m.classify_batch([np.zeros(mn - 1, np.float32), np.zeros(mn + 5, np.float32)])
    assert np.isfinite(m.classify(np.zeros(mn, np.float32)).cpu().numpy()).all()
    m.close()
