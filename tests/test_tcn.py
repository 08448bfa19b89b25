"""TCN and bottleneck TCN (riser/nets/tcn.py, riser/nets/tcn_bot.py): the host-side program and its strided-cone
formulation pinned to the reference's own outputs (tests/golden/tcn.npz, CPU), and the device program behind `Model`."""
import json
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import synth
from riser_amd import tcn as T
from tests.tcn_ref import cone_forward, dense_forward

NAMES = ["tcn_k3_b2", "tcn_k5_b3", "bot_k3", "bot_k5"]


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "tcn.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
    return g, cfg, sd


def _ns(cfg):
    return types.SimpleNamespace(**{k: v for k, v in cfg.items() if k not in ("model", "rf", "lengths")})


def _program(cfg, sd):
    return T.build_tcn_program(sd, _ns(cfg), cfg["model"] == "tcn-bot")


def _inputs(L):
    sigs = synth.make_signals(20260103, 3, L, first_read=60)
    return np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)


def _config(cfg):
    key = "tcnbot" if cfg["model"] == "tcn-bot" else "tcn"
    return types.SimpleNamespace(model=cfg["model"], **{key: _ns(cfg)})


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", NAMES)
def test_dense_forward_on_folded_weights_matches_reference(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    blocks, fw, fb = _program(cfg, sd)
    for L in cfg["lengths"]:
        lg = dense_forward(blocks, fw, fb, _inputs(L))
        assert np.abs(lg - g[f"{name}.L{L}.logits"]).max() < 1e-5, L


@pytest.mark.parametrize("name", NAMES)
def test_strided_cone_matches_reference(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    blocks, fw, fb = _program(cfg, sd)
    for L in cfg["lengths"]:
        x = _inputs(L)
        lg = cone_forward(blocks, fw, fb, x)
        assert np.abs(lg - g[f"{name}.L{L}.logits"]).max() < 1e-5, L
        # a wider pitch (the windows of a longer read) changes nothing: the extra positions are below 0
        assert np.abs(cone_forward(blocks, fw, fb, x, ld=L + 777) - lg).max() == 0.0


def test_cone_window_arithmetic():
    cfg = dict(in_channels=1, n_filters=8, kernel=3, dilation=2, n_layers=8, dropout=0.0, n_classes=2)
    sd = _random_sd(cfg, False, 3)
    blocks, _, _ = T.build_tcn_program(sd, types.SimpleNamespace(**cfg), False)
    need = T.windows(blocks, 16000)
    assert need[-1] == 1 and need[-2] == 5                         # last block of a k 3 TCN: 1 + 2 (k - 1) positions
    for i in range(len(blocks)):
        assert need[i] == min((need[i + 1] - 1) * 2 + 5, -(-16000 // 2 ** i))
    # a huge base: the windows are clamped to what a read of ld samples has
    cfg_big = dict(cfg, dilation=40, n_layers=6)
    b2, _, _ = T.build_tcn_program(_random_sd(cfg_big, False, 4), types.SimpleNamespace(**cfg_big), False)
    assert T.receptive_field(b2) == 1 + 2 * 2 * sum(40 ** i for i in range(6))
    assert all(n <= -(-4000 // b["dilation"]) for n, b in zip(T.windows(b2, 4000), b2))


def _random_sd(cfg, bot, seed, parametrization=False):
    """a reference-format state dict from the reference's key layout (weight_g / weight_v, every shortcut present)"""
    rng = np.random.default_rng(seed)
    sd = {}
    nf, k = cfg["n_filters"], cfg["kernel"]
    for i in range(cfg["n_layers"]):
        cin = cfg["in_channels"] if i == 0 else nf
        if bot:
            ch = nf // 4
            shapes = [(ch, cin, 1), (ch, ch, k), (ch, ch, k), (nf, ch, 1)]
        else:
            shapes = [(nf, cin, k), (nf, nf, k)]
        for j, s in enumerate(shapes):
            pre = f"layers.{i}.blocks.{j}.0"
            g = rng.uniform(0.5, 1.5, (s[0], 1, 1)).astype(np.float32)
            v = rng.standard_normal(s).astype(np.float32)
            if parametrization:
                sd[pre + ".parametrizations.weight.original0"] = g
                sd[pre + ".parametrizations.weight.original1"] = v
            else:
                sd[pre + ".weight_g"] = g
                sd[pre + ".weight_v"] = v
            sd[pre + ".bias"] = rng.standard_normal(s[0]).astype(np.float32) * 0.1
        sd[f"layers.{i}.shortcut.weight"] = rng.standard_normal((nf, cin, 1)).astype(np.float32)
        sd[f"layers.{i}.shortcut.bias"] = rng.standard_normal(nf).astype(np.float32)
    sd["linear.weight"] = rng.standard_normal((cfg["n_classes"], nf)).astype(np.float32) * 0.3
    sd["linear.bias"] = rng.standard_normal(cfg["n_classes"]).astype(np.float32) * 0.1
    return sd


@pytest.mark.parametrize("bot", [False, True], ids=["tcn", "tcnbot"])
def test_build_program_key_spellings_shortcut_and_refusals(bot):
    cfg = dict(in_channels=1, n_filters=16, kernel=3, dilation=3, n_layers=4, dropout=0.2, n_classes=2)
    a = T.build_tcn_program(_random_sd(cfg, bot, 9), types.SimpleNamespace(**cfg), bot)
    b = T.build_tcn_program(_random_sd(cfg, bot, 9, parametrization=True), types.SimpleNamespace(**cfg), bot)
    for x, y in zip(a[0], b[0]):
        for cx, cy in zip(x["convs"], y["convs"]):
            assert np.array_equal(cx["w"], cy["w"]) and np.array_equal(cx["b"], cy["b"])
    blocks = a[0]
    # the shortcut only where in_channels != n_filters (block 0: 1 -> 16), although the state dict has all of them
    assert blocks[0]["shortcut"] is not None and all(bl["shortcut"] is None for bl in blocks[1:])
    # the folded weight: g * v / ||v|| per output channel
    sd = _random_sd(cfg, bot, 9)
    v, g = sd["layers.1.blocks.1.0.weight_v"].astype(np.float64), sd["layers.1.blocks.1.0.weight_g"].astype(np.float64)
    want = g * v / np.sqrt((v ** 2).sum(axis=(1, 2), keepdims=True))
    assert np.abs(blocks[1]["convs"][1]["w"] - want).max() < 1e-6
    base = 2 if bot else 3
    assert [bl["dilation"] for bl in blocks] == [base ** i for i in range(4)]
    # receptive field = the reference's get_receptive_field (tcn.py:90-91, tcn_bot.py:91-92)
    assert T.receptive_field(blocks) == 1 + 2 * sum(base ** i * (cfg["kernel"] - 1) for i in range(cfg["n_layers"]))
    for bad in (dict(kernel=1), dict(in_channels=2), dict(n_classes=3)):
        c2 = dict(cfg, **bad)
        with pytest.raises(ValueError):
            T.build_tcn_program(_random_sd(c2, bot, 9), types.SimpleNamespace(**c2), bot)


def test_base_one_is_dense():
    cfg = dict(in_channels=1, n_filters=8, kernel=4, dilation=1, n_layers=3, dropout=0.0, n_classes=2)
    blocks, fw, fb = T.build_tcn_program(_random_sd(cfg, False, 5), types.SimpleNamespace(**cfg), False)
    x = _inputs(50)
    assert np.abs(cone_forward(blocks, fw, fb, x) - dense_forward(blocks, fw, fb, x)).max() < 1e-9


TCN_YAML = """model: tcn
batch_size: 32
n_epochs: 10
learning_rate: 0.0001

tcn:
  in_channels: 1
  n_filters: 24
  kernel: 3
  dilation: 2
  n_layers: 5
  dropout: 0.2
  n_classes: 2
"""


def _write_model_dir(tmp_path, golden_dir, name="tcn_k3_b2"):
    import torch
    g, cfg, sd = _load(golden_dir, name)
    d = tmp_path / "model"
    d.mkdir(exist_ok=True)
    (d / "mRNA_config_RNA004_RP4.yaml").write_text(TCN_YAML)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(d / "mRNA_model_RNA004_RP4.pth"))
    return str(d), cfg, sd


@pytest.mark.parametrize("parser", ["yaml", "flat"])
def test_modeldir_reads_a_tcn_config(tmp_path, golden_dir, monkeypatch, parser):
    import builtins
    from riser_amd import modeldir
    d, cfg, _ = _write_model_dir(tmp_path, golden_dir)
    if parser == "flat":                                    # the fallback parser, as on a host without PyYAML
        real = builtins.__import__

        def no_yaml(name, *a, **kw):
            if name == "yaml":
                raise ImportError(name)
            return real(name, *a, **kw)
        monkeypatch.setattr(builtins, "__import__", no_yaml)
    c = modeldir.get_config(os.path.join(d, "mRNA_config_RNA004_RP4.yaml"))
    assert c.model == "tcn" and not hasattr(c, "cnn")
    for k in ("in_channels", "n_filters", "kernel", "dilation", "n_layers", "dropout", "n_classes"):
        assert getattr(c.tcn, k) == cfg[k], k


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_model_matches_reference(golden_dir, name):
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, name)
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    assert m.dtype == "f32" and m.min_length == 1 and m._seq.receptive_field == cfg["rf"]
    for L in cfg["lengths"]:
        x = _inputs(L)
        wl, wp = g[f"{name}.L{L}.logits"], g[f"{name}.L{L}.probs"]
        probs, logits = m.classify_batch(x, return_logits=True)
        assert np.abs(logits.cpu().numpy() - wl).max() < 1e-4, L
        assert np.abs(probs.cpu().numpy() - wp).max() < 1e-4, L
        assert np.array_equal(probs.cpu().numpy().argmax(1), wp.argmax(1))
        import torch
        fb = m.forward_batch(torch.from_numpy(x).to(m.device), np.full(3, L, dtype=np.int32)).cpu().numpy()
        assert np.abs(fb - wp).max() < 1e-4
        for i in range(3):
            one = m.classify(x[i]).cpu().numpy()
            assert np.abs(one - wp[i]).max() < 1e-4
    m.close()


def ragged_lengths(rf):
    return [1, rf // 2, rf, rf + 1, 4097, 16000, 70000]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_ragged_batch_equals_every_read_alone(golden_dir, name):
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, name)
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    lens = ragged_lengths(cfg["rf"])
    sigs = [ro.mad_normalise(synth.make_signals(20260103, 1, n, first_read=500 + i)[0]).astype(np.float32)
            for i, n in enumerate(lens)]
    blocks, fw, fb = _program(cfg, sd)
    probs, logits = m.classify_batch(sigs, return_logits=True)
    probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
    for i, s in enumerate(sigs):
        p1, l1 = m.classify_batch([s], return_logits=True)
        assert np.array_equal(probs[i], p1.cpu().numpy()[0]), (i, lens[i])
        assert np.array_equal(logits[i], l1.cpu().numpy()[0]), (i, lens[i])
        assert np.array_equal(probs[i], m.classify(s).cpu().numpy()), (i, lens[i])
        want = cone_forward(blocks, fw, fb, s[None])[0]
        assert np.abs(logits[i] - want).max() < 1e-4, (i, lens[i])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tcn_k3_b2", "bot_k5"])
def test_only_the_last_receptive_field_matters(golden_dir, name):
    from riser_amd.model import Model
    g, cfg, sd = _load(golden_dir, name)
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    rf = cfg["rf"]
    a = _inputs(5000)[0]
    b = a.copy()
    b[: 5000 - rf] = np.random.default_rng(3).standard_normal(5000 - rf).astype(np.float32) * 3
    c = a.copy()
    c[-1] += 0.5                                             # inside the field: the result moves
    e = a.copy()
    e[5000 - rf] += 5.0                                      # the field's first sample: what the float64 forward says
    p = m.classify_batch(np.stack([a, b, c, e])).cpu().numpy()
    assert np.array_equal(p[0], p[1])
    assert not np.array_equal(p[0], p[2])
    blocks, fw, fb = _program(cfg, sd)
    assert np.abs(p[3] - ro.softmax(dense_forward(blocks, fw, fb, e[None]))[0]).max() < 1e-4
    # a shorter read with the same last RF samples
    assert np.array_equal(m.classify_batch([a[-rf - 10:]]).cpu().numpy()[0], p[0])
    m.close()


def _raw_reads(lens, first=700):
    return [synth.make_signals(20260103, 1, n, first_read=first + i)[0] for i, n in enumerate(lens)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tcn_k5_b3", "bot_k3"])
def test_classify_raw_normalises_the_whole_read(golden_dir, name):
    from riser_amd.model import Model
    from riser_amd.preprocess import pack_reads
    g, cfg, sd = _load(golden_dir, name)
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    blocks, fw, fb = _program(cfg, sd)
    sigs = _raw_reads([4096, 5000, 8615, 300, 12000])
    sig, off, ln, lh = pack_reads(sigs, m.device)
    probs = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    for i, s in enumerate(sigs):
        x = ro.mad_normalise(s).astype(np.float32)
        want = ro.softmax(dense_forward(blocks, fw, fb, x[None]))[0]
        assert np.abs(probs[i] - want).max() < 1e-4, i
    m.close()


@pytest.mark.gpu
def test_ensemble_of_two_tcns_decides_like_rs_decide(golden_dir):
    import torch
    from riser_amd import _native as nv
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    g1, c1, sd1 = _load(golden_dir, "tcn_k3_b2")
    g2, c2, sd2 = _load(golden_dir, "bot_k5")
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
    g, cfg, sd = _load(golden_dir, "tcn_k3_b2")
    m = Model(sd, _config(cfg), None, "mRNA", device=_dev())
    lens = [4097, 300, 16000, 125, 9000, 70, 12000]
    sigs = [ro.mad_normalise(s).astype(np.float32) for s in _raw_reads(lens, first=40)]
    whole = m.classify_batch(sigs).cpu().numpy()
    assert m.max_batch(16000) > len(sigs)
    monkeypatch.setattr(type(m._seq), "max_batch", lambda self, L: 3)
    split = m.classify_batch(sigs).cpu().numpy()
    assert np.array_equal(whole, split)
    for i, s in enumerate(sigs):
        assert np.array_equal(whole[i], m.classify_batch([s]).cpu().numpy()[0])
    m.close()


@pytest.mark.gpu
def test_get_models_and_sequencer_control_run_a_tcn(tmp_path, golden_dir):
    import logging
    import torch
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd import _native as nv
    from riser_amd.fake_client import FakeClient, FakeRead
    from riser_amd.modeldir import get_models
    d, cfg, sd = _write_model_dir(tmp_path, golden_dir)
    dev = _dev()
    (m,) = get_models(["mRNA"], logging.getLogger("t"), "RNA004", model_dir=d, device=dev)
    assert m._h is None and m._seq is not None and m._seq.receptive_field == cfg["rf"]
    rng = np.random.default_rng(12)
    batches = [[(ch, FakeRead(f"id-{b * 7 + ch}", synth.make_raw_read(56, b * 7 + ch, int(rng.integers(3000, 24000)),
                                                                      polya=((b * 7 + ch) % 4 != 0))))
                for ch in range(1, 25)] for b in range(2)]
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    out = str(tmp_path / "o")
    ctl = SequencerControl(FakeClient(batches), [m], proc, logging.getLogger("c"), out)
    ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
    lines = open(out + ".csv").read().strip().split("\n")
    header, rows = lines[0].split(","), [ln.split(",") for ln in lines[1:]]
    assert len(rows) > 10
    names = {"try_again": nv.RS_TRY_AGAIN, "accept": nv.RS_ACCEPT, "reject": nv.RS_REJECT, "no_decision": nv.RS_NO_DECISION}
    p1 = np.array([[float(v) for v in r[5].split(";")] for r in rows], dtype=np.float32)
    probs = torch.from_numpy(np.stack([1 - p1[:, 0], p1[:, 0]], axis=1)[None].copy()).to(dev)
    lens = torch.tensor([int(r[3]) for r in rows], dtype=torch.int32, device=dev)
    dec = torch.empty(len(rows), dtype=torch.uint8, device=dev)
    max_len = ro.kit_max_length("RNA004")
    nv.check(nv.lib().rs_decide(probs.data_ptr(), 1, len(rows), lens.data_ptr(), max_len, 0.9, nv.RS_ENRICH, dec.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    dec = dec.cpu().numpy()
    for r, dk in zip(rows, dec):
        q = float(r[5])
        if abs(q - 0.9) < 1e-4 or abs(1 - q - 0.9) < 1e-4:       # p_off is logged only as 1 - p_on
            continue
        assert names[r[8]] == dk, (r, header)
    m.close()
