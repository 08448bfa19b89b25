"""TCN and bottleneck TCN in bf16x3 split precision (rs_tcn_set_mode(h, RS_BF16X3), csrc/tcn_x3.hip): every conv of every
temporal block on the bf16 MFMA with hi = bf16(v), lo = bf16(v - hi) and hi*hi + lo*hi + hi*lo, fp32 accumulation.  A numpy
emulation of that arithmetic on the strided cone, pinned to the reference's golden logits on the CPU, sets the tolerances the
device is held to; on the GPU the mode runs through every entry point the fp32 TCN runs through."""
import json
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import synth
from riser_amd import tcn as T
from tests.tcn_ref import bf16, x3_cone_forward, x3_matmul

NAMES = ["tcn_k3_b2", "tcn_k5_b3", "bot_k3", "bot_k5"]

# the emulation misses the golden logits by 6.1e-5 at most over the four configs and all lengths (probabilities: 7e-6;
# test_emulated_split_cone_matches_reference); the device is held to over ten times that, for its own fp32 accumulation order
LOGIT_TOL = 1e-3
PROB_TOL = 1e-3


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "tcn.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
    return g, cfg, sd


def _ns(cfg):
    return types.SimpleNamespace(**{k: v for k, v in cfg.items() if k not in ("model", "rf", "lengths")})


def _program(cfg, sd):
    return T.build_tcn_program(sd, _ns(cfg), cfg["model"] == "tcn-bot")


def _config(cfg):
    key = "tcnbot" if cfg["model"] == "tcn-bot" else "tcn"
    return types.SimpleNamespace(model=cfg["model"], **{key: _ns(cfg)})


def _inputs(L):
    sigs = synth.make_signals(20260103, 3, L, first_read=60)
    return np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU
def test_set_mode_tile_plan_and_launch_plan_abi_without_a_gpu():
    import ctypes as C
    from riser_amd import _native as nv
    lib = nv.lib()
    assert lib.rs_version() == (2 << 16) | 9
    assert lib.rs_tcn_set_mode(None, nv.RS_BF16X3) == nv.RS_ERR_ARG
    assert b"rs_tcn_set_mode" in lib.rs_last_error()
    assert lib.rs_tcn_set_mode(None, nv.RS_F32) == nv.RS_ERR_ARG
    # ABI 2.8: the tile-plan query refuses a null handle and leaves its outputs alone
    t, nb, tiles = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    assert lib.rs_tcn_tile_plan(None, 0, 1, 1, C.byref(t), C.byref(nb), C.byref(tiles)) == nv.RS_ERR_ARG
    assert b"rs_tcn_tile_plan" in lib.rs_last_error()
    assert (t.value, nb.value, tiles.value) == (-7, -7, -7)
    # ABI 2.9: the conv program's launch-plan query refuses a null model, B < 1, an empty length and a NULL count (the
    # length below a program's minimum is refused on the GPU, tests/test_resnet_shapes.py)
    n = C.c_int32(-7)
    for args in ((None, 1, 4000, 0, None, 0, C.byref(n)), (None, 0, 4000, 0, None, 0, C.byref(n)),
                 (None, 1, 0, 1, None, 0, C.byref(n)), (None, 1, 4000, 0, None, 0, None)):
        assert lib.rs_seqnet_launch_plan(*args) == nv.RS_ERR_ARG
        assert b"rs_seqnet_launch_plan" in lib.rs_last_error()
    assert n.value == -7


@pytest.mark.parametrize("name", NAMES)
def test_emulated_split_cone_matches_reference(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    blocks, fw, fb = _program(cfg, sd)
    worst = 0.0
    for L in cfg["lengths"]:
        want = g[f"{name}.L{L}.logits"]
        lg = x3_cone_forward(blocks, fw, fb, _inputs(L))
        err = np.abs(lg - want).max()
        worst = max(worst, err)
        assert err < 1e-4, (L, err)
        assert np.array_equal(lg.argmax(1), want.argmax(1)), L
        assert np.abs(ro.softmax(lg) - g[f"{name}.L{L}.probs"]).max() < 5e-5, L
    assert worst > 0.0                     # it is another arithmetic than the reference's
    assert 10 * worst < LOGIT_TOL          # the device tolerance sits well above what the arithmetic itself costs


def test_emulated_split_is_not_plain_bf16():
    """the lo halves matter: the split product is two orders of magnitude closer to the exact one than a plain bf16 product"""
    rng = np.random.default_rng(1)
    a = rng.standard_normal((64, 96)).astype(np.float32)
    w = rng.standard_normal((96, 32)).astype(np.float32)
    exact = a.astype(np.float64) @ w.astype(np.float64)
    e3 = np.abs(x3_matmul(a, w) - exact).max()
    e1 = np.abs(bf16(a).astype(np.float64) @ bf16(w).astype(np.float64) - exact).max()
    assert e3 < 1e-2 * e1 and e3 < 1e-3


def _small_tcn():
    cfg = dict(in_channels=1, n_filters=8, kernel=3, dilation=2, n_layers=2, dropout=0.0, n_classes=2)
    return synth.make_tcn_state_dict(3, cfg, False), types.SimpleNamespace(model="tcn", tcn=types.SimpleNamespace(**cfg))


@pytest.mark.parametrize("dtype", ["f16x3", "f16xf8", "f16", "bf16"])
def test_half_and_plain_bf16_tcn_nets_are_refused(dtype):
    sd, config = _small_tcn()
    with pytest.raises(ValueError, match="bf16x3"):
        T.TCNNet(*T.build_tcn_program(sd, config.tcn, False), device=None, dtype=dtype)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _model(sd, config, dtype="bf16x3", target="mRNA"):
    from riser_amd.model import Model
    return Model(sd, config, None, target, dtype=dtype, device=_dev())


def _raw_reads(lens, first=700):
    return [synth.make_signals(20260103, 1, n, first_read=first + i)[0] for i, n in enumerate(lens)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16x3", "f16xf8", "f16", "bf16"])
def test_half_and_plain_bf16_tcn_models_are_refused(dtype):
    from riser_amd.model import Model
    sd, config = _small_tcn()
    with pytest.raises(ValueError, match="bf16x3"):
        Model(sd, config, None, "x", dtype=dtype, device=_dev())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_model_bf16x3_matches_reference(golden_dir, name):
    import torch
    g, cfg, sd = _load(golden_dir, name)
    m = _model(sd, _config(cfg))
    assert m.dtype == "bf16x3" and m._seq.dtype == "bf16x3" and m._seq.receptive_field == cfg["rf"]
    blocks, fw, fb = _program(cfg, sd)
    for L in cfg["lengths"]:
        x = _inputs(L)
        wl, wp = g[f"{name}.L{L}.logits"], g[f"{name}.L{L}.probs"]
        probs, logits = m.classify_batch(x, return_logits=True)
        probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
        assert np.abs(logits - wl).max() < LOGIT_TOL, L
        assert np.abs(probs - wp).max() < PROB_TOL, L
        assert np.array_equal(probs.argmax(1), wp.argmax(1)), L
        # the device and the emulation of the same arithmetic agree far more closely than either with the reference needs
        assert np.abs(logits - x3_cone_forward(blocks, fw, fb, x)).max() < LOGIT_TOL, L
        fb_ = m.forward_batch(torch.from_numpy(x).to(m.device), np.full(3, L, dtype=np.int32)).cpu().numpy()
        assert np.array_equal(fb_, probs)
        for i in range(3):
            assert np.array_equal(m.classify(x[i]).cpu().numpy(), probs[i])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_bf16x3_is_another_arithmetic_than_fp32(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    m3, m1 = _model(sd, _config(cfg)), _model(sd, _config(cfg), dtype="f32")
    assert m1.dtype == "f32"
    x = _inputs(4097)
    _, l3 = m3.classify_batch(x, return_logits=True)
    _, l1 = m1.classify_batch(x, return_logits=True)
    diff = np.abs(l3.cpu().numpy() - l1.cpu().numpy()).max()
    assert 0.0 < diff < LOGIT_TOL, diff
    m3.close()
    m1.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_ragged_batch_equals_every_read_alone(golden_dir, name):
    import torch
    g, cfg, sd = _load(golden_dir, name)
    m = _model(sd, _config(cfg))
    rf = cfg["rf"]
    lens = [1, rf // 2, rf, rf + 1, 4097, 16000]
    sigs = [ro.mad_normalise(synth.make_signals(20260103, 1, n, first_read=500 + i)[0]).astype(np.float32)
            for i, n in enumerate(lens)]
    probs, logits = m.classify_batch(sigs, return_logits=True)
    for i, s in enumerate(sigs):
        p1, l1 = m.classify_batch([s], return_logits=True)
        assert torch.equal(probs[i], p1[0]), (i, lens[i])
        assert torch.equal(logits[i], l1[0]), (i, lens[i])
        assert torch.equal(probs[i], m.classify(s)), (i, lens[i])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tcn_k3_b2", "bot_k5"])
def test_only_the_last_receptive_field_matters(golden_dir, name):
    g, cfg, sd = _load(golden_dir, name)
    m = _model(sd, _config(cfg))
    rf = cfg["rf"]
    a = _inputs(5000)[0]
    b = a.copy()
    b[: 5000 - rf] = np.random.default_rng(3).standard_normal(5000 - rf).astype(np.float32) * 3
    c = a.copy()
    c[-1] += 0.5                                             # inside the field: the result moves
    p = m.classify_batch(np.stack([a, b, c])).cpu().numpy()
    assert np.array_equal(p[0], p[1])
    assert not np.array_equal(p[0], p[2])
    assert np.array_equal(m.classify_batch([a[-rf - 10:]]).cpu().numpy()[0], p[0])
    m.close()


def _bench_models(bot):
    cfg = dict(synth.TCN_BENCH_CFG)
    sd = synth.make_tcn_state_dict(11, cfg, bot)
    config = types.SimpleNamespace(model="tcn-bot" if bot else "tcn", **{"tcnbot" if bot else "tcn": types.SimpleNamespace(**cfg)})
    return _model(sd, config), _model(sd, config, dtype="f32")


@pytest.mark.gpu
@pytest.mark.parametrize("bot", [False, True])
def test_bench_size_nets_against_fp32(bot):
    from riser_amd.preprocess import pack_reads
    m3, m1 = _bench_models(bot)
    sigs = [synth.make_signals(20260103, 1, 16000, first_read=3000 + i)[0] for i in range(512)]
    sig, off, ln, lh = pack_reads(sigs, m3.device)
    p3 = m3.classify_raw(sig, off, ln, lh).cpu().numpy()
    p1 = m1.classify_raw(sig, off, ln, lh).cpu().numpy()
    assert np.abs(p3 - p1).max() <= 1e-3
    sure = np.abs(p1[:, 1] - 0.5) > 1e-3
    assert sure.sum() > 400
    assert np.array_equal(p3[sure].argmax(1), p1[sure].argmax(1))
    m3.close()
    m1.close()


@pytest.mark.gpu
def test_ensemble_of_bf16x3_tcn_tcnbot_and_convnet_decides_like_rs_decide(golden_dir):
    import torch
    from riser_amd import _native as nv
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    g1, c1, sd1 = _load(golden_dir, "tcn_k3_b2")
    g2, c2, sd2 = _load(golden_dir, "bot_k5")
    dev = _dev()
    models = [_model(sd1, _config(c1), target="a"), _model(sd2, _config(c2), target="b"),
              Model(synth.make_state_dict(7), synth.Config(), None, "c", dtype="bf16x3", device=dev)]
    assert [m.dtype for m in models] == ["bf16x3"] * 3
    sigs = _raw_reads([4096, 5000, 8615, 4500, 12000, 16000, 6025], first=900)      # the ConvNet takes 4096 samples or more
    sig, off, ln, lh = pack_reads(sigs, dev)
    dec = torch.empty(len(sigs), dtype=torch.uint8, device=dev)
    probs = classify_raw_ensemble(models, sig, off, ln, lh, decision=dec, max_len=12000, threshold=0.6)
    for k, m in enumerate(models):
        assert torch.equal(probs[k], m.classify_raw(sig, off, ln, lh)), k
    want = torch.empty_like(dec)
    p2 = probs.contiguous()
    nv.check(nv.lib().rs_decide(p2.data_ptr(), len(models), len(sigs), ln.data_ptr(), 12000, 0.6, nv.RS_ENRICH,
                                want.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    assert torch.equal(dec, want)
    for m in models:
        m.close()


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


@pytest.mark.gpu
def test_get_models_and_sequencer_control_in_bf16x3(tmp_path, golden_dir):
    import logging
    import torch
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd import _native as nv
    from riser_amd.fake_client import FakeClient, FakeRead
    from riser_amd.modeldir import get_models
    from riser_amd.preprocess import pack_reads
    g, cfg, sd = _load(golden_dir, "tcn_k3_b2")
    d = tmp_path / "model"
    d.mkdir()
    (d / "mRNA_config_RNA004_RP4.yaml").write_text(TCN_YAML)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(d / "mRNA_model_RNA004_RP4.pth"))
    dev = _dev()
    (m,) = get_models(["mRNA"], logging.getLogger("t"), "RNA004", model_dir=str(d), dtype="bf16x3", device=dev)
    assert m.dtype == "bf16x3" and m._seq.dtype == "bf16x3" and m._seq.receptive_field == cfg["rf"]
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
    # the CSV's probabilities are those of direct classify_raw calls on the same signals: a row shorter than the kit's
    # maximum is the read from behind its poly(A) tail to its end (column 3: the samples assessed)
    max_len = proc.get_max_length()
    raw = {(r.id, ch): np.frombuffer(r.raw_data, dtype=np.int16) for bt in batches for ch, r in bt}   # ids repeat across batches
    short = [r for r in rows if int(r[3]) < max_len]
    assert len(short) > 5
    sig, off, ln, lh = pack_reads([raw[(r[1], int(r[2]))][-int(r[3]):] for r in short], dev)
    direct = m.classify_raw(sig, off, ln, lh).cpu().numpy()[:, 1]
    assert np.abs(direct - np.array([float(r[5]) for r in short])).max() <= 1e-6
    names = {"try_again": nv.RS_TRY_AGAIN, "accept": nv.RS_ACCEPT, "reject": nv.RS_REJECT, "no_decision": nv.RS_NO_DECISION}
    p1 = np.array([[float(v) for v in r[5].split(";")] for r in rows], dtype=np.float32)
    probs = torch.from_numpy(np.stack([1 - p1[:, 0], p1[:, 0]], axis=1)[None].copy()).to(dev)
    lens = torch.tensor([int(r[3]) for r in rows], dtype=torch.int32, device=dev)
    dec = torch.empty(len(rows), dtype=torch.uint8, device=dev)
    nv.check(nv.lib().rs_decide(probs.data_ptr(), 1, len(rows), lens.data_ptr(), max_len, 0.9, nv.RS_ENRICH, dec.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream), "rs_decide")
    dec = dec.cpu().numpy()
    for r, dk in zip(rows, dec):
        q = float(r[5])
        if abs(q - 0.9) < 1e-4 or abs(1 - q - 0.9) < 1e-4:
            continue
        assert names[r[8]] == dk, (r, header)
    m.close()


@pytest.mark.gpu
def test_batch_beyond_max_batch_is_split(golden_dir, monkeypatch):
    g, cfg, sd = _load(golden_dir, "tcn_k3_b2")
    m = _model(sd, _config(cfg))
    lens = [4097, 300, 16000, 125, 9000, 70, 12000]
    sigs = [ro.mad_normalise(s).astype(np.float32) for s in _raw_reads(lens, first=40)]
    whole = m.classify_batch(sigs).cpu().numpy()
    assert m.max_batch(16000) > len(sigs)
    monkeypatch.setattr(type(m._seq), "max_batch", lambda self, L: 3)
    split_ = m.classify_batch(sigs).cpu().numpy()
    assert np.array_equal(whole, split_)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tcn_k5_b3", "bot_k3"])
def test_mode_switch_leaves_no_residue(golden_dir, name):
    import torch
    from riser_amd import _native as nv
    g, cfg, sd = _load(golden_dir, name)
    blocks, fw, fb = _program(cfg, sd)
    dev = _dev()
    fresh = T.TCNNet(blocks, fw, fb, device=dev, dtype="f32")
    h = T.TCNNet(blocks, fw, fb, device=dev, dtype="f32")
    lens = [1, 300, 4097, 12000]
    x = torch.zeros((len(lens), 12000), dtype=torch.float32, device=dev)
    for i, n in enumerate(lens):
        x[i, :n] = torch.from_numpy(_inputs(n)[0])
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    want = fresh.forward_ragged(x, ln).clone()
    lib = nv.lib()
    w0 = lib.rs_tcn_workspace_bytes(h._h, len(lens), 12000)
    mb0 = lib.rs_tcn_max_batch(h._h, 12000)
    nv.check(lib.rs_tcn_set_mode(h._h, nv.RS_BF16X3), "rs_tcn_set_mode")
    x3 = h.forward_ragged(x, ln).clone()
    assert not torch.equal(x3, want)
    # the active mode's needs (the same buffers in both modes)
    assert lib.rs_tcn_workspace_bytes(h._h, len(lens), 12000) == w0 and lib.rs_tcn_max_batch(h._h, 12000) == mb0
    for bad in (nv.RS_F16, nv.RS_BF16, nv.RS_F16X3, nv.RS_F16XF8, 99):
        assert lib.rs_tcn_set_mode(h._h, bad) == nv.RS_ERR_ARG
    assert torch.equal(h.forward_ragged(x, ln), x3)           # a refused switch keeps the mode
    nv.check(lib.rs_tcn_set_mode(h._h, nv.RS_F32), "rs_tcn_set_mode")
    assert torch.equal(h.forward_ragged(x, ln), want)
    nv.check(lib.rs_tcn_set_mode(h._h, nv.RS_BF16X3), "rs_tcn_set_mode")
    nv.check(lib.rs_tcn_set_mode(h._h, nv.RS_F32W), "rs_tcn_set_mode")
    assert torch.equal(h.forward_ragged(x, ln), want)
    fresh.close()
    h.close()
