"""The generic ConvNet family in bf16x3 (csrc/gconv_x3.hip, rs_gconv_set_mode(h, RS_BF16X3)) on the device, on the shapes of
tests/test_gconv.py: the edge table's 11 configs x 77 ragged reads in rows 64 samples longer than the longest read, NaN behind
every read.  Logits are held to float64 within X3_BARS[config] x max(1, |logit|) - bars that tests/gconv_x3_ref.py derives on
the CPU from an emulation of the arithmetic, never from a device run; every read keeps its solo bits; the same call on a
workspace of 0xFF bytes, in a doubled batch, reversed and in batches of one; the length contract; the switch to fp32 and back on
one handle; and the mode behind Model, get_models and SequencerControl on the three golden variants.

Without the mode `GConvNet(..., dtype="bf16x3")`, `Model(..., dtype="bf16x3")` on a generic config and rs_gconv_set_mode do not
exist: every test of this file fails on a tree that lacks it."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from oracle import riser_oracle as ro
from riser_amd import gconv as G
from riser_amd import synth
from tests import gconv_ref as R
from tests import gconv_x3_ref as X

pytestmark = pytest.mark.gpu
SIG_SEED = 20260103


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_CASES = {}


def _case(name, dev):
    """program, bf16x3 net, the ragged batch and its float64 logits: made once per config and left unchanged"""
    if name not in _CASES:
        cfg = R.CONFIGS[name]
        prog = G.build_gconv_program(R.make_state_dict(cfg, R.SEED[name]), R.cnn_config(cfg))
        lens, rows = X.edge_batch(name)
        want = R.forward(prog, rows, lens)
        net = G.GConvNet(prog, device=dev, dtype="bf16x3")
        assert net.dtype == "bf16x3"
        _CASES[name] = dict(cfg=cfg, prog=prog, lens=lens, rows=rows, want=want, net=net,
                            x=torch.from_numpy(rows).to(dev), ln=torch.from_numpy(lens).to(dev))
    return _CASES[name]


def _run(c, x=None, ln=None, net=None):
    probs, logits = (net or c["net"]).forward_ragged(c["x"] if x is None else x, c["ln"] if ln is None else ln,
                                                      return_logits=True)
    return probs.cpu().numpy(), logits.cpu().numpy()


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_ragged_sweep_against_float64(dev, name):
    c = _case(name, dev)
    lens, want, bar = c["lens"], c["want"], X.X3_BARS[name]
    probs, logits = _run(c)
    gap = R.gap(logits, want)
    print(f"GCONV_X3_GAP {name} device {gap:.2e} E64 {X.X3_E64[name]:.2e} E32 {X.X3_E32[name]:.2e} bar {bar:.0e}")
    assert np.isfinite(logits).all() and np.isfinite(probs).all()
    assert gap <= bar, (name, gap)
    assert np.abs(probs - R.softmax(want)).max() <= bar         # d softmax / d logit <= 1/4 in a two-class head
    # every read alone, at its own pitch: the same bits
    for b, L in enumerate(lens):
        one = c["net"].forward(c["x"][b: b + 1, : int(L)].contiguous(), return_logits=True)
        assert np.array_equal(one[1].cpu().numpy()[0], logits[b]) and np.array_equal(one[0].cpu().numpy()[0], probs[b]), (name, b, L)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_workspace_contents_and_batch_forms(dev, name):
    c = _case(name, dev)
    net, lens = c["net"], c["lens"]
    probs, logits = _run(c)
    net._ws.fill_(0xFF)                                             # NaN in every float of it
    p2, l2 = _run(c)
    assert np.array_equal(l2, logits) and np.array_equal(p2, probs)
    big = torch.cat([c["x"], c["x"]], dim=0)                        # a larger batch grows and dirties the workspace
    pb, lb = _run(c, big, torch.cat([c["ln"], c["ln"]]))
    assert np.array_equal(lb[: len(lens)], logits) and np.array_equal(lb[len(lens):], logits)
    net._ws.fill_(0xFF)
    p3, l3 = _run(c)
    assert np.array_equal(l3, logits)
    # the batch reversed, batches of one at the batch's pitch
    pr, lr = _run(c, torch.flip(c["x"], dims=[0]).contiguous(), torch.flip(c["ln"], dims=[0]).contiguous())
    assert np.array_equal(lr[::-1], logits) and np.array_equal(pr[::-1], probs)
    for b in (0, 1, len(lens) // 2, len(lens) - 1):
        p1, l1 = _run(c, c["x"][b: b + 1], c["ln"][b: b + 1])
        assert np.array_equal(l1[0], logits[b])


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_length_contract(dev, name):
    c = _case(name, dev)
    lens, ld = c["lens"].copy(), c["rows"].shape[1]
    lo = 1 << c["cfg"]["n_layers"]
    probs, logits = _run(c)
    x = torch.nan_to_num(c["x"], nan=0.25)                          # finite behind the reads: a length beyond them reads it
    base_p, base_l = _run(c, x)
    assert np.array_equal(base_l, logits)                           # what lies behind a read never mattered
    odd = lens.copy()
    odd[3], odd[4], odd[5], odd[40] = ld + 1000, lo - 1, -7, 0
    p, l = _run(c, x, torch.from_numpy(odd).to(dev))
    full = lens.copy()
    full[3] = ld
    pf, lf = _run(c, x, torch.from_numpy(full).to(dev))
    assert np.array_equal(l[3], lf[3]) and np.isfinite(l[3]).all()  # beyond the pitch: the bits of len = ld
    for b in (4, 5, 40):
        assert np.isnan(p[b]).all(), (name, b)
    keep = [b for b in range(len(lens)) if b not in (3, 4, 5, 40)]
    assert np.array_equal(l[keep], logits[keep]) and np.array_equal(p[keep], probs[keep])
    with pytest.raises(ValueError):
        c["net"].forward(c["x"][:2, : lo - 1].contiguous())


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_mode_switch_on_one_handle(dev, name):
    from riser_amd import _native as nv
    c = _case(name, dev)
    lib = nv.lib()
    fresh = G.GConvNet(c["prog"], device=dev)
    net = G.GConvNet(c["prog"], device=dev)
    assert fresh.dtype == net.dtype == "f32"
    pf, lf = _run(c, net=fresh)
    ws = [lib.rs_gconv_workspace_bytes(net._h, 77, 4160), lib.rs_gconv_max_batch(net._h, 4160)]
    net.set_mode("bf16x3")
    assert net.dtype == "bf16x3"
    assert ws == [lib.rs_gconv_workspace_bytes(net._h, 77, 4160), lib.rs_gconv_max_batch(net._h, 4160)]
    px, lx = _run(c, net=net)
    p0, l0 = _run(c)                                                # the handle that was created in bf16x3
    assert np.array_equal(lx, l0) and np.array_equal(px, p0)
    assert not np.array_equal(lx, lf) and R.gap(lx, lf) <= 2 * X.X3_BARS[name]       # the mode really switched
    for bad in (nv.RS_F16, nv.RS_BF16, nv.RS_F16X3, nv.RS_F16XF8, 77):
        assert lib.rs_gconv_set_mode(net._h, bad) == nv.RS_ERR_ARG and b"rs_gconv_set_mode" in lib.rs_last_error()
    with pytest.raises(ValueError):
        net.set_mode("f16x3")
    assert net.dtype == "bf16x3" and np.array_equal(_run(c, net=net)[1], lx)          # a refusal leaves the mode as it was
    for back in ("f32", "f32w"):
        net.set_mode(back)
        assert net.dtype == "f32"
        p1, l1 = _run(c, net=net)
        assert np.array_equal(l1, lf) and np.array_equal(p1, pf)                     # the bits of a fresh fp32 handle
        net.set_mode("bf16x3")
        p2, l2 = _run(c, net=net)
        assert np.array_equal(l2, lx) and np.array_equal(p2, px)                     # the bits of the first bf16x3 run
    assert net.layer_plans() == fresh.layer_plans()
    net.close()
    fresh.close()


def _variant(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "convnet_variants.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
    config = synth.Config(synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"]))
    return cfg, sd, config, g[f"{name}.lens"], g[f"{name}.probs"]


@pytest.mark.parametrize("name", ["depth2_k5373", "depth1_k7", "depth3_k3"])
def test_model_runs_the_family_in_bf16x3(dev, golden_dir, name, monkeypatch):
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    cfg, sd, config, glens, want = _variant(golden_dir, name)
    bar = X.VARIANT_BARS[name]
    m = Model(sd, config, None, "x", device=dev, dtype="bf16x3")
    assert isinstance(m._seq, G.GConvNet) and m._seq.ragged_ok and m.dtype == "bf16x3" and m._seq.dtype == "bf16x3"
    f32 = Model(sd, config, None, "x", device=dev)
    assert f32.dtype == "f32" and f32._seq.dtype == "f32"           # the default stays fp32
    sigs = [synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0] for j, L in enumerate(glens)]
    xs = [ro.mad_normalise(s) for s in sigs]
    one = np.stack([m.classify(x).cpu().numpy() for x in xs])
    rng = np.random.default_rng(5)
    lo = 1 << cfg["n_layers"]
    more = [rng.standard_normal(int(L)).astype(np.float32) for L in rng.integers(lo, 3000, size=77 - len(xs))]
    mixed = xs + more
    got = m.classify_batch(mixed).cpu().numpy()
    ref = f32.classify_batch(mixed).cpu().numpy()
    sig, off, ln, lh = pack_reads(sigs, dev)
    raw = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    gaps = [float(np.abs(v - want).max()) for v in (one, got[: len(xs)], raw)]
    print(f"GCONV_X3_MODEL {name} classify {gaps[0]:.2e} classify_batch {gaps[1]:.2e} classify_raw {gaps[2]:.2e} "
          f"E64 {X.VARIANT_GAPS[name]['E64']:.2e} E32 {X.VARIANT_GAPS[name]['E32']:.2e} bar {bar:.0e}")
    assert max(gaps) <= bar, (name, gaps)
    assert np.array_equal(one, got[: len(xs)])                      # a read alone and in a batch: the same bits
    assert not np.array_equal(got, ref) and np.abs(got - ref).max() < 1e-3
    assert np.array_equal(m.classify_batch(mixed[::-1]).cpu().numpy()[::-1], got)
    m2 = Model(sd, config, None, "y", device=dev, dtype="bf16x3")
    dec = torch.zeros(len(sigs), dtype=torch.uint8, device=dev)
    ens = classify_raw_ensemble([m, m2], sig, off, ln, lh, decision=dec, max_len=4096, threshold=0.9).cpu().numpy()
    assert ens.shape == (2, len(sigs), 2) and np.array_equal(ens[0], raw) and np.array_equal(ens[1], raw)
    assert set(dec.cpu().numpy().tolist()) <= {0, 1, 2, 3}
    m2.close()
    f32.close()
    # still refused: the f16-based and plain 16-bit modes; bf16x3 where the conv / max-pool program of seqnet.hip is kept
    for dt in ("f16", "bf16", "f16x3", "f16xf8"):
        with pytest.raises(ValueError):
            Model(sd, config, None, "x", device=dev, dtype=dt)
    for var, val in (("RS_GCONV", "0"), ("RS_SEQ_SCALAR", "1")):
        monkeypatch.setenv(var, val)
        with pytest.raises(ValueError):
            Model(sd, config, None, "x", device=dev, dtype="bf16x3")
        monkeypatch.delenv(var)
    # a batch beyond max_batch is split and keeps its bits
    monkeypatch.setattr(G.GConvNet, "max_batch", lambda self, L: 3)
    assert np.array_equal(m.classify_batch(mixed).cpu().numpy(), got)
    m.close()


def test_gap_head_refuses_bf16x3(dev, golden_dir):
    from test_oracle_golden import _gap_cases
    from riser_amd.model import Model
    tried = 0
    for _, cfg, sd, _, _ in _gap_cases(golden_dir):
        if cfg["depth"] == 1 and all(int(k) == 3 for k in cfg["kernels"]):
            continue
        config = synth.Config(synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"],
                                              classifier="gap"))
        with pytest.raises(ValueError):
            Model(sd, config, None, "x", dtype="bf16x3", device=dev)
        tried += 1
    assert tried >= 1


CNN_YAML = """model: cnn
batch_size: 32
n_epochs: 30
learning_rate: 0.0001

cnn:
  n_layers: 4
  depth: 2
  channels: [6,9,14,20]
  kernels: [5,3,7,3]
  n_classes: 2
  classifier: gap_fc # fc / gap_fc / gap
"""


def test_get_models_and_sequencer_control_in_bf16x3(dev, tmp_path, golden_dir):
    from riser_amd import Kit, SequencerControl, SignalProcessor
    from riser_amd.fake_client import FakeClient, FakeRead
    from riser_amd.modeldir import get_models
    from riser_amd.preprocess import pack_reads
    cfg, sd, config, glens, want = _variant(golden_dir, "depth2_k5373")
    assert cfg["channels"] == [6, 9, 14, 20] and cfg["kernels"] == [5, 3, 7, 3] and cfg["depth"] == 2
    d = tmp_path / "model"
    d.mkdir()
    (d / "mRNA_config_RNA004_RP4.yaml").write_text(CNN_YAML)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(d / "mRNA_model_RNA004_RP4.pth"))
    (m,) = get_models(["mRNA"], logging.getLogger("t"), "RNA004", model_dir=str(d), dtype="bf16x3", device=dev)
    assert m.dtype == "bf16x3" and isinstance(m._seq, G.GConvNet) and m._seq.dtype == "bf16x3"
    sigs = [synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0] for j, L in enumerate(glens)]
    sig, off, ln, lh = pack_reads(sigs, dev)
    assert np.abs(m.classify_raw(sig, off, ln, lh).cpu().numpy() - want).max() <= X.VARIANT_BARS["depth2_k5373"]
    rng = np.random.default_rng(12)
    batches = [[(ch, FakeRead(f"id-{b * 7 + ch}", synth.make_raw_read(56, b * 7 + ch, int(rng.integers(3000, 24000)),
                                                                      polya=((b * 7 + ch) % 4 != 0))))
                for ch in range(1, 25)] for b in range(2)]
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    out = str(tmp_path / "o")
    ctl = SequencerControl(FakeClient(batches), [m], proc, logging.getLogger("c"), out)
    ctl.start(); ctl.target("enrich", 0.5, 0.9); ctl.finish()
    rows = [ln_.split(",") for ln_ in open(out + ".csv").read().strip().split("\n")[1:]]
    assert len(rows) > 10 and all(np.isfinite(float(r[5])) for r in rows)
    m.close()
