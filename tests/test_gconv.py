"""The generic ConvNet family (csrc/gconv.hip) on the device, across the shape classes its planner branches on (the edge table
and its tags: tests/gconv_ref.py), against a float64 forward, and behind Model on the three golden variants.

Per config: one ragged batch of 77 reads in rows 64 samples longer than the longest read, NaN behind every read; logits held
to float64 within BARS[config] x max(1, |logit|), every read equal to its solo forward bit for bit; the same call on a
workspace of 0xFF bytes before and after a larger batch used it; batches of one; the batch reversed; the length contract (a
length beyond the pitch, below the minimum, negative).  Each case prints its GCONV_GAP and numpy-fp32's own gap to float64
on the same inputs before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import riser_oracle as ro
from riser_amd import gconv as G
from riser_amd import synth
from tests import gconv_ref as R

pytestmark = pytest.mark.gpu
SIG_SEED = 20260103
PAD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


_CASES = {}


def _case(name, dev):
    """program, net, the ragged batch and its float64 logits: made once per config and left unchanged"""
    if name not in _CASES:
        cfg = R.CONFIGS[name]
        prog = G.build_gconv_program(R.make_state_dict(cfg, R.SEED[name]), R.cnn_config(cfg))
        lens = R.edge_lengths(cfg, R.SEED[name])
        rng = np.random.default_rng(R.SEED[name] + 1)
        rows = np.full((len(lens), int(lens.max()) + PAD), np.nan, np.float32)
        for b, L in enumerate(lens):
            rows[b, :L] = rng.standard_normal(L).astype(np.float32)
        want = R.forward(prog, rows, lens)
        net = G.GConvNet(prog, device=dev)
        _CASES[name] = dict(cfg=cfg, prog=prog, lens=lens, rows=rows, want=want, net=net,
                            x=torch.from_numpy(rows).to(dev), ln=torch.from_numpy(lens).to(dev))
    return _CASES[name]


def _run(c, x=None, ln=None):
    probs, logits = c["net"].forward_ragged(c["x"] if x is None else x, c["ln"] if ln is None else ln, return_logits=True)
    return probs.cpu().numpy(), logits.cpu().numpy()


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_ragged_sweep_against_float64(dev, name):
    c = _case(name, dev)
    lens, rows, want = c["lens"], c["rows"], c["want"]
    plans = c["net"].layer_plans()
    assert [{k: p[k] for k in ("shape", "kc", "n_chunks", "vec")} for p in plans] == \
        [{k: R.plan_conv(*cv[:3])[k] for k in ("shape", "kc", "n_chunks", "vec")} for cv in R.convs_of(c["cfg"])]
    probs, logits = _run(c)
    f32 = R.gap(R.forward(c["prog"], rows, lens, dtype=np.float32), want)     # numpy-fp32's own gap on the same reads
    gap = R.gap(logits, want)
    print(f"GCONV_GAP {name} device {gap:.2e} numpy_fp32 {f32:.2e} bar {R.BARS[name]:.0e}")
    assert np.isfinite(logits).all()
    assert gap <= R.BARS[name], (name, gap)
    assert gap <= 10 * max(f32, R.BAR_FLOOR), (name, gap, f32)         # beyond that a gap is a defect, not round-off
    assert np.abs(probs - R.softmax(want)).max() < 1e-5
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


def _variant(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "convnet_variants.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
    config = synth.Config(synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"]))
    return cfg, sd, config, g[f"{name}.lens"], g[f"{name}.probs"]


@pytest.mark.parametrize("name", ["depth2_k5373", "depth1_k7", "depth3_k3"])
def test_model_runs_the_family(dev, golden_dir, name, monkeypatch):
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd.preprocess import pack_reads
    from riser_amd.resnet import SeqNet
    cfg, sd, config, glens, want = _variant(golden_dir, name)
    m = Model(sd, config, None, "x", device=dev)
    assert isinstance(m._seq, G.GConvNet) and m._seq.ragged_ok and m.dtype == "f32"
    sigs = [synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0] for j, L in enumerate(glens)]
    xs = [ro.mad_normalise(s) for s in sigs]
    rng = np.random.default_rng(5)
    lo = 1 << cfg["n_layers"]
    more = [rng.standard_normal(int(L)).astype(np.float32) for L in rng.integers(lo, 3000, size=77 - len(xs))]
    mixed = xs + more
    got = m.classify_batch(mixed).cpu().numpy()
    assert np.abs(got[: len(xs)] - want).max() < 1e-3
    assert np.array_equal(m.classify_batch(mixed[::-1]).cpu().numpy()[::-1], got)
    sig, off, ln, lh = pack_reads(sigs, dev)
    raw = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    assert np.abs(raw - want).max() < 1e-3
    m2 = Model(sd, config, None, "y", device=dev)
    dec = torch.zeros(len(sigs), dtype=torch.uint8, device=dev)
    ens = classify_raw_ensemble([m, m2], sig, off, ln, lh, decision=dec, max_len=4096, threshold=0.9).cpu().numpy()
    assert ens.shape == (2, len(sigs), 2) and np.array_equal(ens[0], raw) and np.array_equal(ens[1], raw)
    assert np.abs(ens[0] - want).max() < 1e-3 and set(dec.cpu().numpy().tolist()) <= {0, 1, 2, 3}
    m2.close()
    # the A/B hook: today's conv / max-pool program, within fp32 round-off of the new path
    monkeypatch.setenv("RS_GCONV", "0")
    old = Model(sd, config, None, "x", device=dev)
    monkeypatch.delenv("RS_GCONV")
    assert isinstance(old._seq, SeqNet) and not old._seq.ragged_ok
    assert np.abs(old.classify_batch(xs).cpu().numpy() - got[: len(xs)]).max() < 1e-5
    old.close()
    # a batch beyond max_batch is split and keeps its bits
    monkeypatch.setattr(G.GConvNet, "max_batch", lambda self, L: 3)
    assert np.array_equal(m.classify_batch(mixed).cpu().numpy(), got)
    m.close()
