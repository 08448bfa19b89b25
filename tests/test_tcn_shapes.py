"""TCN and TCNBot across every tile regime of the device program, in both modes, against float64.

The shared host side of csrc/tcn.hip - the windows, the tile planner, the workspace layout and the head - is the same for
fp32 and bf16x3, so comparing the two modes cannot see a bug there.  Here each config runs one ragged batch of 77 reads
(lengths 1 ... 16000 around its receptive field, a row pitch longer than the longest read) in each mode and is held to:
  fp32    the float64 dense forward (tcn_ref.dense_forward), logits and probabilities within 1e-4;
  bf16x3  the numpy emulation of its arithmetic (tcn_ref.x3_cone_forward) within X3_DEV_TOL[config], float64 within 1e-3;
  both    every read's bits equal to those it gets alone; rs_tcn_tile_plan equal to the planner mirror
          (tcn_ref.tile_regimes), and across the sweep every regime of the planner reached in each mode.
The edge configs are pinned to the reference's own logits (tests/golden/tcn_edges.npz) on the CPU, and every mutant of
tcn_ref must miss the correct logits by more than ten times the tolerance its config is held to, so the tolerances can
catch those bugs."""
import json
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import synth
from riser_amd import tcn as T
from tests import tcn_ref as R

EDGES = ["tcn_f1_k2", "tcn_k5_l1", "tcn_k2_b4", "tcn_f68", "bot_f4", "bot_f22_k2"]
SYNTH = {
    # name: (bottleneck, n_filters, kernel, dilation, n_layers); regimes at the sweep's batch (77 reads, pitch LD)
    "tcn_f100": (False, 100, 3, 2, 6),               # np 112: a partial second column group; T cut by LDS in block 1
    "tcn_f128_k7": (False, 128, 7, 2, 4),            # T cut in blocks 0-1
    "tcn_f48_k9_b1": (False, 48, 9, 1, 3),           # base 1: no subsample
    "tcn_f8_d40": (False, 8, 3, 40, 9),              # dilations past every read and past 2^40
    "bot_f256_k5": (True, 256, 5, 2, 6),             # T 16-17; four column groups in the closing 1x1
    "bench_tcn": (False,) + tuple(synth.TCN_BENCH_CFG[k] for k in ("n_filters", "kernel", "dilation", "n_layers")),
    "bench_bot": (True,) + tuple(synth.TCN_BENCH_CFG[k] for k in ("n_filters", "kernel", "dilation", "n_layers")),
}
NAMES = EDGES + list(SYNTH)
MODES = ["f32", "bf16x3"]

N_READS = 77
MAX_LEN = 16000
LD = MAX_LEN + 123                                   # the row pitch: longer than the longest read

F32_TOL = 1e-4                                       # fp32 device against float64: logits and probabilities
X3_F64_TOL = 1e-3                                    # bf16x3 device against float64
# bf16x3 device against the emulation of its arithmetic, per config: about 4x the largest gap measured on an MI355X over the
# sweep's 77 reads (and the bench nets' 512 raw reads), rounded up, at least 1e-5.  The gap is fp32 accumulation order
# against float64 and grows with the logits' scale: 3.2e-8 (one filter) ... 9.2e-5 (tcn_k2_b4, logits near 10).
X3_DEV_TOL = {
    "tcn_f1_k2": 1e-5, "tcn_k5_l1": 1e-5, "tcn_k2_b4": 4e-4, "tcn_f68": 2e-5, "bot_f4": 1e-5, "bot_f22_k2": 5e-5,
    "tcn_f100": 2e-4, "tcn_f128_k7": 8e-5, "tcn_f48_k9_b1": 3e-5, "tcn_f8_d40": 2e-5, "bot_f256_k5": 2e-4,
    "bench_tcn": 3e-4, "bench_bot": 2e-4,
}


def _edge(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "tcn_edges.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
    return g, cfg, sd


def _cfg_sd(name):
    """(config dict, bottleneck, state dict) of a sweep config"""
    if name in SYNTH:
        bot, nf, k, dil, nl = SYNTH[name]
        cfg = dict(in_channels=1, n_filters=nf, kernel=k, dilation=dil, n_layers=nl, dropout=0.2, n_classes=2)
        return cfg, bot, synth.make_tcn_state_dict(11 if name.startswith("bench") else 29, cfg, bot)
    g, cfg, sd = _edge(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), name)
    return {k: v for k, v in cfg.items() if k not in ("model", "rf", "lengths")}, cfg["model"] == "tcn-bot", sd


_PROGRAMS = {}


def program(name):
    if name not in _PROGRAMS:
        cfg, bot, sd = _cfg_sd(name)
        blocks, fw, fb = T.build_tcn_program(sd, types.SimpleNamespace(**cfg), bot)
        _PROGRAMS[name] = (cfg, bot, sd, blocks, fw, fb)
    return _PROGRAMS[name]


def sweep_lengths(name):
    """1, 2, k-1, RF//2, RF-1, RF, RF+1, 4097, 16000 (capped at 16000) and seeded random lengths in between: 77 reads"""
    cfg, _, _, blocks, _, _ = program(name)
    rf = T.receptive_field(blocks)
    fixed = [1, 2, cfg["kernel"] - 1, rf // 2, rf - 1, rf, rf + 1, 4097, MAX_LEN]
    fixed = [int(min(max(v, 1), MAX_LEN)) for v in fixed]
    rng = np.random.default_rng(sum(map(ord, name)))
    rest = rng.integers(1, MAX_LEN + 1, N_READS - len(fixed)).tolist()
    return fixed + [int(v) for v in rest]


_SIGNALS = []


def reads(name):
    """the sweep's reads: read i is the last n_i samples of a normalised synthetic read of 16000 samples"""
    if not _SIGNALS:
        for i in range(N_READS):
            s = synth.make_signals(20260103, 1, MAX_LEN, first_read=6100 + i)[0]
            _SIGNALS.append(ro.mad_normalise(s).astype(np.float32))
    return [_SIGNALS[i][MAX_LEN - n:] for i, n in enumerate(sweep_lengths(name))]


_REF = {}


def reference(name):
    """float64 logits of every read (the dense forward on the read's last receptive field, dilations clamped to the read's
    length) and the emulated bf16x3 logits (the strided cone at the sweep's pitch)"""
    if name not in _REF:
        _, _, _, blocks, fw, fb = program(name)
        rf = T.receptive_field(blocks)
        f64, x3 = [], []
        for s in reads(name):
            tail = s[-min(len(s), rf):]
            f64.append(R.dense_forward(blocks, fw, fb, tail[None], clamp_len=len(tail))[0])
            x3.append(R.x3_cone_forward(blocks, fw, fb, s[None], ld=LD)[0])
        _REF[name] = (np.array(f64), np.array(x3))
    return _REF[name]


def regimes(name, mode):
    """the planner regimes a config reaches in a mode at the sweep's batch"""
    _, _, _, blocks, _, _ = program(name)
    plan = R.tile_regimes(blocks, N_READS, LD, mode)
    got = set()
    for out_rows, t, nb, tiles in plan:
        if t < min(out_rows, 64):
            got.add("lds_cut_T")
        if tiles > 1 and out_rows % t:
            got.add("partial_position_tile")
        if nb > 1 and N_READS % nb:
            got.add("partial_read_tile")
    if any(cv["w"].shape[0] > 64 for b in blocks for cv in b["convs"]):
        got.add("column_groups")
    if blocks[0]["shortcut"] is None:
        got.add("identity_block0")
    return got


ALL_REGIMES = {"lds_cut_T", "partial_position_tile", "partial_read_tile", "column_groups", "identity_block0"}


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", EDGES)
def test_edge_configs_match_the_reference(golden_dir, name):
    """the float64 forwards, the emulation and the program builder pinned to the reference's own TCN / TCNBot at the edges"""
    g, cfg, sd = _edge(golden_dir, name)
    blocks, fw, fb = program(name)[3:]
    assert T.receptive_field(blocks) == cfg["rf"]
    for L in cfg["lengths"]:
        sigs = synth.make_signals(20260103, 3, L, first_read=60)
        x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
        want = g[f"{name}.L{L}.logits"]
        assert np.abs(R.dense_forward(blocks, fw, fb, x) - want).max() < 1e-5, L
        assert np.abs(R.cone_forward(blocks, fw, fb, x) - want).max() < 1e-5, L
        assert np.abs(R.x3_cone_forward(blocks, fw, fb, x) - want).max() < 1e-4, L


def test_clamped_dense_forward_is_exact():
    cfg = dict(in_channels=1, n_filters=6, kernel=3, dilation=40, n_layers=3, dropout=0.0, n_classes=2)
    blocks, fw, fb = T.build_tcn_program(synth.make_tcn_state_dict(3, cfg), types.SimpleNamespace(**cfg), False)
    sig = reads("tcn_f8_d40")[-1]
    for L in (1, 39, 40, 41, 300, 1601):              # dilations 1, 40, 1600: below, at and past the read's length
        s = sig[-L:][None]
        full = R.dense_forward(blocks, fw, fb, s)
        assert np.abs(R.dense_forward(blocks, fw, fb, s, clamp_len=L) - full).max() < 1e-12, L
        assert np.abs(R.cone_forward(blocks, fw, fb, s) - full).max() < 1e-9, L


def test_sweep_reaches_every_planner_regime_in_both_modes():
    for mode in MODES:
        got = set().union(*(regimes(n, mode) for n in NAMES))
        assert got == ALL_REGIMES, (mode, ALL_REGIMES - got)
    # the cut the LDS budget makes at 64 filters, as measured on the bench nets
    blocks = program("bench_tcn")[3]
    assert [p[1] for p in R.tile_regimes(blocks, 512, 16000, "f32")][1:4] == [59, 59, 59]
    assert [p[1] for p in R.tile_regimes(blocks, 512, 16000, "bf16x3")][1:4] == [55, 55, 55]


# mutants that are the identity on a config (the split-precision mutants are caught on every config, 1 filter included)
EXEMPT = {
    ("tcn_f48_k9_b1", "unstrided_residual"): "base 1: row q is row q * base",
    ("tcn_f1_k2", "unstrided_residual"): "base 1: row q is row q * base",
    ("tcn_k5_l1", "unstrided_residual"): "one block: its one output row is row 0",
}


@pytest.mark.parametrize("name", NAMES)
def test_mutants_are_caught_at_the_sweep_tolerances(name):
    """every mutant of tcn_ref moves some logit of the sweep's batch by more than 10x the tolerance the config is held to"""
    _, _, _, blocks, fw, fb = program(name)
    sigs = reads(name)
    # a read of every length class; the random ones add nothing a mutant needs
    sel = sigs[:9] + sigs[9:14]
    base64 = [R.cone_forward(blocks, fw, fb, s[None], ld=LD)[0] for s in sel]
    base3 = [R.x3_cone_forward(blocks, fw, fb, s[None], ld=LD)[0] for s in sel]
    for mutant in R.X3_MUTANTS:
        if (name, mutant) in EXEMPT:
            continue
        if mutant in R.MUTANTS:
            got = [R.cone_forward(blocks, fw, fb, s[None], ld=LD, mutant=mutant)[0] for s in sel]
            miss = np.abs(np.array(got) - np.array(base64)).max()
            assert miss > 10 * F32_TOL, (mutant, "f32", miss)
        got = [R.x3_cone_forward(blocks, fw, fb, s[None], ld=LD, mutant=mutant)[0] for s in sel]
        miss = np.abs(np.array(got) - np.array(base3)).max()
        assert miss > 10 * X3_DEV_TOL[name], (mutant, "bf16x3", miss)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _model(name, mode):
    from riser_amd.model import Model
    cfg, bot, sd = program(name)[:3]
    config = types.SimpleNamespace(model="tcn-bot" if bot else "tcn",
                                   **{"tcnbot" if bot else "tcn": types.SimpleNamespace(**cfg)})
    return Model(sd, config, None, "t", dtype=mode, device=_dev())


def _tile_plan(net, block, B, ld):
    import ctypes as C
    from riser_amd import _native as nv
    t, nb, tiles = C.c_int(), C.c_int(), C.c_int()
    nv.check(nv.lib().rs_tcn_tile_plan(net._h, block, B, ld, C.byref(t), C.byref(nb), C.byref(tiles)), "rs_tcn_tile_plan")
    return t.value, nb.value, tiles.value


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_sweep(name, mode):
    import torch
    m = _model(name, mode)
    net = m._seq
    assert net.dtype == mode
    _, _, _, blocks, fw, fb = program(name)
    # the receptive field is the exact integer, dilations past 2^40 included
    assert net.receptive_field == T.receptive_field(blocks)
    # the planner the forward runs is the mirror's, block by block
    for i, (out_rows, t, nb, tiles) in enumerate(R.tile_regimes(blocks, N_READS, LD, mode)):
        assert _tile_plan(net, i, N_READS, LD) == (t, nb, tiles), (i, out_rows)
    sigs = reads(name)
    lens = [len(s) for s in sigs]
    x = torch.zeros((N_READS, LD), dtype=torch.float32)
    for i, s in enumerate(sigs):
        x[i, :len(s)] = torch.from_numpy(s)
    ln = torch.tensor(lens, dtype=torch.int32, device=m.device)
    probs, logits = net.forward_ragged(x.to(m.device), ln, return_logits=True)
    probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
    f64, emu = reference(name)
    p64 = ro.softmax(f64)
    d64, dp64 = np.abs(logits - f64).max(), np.abs(probs - p64).max()
    if mode == "f32":
        assert d64 < F32_TOL and dp64 < F32_TOL, (d64, dp64)
        sure = np.abs(p64[:, 1] - 0.5) > 1e-3
        assert np.array_equal(probs[sure].argmax(1), p64[sure].argmax(1))
        print(f"\nSWEEP {name} f32 max|dev-f64| logits {d64:.3e} probs {dp64:.3e}")
    else:
        demu = np.abs(logits - emu).max()
        print(f"\nSWEEP {name} bf16x3 max|dev-emu| logits {demu:.3e}; max|dev-f64| logits {d64:.3e} probs {dp64:.3e}")
        assert demu < X3_DEV_TOL[name], demu
        assert d64 < X3_F64_TOL and dp64 < X3_F64_TOL, (d64, dp64)
    if name != "tcn_f1_k2":                          # one filter: a read of every length sits near the same logits
        assert logits[:, 1].std() >= 0.05, logits[:, 1].std()
    # every read alone, bit for bit
    for i, s in enumerate(sigs):
        p1, l1 = m.classify_batch([s], return_logits=True)
        assert np.array_equal(p1.cpu().numpy()[0], probs[i]), (i, lens[i])
        assert np.array_equal(l1.cpu().numpy()[0], logits[i]), (i, lens[i])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bot", [False, True], ids=["tcn", "tcnbot"])
def test_bench_nets_on_512_raw_reads_against_the_cone(bot, mode):
    from riser_amd.preprocess import pack_reads
    name = "bench_bot" if bot else "bench_tcn"
    m = _model(name, mode)
    _, _, _, blocks, fw, fb = program(name)
    raw = [synth.make_signals(20260103, 1, MAX_LEN, first_read=3000 + i)[0] for i in range(512)]
    sig, off, ln, lh = pack_reads(raw, m.device)
    probs = m.classify_raw(sig, off, ln, lh).cpu().numpy()
    x = np.stack([ro.mad_normalise(s) for s in raw]).astype(np.float32)
    p64 = ro.softmax(R.cone_forward(blocks, fw, fb, x))
    dp = np.abs(probs - p64).max()
    if mode == "f32":
        assert dp < F32_TOL, dp
        sure = np.abs(p64[:, 1] - 0.5) > 1e-3
        assert np.array_equal(probs[sure].argmax(1), p64[sure].argmax(1))
    else:
        pemu = ro.softmax(R.x3_cone_forward(blocks, fw, fb, x))
        demu = np.abs(probs - pemu).max()
        print(f"\nRAW512 {name} bf16x3 max|dev-emu| probs {demu:.3e}; max|dev-f64| probs {dp:.3e}")
        assert demu < X3_DEV_TOL[name] and dp < X3_F64_TOL, (demu, dp)
    m.close()
