"""The ResNet's conv programs across every launch form of csrc/seqnet.hip, in both modes, against float64.

The forward picks one of ~70 kernel instantiations per launch from channel counts, LDS footprints, the read's length and the
mode (rs_seqnet_launch_plan reports the choice; resnet_ref.Program mirrors it).  The configs below are chosen with the mirror so
that together they launch every reachable instantiation in each mode.  Each config runs, per mode:
  ragged_ok   one ragged batch of 77 reads (NaNs behind every read in its row), every read equal to its solo run bit for bit;
  otherwise   uniform calls per length group, plus one under RS_SEQ_NOFUSE=1, one with a buffer window too small for any
              fused launch (RS_SEQ_WINDOW_BYTES) and one on the scalar conv (RS_SEQ_SCALAR=1), each reporting that path in its
              plan and held to the same bounds;
and is held to:
  fp32    float64 (resnet_ref.f64_ragged) within F32_TOL[config] x max(1, |logit|), probabilities within 1e-5;
  bf16x3  the numpy emulation of the split arithmetic (resnet_ref.x3_ragged) within X3_DEV_TOL[config], float64 within
          5e-3 x max(1, |logit|), probabilities within 1e-3.
Bottleneck configs run bf16x3 as created under RS_SEQ_BNECK_X3=1 (split bottleneck blocks).  Every mutant of resnet_ref must
miss by more than ten times its config's tolerance, so that the tolerances can see those bugs.  Six edge configs are pinned to
the reference's own ResNet (tests/golden/resnet_edges.npz) on the CPU."""
import os
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import resnet as RN
from riser_amd import synth
from tests import resnet_ref as R

_B = lambda ch, bl, k=19, p=5, s=3: dict(channels=ch, kernel=k, padding=p, stride=s, block="basic", n_layers=len(ch), blocks=bl,
                                         n_classes=2)
_N = lambda ch, bl, k=19, p=5, s=3: dict(_B(ch, bl, k, p, s), block="bottleneck")
CONFIGS = {
    "bench": dict(synth.RESNET_BENCH_CFG),              # stem nt 2; <2,2,4>, <3,1,4>, 8-wave nt 5; x3 <3,1,8>
    "s1_w8_np56": _B([12, 56], [1, 2]),                 # stem nt 1, 8-wave <4,1,8>, compact NP 56 < 64
    "np40": _B([44, 40], [1, 2], k=9, p=4, s=2),        # a 40-channel stage after a 44-channel one: NP 40 < 48
    "odd_c": _B([5, 9, 17, 33], [1, 1, 1, 1], k=7, p=3, s=1),   # widths 1 mod 4 / 8 / 16; stem nt 1; mtw 2 forms
    "s3_s5": _B([40, 60, 76], [1, 1, 1], k=11, p=2, s=4),       # stem nt 3, nt 4 / 5 blocks
    "s4": _B([52, 24, 66], [1, 1, 1]),                  # stem nt 4
    "mixed": _B([40, 36, 76], [1, 1, 1], k=9, p=4, s=2),        # bf16x3: the 36 -> 76 block fits fp32 LDS only and stays fp32
    "s5": _B([72, 80], [1, 1], k=5, p=0, s=2),          # stem nt 5, widest fused block
    "mtw2": _B([8, 49, 24, 40], [2, 1, 1, 1], k=3, p=1, s=1),   # two row tiles per wave at nt 1-4 (8 -> 49: small enough)
    "wide_stem": _B([96, 40], [1, 1], k=7, p=3, s=2),   # > 80 channels: unfused stem conv + pool and stage (conv_mfma<4>, 2 groups)
    "w8_nt1": _B([300, 13], [1, 1], k=9, p=4, s=8),     # a 300-channel input: 8-wave nt 1 blocks
    "w8_nt2": _B([128, 29], [1, 1], k=9, p=4, s=8),     # 8-wave nt 2
    "bneck_nto123": _N([16, 32, 48], [1, 1, 1]),        # NTM 1 with NTO 1, 2, 3
    "bneck_nto45": _N([64, 66, 72], [1, 1, 1], k=9, p=4, s=2),  # NTO 4; NTO 5 at NTM 1 (66) and NTM 2 (72)
    "bneck_wide": dict(channels=[32, 48, 68], kernel=19, padding=5, stride=3, block="bottleneck", n_layers=3, blocks=[2, 2, 1],
                       n_classes=2),
}
NAMES = list(CONFIGS)
MODES = ["f32", "bf16x3"]
N_READS = 77
MAX_LEN = 16000
LD = MAX_LEN + 123                                   # the ragged batch's row pitch: longer than the longest read

# fp32 device against float64, x max(1, |logit|), per config: about 4x the largest gap measured on an MI355X over the sweep
# (ragged batch, length groups, the unfused paths), rounded up; far inside the 1e-4 test_resnet.py holds the golden nets to.
# Measured:
F32_GAP = {"bench": 4.1e-07, "s1_w8_np56": 2.5e-07, "np40": 3.5e-07, "odd_c": 2.4e-07, "s3_s5": 4.6e-07, "s4": 3.4e-07, "s5":
           3.5e-07, "mtw2": 3.2e-07, "wide_stem": 3.0e-07, "w8_nt1": 2.1e-07, "w8_nt2": 2.7e-07, "bneck_nto123": 1.6e-07,
           "bneck_nto45": 4.0e-07, "bneck_wide": 2.8e-07, "mixed": 4.2e-07}
F32_TOL = {"bench": 2e-6, "s1_w8_np56": 2e-6, "np40": 2e-6, "odd_c": 1e-6, "s3_s5": 2e-6, "s4": 2e-6, "s5": 2e-6, "mtw2": 2e-6,
           "wide_stem": 2e-6, "w8_nt1": 9e-7, "w8_nt2": 2e-6, "bneck_nto123": 7e-7, "bneck_nto45": 2e-6, "bneck_wide": 2e-6, "mixed": 2e-6}
# bf16x3 device against the emulation of its arithmetic (absolute, logits), per config: about 4x the largest measured gap,
# rounded up.  The gap is the device's fp32 accumulation against float64 sums.  Measured:
X3_GAP = {"bench": 7.3e-06, "s1_w8_np56": 1.3e-06, "np40": 1.3e-06, "odd_c": 1.0e-06, "s3_s5": 1.2e-06, "s4": 4.8e-06, "s5":
          5.2e-07, "mtw2": 3.3e-06, "wide_stem": 4.9e-07, "w8_nt1": 7.0e-07, "w8_nt2": 6.7e-07, "bneck_nto123": 1.8e-06,
          "bneck_nto45": 1.6e-06, "bneck_wide": 3.9e-06, "mixed": 1.8e-06}
X3_DEV_TOL = {"bench": 3e-5, "s1_w8_np56": 6e-6, "np40": 6e-6, "odd_c": 5e-6, "s3_s5": 5e-6, "s4": 2e-5, "s5": 3e-6, "mtw2":
              2e-5, "wide_stem": 2e-6, "w8_nt1": 3e-6, "w8_nt2": 3e-6, "bneck_nto123": 8e-6, "bneck_nto45": 7e-6, "bneck_wide":
              2e-5, "mixed": 8e-6}
X3_F64_TOL = 5e-3                                    # bf16x3 device against float64, x max(1, |logit|)


_CACHE = {}


def program(name):
    """(cfg, sd, prog, n_buffers, fw, fb, c_last) of a sweep config: synth weights, seed 17"""
    if name not in _CACHE:
        cfg = CONFIGS[name]
        sd = synth.make_resnet_state_dict(17, cfg)
        _CACHE[name] = (cfg, sd) + RN.build_program(sd, types.SimpleNamespace(**cfg))
    return _CACHE[name]


def mirror(name, mode, **env):
    cfg, sd, prog, nb, fw, fb, c_last = program(name)
    return R.Program(prog, nb, c_last, bneck_x3=mode == "bf16x3" and cfg["block"] == "bottleneck", **env)


def _first_length(pm, op, target, lo):
    """the smallest L >= lo at which op's output has `target` rows (None if the length jumps over it)"""
    while True:
        s = pm.shapes(lo)
        if s is not None and s[op][1] >= target:
            return lo if s[op][1] == target else None
        lo = lo + 1 if s is None else max(lo + 1, lo + (target - s[op][1]) // 2)
        if lo > MAX_LEN:
            return None


def sweep_lengths(name):
    """77 read lengths: the program minimum (and +1), per fused block and mode a length whose block output is below one
    tile, exactly one, one plus one and = -1 (mod tile), MAX_LEN, seeded random lengths in between"""
    fixed = set()
    for mode in MODES:
        pm = mirror(name, mode)
        lo = pm.min_length()
        fixed |= {lo, lo + 1, MAX_LEN}
        for l in pm.plan(1, 4000, mode):
            if l["family"] == "basic_block":
                op, tos = l["op"] + l["n_ops"] - 2, (62, 126)
            elif l["family"] == "bottleneck":
                op, tos = l["op"] + l["n_ops"] - 2, ((128 - 3) // pm.ops[l["op"] + l["n_ops"] - 2]["stride"] + 1,)
            else:
                continue
            for to in tos:
                for ts in ([to - 1], [to], [to + 1], [j * to - 1 for j in range(2, 9)]):
                    for t in ts:                     # (a stride-2 chain can jump over a target: the next of the class)
                        L = _first_length(pm, op, t, lo)
                        if L is not None:
                            fixed |= {L, min(L + 1, MAX_LEN)}
                            break
    fixed = sorted(fixed)[:60]
    rng = np.random.default_rng(sum(map(ord, name)))
    rest = rng.integers(min(fixed), MAX_LEN + 1, N_READS - len(fixed)).tolist()
    return fixed + [int(v) for v in rest]


_SIGNALS = []


def reads(name):
    """the sweep's reads: read i is the last n_i samples of a normalised synthetic read of 16000 samples"""
    if not _SIGNALS:
        for i in range(N_READS):
            s = synth.make_signals(20260104, 1, MAX_LEN, first_read=7100 + i)[0]
            _SIGNALS.append(ro.mad_normalise(s).astype(np.float32))
    return [_SIGNALS[i][MAX_LEN - n:] for i, n in enumerate(sweep_lengths(name))]


_REF = {}


def reference(name):
    """float64 logits and emulated bf16x3 logits of every read of the sweep"""
    if name not in _REF:
        cfg, sd = program(name)[:2]
        rs = reads(name)
        _REF[name] = (R.f64_ragged(sd, cfg, rs), R.x3_ragged(sd, cfg, rs, bneck_x3=cfg["block"] == "bottleneck"))
    return _REF[name]


def sweep_plans(name, mode):
    """the launch lists of the sweep in a mode: the batch call(s) and every read alone"""
    pm = mirror(name, mode)
    lens = sweep_lengths(name)
    plans = [pm.plan(1, L, mode) for L in lens]
    if pm.ragged_ok():
        plans.append(pm.plan(N_READS, LD, mode, ragged=True))
    else:
        for L in sorted(set(lens)):
            plans.append(pm.plan(lens.count(L), L, mode))
        L = max(lens)
        plans.append(mirror(name, mode, nofuse=True).plan(1, L, mode) if mode == "f32" else [])
        plans.append(mirror(name, mode, window=_small_window(name, L)).plan(1, L, mode) if mode == "f32" else [])
        plans.append(mirror(name, mode, scalar=True).plan(1, L, mode) if mode == "f32" else [])
    return plans


def _small_window(name, L):
    """a buffer window below every fused launch's buffers but above the program input of one read of L samples"""
    return 4 * L


def reached(mode):
    return {R.instantiation(l) for n in NAMES for p in sweep_plans(n, mode) for l in p}


# instantiations no config can launch, with the reason (resnet_ref.Program enumerated over stems of 1-96 channels, stages of
# 1-96 channels behind stems of up to 512, both blocks, lengths 200-16000)
UNREACHABLE = {
    "basic_block<5,2,4>": "nt 5 (65-80 channels): the 3x3 weights alone are >= 55 KB, so a 128-row tile never leaves room for "
                          "a second workgroup",
    "basic_block_x3<4,2,4>": "the split planes double the weights: no nt-4 block fits two 128-row workgroups per CU",
    "basic_block_x3<5,2,4>": "as basic_block_x3<4,2,4>",
    **{f"bottleneck{x}<2,{n}>": "the reference's c_mid = c_out // 4: c_mid >= 17 (NTM 2) forces c_out >= 68 (NTO 5)"
       for x in ("", "_x3") for n in (1, 2, 3, 4)},
}


# ------------------------------------------------------------------------------------------------ CPU
def test_sweep_reaches_every_launch_form_in_both_modes():
    allset = R.all_instantiations()
    assert set(UNREACHABLE) <= allset
    got = reached("f32") | reached("bf16x3")
    assert got == allset - set(UNREACHABLE), sorted((allset - set(UNREACHABLE)) ^ got)
    for mode in MODES:
        x = "_x3" if mode == "bf16x3" else ""
        for nt in range(1, 6):                          # the stem at every width, in each mode
            assert f"stem_pool{x}<{nt}>" in reached(mode), (mode, nt)


def test_sweep_configs_cover_the_layout_branches():
    """the layout branches of fuse_program that no instantiation name shows"""
    pitches, mixed, not_ragged = set(), False, []
    for name in NAMES:
        pm = mirror(name, "bf16x3")
        if not pm.ragged_ok():
            not_ragged.append(name)
        blocks = [o for o in pm.ops if o["fuse"] == 2]
        for o in blocks:
            pitches.add(("f32", o["f_np"] < 16 * o["f_nt"]))
            pitches.add(("x3", o["x_np"] < 16 * o["f_nt"]))
        mixed |= any(not o["x"] for o in blocks) and any(o["x"] for o in blocks)
    assert pitches == {(m, c) for m in ("f32", "x3") for c in (False, True)}, pitches
    assert {"wide_stem", "w8_nt1", "w8_nt2"} <= set(not_ragged) and "bench" not in not_ragged, not_ragged
    assert mixed


def test_sweep_lengths_cover_the_tile_edges():
    """per config and mode, every fused basic block sees outputs below one tile, one tile, one plus one and -1 mod the tile"""
    for name in NAMES:
        for mode in MODES:
            pm = mirror(name, mode)
            lens = sweep_lengths(name)
            seen = {}
            for L in lens:
                shp = pm.shapes(L)
                for l in pm.plan(1, L, mode):
                    if l["family"] == "basic_block":
                        to = 16 * l["mtw"] * l["waves"] - 2
                        t = shp[l["op"] + l["n_ops"] - 2][1]
                        seen.setdefault(l["op"], set()).update(
                            {"below" if t < to else "one" if t == to else "one+1" if t == to + 1 else None,
                             "-1" if t % to == to - 1 and t > to else None})
            for op, s in seen.items():
                assert {"below", "one", "one+1", "-1"} <= s, (name, mode, op, s)


EDGES = ["s1_w8_np56", "np40", "bneck_nto123", "bneck_nto45", "wide_stem", "mixed"]


@pytest.mark.parametrize("name", EDGES)
def test_edge_configs_match_the_reference(golden_dir, name):
    """the float64 forward pinned to the reference's own ResNet (tests/golden/resnet_edges.npz) on edge configs of the sweep:
    the same config and weights (rebuilt from the seed, checked by their digest), the program's minimum length and beyond"""
    import json
    g = np.load(os.path.join(golden_dir, "resnet_edges.npz"))
    cfg = json.loads(str(g[f"{name}.cfg"]))
    lens, seed, sha = cfg.pop("lengths"), cfg.pop("seed"), cfg.pop("sd_sha16")
    assert cfg == CONFIGS[name]
    sd = program(name)[1]
    assert seed == 17 and synth.state_dict_sha16(sd) == sha
    assert lens[0] == mirror(name, "f32").min_length()
    for L in lens:
        sigs = synth.make_signals(20260103, 3, L, first_read=80)
        x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
        lg = R.f64_ragged(sd, cfg, x)
        assert np.abs(lg - g[f"{name}.L{L}.logits"]).max() < 1e-5, L
        assert np.abs(ro.softmax(lg) - g[f"{name}.L{L}.probs"]).max() < 1e-5, L


# mutants that are the identity on a config
def _applies(name, mutant):
    cfg = CONFIGS[name]
    if mutant == "bneck_stride_1x1":
        return cfg["block"] == "bottleneck"
    if mutant == "basic_stride_conv2":
        return cfg["block"] == "basic"
    return True


@pytest.mark.parametrize("name", NAMES)
def test_mutants_are_caught_at_the_sweep_tolerances(name):
    """every applicable mutant moves some logit of the sweep by more than 10x the tolerance its config is held to"""
    cfg, sd = program(name)[:2]
    sel = reads(name)[:6] + reads(name)[-2:]
    base = R.f64_ragged(sd, cfg, sel)
    scale = np.maximum(1.0, np.abs(base))
    for mutant in R.MUTANTS:
        if not _applies(name, mutant):
            continue
        with np.errstate(invalid="ignore"):          # the unpadded pool leaves the shortest read no rows: NaN, left out
            miss = np.nanmax(np.abs(R.f64_ragged(sd, cfg, sel, mutant=mutant) - base) / scale)
        assert miss > 10 * F32_TOL[name], (mutant, miss)
    bx = cfg["block"] == "bottleneck"
    emu = R.x3_ragged(sd, cfg, sel, bneck_x3=bx)
    for mutant in R.X3_MUTANTS:
        miss = np.abs(R.x3_ragged(sd, cfg, sel, mutant=mutant, bneck_x3=bx) - emu).max()
        assert miss > 10 * X3_DEV_TOL[name], (mutant, miss)


def test_every_mutant_applies_somewhere():
    assert all(any(_applies(n, m) for n in NAMES) for m in R.MUTANTS)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _net(name, mode, env=None):
    """a SeqNet of the config, created with the RS_SEQ_* variables of env set (restored afterwards)"""
    cfg, sd, prog, nb, fw, fb, c_last = program(name)
    env = dict(env or {})
    if mode == "bf16x3" and cfg["block"] == "bottleneck":
        env["RS_SEQ_BNECK_X3"] = "1"
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return RN.SeqNet(prog, nb, fw, fb, c_last, device=_dev(), dtype=mode)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check(name, mode, logits, probs, idx, tag):
    f64, emu = reference(name)
    f64, emu = f64[idx], emu[idx]
    scale = np.maximum(1.0, np.abs(f64))
    d64 = (np.abs(logits - f64) / scale).max()
    dp = np.abs(probs - ro.softmax(f64)).max()
    if mode == "f32":
        print(f"\nRESNET_SWEEP {name} {tag} f32 max|dev-f64|/scale {d64:.3e} probs {dp:.3e}")
        assert d64 < F32_TOL[name] and dp < 1e-5, (d64, dp)
    else:
        demu = np.abs(logits - emu).max()
        print(f"\nRESNET_SWEEP {name} {tag} bf16x3 max|dev-emu| {demu:.3e} max|dev-f64|/scale {d64:.3e} probs {dp:.3e}")
        assert demu < X3_DEV_TOL[name], demu
        assert d64 < X3_F64_TOL and dp < 1e-3, (d64, dp)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_sweep(name, mode):
    import torch
    net = _net(name, mode)
    pm = mirror(name, mode)
    sigs = reads(name)
    lens = [len(s) for s in sigs]
    assert net.ragged_ok == pm.ragged_ok()
    for L in sorted(set(lens)):                      # the query is the mirror, every read alone
        assert net.launch_plan(1, L) == pm.plan(1, L, mode), L
    if pm.ragged_ok():
        assert net.launch_plan(N_READS, LD, ragged=True) == pm.plan(N_READS, LD, mode, ragged=True)
        x = torch.full((N_READS, LD), float("nan"), dtype=torch.float32)
        for i, s in enumerate(sigs):
            x[i, :len(s)] = torch.from_numpy(s)
        ln = torch.tensor(lens, dtype=torch.int32, device=net.device)
        probs, logits = net.forward_ragged(x.to(net.device), ln, return_logits=True)
        probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
        _check(name, mode, logits, probs, np.arange(N_READS), "ragged")
        for i, s in enumerate(sigs):                 # every read alone, bit for bit
            p1, l1 = net.forward(torch.from_numpy(s)[None].to(net.device), return_logits=True)
            assert np.array_equal(p1.cpu().numpy()[0], probs[i]), (i, lens[i])
            assert np.array_equal(l1.cpu().numpy()[0], logits[i]), (i, lens[i])
    else:
        with pytest.raises(Exception, match="outside its fused launches"):
            net.launch_plan(N_READS, LD, ragged=True)
        for L in sorted(set(lens)):                  # uniform calls per length group
            idx = np.array([i for i, n in enumerate(lens) if n == L])
            assert net.launch_plan(len(idx), L) == pm.plan(len(idx), L, mode), L
            x = torch.from_numpy(np.stack([sigs[i] for i in idx])).to(net.device)
            probs, logits = net.forward(x, return_logits=True)
            _check(name, mode, logits.cpu().numpy(), probs.cpu().numpy(), idx, f"L{L}")
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in NAMES if not R.Program(*[program(n)[i] for i in (2, 3, 6)]).ragged_ok()])
def test_unfused_paths_of_programs_that_are_not_ragged_ok(name):
    """the same config op by op (RS_SEQ_NOFUSE=1), with a buffer window too small for any fused launch, and on the scalar conv
    kernel (RS_SEQ_SCALAR=1): the plan reports that path and the logits hold the same bounds"""
    import torch
    lens = sweep_lengths(name)
    L = max(lens)
    idx = np.array([i for i, n in enumerate(lens) if n == L])
    x = torch.from_numpy(np.stack([reads(name)[i] for i in idx])).to(_dev())
    for env, kw in (({"RS_SEQ_NOFUSE": "1"}, dict(nofuse=True)),
                    ({"RS_SEQ_WINDOW_BYTES": str(_small_window(name, L))}, dict(window=_small_window(name, L))),
                    ({"RS_SEQ_SCALAR": "1"}, dict(scalar=True))):
        net = _net(name, "f32", env)
        plan = net.launch_plan(len(idx), L)
        assert plan == mirror(name, "f32", **kw).plan(len(idx), L, "f32"), env
        assert not {l["family"] for l in plan} & {"stem_pool", "basic_block", "bottleneck"}, env
        probs, logits = net.forward(x, return_logits=True)
        _check(name, "f32", logits.cpu().numpy(), probs.cpu().numpy(), idx, "+".join(env))
        net.close()


@pytest.mark.gpu
def test_launch_plan_refusals():
    """rs_seqnet_launch_plan refuses what the forward refuses, with the forward's error text"""
    import ctypes as C
    from riser_amd import _native as nv
    net = _net("bench", "f32")
    lib, n = nv.lib(), C.c_int32(-7)
    pm = mirror("bench", "f32")
    lo = pm.min_length()
    assert lib.rs_seqnet_launch_plan(net._h, 0, 4000, 0, None, 0, C.byref(n)) == nv.RS_ERR_ARG
    assert lib.rs_seqnet_launch_plan(net._h, 1, 4000, 0, None, 0, None) == nv.RS_ERR_ARG
    assert b"rs_seqnet_launch_plan" in lib.rs_last_error()
    assert lib.rs_seqnet_launch_plan(net._h, 1, lo - 1, 0, None, 0, C.byref(n)) == nv.RS_ERR_LENGTH
    assert b"too short for this network" in lib.rs_last_error()
    assert n.value == -7
    assert lib.rs_seqnet_launch_plan(net._h, 1, lo, 0, None, 0, C.byref(n)) == nv.RS_OK and n.value == len(pm.plan(1, lo))
    with pytest.raises(ValueError):
        net.forward(__import__("torch").zeros((1, lo - 1), device=net.device))
    net.close()
