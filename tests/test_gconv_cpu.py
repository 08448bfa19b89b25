"""Generic ConvNet family (riser_amd/gconv.py, csrc/gconv.hip) without a GPU: the float64 forward of tests/gconv_ref.py against
the reference's own numbers, its defect mutants, the planner mirror against the library's planner, the host program builder's
refusals, and the C ABI's refusals that must come before any device call."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import gconv as G
from riser_amd import synth
from tests import gconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG_SEED = 20260103
GOLDEN_BAR = 1e-3            # tests/golden/convnet_variants.npz: the bar its GPU test holds probabilities to


def _prog(name):
    cfg = R.CONFIGS[name]
    return cfg, G.build_gconv_program(R.make_state_dict(cfg, R.SEED[name]), R.cnn_config(cfg))


def test_float64_forward_reproduces_the_golden_variants(golden_dir):
    g = np.load(os.path.join(golden_dir, "convnet_variants.npz"))
    worst = 0.0
    for name in ("depth2_k5373", "depth1_k7", "depth3_k3"):
        cfg = json.loads(str(g[f"{name}.cfg"]))
        sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
        prog = G.build_gconv_program(sd, synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"]))
        assert G.min_length(prog) == 2 ** cfg["n_layers"]
        for j, L in enumerate(g[f"{name}.lens"]):
            x = ro.mad_normalise(synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0]).astype(np.float32)
            got = R.softmax(R.forward_one(prog, x))
            worst = max(worst, float(np.abs(got - g[f"{name}.probs"][j]).max()))
    print("GCONV_CPU golden variants: largest |float64 - reference| on a probability %.2e" % worst)
    assert worst < 1e-5 < GOLDEN_BAR          # measured 3e-7: the reference's own fp32 round-off


def test_float64_forward_reproduces_the_edge_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "gconv_edges.npz"))
    worst = 0.0
    for name in R.GOLDEN_EDGES:
        cfg, prog = _prog(name)
        meta = json.loads(str(g[f"{name}.cfg"]))
        assert {k: meta[k] for k in cfg} == cfg and meta["seed"] == R.SEED[name]
        assert meta["lengths"][0] == G.min_length(prog) == 2 ** cfg["n_layers"]
        for L in meta["lengths"]:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
            worst = max(worst, R.gap(g[f"{name}.L{L}.logits"], R.forward(prog, x, [L] * 3)))
    print("GCONV_CPU edge fixture: largest gap of the reference's fp32 logits to float64 %.2e" % worst)
    assert worst < 1e-5                       # measured 1.7e-6 when the fixture was made


@pytest.mark.parametrize("mutant", sorted(R.DEVICE_MUTANTS))
def test_every_mutant_misses_the_bar(mutant):
    hit = 0
    for name, cfg in R.CONFIGS.items():
        if not R.mutant_applies(mutant, cfg) or max(cfg["channels"]) > 140:
            continue
        _, prog = _prog(name)
        rng = np.random.default_rng(R.SEED[name])
        lo = 2 ** cfg["n_layers"]
        lens = [lo + 1, 3 * lo, 5 * lo + 2, 7 * lo + 3]             # even and odd row counts at the first pools
        rows = rng.standard_normal((len(lens), max(lens) + 64)).astype(np.float32)
        want = R.forward(prog, rows, lens)
        got = R.forward(prog, rows, lens, mutant=mutant)
        assert R.gap(got, want) > 10 * R.BARS[name], (mutant, name, R.gap(got, want))
        hit += 1
    assert hit >= 2, mutant


def test_edge_table_reaches_every_tag():
    seen = set()
    for cfg in R.CONFIGS.values():
        seen |= R.shape_tags(cfg)
    assert sorted(seen) == R.ALL_TAGS
    assert len(R.CONFIGS) == 11 and {c["depth"] for c in R.CONFIGS.values()} == {1, 2, 3}
    assert {1, 3, 5, 9, 19} <= {k for c in R.CONFIGS.values() for k in c["kernels"]}
    for name, cfg in R.CONFIGS.items():
        lens = R.edge_lengths(cfg, R.SEED[name])
        assert len(lens) == R.N_READS and lens.min() == 2 ** cfg["n_layers"] and lens.max() <= cfg["max_len"]
        assert {4096, 4097} <= set(lens.tolist())


def test_bars_follow_the_rule():
    for name in R.CONFIGS:
        assert R.BARS[name] == pytest.approx(R.bar_of(R.GCONV_GAP[name]), rel=1e-9), name


def test_build_gconv_program_refusals():
    cfg = R.CONFIGS["d2_k5373"]
    sd = R.make_state_dict(cfg, 1)
    cnn = R.cnn_config(cfg)
    prog = G.build_gconv_program(sd, cnn)
    assert len(prog["convs"]) == 8 and prog["convs"][1]["w"].shape == (6, 6, 5)
    assert G.program_macs(prog, 16) == sum((16 >> (i // 2)) * int(np.prod(c["w"].shape)) for i, c in enumerate(prog["convs"]))
    for field, value in (("kernels", [5, 4, 7, 3]), ("n_classes", 3), ("classifier", "gap"), ("classifier", "fc"),
                         ("channels", [6, 9, 14]), ("n_layers", 0)):
        bad = types.SimpleNamespace(**{**vars(cnn), field: value})
        with pytest.raises(ValueError):
            G.build_gconv_program(sd, bad)
    with pytest.raises(ValueError, match="even conv kernels"):           # before the state dict is looked at
        G.build_gconv_program({}, types.SimpleNamespace(**{**vars(cnn), "kernels": [4, 3, 3, 3]}))
    with pytest.raises(ValueError, match="layers.0.0"):
        G.build_gconv_program({k: v for k, v in sd.items() if k != "layers.0.0.bias"}, cnn)
    wrong = dict(sd)
    wrong["layers.1.2.weight"] = np.zeros((9, 9, 5), np.float32)
    with pytest.raises(ValueError, match="layers.1.2"):
        G.build_gconv_program(wrong, cnn)


def test_min_length_is_two_to_the_layers():
    for name, cfg in R.CONFIGS.items():
        assert G.min_length(_prog(name)[1]) == 2 ** cfg["n_layers"]


def test_header_declares_what_native_binds():
    from riser_amd import _native as nv
    src = open(os.path.join(ROOT, "include", "riser_amd.h")).read()
    bound = [s for s in nv.SYMBOLS if s.startswith("rs_gconv_")]
    assert len(bound) >= 6
    for s in bound:
        m = re.search(r"/\*(?:(?!\*/).)*\*/\s*RS_API[^;]*\b%s\s*\(" % s, src, flags=re.S)
        assert m, f"{s} is not declared in include/riser_amd.h under a comment"
        assert "riser/nets/cnn.py:12-18" in m.group(0) and "43-65" in m.group(0), f"{s} does not cite the reference"


def test_create_refusals_come_before_any_device_call():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    lib = nv.lib()
    assert lib.rs_version() == (2 << 16) | 9
    w = np.zeros(2048 * 2048 * 3, np.float32)
    b = np.zeros(2048, np.float32)
    fc = np.zeros(2 * 2048, np.float32)

    def create(convs, n_layers, depth, device=10 ** 6):
        arr = (G._Conv * len(convs))(*[G._Conv(ci, co, k, 0, w.ctypes.data, b.ctypes.data) for ci, co, k in convs])
        h = C.c_void_p()
        rc = lib.rs_gconv_create(arr, n_layers, depth, fc.ctypes.data, fc.ctypes.data, device, C.byref(h))
        assert not h.value
        return rc, lib.rs_last_error()

    # device 1 000 000 does not exist: a refusal that names the argument was made without asking for it
    rc, msg = create([(1, 8, 4)], 1, 1)
    assert rc == nv.RS_ERR_ARG and b"even kernel" in msg
    rc, msg = create([(1, 8, 3), (9, 8, 3)], 2, 1)
    assert rc == nv.RS_ERR_ARG and b"chained" in msg
    rc, msg = create([(1, 4, 3)] + [(4, 4, 3)] * 16, 17, 1)
    assert rc == nv.RS_ERR_ARG and b"length table" in msg
    rc, msg = create([(1, 8, 3), (8, 2048, 129)], 2, 1)
    assert rc == nv.RS_ERR_ARG and b"LDS" in msg
    assert lib.rs_gconv_create(None, 1, 1, None, None, 0, None) == nv.RS_ERR_ARG
    assert lib.rs_gconv_min_length(None) == nv.RS_ERR_ARG and b"rs_gconv_min_length" in lib.rs_last_error()
    assert lib.rs_gconv_workspace_bytes(None, 1, 64) == 0 and lib.rs_gconv_max_batch(None, 64) == 0
    assert lib.rs_gconv_destroy(None) == nv.RS_OK
    # what the family must run: k <= 19 at up to 2048 channels
    for ci, co, k in ((2048, 2048, 19), (1, 2048, 19), (2048, 5, 19), (1702, 1135, 5)):
        assert G.layer_plan(ci, co, k)["lds_bytes"] <= 160 * 1024


def test_planner_mirror_matches_the_library():
    from riser_amd import build
    build.build()
    seen = set()
    for cfg in R.CONFIGS.values():
        seen |= {c[:3] for c in R.convs_of(cfg)}
    seen |= {(757, 1135, 5), (1135, 1702, 5), (20, 30, 3), (2048, 2048, 19), (64, 64, 7), (65, 128, 3), (16, 256, 5), (16, 257, 7)}
    for ci, co, k in sorted(seen):
        want = R.plan_conv(ci, co, k)
        got = G.layer_plan(ci, co, k)
        assert {f: got[f] for f in want} == want, (ci, co, k)
