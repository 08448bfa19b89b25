"""The generic ConvNet family's bf16x3 mode (csrc/gconv_x3.hip, rs_gconv_set_mode) without a GPU: the C ABI's refusals, the host
packer decoded through the lane map for every conv of the edge table, the emulation of tests/gconv_x3_ref.py against the
reference's own numbers, the recorded gaps the bars come from, and the conditions under which the bars are worth something:
every arithmetic mutant of the split and every device mutant of gconv_ref must miss them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import gconv as G
from riser_amd import synth
from tests import gconv_ref as R
from tests import gconv_x3_ref as X
from tests.tcn_ref import bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG_SEED = 20260103


def _prog(name):
    cfg = R.CONFIGS[name]
    return cfg, G.build_gconv_program(R.make_state_dict(cfg, R.SEED[name]), R.cnn_config(cfg))


_BATCH = {}


def _batch(name):
    """the config's 77 reads, their float64 logits and both emulations' logits: computed once and left unchanged"""
    if name not in _BATCH:
        _, prog = _prog(name)
        lens, rows = X.edge_batch(name)
        _BATCH[name] = dict(prog=prog, lens=lens, rows=rows, want=R.forward(prog, rows, lens),
                            e64=X.forward(prog, rows, lens, np.float64), e32=X.forward(prog, rows, lens, np.float32))
    return _BATCH[name]


def test_abi_refusals_come_before_any_device_call():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    lib = nv.lib()
    assert lib.rs_version() == (2 << 16) | 9
    for dt in (nv.RS_BF16X3, nv.RS_F32, nv.RS_F32W, nv.RS_F16, 99):
        assert lib.rs_gconv_set_mode(None, dt) == nv.RS_ERR_ARG
        assert b"rs_gconv_set_mode" in lib.rs_last_error()
    assert "rs_gconv_set_mode" in nv.SYMBOLS and "rs_gconv_x3_layout" in nv.SYMBOLS
    src = open(os.path.join(ROOT, "include", "riser_amd.h")).read()
    assert re.search(r"RS_API\s+int\s+rs_gconv_set_mode\s*\(\s*rs_gconv\s*\*\s*m\s*,\s*int\s+dtype", src)
    # the x3 form of a conv that fits fp32's LDS but not its own split panel is refused on the host, as set_mode refuses it
    assert G.layer_plan(8, 16, 73)["lds_bytes"] <= 160 * 1024 and G.x3_layout(2048, 2048, 19)["lds_bytes"] <= 160 * 1024
    with pytest.raises(nv.NativeError, match="LDS"):
        G.x3_layout(8, 16, 73)
    with pytest.raises(nv.NativeError, match="c_in <= 4"):
        G.x3_layout(4, 20, 5)
    with pytest.raises(nv.NativeError):
        G.x3_layout(8, 20, 4)


def _x3_convs():
    seen = set()
    for cfg in R.CONFIGS.values():
        seen |= {c[:3] for c in R.convs_of(cfg) if c[0] > 4}
    return sorted(seen)


def test_only_the_first_conv_stays_fp32():
    for cfg in R.CONFIGS.values():
        convs = R.convs_of(cfg)
        assert [i for i, c in enumerate(convs) if R.plan_conv(*c[:3])["vec"] == 1] == [i for i, c in enumerate(convs) if c[0] <= 4]
        assert convs[0][0] == 1 and any(c[0] > 4 for c in convs)


@pytest.mark.parametrize("conv", _x3_convs(), ids=lambda c: "%dx%dk%d" % c)
def test_packer_decodes_through_the_lane_map(conv):
    from riser_amd import build
    build.build()
    ci_n, co_n, k = conv
    p = R.plan_conv(ci_n, co_n, k)
    kc, cols, nchunk = p["kc"], p["cols"], p["n_chunks"]
    c8n, nct, ncb = kc // 8, cols // 16, -(-co_n // cols)
    w = np.random.default_rng(ci_n * 1000 + co_n + k).standard_normal((co_n, ci_n, k)).astype(np.float32)
    lay = G.x3_layout(ci_n, co_n, k, w)
    steps = -(-k * kc // 32)
    assert lay["steps"] == steps and lay["plane"] == ncb * nchunk * cols * steps * 32
    # the last pair of the last step addresses tap (4 steps - 1) // c8n: the slab owns every row up to it, and its pitch is an
    # odd number of 16-byte units
    last_tap = (4 * steps - 1) // c8n
    assert last_tap in (k - 1, k) and lay["slab_rows"] == p["rows"] + last_tap
    assert lay["slab_pitch"] >= kc and lay["slab_pitch"] % 8 == 0 and (lay["slab_pitch"] // 8) % 2 == 1
    assert lay["lds_bytes"] == 4 * (lay["slab_rows"] * lay["slab_pitch"] + cols * steps * 32) <= R.LDS_MAX
    # where the lane map puts weight (col, ci, tap)
    col, ci, tap = np.meshgrid(np.arange(co_n), np.arange(ci_n), np.arange(k), indexing="ij")
    nb, ct, rl = col // cols, (col % cols) // 16, col % 16
    chunk, cc = ci // kc, ci % kc
    pair = tap * c8n + cc // 8
    s, kq, e = pair // 4, pair % 4, cc % 8
    idx = ((((nb * nchunk + chunk) * nct + ct) * steps + s) * 64 + 16 * kq + rl) * 8 + e
    assert len(np.unique(idx)) == idx.size
    hi = (lay["packed"][0].astype(np.uint32) << 16).view(np.float32)
    lo = (lay["packed"][1].astype(np.uint32) << 16).view(np.float32)
    want_hi = bf16(w)
    assert np.array_equal(hi[idx], want_hi) and np.array_equal(lo[idx], bf16(w - want_hi))
    assert np.abs((hi[idx].astype(np.float64) + lo[idx]) - w).max() <= np.abs(w).max() * 2.0 ** -16
    pad = np.ones(lay["plane"], bool)
    pad[idx.ravel()] = False
    assert pad.sum() == lay["plane"] - w.size
    assert not lay["packed"][0][pad].any() and not lay["packed"][1][pad].any()


def test_emulation_reproduces_the_edge_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "gconv_edges.npz"))
    for name in R.GOLDEN_EDGES:
        _, prog = _prog(name)
        meta = json.loads(str(g[f"{name}.cfg"]))
        worst = 0.0
        for L in meta["lengths"]:
            sigs = synth.make_signals(SIG_SEED, 3, L, first_read=60)
            x = np.stack([ro.mad_normalise(s) for s in sigs]).astype(np.float32)
            want = g[f"{name}.L{L}.logits"].astype(np.float64)
            for acc in (np.float64, np.float32):
                worst = max(worst, R.gap(X.forward(prog, x, [L] * 3, acc), want))
        print(f"GCONV_X3_CPU edge fixture {name}: emulation to the reference's logits {worst:.2e} bar {X.X3_BARS[name]:.0e}")
        assert worst <= X.X3_BARS[name], (name, worst)


def test_emulation_reproduces_the_golden_variants(golden_dir):
    g = np.load(os.path.join(golden_dir, "convnet_variants.npz"))
    for name in ("depth2_k5373", "depth1_k7", "depth3_k3"):
        cfg = json.loads(str(g[f"{name}.cfg"]))
        sd = {k[len(name) + 4:]: g[k] for k in g.files if k.startswith(name + ".sd.")}
        prog = G.build_gconv_program(sd, synth.CnnConfig(channels=cfg["channels"], kernels=cfg["kernels"], depth=cfg["depth"]))
        worst = {"E64": 0.0, "E32": 0.0}
        for j, L in enumerate(g[f"{name}.lens"]):
            x = ro.mad_normalise(synth.make_signals(SIG_SEED, 1, int(L), first_read=60 + j)[0]).astype(np.float32)
            for tag, acc in (("E64", np.float64), ("E32", np.float32)):
                got = R.softmax(X.forward_one(prog, x, acc))
                worst[tag] = max(worst[tag], float(np.abs(got - g[f"{name}.probs"][j]).max()))
        print(f"GCONV_X3_CPU golden variant {name}: E64 {worst['E64']:.2e} E32 {worst['E32']:.2e} "
              f"bar {X.VARIANT_BARS[name]:.0e}")
        for tag in worst:
            assert worst[tag] == pytest.approx(X.VARIANT_GAPS[name][tag], rel=0.02), (name, tag, worst[tag])
        assert X.VARIANT_BARS[name] == pytest.approx(R.bar_of(max(X.VARIANT_GAPS[name].values())), rel=1e-9)
        assert max(worst.values()) <= X.VARIANT_BARS[name]


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_recorded_gaps_and_bars(name):
    c = _batch(name)
    e64, e32 = R.gap(c["e64"], c["want"]), R.gap(c["e32"], c["want"])
    print(f"GCONV_X3_CPU {name} E64 {e64:.3e} E32 {e32:.3e} recorded {X.X3_E64[name]:.2e} / {X.X3_E32[name]:.2e} "
          f"bar {X.X3_BARS[name]:.0e} E32 vs E64 {R.gap(c['e32'], c['e64']):.2e}")
    assert np.isfinite(c["e64"]).all() and np.isfinite(c["e32"]).all()
    assert e64 == pytest.approx(X.X3_E64[name], rel=0.02) and e32 == pytest.approx(X.X3_E32[name], rel=0.02)
    rule = R.bar_of(max(X.X3_E64[name], X.X3_E32[name]))                # 4 x the larger gap, rounded up to one digit
    assert X.X3_BARS[name] == pytest.approx(min(rule, X.DRAFT_BARS[name]), rel=1e-9) and X.X3_BARS[name] >= 3 * max(e64, e32)
    # split precision is an approximation of fp32, not of bf16: far above fp32's bar, far below plain bf16's 2^-9
    assert R.BARS[name] < X.X3_BARS[name] <= 5e-4


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_arithmetic_mutants_miss_the_bar(name):
    """plain bf16, lo*hi dropped, hi*lo dropped: each at least MUTANT_MARGIN bars from float64.  On the config's 24 shortest
    reads: the gap is a maximum over reads, so a part of the batch can only make the condition harder to meet."""
    c = _batch(name)
    sub = np.argsort(c["lens"], kind="stable")[:24]
    for arith in X.ARITH_MUTANTS:
        got = X.forward(c["prog"], c["rows"][sub], c["lens"][sub], np.float64, arith=arith)
        gap = R.gap(got, c["want"][sub])
        print(f"GCONV_X3_CPU {name} {arith} {gap:.2e} = {gap / X.X3_BARS[name]:.0f} bars")
        assert gap >= X.MUTANT_MARGIN * X.X3_BARS[name], (name, arith, gap)


@pytest.mark.parametrize("mutant", sorted(R.DEVICE_MUTANTS))
def test_every_device_mutant_misses_the_bar_in_the_emulation(mutant):
    """The shapes of test_gconv_cpu.py's mutant test.  Every mutant misses the x3 bar, and by more than 10 bars (measured: 100
    bars and more) with one exception: one row of right padding read from a finite pitch moves d1_six_layers (kernel 3, six
    pools) by 1.02 bars only.  The x3 bar is some 40 x fp32's and cannot see that leak by accuracy; the device tests see it
    because NaN sits behind every read there - asserted here on the same mutant - and because a read must keep its solo bits."""
    hit, weak = 0, []
    for name, cfg in R.CONFIGS.items():
        if not R.mutant_applies(mutant, cfg) or max(cfg["channels"]) > 140:
            continue
        _, prog = _prog(name)
        rng = np.random.default_rng(R.SEED[name])
        lo = 2 ** cfg["n_layers"]
        lens = [lo + 1, 3 * lo, 5 * lo + 2, 7 * lo + 3]             # even and odd row counts at the first pools
        rows = rng.standard_normal((len(lens), max(lens) + 64)).astype(np.float32)
        want = R.forward(prog, rows, lens)
        assert R.gap(X.forward(prog, rows, lens), want) <= X.X3_BARS[name]
        gap = R.gap(X.forward(prog, rows, lens, mutant=mutant), want)
        assert gap > X.X3_BARS[name], (mutant, name, gap)
        if gap <= 10 * X.X3_BARS[name]:
            weak.append(name)
            for b, L in enumerate(lens):
                rows[b, L:] = np.nan
            assert not np.isfinite(X.forward(prog, rows, lens, mutant=mutant)).all(), (mutant, name)
        hit += 1
    assert hit >= 2, mutant
    assert weak == (["d1_six_layers"] if mutant == "right_pad_reads_pitch" else []), (mutant, weak)


def test_dtypes_and_heads_still_refused():
    import types
    cfg, prog = _prog("d2_k5373")
    for dt in ("f16", "bf16", "f16x3", "f16xf8", "int8"):
        with pytest.raises(ValueError, match="dtype"):              # before any device is asked for
            G.GConvNet(prog, device=None, dtype=dt)
    cnn = R.cnn_config(cfg)
    sd = R.make_state_dict(cfg, 1)
    for field, value in (("kernels", [5, 4, 7, 3]), ("n_classes", 3), ("classifier", "gap"), ("classifier", "fc")):
        with pytest.raises(ValueError):
            G.build_gconv_program(sd, types.SimpleNamespace(**{**vars(cnn), field: value}))
