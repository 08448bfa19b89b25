"""Every tile shape of the three fp32 conv kernels (direct, Winograd F(2,3), Winograd F(4,3)) held to the planner's bits and,
one layer at a time, to float64.

The kernels pick one entry of a shape table (kShapes[] in csrc/conv_f32.hip, conv_wino.hip, conv_wino4.hip) per launch; the
tables are read out of the sources here (tests/convnet_ref.py), so a shape added later is swept without an edit.  Per net
variant (convnet_ref.VARIANTS: the shipped 12-layer net and a narrow 6-layer one, each as direct, all-F(2,3) and all-F(4,3)
with chunks of 16 and of 20, plus the model of record) on one ragged batch of 77 reads (lengths by rule:
convnet_ref.sweep_lengths; NaNs behind every read):
  same bits   every table entry forced onto every layer of its family (RS_FORCE_SHAPE_F32 / _WINO / _WINO4), the RS_SHAPE_D
              entries also under RS_NO_DEEP_STAGING=1, reproduces the planner's probabilities, logits and the family's last
              layer bit for bit; a force is honoured exactly where the mirror of lds_bytes() says it fits, and the union of
              honoured (family, shape, chunk, deep?) EQUALS the mirror's set of fitting instantiations (UNREACHABLE lists
              what cannot be launched, with the reason);
  float64     every conv layer i of the planner's own model against conv -> bias -> ReLU -> MaxPool in float64 computed from
              the DEVICE's layer i - 1 output (one kernel's error, not twelve layers' sum), every read, valid row and channel,
              padding rows and channels exactly zero; logits and probabilities against the float64 forward.
Batches of 576 and 640 full-length reads run F(4,3) and F(2,3) layers as head + tail launches: equal bits with RS_NO_TAIL_SPLIT=1
and RS_NO_RECT_ORDER=1.
The tolerances are about four times the largest gap measured on an MI355X (below, next to each other); on the CPU every mutant
of convnet_ref (a defect of the float64 reference) must miss by more than ten times the tolerance, so the bars can see them."""
import contextlib
import re
import time

import numpy as np
import pytest

from oracle import riser_oracle as ro
from riser_amd import synth
from tests import convnet_ref as R

from conftest import hooked_model

# device against float64 per layer, x max(1, max |reference|) of the layer and read.  Measured on an MI355X over the whole
# sweep (every variant, layer, read, row, channel), and the bar: about 4x, rounded up.  (The fp32 numpy oracle, acc=float32,
# on the same layers from the same inputs: LAYER_GAP_NUMPY32.)
LAYER_GAP = {"direct": 2.3e-6, "wino": 1.7e-6, "wino4": 2.3e-6}
LAYER_GAP_NUMPY32 = {"direct": 1.3e-6, "wino": 1.8e-6, "wino4": 1.3e-6}
LAYER_TOL = {"direct": 1e-5, "wino": 7e-6, "wino4": 1e-5}
# end to end: logits x max(1, |logit|), probabilities absolute
E2E_GAP = {"logits": 2.6e-5, "probs": 8.8e-6}
E2E_TOL = {"logits": 1.1e-4, "probs": 4e-5}

BASE_ENV = {"RS_SMALL_F32_WAVES": "0", "RS_NO_STREAM_F32": "1"}     # the tiled kernels on every layer
SWEPT = [v for v, spec in R.VARIANTS.items() if spec[3]]

# instantiations no variant can launch, with the reason
UNREACHABLE = {}


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_shape_tables_parse(family):
    shapes = R.parse_shapes(family)
    assert shapes
    assert len({s[:4] for s in shapes}) == len(shapes)                       # no duplicates
    assert all(s[0] * s[1] in (4, 8) for s in shapes)
    assert all((s[0] * s[1] == 4) == (s[4] == "4") for s in shapes if family != "direct")
    n4 = sum(s[0] * s[1] == 4 for s in shapes)
    assert 0 < n4 < len(shapes)


def test_lds_mirror():
    """the mirror against footprints worked out by hand from the kernels' comments, and the limit's two sides"""
    assert R.lds_bytes("direct", (8, 1, 4, 2), 16) == 2 * ((512 + 2) + 3 * 32) * 18 * 4
    assert R.lds_bytes("wino", (8, 1, 2, 2), 20) == 2 * (2 * (256 + 1) + 4 * 32) * 22 * 4
    assert R.lds_bytes("wino4", (8, 1, 1, 6), 16) == 2 * (4 * (128 + 1) + 6 * 96) * 18 * 4
    # conv_wino4.hip: the 512 x 96 tile fits with chunks of 16 only (157 KB)
    assert R.fits("wino4", (8, 1, 1, 6), 16) and not R.fits("wino4", (8, 1, 1, 6), 20)
    assert R.tile("wino4", (8, 1, 1, 6)) == (512, 96) and R.tile("wino", (8, 1, 2, 2)) == (512, 32)
    for fam in R.FAMILIES:
        inst = R.instantiations(fam)
        assert all(R.fits(f, s, kc or R.RT_KC_MAX) for f, s, kc, _ in inst)
        assert {kc for _, _, kc, _ in inst} == set(R.FAMILIES[fam]["kcs"])
        assert any(d for *_, d in inst) == (fam != "direct")
        # some (shape, chunk) of every table does NOT fit: the silent "force ignored" path exists and is exercised
        assert any(not R.fits(fam, s, kc) for s in R.parse_shapes(fam) for kc in R.FAMILIES[fam]["kcs"] if kc)
    assert set(UNREACHABLE) <= set().union(*(R.instantiations(f) for f in R.FAMILIES))


def test_sweep_lengths_follow_the_rules():
    for n_layers in (12, 6):
        lens = R.sweep_lengths(n_layers)
        lo = 1 << n_layers
        assert len(lens) == R.N_READS and R.N_READS % 2 == 1 and min(lens) == lo and lo + 1 in lens and max(lens) == R.MAX_LEN
        for i in range(n_layers):
            assert {(n >> i) % 4 for n in lens} == {0, 1, 2, 3}, i
            assert any((n >> i) % 2 for n in lens)                           # an odd count loses a row to the pool
        for blk in (1024, 4096, 8192):
            assert {n % blk for n in lens} >= {blk - 1, 0, 1}, blk


def test_layer_reference_is_the_oracle():
    """convnet_ref.layer_f64, direct and as F(4,3), against oracle.riser_oracle.conv_block in float64"""
    sd = R.state_dict(R.NARROW)
    x = R.reads(6)[5]
    ins = R.layer_inputs(sd, x, 5)
    for i in range(1, 6):
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        want = ro.conv_block(ins[i][None], w, b, acc=np.float64)[0]
        assert np.array_equal(R.layer_f64(ins[i], w, b), want), i
        assert np.abs(R.layer_f64(ins[i], w, b, wino4=True) - want).max() < 1e-12 * max(1.0, np.abs(want).max()), i


def _mutant_misses(channels, layers, sigs, mutant):
    """per layer the largest miss of a mutant over the reads, x max(1, max |reference|) of the layer and read"""
    sd = R.state_dict(channels)
    ins = [R.layer_inputs(sd, x, max(layers)) for x in sigs]
    out = {}
    for i in layers:
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        kcs = [kc for kc in (16, 20, 24) if w.shape[1] % kc] if mutant == "weigh_pad_channels" else [16]
        for kc in kcs:
            miss = 0.0
            for k, h in enumerate(ins):
                ref = R.layer_f64(h[i], w, b)
                bad = R.layer_f64(h[i], w, b, mutant=mutant, kc=kc, prev_last=ins[k - 1][i][:, -1])
                miss = max(miss, float(np.abs(bad - ref).max()) / max(1.0, float(np.abs(ref).max())))
            out[(i, kc)] = miss
    return out


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_caught_at_the_sweep_tolerances(mutant):
    """each defect of the float64 reference, in every layer of the narrow net and in layers 1-5 of the shipped one, misses the
    unmodified reference by more than ten times the bar of the layer it hits (any family can run any layer: the largest bar;
    the F(4,3) tap swap: that family's)"""
    bar = LAYER_TOL["wino4"] if mutant == "wino4_tap_swap" else max(LAYER_TOL.values())
    narrow = R.reads(6)
    cases = ((R.NARROW, range(1, 6), [narrow[k] for k in (0, 1, 2, 40, 41)]),
             (synth.CHANNELS, range(1, 6), [R.reads(12)[k] for k in (0, 1, 2)]))
    for channels, layers, sigs in cases:
        for key, miss in _mutant_misses(channels, layers, sigs, mutant).items():
            assert miss > 10 * bar, (mutant, len(channels), key, miss)


def test_bars_are_inside_the_layerwise_test():
    assert all(t < 2e-4 for t in LAYER_TOL.values())


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _model(variant, dev, extra=None):
    channels, dtype, env, _ = R.VARIANTS[variant]
    return hooked_model({**BASE_ENV, **env, **(extra or {})}, R.state_dict(channels), dtype, dev, config=R.config(channels))


_BATCH = {}


def _batch(n_layers, dev):
    """the ragged batch: rows of LD floats, NaN behind every read"""
    import torch
    if n_layers not in _BATCH:
        sigs = R.reads(n_layers)
        x = torch.full((R.N_READS, R.LD), float("nan"), dtype=torch.float32)
        for k, s in enumerate(sigs):
            x[k, :len(s)] = torch.from_numpy(s)
        _BATCH[n_layers] = (x.to(dev), np.array([len(s) for s in sigs], dtype=np.int32))
    return _BATCH[n_layers]


def _forward(m, dev, layer=None):
    """(probs, logits) of the ragged batch, and the output buffer of conv layer `layer` as the device laid it out"""
    import torch
    x, lens = _batch(m.n_layers, dev)
    cap = None
    if layer is not None:
        cap = torch.full(m.layer_rows(lens, layer)[:2], float("nan"), dtype=torch.float32, device=dev)
    with m.capture_layer(layer, cap) if layer is not None else contextlib.nullcontext():
        probs, logits = m.forward_batch(x, lens, return_logits=True)
        torch.cuda.synchronize(dev)
    return probs, logits, cap


def _families(m):
    """{conv layer: family} of a model, from rs_layer_info"""
    by_div = {spec["row_div"]: f for f, spec in R.FAMILIES.items()}
    return {i: ("direct" if m.dtype == "f32" else by_div[li["gemm_row_div"]]) for i, li in enumerate(m.layer_info()) if i >= 1}


_SWEEP = {}


def _sweep(variant, dev):
    """every table entry of every family of the variant forced onto all its layers: asserts the planner's bits and that the
    force was honoured exactly where it fits; returns the honoured instantiations"""
    if variant not in _SWEEP:
        try:
            _SWEEP[variant] = _run_sweep(variant, dev)
        except BaseException as e:                                            # kept: the coverage test shows it again
            _SWEEP[variant] = e
    if isinstance(_SWEEP[variant], BaseException):
        raise _SWEEP[variant]
    return _SWEEP[variant]


def _run_sweep(variant, dev):
    import torch
    m0 = _model(variant, dev)
    n = m0.n_layers
    fam_of = _families(m0)
    honoured = set()
    for fam in sorted(set(fam_of.values())):
        layers = [i for i in fam_of if fam_of[i] == fam]
        want = _forward(m0, dev, layers[-1])
        info0 = m0.layer_info()
        assert not torch.isnan(want[2]).any() and not torch.isnan(want[1]).any()
        for s in R.parse_shapes(fam):
            for no_deep in ((False, True) if s[4] == "D" else (False,)):
                env = {R.FAMILIES[fam]["hook"]: ";".join("%d:%d,%d,%d,%d" % ((i,) + s[:4]) for i in range(1, n))}
                if no_deep:
                    env["RS_NO_DEEP_STAGING"] = "1"
                m = _model(variant, dev, env)
                got = _forward(m, dev, layers[-1])
                info = m.layer_info()
                m.close()
                for a, b, what in zip(got, want, ("probabilities", "logits", "layer %d" % layers[-1])):
                    assert torch.equal(a, b), (variant, fam, s, "no deep staging" if no_deep else "", what)
                for i in layers:
                    kc, bm, bn = info[i]["kc"], info[i]["bm"], info[i]["bn"]
                    assert R.lds_bytes_of_tile(fam, bm, bn, kc) <= R.LDS_LIMIT, (variant, fam, s, i)
                    if R.fits(fam, s, kc):
                        assert (bm, bn) == R.tile(fam, s), (variant, fam, s, i, kc, bm, bn)
                        honoured.add((fam, s[:4], kc if kc >= 16 else 0, s[4] == "D" and not no_deep))
                    else:                                                     # ignored: the planner's own choice
                        assert (bm, bn) == (info0[i]["bm"], info0[i]["bn"]), (variant, fam, s, i, kc, bm, bn)
    m0.close()
    return honoured


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SWEPT)
def test_every_forced_shape_keeps_the_planners_bits(dev, variant):
    t0 = time.time()
    honoured = _sweep(variant, dev)
    print(f"\nF32_SHAPES {variant}: {len(honoured)} instantiations honoured, {time.time() - t0:.1f} s")
    assert honoured


@pytest.mark.gpu
def test_the_sweep_launches_every_fitting_instantiation(dev):
    got = set().union(*(_sweep(v, dev) for v in SWEPT))
    target = set().union(*(R.instantiations(f) for f in R.FAMILIES))
    assert set(UNREACHABLE) <= target
    assert got == target - set(UNREACHABLE), sorted((target - set(UNREACHABLE)) ^ got)


@pytest.mark.gpu
def test_the_variants_cover_the_channel_edges(dev):
    """per family and chunk size: a ragged last chunk and a whole one, c_in not a multiple of 4, c_out not a multiple of 16;
    per wide shape a layer whose 16-channel column count is not a multiple of the tile's; the direct kernel below 16 channels"""
    seen, n16s = {}, {}
    for v in R.VARIANTS:
        m = _model(v, dev)
        for i, fam in _families(m).items():
            li = m.layer_info()[i]
            key = (fam, li["kc"] if li["kc"] >= 16 else 0)
            seen.setdefault(key, set()).update({"ragged" if li["cp_in"] % li["kc"] else "whole",
                                                "c_in % 4" if li["c_in"] % 4 else "", "c_out % 16" if li["c_out"] % 16 else ""})
            n16s.setdefault(fam, set()).add(-(-li["c_out"] // 16))
        m.close()
    assert set(seen) == {(f, kc) for f, spec in R.FAMILIES.items() for kc in spec["kcs"]}, sorted(seen)
    for key, s in seen.items():
        need = {"whole", "c_in % 4", "c_out % 16"} | ({"ragged"} if key[1] else set())    # a run-time chunk is cut to fit
        assert need <= s, (key, s)
    for fam in R.FAMILIES:
        for s in R.parse_shapes(fam):
            assert s[1] * s[3] == 1 or any(n16 % (s[1] * s[3]) for n16 in n16s[fam]), (fam, s)


_F64 = {}


def _f64_forward(channels):
    """float64 logits of the ragged batch"""
    channels = tuple(channels)
    if channels not in _F64:
        sd = R.state_dict(channels)
        _F64[channels] = np.concatenate([ro.convnet_forward(sd, x[None], acc=np.float64) for x in R.reads(len(channels))])
    return _F64[channels]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_each_layer_against_float64_from_the_devices_own_input(dev, variant):
    channels = R.VARIANTS[variant][0]
    sd = R.state_dict(channels)
    sigs = R.reads(len(channels))
    m = _model(variant, dev)
    fam_of = _families(m)
    lens = _batch(m.n_layers, dev)[1]
    gaps, anchor = {}, {}
    prev = None
    for i in range(1, m.n_layers):
        probs, logits, cap = _forward(m, dev, i)
        li = m.layer_info()[i]
        fam, key = fam_of[i], (fam_of[i], li["kc"])
        got_all = cap.cpu().numpy()
        U, bases = li["block_samples"], m.block_bases(lens, i)
        assert list(np.diff(bases)) == [n // U + 1 for n in lens]
        P_out, P_in = U >> (i + 1), m.layer_info()[i - 1]["block_samples"] >> i
        bases_in = m.block_bases(lens, i - 1)
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        for k, n in enumerate(lens):
            got = got_all[bases[k] * P_out: bases[k + 1] * P_out]
            if i == 1:                                                        # from the normalised signal through layers 0 and 1
                x = ro.conv_block(sigs[k][None, None, :], sd["layers.0.0.weight"], sd["layers.0.0.bias"], acc=np.float64)
                x32 = ro.conv_block(sigs[k][None, None, :], sd["layers.0.0.weight"], sd["layers.0.0.bias"], acc=np.float32)
            else:
                x = prev[bases_in[k] * P_in: bases_in[k] * P_in + (n >> i), :w.shape[1]].T[None]
                x32 = x
            ref = ro.conv_block(x, w, b, acc=np.float64)[0].T                 # [L_out, C]
            ref32 = ro.conv_block(x32, w, b, acc=np.float32)[0].T
            L_out, C = ref.shape
            assert L_out == n >> (i + 1)
            assert not got[L_out:, :].any(), (variant, i, k)                  # padding rows of the read's blocks
            assert not got[:, C:].any(), (variant, i, k)                      # padding channels
            scale = max(1.0, float(np.abs(ref).max()))
            gaps[key] = max(gaps.get(key, 0.0), float(np.abs(got[:L_out, :C] - ref).max()) / scale)
            anchor[key] = max(anchor.get(key, 0.0), float(np.abs(ref32 - ref).max()) / scale)
        prev = got_all
    m.close()
    f64 = _f64_forward(channels)
    dl = float((np.abs(logits.cpu().numpy() - f64) / np.maximum(1.0, np.abs(f64))).max())
    dp = float(np.abs(probs.cpu().numpy() - ro.softmax(f64)).max())
    for key in sorted(gaps):
        print(f"\nF32_SHAPES {variant} {key[0]} kc {key[1]}: max|dev-f64|/scale {gaps[key]:.3e}  numpy fp32 {anchor[key]:.3e}")
    print(f"\nF32_SHAPES {variant} end to end: logits {dl:.3e} probs {dp:.3e}")
    for key, g in gaps.items():
        assert g < LAYER_TOL[key[0]], (variant, key, g)
    assert dl < E2E_TOL["logits"] and dp < E2E_TOL["probs"], (variant, dl, dp)


@pytest.mark.gpu
def test_head_and_tail_launches_and_the_tile_order_keep_the_bits(dev, capfd):
    """576 and 640 reads of 16000 samples (off the multiples of 256, where the split was introduced): the planner of the model of
    record runs F(4,3) layers (both batches) and an F(2,3) layer (layer 11 at 640 reads) as a head and a tail launch of different
    shapes; one launch per layer (RS_NO_TAIL_SPLIT=1) and the plain tile order (RS_NO_RECT_ORDER=1) give the same bits"""
    import torch
    from riser_amd.preprocess import pack_reads
    sd = synth.make_state_dict(R.SEED)
    sigs = list(synth.make_signals(20260103, 640, 16000))
    seen = set()
    for B in (576, 640):
        sig, off, ln, lh = pack_reads(sigs[:B], dev)

        def run(env):
            m = hooked_model(dict(env, RS_TAIL_DEBUG="1"), sd, "f32w", dev)
            capfd.readouterr()
            out = m.classify_raw(sig, off, ln, lh, return_logits=True)
            torch.cuda.synchronize(dev)
            split = [int(v) for v in re.findall(r"\[tail-split\] layer (\d+):", capfd.readouterr().err)]
            divs = {m.layer_info()[i]["gemm_row_div"] for i in split}
            m.close()
            return out, divs

        want, divs = run({})
        print(f"\nF32_SHAPES {B} reads: head + tail launches in families {sorted(divs)}")
        assert divs, B
        seen |= divs
        got, none = run({"RS_NO_TAIL_SPLIT": "1"})
        assert not none
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), B
        got, again = run({"RS_NO_RECT_ORDER": "1"})
        assert again == divs
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), B
    assert seen == {2, 4}, seen
