"""The tiled F(4,3) kernel (csrc/conv_wino4.hip) on chunks of 20 channels - its 512 x 80 tile on unpadded LDS rows, the k index
swizzled by bit 3 of the row (csrc/conv_wino_device.hpp: wino_unpadded, wino_swizzle) - held to the bits of chunks of 16 and,
one layer at a time, to float64.

The accumulation order of a layer is channels ascending whatever the chunk, and the padding steps add 0 * 0, so the two chunk
sizes claim the same bits.  One 7-layer net (convnet_ref.state_dict / config) with F(4,3) on layers 3 - 5 (c_in -> c_out):
  3: 100 -> 70   five exact chunks of 20 (seven of 16, the last ragged), five column groups, c_out % 16 != 0
  4:  70 -> 45   four chunks, the last ragged (72 padded channels), three column groups, c_out % 16 != 0
  5:  45 -> 67   three chunks, the last ragged (48 padded channels: three exact chunks of 16), five column groups
runs the 77 raw reads of convnet_ref.sweep_lengths (block edges, dead tails, dead blocks) through classify_raw with the tiled
kernels on every such layer (RS_WRES_F32=0 RS_SMALL_F32_WAVES=0), every conv layer captured into a NaN-filled buffer:
  same bits   RS_PLAN_KC forcing 20 ("layer:20u": the chunk with its unpadded tile, as the planner takes it; a plain "layer:20"
              keeps the tiles at the pitch of kc + 2, the set tests/test_gpu_f32_shapes.py sweeps by convnet_ref's mirror of
              that footprint) against RS_PLAN_KC forcing 16 on layers 3 - 5: valid rows and real channels, logits and
              probabilities byte for byte, padding rows and channels exactly zero; the same for every entry of the F(4,3) shape
              table forced onto the three layers at chunks of 20 (RS_FORCE_SHAPE_WINO4; the RS_SHAPE_D entries also without the
              one-item-ahead form): eight waves, one item ahead, four waves;
  really ran  by the tile report: kc == 20 and the forced tile wherever the shape fits the LDS (lds_bytes_20 below: convnet_ref's
              mirror, or the unpadded footprint where only that fits), the planner's own tile where it does not; <8,1,1,5>
              (512 x 80, 159 360 B with unpadded rows) must be among the honoured ones, <8,1,1,6> (512 x 96, 174 720 B even
              unpadded) must not; under a plain "layer:20" <8,1,1,5> is ignored as it always was;
  float64     layers 3 - 5 against conv -> bias -> ReLU -> MaxPool in float64 from the DEVICE's own layer i - 1, the logits and
              probabilities against the float64 forward, at the unchanged bars of the tile-shape sweep
              (test_gpu_f32_shapes.LAYER_TOL / E2E_TOL), for the planner's model and for the forced 512 x 80 tile."""
import numpy as np
import pytest

from oracle import riser_oracle as ro
from tests import convnet_ref as R
from tests import test_gpu_f32_shapes as S
from tests import test_gpu_f32_thin as T

from conftest import hooked_model

LAYER_TOL, E2E_TOL = S.LAYER_TOL, S.E2E_TOL                                   # unchanged: no tolerance of this module's own
CHANNELS = (18, 27, 100, 70, 45, 67, 9)
W4 = (3, 4, 5)
BASE = {"RS_WINO4": ",".join(str(i) for i in W4), "RS_WRES_F32": "0", "RS_SMALL_F32_WAVES": "0"}
_KC = lambda kc: {"RS_PLAN_KC": ";".join(f"{i}:{kc}" for i in W4)}
K20 = "20u"                                                                   # chunks of 20 with the unpadded tile
SHAPES = R.parse_shapes("wino4")
WIDE, TOO_WIDE = (8, 1, 1, 5), (8, 1, 1, 6)


def lds_bytes_20(shape):
    """both LDS buffers of a table entry at chunks of 20: rows of kc + 2 floats (convnet_ref.lds_bytes) where that fits, else
    unpadded rows of kc floats (csrc/conv_wino_device.hpp: wino_unpadded; whether THAT fits is the caller's question)"""
    padded = R.lds_bytes("wino4", shape, 20)
    return padded if padded <= R.LDS_LIMIT else padded // 22 * 20


def fits_20(shape):
    return lds_bytes_20(shape) <= R.LDS_LIMIT


def _force(s):
    return {"RS_FORCE_SHAPE_WINO4": ";".join("%d:%d,%d,%d,%d" % ((i,) + tuple(s[:4])) for i in W4)}


def test_the_net_holds_the_cases():
    """CPU: what the module docstring says of the channel list, and the two sides of the LDS limit in the mirror"""
    want = {3: (5, 0, 5), 4: (4, 12, 3), 5: (3, 8, 5)}                        # chunks of 20, channels of the last one, groups
    for i, (nch, last, n16) in want.items():
        c_in, c_out = CHANNELS[i - 1], CHANNELS[i]
        cp_in = -(-c_in // 4) * 4
        assert -(-cp_in // 20) == nch and cp_in % 20 == last and -(-c_out // 16) == n16, i
    assert CHANNELS[3] % 16 and CHANNELS[4] % 16
    assert -(-100 // 16) == 7 and 100 % 16 and 48 % 16 == 0
    assert R.lds_bytes("wino4", WIDE, 20) == 2 * (4 * 129 + 6 * 80) * 22 * 4 == 175296 > R.LDS_LIMIT   # at the pitch of kc + 2
    assert lds_bytes_20(WIDE) == 2 * (4 * 129 + 6 * 80) * 20 * 4 == 159360 <= R.LDS_LIMIT
    assert lds_bytes_20(TOO_WIDE) == 2 * (4 * 129 + 6 * 96) * 20 * 4 == 174720 > R.LDS_LIMIT           # 512 x 96 fits neither way
    assert fits_20(WIDE) and not fits_20(TOO_WIDE) and R.fits("wino4", TOO_WIDE, 16)
    assert lds_bytes_20((8, 1, 1, 4)) == 2 * (4 * 129 + 6 * 64) * 22 * 4       # a tile that fits at kc + 2 keeps that pitch
    for s in SHAPES:                                                          # only 512 x 80 changes sides
        assert fits_20(s) == (R.fits("wino4", s, 20) or s[:4] == WIDE), s
    assert [s[:4] for s in SHAPES].count(WIDE) == 1 and [s[:4] for s in SHAPES].count(TOO_WIDE) == 1
    kinds = {s[4] for s in SHAPES if fits_20(s)}
    assert kinds == {"", "D", "4"}                                            # eight waves, one item ahead, four waves
    lens = R.sweep_lengths(len(CHANNELS))
    assert len(lens) == 77 and min(lens) == 128
    for blk in (1024, 4096, 8192):
        assert any(n % blk == blk - 1 for n in lens) and any(n % blk == 0 for n in lens) and any(n % blk == 1 for n in lens)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


_OUTS = {}


def _out(name, env, dev, layers=None, keep=True):
    """the model `env` of the net on the 77 reads with the conv layers `layers` (default: all) captured; run once and kept"""
    if name in _OUTS:
        return _OUTS[name]
    n = len(CHANNELS)
    m = hooked_model({**BASE, **env}, R.state_dict(CHANNELS), "f32w", dev, config=R.config(CHANNELS))
    try:
        o = T._Out(m, T._packed(n, dev), dev, range(1, n) if layers is None else layers)
    finally:
        m.close()
    if keep:
        _OUTS[name] = o
    return o


def _assert_same(got, want, tag):
    assert not np.isnan(want.logits).any() and not np.isnan(want.probs).any()
    assert T._same(got.probs, want.probs) and T._same(got.logits, want.logits), tag
    for i in sorted(got.caps):
        C = CHANNELS[i]
        for k, n in enumerate(want.lens):
            a, b = got.rows(i, k), want.rows(i, k)
            L_out = int(n) >> (i + 1)
            assert T._same(a[:L_out, :C], b[:L_out, :C]), (tag, "layer", i, "read", k, n)
            assert not a[L_out:, :].any(), (tag, "padding rows", i, k, n)
            assert not a[:, C:].any(), (tag, "padding channels", i, k, n)


def _report(o):
    return " ".join(f"{i}:kc{li['kc']} {li['bm']}x{li['bn']}" for i, li in enumerate(o.info) if i in W4)


@pytest.mark.gpu
def test_chunks_of_20_have_the_bits_of_chunks_of_16(dev):
    want, got = _out("kc16", _KC(16), dev), _out("kc20", _KC(K20), dev)
    print(f"\nF32_KC20 planner: kc16 {_report(want)} | kc20 {_report(got)}")
    for i in W4:
        assert want.info[i]["gemm_row_div"] == got.info[i]["gemm_row_div"] == 4, i
        assert want.info[i]["kc"] == 16 and got.info[i]["kc"] == 20, i
    _assert_same(got, want, "planner")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d_%d%s" % s)
def test_every_forced_shape_at_chunks_of_20(dev, shape):
    """the table entry forced onto layers 3 - 5 at chunks of 20 (an RS_SHAPE_D entry also under RS_NO_DEEP_STAGING=1): the tile
    report shows it exactly where it fits, and the bits are those of chunks of 16"""
    want, plan = _out("kc16", _KC(16), dev), _out("kc20", _KC(K20), dev)
    fits = fits_20(shape)
    assert fits or shape[:4] != WIDE
    assert not fits or shape[:4] != TOO_WIDE
    for no_deep in ((False, True) if shape[4] == "D" else (False,)):
        tag = "%d,%d,%d,%d%s" % (shape[:4] + (" no deep staging" if no_deep else "",))
        env = {**_KC(K20), **_force(shape), **({"RS_NO_DEEP_STAGING": "1"} if no_deep else {})}
        got = _out("kc20 " + tag, env, dev, W4, keep=False)
        for i in W4:
            li = got.info[i]
            assert li["kc"] == 20 and li["gemm_row_div"] == 4, (tag, i, li)
            ran = [s for s in SHAPES if R.tile("wino4", s) == (li["bm"], li["bn"])]
            assert ran and fits_20(ran[0]), (tag, i, li)
            if fits:
                assert (li["bm"], li["bn"]) == R.tile("wino4", shape), (tag, i, li)
            else:                                                             # ignored: the planner's own choice
                assert (li["bm"], li["bn"]) == (plan.info[i]["bm"], plan.info[i]["bn"]), (tag, i, li)
                assert (li["bm"], li["bn"]) != R.tile("wino4", shape), (tag, i, li)
        _assert_same(got, want, tag)


@pytest.mark.gpu
def test_a_plain_20_keeps_the_padded_tiles(dev):
    """RS_PLAN_KC "layer:20" without the u: 512 x 80 stays out of reach (a force of it is ignored) and the bits are the same"""
    want = _out("kc16", _KC(16), dev)
    plan = _out("kc20 padded", _KC(20), dev, W4, keep=False)
    got = _out("kc20 padded 8,1,1,5", {**_KC(20), **_force(WIDE)}, dev, W4, keep=False)
    for i in W4:
        assert plan.info[i]["kc"] == got.info[i]["kc"] == 20, i
        assert (got.info[i]["bm"], got.info[i]["bn"]) == (plan.info[i]["bm"], plan.info[i]["bn"]) != (512, 80), (i, got.info[i])
    _assert_same(got, want, "plain 20, 8,1,1,5 forced")


def _float64_gaps(o):
    """{layer: max |device - float64| / scale} of layers 3 - 5 from the device's own layer i - 1, and the end-to-end gaps"""
    sd = R.state_dict(CHANNELS)
    gaps = {}
    for i in W4:
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        xs = [o.rows(i - 1, k)[:int(n) >> i, :w.shape[1]] for k, n in enumerate(o.lens)]
        assert all(np.isfinite(x).all() for x in xs), i
        ref = [r.T for r in R.layer_f64_reads([x.T for x in xs], w, b)]
        gap = 0.0
        for k, n in enumerate(o.lens):
            r = ref[k]
            assert r.shape == (int(n) >> (i + 1), CHANNELS[i])
            got = o.rows(i, k)[:r.shape[0], :r.shape[1]]
            gap = max(gap, float(np.abs(got - r).max(initial=0.0)) / max(1.0, float(np.abs(r).max(initial=0.0))))
        gaps[i] = gap
    f64 = R.forward_f64_reads(sd, R.raw_normalised(len(CHANNELS)))
    dl = float((np.abs(o.logits - f64) / np.maximum(1.0, np.abs(f64))).max())
    dp = float(np.abs(o.probs - ro.softmax(f64)).max())
    return gaps, dl, dp


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["planner", "512x80"])
def test_each_layer_against_float64_from_the_devices_own_input(dev, model):
    env = {**_KC(K20), **(_force(WIDE) if model == "512x80" else {})}
    o = _out("f64 " + model, env, dev, range(2, 6), keep=False)                         # layer 2: the input of layer 3
    for i in W4:
        assert o.info[i]["kc"] == 20, (model, i, o.info[i])
        if model == "512x80":
            assert (o.info[i]["bm"], o.info[i]["bn"]) == (512, 80), (model, i, o.info[i])
    gaps, dl, dp = _float64_gaps(o)
    for i, g in gaps.items():
        print(f"\nF32_KC20 {model} layer {i} {o.info[i]['bm']}x{o.info[i]['bn']}: max|dev-f64|/scale {g:.3e} (bar {LAYER_TOL['wino4']:.0e})")
    print(f"\nF32_KC20 {model} end to end: logits {dl:.3e} (bar {E2E_TOL['logits']:.1e}) probs {dp:.3e} (bar {E2E_TOL['probs']:.0e})")
    assert all(g < LAYER_TOL["wino4"] for g in gaps.values()), (model, gaps)
    assert dl < E2E_TOL["logits"] and dp < E2E_TOL["probs"], (model, dl, dp)
