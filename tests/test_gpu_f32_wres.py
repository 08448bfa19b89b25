"""K3r, the fp32 weights-resident kernel of the narrow tiled Winograd layers (csrc/conv_wres_f32.hip), held to the tiled kernels'
bits and, one layer at a time, to float64.

The kernel claims the bits of conv_wino.hip / conv_wino4.hip.  Small nets (convnet_ref.state_dict / config, not the shipped
widths) run the raw reads of convnet_ref.raw_reads through classify_raw on two models
  wres    RS_WRES_F32=1: K3r on every eligible layer whatever the launch size
  tiled   the reference: RS_WRES_F32=0 RS_SMALL_F32_WAVES=0
with every conv layer from 1 upward captured into a NaN-filled buffer.
  same bits   every layer, read by read through each model's own block layout: valid rows and real channels, logits and
              probabilities byte for byte; padding rows and padding channels exactly zero;
  float64     every K3r layer against conv -> bias -> ReLU -> MaxPool in float64 from the DEVICE's own layer i - 1, at the
              unchanged per-layer bars of the tile-shape sweep (test_gpu_f32_shapes.LAYER_TOL);
  really ran  by the tile report: 16 Winograd units by all padded output channels, (32, 16 n16) for F(2,3) and (64, 16 n16) for
              F(4,3); the expected layers are listed per net (WANT) and asserted; the reference reports none of them there;
  stepped     aside under RS_NO_STREAM_F32=1, under a forced small kernel and under a forced tile shape of the layer.
Cases, by net (layer: c_in -> c_out):
  w2      F(2,3) everywhere.  2: 27 -> 10 two chunks, the last ragged (28 padded channels), c_in % 4 != 0, one column sub-tile
          (the smallest), c_out % 16 != 0; 3: 10 -> 48 one ragged chunk (12), three sub-tiles (the largest); 5: 10 -> 9.  The
          F(2,3) packing never has three chunks of 16 (convnet_model.hpp: plan_static_wino takes two of 24 from 41 channels on).
  w4      F(4,3) on layers 2 - 5 with chunks of 16.  2: 27 -> 10 two chunks, ragged, one sub-tile (the smallest); 3: 10 -> 70 one
          ragged chunk, five sub-tiles (the largest), c_out % 16 != 0; 4: 70 -> 40 five chunks, ragged; 5: 40 -> 9 three
          chunks, ragged.
  deep    twelve layers, F(4,3) on 3, 5, 8, 9: the late layers' blocks hold fewer pooled rows than a step (8, 4, 2, 1), so a
          step spans several blocks and the last one overhangs the buffer (asserted from layer_rows); two and three sub-tiles.
The 77 reads hold the minimum length and + 1, one sample either side of the fine, coarse and doubled block edges (1024, 4096,
8192: convnet_ref.sweep_lengths), blocks whose tail steps are dead and blocks that are dead altogether (a read of k x 1024
samples owns an empty block), and their step counts are no multiple of the eight waves of a workgroup (asserted).  The minimum
read runs alone as well, and five reads run with runs of one and of eight steps per wave (RS_SF32_MIN_RUN)."""
import numpy as np
import pytest

from tests import convnet_ref as R
from tests import test_gpu_f32_shapes as S
from tests import test_gpu_f32_thin as T

from conftest import hooked_model

LAYER_TOL, E2E_TOL = S.LAYER_TOL, S.E2E_TOL                                   # unchanged: no tolerance of this module's own
WRES = {"RS_WRES_F32": "1"}
TILED = {"RS_WRES_F32": "0", "RS_SMALL_F32_WAVES": "0"}
_KC16 = lambda n: ";".join(f"{i}:16" for i in range(1, n))
# net -> (channels, env of the model, {layer: (wino_m, column sub-tiles, chunks)} that K3r must run)
NETS = {
    "w2": ((18, 27, 10, 48, 10, 9), {"RS_WINO4": "none"}, {2: (2, 1, 2), 3: (2, 3, 1), 5: (2, 1, 1)}),
    "w4": ((18, 27, 10, 70, 40, 9), {"RS_WINO4": "2,3,4,5", "RS_PLAN_KC": _KC16(6)},
           {2: (4, 1, 2), 3: (4, 5, 1), 4: (4, 3, 5), 5: (4, 1, 3)}),
    "deep": ((18, 27, 10, 48, 10, 9, 12, 10, 30, 27, 13, 9), {"RS_WINO4": "3,5,8,9", "RS_PLAN_KC": _KC16(12)},
             {2: (2, 1, 2), 3: (4, 3, 1), 5: (4, 1, 1), 6: (2, 1, 1), 7: (2, 1, 1), 8: (4, 2, 1), 9: (4, 2, 2), 10: (2, 1, 2),
              11: (2, 1, 1)}),
}
FAMILY = {2: "wino", 4: "wino4"}


def _tile(m_, nt):
    return (16 * m_, 16 * nt)


def test_the_nets_hold_the_cases():
    """CPU: what the module docstring says of the channel lists, as far as the channels decide it"""
    seen = set()
    for name, (channels, env, want) in NETS.items():
        w4 = set() if env["RS_WINO4"] == "none" else {int(v) for v in env["RS_WINO4"].split(",")}
        for i, (m_, nt, nch) in want.items():
            c_in, c_out = channels[i - 1], channels[i]
            cp_in = -(-c_in // 4) * 4
            assert m_ == (4 if i in w4 else 2) and nt == -(-c_out // 16) and nch == -(-cp_in // 16), (name, i)
            assert nt <= (3 if m_ == 2 else 5)
            if m_ == 2:                                                       # plan_static_wino's chunk of 16
                assert cp_in <= 16 or 25 <= cp_in <= 32, (name, i, cp_in)
            seen.add((m_, nt, nch, cp_in % 16 != 0, c_in % 4 != 0, c_out % 16 != 0))
    for m_, hi in ((2, 3), (4, 5)):
        assert {nt for mm, nt, *_ in seen if mm == m_} >= {1, hi}
        assert any(mm == m_ and rag and nch == 1 for mm, _, nch, rag, _, _ in seen)
        assert any(mm == m_ and rag and nch == 2 for mm, _, nch, rag, _, _ in seen)
        assert any(mm == m_ and c4 for mm, _, _, _, c4, _ in seen) and any(mm == m_ and c16 for mm, *_, c16 in seen)
    assert any(mm == 4 and rag and nch == 3 for mm, _, nch, rag, _, _ in seen)
    lens = R.sweep_lengths(6)
    assert min(lens) == 64 and 65 in lens
    for blk in (1024, 4096, 8192):
        assert any(n % blk == blk - 1 for n in lens) and any(n % blk == 0 for n in lens) and any(n % blk == 1 for n in lens)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _make(net, env, dev):
    channels, nenv, _ = NETS[net]
    return hooked_model({**nenv, **env}, R.state_dict(channels), "f32w", dev, config=R.config(channels))


_OUTS = {}


def _out(net, name, env, dev, which=None):
    """the model `env` of a net on the 77 reads (or the reads `which`), every conv layer captured; run once and kept"""
    key = (net, name, None if which is None else tuple(which))
    if key not in _OUTS:
        n = len(NETS[net][0])
        m = _make(net, env, dev)
        try:
            _OUTS[key] = T._Out(m, T._packed(n, dev, which), dev, range(1, n))
        finally:
            m.close()
    return _OUTS[key]


def _ran(net, info):
    """asserts K3r's tile report on the layers WANT names, and returns them"""
    want = NETS[net][2]
    for i, (m_, nt, nch) in want.items():
        li = info[i]
        assert li["gemm_row_div"] == m_ and li["kc"] == 16 and -(-li["cp_in"] // 16) == nch, (net, i, li)
        assert (li["bm"], li["bn"]) == _tile(m_, nt), (net, i, li)
    return want


def _assert_same(net, got, want, tag):
    channels = NETS[net][0]
    assert not np.isnan(want.logits).any() and not np.isnan(want.probs).any()
    assert T._same(got.probs, want.probs) and T._same(got.logits, want.logits), (net, tag)
    for i in range(1, len(channels)):
        C = channels[i]
        for k, n in enumerate(want.lens):
            a, b = got.rows(i, k), want.rows(i, k)
            L_out = int(n) >> (i + 1)
            assert T._same(a[:L_out, :C], b[:L_out, :C]), (net, tag, "layer", i, "read", k, n)
            assert not a[L_out:, :].any(), (net, tag, "padding rows", i, k, n)
            assert not a[:, C:].any(), (net, tag, "padding channels", i, k, n)


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(NETS))
def test_same_bits_as_the_tiled_kernels(dev, net):
    want, got = _out(net, "tiled", TILED, dev), _out(net, "wres", WRES, dev)
    ran = _ran(net, got.info)
    for i, (m_, nt, _) in ran.items():                                        # the reference ran something else there
        assert (want.info[i]["bm"], want.info[i]["bn"]) != _tile(m_, nt), (net, i, want.info[i])
    print(f"\nF32_WRES {net}: " + " ".join(f"{i}:{li['bm']}x{li['bn']}" for i, li in enumerate(got.info) if i))
    _assert_same(net, got, want, "77 reads")
    # the batch meets the launch-shape cases: step counts that are no multiple of a workgroup's waves, steps that overhang
    n = len(NETS[net][0])
    m = _make(net, WRES, dev)
    try:
        steps = {i: -(-m.layer_rows(want.lens, i)[0] // (8 * m_)) for i, (m_, _, _) in ran.items()}
        over = {i: m.layer_rows(want.lens, i)[0] % (8 * m_) for i, (m_, _, _) in ran.items()}
    finally:
        m.close()
    assert any(s % 8 for s in steps.values()), (net, steps)
    if net == "deep":
        assert any(over.values()), (net, over)
        assert any(got.P_out[i] < 8 * m_ for i, (m_, _, _) in ran.items())
    # dead steps: the last block of some read holds v valid rows of layer i and at least one whole step behind them
    for i, (m_, _, _) in ran.items():
        P, rows, U = got.P_out[i], 8 * m_, got.info[i]["block_samples"]
        if P >= rows:
            assert any(-(-((int(nk) % U) >> (i + 1)) // rows) * rows + rows <= P for nk in want.lens), (net, i)


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(NETS))
def test_each_layer_against_float64_from_the_devices_own_input(dev, net):
    channels = NETS[net][0]
    sd = R.state_dict(channels)
    o = _out(net, "wres", WRES, dev)
    fails = []
    for i, (m_, nt, nch) in _ran(net, o.info).items():
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        xs = [o.rows(i - 1, k)[:int(n) >> i, :w.shape[1]] for k, n in enumerate(o.lens)]
        assert all(np.isfinite(x).all() for x in xs), (net, i)
        ref = [r.T for r in R.layer_f64_reads([x.T for x in xs], w, b)]
        gap = 0.0
        for k, n in enumerate(o.lens):
            r = ref[k]
            assert r.shape == (int(n) >> (i + 1), channels[i])
            got = o.rows(i, k)[:r.shape[0], :r.shape[1]]
            gap = max(gap, float(np.abs(got - r).max(initial=0.0)) / max(1.0, float(np.abs(r).max(initial=0.0))))
        bar = LAYER_TOL[FAMILY[m_]]
        print(f"\nF32_WRES {net} layer {i} F({m_},3) nt {nt} chunks {nch}: max|dev-f64|/scale {gap:.3e} (bar {bar:.0e})")
        if not gap < bar:
            fails.append((net, i, gap, bar))
    f64 = R.forward_f64_reads(sd, R.raw_normalised(len(channels)))
    dl = float((np.abs(o.logits - f64) / np.maximum(1.0, np.abs(f64))).max())
    print(f"\nF32_WRES {net} end to end: logits {dl:.3e} (bar {E2E_TOL['logits']:.1e})")
    if not dl < E2E_TOL["logits"]:
        fails.append((net, "logits", dl))
    assert not fails, fails


def _few(n_layers):
    a = T._alone(n_layers)
    return [a[0], a[1], 30, 50, a[-1]]


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["w2", "w4"])
def test_a_minimum_read_alone_and_forced_run_lengths(dev, net):
    """the minimum-length read alone (one live step, the rest of its block dead), and five reads with runs of one and of eight
    steps per wave: the tiled model's bytes"""
    n = len(NETS[net][0])
    lone = [T._alone(n)[0]]
    want, got = _out(net, "tiled", TILED, dev, lone), _out(net, "wres", WRES, dev, lone)
    assert list(want.lens) == [1 << n]
    _ran(net, got.info)
    _assert_same(net, got, want, "minimum read alone")
    want = _out(net, "tiled", TILED, dev, _few(n))
    for run in ("1", "8"):
        got = _out(net, "runs of " + run, {**WRES, "RS_SF32_MIN_RUN": run}, dev, _few(n))
        _ran(net, got.info)
        _assert_same(net, got, want, "runs of " + run)


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["w2", "w4"])
def test_the_kernel_steps_aside(dev, net):
    """RS_WRES_F32=1 with RS_NO_STREAM_F32=1 (tiled kernels on every layer), with a forced small kernel, and with a forced tile
    shape: none of the layers reports K3r's tile (layer 3: three / five sub-tiles, which the small kernel never reports); and
    the planner's own model leaves a batch of five reads to the small and tiled kernels"""
    n = len(NETS[net][0])
    m_ = NETS[net][2][3][0]
    k3r = _tile(*NETS[net][2][3][:2])
    fam, shape, bm = ("RS_FORCE_SHAPE_WINO", "8,1,2,2", 512) if m_ == 2 else ("RS_FORCE_SHAPE_WINO4", "8,1,1,4", 512)
    want = _out(net, "tiled", TILED, dev, _few(n))
    for tag, env in (("no stream", {"RS_NO_STREAM_F32": "1"}), ("forced small", {"RS_SMALL_F32_WAVES": "100000000", "RS_SMALL_NW": "1"}),
                     ("forced shape", {fam: "3:" + shape, "RS_SMALL_F32_WAVES": "0"}), ("default", None)):
        got = _out(net, tag, {} if env is None else {**WRES, **env}, dev, _few(n))
        li = got.info[3]
        assert (li["bm"], li["bn"]) != k3r, (net, tag, li)
        if tag == "forced small":
            assert (li["bm"], li["bn"]) == (16 * m_, 16), (net, tag, li)
        if tag == "forced shape":
            assert li["bm"] == bm, (net, tag, li)
            assert (got.info[2]["bm"], got.info[2]["bn"]) == _tile(*NETS[net][2][2][:2]), (net, tag, got.info[2])   # layer 2 is not named
        _assert_same(net, got, want, tag)
