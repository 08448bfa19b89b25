"""The two fp32 kernels that the tile-shape sweep (tests/test_gpu_f32_shapes.py) switches off - K3s, the streaming kernel of
layers 0 + 1 (csrc/conv_stream_f32.hip), and K3m, the small-batch kernel (csrc/conv_small_f32.hip) - held to the tiled kernels'
bits and, one layer at a time, to float64.

Both claim the tiled Winograd kernels' bits.  Per net variant (convnet_ref.THIN_VARIANTS: the shipped and the narrow net as
all-F(2,3) and all-F(4,3) with chunks of 16 and 20, the model of record, and 6-layer nets whose first two layers sit on the
streaming kernel's edges: c0 = 17, 18, 19 below the 20 padded channels, c1 = 13 (one column sub-tile), 29 (a partial second
one), 32) the 77 raw int16 reads of convnet_ref.raw_reads run through classify_raw - the streaming kernel is chosen on the raw
entry point only - on five models:
  tiled     the reference: RS_SMALL_F32_WAVES=0 RS_NO_STREAM_F32=1 (the BASE_ENV of the tile-shape sweep)
  default   the planner's own choice
  forced    RS_SMALL_F32_WAVES=100000000, K3m on every Winograd layer the streaming kernel does not take, in its three forms:
            private input rows (RS_SMALL_SHARED=0), shared rows with one (RS_SMALL_NW=1) and two (RS_SMALL_NW=2) channel
            sub-tiles per wave
with every conv layer from 1 upward captured (Model.capture_layer, the buffer filled with NaN first).
  same bits   default and forced against tiled, read by read through each model's own block_bases: valid rows and real
              channels, probabilities and logits byte for byte; padding rows and padding channels exactly zero;
  float64     every layer of default and forced against conv -> bias -> ReLU -> MaxPool in float64 computed from the DEVICE's
              layer i - 1 output (layer 1: from the oracle's normalised signal through layers 0 and 1), at the UNCHANGED bars
              of the tile-shape sweep (LAYER_TOL, E2E_TOL: a kernel that claims the tiled kernels' bits gets their bars); the
              mutants of convnet_ref miss those bars tenfold on the new channel lists (CPU);
  really ran  K3m by its tile report (32 conv rows for F(2,3), 64 for F(4,3), by 16 channels per sub-tile; no entry of the
              tiled tables reports that: the only one as low is 32 x 128).  K3s reports 32 x round_up(c1, 16), which K3m with the
              matching number of sub-tiles reports too, so it is told apart by DIFFERENCE: the report does not follow
              RS_SMALL_NW (K3m's would), and the RS_NO_STREAM_F32=1 model reports a conv_wino tile for layer 1.  The layouts
              do not differ: block_samples of layers 0 and 1 are the same with and without the streaming kernel (asserted);
  coverage    the (nc, kc, shared, nw) launched by the forced models, over the variants, EQUAL the instantiations read out of
              pick() (convnet_ref.parse_small_instantiations) minus UNREACHABLE; per (nc, kc) a ragged and a whole last chunk,
              c_in % 4 != 0, c_out % 16 != 0 and, with two sub-tiles, an odd number of 16-channel columns;
  thin forms  reads alone (B = 1, Model.classify's regime: the minimum length, + 1, one per rows % 4 class of the last layer,
              16000) give at every layer the bytes of their rows of the 77-read batch; five reads under RS_SF32_MIN_RUN=1
              and =8 keep layer 1 and the logits.
Largest gaps measured on an MI355X next to the bars: see GAPS below."""
import time

import numpy as np
import pytest

from oracle import riser_oracle as ro
from tests import convnet_ref as R
from tests import test_gpu_f32_shapes as S

from conftest import hooked_model

LAYER_TOL, E2E_TOL, BASE_ENV = S.LAYER_TOL, S.E2E_TOL, S.BASE_ENV          # unchanged: no tolerance of this module's own
FORCE = {"RS_SMALL_F32_WAVES": "100000000"}
# form of the small kernel -> (hook, (shared, nw) it launches)
FORMS = {"private": ({"RS_SMALL_SHARED": "0"}, (False, 1)), "nw1": ({"RS_SMALL_NW": "1"}, (True, 1)),
         "nw2": ({"RS_SMALL_NW": "2"}, (True, 2))}
MODELS = {"tiled": BASE_ENV, "default": {}, **{"forced " + f: {**FORCE, **env} for f, (env, _) in FORMS.items()}}
NC_OF_DIV = {2: 4, 4: 6}                      # Winograd components (= waves of a K3m workgroup) by gemm_row_div
SMALL_BM = {2: 32, 4: 64}                     # conv rows of a K3m tile: 16 units of 2 (F(2,3)) or 4 (F(4,3))
FAMILY = {2: "wino", 4: "wino4"}
# instantiations of pick() that no variant can launch, with the reason
UNREACHABLE = {}
# largest |device - float64| / max(1, max |float64|) over every variant, model, layer, read, row and channel, measured on an
# MI355X (profiles/f32_thin_gpu_tests.txt), by (kernel, nc, kc); the bars are LAYER_TOL["wino"] = 7e-6 for nc = 4 and
# LAYER_TOL["wino4"] = 1e-5 for nc = 6.  End to end: logits 2.6e-5 (bar 1.1e-4), probabilities 4.7e-6 (bar 4e-5)
GAPS = {("K3s", 4, 20): 3.2e-7, ("K3m", 4, 16): 3.3e-7, ("K3m", 4, 20): 9.0e-7, ("K3m", 4, 24): 1.8e-6, ("K3m", 6, 16): 2.1e-6,
        ("K3m", 6, 20): 2.1e-6}


# ------------------------------------------------------------------------------------------------ CPU
def test_small_kernel_instantiations_parse():
    inst = R.parse_small_instantiations()
    assert len(inst) == 15
    assert {(nc, kc) for nc, kc, _, _ in inst} == {(4, 16), (4, 20), (4, 24), (6, 16), (6, 20)}
    assert {(sh, nw) for _, _, sh, nw in inst} == {(False, 1), (True, 1), (True, 2)} == {k for _, k in FORMS.values()}
    assert set(UNREACHABLE) <= inst


def test_raw_sweep_lengths_follow_the_rules():
    """the raw reads have the lengths of the normalised sweep (whose rules test_gpu_f32_shapes checks), are tails of the same
    synthetic reads, normalise to something (MAD > 0), and each net's lists meet what its variants need"""
    for n_layers in (12, 6):
        raw, lens = R.raw_reads(n_layers), R.sweep_lengths(n_layers)
        assert [len(r) for r in raw] == lens and len(raw) == R.N_READS == 77
        assert all(r.dtype == np.int16 for r in raw)
        lo = 1 << n_layers
        assert min(lens) == lo and lo + 1 in lens and max(lens) == R.MAX_LEN
        assert {(n >> (n_layers - 1)) % 4 for n in lens} == {0, 1, 2, 3}
        for i in range(n_layers):                                         # F(4,3) unit counts (rows + 3) / 4 with rows % 4 = 1, 2, 3
            assert {(n >> i) % 4 for n in lens} == {0, 1, 2, 3}, i
        assert all(ro.median_mad(r)[1] > 0 for r in raw)
        norm = R.raw_normalised(n_layers)
        assert all(x.dtype == np.float32 and len(x) == n and np.isfinite(x).all() for x, n in zip(norm, lens))
        assert _alone(n_layers)[:2] == [lens.index(lo), lens.index(lo + 1)] and len(set(_alone(n_layers))) == 7
    # a raw read is normalised by ITS OWN median: not the tail of the normalised long read
    assert not np.array_equal(R.raw_normalised(6)[0], R.reads(6)[0])
    for v in R.THIN_VARIANTS:
        channels = R.THIN_VARIANTS[v][0]
        assert R.THIN_VARIANTS[v][1] == "f32w" and len(channels) in (6, 12)
        if v.startswith("stream_"):                                       # conv_stream_f32_ok, as far as the channels decide it
            assert 16 < channels[0] <= 20 and channels[1] <= 32 and channels[2:] == R.NARROW[2:]
            assert "1" not in R.THIN_VARIANTS[v][2].get("RS_WINO4", "").split(",")
    c01 = {R.THIN_VARIANTS[v][0][:2] for v in R.THIN_STREAMING}
    assert any(c0 < 20 for c0, _ in c01) and any(c0 == 20 for c0, _ in c01)
    assert any(c1 <= 16 for _, c1 in c01) and any(16 < c1 < 32 for _, c1 in c01) and any(c1 == 32 for _, c1 in c01)


def test_batched_reference_is_the_layer_reference():
    """convnet_ref.layer_f64_reads / forward_f64_reads (one product per tap for all reads) against layer_f64 and the oracle"""
    channels = R.THIN_VARIANTS["stream_19_29"][0]
    sd = R.state_dict(channels)
    xs = [R.raw_normalised(6)[k] for k in (0, 1, 2, 40)]
    hs = [np.asarray(x, dtype=np.float64)[None, :] for x in xs]
    for i in range(6):
        w, b = sd[f"layers.{i}.0.weight"], sd[f"layers.{i}.0.bias"]
        got = R.layer_f64_reads(hs, w, b)
        for g, h in zip(got, hs):
            want = R.layer_f64(h, w, b)
            assert g.shape == want.shape and np.abs(g - want).max(initial=0.0) <= 1e-13 * max(1.0, np.abs(want).max(initial=0.0)), i
        hs = got
    want = np.concatenate([ro.convnet_forward(sd, x[None], acc=np.float64) for x in xs])
    assert np.abs(R.forward_f64_reads(sd, xs) - want).max() < 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_caught_on_the_new_channel_lists(mutant):
    """the defects of the float64 reference that the tile-shape sweep proves against its bars, in every layer of the nets this
    module adds: they miss the unmodified reference by more than ten times the bar (F(2,3) or F(4,3) can run any layer but
    layer 1: the larger bar; the F(4,3) tap swap: that family's)"""
    bar = LAYER_TOL["wino4"] if mutant == "wino4_tap_swap" else max(LAYER_TOL["wino"], LAYER_TOL["wino4"])
    sigs = [R.raw_normalised(6)[k] for k in (0, 1, 2, 40, 41)]
    for channels in sorted({R.THIN_VARIANTS[v][0] for v in R.THIN_VARIANTS if v.startswith("stream_")}):
        for key, miss in S._mutant_misses(channels, range(1, 6), sigs, mutant).items():
            assert miss > 10 * bar, (mutant, channels, key, miss)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda", 0)


def _alone(n_layers):
    """the reads that also run alone: the minimum length, + 1, one per rows % 4 class of the last layer, 16000"""
    lens = R.sweep_lengths(n_layers)
    lo = 1 << n_layers
    pick = [lens.index(lo), lens.index(lo + 1)]
    for r in range(4):
        pick.append(next(k for k, n in enumerate(lens) if k not in pick and n != R.MAX_LEN and (n >> (n_layers - 1)) % 4 == r))
    return pick + [lens.index(R.MAX_LEN)]


_PACKED = {}


def _packed(n_layers, dev, which=None):
    """pack_reads of the raw reads (all 77, back to back, or the reads `which`)"""
    from riser_amd.preprocess import pack_reads
    key = (n_layers, None if which is None else tuple(which))
    if key not in _PACKED:
        raw = R.raw_reads(n_layers)
        _PACKED[key] = pack_reads(raw if which is None else [raw[k] for k in which], dev)
    return _PACKED[key]


def _make(variant, env, dev):
    channels, dtype, venv, _ = R.THIN_VARIANTS[variant]
    return hooked_model({**venv, **env}, R.state_dict(channels), dtype, dev, config=R.config(channels))


class _Out:
    """what one model made of one batch: probabilities, logits, layer_info and every captured layer as the device laid it out"""

    def __init__(self, m, batch, dev, layers):
        import torch
        sig, off, ln, lens = batch
        self.lens, self.caps, self.bases, self.P_out = lens, {}, {}, {}
        self.probs = self.logits = None
        for i in list(layers) or [None]:
            cap = None
            if i is not None:
                cap = torch.full(m.layer_rows(lens, i)[:2], float("nan"), dtype=torch.float32, device=dev)
                with m.capture_layer(i, cap):
                    probs, logits = m.classify_raw(sig, off, ln, lens, return_logits=True)
                    torch.cuda.synchronize(dev)
            else:
                probs, logits = m.classify_raw(sig, off, ln, lens, return_logits=True)
            probs, logits = probs.cpu().numpy(), logits.cpu().numpy()
            if self.probs is not None:                                   # the capture changes nothing
                assert _same(probs, self.probs) and _same(logits, self.logits), i
            self.probs, self.logits = probs, logits
            if i is not None:
                self.caps[i] = cap.cpu().numpy()
        self.info = m.layer_info()
        for i in self.caps:
            self.bases[i] = m.block_bases(lens, i)
            self.P_out[i] = self.info[i]["block_samples"] >> (i + 1)
            assert list(np.diff(self.bases[i])) == [n // self.info[i]["block_samples"] + 1 for n in lens]
            assert self.caps[i].shape[0] == self.bases[i][-1] * self.P_out[i]

    def rows(self, i, k):
        """read k's blocks of layer i's output"""
        return self.caps[i][self.bases[i][k] * self.P_out[i]: self.bases[i][k + 1] * self.P_out[i]]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _kernels(variant, info):
    """{conv layer: (kernel, nc, kc)} of a model that has run: "K3s" where the streaming kernel is expected and its report is
    there, "K3m" by the small kernel's tile, else "tiled" """
    out = {}
    for i in range(1, len(info)):
        li = info[i]
        div = li["gemm_row_div"]
        if i == 1 and variant in R.THIN_STREAMING and (li["bm"], li["bn"]) == (32, -(-li["c_out"] // 16) * 16):
            out[i] = ("K3s", 4, li["kc"])
        elif li["bm"] == SMALL_BM[div] and li["bn"] in (16, 32):
            out[i] = ("K3m", NC_OF_DIV[div], li["kc"])
        else:
            out[i] = ("tiled", NC_OF_DIV[div], li["kc"])
    return out


# what the forced models launched: variant -> {(nc, kc, shared, nw)}; (nc, kc) -> edges met; (c0, c1) of streaming launches
_REACHED, _EDGES, _STREAMED = {}, {}, set()


def _note_forced(variant, form, info):
    """asserts that a forced model ran K3m (by its tile report) on every layer but a streamed layer 1, and K3s there"""
    shared, nw = FORMS[form][1]
    for i in range(1, len(info)):
        li = info[i]
        div, n16 = li["gemm_row_div"], -(-li["c_out"] // 16)
        if i == 1 and variant in R.THIN_STREAMING:
            # conv_stream_f32_ok, from the report
            assert div == 2 and li["cp_in"] == 20 and li["kc"] == 20 and li["c_in"] <= 20 and li["c_out"] <= 32, (variant, li)
            assert info[0]["block_samples"] >> 1 >= 64
            assert (li["bm"], li["bn"]) == (32, 16 * n16), (variant, form, li)          # whatever RS_SMALL_NW says
            _STREAMED.add((li["c_in"], li["c_out"]))
            continue
        assert (li["bm"], li["bn"]) == (SMALL_BM[div], 16 * nw), (variant, form, i, li)
        nc, kc = NC_OF_DIV[div], li["kc"]
        _REACHED.setdefault(variant, set()).add((nc, kc, shared, nw))
        e = _EDGES.setdefault((nc, kc), set())
        e.update({"ragged" if li["cp_in"] % kc else "whole", "c_in % 4" if li["c_in"] % 4 else "", "c_out % 16" if li["c_out"] % 16 else ""})
        if nw == 2 and n16 % 2:
            e.add("nw 2, odd columns")


class _Variant:
    """the five models of a variant on the 77-read batch, each run once and kept while the variant's tests run"""

    def __init__(self, variant, dev):
        self.variant, self.dev = variant, dev
        self.channels = R.THIN_VARIANTS[variant][0]
        self.n = len(self.channels)
        self.sd = R.state_dict(self.channels)
        self.lens = R.sweep_lengths(self.n)
        self._outs, self._ref = {}, {}

    def out(self, name, capture=True):
        key = (name, capture)
        if (name, True) in self._outs:
            return self._outs[(name, True)]
        if key not in self._outs:
            m = _make(self.variant, MODELS[name], self.dev)
            try:
                self._outs[key] = _Out(m, _packed(self.n, self.dev), self.dev, range(1, self.n) if capture else ())
            finally:
                m.close()
            if name.startswith("forced "):
                _note_forced(self.variant, name[len("forced "):], self._outs[key].info)
        return self._outs[key]

    def reference(self, o, i):
        """float64 layer i of every read from o's own layer i - 1 (layer 1: from the normalised signal through layers 0 and 1):
        [k] = [L_out, C_out].  Computed once per distinct input: models whose layer i - 1 has the same bytes share it"""
        w, b = self.sd[f"layers.{i}.0.weight"], self.sd[f"layers.{i}.0.bias"]
        if i == 1:
            xs = [np.asarray(x, dtype=np.float64)[None, :] for x in R.raw_normalised(self.n)]
            if 1 not in self._ref:
                h = R.layer_f64_reads(xs, self.sd["layers.0.0.weight"], self.sd["layers.0.0.bias"])
                self._ref[1] = [(None, [r.T for r in R.layer_f64_reads(h, w, b)])]
            return self._ref[1][0][1]
        xs = [o.rows(i - 1, k)[:n >> i, :w.shape[1]] for k, n in enumerate(self.lens)]
        for seen, ref in self._ref.setdefault(i, []):
            if all(np.array_equal(a, c) for a, c in zip(xs, seen)):
                return ref
        assert all(np.isfinite(x).all() for x in xs), (self.variant, i)
        ref = [r.T for r in R.layer_f64_reads([x.T for x in xs], w, b)]
        self._ref[i].append((xs, ref))
        return ref


@pytest.fixture(scope="module", params=list(R.THIN_VARIANTS))
def thin(request, dev):
    return _Variant(request.param, dev)


@pytest.mark.gpu
def test_same_bits_layer_by_layer(thin):
    """default and forced against tiled: valid rows and real channels, probabilities, logits byte for byte, read by read through
    each model's own block layout; padding rows and channels exactly zero (the capture buffer starts as NaN); and the kernel
    under test really ran (module docstring: really ran)"""
    t0 = time.time()
    want = thin.out("tiled")
    v = thin.variant
    kern = _kernels(v, want.info)
    assert set(k for k, _, _ in kern.values()) == {"tiled"}, (v, kern)
    for fam in ("wino", "wino4"):                                            # no tiled shape reports K3m's (or K3s's) tile
        tiles = {R.tile(fam, s) for s in R.parse_shapes(fam)}
        assert not tiles & {(SMALL_BM[R.FAMILIES[fam]["row_div"]], bn) for bn in (16, 32)}, (fam, sorted(tiles))
    assert not np.isnan(want.logits).any() and not np.isnan(want.probs).any()
    for name in MODELS:
        got = thin.out(name)
        kern = _kernels(v, got.info)
        print(f"\nF32_THIN {v} {name}: " + " ".join(f"{i}:{k}/{nc}x{kc}/{got.info[i]['bm']}x{got.info[i]['bn']}" for i, (k, nc, kc) in kern.items()))
        if name == "default" and v in R.THIN_STREAMING:
            assert kern[1][0] == "K3s", (v, got.info[1])
            assert _kernels(v, want.info)[1][0] == "tiled"                       # RS_NO_STREAM_F32=1: a conv_wino tile
            assert [got.info[i]["block_samples"] for i in (0, 1)] == [want.info[i]["block_samples"] for i in (0, 1)]
        assert _same(got.probs, want.probs), (v, name)
        assert _same(got.logits, want.logits), (v, name)
        for i in range(1, thin.n):
            C = thin.channels[i]
            for k, n in enumerate(thin.lens):
                a, b = got.rows(i, k), want.rows(i, k)
                L_out = n >> (i + 1)
                assert _same(a[:L_out, :C], b[:L_out, :C]), (v, name, "layer", i, "read", k, n, kern[i])
                assert not a[L_out:, :].any(), (v, name, "padding rows", i, k, n, kern[i])
                assert not a[:, C:].any(), (v, name, "padding channels", i, k, n, kern[i])
    print(f"\nF32_THIN {v}: {len(MODELS) - 1} models x {thin.n - 1} layers x {len(thin.lens)} reads equal the tiled bits, {time.time() - t0:.1f} s")


_F64 = {}


@pytest.mark.gpu
def test_each_layer_against_float64_from_the_devices_own_input(thin):
    """default and forced, every layer: one kernel's error against float64, at the tile-shape sweep's bars"""
    t0 = time.time()
    v = thin.variant
    if thin.channels not in _F64:
        _F64[thin.channels] = R.forward_f64_reads(thin.sd, R.raw_normalised(thin.n))
    f64 = _F64[thin.channels]
    worst, fails = {}, []
    for name in [m for m in MODELS if m != "tiled"]:
        o = thin.out(name)
        kern = _kernels(v, o.info)
        for i in range(1, thin.n):
            ref = thin.reference(o, i)
            fam = FAMILY[o.info[i]["gemm_row_div"]]
            gap = 0.0
            for k, n in enumerate(thin.lens):
                r = ref[k]
                L_out, C = r.shape
                assert L_out == n >> (i + 1) and C == thin.channels[i]
                got = o.rows(i, k)[:L_out, :C]
                gap = max(gap, float(np.abs(got - r).max(initial=0.0)) / max(1.0, float(np.abs(r).max(initial=0.0))))
            print(f"\nF32_THIN {v} {name} layer {i} {kern[i][0]} nc {kern[i][1]} kc {kern[i][2]}: max|dev-f64|/scale {gap:.3e} (bar {LAYER_TOL[fam]:.0e})")
            worst[kern[i]] = max(worst.get(kern[i], 0.0), gap)
            if not gap < LAYER_TOL[fam]:
                fails.append((v, name, i, kern[i], gap))
        dl = float((np.abs(o.logits - f64) / np.maximum(1.0, np.abs(f64))).max())
        dp = float(np.abs(o.probs - ro.softmax(f64)).max())
        print(f"\nF32_THIN {v} {name} end to end: logits {dl:.3e} (bar {E2E_TOL['logits']:.1e}) probs {dp:.3e} (bar {E2E_TOL['probs']:.0e})")
        if not (dl < E2E_TOL["logits"] and dp < E2E_TOL["probs"]):
            fails.append((v, name, "end to end", dl, dp))
    for key in sorted(worst):
        print(f"\nF32_THIN {v} {key[0]} nc {key[1]} kc {key[2]}: max|dev-f64|/scale {worst[key]:.3e}")
    print(f"\nF32_THIN {v}: float64 in {time.time() - t0:.1f} s")
    assert not fails, fails


@pytest.mark.gpu
def test_a_read_alone_has_the_bytes_of_its_rows_in_the_batch(thin):
    """B = 1 on the default model (Model.classify's regime: the planner takes K3m where the 77-read batch ran tiled kernels):
    every layer, the probabilities and the logits of a read alone against its rows of the 77-read batch of the tiled model"""
    want = thin.out("tiled")
    v = thin.variant
    m = _make(v, {}, thin.dev)
    try:
        ran = set()
        for k in _alone(thin.n):
            n = thin.lens[k]
            o = _Out(m, _packed(thin.n, thin.dev, [k]), thin.dev, range(1, thin.n))
            kern = _kernels(v, o.info)
            ran |= {kk[0] for kk in kern.values()}
            assert _same(o.probs[0], want.probs[k]) and _same(o.logits[0], want.logits[k]), (v, k, n)
            for i in range(1, thin.n):
                a, b = o.rows(i, 0), want.rows(i, k)
                L_out, C = n >> (i + 1), thin.channels[i]
                assert _same(a[:L_out, :C], b[:L_out, :C]), (v, "layer", i, "read", k, n, kern[i])
                assert not a[L_out:, :].any() and not a[:, C:].any(), (v, "padding", i, k, n, kern[i])
        print(f"\nF32_THIN {v} reads alone {[thin.lens[k] for k in _alone(thin.n)]}: kernels {sorted(ran)}, 16000 samples: "
              + " ".join(f"{i}:{kk[0]}" for i, kk in kern.items()))
        assert "K3m" in ran, (v, ran)                                      # the regime the small kernel was written for
        assert ("K3s" in ran) == (v in R.THIN_STREAMING), (v, ran)
    finally:
        m.close()


_STREAM_NEW = [v for v in R.THIN_VARIANTS if v.startswith("stream_")]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", _STREAM_NEW)
def test_streaming_run_lengths_keep_the_bits(dev, variant):
    """five reads: a wave of the streaming kernel takes runs of one (RS_SF32_MIN_RUN=1), of eight (=8) or what the launch size
    says - layer 1 and the logits keep their bits, which are the tiled model's; and the planner's own model DID stream: its
    layer-1 report is 32 x round_up(c1, 16) with RS_SMALL_NW set to the OTHER number of sub-tiles (K3m would follow the hook)"""
    channels = R.THIN_VARIANTS[variant][0]
    n = len(channels)
    which = [_alone(n)[0], _alone(n)[1], 30, 50, _alone(n)[-1]]
    batch = _packed(n, dev, which)
    outs = {}
    n16 = -(-channels[1] // 16)
    for name, env in (("tiled", BASE_ENV), ("default", {}), ("runs of 1", {"RS_SF32_MIN_RUN": "1"}), ("runs of 8", {"RS_SF32_MIN_RUN": "8"}),
                      ("other nw", {"RS_SMALL_NW": str(3 - n16)})):
        m = _make(variant, env, dev)
        try:
            outs[name] = _Out(m, batch, dev, [1])
        finally:
            m.close()
        li = outs[name].info[1]
        if name == "tiled":
            assert (li["bm"], li["bn"]) != (32, 16 * n16), li
        else:
            assert (li["bm"], li["bn"]) == (32, 16 * n16), (variant, name, li)
    want = outs["tiled"]
    for name, o in outs.items():
        assert _same(o.logits, want.logits) and _same(o.probs, want.probs), (variant, name)
        for k, nk in enumerate(want.lens):
            a, b = o.rows(1, k), want.rows(1, k)
            assert _same(a[:nk >> 2, :channels[1]], b[:nk >> 2, :channels[1]]), (variant, name, k, nk)
            assert not a[nk >> 2:, :].any() and not a[:, channels[1]:].any(), (variant, name, k, nk)


@pytest.mark.gpu
def test_the_forced_models_launch_every_instantiation(dev):
    """coverage is asserted: the union over the variants EQUALS pick()'s set minus UNREACHABLE, every (nc, kc) meets its edges,
    and the streaming kernel was seen on both sides of each of its own"""
    for v in R.THIN_VARIANTS:
        tv = _Variant(v, dev)
        for f in FORMS:
            if not any(k[2:] == FORMS[f][1] for k in _REACHED.get(v, ())):
                tv.out("forced " + f, capture=False)
    got = set().union(*_REACHED.values())
    target = R.parse_small_instantiations()
    print(f"\nF32_THIN instantiations launched: {len(got)} of {len(target)} in pick(), unreachable {sorted(UNREACHABLE)}")
    for v in R.THIN_VARIANTS:
        print(f"\nF32_THIN {v}: {sorted(_REACHED[v])}")
    assert set(UNREACHABLE) <= target
    assert got == target - set(UNREACHABLE), sorted((target - set(UNREACHABLE)) ^ got)
    assert set(_EDGES) == {(nc, kc) for nc, kc, _, _ in target}
    for key, e in sorted(_EDGES.items()):
        print(f"\nF32_THIN edges {key}: {sorted(x for x in e if x)}")
        assert {"ragged", "whole", "c_in % 4", "c_out % 16", "nw 2, odd columns"} <= e, (key, e)
    print(f"\nF32_THIN streamed (c0, c1): {sorted(_STREAMED)}")
    assert any(c0 < 20 for c0, _ in _STREAMED) and any(c0 == 20 for c0, _ in _STREAMED), _STREAMED
    assert any(c1 <= 16 for _, c1 in _STREAMED) and any(16 < c1 < 32 for _, c1 in _STREAMED) and any(c1 == 32 for _, c1 in _STREAMED), _STREAMED
