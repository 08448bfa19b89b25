"""Training at any depth and any odd kernel (riser_amd.train.GenericTrainer, rs_train_create_generic) without a GPU: the
float64 reference the device tests lean on (train_ref) and what it gave for the shipped class before it was the only one, the
configs taken and refused, the handle's argument checks and the plans."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import train_ref as R
from riser_amd import synth

MiB = 1 << 20


def config_of(channels, kernels, depth=1, **over):
    cnn = synth.CnnConfig(channels=channels, kernels=kernels, depth=depth)
    for k in [k for k in over if hasattr(cnn, k)]:
        setattr(cnn, k, over.pop(k))
    return types.SimpleNamespace(**{"model": "cnn", "learning_rate": 1e-3, "cnn": cnn, **over})


@pytest.fixture(scope="module")
def lib():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    return nv.lib()


def test_configs_taken_and_refused(lib):
    from riser_amd import train as T
    ch = [8, 12]
    assert T.check_generic_config(config_of(ch, [5, 7], 3)) == (ch, [5, 7], 3)
    assert T.check_generic_config(config_of(ch, [3, 3], 1)) == (ch, [3, 3], 1)
    assert T.check_generic_config(config_of(ch, [1, 9], 2)) == (ch, [1, 9], 2)
    for cfg, match in ((config_of(ch, [3, 4], 2), "even"), (config_of(ch, [3, 5], 2, classifier="fc"), "classifier"),
                       (config_of(ch, [3, 5], 2, classifier="gap"), "classifier"), (config_of(ch, [3, 5], 2, model="tcn"), "model"),
                       (config_of(ch, [3, 5], 2, dtype="bf16x3"), "dtype"), (config_of(ch, [3, 5], 0), "depth"),
                       (config_of(ch, [3], 2), "shorter"), (config_of(ch, [3, 5], 2, n_classes=3), "two-class")):
        for fn in (T.check_generic_config, T.GenericTrainer, T.trainer_for):
            with pytest.raises(ValueError, match=match):    # a ValueError, not the NativeError of a missing device
                fn(cfg)
    with pytest.raises(ValueError, match="dtype"):
        T.GenericTrainer(config_of(ch, [3, 5], 2), dtype="bf16")
    sd = R.make_state(ch, [3, 5], 2, 1)
    with pytest.raises(ValueError, match="layers.1.2.weight"):
        T.GenericTrainer(config_of(ch, [3, 5], 2), {k: v for k, v in sd.items() if k != "layers.1.2.weight"})
    with pytest.raises(ValueError, match="layers.1.0.weight"):         # kernel 5 where the config says 7
        T.trainer_for(config_of(ch, [3, 7], 2), sd)
    # what the shipped class's entry points refuse stays refused there, and trainer_for routes: with a complete state both
    # get as far as asking for a device
    from riser_amd import _native as nv
    from riser_amd.train import Trainer
    with pytest.raises(ValueError, match="depth"):
        Trainer(config_of(ch, [3, 3], 2))
    if lib.rs_device_count() < 1:
        with pytest.raises(nv.NativeError, match="no HIP device"):
            T.trainer_for(config_of(ch, [3, 5], 2), sd)
        with pytest.raises(nv.NativeError, match="no HIP device"):
            T.trainer_for(config_of(ch, [3, 3], 1), R.make_state(ch, [3, 3], 1, 1))
    assert T.is_shipped_class(config_of(ch, [3, 3], 1)) and not T.is_shipped_class(config_of(ch, [3, 3], 2))
    assert not T.is_shipped_class(config_of(ch, [3, 5], 1))


def test_state_dict_layout_is_the_inference_familys(lib):
    from riser_amd import train as T
    from riser_amd.gconv import build_gconv_program
    channels, kernels, depth = [3, 7, 18], [5, 3, 7], 2
    cfg = config_of(channels, kernels, depth)
    keys, shapes = T.param_keys(3, depth), T.param_shapes(channels, kernels, depth)
    assert keys[:4] == ["layers.0.0.weight", "layers.0.0.bias", "layers.0.2.weight", "layers.0.2.bias"]
    assert keys[-2:] == ["classifier.2.weight", "classifier.2.bias"] and len(keys) == 2 * 6 + 2 and list(shapes) == keys
    assert shapes["layers.0.0.weight"] == (3, 1, 5) and shapes["layers.0.2.weight"] == (3, 3, 5)
    assert shapes["layers.2.2.weight"] == (18, 18, 7) and shapes["classifier.2.weight"] == (2, 18)
    sd = T.init_state(channels, kernels, depth)
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    prog = build_gconv_program(sd, cfg.cnn)
    assert [tuple(cv["w"].shape) for cv in prog["convs"]] == [shapes[k] for k in keys[:-2:2]]
    assert (prog["n_layers"], prog["depth"]) == (3, depth)
    assert {k: v.shape for k, v in R.make_state(channels, kernels, depth, 1).items()} == shapes
    # the defaults are the shipped class: depth 1, every kernel 3
    assert T.param_keys(4, 1) == T.param_keys(4) == [f"layers.{i}.0.{w}" for i in range(4) for w in ("weight", "bias")] + keys[-2:]
    assert T.param_shapes([3, 7], [3, 3], 1) == T.param_shapes([3, 7])


def create_generic(lib, convs, n_layers, depth, device=10 ** 6):
    from riser_amd.gconv import _Conv
    w, b = np.zeros(64 * 64 * 9, np.float32), np.zeros(64, np.float32)
    arr = (_Conv * len(convs))(*[_Conv(ci, co, k, 0, w.ctypes.data, b.ctypes.data) for ci, co, k in convs])
    h = C.c_void_p()
    rc = lib.rs_train_create_generic(arr, n_layers, depth, w.ctypes.data, b.ctypes.data, device, C.byref(h))
    return rc, lib.rs_last_error(), h


def test_handle_checks_without_gpu(lib):
    from riser_amd import _native as nv
    # device 1 000 000 does not exist: a refusal that names the argument was made without asking for it
    for convs, n_layers, depth, word in (([(1, 8, 4)], 1, 1, b"even kernel 4"), ([(1, 8, 3), (8, 8, 6)], 1, 2, b"even kernel 6"),
                                         ([(1, 8, 5), (9, 8, 5)], 1, 2, b"chained"), ([(1, 8, 5), (8, 6, 5), (8, 6, 5)], 1, 3, b"chained"),
                                         ([(1, 8, 5)], 1, 0, b"depth 1-64"), ([(1, 8, 5)], 1, 65, b"depth 1-64"),
                                         ([(1, 8, 5)] + [(8, 8, 5)] * 16, 17, 1, b"17 layers"), ([(1, 8, 0)], 1, 1, b"k >= 1")):
        rc, msg, h = create_generic(lib, convs, n_layers, depth)
        assert rc == nv.RS_ERR_ARG and word in msg and not h.value, (convs, msg)
    assert lib.rs_train_create_generic(None, 1, 1, None, None, 0, None) == nv.RS_ERR_ARG
    rc, msg, h = create_generic(lib, [(1, 8, 5), (8, 8, 5), (8, 6, 7), (6, 6, 7)], 2, 2, device=-1)
    assert rc == nv.RS_OK and h.value
    try:
        n, s = C.c_int32(), C.c_int32()
        p, buf = 4096, np.zeros(512, np.float32)
        assert lib.rs_train_workspace_bytes(h, 3, 100) > 0 and lib.rs_train_workspace_bytes(h, 3, 3) == 0      # two pools
        assert lib.rs_train_max_batch(h, 100) >= 3 and lib.rs_train_max_batch(h, 3) == 0
        assert lib.rs_train_slice_plan(h, 3, 3, 100, C.byref(n), C.byref(s)) == nv.RS_OK                      # conv indices 0 .. 3
        assert lib.rs_train_slice_plan(h, 4, 3, 100, C.byref(n), C.byref(s)) == nv.RS_ERR_ARG
        for fn in (lib.rs_train_get_params, lib.rs_train_get_grads, lib.rs_train_set_params):
            assert fn(h, 10, buf.ctypes.data, 2) == nv.RS_ERR_ARG            # tensors 0 .. 9: four convs and the head
            assert fn(h, 2, buf.ctypes.data, 8 * 8 * 3) == nv.RS_ERR_ARG     # conv 1's weight has 8 x 8 x 5 elements
            assert fn(h, 2, buf.ctypes.data, 8 * 8 * 5) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
            assert fn(h, 4, buf.ctypes.data, 6 * 8 * 7) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
            assert fn(h, 8, buf.ctypes.data, 12) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
        assert lib.rs_train_debug_copy(h, 4, 0, p, 64) == nv.RS_ERR_ARG
        assert lib.rs_train_debug_copy(h, 0, 1, p, 64) == nv.RS_ERR_ARG and b"no selectors" in lib.rs_last_error()
        assert lib.rs_train_debug_copy(h, 1, 1, p, 64) == nv.RS_ERR_ARG and b"no rs_train_forward_backward" in lib.rs_last_error()
        big = 1 << 40
        assert lib.rs_train_forward_backward(h, p, p, 3, 3, 3, p, big, p, None) == nv.RS_ERR_LENGTH
        need = lib.rs_train_workspace_bytes(h, 3, 100)
        assert lib.rs_train_forward_backward(h, p, p, 3, 100, 100, p, need - 1, p, None) == nv.RS_ERR_WORKSPACE
        assert lib.rs_train_forward_backward(h, p, p, 3, 100, 100, p, need, p, None) == nv.RS_ERR_ARG
        assert b"without a device" in lib.rs_last_error()
    finally:
        assert lib.rs_train_destroy(h) == nv.RS_OK


def plan_handle(channels, kernels, depth):
    from riser_amd.train import create_handle
    return create_handle(channels, R.make_state(channels, kernels, depth, 1), -1, kernels, depth, generic=True)


def test_slice_plan_and_workspace(lib):
    n, s = C.c_int32(), C.c_int32()
    channels, kernels, depth, B, L, _ = R.CASES["slices"]
    h = plan_handle(channels, kernels, depth)
    try:
        for j, (level, ci, co, k) in enumerate(R.convs_of(channels, kernels, depth)):
            assert lib.rs_train_slice_plan(h, j, B, L, C.byref(n), C.byref(s)) == 0
            assert (n.value, s.value) == R.slice_plan(B, L, level, ci, co, k), j
        assert lib.rs_train_slice_plan(h, 0, B, L, C.byref(n), C.byref(s)) == 0
        assert n.value >= 3 and s.value % 4 == 0 and (n.value - 1) * s.value < B * L < n.value * s.value
        assert lib.rs_train_slice_plan(h, 1, B, L, C.byref(n), C.byref(s)) == 0 and n.value * s.value > B * L   # level 0 too
        assert lib.rs_train_slice_plan(h, 2, B, L, C.byref(n), C.byref(s)) == 0 and n.value * s.value < B * L   # behind a pool
    finally:
        lib.rs_train_destroy(h)
    # the shipped channel list at depth 2, kernel 5 and 32 x 16000: the bound bites with k in the formula
    channels, kernels, B, L = list(synth.CHANNELS), [5] * len(synth.CHANNELS), 32, 16000
    sizes = {}
    for depth in (1, 2):
        h = plan_handle(channels, kernels, depth)
        try:
            bound_bites = False
            for j, (level, ci, co, k) in enumerate(R.convs_of(channels, kernels, depth)):
                assert lib.rs_train_slice_plan(h, j, B, L, C.byref(n), C.byref(s)) == 0
                assert (n.value, s.value) == R.slice_plan(B, L, level, ci, co, k), (depth, j)
                tile = (co * ci * k + co) * 4
                assert n.value == 1 or n.value * tile <= 32 * MiB, (depth, j)
                assert (n.value - 1) * s.value < B * (L >> level) <= n.value * s.value
                bound_bites |= n.value < -(-B * (L >> level) // 256) and (n.value + 1) * tile > 32 * MiB > n.value * (co * ci * 3 + co) * 4
            assert bound_bites, "no conv of this net is held by the 32 MiB bound: the case checks nothing"
            sizes[depth] = lib.rs_train_workspace_bytes(h, B, L)
            assert lib.rs_train_max_batch(h, L) >= B
        finally:
            lib.rs_train_destroy(h)
    print(f"workspace at {B} x {L}, kernel 5: depth 1 {sizes[1] / MiB:.1f} MiB, depth 2 {sizes[2] / MiB:.1f} MiB")
    assert sizes[2] > sizes[1] > 0
    # an inner conv keeps all its rows: at depth 2 the largest per-read buffer doubles, and max_batch halves (within one)
    a, b = plan_handle([64], [3], 1), plan_handle([64], [3], 2)
    try:
        ma, mb = lib.rs_train_max_batch(a, 1 << 16), lib.rs_train_max_batch(b, 1 << 16)
        window = (1 << 31) - 4096
        assert ma == window // ((1 << 15) * 64 * 4) and mb == window // ((1 << 16) * 64 * 4), (ma, mb)
    finally:
        lib.rs_train_destroy(a)
        lib.rs_train_destroy(b)


def test_numpy_backward_equals_float64_autograd():
    cases = [(name,) + R.case_of(name) for name in R.CASES if name != "slices"] + list(R.special_cases())
    channels, kernels, depth, _, _, seed = R.CASES["slices"]
    cases.append(("slices", R.make_state(channels, kernels, depth, seed)) + R.make_batch(2, 1201, seed + 100))
    for name, sd, x, y in cases:
        fwd = R.forward64(sd, x)
        grads, dys = R.backward64(sd, fwd, y)
        l64, g64, d64, lg64 = R.torch_loss_and_grads(sd, x, y)
        assert abs(R.loss64(fwd["logits"], y) - l64) <= 1e-12 * abs(l64), name
        assert R.gap_of(fwd["logits"], lg64) <= 1e-12, name
        assert len(dys) == len(d64) == len(R.conv_keys(sd))
        for k in g64:
            assert R.gap_of(grads[k], g64[k]) <= 1e-12, (name, k)
        for j, (a, b) in enumerate(zip(dys, d64)):
            assert a.shape == b.shape and R.gap_of(a, b) <= 1e-12, (name, j)


def test_depth_one_kernel_three_is_the_recorded_shipped_reference():
    """at the shipped class the reference gives, bit for bit, what the depth-1, kernel-3 reference it replaced gave: that
    module's gradients, per-layer dY and fragile masks are tests/golden/train_ref_shipped.npz"""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_ref_shipped.npz"))
    sd = R.make_state([3, 7, 18], [3] * 3, 1, 5)
    x, y = R.make_batch(3, 100, 6)
    fwd = R.forward64(sd, x)
    grads, dys = R.backward64(sd, fwd, y)
    got = {f"grad.{k}": v for k, v in grads.items()}
    got.update({f"dy.{l}": v for l, v in enumerate(dys)})
    got.update({f"fragile.{l}": v for l, v in enumerate(R.fragile(fwd))})
    assert sorted(got) == sorted(want.files) and len(got) == 8 + 3 + 3
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_fragile_share_of_the_committed_seeds():
    for name in R.CASES:
        sd, x, y = R.case_of(name)
        share = R.fragile_share(R.forward64(sd, x))
        print(f"{name}: fragile share {share:.3e}")
        assert share == 0 if name in R.SMALL else share < 1e-4, (name, share)
    for name, sd, x, y in R.special_cases():
        assert R.fragile_share(R.forward64(sd, x)) == 0, name


def test_planted_defects_miss_by_more_than_ten_bars():
    """each defect planted in the float64 reference must be far outside the bars the device is held to"""
    sd, x, y = R.case_of("depth2")
    bars, dbars, _, _, _ = R.bars_of(sd, x, y)
    fwd = R.forward64(sd, x)
    good, good_dy = R.backward64(sd, fwd, y)
    for defect in sorted(set(R.GENERIC_DEFECTS + R.SHIPPED_DEFECTS[1:])):         # the pooling defects at depth 2 as well
        grads, dys = R.backward64(sd, fwd, y, defect=defect)
        worst = max([R.gap_of(grads[k], good[k]) / bars[k] for k in good] +
                    [R.gap_of(a, b) / d for a, b, d in zip(dys, good_dy, dbars)])
        print(f"{defect}: {worst:.3g} bars")
        assert worst > 10, defect
