"""TCN training without a GPU: the configs TcnTrainer refuses, the state dict's keys, the plans of device-less handles, the
dropout hash, and the float64 cone reference of tests/tcn_train_ref.py held to dense autograd - with the defects a cone backward
can have planted one by one, each of which must show."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import tcn_train_ref as R
from train_ref import slice_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for _, n in R.NETS]
DROP_SEED = 7


@pytest.fixture(scope="module")
def lib():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    return nv.lib()


def config_of(cfg, **over):
    tcn = {k: v for k, v in cfg.items() if k not in ("model", "rf", "lengths")}
    tcn.update({k: v for k, v in over.items() if k in tcn})
    top = {k: v for k, v in over.items() if k not in tcn}
    return types.SimpleNamespace(model=top.pop("model", cfg["model"]), tcn=types.SimpleNamespace(**tcn), **top)


def test_header_symbols_and_sources_agree(lib):
    from riser_amd import _native as nv
    from riser_amd import build
    src = open(os.path.join(ROOT, "include", "riser_amd.h")).read()
    assert "Added after ABI 2.9, rs_version unchanged: TCN training" in src
    declared = sorted(set(re.findall(r"\b(rs_tcn_train_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(s for s in nv.SYMBOLS if s.startswith("rs_tcn_train_")) and len(declared) == 13
    assert all(hasattr(lib, s) for s in declared)
    assert "tcn_train.hip" in build.SOURCES and lib.rs_version() == (2 << 16) | 9
    # the kernels both training families launch live in one header, and neither file keeps a copy
    csrc = os.path.join(ROOT, "riser_amd", "csrc")
    shared = open(os.path.join(csrc, "train", "kernels.hpp")).read()
    for kernel in ("train_loss_kernel", "train_adam_kernel", "train_reduce_kernel"):
        assert f"void {kernel}(" in shared
        for f in ("train.hip", "tcn_train.hip"):
            text = open(os.path.join(csrc, f)).read()
            assert f"void {kernel}(" not in text and '#include "train/kernels.hpp"' in text


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    from riser_amd import tcn_train as T
    cfg, sd = R.load_net(name)
    net = T.check_tcn_config(config_of(cfg))
    shapes = T.param_shapes(net)
    assert list(shapes) == list(sd) and all(shapes[k] == sd[k].shape for k in sd)
    assert T.device_keys(net) == R.device_keys(cfg)
    torch.manual_seed(3)
    init = T.init_state(net)
    assert list(init) == list(sd) and all(tuple(init[k].shape) == sd[k].shape for k in sd)
    for k, v in init.items():
        if k.endswith("weight_g"):                         # g = ||v||: _init_weights cannot reach a weight-normed conv
            vv = init[k[:-1] + "v"].double()
            assert torch.allclose(v.double().flatten(), vv.pow(2).sum((1, 2)).sqrt(), rtol=1e-6)
    torch.manual_seed(3)
    again = T.init_state(net)
    assert all(torch.equal(init[k], again[k]) for k in init)
    # both weight-norm spellings load
    alt = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v
           for k, v in sd.items()}
    got = T._checked_state(alt, shapes)
    assert all(np.array_equal(got[k], sd[k]) for k in sd)


def test_refusals_raise_before_any_gpu_call(lib):
    from riser_amd import _native as nv
    from riser_amd import tcn_train as T
    cfg, sd = R.load_net("tcn_k3_b2")
    T.check_tcn_config(config_of(cfg))
    for bad in (dict(model="tcn-bot"), dict(model="cnn"), dict(dtype="bf16"), dict(dtype="bf16x3"), dict(n_classes=3),
                dict(kernel=1), dict(in_channels=2), dict(dropout=1.0), dict(dropout=-0.1), dict(n_layers=0)):
        with pytest.raises(ValueError):
            T.check_tcn_config(config_of(cfg, **bad))
        with pytest.raises(ValueError):
            T.TcnTrainer(config_of(cfg, **bad), sd)
    net = T.check_tcn_config(config_of(cfg))
    # the C ABI refuses the same before it touches a device: a device index that does not exist is never reached
    for bad in (dict(bottleneck=True), dict(dtype=nv.RS_BF16), dict(dtype=nv.RS_BF16X3), dict(n_classes=3), dict(in_channels=2)):
        with pytest.raises(nv.NativeError):
            T.create_handle(net, sd, 10 ** 6, **bad)
    for bad in (dict(kernel=1), dict(dropout=1.0), dict(dropout=-0.5), dict(dropout=float("nan"))):
        with pytest.raises(nv.NativeError):
            T.create_handle(dict(net, **bad), sd, 10 ** 6)
    assert lib.rs_tcn_train_create(None, None, 0, -1, None) == nv.RS_ERR_ARG
    assert lib.rs_tcn_train_workspace_bytes(None, 1, 100) == 0 and lib.rs_tcn_train_max_batch(None, 100) == 0
    assert lib.rs_tcn_train_destroy(None) == 0
    # riser_amd.train keeps its refusals
    from riser_amd import train
    with pytest.raises(ValueError):
        train.net_of(config_of(cfg))


@pytest.mark.parametrize("name", NAMES + ["bench"])
def test_plans_of_a_deviceless_handle(lib, name):
    from riser_amd import _native as nv
    from riser_amd import tcn_train as T
    if name == "bench":
        cfg = dict(in_channels=1, n_filters=64, kernel=3, dilation=2, n_layers=8, dropout=0.2, n_classes=2, model="tcn")
        net = T.check_tcn_config(config_of(cfg))
        sd = {k: np.zeros(s, np.float32) for k, s in T.param_shapes(net).items()}
    else:
        cfg, sd = R.load_net(name)
        net = T.check_tcn_config(config_of(cfg))
    h = T.create_handle(net, sd, -1)
    try:
        n, s, r = C.c_int32(), C.c_int32(), C.c_int32()
        for L in (1, 7, 125, 16000):
            mb = lib.rs_tcn_train_max_batch(h, L)
            assert mb >= 1
            cone = R.cone(cfg, L)
            F = cfg["n_filters"]
            row = ((F + 3) & ~3) * 4
            per = max([L * 4] + [max(r1, ro) * row for _, r1, ro, _ in cone])
            assert mb == max(1, min(1 << 30, ((1 << 31) - 4096) // per))
            for B in (1, 5, mb):
                ws = lib.rs_tcn_train_workspace_bytes(h, B, L)
                assert ws > 0
                for i, (rin, r1, ro, d) in enumerate(cone):
                    c_in = 1 if i == 0 else F
                    for which, rows, ci, k in ((0, r1, c_in, cfg["kernel"]), (1, ro, F, cfg["kernel"]), (2, ro, c_in, 1)):
                        rc = lib.rs_tcn_train_slice_plan(h, i, which, B, L, C.byref(n), C.byref(s), C.byref(r))
                        if which == 2 and not R.applied(cfg, i):
                            assert rc == nv.RS_ERR_ARG
                            continue
                        assert rc == 0 and r.value == rows
                        assert (n.value, s.value) == slice_plan(B, rows, 0, ci, F, k)
                        # every launch's grid: the slices in y, 128 rows of all reads per workgroup in x
                        assert 1 <= n.value <= 65535 and (n.value - 1) * s.value < B * rows <= n.value * s.value
                        assert B * rows < 2 ** 31 and -(-B * max(rin, r1, ro) // 128) < 2 ** 31
                        assert n.value * (F * ci * k + F) * 4 <= ws
            # a call on a device-less handle is refused after its argument checks
            one = C.c_float()
            assert lib.rs_tcn_train_forward_backward(h, C.byref(one), C.byref(one), 1, L, L, C.byref(one), 1 << 40, C.byref(one),
                                                     None) == nv.RS_ERR_ARG
            assert b"without a device" in lib.rs_last_error()
            assert lib.rs_tcn_train_forward_backward(h, C.byref(one), C.byref(one), 1, L, L - 1, C.byref(one), 1 << 40,
                                                     C.byref(one), None) == nv.RS_ERR_ARG
            assert lib.rs_tcn_train_forward_backward(h, C.byref(one), C.byref(one), 1, L, L, C.byref(one), 16, C.byref(one),
                                                     None) == nv.RS_ERR_WORKSPACE
        assert lib.rs_tcn_train_debug_copy(h, 0, 0, C.byref(one), 4) == nv.RS_ERR_ARG
        assert lib.rs_tcn_train_set_dropout(h, 1.0, 0, 0) == nv.RS_ERR_ARG and lib.rs_tcn_train_set_dropout(h, 0.5, 1, 2) == 0
    finally:
        lib.rs_tcn_train_destroy(h)


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_hash_keeps_its_share_and_keys_are_independent(p):
    n = 1 << 20
    base = R.keep_mask(p, DROP_SEED, 0, 0, 16, np.arange(1024), 64)
    assert base.size == n
    sd4 = 4 * np.sqrt(n * p * (1 - p))
    assert abs(int(base.sum()) - n * (1 - p)) <= sd4
    # another step, another conv, another seed: the masks agree on no more than chance, (1 - p)^2 + p^2
    chance = (1 - p) ** 2 + p ** 2
    sd4 = 4 * np.sqrt(n * chance * (1 - chance))
    for other in (R.keep_mask(p, DROP_SEED, 1, 0, 16, np.arange(1024), 64), R.keep_mask(p, DROP_SEED, 0, 1, 16, np.arange(1024), 64),
                  R.keep_mask(p, DROP_SEED + 1, 0, 0, 16, np.arange(1024), 64),
                  R.keep_mask(p, DROP_SEED, 1 << 32, 0, 16, np.arange(1024), 64)):
        assert abs(int((other == base).sum()) - n * chance) <= sd4
    # neighbours along every key agree on no more than chance either
    for a, b in ((base[1:], base[:-1]), (base[:, 1:], base[:, :-1]), (base[:, :, 1:], base[:, :, :-1])):
        m = a.size
        assert abs(int((a == b).sum()) - m * chance) <= 4 * np.sqrt(m * chance * (1 - chance))
    assert R.keep_mask(0.0, DROP_SEED, 0, 0, 2, np.arange(3), 4).all()
    assert R.threshold(0.2) == 858993459 and R.scale_of(0.2) == float(np.float32(1.25))


def cases():
    for name in NAMES:
        cfg, _ = R.load_net(name)
        for L in R.lengths_of(name, cfg):
            yield name, L


@pytest.mark.parametrize("name,L", list(cases()))
def test_cone_backward_equals_dense_autograd(name, L):
    cfg, sd = R.load_net(name)
    x, y = R.make_batch(R.B_CASE, L, R.case_seed(name, L))
    for p in (0.0, 0.2):
        masks = R.masks_of(cfg, R.B_CASE, L, p, DROP_SEED, 0)
        fwd = R.forward64(sd, cfg, x, p, masks)
        assert R.fragile_share(fwd) <= 1e-3, R.fragile_share(fwd)
        grads, douts, da1s = R.backward64(sd, cfg, fwd, y, p)
        loss, g64, d64, a64, logits = R.torch_loss_and_grads(sd, cfg, x, y, torch.float64, p,
                                                             R.dense_masks(cfg, R.B_CASE, L, p, DROP_SEED, 0))
        assert R.gap_of(fwd["logits"], logits) <= 1e-10 and abs(R.loss64(fwd["logits"], y) - loss) <= 1e-10 * abs(loss)
        for k in R.device_keys(cfg):
            assert R.gap_of(grads[k], g64[k]) <= 1e-10, k
        assert set(grads) == set(R.device_keys(cfg))        # an unapplied shortcut has no gradient
        for i in range(cfg["n_layers"]):
            assert R.gap_of(douts[i], d64[i]) <= 1e-10 and R.gap_of(da1s[i], a64[i]) <= 1e-10, i
            assert all(np.abs(g64[f"layers.{i}.shortcut.{t}"]).max() == 0 for t in ("weight", "bias")) or R.applied(cfg, i)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_shows(defect):
    """every defect misses autograd by more than ten bars on some tensor of some net"""
    worst = 0.0
    for name, L in cases():
        cfg, sd = R.load_net(name)
        if cfg["rf"] > 1000 and L > 1500:
            continue
        x, y = R.make_batch(R.B_CASE, L, R.case_seed(name, L))
        p = 0.2
        dense = R.dense_masks(cfg, R.B_CASE, L, p, DROP_SEED, 0)
        bars, _, _, _, (_, g64, _, _, _) = R.bars_of(sd, cfg, x, y, p, dense)
        masks = R.masks_of(cfg, R.B_CASE, L, p, DROP_SEED, 0, keyed_on_p=defect == "mask_keyed_on_p")
        fwd = R.forward64(sd, cfg, x, p, masks)
        grads, _, _ = R.backward64(sd, cfg, fwd, y, p, defect=defect)
        worst = max([worst] + [R.gap_of(grads[k], g64[k]) / bars[k] for k in grads])
        if worst > 10:
            return
    assert worst > 10, worst
