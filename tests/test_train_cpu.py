"""Training (riser_amd.train, csrc/train.hip, rs_train_*) without a GPU: the float64 reference the device tests lean on (train_ref, here at the
shipped class: depth 1, every kernel 3), the C ABI's argument checks, the refusals, and the loop of riser/train.py on a stub trainer."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import train_ref as R
from riser_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ([3, 7, 18, 37], 3, 100, 11)
LARGE = (([5, 17, 33], 2, 9002, 23), (list(synth.CHANNELS), 2, 4100, 23))


def config_of(channels, **over):
    cnn = synth.CnnConfig(channels=channels, kernels=[3] * len(channels))
    for k in [k for k in over if hasattr(cnn, k)]:
        setattr(cnn, k, over.pop(k))
    return types.SimpleNamespace(**{"model": "cnn", "learning_rate": 1e-3, "cnn": cnn, **over})


def state_of(channels, seed, bias=None):
    return R.make_state(channels, [3] * len(channels), 1, seed, bias)


def small_cases():
    channels, B, L, seed = SMALL
    sd = state_of(channels, seed)
    x, y = R.make_batch(B, L, seed + 100)
    yield "random", sd, x, y
    yield "ties", sd, *R.constant_reads(3, 200)
    yield "dead", state_of(channels, seed, bias=-50.0), x, y


def test_numpy_backward_equals_float64_autograd():
    for name, sd, x, y in small_cases():
        fwd = R.forward64(sd, x)
        grads, dys = R.backward64(sd, fwd, y)
        l64, g64, d64, lg64 = R.torch_loss_and_grads(sd, x, y)
        assert abs(R.loss64(fwd["logits"], y) - l64) <= 1e-12 * abs(l64), name
        assert R.gap_of(fwd["logits"], lg64) <= 1e-12, name
        for k in g64:
            assert R.gap_of(grads[k], g64[k]) <= 1e-12, (name, k)
        for l, (a, b) in enumerate(zip(dys, d64)):
            assert R.gap_of(a, b) <= 1e-12, (name, l)


def test_selector_rule_is_torchs():
    """row 2 j wins unless row 2 j + 1 is strictly larger: max_pool1d's indices on ties, checked on the CPU"""
    r = torch.tensor([[[1.0, 1.0, 0.0, 0.0, 2.0, 3.0, 3.0, 2.0, 5.0]]], dtype=torch.float64)
    _, idx = torch.nn.functional.max_pool1d(r, 2, 2, return_indices=True)
    assert (idx[0, 0] % 2).tolist() == [0, 0, 1, 0]
    sd = {"layers.0.0.weight": np.array([[[0.0, 1.0, 0.0]]], np.float32), "layers.0.0.bias": np.zeros(1, np.float32),
          "classifier.2.weight": np.ones((2, 1), np.float32), "classifier.2.bias": np.zeros(2, np.float32)}
    assert R.forward64(sd, r[0].numpy())["sel"][0][0, :, 0].tolist() == [0, 0, 1, 0]


def test_small_shapes_have_no_fragile_element():
    for name, sd, x, y in small_cases():
        assert sum(int(f.sum()) for f in R.fragile(R.forward64(sd, x))) == 0, name


def test_fragile_share_of_the_large_shapes():
    for channels, B, L, seed in LARGE:
        frag = R.fragile(R.forward64(state_of(channels, seed), R.make_batch(B, L, seed + 100)[0]))
        share = sum(int(f.sum()) for f in frag) / sum(f.size for f in frag)
        print(f"{len(channels)} layers, {B} x {L}: fragile share {share:.3e}")
        assert share < 1e-4, (channels[:3], share)


@pytest.fixture(scope="module")
def lib():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    return nv.lib()


def plan_handle(channels):
    from riser_amd.train import create_handle
    return create_handle(channels, state_of(channels, 1), -1)


def test_header_symbols_and_sources_agree(lib):
    from riser_amd import _native as nv
    from riser_amd import build
    src = open(os.path.join(ROOT, "include", "riser_amd.h")).read()
    assert "Added after ABI 2.9, rs_version unchanged: training" in src
    declared = sorted(set(re.findall(r"\b(rs_train_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert declared == sorted(s for s in nv.SYMBOLS if s.startswith("rs_train_")) and len(declared) >= 11
    assert all(hasattr(lib, s) for s in declared)
    assert "train.hip" in build.SOURCES and os.path.isdir(os.path.join(ROOT, "riser_amd", "csrc", "train"))
    assert lib.rs_version() == (2 << 16) | 9


def test_argument_validation_without_gpu(lib):
    from riser_amd import _native as nv
    from riser_amd.gconv import _Conv
    w, b = np.zeros(64 * 64 * 3, np.float32), np.zeros(64, np.float32)

    def create(convs, n_layers, device=10 ** 6):
        arr = (_Conv * len(convs))(*[_Conv(ci, co, k, 0, w.ctypes.data, b.ctypes.data) for ci, co, k in convs])
        h = C.c_void_p()
        rc = lib.rs_train_create(arr, n_layers, w.ctypes.data, b.ctypes.data, device, C.byref(h))
        assert not h.value
        return rc, lib.rs_last_error()

    # device 1 000 000 does not exist: a refusal that names the argument was made without asking for it
    rc, msg = create([(1, 8, 5)], 1)
    assert rc == nv.RS_ERR_ARG and b"kernels of 3" in msg
    rc, msg = create([(1, 8, 3), (9, 8, 3)], 2)
    assert rc == nv.RS_ERR_ARG and b"chained" in msg
    assert lib.rs_train_create(None, 1, None, None, 0, None) == nv.RS_ERR_ARG
    assert lib.rs_train_destroy(None) == nv.RS_OK
    assert lib.rs_train_workspace_bytes(None, 1, 64) == 0 and lib.rs_train_max_batch(None, 64) == 0

    h = plan_handle([3, 7, 18, 37])
    try:
        n, s = C.c_int32(), C.c_int32()
        assert lib.rs_train_workspace_bytes(h, 3, 100) > 0 and lib.rs_train_workspace_bytes(h, 3, 15) == 0
        assert lib.rs_train_max_batch(h, 100) >= 3 and lib.rs_train_max_batch(h, 15) == 0
        assert lib.rs_train_slice_plan(h, 4, 3, 100, C.byref(n), C.byref(s)) == nv.RS_ERR_ARG
        assert lib.rs_train_slice_plan(None, 0, 3, 100, C.byref(n), C.byref(s)) == nv.RS_ERR_ARG
        p = 4096                                             # any non-null address: no check dereferences it
        big = 1 << 40
        for fn, name in ((lib.rs_train_forward_backward, b"rs_train_forward_backward"), (lib.rs_train_evaluate, b"rs_train_evaluate")):
            for args in ((None, p, p, 3, 100, 100, p, big, p), (h, None, p, 3, 100, 100, p, big, p), (h, p, None, 3, 100, 100, p, big, p),
                         (h, p, p, 3, 100, 100, None, big, p), (h, p, p, 3, 100, 100, p, big, None), (h, p, p, 0, 100, 100, p, big, p),
                         (h, p, p, 3, 0, 100, p, big, p), (h, p, p, 3, 100, 99, p, big, p)):
                assert fn(*args, None) == nv.RS_ERR_ARG and name + b": bad argument" in lib.rs_last_error(), args
            assert fn(h, p, p, 3, 15, 15, p, big, p, None) == nv.RS_ERR_LENGTH and b"shorter than the network minimum 16" in lib.rs_last_error()
            need = lib.rs_train_workspace_bytes(h, 3, 100)
            assert fn(h, p, p, 3, 100, 100, p, need - 1, p, None) == nv.RS_ERR_WORKSPACE and b"workspace too small" in lib.rs_last_error()
            L = 1 << 20
            mb = lib.rs_train_max_batch(h, L)
            assert 1 <= mb < 1000
            assert fn(h, p, p, mb + 1, L, L, p, big * 1024, p, None) == nv.RS_ERR_ARG and b"2 GiB buffer window" in lib.rs_last_error()
            assert fn(h, p, p, 3, 100, 100, p, big, p, None) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
        assert lib.rs_train_adam_step(None, 1e-3, 0.9, 0.999, 1e-8, None) == nv.RS_ERR_ARG
        assert lib.rs_train_adam_step(h, 0.0, 0.9, 0.999, 1e-8, None) == nv.RS_ERR_ARG
        assert lib.rs_train_adam_step(h, 1e-3, 1.0, 0.999, 1e-8, None) == nv.RS_ERR_ARG
        assert lib.rs_train_adam_step(h, 1e-3, 0.9, 0.999, 1e-8, None) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
        buf = np.zeros(64, np.float32)
        for fn in (lib.rs_train_get_params, lib.rs_train_set_params, lib.rs_train_get_grads):
            assert fn(None, 0, buf.ctypes.data, 9) == nv.RS_ERR_ARG
            assert fn(h, 10, buf.ctypes.data, 9) == nv.RS_ERR_ARG            # tensors 0 .. 9
            assert fn(h, 0, buf.ctypes.data, 8) == nv.RS_ERR_ARG             # layers.0.0.weight has 9 elements
            assert fn(h, 0, None, 9) == nv.RS_ERR_ARG
            assert fn(h, 0, buf.ctypes.data, 9) == nv.RS_ERR_ARG and b"without a device" in lib.rs_last_error()
        assert lib.rs_train_debug_copy(None, 0, 0, p, 64) == nv.RS_ERR_ARG
        assert lib.rs_train_debug_copy(h, 4, 0, p, 64) == nv.RS_ERR_ARG and lib.rs_train_debug_copy(h, 0, 3, p, 64) == nv.RS_ERR_ARG
        assert lib.rs_train_debug_copy(h, 0, 0, p, 64) == nv.RS_ERR_ARG and b"no rs_train_forward_backward has run" in lib.rs_last_error()
    finally:
        assert lib.rs_train_destroy(h) == nv.RS_OK


def test_slice_plan_depends_on_the_shape_alone(lib):
    h = plan_handle([5, 17, 33])
    n, s = C.c_int32(), C.c_int32()
    try:
        assert lib.rs_train_slice_plan(h, 0, 2, 9002, C.byref(n), C.byref(s)) == 0
        assert s.value % 4 == 0 and n.value >= 3 and (n.value - 1) * s.value < 2 * 9002 < n.value * s.value
        for layer in range(3):
            assert lib.rs_train_slice_plan(h, layer, 2, 9002, C.byref(n), C.byref(s)) == 0
            positions = 2 * (9002 >> layer)
            assert (n.value - 1) * s.value < positions <= n.value * s.value and s.value % 4 == 0
    finally:
        lib.rs_train_destroy(h)
    h = plan_handle(list(synth.CHANNELS))
    try:
        tiles = [(20, 1)] + list(zip(synth.CHANNELS[1:], synth.CHANNELS[:-1]))
        for layer, (co, ci) in enumerate(tiles):
            assert lib.rs_train_slice_plan(h, layer, 32, 16000, C.byref(n), C.byref(s)) == 0
            assert n.value == 1 or n.value * (co * ci * 3 + co) * 4 <= 32 << 20, layer     # the partials' bytes are bounded
            assert (n.value - 1) * s.value < 32 * (16000 >> layer) <= n.value * s.value
        assert lib.rs_train_slice_plan(h, 0, 32, 16000, C.byref(n), C.byref(s)) == 0 and n.value == 2000
        assert lib.rs_train_slice_plan(h, 11, 32, 16000, C.byref(n), C.byref(s)) == 0 and (n.value, s.value) == (1, 224)
        assert lib.rs_train_workspace_bytes(h, 32, 16000) < 1 << 30 and lib.rs_train_max_batch(h, 16000) >= 32
    finally:
        lib.rs_train_destroy(h)


def test_refusals_come_before_any_gpu_call():
    from riser_amd.train import Trainer, check_config
    ch = [8, 12]
    for cfg, match in ((config_of(ch, depth=2), "depth"), (config_of(ch, kernels=[3, 5]), "kernels"),
                       (config_of(ch, classifier="fc"), "classifier"), (config_of(ch, classifier="gap"), "classifier"),
                       (config_of(ch, model="tcn"), "model"), (config_of(ch, dtype="bf16x3"), "dtype")):
        with pytest.raises(ValueError, match=match):         # a ValueError, not the NativeError of a missing device
            Trainer(cfg)
        with pytest.raises(ValueError, match=match):
            check_config(cfg)
    with pytest.raises(ValueError, match="dtype"):
        Trainer(config_of(ch), dtype="bf16")
    with pytest.raises(ValueError, match="layers.1.0.weight"):
        Trainer(config_of(ch), {k: v for k, v in state_of(ch, 1).items() if k != "layers.1.0.weight"})
    assert check_config(config_of(ch)) == ch


class StubTrainer:
    """records what fit asks for"""

    def __init__(self, channels):
        self.channels, self.calls, self.n_eval = channels, [], 0

    def step(self, x, y):
        self.calls.append(("step", tuple(x.shape), sorted(int(v) for v in x[:, 0])))
        return 1.0 / len(self.calls)

    def evaluate(self, x, y):
        self.calls.append(("eval", tuple(x.shape), [int(v) for v in x[:, 0]]))
        self.n_eval += 1
        return 0.5, int(len(y)) if self.n_eval > 6 else 0     # six batches per epoch: the second epoch is strictly better

    def state_dict(self):
        from riser_amd.train import init_state
        return init_state(self.channels)


def numbered(n, L):
    """reads whose first sample is their index in the loader's dataset (negatives in front)"""
    data = torch.zeros((2 * n, L))
    data[:, 0] = torch.arange(2 * n)
    return data, torch.cat((torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long)))


def test_fit_steps_the_loaders_together_until_the_longest_ends(tmp_path):
    from riser_amd import train as T
    sets = {"2s": numbered(3, 8), "3s": numbered(5, 12), "4s": numbered(2, 16)}       # 6, 10 and 4 reads: 2, 3 and 1 batches of 4
    stub = StubTrainer([4, 6])
    logs = []
    best = T.fit(stub, sets, sets, 2, 4, str(tmp_path / "run9"), "run9", seed=4, log=logs.append)
    per_epoch = len(stub.calls) // 2
    first = stub.calls[:per_epoch]
    steps, evals = [c for c in first if c[0] == "step"], [c for c in first if c[0] == "eval"]
    assert [c[1] for c in evals] == [(4, 8), (4, 12), (4, 16), (2, 8), (4, 12), (2, 12)]      # rounds of 2s, 3s, 4s; None skipped
    assert [c[2] for c in evals] == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [4, 5], [4, 5, 6, 7], [8, 9]]      # unshuffled
    widths = [c[1][1] for c in steps]
    assert sorted(widths[:3]) == [8, 12, 16] and sorted(widths[3:5]) == [8, 12] and widths[5:] == [12]
    for L, n in ((8, 6), (12, 10), (16, 4)):                 # every loader is a permutation of its own reads
        assert sorted(i for c in steps if c[1][1] == L for i in c[2]) == list(range(n))
    assert [c[2] for c in steps if c[1][1] == 12] != [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    stub2 = StubTrainer([4, 6])
    T.fit(stub2, sets, sets, 2, 4, str(tmp_path / "again"), "again", seed=4, log=lambda *_: None)
    assert stub2.calls == stub.calls                         # the seed fixes the shuffles and the key order
    assert best == (100.0, 1)
    rows = [r.split("\t") for r in open(tmp_path / "run9" / "metrics.tsv").read().splitlines()]
    assert rows[0] == list(T.METRICS) and [r[0] for r in rows[1:]] == ["0", "1"]
    assert float(rows[1][1]) == pytest.approx(sum(1.0 / k for k in range(1, 7)) / 6) and float(rows[1][2]) == 0.5
    assert [float(r[3]) for r in rows[1:]] == [0.0, 100.0]
    assert any("Number of batches in training set: 6" in m for m in logs)
    assert sorted(os.listdir(tmp_path / "run9")) == ["metrics.tsv", "run9_0_best_model.pth", "run9_latest_model.pth"]
    sd = torch.load(tmp_path / "run9" / "run9_0_best_model.pth")
    assert list(sd) == ["layers.0.0.weight", "layers.0.0.bias", "layers.1.0.weight", "layers.1.0.bias",
                        "classifier.2.weight", "classifier.2.bias"]
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"layers.0.0.weight": (4, 1, 3), "layers.0.0.bias": (4,),
                                                          "layers.1.0.weight": (6, 4, 3), "layers.1.0.bias": (6,),
                                                          "classifier.2.weight": (2, 6), "classifier.2.bias": (2,)}
    assert all(v.dtype == torch.float32 for v in sd.values())


def test_checkpoint_names_and_command_line():
    from riser_amd import train as T
    assert T.checkpoint_names("/d/exp3", "exp3", 4) == ("/d/exp3/exp3_4_best_model.pth", "/d/exp3/exp3_latest_model.pth")
    a = T.parse_args(["runs/exp3", "data", "None", "cfg.yaml", "0"])
    assert (a.exp_dir, a.data_dir, a.checkpt, a.config_file, a.start_epoch, a.exp_id) == ("runs/exp3", "data", None, "cfg.yaml", 0, "exp3")
    a = T.parse_args(["runs/exp3", "data", "exp3_latest_model.pth", "cfg.yaml", "7"])
    assert a.checkpt == "exp3_latest_model.pth" and a.start_epoch == 7
    with pytest.raises(AssertionError):
        T.parse_args(["runs/exp3", "data", "None", "cfg.yaml", "3"])
    with pytest.raises(AssertionError):
        T.parse_args(["runs/exp3", "data", "exp3_latest_model.pth", "cfg.yaml", "0"])
    with pytest.raises(SystemExit):
        T.parse_args(["runs/exp3", "data"])


def test_load_set_puts_negatives_first(tmp_path):
    from riser_amd import train as T
    torch.save(torch.ones((3, 8)), tmp_path / "positive.pt")
    torch.save(torch.zeros((2, 8)), tmp_path / "negative.pt")
    data, label = T.load_set(str(tmp_path))
    assert label.tolist() == [0, 0, 1, 1, 1] and data[:, 0].tolist() == [0, 0, 1, 1, 1] and data.dtype == torch.float32
