"""Training at any depth and any odd kernel (csrc/train.hip through rs_train_create_generic, riser_amd.train.GenericTrainer)
on the device against float64.

Gap = largest absolute difference over a tensor / largest magnitude of the float64 tensor.  The bar of a tensor is four times
the gap torch's own fp32 autograd, run on the CPU, shows against float64 on the same inputs, with a floor of 1e-6; it is
computed here at run time (train_ref.bars_of) and never taken from the code under test.  Where a case has fragile elements
(train_ref.fragile) the backward kernels are held to the numpy float64 backward fed the DEVICE's selectors and gates, and the
device's decisions must equal float64's outside the fragile set.  Convs are numbered j = layer * depth + d; the device helpers are
train_device's.  Measured gaps and
bars: profiles/gtrain_gpu_tests.txt, DESIGN.md section 17.
"""
import numpy as np
import pytest
import torch

import train_device as D
import train_ref as R
from train_device import assert_all, check, config_of, run_device, trainer_of


def against_autograd(name):
    """a case without fragile elements: the loss and every gradient against float64 autograd"""
    sd, x, y = R.case_of(name)
    bars, _, loss_bar, _, (l64, g64, _, _) = R.bars_of(sd, x, y)
    assert R.fragile_share(R.forward64(sd, x)) == 0
    loss, grads = run_device(name, sd, x, y)
    print(f"{name} loss: device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(f"{name} {k}", grads[k], g64[k], bars[k]) for k in g64])


def held_to_numpy_backward(name):
    sd, x, y = R.case_of(name)
    return D.held_to_numpy_backward(name, sd, x, y, label=f"{name} ")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["depth2", "depth3"])
def test_end_to_end_against_float64_autograd(name):
    against_autograd(name)
    held_to_numpy_backward(name)                # and every conv's incoming gradient, pooled or full resolution


@pytest.mark.gpu
def test_kernel_wider_than_the_read():
    against_autograd("wider_than_read")
    held_to_numpy_backward("wider_than_read")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 7])
def test_tap_groups(k):
    grads, g_ref, bars = held_to_numpy_backward(f"taps{k}")
    assert grads["layers.1.0.weight"].shape == (33, 17, k)
    against_autograd(f"taps{k}")


@pytest.mark.gpu
def test_bias_gradient_is_the_same_whatever_the_group_count():
    """a kernel-1 net, and the same net as kernel 5 and kernel 7 with zeros around the centre tap: the forward pass adds exact
    zeros, dZ is the same, so db - written by the first tap group only - and the centre tap of dW keep their bits"""
    sd1, x, y = R.case_of("taps1")
    channels = R.CASES["taps1"][0]
    got = {}
    for k in (1, 5, 7):
        sd = {key: v.copy() for key, v in sd1.items()}
        for key in [key for key in sd if key.startswith("layers.") and key.endswith(".weight")]:
            w = np.zeros(sd1[key].shape[:2] + (k,), np.float32)
            w[:, :, k // 2] = sd1[key][:, :, 0]
            sd[key] = w
        got[k] = run_device((channels, [k, k], 1), sd, x, y)
    l1, g1 = got[1]
    for k in (5, 7):
        lk, gk = got[k]
        assert lk == l1, k
        for key in g1:
            if key.endswith(".weight") and key.startswith("layers."):
                assert np.array_equal(gk[key][:, :, k // 2], g1[key][:, :, 0]), (k, key)
                assert np.abs(gk[key]).max(axis=(0, 1)).min() > 0, (k, key)         # every tap of every group was written
            else:
                assert np.array_equal(gk[key], g1[key]), (k, key)


@pytest.mark.gpu
def test_slice_boundaries():
    channels, kernels, depth, B, L, _ = R.CASES["slices"]
    sd, x, y = R.case_of("slices")
    t = trainer_of("slices", sd)
    try:
        plans = [t.slice_plan(j, B, L) for j in range(len(channels) * depth)]
    finally:
        t.close()
    assert plans == [R.slice_plan(B, L, level, ci, co, k) for level, ci, co, k in R.convs_of(channels, kernels, depth)]
    n, s = plans[0]
    assert n >= 3 and s % 4 == 0 and (n - 1) * s < B * L < n * s, (n, s)           # several slices, the last one not full
    held_to_numpy_backward("slices")


@pytest.mark.gpu
def test_block_boundary():
    held_to_numpy_backward("block")


@pytest.mark.gpu
def test_exact_ties_and_dead_units():
    cases = {name: (sd, x, y) for name, sd, x, y in R.special_cases()}
    shape = R.CASES["depth2"][:3]
    sd, x, y = cases["ties"]
    fwd = R.forward64(sd, x)
    z = fwd["z"][1]                                          # the first pooling conv
    assert (z[:, 0:-1:2] == z[:, 1::2]).mean() >= 0.9
    bars, _, loss_bar, _, (l64, g64, _, _) = R.bars_of(sd, x, y)
    loss, grads, sel, gate, _ = run_device(shape, sd, x, y, debug=True)
    for j, s in enumerate(sel):
        if s is not None:
            assert np.array_equal(s, fwd["sel"][j]), f"ties: conv {j}"
        assert np.array_equal(gate[j], fwd["gate"][j]), f"ties: conv {j}"
    assert int(sel[1][:, 3:-3].sum()) == 0                   # exact ties go to the even row
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(f"ties {k}", grads[k], g64[k], bars[k]) for k in g64])
    sd, x, y = cases["dead"]
    fwd = R.forward64(sd, x)
    _, g64, _, _ = R.torch_loss_and_grads(sd, x, y)
    loss, grads, sel, gate, _ = run_device(shape, sd, x, y, debug=True)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    for j, s in enumerate(sel):
        assert s is None or np.array_equal(s, fwd["sel"][j]), f"dead: conv {j}"
        assert not gate[j].any()
    for k, g in grads.items():
        if not g64[k].any():
            assert not g.any(), k
    assert all(not g64[k].any() for k in g64 if k.startswith("layers.") or k == "classifier.2.weight")
    assert R.gap_of(grads["classifier.2.bias"], g64["classifier.2.bias"]) <= 1e-6


@pytest.mark.gpu
def test_five_adam_steps_against_torch_float64():
    sd, x, y = R.case_of("depth2")
    l64, p64 = R.torch_adam(sd, x, y, torch.float64, 5, 1e-3)
    l32, p32 = R.torch_adam(sd, x, y, torch.float32, 5, 1e-3)
    t = trainer_of("depth2", sd, lr=1e-3)
    losses = [t.step(torch.from_numpy(x), torch.from_numpy(y)) for _ in range(5)]
    got = {k: v.numpy() for k, v in t.state_dict().items()}
    t.close()
    for i in range(5):
        bar = max(4 * abs(l32[i] - l64[i]) / abs(l64[i]), 1e-6)
        print(f"step {i}: loss {losses[i]!r} float64 {l64[i]!r} bar {bar:.3e}")
        assert abs(losses[i] - l64[i]) <= bar * abs(l64[i]), i
    assert_all([check(f"adam {k}", got[k], p64[k], max(4 * R.gap_of(p32[k], p64[k]), 1e-6)) for k in p64])


@pytest.mark.gpu
def test_same_state_and_batch_give_the_same_bits():
    sd, x, y = R.case_of("slices")
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    t = trainer_of("slices", sd)
    l1, g1 = t.loss_and_grads(xs, ys)
    l2, g2 = t.loss_and_grads(xs, ys)
    assert l1 == l2 and all(torch.equal(g1[k], g2[k]) for k in g1)
    u = trainer_of("slices", sd)
    losses = [[tr.step(xs, ys) for _ in range(3)] for tr in (t, u)]
    a, b = t.state_dict(), u.state_dict()
    t.close()
    u.close()
    assert losses[0] == losses[1] and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k].numpy(), sd[k]) for k in a)


@pytest.mark.gpu
def test_generic_constructor_gives_the_shipped_class_its_bits():
    from riser_amd.train import GenericTrainer, Trainer
    shape = ([3, 7, 18, 37], [3] * 4, 1)
    sd = R.make_state(*shape, 11)
    x, y = R.make_batch(3, 100, 111)
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    ours, ref = trainer_of(shape, sd, cls=GenericTrainer), trainer_of(shape, sd, cls=Trainer)
    try:
        (la, ga), (lb, gb) = ours.loss_and_grads(xs, ys), ref.loss_and_grads(xs, ys)
        assert la == lb and list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
        assert [ours.slice_plan(j, 3, 100) for j in range(4)] == [ref.slice_plan(j, 3, 100) for j in range(4)]
        assert [ours.step(xs, ys) for _ in range(3)] == [ref.step(xs, ys) for _ in range(3)]
        pa, pb = ours.state_dict(), ref.state_dict()
        assert all(torch.equal(pa[k], pb[k]) for k in pb) and any(not np.array_equal(pa[k].numpy(), sd[k]) for k in pa)
    finally:
        ours.close()
        ref.close()


@pytest.mark.gpu
def test_checkpoint_loads_into_the_inference_family(tmp_path):
    from riser_amd.gconv import GConvNet, build_gconv_program
    channels, kernels, depth = R.CASES["depth2"][:3]
    sd, x, y = R.case_of("depth2")
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    t = trainer_of("depth2", sd)
    t.step(xs, ys)
    torch.save(t.state_dict(), tmp_path / "depth2_latest_model.pth")
    logits = t.logits(xs, ys).numpy()
    t.close()
    state = torch.load(tmp_path / "depth2_latest_model.pth")
    assert list(state) == list(sd) and all(v.dtype == torch.float32 and v.device.type == "cpu" for v in state.values())
    assert any(not np.array_equal(state[k].numpy(), sd[k]) for k in sd)
    stepped = {k: v.numpy() for k, v in state.items()}
    _, _, _, logits_bar, (_, _, _, lg64) = R.bars_of(stepped, x, y)
    dev = torch.device("cuda", 0)
    net = GConvNet(build_gconv_program(str(tmp_path / "depth2_latest_model.pth"), config_of(channels, kernels, depth).cnn), dev)
    try:
        _, got = net.forward(xs.to(dev), return_logits=True)
        got = got.cpu().numpy()
    finally:
        net.close()
    assert_all([check("trainer logits against float64", logits, lg64, logits_bar),
                check("inference family's logits against the trainer's", got, logits, logits_bar)])
