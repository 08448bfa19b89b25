"""The training kernels (csrc/train.hip, riser_amd.train) on the device against float64, on the shipped class: depth 1, every
kernel 3 (train_ref's net at that shape; the device helpers are train_device's).

Gap = largest absolute difference over a tensor / largest magnitude of the float64 tensor.  The bar of a tensor is four times
the gap torch's own fp32 autograd, run on the CPU, shows against float64 on the same inputs (the device sums in another order,
and the MFMA does not round as sequential FMAs do), with a floor of 1e-6; it is computed here at run time (train_ref.bars_of)
and never taken from the code under test.  Where a case has fragile elements (train_ref.fragile) the backward kernels are held
to the numpy float64 backward fed the DEVICE's selectors and gates: one kernel's rounding, not a decision fp32 may take the
other way.  Measured gaps and bars: profiles/train_gpu_tests.txt, DESIGN.md section 16.
"""
import os

import numpy as np
import pytest
import torch

import train_ref as R
from riser_amd import synth
from train_device import assert_all, check, config_of, held_to_numpy_backward, run_device, trainer_of

SMALL = ([3, 7, 18, 37], 3, 100, 11)            # crosses the 4-channel pad and the 16-column tile edge; rows 100, 50, 25 (odd), 12, 6
SLICES = ([5, 17, 33], 2, 9002, 23)             # layer 0 contracts 18 004 positions: several slices, the last not full
WIDTH = (list(synth.CHANNELS), 2, 4100, 23)     # the shipped 12-layer channel list


def shipped(channels):
    """the shape (channels, kernels, depth) of the shipped class"""
    return channels, [3] * len(channels), 1


def case_of(spec):
    channels, B, L, seed = spec
    sd = R.make_state(*shipped(channels), seed)
    x, y = R.make_batch(B, L, seed + 100)
    return shipped(channels), sd, x, y


@pytest.mark.gpu
def test_small_end_to_end_against_float64_autograd():
    shape, sd, x, y = case_of(SMALL)
    bars, _, loss_bar, _, (l64, g64, _, _) = R.bars_of(sd, x, y)
    assert sum(int(f.sum()) for f in R.fragile(R.forward64(sd, x))) == 0
    loss, grads = run_device(shape, sd, x, y)
    print(f"loss: device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(k, grads[k], g64[k], bars[k]) for k in g64])


@pytest.mark.gpu
def test_exact_ties_go_to_the_even_row():
    shape, seed = shipped(SMALL[0]), SMALL[3]
    sd = R.make_state(*shape, seed)
    x, y = R.constant_reads(3, 200)
    fwd = R.forward64(sd, x)
    z = fwd["z"][0]
    tied = (z[:, 0::2] == z[:, 1::2]).mean()
    assert tied >= 0.97, tied                               # every pair but each read's first and last
    bars, _, loss_bar, _, (l64, g64, _, _) = R.bars_of(sd, x, y)
    loss, grads, sel, _, _ = run_device(shape, sd, x, y, debug=True)
    assert np.array_equal(sel[0], fwd["sel"][0]) and int(sel[0][:, 1:-1].sum()) == 0
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(k, grads[k], g64[k], bars[k]) for k in g64])


@pytest.mark.gpu
def test_dead_units_give_zero_gradients_and_no_nan():
    channels, B, L, seed = SMALL
    shape = shipped(channels)
    sd = R.make_state(*shape, seed, bias=-50.0)
    x, y = R.make_batch(B, L, seed + 100)
    _, g64, _, _ = R.torch_loss_and_grads(sd, x, y)
    loss, grads = run_device(shape, sd, x, y)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    for k, g in grads.items():
        if k.startswith("layers.") or k == "classifier.2.weight":
            assert not g.any(), k
    assert R.gap_of(grads["classifier.2.bias"], g64["classifier.2.bias"]) <= 1e-6


@pytest.mark.gpu
def test_slice_boundaries():
    shape, sd, x, y = case_of(SLICES)
    B, L = x.shape
    t = trainer_of(shape, sd)
    n, s = t.slice_plan(0, B, L)
    t.close()
    assert n >= 3 and s % 4 == 0 and (n - 1) * s < B * L < n * s, (n, s)          # several slices, the last one not full
    held_to_numpy_backward(shape, sd, x, y)


@pytest.mark.gpu
def test_shipped_width():
    held_to_numpy_backward(*case_of(WIDTH))


def test_planted_defects_miss_by_more_than_ten_bars():
    """on the CPU: each defect planted in the float64 reference must be far outside the bars the device is held to"""
    shape, sd, x, y = case_of(SMALL)
    bars, dbars, _, _, _ = R.bars_of(sd, x, y)
    fwd = R.forward64(sd, x)
    good, good_dy = R.backward64(sd, fwd, y)

    def worst(grads, dys, bars, dbars, good, good_dy):
        return max([R.gap_of(grads[k], good[k]) / bars[k] for k in good] +
                   [R.gap_of(a, b) / d for a, b, d in zip(dys, good_dy, dbars)])

    for defect in R.SHIPPED_DEFECTS[1:]:
        grads, dys = R.backward64(sd, fwd, y, defect=defect)
        assert worst(grads, dys, bars, dbars, good, good_dy) > 10, defect
    xt, yt = R.constant_reads(3, 200)
    tbars, tdbars, _, _, _ = R.bars_of(sd, xt, yt)
    good, good_dy = R.backward64(sd, R.forward64(sd, xt), yt)
    grads, dys = R.backward64(sd, R.forward64(sd, xt, tie_to_odd=True), yt)
    assert worst(grads, dys, tbars, tdbars, good, good_dy) > 10, "tie_to_odd"


@pytest.mark.gpu
def test_same_state_and_batch_give_the_same_bits():
    shape, sd, x, y = case_of(SLICES)
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    t = trainer_of(shape, sd)
    l1, g1 = t.loss_and_grads(xs, ys)
    l2, g2 = t.loss_and_grads(xs, ys)
    assert l1 == l2 and all(torch.equal(g1[k], g2[k]) for k in g1)
    u = trainer_of(shape, sd)
    losses = [[tr.step(xs, ys) for _ in range(5)] for tr in (t, u)]
    a, b = t.state_dict(), u.state_dict()
    t.close()
    u.close()
    assert losses[0] == losses[1] and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k].numpy(), sd[k]) for k in a)


@pytest.mark.gpu
def test_five_adam_steps_against_torch_float64():
    shape, sd, x, y = case_of(SMALL)
    l64, p64 = R.torch_adam(sd, x, y, torch.float64, 5, 1e-3)
    l32, p32 = R.torch_adam(sd, x, y, torch.float32, 5, 1e-3)
    t = trainer_of(shape, sd, lr=1e-3)
    losses = [t.step(torch.from_numpy(x), torch.from_numpy(y)) for _ in range(5)]
    got = {k: v.numpy() for k, v in t.state_dict().items()}
    t.close()
    for i in range(5):
        bar = max(4 * abs(l32[i] - l64[i]) / abs(l64[i]), 1e-6)
        print(f"step {i}: loss {losses[i]!r} float64 {l64[i]!r} bar {bar:.3e}")
        assert abs(losses[i] - l64[i]) <= bar * abs(l64[i]), i
    assert_all([check(k, got[k], p64[k], max(4 * R.gap_of(p32[k], p64[k]), 1e-6)) for k in p64])


@pytest.mark.gpu
def test_state_dict_hands_over_to_model_and_torch():
    from riser_amd.model import Model
    shape = shipped(list(synth.FC_CHANNELS))
    sd = R.make_state(*shape, 31)
    x, y = R.make_batch(4, 4096, 131)
    dev = torch.device("cuda", 0)
    t = trainer_of(shape, sd)
    t.step(torch.from_numpy(x), torch.from_numpy(y))
    state = t.state_dict()
    logits = t.logits(torch.from_numpy(x), torch.from_numpy(y))
    t.close()
    assert list(state) == [k for i in range(4) for k in (f"layers.{i}.0.weight", f"layers.{i}.0.bias")] + \
        ["classifier.2.weight", "classifier.2.bias"]
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in state.values())
    probs = torch.softmax(logits.double(), 1).numpy()
    _, _, _, lg64 = R.torch_loss_and_grads({k: v.numpy() for k, v in state.items()}, x, y)
    assert np.abs(torch.softmax(torch.from_numpy(lg64), 1).numpy() - probs).max() <= 2e-4
    m = Model(state, config_of(*shape), None, "mRNA", device=dev)
    got = m.classify_batch(torch.from_numpy(x).to(dev)).cpu().numpy()
    m.close()
    assert np.abs(got - probs).max() <= 2e-4


@pytest.mark.gpu
def test_fit_end_to_end(tmp_path):
    from riser_amd import train as T
    channels = [8, 12, 16, 24]
    rng = np.random.RandomState(5)

    def make(n, L):
        neg = rng.standard_normal((n, L)).astype(np.float32)
        pos = (rng.standard_normal((n, L)) + 1.5 * np.sin(np.arange(L) / 3.0)).astype(np.float32)
        return torch.from_numpy(np.concatenate([neg, pos])), torch.cat((torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long)))

    train_sets = {k: make(64, L) for k, L in zip(T.LENGTH_KEYS, (256, 384, 512))}
    val_sets = {k: make(16, L) for k, L in zip(T.LENGTH_KEYS, (256, 384, 512))}
    torch.manual_seed(3)
    trainer = T.Trainer(config_of(*shipped(channels), lr=3e-3), None, device=torch.device("cuda", 0))
    exp_dir = str(tmp_path / "exp7")
    best_acc, best_epoch = T.fit(trainer, train_sets, val_sets, 2, 32, exp_dir, "exp7", seed=9, log=lambda *_: None)
    trainer.close()
    assert sorted(os.listdir(exp_dir)) == ["exp7_0_best_model.pth", "exp7_latest_model.pth", "metrics.tsv"]
    rows = [line.split("\t") for line in open(os.path.join(exp_dir, "metrics.tsv")).read().splitlines()]
    assert rows[0] == list(T.METRICS) and [r[0] for r in rows[1:]] == ["0", "1"] and all(len(r) == 7 for r in rows)
    assert float(rows[2][1]) < float(rows[1][1]), "the training loss of the last epoch is not below the first's"
    assert 0 <= best_epoch <= 1 and best_acc == max(float(r[3]) for r in rows[1:])
    sd = torch.load(os.path.join(exp_dir, "exp7_latest_model.pth"))
    assert {k: tuple(v.shape) for k, v in sd.items()} == T.param_shapes(channels)
