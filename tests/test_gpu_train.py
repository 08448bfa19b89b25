"""The training kernels (csrc/train.hip, riser_amd.train) on the device against float64.

Gap = largest absolute difference over a tensor / largest magnitude of the float64 tensor.  The bar of a tensor is four times
the gap torch's own fp32 autograd, run on the CPU, shows against float64 on the same inputs (the device sums in another order,
and the MFMA does not round as sequential FMAs do), with a floor of 1e-6; it is computed here at run time (train_ref.bars_of)
and never taken from the code under test.  Where a case has fragile elements (train_ref.fragile) the backward kernels are held
to the numpy float64 backward fed the DEVICE's selectors and gates: one kernel's rounding, not a decision fp32 may take the
other way.  Measured gaps and bars: profiles/train_gpu_tests.txt, DESIGN.md section 16.
"""
import os
import types

import numpy as np
import pytest
import torch

import train_ref as R
from riser_amd import synth

SMALL = ([3, 7, 18, 37], 3, 100, 11)            # crosses the 4-channel pad and the 16-column tile edge; rows 100, 50, 25 (odd), 12, 6
SLICES = ([5, 17, 33], 2, 9002, 23)             # layer 0 contracts 18 004 positions: several slices, the last not full
WIDTH = (list(synth.CHANNELS), 2, 4100, 23)     # the shipped 12-layer channel list


def config_of(channels, lr=1e-3):
    return types.SimpleNamespace(model="cnn", learning_rate=lr, cnn=synth.CnnConfig(channels=channels, kernels=[3] * len(channels)))


def case_of(spec):
    channels, B, L, seed = spec
    sd = R.make_state(channels, seed)
    x, y = R.make_batch(B, L, seed + 100)
    return channels, sd, x, y


def trainer_of(channels, sd, lr=1e-3):
    from riser_amd.train import Trainer
    return Trainer(config_of(channels, lr), sd, device=torch.device("cuda", 0))


def run_device(channels, sd, x, y, debug=False):
    """-> loss, {key: grad as float64 numpy}, and with debug the device's per-layer (sel, gate, dy)"""
    t = trainer_of(channels, sd)
    try:
        loss, grads = t.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
        grads = {k: v.numpy().astype(np.float64) for k, v in grads.items()}
        if not debug:
            return loss, grads
        B, L = x.shape
        sel = [t.debug_copy(l, "sel", B, L).numpy() for l in range(len(channels))]
        gate = [t.debug_copy(l, "y", B, L).numpy() > 0 for l in range(len(channels))]
        dy = [t.debug_copy(l, "dy", B, L).numpy().astype(np.float64) for l in range(len(channels))]
        return loss, grads, sel, gate, dy
    finally:
        t.close()


def check(name, got, want, bar):
    gap = R.gap_of(got, want)
    print(f"{name}: gap {gap:.3e} bar {bar:.3e}")
    return gap <= bar, f"{name}: gap {gap:.3e} > bar {bar:.3e}"


def assert_all(results):
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_small_end_to_end_against_float64_autograd():
    channels, sd, x, y = case_of(SMALL)
    bars, _, loss_bar, (l64, g64, _, _) = R.bars_of(sd, x, y)
    assert sum(int(f.sum()) for f in R.fragile(R.forward64(sd, x))) == 0
    loss, grads = run_device(channels, sd, x, y)
    print(f"loss: device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(k, grads[k], g64[k], bars[k]) for k in g64])


def constant_reads(B, L):
    return np.repeat(np.array([0.75, -1.25, 0.5], np.float32)[:B, None], L, axis=1), np.array([1, 0, 1])[:B]


@pytest.mark.gpu
def test_exact_ties_go_to_the_even_row():
    channels, seed = SMALL[0], SMALL[3]
    sd = R.make_state(channels, seed)
    x, y = constant_reads(3, 200)
    fwd = R.forward64(sd, x)
    z = fwd["z"][0]
    tied = (z[:, 0::2] == z[:, 1::2]).mean()
    assert tied >= 0.97, tied                               # every pair but each read's first and last
    bars, _, loss_bar, (l64, g64, _, _) = R.bars_of(sd, x, y)
    loss, grads, sel, _, _ = run_device(channels, sd, x, y, debug=True)
    assert np.array_equal(sel[0], fwd["sel"][0]) and int(sel[0][:, 1:-1].sum()) == 0
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(k, grads[k], g64[k], bars[k]) for k in g64])


@pytest.mark.gpu
def test_dead_units_give_zero_gradients_and_no_nan():
    channels, B, L, seed = SMALL
    sd = R.make_state(channels, seed, bias=-50.0)
    x, y = R.make_batch(B, L, seed + 100)
    _, g64, _, _ = R.torch_loss_and_grads(sd, x, y)
    loss, grads = run_device(channels, sd, x, y)
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    for k, g in grads.items():
        if k.startswith("layers.") or k == "classifier.2.weight":
            assert not g.any(), k
    assert R.gap_of(grads["classifier.2.bias"], g64["classifier.2.bias"]) <= 1e-6


def held_to_numpy_backward(spec, want_slices=False):
    channels, sd, x, y = case_of(spec)
    B, L = x.shape
    bars, dbars, loss_bar, (l64, _, _, _) = R.bars_of(sd, x, y)
    fwd = R.forward64(sd, x)
    frag = R.fragile(fwd)
    if want_slices:
        t = trainer_of(channels, sd)
        n, s = t.slice_plan(0, B, L)
        t.close()
        assert n >= 3 and s % 4 == 0 and (n - 1) * s < B * L < n * s, (n, s)      # several slices, the last one not full
    loss, grads, sel, gate, dy = run_device(channels, sd, x, y, debug=True)
    for l in range(len(channels)):
        differs = (sel[l] != fwd["sel"][l]) & fwd["gate"][l] & gate[l]              # a selector matters where a gradient flows
        assert not (differs & ~frag[l]).any(), f"layer {l}: a selector differs from float64's outside the fragile elements"
        assert not ((gate[l] != fwd["gate"][l]) & ~frag[l]).any(), f"layer {l}: a gate differs outside the fragile elements"
    g_ref, dy_ref = R.backward64(sd, fwd, y, sels=sel, gates=gate)
    print(f"loss: device {loss!r} float64 {l64!r}")
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(k, grads[k], g_ref[k], bars[k]) for k in g_ref] +
               [check(f"dY_{l}", dy[l], dy_ref[l], dbars[l]) for l in range(len(channels))])


@pytest.mark.gpu
def test_slice_boundaries():
    held_to_numpy_backward(SLICES, want_slices=True)


@pytest.mark.gpu
def test_shipped_width():
    held_to_numpy_backward(WIDTH)


def test_planted_defects_miss_by_more_than_ten_bars():
    """on the CPU: each defect planted in the float64 reference must be far outside the bars the device is held to"""
    channels, sd, x, y = case_of(SMALL)
    bars, dbars, _, _ = R.bars_of(sd, x, y)
    fwd = R.forward64(sd, x)
    good, good_dy = R.backward64(sd, fwd, y)

    def worst(grads, dys, bars, dbars, good, good_dy):
        return max([R.gap_of(grads[k], good[k]) / bars[k] for k in good] +
                   [R.gap_of(a, b) / d for a, b, d in zip(dys, good_dy, dbars)])

    for defect in R.DEFECTS[1:]:
        grads, dys = R.backward64(sd, fwd, y, defect=defect)
        assert worst(grads, dys, bars, dbars, good, good_dy) > 10, defect
    xt, yt = constant_reads(3, 200)
    tbars, tdbars, _, _ = R.bars_of(sd, xt, yt)
    good, good_dy = R.backward64(sd, R.forward64(sd, xt), yt)
    grads, dys = R.backward64(sd, R.forward64(sd, xt, tie_to_odd=True), yt)
    assert worst(grads, dys, tbars, tdbars, good, good_dy) > 10, "tie_to_odd"


@pytest.mark.gpu
def test_same_state_and_batch_give_the_same_bits():
    channels, sd, x, y = case_of(SLICES)
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    t = trainer_of(channels, sd)
    l1, g1 = t.loss_and_grads(xs, ys)
    l2, g2 = t.loss_and_grads(xs, ys)
    assert l1 == l2 and all(torch.equal(g1[k], g2[k]) for k in g1)
    u = trainer_of(channels, sd)
    losses = [[tr.step(xs, ys) for _ in range(5)] for tr in (t, u)]
    a, b = t.state_dict(), u.state_dict()
    t.close()
    u.close()
    assert losses[0] == losses[1] and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k].numpy(), sd[k]) for k in a)


def torch_adam(sd, x, y, dtype, steps, lr):
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    losses = []
    for _ in range(steps):
        h = torch.tensor(x, dtype=dtype).unsqueeze(1)
        for i in range(R.n_layers_of(sd)):
            h = torch.nn.functional.max_pool1d(torch.relu(torch.nn.functional.conv1d(
                h, p[f"layers.{i}.0.weight"], p[f"layers.{i}.0.bias"], padding=1)), 2, 2)
        loss = torch.nn.functional.cross_entropy(h.mean(2) @ p["classifier.2.weight"].T + p["classifier.2.bias"],
                                                 torch.tensor(y, dtype=torch.long))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach().double().numpy() for k, v in p.items()}


@pytest.mark.gpu
def test_five_adam_steps_against_torch_float64():
    channels, sd, x, y = case_of(SMALL)
    l64, p64 = torch_adam(sd, x, y, torch.float64, 5, 1e-3)
    l32, p32 = torch_adam(sd, x, y, torch.float32, 5, 1e-3)
    t = trainer_of(channels, sd, lr=1e-3)
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
    channels = list(synth.FC_CHANNELS)
    sd = R.make_state(channels, 31)
    x, y = R.make_batch(4, 4096, 131)
    dev = torch.device("cuda", 0)
    t = trainer_of(channels, sd)
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
    m = Model(state, config_of(channels), None, "mRNA", device=dev)
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
    trainer = T.Trainer(config_of(channels, lr=3e-3), None, device=torch.device("cuda", 0))
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
