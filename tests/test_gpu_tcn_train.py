"""TCN training on the device (csrc/tcn_train.hip, riser_amd.tcn_train.TcnTrainer) against float64.

Gap = largest absolute difference over a tensor / largest magnitude of the float64 tensor.  The bar of a tensor is four times
the gap torch's own fp32 autograd, run on the CPU on the dense net, shows against float64 on the same inputs and the same
dropout masks, with a floor of 1e-6; it is computed here at run time (tcn_train_ref.bars_of), never taken from the code under
test.  The device's gates (a1, a2, out > 0) must equal float64's outside the fragile elements (tcn_train_ref.fragile), and the
backward is held to the numpy float64 cone backward fed the DEVICE's gates.  The nets are the golden TCNs of tests/golden.
Measured gaps and bars: profiles/tcn_train_gpu_tests.txt, DESIGN.md section 18.
"""
import functools
import types

import numpy as np
import pytest
import torch

import tcn_train_ref as R
from train_device import assert_all, check

DROP_SEED = 7
NAMES = [n for _, n in R.NETS]
WHATS = ("a1", "a2", "out", "da1", "dout")


def config_of(cfg, dropout, lr=1e-3):
    tcn = {k: v for k, v in cfg.items() if k not in ("model", "rf", "lengths")}
    tcn["dropout"] = dropout
    return types.SimpleNamespace(model="tcn", learning_rate=lr, tcn=types.SimpleNamespace(**tcn))


def trainer_of(cfg, sd, p, lr=1e-3):
    from riser_amd.tcn_train import TcnTrainer
    return TcnTrainer(config_of(cfg, p, lr), sd, seed=DROP_SEED)


def run_device(t, x, y, debug=False):
    """(loss, logits of the training forward, {key: grad}, [per block {what: array}]) of one forward + backward"""
    B, L = x.shape
    loss, _, logits = t._call("rs_tcn_train_forward_backward", torch.from_numpy(x), torch.from_numpy(y))
    grads = {k: v.numpy() for k, v in t._tensors("rs_tcn_train_get_grads").items()}
    bufs = [{w: t.debug_copy(i, w, B, L).numpy() for w in WHATS} for i in range(t.net["n_layers"])] if debug else None
    return loss, logits.numpy(), grads, bufs


@functools.lru_cache(maxsize=None)
def reference(name, L, p):
    """what the case's tests share: the batch, the masks of step 0, the float64 cone forward, the bars"""
    cfg, sd = R.load_net(name)
    x, y = R.make_batch(R.B_CASE, L, R.case_seed(name, L))
    masks = R.masks_of(cfg, R.B_CASE, L, p, DROP_SEED, 0)
    fwd = R.forward64(sd, cfg, x, p, masks)
    bars = R.bars_of(sd, cfg, x, y, p, R.dense_masks(cfg, R.B_CASE, L, p, DROP_SEED, 0))
    return cfg, sd, x, y, fwd, bars


def cases():
    for name in NAMES:
        cfg, _ = R.load_net(name)
        for L in R.lengths_of(name, cfg):
            for p in (0.0, 0.2):
                yield name, L, p


@pytest.mark.gpu
@pytest.mark.parametrize("name,L,p", list(cases()))
def test_loss_logits_and_every_gradient_against_float64(name, L, p):
    cfg, sd, x, y, fwd, (bars, dbars, loss_bar, logit_bar, (l64, g64, d64, _, lg64)) = reference(name, L, p)
    t = trainer_of(cfg, sd, p)
    try:
        if name == "tcn_k3_b2" and L == cfg["rf"] + 37:    # block 0's conv1 crosses slice boundaries, the last slice short
            n, s, rows = t.slice_plan(0, 0, R.B_CASE, L)
            assert n >= 2 and s % 4 == 0 and (n - 1) * s < R.B_CASE * rows < n * s, (n, s, rows)
        loss, logits, grads, bufs = run_device(t, x, y, debug=True)
    finally:
        t.close()
    label = f"{name} L {L} p {p}"
    print(f"{label} loss: device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert abs(loss - l64) <= loss_bar * abs(l64)
    results = [check(f"{label} logits", logits, lg64, logit_bar)]
    frag = R.fragile(fwd)
    gates = []
    for i, (blk, dev) in enumerate(zip(fwd["blocks"], bufs)):
        dev_gates = tuple(dev[w] > 0 for w in ("a1", "a2", "out"))
        for w, dg, fr in zip(("a1", "a2", "out"), dev_gates, frag[i]):
            assert np.array_equal(dg | fr, (blk[w] > 0) | fr), f"{label}: block {i} gate of {w}"
        gates.append(dev_gates)
    want, douts, _ = R.backward64(sd, cfg, fwd, y, p, gates=gates)
    assert set(grads) == set(want) == set(R.device_keys(cfg))
    results += [check(f"{label} {k}", grads[k], want[k], bars[k]) for k in want]
    results += [check(f"{label} block {i} dOut", bufs[i]["dout"], douts[i], dbars[i]) for i in range(cfg["n_layers"])]
    assert_all(results)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("name", ["tcn_k3_b2", "tcn_k5_b3", "tcn_f68"])
def test_a_longer_read_gives_the_bits_of_its_own_tail(name, p):
    cfg, sd = R.load_net(name)
    rf = cfg["rf"]
    x, y = R.make_batch(R.B_CASE, rf + 37, 5)
    got = []
    for xs in (x, np.ascontiguousarray(x[:, 37:])):
        t = trainer_of(cfg, sd, p)
        try:
            loss, logits, grads, _ = run_device(t, xs, y)
        finally:
            t.close()
        got.append((loss, logits, grads))
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])
    assert all(np.array_equal(got[0][2][k], got[1][2][k]) for k in got[0][2])
    assert any(np.abs(g).max() > 0 for g in got[0][2].values())


@pytest.mark.gpu
def test_same_state_and_batch_give_the_same_bits_whatever_the_workspace_held():
    cfg, sd = R.load_net("tcn_k3_b2")
    x, y = R.make_batch(R.B_CASE, cfg["rf"] + 37, 6)
    t = trainer_of(cfg, sd, 0.2)
    try:
        first = run_device(t, x, y, debug=True)
        t.set_dropout(0.2, DROP_SEED, 0)
        t._ws.fill_(0xFF)                                   # every float a NaN: nothing is read before it is written
        second = run_device(t, x, y, debug=True)
        third = run_device(t, x, y)                         # the counter moved: another mask
    finally:
        t.close()
    assert first[0] == second[0] and np.array_equal(first[1], second[1])
    assert all(np.array_equal(first[2][k], second[2][k]) for k in first[2])
    assert all(np.array_equal(a[w], b[w]) for a, b in zip(first[3], second[3]) for w in WHATS)
    assert third[0] != first[0]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_five_adam_steps_against_torch_float64(p):
    cfg, sd = R.load_net("tcn_k3_b2")
    L = cfg["rf"] + 37
    x, y = R.make_batch(R.B_CASE, L, 8)
    masks = (lambda step: R.dense_masks(cfg, R.B_CASE, L, p, DROP_SEED, step)) if p else None
    l64, p64 = R.torch_adam(sd, cfg, x, y, torch.float64, 5, 1e-3, p, masks)
    l32, p32 = R.torch_adam(sd, cfg, x, y, torch.float32, 5, 1e-3, p, masks)
    t = trainer_of(cfg, sd, p, lr=1e-3)
    try:
        losses = [t.step(torch.from_numpy(x), torch.from_numpy(y)) for _ in range(5)]
        got = {k: v.numpy() for k, v in t.state_dict().items()}
    finally:
        t.close()
    for i in range(5):
        bar = max(4 * abs(l32[i] - l64[i]) / abs(l64[i]), 1e-6)
        print(f"p {p} step {i}: loss {losses[i]!r} float64 {l64[i]!r} bar {bar:.3e}")
        assert abs(losses[i] - l64[i]) <= bar * abs(l64[i]), i
    assert list(got) == list(sd)
    assert_all([check(f"p {p} adam {k}", got[k], p64[k], max(4 * R.gap_of(p32[k], p64[k]), 1e-6)) for k in R.device_keys(cfg)])
    for i in range(1, cfg["n_layers"]):                     # built, never applied: the bits they came in with
        for tail in ("weight", "bias"):
            k = f"layers.{i}.shortcut.{tail}"
            assert np.array_equal(got[k], sd[k]) and np.array_equal(p64[k], sd[k].astype(np.float64)), k
    assert any(not np.array_equal(got[k], sd[k]) for k in R.device_keys(cfg))


PLAN = ((3, 0), (5, 37), (2, 0), (5, 37), (1, -60))        # (reads, samples beyond the receptive field): the workspace regrows


def batch_of(cfg, step):
    B, extra = PLAN[step]
    return R.make_batch(B, cfg["rf"] + extra, 40 + step)


@pytest.mark.gpu
def test_a_sequence_of_calls_equals_fresh_handles():
    """one handle through three lengths, short batches, an evaluate of another shape in front of every step and an Adam step
    behind it, against a fresh handle per step given the parameters and the dropout counter the sequence had reached"""
    cfg, sd = R.load_net("tcn_k3_b2")
    t = trainer_of(cfg, sd, 0.2)
    seen = []
    try:
        for step in range(len(PLAN)):
            x, y = batch_of(cfg, step)
            t.evaluate(torch.from_numpy(x[:1, 5:]), torch.from_numpy(y[:1]))
            state = {k: v.numpy().copy() for k, v in t.state_dict().items()}
            loss, grads = t.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
            t._adam()
            seen.append((state, loss, {k: v.numpy() for k, v in grads.items()}))
    finally:
        t.close()
    assert any(not np.array_equal(seen[0][0][k], seen[-1][0][k]) for k in seen[0][0])
    for step, (state, loss, grads) in enumerate(seen):
        x, y = batch_of(cfg, step)
        u = trainer_of(cfg, state, 0.2)
        try:
            u.set_dropout(0.2, DROP_SEED, step)
            loss_u, grads_u = u.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
        finally:
            u.close()
        assert loss == loss_u, step
        assert all(np.array_equal(grads[k], grads_u[k].numpy()) for k in grads), step


@pytest.mark.gpu
def test_bad_labels_are_refused_and_debug_copy_follows_the_last_call():
    from riser_amd import _native as nv
    cfg, sd = R.load_net("tcn_k5_l1")
    x, y = R.make_batch(R.B_CASE, 20, 9)
    t = trainer_of(cfg, sd, 0.2)
    try:
        before = {k: v.numpy() for k, v in t.state_dict().items()}
        for bad in (2, -1):
            yb = y.copy()
            yb[3] = bad
            with pytest.raises(nv.NativeError, match="label"):
                t.loss_and_grads(torch.from_numpy(x), torch.from_numpy(yb))
            with pytest.raises(nv.NativeError):
                t.debug_copy(0, "out", R.B_CASE, 20)
        after = {k: v.numpy() for k, v in t.state_dict().items()}
        assert all(np.array_equal(before[k], after[k]) for k in before)
        # the refused calls did not count: the next call has the mask of step 0
        loss, grads = t.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
        t.debug_copy(0, "out", R.B_CASE, 20)
        u = trainer_of(cfg, sd, 0.2)
        loss_u, grads_u = u.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
        u.close()
        assert loss == loss_u and all(torch.equal(grads[k], grads_u[k]) for k in grads)
        t.evaluate(torch.from_numpy(x), torch.from_numpy(y))
        with pytest.raises(nv.NativeError):
            t.debug_copy(0, "out", R.B_CASE, 20)
    finally:
        t.close()


@pytest.mark.gpu
def test_a_dead_net_gives_exact_zeros_and_no_nan():
    cfg, sd = R.load_net("tcn_k3_b2")
    sd = {k: (np.full_like(v, -50.0) if ".blocks." in k and k.endswith(".bias") else v) for k, v in sd.items()}
    x, y = R.make_batch(R.B_CASE, cfg["rf"], 10)
    t = trainer_of(cfg, sd, 0.2)
    try:
        loss, logits, grads, bufs = run_device(t, x, y, debug=True)
    finally:
        t.close()
    assert np.isfinite(loss) and np.isfinite(logits).all() and all(np.isfinite(g).all() for g in grads.values())
    assert all(not b["a1"].any() and not b["a2"].any() for b in bufs)
    for k, g in grads.items():
        if ".blocks." in k:
            assert not g.any(), k
    _, g64, _, _, _ = R.torch_loss_and_grads(sd, cfg, x, y)
    assert R.gap_of(grads["linear.bias"], g64["linear.bias"]) <= 1e-6


@pytest.mark.gpu
def test_a_checkpoint_loads_into_model(tmp_path):
    from riser_amd.model import Model
    cfg, sd, x, y, _, _ = reference("tcn_k3_b2", 162, 0.0)
    t = trainer_of(cfg, sd, 0.2)
    try:
        t.step(torch.from_numpy(x), torch.from_numpy(y))
        path = str(tmp_path / "tcn_latest_model.pth")
        torch.save(t.state_dict(), path)
        own = t.logits(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    finally:
        t.close()
    state = torch.load(path)
    assert list(state) == list(sd)
    m = Model(path, config_of(cfg, 0.2), None, "mRNA", dtype="f32")
    try:
        _, logits = m.forward_batch(torch.from_numpy(x).to(m.device), np.full(len(x), x.shape[1], np.int32), return_logits=True)
    finally:
        m.close()
    trained = {k: v.numpy() for k, v in state.items()}
    logit_bar = R.bars_of(trained, cfg, x, y)[3]            # eval mode: no mask
    lg = R.forward64(trained, cfg, x)["logits"]
    print(f"logits: trainer gap {R.gap_of(own, lg):.3e} Model gap {R.gap_of(logits.cpu().numpy(), lg):.3e} bar {logit_bar:.3e}")
    assert R.gap_of(own, lg) <= logit_bar and R.gap_of(logits.cpu().numpy(), lg) <= logit_bar
