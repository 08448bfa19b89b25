"""The call surface of the training family (csrc/train.hip, riser_amd.train) on the device: what a call returns must be a
function of the handle's state and that call's batch alone - never of the calls before it, of what the workspace held, of a
padded row pitch - and the paths a real fit() takes beside the backward kernels (evaluate, the loss edges, the label check,
load_state_dict, Adam by itself) against float64.

Every test runs once on the shipped class (`Trainer`, channels [3, 7, 18, 37]) and once on train_ref.CASES["depth2"]
(`GenericTrainer`), at B <= 16 and L <= 1001.  Bit equality (`==`, torch.equal) is the bar wherever two runs of the same
arithmetic are compared: csrc/train/plan.hpp makes every sum a function of (B, L, shapes) alone, and
test_same_state_and_batch_give_the_same_bits holds run-to-run determinism.  Against float64 the bars are train_ref.bars_of's:
four times the gap of torch's own fp32 CPU run, floor 1e-6, computed here at run time and never from the device.  Measured
gaps and bars: profiles/train_calls_gpu_tests.txt, DESIGN.md sections 16 and 17.
"""
import math

import numpy as np
import pytest
import torch

import train_calls_ref as T
import train_ref as R
from train_device import assert_all, check

kinds = pytest.mark.parametrize("kind", T.KINDS)


def numpy_of(tensors):
    return {k: v.numpy().copy() for k, v in tensors.items()}


def alone(kind, sd, backward, x, y):
    """the call on a handle that has seen nothing else"""
    t = T.trainer_of(kind, sd)
    try:
        return T.full_call(t, backward, x, y)
    finally:
        t.close()


@pytest.mark.gpu
@kinds
def test_a_calls_bits_do_not_depend_on_the_calls_before_it(kind):
    """three read lengths interleaved, an odd length, the shortest read, an odd row at level 0 and a workspace that regrows,
    on ONE handle: every call returns the bits a fresh handle returns for that call alone"""
    sd = T.make_state(kind, 11)
    seq = [(True, 4, 1000), (True, 3, 100), (False, 2, 333), (True, 1, T.min_length(kind)), (True, 5, 101), (False, 6, 1001),
           (True, 3, 100)]
    batches = [T.batch_of(B, L, 300 + (1 if i == 6 else i)) for i, (_, B, L) in enumerate(seq)]     # steps 2 and 7: one batch
    t = T.trainer_of(kind, sd)
    got, sizes = [], []
    try:
        for (backward, B, L), (x, y) in zip(seq, batches):
            got.append(T.full_call(t, backward, x, y))
            sizes.append(t._ws.numel())
    finally:
        t.close()
    assert sizes[5] > sizes[4] and sizes[6] == sizes[5], sizes        # the workspace regrew at step 6 and was reused behind it
    for i, ((backward, B, L), (x, y)) in enumerate(zip(seq, batches)):
        want = alone(kind, sd, backward, x, y)
        assert got[i][2].shape == (B, 2) and np.isfinite(got[i][0])
        if backward:
            assert T.same_bits(got[i], want), f"step {i + 1}: {B} x {L} differs from the same call on a fresh handle"
        else:
            assert got[i][:2] == want[:2] and torch.equal(got[i][2], want[2]), f"step {i + 1}: evaluate {B} x {L} differs"
            assert T.same_tensors(got[i][3], got[i - 1][3]), f"step {i + 1}: evaluate moved the gradients of step {i}"
    assert T.same_bits(got[1], got[6]), "steps 2 and 7 ran the same batch on the same state"
    assert any(bool(g.any()) for g in got[6][3].values())


@pytest.mark.gpu
@kinds
def test_the_same_across_updates_and_through_load_state_dict(kind):
    """step and evaluate interleaved at different shapes; after every step the state is loaded into a handle made from OTHER
    weights (rs_train_set_params and its re-pack of the two MFMA weight forms), which must then give the bits of a handle
    constructed from that state.

    load_state_dict replaces the parameters only: the Adam moments and the step count of the handle stay as they are
    (riser_amd.train: "a resumed run starts a fresh Adam" is the constructor's doing, not this call's).  Pinned below: loading
    a handle's own state is a no-op on its next step, and that step is not a fresh handle's first step."""
    sd = T.make_state(kind, 11)
    probe_x, probe_y = T.batch_of(3, 100, 411)
    plan = [("step", 4, 1000), ("evaluate", 2, 333), ("step", 3, 100), ("evaluate", 6, 1001), ("step", 5, 101)]
    a, b = T.trainer_of(kind, sd), T.trainer_of(kind, T.make_state(kind, 77))
    try:
        for i, (op, B, L) in enumerate(plan):
            x, y = T.batch_of(B, L, 400 + i)
            if op == "evaluate":
                a.evaluate(x, y)
                continue
            a.step(x, y)
            state = a.state_dict()
            assert any(not np.array_equal(state[k].numpy(), sd[k]) for k in state)
            b.load_state_dict(state)
            assert T.same_tensors(b.state_dict(), state)
            c = T.trainer_of(kind, state)
            try:
                for backward in (True, False):
                    assert T.same_bits(T.full_call(b, backward, probe_x, probe_y), T.full_call(c, backward, probe_x, probe_y)), \
                        f"after step {i + 1}: the loaded handle differs from one constructed from the state ({backward})"
            finally:
                c.close()
    finally:
        a.close()
        b.close()
    # the moments and the step count survive load_state_dict
    x1, y1 = T.batch_of(3, 100, 421)
    x2, y2 = T.batch_of(5, 101, 422)
    h, u = T.trainer_of(kind, sd), T.trainer_of(kind, sd)
    try:
        assert h.step(x1, y1) == u.step(x1, y1)
        s1 = h.state_dict()
        h.load_state_dict(s1)                               # its own state: the parameters do not change
        fresh = T.trainer_of(kind, s1)
        try:
            losses = [tr.step(x2, y2) for tr in (h, u, fresh)]
            after = [tr.state_dict() for tr in (h, u, fresh)]
        finally:
            fresh.close()
    finally:
        h.close()
        u.close()
    assert losses[0] == losses[1] == losses[2]              # the same parameters saw the same batch
    assert T.same_tensors(after[0], after[1]), "load_state_dict moved the Adam moments or the step count"
    assert not T.same_tensors(after[0], after[2]), "a second step equals a fresh handle's first: the moments were reset"


def raw_call(lib, h, n_tensors_of, x, labels, B, L, ld, fill):
    """rs_train_forward_backward in a test-owned workspace of exactly rs_train_workspace_bytes bytes filled with `fill` ->
    (out vector, [gradient tensors]) on the host"""
    from riser_amd import _native as nv
    dev = x.device
    need = lib.rs_train_workspace_bytes(h, B, L)
    assert need > 0
    ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
    out = torch.full((2 + 2 * B,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    nv.check(lib.rs_train_forward_backward(h, x.data_ptr(), labels.data_ptr(), B, L, ld, ws.data_ptr(), need, out.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream), "rs_train_forward_backward")
    grads = []
    for i, shape in enumerate(n_tensors_of):
        a = np.empty(shape, np.float32)
        nv.check(lib.rs_train_get_grads(h, i, a.ctypes.data, a.size), "rs_train_get_grads")
        grads.append(a)
    return out.cpu().numpy(), grads


@pytest.mark.gpu
@kinds
def test_the_workspaces_contents_do_not_matter(kind):
    """the raw C ABI in a workspace of 0x00, 0xFF (NaN floats, selector 255) and 0x7F (3.4e38, selector 127) bytes: every pad
    channel, dropped odd row and short last slice is guarded, so the bits are the same; and a row pitch ld > L with NaN behind
    column L gives the bits of the contiguous call"""
    from riser_amd import _native as nv
    from riser_amd.train import param_shapes
    lib = nv.lib()
    shapes = list(param_shapes(*T.NETS[kind]).values())
    sd = T.make_state(kind, 11)
    dev = torch.device("cuda", 0)
    h = T.raw_handle(kind, sd, 0)
    try:
        for B, L, seed in ((3, 100, 501), (5, 101, 502)):
            x, y = T.batch_of(B, L, seed)
            xd, yd = x.to(dev).contiguous(), y.to(dev, dtype=torch.int32).contiguous()
            runs = {fill: raw_call(lib, h, shapes, xd, yd, B, L, L, fill) for fill in (0x00, 0xFF, 0x7F)}
            out0, g0 = runs[0x00]
            assert np.isfinite(out0).all() and all(np.isfinite(g).all() for g in g0) and any(g.any() for g in g0)
            for fill in (0xFF, 0x7F):
                out, g = runs[fill]
                assert np.array_equal(out, out0, equal_nan=True), f"{B} x {L}: the fill {fill:#x} changed loss, count or logits"
                for i, (a, b) in enumerate(zip(g, g0)):
                    assert np.array_equal(a, b, equal_nan=True), f"{B} x {L}: the fill {fill:#x} changed gradient tensor {i}"
            wide = torch.full((B, L + 37), float("nan"), dtype=torch.float32)
            wide[:, :L] = x
            out, g = raw_call(lib, h, shapes, wide.to(dev).contiguous(), yd, B, L, L + 37, 0xFF)
            assert np.array_equal(out, out0, equal_nan=True), f"{B} x {L}: ld = L + 37 changed loss, count or logits"
            for i, (a, b) in enumerate(zip(g, g0)):
                assert np.array_equal(a, b, equal_nan=True), f"{B} x {L}: ld = L + 37 changed gradient tensor {i}"
    finally:
        lib.rs_train_destroy(h)


@pytest.mark.gpu
@kinds
def test_debug_copy_refuses_after_an_evaluate(kind):
    """rs_train_debug_copy reads the workspace at the offsets of the last forward + backward; an evaluate of another shape
    carves the same workspace at other offsets, so behind it the hook refuses (RS_ERR_ARG) instead of returning a mixture.
    The evaluate is smaller than the backward call: the workspace is not reallocated."""
    from riser_amd._native import NativeError
    sd = T.make_state(kind, 11)
    x, y = T.batch_of(3, 100, 601)
    xe, ye = T.batch_of(2, 50, 602)
    n_convs = len(T.conv_shapes(kind))
    pools = [j % T.NETS[kind][2] == T.NETS[kind][2] - 1 for j in range(n_convs)]

    def window(t):
        return [t.debug_copy(j, what, 3, 100) for j in range(n_convs) for what in ("y", "sel", "dy") if what != "sel" or pools[j]]

    t = T.trainer_of(kind, sd)
    try:
        with pytest.raises(NativeError, match="no rs_train_forward_backward has run"):
            t.debug_copy(0, "y", 3, 100)
        t.loss_and_grads(x, y)
        first = window(t)
        assert any(bool(w.any()) for w in first)
        size = t._ws.numel()
        t.evaluate(xe, ye)
        assert t._ws.numel() == size
        for j in range(n_convs):
            with pytest.raises(NativeError, match="since the last rs_train_evaluate"):
                t.debug_copy(j, "y", 3, 100)
        with pytest.raises(NativeError):                    # a refused call leaves nothing to look at either
            t.loss_and_grads(x, torch.full((3,), 2))
        with pytest.raises(NativeError, match="since the last rs_train_evaluate"):
            t.debug_copy(0, "dy", 3, 100)
        t.loss_and_grads(x, y)
        again = window(t)
    finally:
        t.close()
    assert len(first) == len(again) and all(torch.equal(a, b) for a, b in zip(first, again))


def balanced_case(kind):
    """B = 16, L = 100; classifier.2.bias[0] shifted by the median float64 margin l1 - l0, so that float64 predicts eight
    reads of each class"""
    seed = {"shipped": 11, "generic": 12}[kind]
    sd = T.make_state(kind, seed)
    x, y = R.make_batch(16, 100, seed + 100)
    lg = R.torch_loss_and_grads(sd, x, y)[3]
    sd["classifier.2.bias"] = sd["classifier.2.bias"].copy()
    sd["classifier.2.bias"][0] += np.float32(np.median(lg[:, 1] - lg[:, 0]))
    return sd, x, y


@pytest.mark.gpu
@kinds
def test_evaluate_against_float64(kind):
    sd, x, y = balanced_case(kind)
    _, _, loss_bar, logits_bar, (l64, _, _, lg64) = R.bars_of(sd, x, y)
    lg32 = R.torch_loss_and_grads(sd, x, y, torch.float32)[3]
    margin = lg64[:, 1] - lg64[:, 0]
    fp32_gap = float(np.abs(lg32 - lg64).max())
    print(f"{kind} evaluate: smallest |l1 - l0| {np.abs(margin).min():.3e}, torch fp32 against float64 logits {fp32_gap:.3e}")
    assert int((margin > 0).sum()) == 8, "float64 does not predict eight reads of each class"
    assert np.abs(margin).min() >= 100 * fp32_gap, "a read sits too close to the decision for fp32 to be held to float64's count"
    want_count = int(((margin > 0).astype(np.int64) == y).sum())
    xs, ys = torch.from_numpy(x), torch.from_numpy(y)
    t = T.trainer_of(kind, sd)
    try:
        x0, y0 = T.batch_of(3, 100, 701)
        _, grads_before = t.loss_and_grads(x0, y0)
        params_before = t.state_dict()
        loss, count = t.evaluate(xs, ys)
        logits = t.logits(xs, ys)
        grads_after, params_after = t._tensors("rs_train_get_grads"), t.state_dict()
    finally:
        t.close()
    print(f"{kind} evaluate: count {count} float64 {want_count} of 16; loss device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert count == want_count
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(f"{kind} evaluate logits", logits.numpy(), lg64, logits_bar)])
    assert any(bool(g.any()) for g in grads_before.values())
    assert T.same_tensors(grads_before, grads_after), "evaluate moved the gradients"
    assert T.same_tensors(params_before, params_after), "evaluate moved the parameters"


@pytest.mark.gpu
@kinds
def test_tied_logits(kind):
    """both rows of the Linear equal: the two logits are the same bits, argmax takes the first, the loss is ln 2 (one rounding
    of a double to float: 1e-6 relative is generous) and db_fc = +-(n1 - n0) / (2 B)"""
    sd = T.make_state(kind, 11)
    sd["classifier.2.weight"] = np.repeat(sd["classifier.2.weight"][:1], 2, axis=0).copy()
    sd["classifier.2.bias"] = np.repeat(sd["classifier.2.bias"][:1], 2).copy()
    x, y = R.make_batch(3, 100, 111)
    B, n0, n1 = len(y), int((y == 0).sum()), int((y == 1).sum())
    assert n0 != n1
    bars = R.bars_of(sd, x, y)[0]
    t = T.trainer_of(kind, sd)
    try:
        loss, count, logits, grads = T.full_call(t, True, torch.from_numpy(x), torch.from_numpy(y))
        e_loss, e_count = t.evaluate(torch.from_numpy(x), torch.from_numpy(y))
    finally:
        t.close()
    assert torch.equal(logits[:, 0], logits[:, 1]) and bool(logits.abs().max() > 0)
    assert count == n0 and e_count == n0
    print(f"{kind} tied: loss device {loss!r} ln 2 {math.log(2.0)!r} bar 1.000e-06")
    assert abs(loss - math.log(2.0)) <= 1e-6 * math.log(2.0) and e_loss == loss
    want = np.array([n1 - n0, n0 - n1], np.float64) / (2 * B)
    assert_all([check(f"{kind} tied classifier.2.bias", grads["classifier.2.bias"].numpy(), want, bars["classifier.2.bias"])])


@pytest.mark.gpu
@kinds
def test_saturated_logits(kind):
    """the Linear's weights times 1e4: logits in the thousands, where log(sum(exp)) written naively is inf"""
    sd = T.make_state(kind, 11)
    sd["classifier.2.weight"] = sd["classifier.2.weight"] * np.float32(1e4)
    x, y = R.make_batch(3, 100, 111)
    bars, _, loss_bar, logits_bar, (l64, g64, _, lg64) = R.bars_of(sd, x, y)
    assert np.abs(lg64).max() > 1000 and l64 > 100           # a read is wrong by thousands: exp() of it overflows a double
    with np.errstate(over="ignore", divide="ignore"):
        assert np.isinf(np.log(np.exp(lg64).sum(1))).any()
    t = T.trainer_of(kind, sd)
    try:
        loss, _, logits, grads = T.full_call(t, True, torch.from_numpy(x), torch.from_numpy(y))
    finally:
        t.close()
    print(f"{kind} saturated: loss device {loss!r} float64 {l64!r} bar {loss_bar:.3e}")
    assert np.isfinite(loss) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(f"{kind} saturated logits", logits.numpy(), lg64, logits_bar)] +
               [check(f"{kind} saturated {k}", grads[k].numpy(), g64[k], bars[k]) for k in g64])


@pytest.mark.gpu
@kinds
def test_the_label_check(kind):
    from riser_amd._native import NativeError
    sd = T.make_state(kind, 11)
    x, y = T.batch_of(3, 100, 801)
    t, fresh = T.trainer_of(kind, sd), T.trainer_of(kind, sd)
    try:
        for bad in (torch.tensor([0, 2, 1]), torch.tensor([1, 0, -1])):
            for call in (t.loss_and_grads, t.evaluate, t.step):
                with pytest.raises(NativeError, match="a label outside"):
                    call(x, bad)
        for bad in (y.float(), y.bool(), torch.tensor([0, 1]), torch.tensor([0, 1, 0, 1])):
            for call in (t.loss_and_grads, t.evaluate, t.step):
                with pytest.raises(ValueError, match="one label per read"):
                    call(x, bad)
        assert T.same_tensors(t.state_dict(), {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}), \
            "a refused step moved the parameters"
        # the moments and the step count did not move either: the next good step is a fresh handle's first
        assert t.step(x, y) == fresh.step(x, y)
        moved, want = t.state_dict(), fresh.state_dict()
    finally:
        t.close()
        fresh.close()
    assert T.same_tensors(moved, want)
    assert any(not np.array_equal(moved[k].numpy(), sd[k]) for k in moved)


def adam_run(kind, sd, x, y, steps, change_lr):
    """`steps` of (state_dict, loss_and_grads, step) on one batch -> (p_0, [g_t], {t: parameters after step t})"""
    t = T.trainer_of(kind, sd, lr=T.lr_of(1))
    grads, after = [], {}
    try:
        p0 = numpy_of(t.state_dict())
        for step in range(1, steps + 1):
            if change_lr:
                t.learning_rate = T.lr_of(step)
            grads.append(numpy_of(t.loss_and_grads(x, y)[1]))
            t.step(x, y)
            after[step] = numpy_of(t.state_dict())
    finally:
        t.close()
    return p0, grads, after


@pytest.mark.gpu
@kinds
def test_adam_on_its_own(kind):
    """40 steps on one batch, the learning rate 1e-3 up to step 20 and 3e-3 from step 21.  The reference is torch.optim.Adam on
    the CPU fed the DEVICE's own gradient of every step, so that only the optimiser is measured: after steps 1, 2, 20, 21 and
    40 every tensor within four times the gap of torch's float32 run against its float64 run (floor 1e-6).  The first steps
    see the bias corrections at full size (1 - beta2 = 1e-3), step 21 the changed rate."""
    sd = T.make_state(kind, 11)
    x, y = T.batch_of(3, 100, 111)
    p0, grads, after = adam_run(kind, sd, x, y, T.ADAM_STEPS, True)
    assert all(np.array_equal(p0[k], sd[k]) for k in sd)
    p64, p32 = T.torch_adam_on(p0, grads, torch.float64), T.torch_adam_on(p0, grads, torch.float32)
    bars = T.adam_bars(p32, p64)
    assert_all([check(f"{kind} adam step {t} {k}", after[t][k], p64[t][k], bars[t][k]) for t in T.ADAM_CHECKED for k in p0])
    for k in p0:                                            # an element that never saw a gradient never moves
        never = np.all([g[k] == 0 for g in grads], axis=0)
        assert np.array_equal(after[T.ADAM_STEPS][k][never], p0[k][never]), k
        assert (after[T.ADAM_STEPS][k][~never] != p0[k][~never]).any() or never.all(), k


@pytest.mark.gpu
@kinds
def test_adam_leaves_dead_units_where_they_are(kind):
    """bias -50: no unit alive, every gradient but db_fc exactly zero for five steps - those elements keep their bits"""
    sd = T.make_state(kind, 11, bias=-50.0)
    x, y = T.batch_of(3, 100, 111)
    p0, grads, after = adam_run(kind, sd, x, y, 5, False)
    for k in p0:
        if k != "classifier.2.bias":
            assert not any(g[k].any() for g in grads), k
            assert np.array_equal(after[5][k], p0[k]), k
    assert all(g["classifier.2.bias"].all() for g in grads)
    assert (after[5]["classifier.2.bias"] != p0["classifier.2.bias"]).all()
