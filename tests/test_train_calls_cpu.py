"""The call surface of the training family without a GPU: that the Adam bars of test_gpu_train_calls.py would catch the
optimiser's classic defects, that rs_train_max_batch promises no batch a launch of csrc/train.hip cannot express, and that the
Python layer refuses a bad label tensor before it touches a device."""
import numpy as np
import pytest
import torch

import train_calls_ref as T
import train_ref as R

kinds = pytest.mark.parametrize("kind", T.KINDS)


@pytest.fixture(scope="module")
def lib():
    from riser_amd import _native as nv
    from riser_amd import build
    build.build()
    return nv.lib()


@kinds
def test_planted_adam_defects_miss_by_more_than_ten_bars(kind):
    """a float64 numpy Adam fed torch's float64 gradients along its own trajectory on the (3, 100) case, 40 steps with the
    learning rate changed behind step 20.  Written correctly it sits on torch's float64 Adam; with each defect planted it
    misses the bars the device is held to (four times torch's float32 gap, floor 1e-6) by more than ten times at one of the
    checked steps 1, 2, 20, 21, 40 - the steps were chosen for that: the bias corrections are largest at steps 1 and 2, a stuck
    step count and swapped betas show from step 2, the ignored rate change at step 21."""
    sd = T.make_state(kind, 11)
    x, y = R.make_batch(3, 100, 111)
    grads, cur = [], dict(sd)
    for t in range(1, T.ADAM_STEPS + 1):
        grads.append(R.torch_loss_and_grads(cur, x, y)[1])
        cur = {k: v.astype(np.float32) for k, v in T.numpy_adam_on(sd, grads, checked=(t,))[t].items()}
    p64, p32 = T.torch_adam_on(sd, grads, torch.float64), T.torch_adam_on(sd, grads, torch.float32)
    bars = T.adam_bars(p32, p64)
    assert sorted(bars) == list(T.ADAM_CHECKED)

    def worst(got):
        return {t: max(R.gap_of(got[t][k], p64[t][k]) / bars[t][k] for k in p64[t]) for t in T.ADAM_CHECKED}

    good = worst(T.numpy_adam_on(sd, grads))
    assert max(good.values()) < 1e-3, good                   # two float64 runs of one formula
    first_seen = {"no_first_correction": 1, "no_second_correction": 1, "eps_inside_sqrt": 1, "betas_swapped": 2,
                  "step_stuck_at_1": 2, "lr_change_ignored": 21}
    for defect in T.ADAM_DEFECTS:
        miss = worst(T.numpy_adam_on(sd, grads, defect=defect))
        print(f"{kind} {defect}: " + ", ".join(f"step {t} {m:.1e} bars" for t, m in miss.items()))
        assert miss[first_seen[defect]] > 10, (defect, miss)
        assert all(m < 1e-3 for t, m in miss.items() if t < first_seen[defect]), (defect, miss)      # and not before


@kinds
def test_max_batch_promises_only_what_the_launches_take(lib, kind):
    """every launch of a training call at B = rs_train_max_batch(L): a grid's x extent holds 2^31 - 1 blocks, y and z 65535.
    train_head_bwd_kernel has the reads in y, train_wgrad_kernel the slices: both are capped (csrc/train/plan.hpp kMaxGridY).
    A length below the net's minimum promises no batch at all."""
    h = T.raw_handle(kind, T.make_state(kind, 1), -1)
    try:
        for L in (8, 16, 64, 100, 16000):
            mb = lib.rs_train_max_batch(h, L)
            if L < T.min_length(kind):
                assert mb == 0 and lib.rs_train_workspace_bytes(h, 1, L) == 0, L
                continue
            assert 1 <= mb <= T.GRID_YZ, (L, mb)
            assert lib.rs_train_workspace_bytes(h, mb, L) > 0, (L, mb)
            assert mb * L <= 2 ** 31 - 1                     # positions are counted in int
            plans = [T.slice_plan_of(lib, h, j, mb, L) for j in range(len(T.conv_shapes(kind)))]
            for j, ((n, s), (level, _, _, _)) in enumerate(zip(plans, T.conv_shapes(kind))):
                positions = mb * (L >> level)
                assert s % 4 == 0 and (n - 1) * s < positions <= n * s, (L, j, n, s)
            for name, (gx, gy, gz) in T.launch_grids(kind, mb, L, lambda j: plans[j][0]):
                assert 1 <= gx <= T.GRID_X and 1 <= gy <= T.GRID_YZ and 1 <= gz <= T.GRID_YZ, (L, mb, name, (gx, gy, gz))
        if kind == "shipped":                                # the shipped class's own numbers are what they were
            assert T.slice_plan_of(lib, h, 0, 3, 100) == R.slice_plan(3, 100, 0, 1, 3, 3)
    finally:
        lib.rs_train_destroy(h)


def test_slice_count_is_capped_only_where_a_grid_could_not_hold_it(lib):
    """the cap moves no plan a launch could express before it: below 65535 slices the plan is the uncapped arithmetic"""
    h = T.raw_handle("shipped", T.make_state("shipped", 1), -1)
    try:
        for B, L in ((3, 100), (32, 16000), (512, 16000)):
            for j, (level, c_in, c_out, k) in enumerate(T.conv_shapes("shipped")):
                positions = B * (L >> level)
                cap = max(1, (32 << 20) // ((c_out * c_in * k + c_out) * 4))
                n = max(1, min(-(-positions // 256), cap))
                assert n <= T.GRID_YZ
                s = -(-(-(-positions // n)) // 4) * 4
                assert T.slice_plan_of(lib, h, j, B, L) == (max(1, -(-positions // s)), s), (B, L, j)
        mb = lib.rs_train_max_batch(h, 16000)
        n, s = T.slice_plan_of(lib, h, 0, mb, 16000)
        assert -(-mb * 16000 // 256) > T.GRID_YZ and n <= T.GRID_YZ and s > 256      # the case the cap is for
    finally:
        lib.rs_train_destroy(h)


@kinds
def test_label_tensors_are_refused_before_any_gpu_call(lib, kind):
    """a float, a bool or a wrong-sized label tensor is a ValueError from a trainer whose handle has no device, on a machine
    that may have none: nothing was moved to a device and no launch was asked for"""
    from riser_amd.train import GenericTrainer, Trainer
    cls = Trainer if kind == "shipped" else GenericTrainer
    t = object.__new__(cls)
    t._h, t._ws, t.device = T.raw_handle(kind, T.make_state(kind, 1), -1), None, torch.device("cuda", 0)
    try:
        x, y = T.batch_of(3, 100, 5)
        for bad in (y.float(), y.bool(), torch.tensor([0, 1]), torch.tensor([[0, 1, 0]])):
            for call in (t.step, t.loss_and_grads, t.evaluate):
                with pytest.raises(ValueError, match="one label per read"):
                    call(x, bad)
        with pytest.raises(ValueError, match="float32 tensor"):
            t.step(x.double(), y)
    finally:
        t.close()
