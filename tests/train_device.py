"""What the training tests share around a trainer on the device (test_gpu_train.py, test_gpu_gtrain.py, train_calls_ref.py): the
config and the trainer of a net given as `shape` = (channels, kernels, depth) - the shipped class is ([..], [3] * n, 1) - one
forward + backward with the device's decisions copied out, and the comparison against train_ref's float64."""
import types

import numpy as np
import torch

import train_ref as R
from riser_amd import synth


def config_of(channels, kernels, depth=1, lr=1e-3):
    return types.SimpleNamespace(model="cnn", learning_rate=lr, cnn=synth.CnnConfig(channels=channels, kernels=kernels, depth=depth))


def trainer_of(shape, sd, lr=1e-3, cls=None):
    """the trainer riser_amd.train.trainer_for picks for the net - Trainer for the shipped class, GenericTrainer for every
    other - or a `cls` of the caller's; `shape` may be the name of one of train_ref.CASES"""
    from riser_amd.train import trainer_for
    shape = R.CASES[shape][:3] if isinstance(shape, str) else shape
    return (cls or trainer_for)(config_of(*shape, lr=lr), sd, device=torch.device("cuda", 0))


def run_device(shape, sd, x, y, debug=False):
    """-> loss, {key: grad as float64 numpy}, and with debug the device's per-conv (sel | None, gate, dy)"""
    t = trainer_of(shape, sd)
    try:
        loss, grads = t.loss_and_grads(torch.from_numpy(x), torch.from_numpy(y))
        grads = {k: v.numpy().astype(np.float64) for k, v in grads.items()}
        if not debug:
            return loss, grads
        B, L = x.shape
        pools = [p for _, p in R.conv_keys(sd)]
        sel = [t.debug_copy(j, "sel", B, L).numpy() if p else None for j, p in enumerate(pools)]
        gate = [t.debug_copy(j, "y", B, L).numpy() > 0 for j in range(len(pools))]
        dy = [t.debug_copy(j, "dy", B, L).numpy().astype(np.float64) for j in range(len(pools))]
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


def held_to_numpy_backward(shape, sd, x, y, label=""):
    """the backward kernels against the numpy backward fed the device's decisions, which equal float64's outside the fragile
    elements -> (device grads, numpy grads, bars).  `label` goes in front of every printed name."""
    bars, dbars, loss_bar, _, (l64, _, _, _) = R.bars_of(sd, x, y)
    fwd = R.forward64(sd, x)
    frag = R.fragile(fwd)
    loss, grads, sel, gate, dy = run_device(shape, sd, x, y, debug=True)
    for j in range(len(sel)):
        if sel[j] is not None:
            differs = (sel[j] != fwd["sel"][j]) & fwd["gate"][j] & gate[j]          # a selector matters where a gradient flows
            assert not (differs & ~frag[j]).any(), f"conv {j}: a selector differs from float64's outside the fragile elements"
        assert gate[j].shape == fwd["gate"][j].shape, j
        assert not ((gate[j] != fwd["gate"][j]) & ~frag[j]).any(), f"conv {j}: a gate differs outside the fragile elements"
    g_ref, dy_ref = R.backward64(sd, fwd, y, sels=sel, gates=gate)
    # the unlabelled line of the shipped tests never named its bar: the recorded outputs are compared as text
    print(f"{label}loss: device {loss!r} float64 {l64!r}" + (f" bar {loss_bar:.3e}" if label else ""))
    assert abs(loss - l64) <= loss_bar * abs(l64)
    assert_all([check(f"{label}{k}", grads[k], g_ref[k], bars[k]) for k in g_ref] +
               [check(f"{label}dY_{j}", dy[j], dy_ref[j], dbars[j]) for j in range(len(sel))])
    return grads, g_ref, bars
