"""Helpers of the call-surface tests of the training family (test_gpu_train_calls.py, test_train_calls_cpu.py): the two small
nets the suite already trains - the shipped class, which riser_amd.train.trainer_for gives a `Trainer`, and
train_ref.CASES["depth2"], which it gives a `GenericTrainer` - and Adam on given gradients.  No reference of the net lives
here: float64 comes from train_ref, the trainers from train_device.
"""
import ctypes as C

import numpy as np
import torch

import train_device as D
import train_ref as R

KINDS = ("shipped", "generic")
NETS = {"shipped": ([3, 7, 18, 37], [3, 3, 3, 3], 1), "generic": R.CASES["depth2"][:3]}     # (channels, kernels, depth)
ADAM_STEPS, ADAM_LR_CHANGE, ADAM_LRS = 40, 20, (1e-3, 3e-3)        # steps 1-20 at the first rate, 21-40 at the second
ADAM_CHECKED = (1, 2, 20, 21, 40)
ADAM_DEFECTS = ("no_first_correction", "no_second_correction", "eps_inside_sqrt", "betas_swapped", "step_stuck_at_1",
                "lr_change_ignored")


def min_length(kind):
    """the shortest read the net takes: one row behind its last pool"""
    return 1 << len(NETS[kind][0])


def make_state(kind, seed, bias=None):
    return R.make_state(*NETS[kind], seed, bias)


def trainer_of(kind, sd, lr=1e-3):
    return D.trainer_of(NETS[kind], sd, lr)


def raw_handle(kind, sd, device_index):
    """the C handle of the net's own constructor; device_index < 0: without device memory"""
    from riser_amd.train import create_handle
    channels, kernels, depth = NETS[kind]
    return create_handle(channels, {k: np.ascontiguousarray(v, np.float32) for k, v in sd.items()}, device_index, kernels, depth)


def conv_shapes(kind):
    """[(level, c_in, c_out, k)] per conv, j = layer * depth + d"""
    return list(R.convs_of(*NETS[kind]))


def batch_of(B, L, seed):
    x, y = R.make_batch(B, L, seed)
    return torch.from_numpy(x), torch.from_numpy(y)


def full_call(t, backward, x, y):
    """everything one training call returns: (loss, count, logits [B, 2], {key: gradient} as the handle holds them now)"""
    loss, count, logits = t._call("rs_train_forward_backward" if backward else "rs_train_evaluate", x, y)
    return loss, count, logits, t._tensors("rs_train_get_grads")


def same_bits(a, b):
    """two results of full_call: the loss and count equal, the logits and every gradient torch.equal"""
    return (a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and list(a[3]) == list(b[3])
            and all(torch.equal(a[3][k], b[3][k]) for k in a[3]))


def same_tensors(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- Adam on given gradients ------------------------------------------------------------------------------------------------

def lr_of(step):
    """the learning rate of step 1 .. ADAM_STEPS"""
    return ADAM_LRS[0] if step <= ADAM_LR_CHANGE else ADAM_LRS[1]


def torch_adam_on(p0, grads, dtype, checked=ADAM_CHECKED):
    """torch.optim.Adam on the CPU from the parameters `p0`, its .grad assigned grads[t - 1] at step t, the learning rate
    changed where lr_of changes it -> {step: {key: float64 parameters}} for the checked steps"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in p0.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr_of(1))
    out = {}
    for t, g in enumerate(grads, 1):
        for group in opt.param_groups:
            group["lr"] = lr_of(t)
        for k in p:
            p[k].grad = torch.tensor(np.asarray(g[k]), dtype=dtype)
        opt.step()
        if t in checked:
            out[t] = {k: v.detach().double().numpy().copy() for k, v in p.items()}
    return out


def numpy_adam_on(p0, grads, defect=None, checked=ADAM_CHECKED, beta1=0.9, beta2=0.999, eps=1e-8):
    """the same in float64 numpy, torch.optim.Adam's formula written out; `defect`: one of ADAM_DEFECTS planted on purpose"""
    if defect == "betas_swapped":
        beta1, beta2 = beta2, beta1
    p = {k: np.asarray(v, np.float64).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v2 = {k: np.zeros_like(v) for k, v in p.items()}
    out = {}
    for t, g in enumerate(grads, 1):
        lr = ADAM_LRS[0] if defect == "lr_change_ignored" else lr_of(t)
        n = 1 if defect == "step_stuck_at_1" else t
        bc1 = 1.0 if defect == "no_first_correction" else 1.0 - beta1 ** n
        bc2 = 1.0 if defect == "no_second_correction" else 1.0 - beta2 ** n
        for k in p:
            gk = np.asarray(g[k], np.float64)
            m[k] = beta1 * m[k] + (1.0 - beta1) * gk
            v2[k] = beta2 * v2[k] + (1.0 - beta2) * gk * gk
            denom = np.sqrt(v2[k] / bc2 + eps) if defect == "eps_inside_sqrt" else np.sqrt(v2[k]) / np.sqrt(bc2) + eps
            p[k] = p[k] - (lr / bc1) * (m[k] / denom)
        if t in checked:
            out[t] = {k: a.copy() for k, a in p.items()}
    return out


def adam_bars(p32, p64, floor=1e-6):
    """{step: {key: bar}}: four times the gap of torch's float32 Adam against its float64 Adam on the same gradients, at least
    `floor` - the convention of test_five_adam_steps_against_torch_float64, never taken from the device"""
    return {t: {k: max(4 * R.gap_of(p32[t][k], p64[t][k]), floor) for k in p64[t]} for t in p64}


# ---- what the launches of one training call can express (csrc/train.hip, run()) ---------------------------------------------

GRID_X, GRID_YZ = 2 ** 31 - 1, 65535


def launch_grids(kind, B, L, slices_of):
    """[(kernel, (x, y, z))] of every launch rs_train_forward_backward makes for B reads of L samples, read off run() and the
    launchers above it; slices_of(j) is conv j's slice count (rs_train_slice_plan)"""
    channels, _, _ = NETS[kind]
    shapes = conv_shapes(kind)
    p16 = lambda c: (c + 15) & ~15
    wc = lambda nc: 1 if nc <= 16 else 2 if nc <= 32 else 4
    grids = []
    for j, (level, c_in, c_out, k) in enumerate(shapes):
        T = L >> level
        tiles = (T + 127) // 128
        grids.append((f"conv {j} forward", (B * tiles, -(-p16(c_out) // (16 * wc(c_out))), 1)))
        grids.append((f"conv {j} weight gradient", (((c_in + 31) // 32) * ((c_out + 31) // 32), slices_of(j), -(-k // 3))))
        grids.append((f"conv {j} reduce", (-(-(c_out * c_in * k + c_out) // 256), 1, 1)))
        if j:
            grids.append((f"conv {j} data gradient", (B * tiles, -(-p16(c_in) // (16 * wc(c_in))), 1)))
    T_last = L >> len(channels)
    grids.append(("head", (B, 1, 1)))
    grids.append(("loss", (1, 1, 1)))
    grids.append(("fc gradient", (-(-channels[-1] // 256), 1, 1)))
    grids.append(("head backward", (min(T_last, 64), B, 1)))
    return grids


def slice_plan_of(lib, h, j, B, L):
    n, s = C.c_int32(), C.c_int32()
    assert lib.rs_train_slice_plan(h, j, B, L, C.byref(n), C.byref(s)) == 0
    return int(n.value), int(s.value)
