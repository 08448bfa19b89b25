"""Train the TCN on the GPU (riser/nets/tcn.py as riser/train.py builds it, `model: tcn`): forward, cross-entropy, backward,
weight norm and Adam are the HIP kernels of csrc/tcn_train.hip (rs_tcn_train_*), and they run on the receptive cone of each
read's last sample alone - the logits are linear(x[:, :, -1]) and every conv is causal, so nothing else carries a gradient.
fp32, two classes, one input channel, one read length per batch.

    python -m riser_amd.tcn_train EXP_DIR DATA_DIR CHECKPT|None CONFIG.yaml START_EPOCH

is riser_amd.train's command line and loop (`fit`) on a TcnTrainer; its checkpoints are state dicts `riser_amd.Model` and the
reference both load.  The parameters are weight norm's (weight_g, weight_v) and the biases; a shortcut the reference builds but
never applies (a block whose input already has n_filters channels) stays on the host and comes back with the bits it came in
with.  Dropout cannot follow torch's random stream: the mask is the counter-based hash include/riser_amd.h states, keyed on
(seed, step, conv, read, distance from the read's end, channel).
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np
import torch

from . import _native as nv
from ._family import load_state
from .train import ADAM

WHAT = {"a1": 0, "a2": 1, "out": 2, "da1": 3, "dout": 4}
_SPELLINGS = (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1"))


class _Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "n_filters", "kernel", "dilation", "in_channels", "n_classes", "dtype",
                                         "bottleneck")] + [("dropout", C.c_double), ("seed", C.c_uint64)]


def check_tcn_config(config) -> dict:
    """dict(n_layers, n_filters, kernel, dilation, dropout) of a config TcnTrainer trains; ValueError - before any GPU call -
    for tcn-bot and every other model, every dtype but fp32, n_classes != 2, kernel < 2, in_channels != 1, dropout outside
    [0, 1)"""
    model = getattr(config, "model", "tcn")
    if model != "tcn":
        raise ValueError(f"model {model!r}: riser_amd.tcn_train trains the `tcn` model only")
    dtype = getattr(config, "dtype", "f32")
    if dtype not in ("f32", "fp32", "float32"):
        raise ValueError(f"dtype {dtype!r}: riser_amd.tcn_train is fp32 only")
    c = config.tcn
    net = dict(n_layers=int(c.n_layers), n_filters=int(c.n_filters), kernel=int(c.kernel), dilation=int(c.dilation),
               dropout=float(getattr(c, "dropout", 0.0)))
    if int(c.n_classes) != 2:
        raise ValueError("riser_amd.tcn_train trains two-class heads only")
    if net["kernel"] < 2:
        raise ValueError(f"kernel {net['kernel']}: the reference's Chomp1d(0) empties the tensor (riser/nets/tcn.py:15); kernel >= 2")
    if int(getattr(c, "in_channels", 1)) != 1:
        raise ValueError(f"in_channels {c.in_channels}: the reference feeds one signal channel (tcn.py:85 unsqueeze(1))")
    if not 0.0 <= net["dropout"] < 1.0:
        raise ValueError(f"dropout {net['dropout']}: outside [0, 1)")
    if net["n_layers"] < 1 or net["n_filters"] < 1 or net["dilation"] < 1:
        raise ValueError(f"n_layers {net['n_layers']} / n_filters {net['n_filters']} / dilation {net['dilation']}: all >= 1")
    return net


def _blocks(net):
    """(key prefix, c_in, shortcut applied) per block"""
    for i in range(net["n_layers"]):
        c_in = 1 if i == 0 else net["n_filters"]
        yield f"layers.{i}", c_in, c_in != net["n_filters"]


def param_shapes(net) -> dict:
    """every key of the reference's state dict in its order - the shortcuts it builds but never applies included"""
    F, k, shapes = net["n_filters"], net["kernel"], {}
    for pre, c_in, _ in _blocks(net):
        for j, ci in ((0, c_in), (1, F)):
            p = f"{pre}.blocks.{j}.0"
            shapes[p + ".bias"], shapes[p + ".weight_g"], shapes[p + ".weight_v"] = (F,), (F, 1, 1), (F, ci, k)
        shapes[pre + ".shortcut.weight"], shapes[pre + ".shortcut.bias"] = (F, c_in, 1), (F,)
    shapes["linear.weight"], shapes["linear.bias"] = (2, F), (2,)
    return shapes


def device_keys(net) -> list:
    """the keys that live on the device, in the order of rs_tcn_train_get_params' tensor index and of the flat Adam vector"""
    keys = []
    for pre, _, applied in _blocks(net):
        for j in (0, 1):
            keys += [f"{pre}.blocks.{j}.0.weight_g", f"{pre}.blocks.{j}.0.weight_v", f"{pre}.blocks.{j}.0.bias"]
        if applied:
            keys += [pre + ".shortcut.weight", pre + ".shortcut.bias"]
    return keys + ["linear.weight", "linear.bias"]


def init_state(net) -> dict:
    """torch's own initialisation on the CPU in the reference's construction order (tcn.py:27-36,69-82): per block the two
    weight-normed convs, the shortcut, then _init_weights - which reaches the shortcut's weight, N(0, 0.01), but of a
    weight-normed conv only the derived `weight`, so v keeps torch's default and g = ||v|| (its draws are made all the same:
    they move the random stream) - and the Linear last"""
    from torch.nn.utils import weight_norm
    F, k, sd = net["n_filters"], net["kernel"], {}
    for pre, c_in, _ in _blocks(net):
        convs = [weight_norm(torch.nn.Conv1d(ci, F, k)) for ci in (c_in, F)]
        shortcut = torch.nn.Conv1d(c_in, F, 1)
        with torch.no_grad():
            for m in convs + [shortcut]:
                torch.nn.init.normal_(m.weight, mean=0, std=0.01)
        for j, m in enumerate(convs):
            p = f"{pre}.blocks.{j}.0"
            sd[p + ".bias"], sd[p + ".weight_g"], sd[p + ".weight_v"] = m.bias.detach(), m.weight_g.detach(), m.weight_v.detach()
        sd[pre + ".shortcut.weight"], sd[pre + ".shortcut.bias"] = shortcut.weight.detach(), shortcut.bias.detach()
    fc = torch.nn.Linear(F, 2)
    sd["linear.weight"], sd["linear.bias"] = fc.weight.detach(), fc.bias.detach()
    return sd


def _checked_state(state, shapes) -> dict:
    """{reference key: contiguous float32 array} of both weight-norm spellings, under the weight_g / weight_v names"""
    sd = load_state(state)
    out = {}
    for key, shape in shapes.items():
        names = [key]
        for g, v in _SPELLINGS[1:]:
            if key.endswith(".weight_g"):
                names.append(key[:-len("weight_g")] + g)
            elif key.endswith(".weight_v"):
                names.append(key[:-len("weight_v")] + v)
        found = [n for n in names if n in sd]
        if not found:
            raise ValueError(f"state dict has no {key!r}")
        a = np.ascontiguousarray(sd[found[0]], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{key}: shape {a.shape}, expected {shape}")
        out[key] = a
    return out


def create_handle(net, state, device_index: int, seed: int = 0, dtype: int = nv.RS_F32, bottleneck: bool = False,
                  in_channels: int = 1, n_classes: int = 2):
    """a C handle on the arrays of `state` ({reference key: float32 array}).  device_index < 0: a handle without device
    memory, which answers the plans and the argument checks on a machine without a GPU"""
    cfg = _Config(net["n_layers"], net["n_filters"], net["kernel"], net["dilation"], in_channels, n_classes, dtype,
                  int(bottleneck), net["dropout"], int(seed) & (2 ** 64 - 1))
    keys = device_keys(net)
    ptrs = (C.c_void_p * len(keys))(*[state[k].ctypes.data for k in keys])
    h = C.c_void_p()
    nv.check(nv.lib().rs_tcn_train_create(C.byref(cfg), ptrs, len(keys), int(device_index), C.byref(h)), "rs_tcn_train_create")
    return h


class TcnTrainer:
    """The TCN's parameters (g, v, b of every conv, an applied shortcut, the Linear), their gradients and the Adam moments on
    the device (rs_tcn_train_*).  x: float32 [B, L] on the device or the host, y: any integer tensor of B labels in {0, 1}.  A
    batch beyond max_batch(L) is refused, not split: a split would change the mean."""

    def __init__(self, config, state_dict=None, device=None, seed: int = 0):
        self._h = None
        self._ws = None
        self.net = check_tcn_config(config)
        self.learning_rate = float(getattr(config, "learning_rate", 1e-3))
        self.seed = int(seed)
        self._shapes = param_shapes(self.net)
        self._keys = device_keys(self.net)
        self._host = _checked_state(state_dict if state_dict is not None else init_state(self.net), self._shapes)
        nv.require_gpu()
        d = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        self._h = create_handle(self.net, self._host, self.device.index, self.seed)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        self._ws = None
        if h:
            nv.lib().rs_tcn_train_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_batch(self, L: int) -> int:
        return int(nv.lib().rs_tcn_train_max_batch(self._h, int(L)))

    def slice_plan(self, block: int, which: int, B: int, L: int):
        """(slices, positions per slice, rows per read) of the weight-gradient contraction of conv1 (which 0), conv2 (1) or the
        applied shortcut (2) of `block` (rs_tcn_train_slice_plan)"""
        n, s, r = C.c_int32(), C.c_int32(), C.c_int32()
        nv.check(nv.lib().rs_tcn_train_slice_plan(self._h, int(block), int(which), int(B), int(L), C.byref(n), C.byref(s),
                                                  C.byref(r)), "rs_tcn_train_slice_plan")
        return int(n.value), int(s.value), int(r.value)

    def set_dropout(self, p: float, seed: int = None, counter: int = 0):
        """dropout probability, seed and step counter of the mask (rs_tcn_train_set_dropout)"""
        self.seed = self.seed if seed is None else int(seed)
        nv.check(nv.lib().rs_tcn_train_set_dropout(self._h, float(p), self.seed & (2 ** 64 - 1), int(counter)),
                 "rs_tcn_train_set_dropout")
        self.net["dropout"] = float(p)

    def _call(self, fn_name: str, x, y):
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("x must be a float32 tensor [B, L]")
        y = torch.as_tensor(y)
        if y.is_floating_point() or y.dtype == torch.bool or y.dim() != 1 or y.shape[0] != x.shape[0]:
            raise ValueError("y must be an integer tensor of one label per read")
        B, L = x.shape
        mb = self.max_batch(L)
        if mb and B > mb:
            raise ValueError(f"{B} reads of {L} samples outgrow the 2 GiB buffer window (max_batch {mb}): a split would change "
                             "the mean, so the batch is refused")
        x = x.to(self.device).contiguous()
        y = y.to(self.device, dtype=torch.int32).contiguous()
        lib = nv.lib()
        need = lib.rs_tcn_train_workspace_bytes(self._h, B, L)
        if self._ws is None or self._ws.numel() < max(need, 256):
            self._ws = None
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        out = torch.empty(2 + 2 * B, dtype=torch.float32, device=self.device)
        nv.check(getattr(lib, fn_name)(self._h, x.data_ptr(), y.data_ptr(), B, L, L, self._ws.data_ptr(), self._ws.numel(),
                                       out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), fn_name)
        host = out.cpu()
        return float(host[0]), int(host[1]), host[2:].reshape(B, 2)

    def _adam(self):
        nv.check(nv.lib().rs_tcn_train_adam_step(self._h, self.learning_rate, ADAM["beta1"], ADAM["beta2"], ADAM["eps"],
                                                 torch.cuda.current_stream(self.device).cuda_stream), "rs_tcn_train_adam_step")

    def step(self, x, y) -> float:
        """forward, backward, Adam, fold; the loss of the batch before the update"""
        loss = self._call("rs_tcn_train_forward_backward", x, y)[0]
        self._adam()
        return loss

    def loss_and_grads(self, x, y):
        """(loss, {reference key: gradient}) - no update; an unapplied shortcut has no entry"""
        loss = self._call("rs_tcn_train_forward_backward", x, y)[0]
        return loss, self._tensors("rs_tcn_train_get_grads")

    def evaluate(self, x, y):
        """(loss, reads classified correctly) of the forward pass alone, in eval mode: no dropout"""
        loss, n_correct, _ = self._call("rs_tcn_train_evaluate", x, y)
        return loss, n_correct

    def logits(self, x, y):
        """the [B, 2] logits of the forward pass alone (eval mode), on the host"""
        return self._call("rs_tcn_train_evaluate", x, y)[2]

    def _tensors(self, fn_name: str) -> dict:
        out = {}
        for i, key in enumerate(self._keys):
            a = np.empty(self._shapes[key], np.float32)
            nv.check(getattr(nv.lib(), fn_name)(self._h, i, a.ctypes.data, a.size), fn_name)
            out[key] = torch.from_numpy(a)
        return out

    def state_dict(self) -> dict:
        """the reference's keys in its order as CPU fp32 tensors, weight norm spelled weight_g / weight_v; the unapplied
        shortcuts are the host's untouched copies"""
        dev = self._tensors("rs_tcn_train_get_params")
        return {k: dev[k] if k in dev else torch.from_numpy(self._host[k].copy()) for k in self._shapes}

    def load_state_dict(self, state):
        sd = _checked_state(state, self._shapes)
        for i, key in enumerate(self._keys):
            nv.check(nv.lib().rs_tcn_train_set_params(self._h, i, sd[key].ctypes.data, sd[key].size), "rs_tcn_train_set_params")
        self._host = sd

    def debug_copy(self, block: int, what: str, B: int, L: int) -> torch.Tensor:
        """block `block`'s 'a1', 'a2', 'out' or the raw gradient arriving at a1 ('da1') or at out ('dout') of the last forward
        + backward of B reads of L samples, on the host: [B, rows, n_filters], row m of a1 at position L-1 - d m, of the
        others at L-1 - d base m (rs_tcn_train_debug_copy)"""
        rows = self.slice_plan(block, 0 if what in ("a1", "da1") else 1, B, L)[2]
        F = self.net["n_filters"]
        dst = torch.empty((B, rows, (F + 3) & ~3), dtype=torch.float32, device=self.device)
        nv.check(nv.lib().rs_tcn_train_debug_copy(self._h, block, WHAT[what], dst.data_ptr(), dst.numel() * 4),
                 "rs_tcn_train_debug_copy")
        return dst[:, :, :F].cpu()


def main(argv=None) -> int:
    import os

    from .modeldir import get_config
    from .train import LENGTH_KEYS, fit, load_set, parse_args
    a = parse_args(argv)
    print(f"Experiment dir: {a.exp_dir}\nData dir: {a.data_dir}\nCheckpoint: {a.checkpt}\nConfig file: {a.config_file}")
    config = get_config(a.config_file)
    check_tcn_config(config)
    print("Creating data loaders...")
    sets = {split: {k: load_set(os.path.join(a.data_dir, k, split)) for k in LENGTH_KEYS} for split in ("train", "val")}
    state = os.path.join(a.exp_dir, a.checkpt) if a.checkpt is not None else None
    trainer = TcnTrainer(config, state)
    try:
        fit(trainer, sets["train"], sets["val"], int(config.n_epochs), int(config.batch_size), a.exp_dir, a.exp_id, a.start_epoch)
    finally:
        trainer.close()
    print("Training complete.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
