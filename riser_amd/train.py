"""Train the ConvNet on the GPU (riser/train.py; riser/nets/cnn.py:12-18,43-65 with `gap_fc`, two classes): forward,
cross-entropy, backward and Adam are the HIP kernels of csrc/train.hip (rs_train_*).  A net is (channels, kernels, depth), read
from a config by `net_of`; `param_keys`, `param_shapes`, `init_state` and `create_handle` take it, the shipped class - depth 1,
every kernel 3 - being their default.  `Trainer` is the shipped class (`check_config`, rs_train_create), `GenericTrainer` the
same body for any `depth` and any odd `kernels` - every net riser_amd.gconv runs (`check_generic_config`,
rs_train_create_generic); `trainer_for` picks.

    python -m riser_amd.train EXP_DIR DATA_DIR CHECKPT|None CONFIG.yaml START_EPOCH

is the reference's command line.  DATA_DIR holds {2s,3s,4s}/{train,val}/{positive,negative}.pt as `python -m riser_amd.retrain
write-tensors` (riser/retrain/write_tensors.py) leaves them; EXP_DIR receives {exp_id}_{START_EPOCH}_best_model.pth on every
strictly better validation accuracy, {exp_id}_latest_model.pth every epoch - state dicts `riser_amd.Model` and the reference
both load - and metrics.tsv in place of TensorBoard.  fp32 only; the optimiser state is not saved (the reference does not
save it either: a resumed run starts a fresh Adam).
"""
from __future__ import annotations

import ctypes as C
import os
import random
import sys
import time

import numpy as np
import torch

from . import _native as nv
from ._family import load_state
from .gconv import _Conv

LENGTH_KEYS = ("2s", "3s", "4s")                   # riser/train.py:42,88
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)      # torch.optim.Adam's defaults (riser/train.py:198)
METRICS = ("epoch", "train_loss", "val_loss", "val_acc", "train_t", "val_t", "train - val loss")     # riser/train.py:226-231


def net_of(config):
    """(channels, kernels, depth) of a config - the one description of the net - behind the checks every trainer shares: the
    `cnn` model, fp32, the `gap_fc` head, two classes, lists as long as n_layers >= 1; ValueError for everything else"""
    model = getattr(config, "model", "cnn")
    if model != "cnn":
        raise ValueError(f"model {model!r}: riser_amd.train trains the `cnn` model only")
    dtype = getattr(config, "dtype", "f32")
    if dtype not in ("f32", "fp32", "float32"):
        raise ValueError(f"dtype {dtype!r}: riser_amd.train is fp32 only")
    cnn = config.cnn
    n_layers, depth = int(cnn.n_layers), int(getattr(cnn, "depth", 1))
    channels, kernels = [int(v) for v in cnn.channels], [int(v) for v in cnn.kernels]
    if n_layers < 1 or len(channels) < n_layers or len(kernels) < n_layers:
        raise ValueError(f"channels {channels} / kernels {kernels}: shorter than n_layers {n_layers} >= 1")
    classifier = getattr(cnn, "classifier", "gap_fc")
    if classifier != "gap_fc":
        raise ValueError(f"classifier {classifier!r}: riser_amd.train trains the `gap_fc` head only")
    if int(cnn.n_classes) != 2:
        raise ValueError("riser_amd.train trains two-class heads only")
    return channels[:n_layers], kernels[:n_layers], depth


def check_config(config) -> list:
    """the channel list of a config of the shipped class (depth 1, every kernel 3); ValueError - before any GPU call - for
    everything else"""
    channels, kernels, depth = net_of(config)
    if depth != 1:
        raise ValueError(f"depth {depth}: riser_amd.train.Trainer trains depth 1 only")
    if any(k != 3 for k in kernels):
        raise ValueError(f"kernels {kernels}: riser_amd.train.Trainer trains kernels of 3 only")
    return channels


def check_generic_config(config):
    """(channels, kernels, depth) of a config GenericTrainer trains - what the generic inference family (riser_amd.gconv)
    runs: 1-16 layers of depth 1-64, every kernel odd; ValueError - before any GPU call - for everything else, a conv that
    fits no tile shape of that family included"""
    from .gconv import layer_plan
    channels, kernels, depth = net_of(config)
    if len(channels) > 16 or depth < 1 or depth > 64:
        raise ValueError(f"n_layers {len(channels)} / depth {depth}: riser_amd.train trains 1-16 layers of depth 1-64")
    if any(k < 1 or k % 2 == 0 for k in kernels):
        raise ValueError(f"kernels {kernels}: even conv kernels ('same' pads them asymmetrically) are not supported")
    if any(c < 1 for c in channels):
        raise ValueError(f"channels {channels}: every layer needs at least one")
    for _, c_in, c, k in _convs(channels, kernels, depth):
        try:
            layer_plan(c_in, c, k)
        except nv.NativeError as e:
            raise ValueError(f"conv {c_in} -> {c}, kernel {k}: the generic ConvNet family could not run it ({e})") from None
    return channels, kernels, depth


def is_shipped_class(config) -> bool:
    """True: check_config takes the config (Trainer's class); False: check_generic_config does; ValueError: neither"""
    try:
        check_config(config)
        return True
    except ValueError:
        check_generic_config(config)
        return False


def _convs(channels, kernels=None, depth=1):
    """(state-dict key prefix, c_in, c_out, k) of every conv in launch order, j = layer * depth + d: layers.{layer}.{2 d}
    (nn.Sequential of conv, ReLU, conv, ReLU, ..., MaxPool1d: riser/nets/cnn.py:52-65).  kernels None: every kernel 3."""
    c_in = 1
    for i, c in enumerate(channels):
        for d in range(depth):
            yield f"layers.{i}.{2 * d}", c_in, c, 3 if kernels is None else kernels[i]
            c_in = c


def param_keys(n_layers: int, depth: int = 1) -> list:
    """the reference's state-dict keys in the order of rs_train_get_params' tensor index"""
    return list(param_shapes([1] * n_layers, None, depth))


def param_shapes(channels, kernels=None, depth=1) -> dict:
    shapes = {}
    for key, c_in, c, k in _convs(channels, kernels, depth):
        shapes[key + ".weight"], shapes[key + ".bias"] = (c, c_in, k), (c,)
    shapes["classifier.2.weight"], shapes["classifier.2.bias"] = (2, channels[-1]), (2,)
    return shapes


def init_state(channels, kernels=None, depth=1) -> dict:
    """torch's own initialisation of nn.Conv1d / nn.Linear tensors of the net's shapes, on the CPU, in the reference's
    construction order: conv by conv as they launch, then the head"""
    sd = {}
    for key, c_in, c, k in _convs(channels, kernels, depth):
        conv = torch.nn.Conv1d(c_in, c, k)
        sd[key + ".weight"], sd[key + ".bias"] = conv.weight.detach(), conv.bias.detach()
    fc = torch.nn.Linear(channels[-1], 2)
    sd["classifier.2.weight"], sd["classifier.2.bias"] = fc.weight.detach(), fc.bias.detach()
    return sd


def _checked_state(state, shapes) -> dict:
    sd = load_state(state)
    out = {}
    for key, shape in shapes.items():
        if key not in sd:
            raise ValueError(f"state dict has no {key!r}")
        a = np.ascontiguousarray(sd[key], dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{key}: shape {a.shape}, expected {shape}")
        out[key] = a
    return out


class Trainer:
    """The net's parameters, their gradients and the Adam moments on the device (rs_train_*), for the shipped class: depth 1,
    every kernel 3 (rs_train_create).  x: float32 [B, L] on the device or the host, y: any integer tensor of B labels in
    {0, 1}.  A batch beyond max_batch(L) is refused, not split: a split would change the mean.  Where a method takes `layer` it
    means the conv index j = layer * depth + d, as the C ABI does."""

    generic = False                                         # which config check applies and which constructor is reached

    def __init__(self, config, state_dict=None, device=None, dtype: str = "f32"):
        if dtype not in ("f32", "fp32", "float32"):
            raise ValueError(f"dtype {dtype!r}: riser_amd.train is fp32 only")
        self._h = None
        self._ws = None
        (check_generic_config if self.generic else check_config)(config)
        self.channels, self.kernels, self.depth = net_of(config)
        self.learning_rate = float(getattr(config, "learning_rate", 1e-3))
        self.n_layers = len(self.channels)
        self._keys = param_keys(self.n_layers, self.depth)
        self._shapes = param_shapes(self.channels, self.kernels, self.depth)
        keep = _checked_state(state_dict if state_dict is not None else init_state(self.channels, self.kernels, self.depth),
                              self._shapes)
        nv.require_gpu()
        d = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        self._h = create_handle(self.channels, keep, self.device.index, self.kernels, self.depth, generic=self.generic)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        self._ws = None
        if h:
            nv.lib().rs_train_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_batch(self, L: int) -> int:
        return int(nv.lib().rs_train_max_batch(self._h, int(L)))

    def slice_plan(self, layer: int, B: int, L: int):
        """(slices, positions per slice) of conv `layer`'s weight-gradient contraction (rs_train_slice_plan)"""
        n, s = C.c_int32(), C.c_int32()
        nv.check(nv.lib().rs_train_slice_plan(self._h, int(layer), int(B), int(L), C.byref(n), C.byref(s)), "rs_train_slice_plan")
        return int(n.value), int(s.value)

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
        need = lib.rs_train_workspace_bytes(self._h, B, L)
        if self._ws is None or self._ws.numel() < max(need, 256):
            self._ws = None
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        out = torch.empty(2 + 2 * B, dtype=torch.float32, device=self.device)
        nv.check(getattr(lib, fn_name)(self._h, x.data_ptr(), y.data_ptr(), B, L, L, self._ws.data_ptr(), self._ws.numel(),
                                       out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), fn_name)
        host = out.cpu()
        return float(host[0]), int(host[1]), host[2:].reshape(B, 2)

    def _adam(self):
        nv.check(nv.lib().rs_train_adam_step(self._h, self.learning_rate, ADAM["beta1"], ADAM["beta2"], ADAM["eps"],
                                             torch.cuda.current_stream(self.device).cuda_stream), "rs_train_adam_step")

    def step(self, x, y) -> float:
        """forward, backward, Adam; the loss of the batch before the update"""
        loss = self._call("rs_train_forward_backward", x, y)[0]
        self._adam()
        return loss

    def loss_and_grads(self, x, y):
        """(loss, {reference key: gradient}) - no update"""
        loss = self._call("rs_train_forward_backward", x, y)[0]
        return loss, self._tensors("rs_train_get_grads")

    def evaluate(self, x, y):
        """(loss, reads classified correctly) of the forward pass alone"""
        loss, n_correct, _ = self._call("rs_train_evaluate", x, y)
        return loss, n_correct

    def logits(self, x, y):
        """the [B, 2] logits of the forward pass alone, on the host"""
        return self._call("rs_train_evaluate", x, y)[2]

    def _tensors(self, fn_name: str) -> dict:
        out = {}
        for i, key in enumerate(self._keys):
            a = np.empty(self._shapes[key], np.float32)
            nv.check(getattr(nv.lib(), fn_name)(self._h, i, a.ctypes.data, a.size), fn_name)
            out[key] = torch.from_numpy(a)
        return out

    def state_dict(self) -> dict:
        """the reference's keys as CPU fp32 tensors (riser/nets/cnn.py's state dict at this depth with `gap_fc`)"""
        return self._tensors("rs_train_get_params")

    def load_state_dict(self, state):
        sd = _checked_state(state, self._shapes)
        for i, key in enumerate(self._keys):
            nv.check(nv.lib().rs_train_set_params(self._h, i, sd[key].ctypes.data, sd[key].size), "rs_train_set_params")

    def debug_copy(self, layer: int, what: str, B: int, L: int) -> torch.Tensor:
        """conv `layer`'s 'y' (the last conv of a layer: pooled rows; an inner conv: its ReLU rows), 'sel' (selectors, pooling
        convs only) or 'dy' (the gradient arriving at 'y') of the last forward + backward of B reads of L samples, on the host:
        [B, rows, c_out], at depth 1 rows = L >> (layer + 1) (rs_train_debug_copy)"""
        level, pools = layer // self.depth, layer % self.depth == self.depth - 1
        c = self.channels[level]
        cp, rows = (c + 3) & ~3, (L >> level) >> (1 if pools else 0)
        dst = torch.empty((B, rows, cp), dtype=torch.uint8 if what == "sel" else torch.float32, device=self.device)
        nv.check(nv.lib().rs_train_debug_copy(self._h, layer, {"y": 0, "sel": 1, "dy": 2}[what], dst.data_ptr(),
                                              dst.numel() * dst.element_size()), "rs_train_debug_copy")
        return dst[:, :, :c].cpu()


class GenericTrainer(Trainer):
    """Trainer for any depth and any odd kernels - every net check_generic_config takes (rs_train_create_generic)"""

    generic = True


def trainer_for(config, state_dict=None, device=None):
    """a Trainer for the shipped class (depth 1, every kernel 3), a GenericTrainer for every other net check_generic_config
    accepts; ValueError before any GPU call for the rest"""
    if is_shipped_class(config):
        return Trainer(config, state_dict, device)
    return GenericTrainer(config, state_dict, device)


def create_handle(channels, state, device_index: int, kernels=None, depth=1, generic=None):
    """a C handle on the arrays of `state` ({reference key: float32 array}): rs_train_create for the shipped class (depth 1,
    every kernel 3), rs_train_create_generic for every other net - the two keep their own limits - or as `generic` says.
    device_index < 0: a handle without device memory, which answers the plan functions and the argument checks on a machine
    without a GPU"""
    specs = list(_convs(channels, kernels, depth))
    convs = (_Conv * len(specs))(*[_Conv(c_in, c, k, 0, state[key + ".weight"].ctypes.data, state[key + ".bias"].ctypes.data)
                                   for key, c_in, c, k in specs])
    head = state["classifier.2.weight"].ctypes.data, state["classifier.2.bias"].ctypes.data
    if generic is None:
        generic = depth != 1 or any(k != 3 for _, _, _, k in specs)
    h = C.c_void_p()
    if generic:
        nv.check(nv.lib().rs_train_create_generic(convs, len(channels), int(depth), *head, int(device_index), C.byref(h)),
                 "rs_train_create_generic")
    else:
        nv.check(nv.lib().rs_train_create(convs, len(channels), *head, int(device_index), C.byref(h)), "rs_train_create")
    return h


# ---- the loop of riser/train.py:31-112,206-245 ------------------------------------------------------------------------------

def load_set(data_dir: str):
    """riser/data.py:5-16: (data [N, cutoff] float32, labels [N] int64), negatives (0) in front of positives (1)"""
    n_x = torch.load(os.path.join(data_dir, "negative.pt"))
    p_x = torch.load(os.path.join(data_dir, "positive.pt"))
    data = torch.cat((n_x, p_x)).float()
    label = torch.cat((torch.zeros(n_x.shape[0], dtype=torch.long), torch.ones(p_x.shape[0], dtype=torch.long)))
    return data, label


def batches_of(n: int, batch_size: int, shuffle: bool, rng) -> list:
    """index batches of one loader over n reads: a permutation when shuffled, the last batch short"""
    order = list(range(n))
    if shuffle:
        rng.shuffle(order)
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def combined_rounds(sets: dict, batch_size: int, shuffle: bool, rng):
    """CombinedLoader(mode="max_size") (riser/train.py:157): the loaders are stepped together until the longest is
    exhausted; a loader that ran out gives None.  Yields {key: index batch | None} per round."""
    plans = {k: batches_of(len(sets[k][1]), batch_size, shuffle, rng) for k in LENGTH_KEYS if k in sets}
    for r in range(max((len(p) for p in plans.values()), default=0)):
        yield {k: (p[r] if r < len(p) else None) for k, p in plans.items()}


def _take(dataset, idx):
    data, label = dataset
    i = torch.as_tensor(idx, dtype=torch.long)
    return data[i], label[i]


def train_epoch(trainer, sets, batch_size, epoch, rng, log_freq=100, log=print) -> float:
    n_samples = sum(len(sets[k][1]) for k in sets)
    n_batches = sum(-(-len(sets[k][1]) // batch_size) for k in sets)
    log(f"Total size of training set: {n_samples}")
    log(f"Number of batches in training set: {n_batches}")
    total, batch_n = 0.0, 0
    keys = [k for k in LENGTH_KEYS if k in sets]
    for rnd in combined_rounds(sets, batch_size, True, rng):
        rng.shuffle(keys)                                   # riser/train.py:46
        for k in keys:
            if rnd[k] is None:
                continue
            X, y = _take(sets[k], rnd[k])
            total += trainer.step(X, y)
            if batch_n != 0 and batch_n % log_freq == 0:
                log(f"loss: {total / batch_n:>7f} [{batch_n * len(X):>5d}/{n_samples:>5d}]")
            batch_n += 1
    return total / max(n_batches, 1)


def validate(trainer, sets, batch_size, log=print):
    n_samples = sum(len(sets[k][1]) for k in sets)
    n_batches = sum(-(-len(sets[k][1]) // batch_size) for k in sets)
    total, n_correct = 0.0, 0
    for rnd in combined_rounds(sets, batch_size, False, None):
        for k in LENGTH_KEYS:
            if k not in rnd or rnd[k] is None:
                continue
            X, y = _take(sets[k], rnd[k])
            loss, ok = trainer.evaluate(X, y)
            total += loss
            n_correct += ok
    avg, acc = total / max(n_batches, 1), n_correct / max(n_samples, 1) * 100
    log(f"Validation set: \n Accuracy: {acc:>0.1f}%, Avg loss: {avg:>8f} \n")
    return avg, acc


def checkpoint_names(exp_dir: str, exp_id: str, start_epoch: int):
    """(best, latest) as riser/train.py:238,242 names them"""
    return (os.path.join(exp_dir, f"{exp_id}_{start_epoch}_best_model.pth"), os.path.join(exp_dir, f"{exp_id}_latest_model.pth"))


def fit(trainer, train_sets, val_sets, n_epochs, batch_size, exp_dir, exp_id, start_epoch=0, seed=None, log=print):
    """riser/train.py:206-245.  train_sets / val_sets: {'2s' | '3s' | '4s': (data [N, cutoff], labels [N])}.  Returns
    (best accuracy, its epoch)."""
    rng = random.Random(seed)
    best_path, latest_path = checkpoint_names(exp_dir, exp_id, start_epoch)
    os.makedirs(exp_dir, exist_ok=True)
    best_acc, best_epoch = 0, 0
    with open(os.path.join(exp_dir, "metrics.tsv"), "a") as tsv:
        if tsv.tell() == 0:
            tsv.write("\t".join(METRICS) + "\n")
        for t in range(start_epoch, n_epochs):
            log(f"Epoch {t}\n-------------------------------")
            t0 = time.time()
            train_loss = train_epoch(trainer, train_sets, batch_size, t, rng, log=log)
            t1 = time.time()
            val_loss, val_acc = validate(trainer, val_sets, batch_size, log=log)
            t2 = time.time()
            row = (t, train_loss, val_loss, val_acc, t1 - t0, t2 - t1, train_loss - val_loss)
            tsv.write("\t".join(str(v) if isinstance(v, int) else f"{v:.9g}" for v in row) + "\n")
            tsv.flush()
            if val_acc > best_acc:
                best_acc, best_epoch = val_acc, t
                torch.save(trainer.state_dict(), best_path)
                log(f"Saved best model at epoch {t} with val accuracy {best_acc}.")
            torch.save(trainer.state_dict(), latest_path)
            log(f"Saved latest model at epoch {t} with val accuracy {val_acc}.")
    log(f"Best model with validation accuracy {best_acc} saved at epoch {best_epoch}.")
    return best_acc, best_epoch


def parse_args(argv=None):
    """riser/train.py:129-133,188-192: five positional arguments; a checkpoint needs START_EPOCH > 0, none needs 0"""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m riser_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("exp_dir")
    ap.add_argument("data_dir")
    ap.add_argument("checkpt", help="file name inside EXP_DIR, or None")
    ap.add_argument("config_file")
    ap.add_argument("start_epoch", type=int)
    a = ap.parse_args(argv)
    a.checkpt = None if a.checkpt == "None" else a.checkpt
    if a.checkpt is not None:
        assert a.start_epoch > 0, "a checkpoint resumes at START_EPOCH > 0"
    else:
        assert a.start_epoch == 0, "without a checkpoint START_EPOCH is 0"
    a.exp_id = a.exp_dir.split("/")[-1]                     # riser/train.py:146
    return a


def main(argv=None) -> int:
    from .modeldir import get_config
    a = parse_args(argv)
    print(f"Experiment dir: {a.exp_dir}\nData dir: {a.data_dir}\nCheckpoint: {a.checkpt}\nConfig file: {a.config_file}")
    config = get_config(a.config_file)
    is_shipped_class(config)
    print("Creating data loaders...")
    sets = {split: {k: load_set(os.path.join(a.data_dir, k, split)) for k in LENGTH_KEYS} for split in ("train", "val")}
    state = os.path.join(a.exp_dir, a.checkpt) if a.checkpt is not None else None
    trainer = trainer_for(config, state)
    try:
        fit(trainer, sets["train"], sets["val"], int(config.n_epochs), int(config.batch_size), a.exp_dir, a.exp_id, a.start_epoch)
    finally:
        trainer.close()
    print("Training complete.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
