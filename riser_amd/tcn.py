"""TCN and bottleneck TCN (riser/nets/tcn.py, riser/nets/tcn_bot.py) on the GPU.

Both nets classify the LAST position of the read (tcn.py:87) through causal convs only (left padding, then Chomp1d), so
the logits depend on the last receptive field of the read and, inside it, on a strided subset of positions: block i
(dilation d_i) is needed only at positions L-1 - d_i * m, m = 0, 1, ...  On that subsequence a k-tap conv of dilation d_i
is a dense k-tap causal conv, and between block i and block i+1 the sequence is subsampled by base = d_{i+1} / d_i,
counting back from the last sample.  This module folds a reference state dict into per-block conv lists (pure numpy,
no GPU), works out the per-block windows of that cone, and drives the device program of csrc/tcn.hip (rs_tcn_*; in dtype
'bf16x3' the blocks run csrc/tcn_x3.hip).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nv
from ._family import FamilyNet, load_state


def _fold_weight_norm(sd, prefix):
    """weight_norm(Conv1d) -> fp32 [c_out, c_in, k]: w = g * v / ||v||, the norm over dims 1 and 2 per output channel, in
    float64.  Accepts both spellings torch writes: `weight_g` / `weight_v` (torch.nn.utils.weight_norm, what the reference
    uses) and `parametrizations.weight.original0` / `original1` (torch.nn.utils.parametrizations.weight_norm)."""
    if prefix + ".weight_g" in sd:
        g, v = sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]
    elif prefix + ".parametrizations.weight.original0" in sd:
        g, v = sd[prefix + ".parametrizations.weight.original0"], sd[prefix + ".parametrizations.weight.original1"]
    elif prefix + ".weight" in sd:
        return np.ascontiguousarray(sd[prefix + ".weight"], dtype=np.float32)
    else:
        raise KeyError(f"{prefix}: no weight_g / weight_v, parametrizations.weight.original0 / 1 or weight")
    v = np.asarray(v, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64).reshape(v.shape[0], 1, 1)
    norm = np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))
    return np.ascontiguousarray((g * v / norm).astype(np.float32))


def _conv(sd, prefix, causal):
    w = _fold_weight_norm(sd, prefix)
    b = np.ascontiguousarray(sd[prefix + ".bias"], dtype=np.float32)
    return dict(w=w, b=b, k=int(w.shape[2]), causal=bool(causal))


def build_tcn_program(sd, c, bottleneck: bool):
    """(blocks, fc_w, fc_b) of a reference TCN (bottleneck=False, riser/nets/tcn.py) or TCNBot (riser/nets/tcn_bot.py)
    state dict.  blocks[i] = dict(convs=[dict(w [co, ci, k] fp32, b, k, causal)], shortcut=(w [co, ci], b) or None,
    base=d_{i+1} / d_i, dilation=d_i).  Every conv is followed by a ReLU; the block output is relu(convs + residual)."""
    sd = load_state(sd)
    k = int(c.kernel)
    n_layers = int(c.n_layers)
    n_filters = int(c.n_filters)
    if k < 2:
        raise ValueError(f"kernel {k}: the reference's Chomp1d(0) empties the tensor (riser/nets/tcn.py:15); kernel >= 2")
    if int(getattr(c, "in_channels", 1)) != 1:
        raise ValueError(f"in_channels {c.in_channels}: the reference feeds one signal channel (tcn.py:85 unsqueeze(1))")
    if int(c.n_classes) != 2:
        raise ValueError("riser_amd supports two-class heads only")
    if n_layers < 1:
        raise ValueError("n_layers must be >= 1")
    base = 2 if bottleneck else int(c.dilation)          # tcn_bot.py:70 hard-wires 2 ** i
    if base < 1:
        raise ValueError(f"dilation {base}: must be >= 1")
    blocks, d = [], 1
    for i in range(n_layers):
        pre = f"layers.{i}"
        c_in = 1 if i == 0 else n_filters
        if bottleneck:
            convs = [_conv(sd, f"{pre}.blocks.0.0", False), _conv(sd, f"{pre}.blocks.1.0", True),
                     _conv(sd, f"{pre}.blocks.2.0", True), _conv(sd, f"{pre}.blocks.3.0", False)]
        else:
            convs = [_conv(sd, f"{pre}.blocks.0.0", True), _conv(sd, f"{pre}.blocks.1.0", True)]
        if convs[0]["w"].shape[1] != c_in or convs[-1]["w"].shape[0] != n_filters:
            raise ValueError(f"{pre}: conv shapes do not match in_channels / n_filters")
        shortcut = None
        if c_in != n_filters:                               # should_apply_shortcut (tcn.py:57-59)
            sw = np.asarray(sd[f"{pre}.shortcut.weight"], dtype=np.float32)
            shortcut = (np.ascontiguousarray(sw[:, :, 0]), np.ascontiguousarray(sd[f"{pre}.shortcut.bias"], dtype=np.float32))
        blocks.append(dict(convs=convs, shortcut=shortcut, base=base, dilation=d))
        d *= base
    fw = np.ascontiguousarray(sd["linear.weight"], dtype=np.float32)
    fb = np.ascontiguousarray(sd["linear.bias"], dtype=np.float32)
    if fw.shape != (2, n_filters):
        raise ValueError(f"linear.weight {fw.shape}: expected (2, {n_filters})")
    return blocks, fw, fb


def receptive_field(blocks) -> int:
    """1 + sum over the causal convs of (k - 1) * dilation (= the reference's get_receptive_field), an exact int"""
    return 1 + sum((cv["k"] - 1) * b["dilation"] for b in blocks for cv in b["convs"] if cv["causal"])


def windows(blocks, ld: int):
    """Input positions of every block for reads of up to ld samples: need[i] = positions L-1 - d_i * m, m < need[i], that
    block i reads; need[n] = 1 (the last position).  need_i = (need_{i+1} - 1) * base + 1 + sum of the block's (k - 1),
    clamped to ceil(ld / d_i): the positions beyond that are below 0 for every read (zero padding, never computed)."""
    n = len(blocks)
    need = [0] * (n + 1)
    need[n] = 1
    for i in range(n - 1, -1, -1):
        b = blocks[i]
        span = sum(cv["k"] - 1 for cv in b["convs"] if cv["causal"])
        want = (need[i + 1] - 1) * b["base"] + 1 + span
        need[i] = int(min(want, -(-int(ld) // b["dilation"])))
    return need


def program_macs(blocks, ld: int) -> int:
    """multiply-adds of one read of ld samples through the cone as csrc/tcn.hip computes it (dense up to the last k-conv of
    a block, strided after it), head excluded"""
    need = windows(blocks, ld)
    total = 0
    for i, b in enumerate(blocks):
        out, r = need[i + 1], b["base"]
        convs = b["convs"]
        jk = max(j for j, cv in enumerate(convs) if cv["k"] > 1)
        rows = out
        for j in range(len(convs) - 1, -1, -1):
            co, ci, k = convs[j]["w"].shape
            total += rows * co * ci * k
            rows = (rows - 1) * (r if j == jk else 1) + k
        if b["shortcut"] is not None:
            total += out * b["shortcut"][0].size
    return int(total)


class _TcnConv(C.Structure):
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("k", C.c_int32), ("causal", C.c_int32),
                ("w", C.c_void_p), ("b", C.c_void_p)]


class _TcnBlock(C.Structure):
    _fields_ = [("n_convs", C.c_int32), ("base", C.c_int32), ("convs", _TcnConv * 4), ("has_shortcut", C.c_int32),
                ("reserved", C.c_int32), ("sc_w", C.c_void_p), ("sc_b", C.c_void_p)]


class TCNNet(FamilyNet):
    """A TCN / TCNBot on the device (rs_tcn_*): the surface Model drives for SeqNet - forward, forward_ragged, max_batch.
    dtype: 'f32' / 'f32w' / 'fp32' (fp32 on the f32-input MFMA) or 'bf16x3' (every conv in split precision on the bf16 MFMA,
    csrc/tcn_x3.hip: rs_tcn_set_mode)"""

    _PREFIX = "rs_tcn"
    min_length = 1                  # causal convs: any read of one sample or more has a last position
    _MODES = {"f32": ("f32", nv.RS_F32), "f32w": ("f32", nv.RS_F32W), "fp32": ("f32", nv.RS_F32),
              "bf16x3": ("bf16x3", nv.RS_BF16X3)}

    def __init__(self, blocks, fw, fb, device, dtype: str = "f32"):
        super().__init__((blocks, fw, fb), device, dtype)

    @classmethod
    def _refused_dtype(cls, dtype):
        return (f"dtype {dtype!r}: a TCN runs in 'f32w' / 'f32' (f32-input MFMA) or 'bf16x3' (split precision on the bf16 "
                "MFMA)")

    def _create(self):
        blocks, fw, fb = self._keep
        arr = (_TcnBlock * len(blocks))()
        for i, b in enumerate(blocks):
            arr[i].n_convs = len(b["convs"])
            arr[i].base = int(b["base"])
            for j, cv in enumerate(b["convs"]):
                co, ci, k = cv["w"].shape
                arr[i].convs[j] = _TcnConv(ci, co, k, int(cv["causal"]), cv["w"].ctypes.data, cv["b"].ctypes.data)
            if b["shortcut"] is not None:
                arr[i].has_shortcut = 1
                arr[i].sc_w = b["shortcut"][0].ctypes.data
                arr[i].sc_b = b["shortcut"][1].ctypes.data
        h = C.c_void_p()
        nv.check(nv.lib().rs_tcn_create(arr, len(blocks), fw.ctypes.data, fb.ctypes.data, int(fw.shape[1]),
                                        self.device.index, C.byref(h)), "rs_tcn_create")
        return h

    @property
    def receptive_field(self) -> int:
        return int(nv.lib().rs_tcn_receptive_field(self._h))
