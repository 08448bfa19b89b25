"""CNN-RNN (riser/nets/cnn_rnn.py, ConvRecNet) on the GPU.

The reference runs n_conv_layers x [valid Conv1d + bias -> MaxPool1d(2, 2) -> ReLU] (cnn_rnn.py:12-18,47-53), permutes to
(B, T, C), runs `rec_layers` and classifies the last step (cnn_rnn.py:36-44).  Two quirks of the reference are kept:
  - `rec_layers` holds n_rec_layers modules and EACH is an nn.LSTM / nn.GRU with num_layers = n_rec_layers
    (cnn_rnn.py:20-27,55-70): n_rec_layers^2 stacked layers;
  - the ReLU runs after each module on its whole output sequence (cnn_rnn.py:43), not between the layers inside one.
This module folds a reference state dict into a flat layer list (pure numpy, no GPU) and drives the device program of
csrc/crnn.hip (rs_crnn_*).  Of the last layer only the final state is read: its output sequence is never written, and in a
bidirectional net its backward direction runs one step (at t = T - 1 it has seen one input, from the zero state).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nv
from ._family import FamilyNet, load_state

CELLS = {"lstm": 0, "gru": 1}
GATES = {"lstm": 4, "gru": 3}


def _get(sd, key):
    if key not in sd:
        raise ValueError(f"state dict has no {key!r}")
    return np.ascontiguousarray(sd[key], dtype=np.float32)


def build_crnn_program(sd, c) -> dict:
    """dict(convs=[dict(w [co, ci, k], b, k)], layers=[dict(cell, in_dim, hidden, bidirectional, w_ih, w_hh, b_ih, b_hh
    (lists per direction), relu_after)], fc_w [2, out_dim], fc_b [2], out_dim) of a reference ConvRecNet state dict and its
    `config.cnn_rnn`.  Refuses (ValueError) what the reference cannot run or what does not match the state dict."""
    sd = load_state(sd)
    cell = str(getattr(c, "cell", "")).lower()
    if cell not in CELLS:
        raise ValueError(f"cell {getattr(c, 'cell', None)!r}: the reference knows 'lstm' and 'gru' (cnn_rnn.py:55-70)")
    if int(c.n_classes) != 2:
        raise ValueError("riser_amd supports two-class heads only")
    n_conv = int(c.n_conv_layers)
    channels, kernels = [int(v) for v in c.channels], [int(v) for v in c.kernels]
    if n_conv < 1:
        raise ValueError("n_conv_layers must be >= 1")
    if len(channels) < n_conv or len(kernels) < n_conv:
        raise ValueError(f"channels {channels} / kernels {kernels}: shorter than n_conv_layers {n_conv}")
    convs, c_in = [], 1
    for i in range(n_conv):
        w, b = _get(sd, f"conv_layers.{i}.0.weight"), _get(sd, f"conv_layers.{i}.0.bias")
        if w.shape != (channels[i], c_in, kernels[i]) or b.shape != (channels[i],):
            raise ValueError(f"conv_layers.{i}.0: weight {w.shape} / bias {b.shape}, expected ({channels[i]}, {c_in}, "
                             f"{kernels[i]}) / ({channels[i]},)")
        convs.append(dict(w=w, b=b, k=kernels[i]))
        c_in = channels[i]
    if channels[-1] != c_in:
        # the reference builds its first recurrent layer for channels[-1] inputs (cnn_rnn.py:25) and crashes on the first read
        raise ValueError(f"channels[-1] = {channels[-1]} is not the last conv layer's {c_in} output channels")
    hidden, n_rec = int(c.hidden), int(c.n_rec_layers)
    bidir = bool(c.bidirectional)
    if hidden < 1 or n_rec < 1:
        raise ValueError("hidden and n_rec_layers must be >= 1")
    ndir = 2 if bidir else 1
    ng = GATES[cell]
    out_dim = hidden * ndir
    layers = []
    for m in range(n_rec):
        for j in range(n_rec):
            in_dim = (channels[-1] if m == 0 else out_dim) if j == 0 else out_dim
            lay = dict(cell=cell, in_dim=in_dim, hidden=hidden, bidirectional=bidir, relu_after=(j == n_rec - 1),
                       w_ih=[], w_hh=[], b_ih=[], b_hh=[])
            for d in range(ndir):
                sfx = f"_l{j}" + ("_reverse" if d else "")
                pre = f"rec_layers.{m}."
                shapes = dict(weight_ih=(ng * hidden, in_dim), weight_hh=(ng * hidden, hidden), bias_ih=(ng * hidden,),
                              bias_hh=(ng * hidden,))
                for name, shp in shapes.items():
                    v = _get(sd, pre + name + sfx)
                    if v.shape != shp:
                        raise ValueError(f"{pre + name + sfx}: shape {v.shape}, expected {shp} ({cell}, hidden {hidden})")
                    lay[{"weight_ih": "w_ih", "weight_hh": "w_hh", "bias_ih": "b_ih", "bias_hh": "b_hh"}[name]].append(v)
            layers.append(lay)
    fw, fb = _get(sd, "linear.weight"), _get(sd, "linear.bias")
    if fw.shape != (2, out_dim) or fb.shape != (2,):
        raise ValueError(f"linear.weight {fw.shape}: expected (2, {out_dim})")
    return dict(convs=convs, layers=layers, fc_w=fw, fc_b=fb, out_dim=out_dim)


def steps(prog, L: int) -> int:
    """recurrent steps T of a read of L samples: L_{i+1} = (L_i - k_i + 1) // 2; 0 where the reference's conv or max_pool
    raises (it needs k_i + 1 samples at every conv layer)"""
    L = int(L)
    for cv in prog["convs"]:
        L = (L - cv["k"] + 1) // 2 if L >= cv["k"] + 1 else 0
    return L


def min_length(prog) -> int:
    """the shortest read with one recurrent step"""
    need = 1
    for cv in reversed(prog["convs"]):
        need = 2 * need + cv["k"] - 1
    return need


def program_macs(prog, L: int) -> int:
    """multiply-adds of one read of L samples as csrc/crnn.hip executes them: the conv front, every layer's input
    projection and recurrence over T steps in both directions, except the last layer's backward direction (one step) -
    head excluded"""
    total, Li = 0, int(L)
    for cv in prog["convs"]:
        co, ci, k = cv["w"].shape
        total += (Li - k + 1) * co * ci * k
        Li = (Li - k + 1) // 2
    T = Li
    for n, lay in enumerate(prog["layers"]):
        g = GATES[lay["cell"]] * lay["hidden"]
        per = g * (lay["in_dim"] + lay["hidden"])
        ndir = 2 if lay["bidirectional"] else 1
        for d in range(ndir):
            total += (1 if (d == 1 and n == len(prog["layers"]) - 1) else T) * per
    return int(total)


class _Conv(C.Structure):
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32),
                ("w", C.c_void_p), ("b", C.c_void_p)]


class _Layer(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("cell", "in_dim", "hidden", "bidirectional", "relu_after", "reserved")] + \
               [(n, C.c_void_p * 2) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


class CRNNNet(FamilyNet):
    """A ConvRecNet on the device (rs_crnn_*): the surface Model drives for SeqNet - forward, forward_ragged, max_batch.
    dtype "f32" (also "f32w" / "fp32": fp32 on the f32-input MFMA, the default) or "f16x3": the gate GEMMs whose input is a
    hidden state (every recurrence, the input projection of every layer but the first) in split precision on the f16 MFMA,
    everything else fp32 (rs_crnn_set_mode, also between forwards).  A hidden state lies in (-1, 1) and the weights are packed
    with a power-of-two scale, so no f16 operand can overflow: the mode has no range check and never reports saturation."""

    _PREFIX = "rs_crnn"
    _MODES = {"f32": ("f32", nv.RS_F32), "f32w": ("f32", nv.RS_F32W), "fp32": ("f32", nv.RS_F32),
              "f16x3": ("f16x3", nv.RS_F16X3)}

    @classmethod
    def _refused_dtype(cls, dtype):
        return (f"dtype {dtype!r}: a CNN-RNN runs in 'f32w' / 'f32' (fp32 on the f32-input MFMA) or 'f16x3' (split precision "
                "on the f16 MFMA for the gate GEMMs of hidden states)")

    def _no_workspace(self, B, ld):
        return f"no workspace for {B} reads of {ld} samples (the network minimum is {self.min_length})"

    def _create(self):
        prog = self._keep
        convs = (_Conv * len(prog["convs"]))()
        for i, cv in enumerate(prog["convs"]):
            co, ci, k = cv["w"].shape
            convs[i] = _Conv(ci, co, k, 0, cv["w"].ctypes.data, cv["b"].ctypes.data)
        layers = (_Layer * len(prog["layers"]))()
        for i, lay in enumerate(prog["layers"]):
            s = layers[i]
            s.cell, s.in_dim, s.hidden = CELLS[lay["cell"]], lay["in_dim"], lay["hidden"]
            s.bidirectional, s.relu_after = int(lay["bidirectional"]), int(lay["relu_after"])
            for d_ in range(2 if lay["bidirectional"] else 1):
                s.w_ih[d_], s.w_hh[d_] = lay["w_ih"][d_].ctypes.data, lay["w_hh"][d_].ctypes.data
                s.b_ih[d_], s.b_hh[d_] = lay["b_ih"][d_].ctypes.data, lay["b_hh"][d_].ctypes.data
        h = C.c_void_p()
        nv.check(nv.lib().rs_crnn_create(convs, len(convs), layers, len(layers), prog["fc_w"].ctypes.data,
                                         prog["fc_b"].ctypes.data, int(prog["out_dim"]), self.device.index, C.byref(h)),
                 "rs_crnn_create")
        return h

    @property
    def min_length(self) -> int:
        """shorter: the reference's conv or max_pool raises"""
        return int(nv.lib().rs_crnn_min_length(self._h))

    def steps(self, L: int) -> int:
        return int(nv.lib().rs_crnn_steps(self._h, int(L)))
