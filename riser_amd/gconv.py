"""Generic ConvNets (riser/nets/cnn.py:12-18,43-65 at any `depth` and any odd `kernels`) on the GPU.

The reference builds n_layers x [depth x (Conv1d(k, stride 1, 'same') + ReLU), MaxPool1d(2, 2)] (cnn.py:52-65) and, with the
`gap_fc` classifier, AdaptiveAvgPool1d(1) + Linear (cnn.py:28-33).  The shipped shape (depth 1, kernel 3) has its own tuned
path (Model); every other shape runs here: this module folds a reference state dict into a flat conv list (pure numpy, no
GPU) and drives the device program of csrc/gconv.hip (rs_gconv_*): one tiled launch per conv with bias, ReLU and the layer's
max-pool in its epilogue, reads of any length in one call.  dtype 'bf16x3' runs the convs with more than 4 input channels in
split precision on the bf16 MFMA (csrc/gconv_x3.hip); fp32 is the default.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as nv
from ._family import FamilyNet, load_state


def _get(sd, key):
    if key not in sd:
        raise ValueError(f"state dict has no {key!r}")
    return np.ascontiguousarray(sd[key], dtype=np.float32)


def build_gconv_program(sd, cnn) -> dict:
    """dict(convs=[dict(w [co, ci, k], b, k)] (layer-major, n_layers * depth entries), n_layers, depth, fc_w [2, c_last],
    fc_b [2]) of a reference ConvNet state dict and its `config.cnn`.  Refuses (ValueError) what the device does not run
    (even kernels, heads other than two-class `gap_fc`) or what does not match the state dict."""
    n_layers, depth = int(cnn.n_layers), int(getattr(cnn, "depth", 1))
    channels, kernels = [int(v) for v in cnn.channels], [int(v) for v in cnn.kernels]
    if n_layers < 1 or depth < 1:
        raise ValueError("n_layers and depth must be >= 1")
    if len(channels) < n_layers or len(kernels) < n_layers:
        raise ValueError(f"channels {channels} / kernels {kernels}: shorter than n_layers {n_layers}")
    if any(k % 2 == 0 for k in kernels[:n_layers]):
        raise ValueError("riser_amd: even conv kernels ('same' pads them asymmetrically) are not supported")
    classifier = getattr(cnn, "classifier", "gap_fc")
    if classifier != "gap_fc":
        raise ValueError(f"classifier {classifier!r}: the generic ConvNet family runs the `gap_fc` head only")
    if int(cnn.n_classes) != 2:
        raise ValueError("riser_amd supports two-class heads only")
    sd = load_state(sd)
    convs, c_in = [], 1
    for i in range(n_layers):
        for d in range(depth):
            # nn.Sequential indices of cnn.py:52-65: conv, ReLU, conv, ReLU, ..., MaxPool1d
            w, b = _get(sd, f"layers.{i}.{2 * d}.weight"), _get(sd, f"layers.{i}.{2 * d}.bias")
            if w.shape != (channels[i], c_in, kernels[i]) or b.shape != (channels[i],):
                raise ValueError(f"layers.{i}.{2 * d}: weight {w.shape} / bias {b.shape}, expected ({channels[i]}, {c_in}, "
                                 f"{kernels[i]}) / ({channels[i]},)")
            convs.append(dict(w=w, b=b, k=kernels[i]))
            c_in = channels[i]
    fw, fb = _get(sd, "classifier.2.weight"), _get(sd, "classifier.2.bias")
    if fw.shape != (2, c_in) or fb.shape != (2,):
        raise ValueError(f"classifier.2.weight {fw.shape}: expected (2, {c_in})")
    return dict(convs=convs, n_layers=n_layers, depth=depth, fc_w=fw, fc_b=fb)


def min_length(prog) -> int:
    """the shortest read the reference can run: every MaxPool1d(2, 2) needs two rows"""
    return 1 << int(prog["n_layers"])


def program_macs(prog, L: int) -> int:
    """multiply-adds of one read of L samples: every conv on the L >> layer rows it keeps ('same'), head excluded"""
    total, depth = 0, int(prog["depth"])
    for i, cv in enumerate(prog["convs"]):
        co, ci, k = cv["w"].shape
        total += (int(L) >> (i // depth)) * co * ci * k
    return int(total)


class _Conv(C.Structure):
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32),
                ("w", C.c_void_p), ("b", C.c_void_p)]


def layer_plan(c_in: int, c_out: int, k: int) -> dict:
    """the tile a conv of these sizes takes (rs_gconv_layer_plan): rows x cols of a workgroup, the K chunk, its LDS; a
    function of the conv alone, never of the batch.  Needs no GPU."""
    p = nv.GConvPlan()
    nv.check(nv.lib().rs_gconv_layer_plan(int(c_in), int(c_out), int(k), C.byref(p)), "rs_gconv_layer_plan")
    return {n: int(getattr(p, n)) for n, _ in nv.GConvPlan._fields_ if n != "reserved"}


def x3_layout(c_in: int, c_out: int, k: int, w=None):
    """the split-precision form of a conv with c_in > 4 (rs_gconv_x3_layout): dict(steps, slab_rows, slab_pitch, lds_bytes,
    plane) and, given its weights w [c_out, c_in, k], `packed`: uint16 [2, plane], the hi and lo planes in the order the
    device's lanes read them.  Needs no GPU."""
    p = nv.GConvX3Plan()
    lib = nv.lib()
    nv.check(lib.rs_gconv_x3_layout(int(c_in), int(c_out), int(k), C.byref(p), None, None), "rs_gconv_x3_layout")
    out = {n: int(getattr(p, n)) for n, _ in nv.GConvX3Plan._fields_}
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.shape != (c_out, c_in, k):
            raise ValueError(f"w {w.shape}: expected ({c_out}, {c_in}, {k})")
        packed = np.zeros((2, out["plane"]), np.uint16)
        nv.check(lib.rs_gconv_x3_layout(int(c_in), int(c_out), int(k), C.byref(p), w.ctypes.data, packed.ctypes.data),
                 "rs_gconv_x3_layout")
        out["packed"] = packed
    return out


class GConvNet(FamilyNet):
    """A generic ConvNet on the device (rs_gconv_*): the surface Model drives for SeqNet - forward, forward_ragged,
    max_batch.  fp32 on the f32-input MFMA (the default) or, dtype 'bf16x3', the convs with more than 4 input channels in
    split precision on the bf16 MFMA (rs_gconv_set_mode, also between forwards: fp32 after bf16x3 gives the bits of a fresh
    fp32 net)."""

    _PREFIX = "rs_gconv"
    _MODES = {"f32": ("f32", nv.RS_F32), "f32w": ("f32", nv.RS_F32W), "fp32": ("f32", nv.RS_F32),
              "bf16x3": ("bf16x3", nv.RS_BF16X3)}

    @classmethod
    def _refused_dtype(cls, dtype):
        return (f"dtype {dtype!r}: configs with depth > 1 or kernels other than 3 run the generic conv program in 'f32w' / "
                "'f32' (f32-input MFMA) or 'bf16x3' (split precision on the bf16 MFMA) only")

    def _no_workspace(self, B, ld):
        return f"no workspace for {B} reads of {ld} samples (the network minimum is {self.min_length})"

    def _create(self):
        prog = self._keep
        convs = (_Conv * len(prog["convs"]))()
        for i, cv in enumerate(prog["convs"]):
            co, ci, k = cv["w"].shape
            convs[i] = _Conv(ci, co, k, 0, cv["w"].ctypes.data, cv["b"].ctypes.data)
        h = C.c_void_p()
        nv.check(nv.lib().rs_gconv_create(convs, int(prog["n_layers"]), int(prog["depth"]), prog["fc_w"].ctypes.data,
                                          prog["fc_b"].ctypes.data, self.device.index, C.byref(h)), "rs_gconv_create")
        return h

    @property
    def min_length(self) -> int:
        return int(nv.lib().rs_gconv_min_length(self._h))

    def layer_plans(self):
        """layer_plan of every conv, in launch order"""
        return [layer_plan(cv["w"].shape[1], cv["w"].shape[0], cv["w"].shape[2]) for cv in self._keep["convs"]]
