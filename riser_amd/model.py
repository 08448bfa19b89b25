"""Model: drop-in for riser/model.py:6-32 on MI355X, plus the batched entry points.

`Model(state, config, logger, target)` and `classify(signal) -> Tensor[2]` keep the
reference's signature and meaning (probabilities in the order (p_off_target, p_on_target),
riser/control.py:69).  The forward pass itself is the HIP library (riser_amd/csrc) reached
through the C ABI; torch is used only for device memory and the current stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _native as nv
from ._family import load_state

_DTYPES = {"f32": nv.RS_F32, "fp32": nv.RS_F32, "float32": nv.RS_F32,
           "bf16": nv.RS_BF16, "bfloat16": nv.RS_BF16, "f16": nv.RS_F16, "fp16": nv.RS_F16,
           "float16": nv.RS_F16, "f32w": nv.RS_F32W, "f32_winograd": nv.RS_F32W,
           "bf16x3": nv.RS_BF16X3, "f16x3": nv.RS_F16X3, "f16xf8": nv.RS_F16XF8}
# the library dtypes that store activations as IEEE half, and the canonical name of every library dtype ("fp16" -> "f16")
_HALF_LIB_DTYPES = (nv.RS_F16, nv.RS_F16X3, nv.RS_F16XF8)
_CANONICAL = {nv.RS_F32: "f32", nv.RS_BF16: "bf16", nv.RS_F16: "f16", nv.RS_F32W: "f32w", nv.RS_BF16X3: "bf16x3",
              nv.RS_F16X3: "f16x3", nv.RS_F16XF8: "f16xf8"}


def is_half_dtype(dtype: str) -> bool:
    """True when `dtype` - a canonical name or an alias ("fp16", "float16") - selects a library mode that stores activations
    as IEEE half (RS_F16 / RS_F16X3 / RS_F16XF8): decided by the library dtype the name maps to, not by its spelling"""
    return _DTYPES.get(dtype) in _HALF_LIB_DTYPES


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def select_architecture(config) -> str:
    """Which of "cnn-rnn", "tcn-bot", "tcn", "resnet", "cnn" a config asks Model for: by its `model`
    string, else by the section it carries - and a `cnn` section beats every other section.  The first rule that holds
    decides; an unknown `model` string names nothing, so the sections decide.  Reads attributes only: no torch, no GPU."""
    kind = getattr(config, "model", None)
    others = not hasattr(config, "cnn")             # the presence of another section counts only without a `cnn` one
    if kind == "cnn-rnn" or (kind is None and others and hasattr(config, "cnn_rnn")):
        return "cnn-rnn"
    if kind == "resnet" or (others and hasattr(config, "resnet")):
        return "resnet"
    if kind == "tcn-bot" or (kind != "tcn" and others and hasattr(config, "tcnbot")):
        return "tcn-bot"
    if kind == "tcn" or (others and hasattr(config, "tcn")):
        return "tcn"
    return "cnn"


def _outputs(device, shape, out=None, return_logits: bool = False):
    """(probs, logits) of an entry point: the caller's `out` or a new fp32 tensor of `shape`, and logits only when asked for"""
    probs = out if out is not None else torch.empty(shape, dtype=torch.float32, device=device)
    return probs, (torch.empty(shape, dtype=torch.float32, device=device) if return_logits else None)


def _call_bounds(B: int, mb: int):
    """[(s0, s1), ...]: the sub-batches a batch of B reads is cut into at mb = Model.call_batch(B, lmax) reads per library call
    (of an ensemble: its most restrictive model's); empty when one call takes the whole batch.  Reads are independent, so the
    cut changes nothing but the time."""
    return [(s0, min(B, s0 + mb)) for s0 in range(0, B, mb)] if B > mb else ()


class Workspace:
    """Grow-only device scratch owned by the caller side of the ABI: ONE BUFFER PER STREAM, so that calls issued on
    different HIP streams (two batches in flight: stream.classify_resident) never share activations.  Keyed by the
    stream that is current when the call is made; a library call only ever touches the workspace it is handed."""

    MAX_STREAMS = 8          # workspaces kept alive: a caller cycling through more streams than this re-allocates

    def __init__(self, device):
        self.device = device
        self._bufs = {}

    def get(self, nbytes: int) -> torch.Tensor:
        key = _stream_ptr(self.device)
        buf = self._bufs.pop(key, None)                      # re-inserted below: the dict's order is the order of last use
        if buf is None or buf.numel() < nbytes:
            buf = None                                       # release the smaller one before the new one is allocated
            if len(self._bufs) >= self.MAX_STREAMS:          # drop the workspace of the stream used longest ago
                del self._bufs[next(iter(self._bufs))]
            with torch.cuda.stream(torch.cuda.current_stream(self.device)):
                buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._bufs[key] = buf
        return buf


class Model:
    @staticmethod
    def dtypes():
        """Arithmetic modes this build of the library accepts (canonical names)."""
        return ("f32w", "f32", "bf16", "f16", "bf16x3", "f16x3", "f16xf8")

    HALF_MODES = ("f16", "f16x3", "f16xf8")        # activations stored as IEEE half: a range of 65504
    HALF_MAX = 65504.0
    # present on every Model, whichever arm built it (and on one no arm has built yet: close(), is_half)
    _h = _seq = _lib_dtype = _canonical = _twin_source = None
    _fc_positions = _fc_hidden = 0

    def __init__(self, state, config, logger, target, dtype: str = "f32w", device=None, range_check: bool = True):
        """dtype: "f32w" (default; fp32 end to end, conv layers as Winograd F(2,3) / F(4,3) on the
        f32-input MFMA), "f32" (fp32, direct lowering: exact fmaf chains), "bf16x3" / "f16x3" (split
        precision on the 16-bit MFMA: hi + lo pairs, three MFMAs per product, fp32 accumulate - the 16-bit mode
        that stays within 1e-3 of the reference), "f16xf8" (f16x3 whose wide layers evaluate the two cross terms of the
        split product as one block-scaled e4m3 product on the 8-bit MFMA: two instruction times per product instead of
        three, within ~3e-4 of the reference), "f16" / "bf16" (plain 16-bit activations and weights, fp32
        accumulate: fast, approximate).  A CNN-RNN (`model: cnn-rnn`) takes "f32w" / "f32" (the same fp32 program) or
        "f16x3": there the split runs on the gate GEMMs whose input is a hidden state (every recurrence and the input
        projection of every layer but the first), whose operands are bounded, so that mode has no range check and
        `saturated()` is always False for it.
        range_check (half-precision modes only): run a small synthetic sample through the new model and REFUSE (ValueError)
        when an activation comes within a factor of 4 of half precision's 65504 - those modes cannot represent larger
        activations, the reference's fp32 path can (riser/model.py:22-28).  RS_RANGE_CHECK=0 or range_check=False skip it;
        at run time `saturated()` (and a warning from `classify`) report an overflow on the real data."""
        self.target, self.logger = target, logger
        self.device = self._get_device(device)
        if logger is not None:
            logger.info('Using %s device', self.device)
        self.model = self            # the reference exposes the nn.Module here; kept as an alias
        self._keep, self._cls_slots, self._cls_next = [], [], 0
        sd = load_state(state)
        kind = select_architecture(config)
        if kind == "cnn-rnn":
            self._init_crnn(sd, config.cnn_rnn, dtype)
        elif kind == "tcn-bot":
            self._init_tcn(sd, config.tcnbot, True, dtype)
        elif kind == "tcn":
            self._init_tcn(sd, config.tcn, False, dtype)
        elif kind == "resnet":
            self._init_resnet(sd, config.resnet, dtype)
        else:
            self._init_cnn(sd, config, dtype)
        if self.is_half and range_check and os.environ.get("RS_RANGE_CHECK", "1") != "0":
            try:
                self._half_range_check()
            except Exception:
                self.close()
                raise

    def _init_cnn(self, sd, config, dtype: str):
        cnn = config.cnn
        self.classifier = getattr(cnn, "classifier", "gap_fc")
        if self.classifier not in ("gap_fc", "gap", "fc"):
            raise ValueError(f"classifier {self.classifier!r}: the reference knows `fc`, `gap_fc` and `gap` "
                             "(riser/nets/cnn.py:21-41)")
        if self.classifier == "gap":
            # Conv1d(C, n_classes, 1) then the mean over positions (riser/nets/cnn.py:34-38) = the mean, then the same
            # matrix: W mean_p(x_p) + b.  Runs as the gap_fc head with the 1 x 1 kernel read as a matrix (fp32 summation
            # order differs from the reference's, ~1e-7 on a probability).
            w0 = np.asarray(sd["classifier.0.weight"])
            if w0.ndim != 3 or w0.shape[2] != 1:
                raise ValueError("classifier.0.weight: expected [n_classes, channels, 1] for the `gap` classifier")
            sd["classifier.2.weight"] = np.ascontiguousarray(w0[:, :, 0])
            sd["classifier.2.bias"] = np.asarray(sd["classifier.0.bias"])
        self.channels = [int(c) for c in cnn.channels][: int(cnn.n_layers)]
        self.n_layers = len(self.channels)
        kernels = [int(k) for k in list(cnn.kernels)[: self.n_layers]]
        shipped = int(getattr(cnn, "depth", 1)) == 1 and all(k == 3 for k in kernels)
        fc = None
        if self.classifier == "fc":
            # Flatten -> Linear(C * P, H) -> ReLU -> Linear(H, n_classes) (riser/nets/cnn.py:22-27; the reference hard-codes
            # C * P = 67 * 753 and H = 4096: one input length of one 4-layer net).  Runs behind the conv stack as two extra
            # kernels (csrc/fc_head.hip); the gap_fc weights the library is created with are placeholders.
            if not shipped or dtype not in ("f32w", "f32"):
                raise ValueError("the `fc` classifier runs behind the depth-1, kernel-3 conv stack in fp32 (dtype f32w / f32)")
            w1 = np.ascontiguousarray(sd["classifier.1.weight"], dtype=np.float32)
            c_last = self.channels[-1]
            if w1.ndim != 2 or w1.shape[1] % c_last != 0:
                raise ValueError(f"classifier.1.weight {w1.shape}: in_features is not a multiple of the last layer's "
                                 f"{c_last} channels")
            fc = (w1, np.ascontiguousarray(sd["classifier.1.bias"], dtype=np.float32),
                  np.ascontiguousarray(sd["classifier.3.weight"], dtype=np.float32),
                  np.ascontiguousarray(sd["classifier.3.bias"], dtype=np.float32))
            if fc[1].shape != (w1.shape[0],) or fc[2].shape != (int(cnn.n_classes), w1.shape[0]) or fc[3].shape != (int(cnn.n_classes),):
                raise ValueError("classifier.1 / classifier.3 shapes do not match each other or n_classes")
            sd["classifier.2.weight"] = np.zeros((int(cnn.n_classes), c_last), dtype=np.float32)
            sd["classifier.2.bias"] = np.zeros(int(cnn.n_classes), dtype=np.float32)
        if not shipped:
            # outside the shipped class (depth > 1 or kernels other than 3, riser/nets/cnn.py:17,52-65).  With the `gap_fc`
            # head: the generic ConvNet family of csrc/gconv.hip (tiled conv + ReLU + pool launches, reads of any length in
            # one call).  RS_GCONV=0 or RS_SEQ_SCALAR=1 in the environment now, and the `gap` head, keep the conv / max-pool
            # program of csrc/seqnet.hip (reads grouped by length)
            if int(cnn.n_classes) != 2:
                raise ValueError("riser_amd supports two-class heads only")
            if any(k % 2 == 0 for k in kernels):
                raise ValueError("riser_amd: even conv kernels ('same' pads them asymmetrically) are not supported")
            family = self.classifier == "gap_fc" and os.environ.get("RS_GCONV", "1") != "0" and "RS_SEQ_SCALAR" not in os.environ
            if dtype not in ("f32w", "f32") and not (family and dtype == "bf16x3"):
                raise ValueError(f"dtype {dtype!r}: configs with depth > 1 or kernels other than 3 run the generic conv "
                                 "program in fp32 ('f32w' / 'f32') or, with the `gap_fc` head on the family of "
                                 "csrc/gconv.hip, in 'bf16x3'")
            if family:
                from .gconv import GConvNet, build_gconv_program
                net = GConvNet(build_gconv_program(sd, cnn), device=self.device, dtype=dtype)
            else:
                from .resnet import SeqNet, build_convnet_program
                net = SeqNet(*build_convnet_program(sd, cnn), device=self.device)      # its default dtype: "f32"
            head = self.classifier
            self._adopt_family(net, self.channels)
            # as this arm always reported: the config's head (`gap` runs as gap_fc above), the reference's minimum length
            self.classifier, self.min_length = head, 1 << self.n_layers
            return
        self.min_length = 1 << self.n_layers
        self.dtype = dtype                    # the caller's spelling; _canonical is what tables are keyed by
        self._canonical = _CANONICAL.get(_DTYPES.get(dtype), dtype)
        conv_w, conv_b = [], []
        c_in = 1
        for i, c_out in enumerate(self.channels):
            w = np.ascontiguousarray(sd[f"layers.{i}.0.weight"], dtype=np.float32)
            b = np.ascontiguousarray(sd[f"layers.{i}.0.bias"], dtype=np.float32)
            if w.shape != (c_out, c_in, 3) or b.shape != (c_out,):
                raise ValueError(f"layers.{i}.0: state dict shape {w.shape} does not match config")
            conv_w.append(w)
            conv_b.append(b)
            c_in = c_out
        fc_w = np.ascontiguousarray(sd["classifier.2.weight"], dtype=np.float32)
        fc_b = np.ascontiguousarray(sd["classifier.2.bias"], dtype=np.float32)
        if fc_w.shape != (int(cnn.n_classes), c_in):
            raise ValueError("classifier.2.weight shape does not match config")
        L = nv.lib()
        wp = (C.c_void_p * self.n_layers)(*[w.ctypes.data for w in conv_w])
        bp = (C.c_void_p * self.n_layers)(*[b.ctypes.data for b in conv_b])
        ch = (C.c_int32 * self.n_layers)(*self.channels)
        h = C.c_void_p()
        nv.check(L.rs_model_create(self.n_layers, ch, int(cnn.n_classes), wp, bp, fc_w.ctypes.data,
                                   fc_b.ctypes.data, _DTYPES[dtype], self.device.index, C.byref(h)),
                 "rs_model_create")
        self._h = h
        self._lib_dtype = _DTYPES[dtype]
        # a half-precision model keeps the host fp32 arrays it was built from (a few MB): fp32_range_twin() needs no file
        self._twin_source = (sd, config) if self.is_half else None
        self._ws = Workspace(self.device)
        if fc is not None:
            w1, b1, w2, b2 = fc
            positions = w1.shape[1] // self.channels[-1]
            nv.check(L.rs_model_set_fc_classifier(h, positions, int(w1.shape[0]), w1.ctypes.data, b1.ctypes.data,
                                                  w2.ctypes.data, b2.ctypes.data), "rs_model_set_fc_classifier")
            self._fc_positions, self._fc_hidden = positions, int(w1.shape[0])

    # ---- half precision's range ----------------------------------------------------------
    @property
    def is_half(self) -> bool:
        """this model runs a library mode that stores activations as IEEE half (a range of 65504) and carries the overflow
        flag: the shipped ConvNet family in f16 / f16x3 / f16xf8, under any spelling of those names.  False for every other
        mode, the generic programs and the CNN-RNN's f16x3 (bounded operands, no flag)."""
        return self._lib_dtype in _HALF_LIB_DTYPES

    def fp32_range_twin(self) -> "Model":
        """A `bf16x3` Model of the same weights, target and device: fp32's exponent range (its saturated() is always False),
        within 1e-3 of the reference, at the speed of the half modes - what the control loop classifies a batch with again
        when this model overflowed (SequencerControl(on_overflow="reclassify")).  Built from the host arrays this model
        kept; the caller owns and closes it."""
        if not self.is_half or self._twin_source is None:
            raise ValueError(f"fp32_range_twin: dtype {self.dtype!r} of target {self.target!r} is not a half-precision mode "
                             "of the shipped ConvNet family - it cannot overflow and has no twin")
        sd, config = self._twin_source
        return Model(sd, config, self.logger, self.target, dtype="bf16x3", device=self.device)

    def half_activation_maxima(self, signals=None) -> list:
        """largest activation (the hi half) of every conv layer i >= 1 of THIS half-precision model on raw int16 `signals`
        (default: 16 synthetic reads of riser_amd.synth; MAD-normalised input is confined to ~[-3.5, 3.5] whatever the
        source), through the library's layer-capture hook.  inf = the layer overflowed."""
        from . import synth
        from .preprocess import pack_reads
        self._need_handle("half_activation_maxima")
        if signals is None:
            signals = [synth.make_raw_read(4242, rid, 2048 + 8615 + 37 * rid, polya=bool(rid % 5))[2048:] for rid in range(16)]
        sig, off, ln, lh = pack_reads(list(signals), self.device)
        out = []
        try:
            for i in range(1, self.n_layers):
                rows, cp, fmt = self.layer_rows(lh, i)
                cap = torch.zeros(rows * cp, dtype=torch.float16, device=self.device)
                with self.capture_layer(i, cap):
                    self.classify_raw(sig, off, ln, lh)
                v = cap.view(rows, cp)
                if fmt == 1:
                    v = v.view(rows, cp // 64, 2, 32)[:, :, 0, :]            # [hi x 32 | lo x 32]
                elif fmt == 2:
                    v = v.view(rows, cp // 128, 2, 64)[:, :, 0, :]           # [hi16 x 64 | e4m3 bytes]
                v = v.float().abs()
                out.append(float("inf") if not torch.isfinite(v).all() else float(v.max().item()))
        finally:
            self.saturated(reset=True)
        return out

    def _half_range_check(self, margin: float = 4.0):
        mx = self.half_activation_maxima()
        worst = max(mx)
        if not worst * margin < self.HALF_MAX:
            layer = 1 + mx.index(worst)
            raise ValueError(
                f"dtype {self.dtype!r} stores activations as IEEE half (largest value 65504): conv layer {layer} of target "
                f"{self.target!r} reaches {worst:.4g} on the synthetic sample, less than x{margin:g} inside that range. Use "
                "'bf16x3' (fp32's exponent range, within 1e-3 of the reference) or 'f32w'; python -m riser_amd.rangecheck "
                "prints every layer's maximum; range_check=False / RS_RANGE_CHECK=0 load the model anyway")

    def saturated(self, reset: bool = True) -> bool:
        """True if a half-precision conversion overflowed (an activation beyond 65504) in any call on this model since the
        flag was last reset; waits for the caller's stream.  Always False for the fp32 / bf16 modes and the generic conv
        programs (fp32's exponent range)."""
        if self._h is None or not self.is_half:
            return False
        rc = nv.lib().rs_model_saturated(self._h, 1 if reset else 0, _stream_ptr(self.device))
        if rc < 0:
            nv.check(rc, "rs_model_saturated")
        return rc == 1

    def warn_if_saturated(self, what: str = "a call") -> bool:
        """`saturated()` turned into a RuntimeWarning (and a logger warning): what classify() does after every call in a
        half-precision mode, and the control loop once per batch"""
        if not self.saturated(reset=True):
            return False
        msg = (f"riser_amd: {what} on target {self.target!r} overflowed half precision (an activation beyond 65504 in dtype "
               f"{self.dtype!r}): the probabilities of the affected reads are WRONG. Use dtype 'bf16x3' or 'f32w' for these weights.")
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
        if self.logger is not None:
            self.logger.warning(msg)
        return True

    # ------------------------------------------------------------------------------------
    def _get_device(self, device=None):
        nv.require_gpu()
        if not torch.cuda.is_available():
            raise nv.NativeError("torch sees no ROCm device")
        if device is None:
            return torch.device("cuda", torch.cuda.current_device())
        d = torch.device(device)
        return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())

    def _adopt_family(self, net, channels):
        """the common end of every family-backed arm: `net` (any FamilyNet) becomes `_seq`, and the
        attributes the entry points read are filled from it"""
        self.classifier, self._fc_positions = "gap_fc", 0
        self.channels, self.n_layers = channels, len(channels)
        self._seq = net
        self.dtype = net.dtype
        self.min_length = net.min_length
        self._ws = Workspace(self.device)

    def _init_resnet(self, sd, rc, dtype: str):
        # `config.resnet` (riser/nets/resnet.py:72-99: channels, kernel, padding, stride, block, n_layers, blocks,
        # n_classes) instead of `config.cnn`: the reference's second architecture.  Its own Model hard-wires ConvNet
        # (riser/model.py:13) and ships no ResNet config or weights; here the same Model surface - classify, the batched
        # entry points, SequencerControl - runs it as a generic conv program (csrc/seqnet.hip: one launch for the stem
        # and one per residual block), in fp32 or, dtype "bf16x3", with stem and basic blocks on the bf16 MFMA.
        from .resnet import SeqNet, build_program
        if int(rc.n_classes) != 2:
            raise ValueError("riser_amd supports two-class heads only")
        seq_dtype = {"f32w": "f32", "f32": "f32", "bf16x3": "bf16x3"}.get(dtype)
        if seq_dtype is None:
            raise ValueError(f"dtype {dtype!r}: a ResNet runs in 'f32w' / 'f32' (f32-input MFMA) or 'bf16x3' (stem and basic "
                             "blocks in split precision on the bf16 MFMA)")
        self._adopt_family(SeqNet(*build_program(sd, rc), device=self.device, dtype=seq_dtype), [int(c) for c in rc.channels])

    def _init_tcn(self, sd, tc, bottleneck: bool, dtype: str):
        # `config.tcnbot` (riser/nets/tcn_bot.py:63-85) or `config.tcn` (riser/nets/tcn.py:62-82), what riser/train.py:175-182
        # trains for `model: tcn-bot` / `tcn`: the receptive cone of the last position (csrc/tcn.hip), behind the same
        # surface as the ResNet above
        from .tcn import TCNNet, build_tcn_program
        if dtype not in ("f32w", "f32", "bf16x3"):
            raise ValueError(f"dtype {dtype!r}: a TCN runs in 'f32w' / 'f32' (fp32 on the f32-input MFMA) or 'bf16x3' (split "
                             "precision on the bf16 MFMA)")
        blocks, fw, fb = build_tcn_program(sd, tc, bottleneck)
        self._adopt_family(TCNNet(blocks, fw, fb, device=self.device, dtype=dtype), [int(tc.n_filters)] * int(tc.n_layers))

    def _init_crnn(self, sd, cc, dtype: str):
        # `config.cnn_rnn` (riser/nets/cnn_rnn.py:7-33, ConvRecNet): conv front + stacked LSTM / GRU (csrc/crnn.hip).
        # The reference's train.py has no branch for it; `model: cnn-rnn`, or a config with a `cnn_rnn` section and
        # neither `model` nor `cnn`, selects it
        from .crnn import CRNNNet, build_crnn_program
        if dtype not in ("f32w", "f32", "f16x3"):
            raise ValueError(f"dtype {dtype!r}: a CNN-RNN runs in 'f32w' / 'f32' (fp32 on the f32-input MFMA) or 'f16x3' "
                             "(split precision on the f16 MFMA for the gate GEMMs of hidden states)")
        prog = build_crnn_program(sd, cc)
        self._adopt_family(CRNNNet(prog, device=self.device, dtype=dtype), [int(cv["w"].shape[0]) for cv in prog["convs"]])

    def close(self):
        h, self._h = self._h, None
        if h:
            nv.lib().rs_model_destroy(h)
        seq, self._seq = self._seq, None
        if seq is not None:
            seq.close()

    def _seq_forward(self, x: torch.Tensor, lens_host: np.ndarray, return_logits: bool, out, lens_dev: torch.Tensor = None):
        """generic program.  A ResNet (stem + residual blocks, all fused) takes the batch as it is - ragged lengths, one call
        (rs_seqnet_forward_ragged: every kernel masks by the read's own rows); any other program runs one uniform length per
        launch, so its reads are grouped by length"""
        B = x.shape[0]
        if self._seq.ragged_ok and x.is_contiguous():
            if lens_dev is None:
                lens_dev = torch.from_numpy(np.ascontiguousarray(lens_host, dtype=np.int32)).to(self.device)
            return self._seq.forward_ragged(x, lens_dev.to(torch.int32), return_logits, out=out)
        probs, logits = _outputs(self.device, (B, 2), out, return_logits)
        for L in np.unique(lens_host):
            idx = torch.from_numpy(np.flatnonzero(lens_host == L)).to(self.device)
            r = self._seq.forward(x[idx, : int(L)].contiguous(), return_logits)
            probs[idx] = r[0] if return_logits else r
            if return_logits:
                logits[idx] = r[1]
        return (probs, logits) if return_logits else probs

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def padded_length(self, lmax: int) -> int:
        if self._seq is not None:
            return int(lmax)
        return nv.lib().rs_padded_length(self._h, int(lmax))

    def block_samples(self, layer: int | None = None) -> int:
        """Block size of the packed activation layout in samples: of the late layers and the head (rs_block_samples), or,
        with `layer`, of the layout conv layer `layer` runs on (the early layers use finer blocks: rs_layer_info)."""
        self._need_handle("block_samples")
        if layer is None:
            return nv.lib().rs_block_samples(self._h)
        return self.layer_info()[layer]["block_samples"]

    def block_bases(self, lens_host, layer: int | None = None) -> np.ndarray:
        """First block of every read of a batch in the packed layout (+ the total as the last entry): read b's rows
        in conv layer i's output start at row bases[b] * (U >> (i + 1)), U = block_samples(i)."""
        U = self.block_samples(layer)
        nblk = np.asarray(lens_host, dtype=np.int64) // U + 1
        return np.concatenate([[0], np.cumsum(nblk)]).astype(np.int64)

    def _need_handle(self, what: str):
        if self._h is None:
            raise NotImplementedError(f"{what}: not available for generic conv programs (depth > 1 / kernels other than 3)")

    def layer_info(self):
        self._need_handle("layer_info")
        out = []
        for i in range(self.n_layers):
            li = nv.LayerInfo()
            nv.check(nv.lib().rs_model_layer_info(self._h, i, C.byref(li)), "rs_model_layer_info")
            out.append({n: getattr(li, n) for n, _ in nv.LayerInfo._fields_})
        return out

    def layer_rows(self, lens_host, layer: int):
        """-> (rows, cp_out, rows_format) of conv layer `layer`'s output buffer for a batch of these lengths: every block of
        the packed layout (block_bases) holds U >> (layer + 1) rows of cp_out padded channels, in the layer's row format
        (rs_layer_info).  What a capture_layer buffer is sized and decoded by."""
        info = self.layer_info()[layer]
        rows = int(self.block_bases(lens_host, layer)[-1]) * (info["block_samples"] >> (layer + 1))
        return rows, info["cp_out"], info["rows_format"]

    @contextlib.contextmanager
    def capture_layer(self, layer: int, buf: torch.Tensor):
        """Inside the block, every call on this model copies conv layer `layer`'s output buffer, as the device laid it out,
        into the device tensor `buf` (any dtype: the library is told its size in bytes and copies no more).  The hook is
        switched off on the way out, whatever happened inside: the library never keeps a pointer to a tensor that may be freed."""
        self._need_handle("capture_layer")
        hook = nv.lib().rs_debug_capture_layer
        nv.check(hook(self._h, int(layer), buf.data_ptr(), buf.numel() * buf.element_size()), "rs_debug_capture_layer")
        try:
            yield buf
        finally:
            if self._h:
                hook(self._h, -1, None, 0)

    def profile(self, on, coarse: bool = False):
        """HIP-event stage timing on the launch stream; coarse = only the conv stack's boundaries (4 events per call)."""
        self._need_handle("profile")
        nv.check(nv.lib().rs_profile_enable(self._h, (2 if coarse else 1) if on else 0), "rs_profile_enable")

    def profile_read(self):
        """-> (stage_ms float32 [n_layers + 2], calls); see rs_profile_read."""
        self._need_handle("profile_read")
        ms = np.zeros(self.n_layers + 2, dtype=np.float32)
        calls = C.c_int32(0)
        nv.check(nv.lib().rs_profile_read(self._h, ms.ctypes.data, C.byref(calls)), "rs_profile_read")
        return ms, calls.value

    def max_batch(self, lmax: int) -> int:
        """Largest batch one library call accepts for reads of up to lmax samples: the conv kernels
        address every activation buffer through a 2 GiB buffer-resource window (32-bit offsets with
        hardware bounds checking).  Bigger batches are split transparently by the methods below."""
        if self._seq is not None:
            return self._seq.max_batch(int(lmax))
        return max(1, nv.lib().rs_max_batch(self._h, int(lmax)))

    # samples (reads x padded length) per library call beyond which a batch is cut into equal sub-batches: throughput is flat
    # from ~1000 reads of 16000 samples on and falls off once a layer's activations outgrow the 256 MB Infinity Cache
    # (profiles/r04_batch_sweep_*.txt: fp32 4096 reads -4 %, split precision 2048 reads -5 %; two bytes more per element there)
    _CALL_SAMPLES = {"f32w": 2048 << 14, "f32": 2048 << 14, "bf16": 2048 << 14, "f16": 2048 << 14,
                     "bf16x3": 1024 << 14, "f16x3": 1024 << 14, "f16xf8": 1024 << 14}

    def call_batch(self, B: int, lmax: int) -> int:
        """Reads per library call for a batch of B reads of up to lmax samples: B itself, or - beyond the 2 GiB buffer
        window (max_batch) or the cache-friendly size - the size of equal sub-batches.  Reads are independent and their
        bits do not depend on their batch-mates, so the cut changes nothing but the time."""
        hard = self.max_batch(lmax)
        cap = hard
        if self._seq is None:
            cap = min(hard, max(512, self._CALL_SAMPLES.get(self._canonical, 2048 << 14) // ((int(lmax) // 1024 + 1) * 1024)))
        if B <= cap or B <= min(hard, cap + cap // 4):          # the cache-friendly size is a preference: no sliver calls
            return B
        n = -(-B // cap)
        # equal shares, rounded up to whole tile rounds of the late layers at 16000-sample reads (a 640-read share is two
        # rounds of tiles for 1.25 rounds of work: 1280 reads run as 768 + 512, not 640 + 640)
        return min(cap, -(-(-(-B // n)) // 256) * 256)

    def reserve(self, B: int, lmax: int):
        """Allocate the workspace of the current stream for batches of up to B reads of up to lmax samples now (a
        growing workspace is a device allocation inside some later call)."""
        if self._h is not None:
            B = max(1, self.call_batch(int(B), lmax))
            self._ws.get(nv.lib().rs_workspace_bytes(self._h, B, int(lmax)))

    def _check_lengths(self, lens_host: np.ndarray):
        if lens_host.size == 0:
            raise ValueError("empty batch")
        if self._fc_positions:
            rows = np.asarray(lens_host, dtype=np.int64) >> self.n_layers
            bad = np.flatnonzero(rows != self._fc_positions)
            if bad.size and int(np.asarray(lens_host).min()) >= self.min_length:
                # what torch raises in the reference's first Linear (riser/nets/cnn.py:24,47) for a read of another length
                c = self.channels[-1]
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied (1x{c * int(rows[bad[0]])} and "
                                   f"{c * self._fc_positions}x{self._fc_hidden})")
        if int(lens_host.min()) < self.min_length:
            # torch raises "max_pool1d() Invalid computed output size: 0" in the reference
            raise ValueError(f"signal of {int(lens_host.min())} samples is shorter than the network "
                             f"minimum {self.min_length}")

    # ------------------------------------------------------------------------------------
    def classify(self, signal):
        """riser/model.py:22-28: normalised signal [L] -> fp32 Tensor[2] on the device."""
        if self.classifier == "gap":
            # the reference cannot classify ONE read with this head: x.squeeze() (riser/nets/cnn.py:48-49) drops the batch
            # dimension and softmax(dim=1) (riser/model.py:27) raises this; the batched entry points below run it
            raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got 1)")
        sig = np.ascontiguousarray(signal)
        if sig.ndim != 1:
            raise ValueError("classify takes ONE normalised signal [L]; classify_batch takes several")
        n = int(sig.shape[0])
        lens = np.array([n], dtype=np.int32)
        if self.device.type != "cuda" or n == 0:
            x = torch.from_numpy(sig).unsqueeze(0).to(self.device, dtype=torch.float)
            return self.forward_batch(x, lens)[0]
        # the reference's loop calls this once per read (riser/control.py:68-69): the signal and its length go to the device
        # through pinned staging slots as asynchronous copies on the caller's stream (a pageable .to() is two blocking copies
        # of ~24 us each that also serialise the host with the previous call's kernels)
        slot = self._classify_slot(n)
        slot["free"].synchronize()                                     # the slot's previous copies have left the host buffer
        slot["x"][:n].copy_(torch.from_numpy(sig))                     # any float dtype / the int64 zeros of mad == 0 -> fp32
        slot["len"][0] = n
        x = torch.empty((1, n), dtype=torch.float32, device=self.device)
        ln = torch.empty((1,), dtype=torch.int32, device=self.device)
        x.copy_(slot["x"][:n].unsqueeze(0), non_blocking=True)
        ln.copy_(slot["len"], non_blocking=True)
        slot["free"].record()
        out = self.forward_batch(x, lens, lens_dev=ln)[0]
        if self.is_half:                           # the reference's fp32 call cannot overflow: say so when this one did
            self.warn_if_saturated("classify()")
        return out

    def _classify_slot(self, n: int):
        """pinned staging for classify(): four slots used in turn, each with an event that says its last copies are done"""
        slots, k = self._cls_slots, self._cls_next
        self._cls_next = (k + 1) & 3
        if len(slots) <= k:
            slots.append({"x": torch.empty(max(n, 16384), dtype=torch.float32).pin_memory(),
                          "len": torch.empty(1, dtype=torch.int32).pin_memory(), "free": torch.cuda.Event()})
        slot = slots[k]
        if slot["x"].numel() < n:
            slot["free"].synchronize()
            slot["x"] = torch.empty(n, dtype=torch.float32).pin_memory()
        return slot

    def classify_batch(self, signals, lengths=None, return_logits: bool = False):
        """Batched classify of already-normalised signals.
        signals: list of 1-D arrays (any float dtype / the int64 zeros of mad == 0), or a
        2-D array / tensor [B, Lmax] with `lengths`.  Returns fp32 [B, 2] on the device."""
        if isinstance(signals, (list, tuple)):
            lens = np.array([len(s) for s in signals], dtype=np.int32)
            self._check_lengths(lens)
            host = np.zeros((len(signals), int(lens.max())), dtype=np.float32)
            for i, s in enumerate(signals):
                host[i, : lens[i]] = np.asarray(s, dtype=np.float32)
            x = torch.from_numpy(host).to(self.device)
        else:
            x = torch.as_tensor(signals).to(self.device, dtype=torch.float)
            if x.dim() != 2:
                raise ValueError("signals must be [B, L]")
            lens = (np.full(x.shape[0], x.shape[1], dtype=np.int32) if lengths is None
                    else np.asarray(lengths, dtype=np.int32))
        return self.forward_batch(x, lens, return_logits=return_logits)

    def forward_batch(self, x: torch.Tensor, lens_host: np.ndarray, lens_dev: torch.Tensor = None,
                      return_logits: bool = False, out: torch.Tensor = None):
        """x: fp32 device tensor [B, ldx] (row b valid for lens[b] samples)."""
        self._check_lengths(lens_host)
        B, ldx = x.shape
        if not x.is_contiguous() or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("x must be a contiguous fp32 tensor on the model's device")
        lmax = int(lens_host.max())
        if lmax > ldx:
            raise ValueError("a length exceeds the row pitch")
        if self._seq is not None:
            return self._seq_forward(x, np.asarray(lens_host), return_logits, out, lens_dev)
        parts = _call_bounds(B, self.call_batch(B, lmax))
        if parts:
            return self._in_parts(parts, B, out, return_logits, lambda s0, s1, o: self.forward_batch(
                x[s0:s1], lens_host[s0:s1], None if lens_dev is None else lens_dev[s0:s1], return_logits, out=o))
        lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
        if lens_dev is None:
            lens_dev = torch.from_numpy(lens_host).to(self.device)
        L = nv.lib()
        ws = self._ws.get(L.rs_workspace_bytes(self._h, B, lmax))
        probs, logits = _outputs(self.device, (B, 2), out, return_logits)
        nv.check(L.rs_forward(self._h, x.data_ptr(), ldx, lens_dev.data_ptr(), lens_host.ctypes.data, B,
                              int(lens_host.min()), lmax, ws.data_ptr(),
                              ws.numel(), probs.data_ptr(), logits.data_ptr() if return_logits else None,
                              _stream_ptr(self.device)), "rs_forward")
        return (probs, logits) if return_logits else probs

    def _in_parts(self, parts, B: int, out, return_logits: bool, call):
        """a batch beyond one library call: call(s0, s1, out=probs[s0:s1]) on each of _call_bounds' parts"""
        probs, logits = _outputs(self.device, (B, 2), out, return_logits)
        for s0, s1 in parts:
            r = call(s0, s1, probs[s0:s1])
            if return_logits:
                logits[s0:s1] = r[1]
        return (probs, logits) if return_logits else probs

    def classify_raw(self, sig_dev: torch.Tensor, off_dev: torch.Tensor, len_dev: torch.Tensor,
                     lens_host: np.ndarray, out: torch.Tensor = None, return_logits: bool = False, packed: bool = True):
        """Fused normalise + forward on raw int16 reads already resident on the device:
        read b = sig_dev[off[b] : off[b] + len[b]].  Returns fp32 [B, 2] on the device.
        packed=False withholds the host's copy of the lengths from the library (every read then takes the blocks of the
        longest one: the layout a caller without host lengths gets; bit-identical results)."""
        self._check_lengths(lens_host)
        B = int(lens_host.shape[0])
        lmax = int(lens_host.max())
        if self._seq is not None:                                      # generic program: normalise, then group by length
            xn = torch.empty((B, lmax), dtype=torch.float32, device=self.device)
            nv.check(nv.lib().rs_normalise(sig_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(), B, lmax,
                                           xn.data_ptr(), lmax, lmax, None, 0, None, _stream_ptr(self.device)),
                     "rs_normalise")
            return self._seq_forward(xn, np.asarray(lens_host), return_logits, out, len_dev)
        parts = _call_bounds(B, self.call_batch(B, lmax))
        if parts:
            return self._in_parts(parts, B, out, return_logits, lambda s0, s1, o: self.classify_raw(
                sig_dev, off_dev[s0:s1], len_dev[s0:s1], lens_host[s0:s1], out=o, return_logits=return_logits, packed=packed))
        L = nv.lib()
        lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
        ws = self._ws.get(L.rs_workspace_bytes(self._h, B, lmax))
        probs, logits = _outputs(self.device, (B, 2), out, return_logits)
        nv.check(L.rs_classify(self._h, sig_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(),
                               lens_host.ctypes.data if packed else None, B, int(lens_host.min()), lmax,
                               ws.data_ptr(), ws.numel(), probs.data_ptr(),
                               logits.data_ptr() if return_logits else None, _stream_ptr(self.device)),
                 "rs_classify")
        return (probs, logits) if return_logits else probs

    def autotune(self, sig_dev: torch.Tensor, off_dev: torch.Tensor, len_dev: torch.Tensor, lens_host: np.ndarray) -> int:
        """Time every feasible tile shape of each tiled conv layer on this batch (rs_autotune) and keep the measured best
        for later batches of the same geometry; returns the number of layers whose choice changed.  Optional: call once per
        deployment batch size (e.g. before a run); results are bit-identical with or without it."""
        self._need_handle("autotune")
        self._check_lengths(lens_host)
        B, lmax = int(lens_host.shape[0]), int(lens_host.max())
        if B > self.max_batch(lmax):
            raise ValueError("autotune: batch exceeds one library call (Model.max_batch)")
        lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
        L = nv.lib()
        ws = self._ws.get(L.rs_workspace_bytes(self._h, B, lmax))
        probs, _ = _outputs(self.device, (B, 2))
        changed = C.c_int32(0)
        nv.check(L.rs_autotune(self._h, sig_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(), lens_host.ctypes.data, B,
                               int(lens_host.min()), lmax, ws.data_ptr(), ws.numel(), probs.data_ptr(), C.byref(changed), _stream_ptr(self.device)),
                 "rs_autotune")
        return changed.value


_CONCURRENT_BELOW_SAMPLES = 1800 * 4096          # csrc/api.hip, rs_classify_ensemble: kConcurrentBelowSamples


def _ensemble_bytes(models, B: int, lmax: int) -> int:
    """workspace of one rs_classify_ensemble call: a pair of activation buffers per model, so that the forwards of the
    models run concurrently (include/riser_amd.h)"""
    hs = (C.c_void_p * len(models))(*[m._h for m in models])
    L = nv.lib()
    serial = max(L.rs_workspace_bytes(m._h, int(B), int(lmax)) for m in models)
    # the library forks the forwards only below ~1800 blocks of 4096 samples (csrc/api.hip, rs_classify_ensemble: beyond that
    # one model's launches fill the chip): a call that can never take the fork needs - and pins - the serial workspace only
    U = int(L.rs_block_samples(models[0]._h))
    if len(models) < 2 or int(B) * (int(lmax) // U + 1) * U >= _CONCURRENT_BELOW_SAMPLES:
        return serial
    need = L.rs_ensemble_workspace_bytes(hs, len(models), int(B), int(lmax))
    return need if need else serial       # 0: models that cannot run concurrently (an `fc` classifier)


def reserve_ensemble(models, B: int, lmax: int):
    """The workspace classify_raw_ensemble will ask for (it lives with models[0]), allocated ahead of the run."""
    m0 = models[0]
    if any(m._h is None for m in models):
        return
    B = max(1, min(m.call_batch(int(B), lmax) for m in models))
    m0._ws.get(_ensemble_bytes(models, B, lmax))


def reserve_ensemble_sets(model_lists, B: int, lmax: int):
    """reserve_ensemble for several model lists of the same length that one caller alternates between (the control loop's
    models, and the same list with overflowed half-precision models replaced by their fp32-range twins): the largest
    workspace any of the lists - or any mix of their members - asks for, on the first model of each, so that whichever list a
    call takes finds it allocated.  (A mix's widest activation buffer is that of one of the lists.)"""
    lists = [list(ms) for ms in model_lists]
    if any(m._h is None for ms in lists for m in ms):         # a generic program among them: one classify_raw per model
        for m in {id(m): m for ms in lists for m in ms}.values():
            m.reserve(B, lmax)
        return
    b = max(1, max(min(m.call_batch(int(B), lmax) for m in ms) for ms in lists))
    need = max(_ensemble_bytes(ms, b, lmax) for ms in lists)
    for m0 in {id(ms[0]): ms[0] for ms in lists}.values():
        m0._ws.get(need)


def classify_raw_ensemble(models, sig_dev: torch.Tensor, off_dev: torch.Tensor, len_dev: torch.Tensor,
                          lens_host: np.ndarray, out: torch.Tensor = None, decision: torch.Tensor = None,
                          max_len: int = 0, threshold: float = 0.9, mode: int = nv.RS_ENRICH):
    """The model loop of riser/control.py:63-82 for a whole batch in ONE library call: raw int16 reads on
    the device are normalised once, every model (same architecture) classifies them, and - when a uint8
    `decision` tensor [B] is given - the accept / reject / try-again decision is taken on the device.
    Returns fp32 probabilities [n_models, B, 2] on the device."""
    m0 = models[0]
    m0._check_lengths(lens_host)
    B, lmax = int(lens_host.shape[0]), int(lens_host.max())
    lens_host = np.ascontiguousarray(lens_host, dtype=np.int32)
    probs, _ = _outputs(m0.device, (len(models), B, 2), out)
    if any(m._h is None for m in models):
        # a generic conv program (depth > 1 / kernels other than 3) among the models: one classify_raw per model and
        # the decision kernel on their probabilities - the same arithmetic, just not one library call
        for k, m in enumerate(models):
            m.classify_raw(sig_dev, off_dev, len_dev, lens_host, out=probs[k])
        if decision is not None:
            nv.check(nv.lib().rs_decide(probs.data_ptr(), len(models), B, len_dev.data_ptr(), int(max_len), float(threshold),
                                        int(mode), decision.data_ptr(), _stream_ptr(m0.device)), "rs_decide")
        return probs
    parts = _call_bounds(B, min(m.call_batch(B, lmax) for m in models))
    if parts:
        for s0, s1 in parts:
            probs[:, s0:s1] = classify_raw_ensemble(models, sig_dev, off_dev[s0:s1].contiguous(), len_dev[s0:s1].contiguous(),
                                                    lens_host[s0:s1], decision=None if decision is None else decision[s0:s1],
                                                    max_len=max_len, threshold=threshold, mode=mode)
        return probs
    L = nv.lib()
    ws = m0._ws.get(_ensemble_bytes(models, B, lmax))
    hs = (C.c_void_p * len(models))(*[m._h for m in models])
    nv.check(L.rs_classify_ensemble(hs, len(models), sig_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(),
                                    lens_host.ctypes.data, B, int(lens_host.min()), lmax, ws.data_ptr(), ws.numel(), probs.data_ptr(),
                                    decision.data_ptr() if decision is not None else None, int(max_len),
                                    float(threshold), int(mode), _stream_ptr(m0.device)), "rs_classify_ensemble")
    return probs
