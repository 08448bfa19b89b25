"""FamilyNet: what the device programs behind Model share on the Python side (TCNNet, CRNNNet, GConvNet, SeqNet).

A family is a set of C entry points rs_<family>_{create, destroy, set_mode, max_batch, workspace_bytes, forward_ragged}
(include/riser_amd.h).  The base class owns the handle (`_h`), the workspace (`_ws`) and the host arrays the handle was
made from (`_keep`), and the calls that differ by that prefix only.  A subclass names its prefix and its modes, marshals
its program into rs_<family>_create (`_create`), words its own refusals, and adds its extras.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as nv


def load_state(state) -> dict:
    """a state dict, or the path of one, as {name: numpy array} on the host; arrays that already are numpy are kept as they are"""
    sd = state if isinstance(state, dict) else torch.load(state, map_location="cpu")              # riser/model.py:19
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}


class FamilyNet:
    _PREFIX = None              # "rs_tcn", ...
    _MODES = {}                 # dtype name -> (canonical name, RS_* code of rs_<family>_set_mode)

    ragged_ok = True

    def __init__(self, keep, device, dtype: str = "f32"):
        mode = self._mode(dtype)[0]                 # a refused dtype: before any GPU call
        nv.require_gpu()
        d = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        self._keep = keep
        self._ws = None
        self.dtype = "f32"
        self._h = self._create()
        if mode != "f32":
            try:
                self.set_mode(dtype)
            except Exception:
                self.close()
                raise

    def _create(self):
        """marshal self._keep into rs_<family>_create on self.device; returns the handle"""
        raise NotImplementedError

    @classmethod
    def _refused_dtype(cls, dtype) -> str:
        """the ValueError text for a dtype outside _MODES"""
        raise NotImplementedError

    def _no_workspace(self, B: int, ld: int) -> str:
        """the ValueError text where rs_<family>_workspace_bytes answers 0 for a live handle"""
        return f"no workspace for {B} reads of {ld} samples"

    @classmethod
    def _mode(cls, dtype):
        mode = cls._MODES.get(dtype)
        if mode is None:
            raise ValueError(cls._refused_dtype(dtype))
        return mode

    def _fn(self, name: str):
        return getattr(nv.lib(), f"{self._PREFIX}_{name}")

    def set_mode(self, dtype: str):
        """the arithmetic of the next forward (rs_<family>_set_mode); a refused dtype leaves the mode as it was"""
        mode, code = self._mode(dtype)
        nv.check(self._fn("set_mode")(self._h, code), f"{self._PREFIX}_set_mode")
        self.dtype = mode

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        self._ws = None
        if h:
            self._fn("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def max_batch(self, L: int) -> int:
        """largest batch of reads of (pitch) L samples one call can address: every activation buffer inside the 2 GiB
        window (rs_<family>_max_batch); forward_ragged splits bigger batches"""
        return max(1, int(self._fn("max_batch")(self._h, int(L))))

    def _workspace(self, B: int, ld: int, refusal) -> torch.Tensor:
        """the workspace of one call, grown where it is too small (the old one is dropped first).  A closed net gets an empty
        one: the call that follows is refused by the library's null-handle check."""
        need = self._fn("workspace_bytes")(self._h, B, ld)
        if need == 0 and self._h:
            raise ValueError(refusal(B, ld))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def forward(self, x: torch.Tensor, return_logits: bool = False):
        """x: fp32 device tensor [B, L] (one common length) -> fp32 [B, 2] on the device."""
        B, L = x.shape
        lens = torch.full((B,), L, dtype=torch.int32, device=self.device)
        return self.forward_ragged(x, lens, return_logits)

    def forward_ragged(self, x: torch.Tensor, lens_dev: torch.Tensor, return_logits: bool = False, out: torch.Tensor = None):
        """x: fp32 device tensor [B, ld], read b = x[b, :lens_dev[b]] (int32 on the device) -> fp32 [B, 2] on the device;
        every read's result is that of forward() on it alone, bit for bit."""
        B, ld = x.shape
        if not x.is_contiguous():                   # the device reads row b at x + b * ld
            raise ValueError("x must be contiguous: its row pitch is its second dimension")
        probs = out if out is not None else torch.empty((B, 2), dtype=torch.float32, device=self.device)
        logits = torch.empty((B, 2), dtype=torch.float32, device=self.device) if return_logits else None
        mb = self.max_batch(ld)
        if B > mb:                                  # reads are independent: equal parts, each inside the buffer window
            parts = -(-B // mb)
            step = -(-B // parts)
            for s0 in range(0, B, step):
                s1 = min(B, s0 + step)
                r = self.forward_ragged(x[s0:s1], lens_dev[s0:s1], return_logits, out=probs[s0:s1])
                if return_logits:
                    logits[s0:s1] = r[1]
            return (probs, logits) if return_logits else probs
        ws = self._workspace(B, ld, self._no_workspace)
        nv.check(self._fn("forward_ragged")(self._h, x.data_ptr(), lens_dev.data_ptr(), B, ld, ws.data_ptr(), ws.numel(),
                                            probs.data_ptr(), logits.data_ptr() if return_logits else None,
                                            torch.cuda.current_stream(self.device).cuda_stream),
                 f"{self._PREFIX}_forward_ragged")
        return (probs, logits) if return_logits else probs
