"""numpy emulation of the CNN-RNN's f16x3 mode (csrc/crnn/x3.hpp): crnn_ref's ragged forward with the gate GEMMs whose input
is a hidden state - every recurrence h W_hh^T and the input projection of every layer but the first - replaced by

    x3_matmul_f16(a, w) = (hi(a') hi(w')^T + lo(a') hi(w')^T + hi(a') lo(w')^T) / (1024 s)

on np.float16 halves: a' = fp32(a) * 1024, w' = w * s with s the packer's power of two (max |w'| in [2^13, 2^14)),
hi(v) = f16(v), lo(v) = f16(v - hi(v)) with the subtraction in fp32.  np.float16 rounds to nearest even and keeps subnormals,
as the device's conversion does.  The PRODUCTS AND SUMS ARE FLOAT64 (the device accumulates in fp32 on the MFMA, in an order
over a 32-wide k-block that is the hardware's own): the emulation isolates what the split loses, and the device bar is ten
times its gap.  Everything else is float64, as crnn_ref does it.

    forward_ragged(prog, reads)                  logits [N, 2] float64
    forward_ragged(prog, reads, mutant=name)     name in MUTANTS: defects of a split-precision program, and two variants
"""
import numpy as np

from tests import crnn_ref

H_SCALE = 1024.0

# the four defects a device program could have; each must miss the device bar
DEFECTS = ("hi_lo_dropped", "lo_hi_dropped", "lo_wrong_sign", "scale_kept_on_one_gate")
# "plain_f16": no lo halves at all (what the split buys); "first_proj_split": the first layer's projection ALSO split - still
# inside the bar on these weights: the scope line of the mode is about range (conv outputs are unbounded), not accuracy
MUTANTS = DEFECTS + ("plain_f16", "first_proj_split")


def weight_scale(w) -> float:
    """the packer's exact power-of-two scale of one weight matrix: max |w s| in [2^13, 2^14)"""
    mx = float(np.abs(w).max()) if w.size else 0.0
    if mx == 0.0:
        return 1.0
    _, ex = np.frexp(np.float32(mx))
    return float(2.0 ** min(14 - int(ex), 110))


def split_f16(v, wrong_sign=False):
    """fp32 array -> (hi, lo) as float64 arrays holding f16 values"""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    sub = hi.astype(np.float32) - v if wrong_sign else v - hi.astype(np.float32)
    return hi.astype(np.float64), sub.astype(np.float16).astype(np.float64)


class X3Weights:
    """one gate matrix w [G, K] as the device holds it"""

    def __init__(self, w, mutant=None, a_scale=H_SCALE):
        w = np.asarray(w, dtype=np.float32)
        self.s = weight_scale(w)
        self.mutant = mutant
        self.a_scale = np.float32(a_scale)
        self.hi, self.lo = split_f16(w * np.float32(self.s), mutant == "lo_wrong_sign")

    def matmul(self, a, gates=1):
        """a [.., K] (float64 holding the layer's fp32 input) -> a w^T [.., G] float64"""
        ah, al = split_f16(np.asarray(a, dtype=np.float32) * self.a_scale, self.mutant == "lo_wrong_sign")
        out = ah @ self.hi.T
        if self.mutant != "plain_f16":
            if self.mutant != "lo_hi_dropped":
                out = out + al @ self.hi.T
            if self.mutant != "hi_lo_dropped":
                out = out + ah @ self.lo.T
        inv = np.full(out.shape[-1], 1.0 / (self.s * float(self.a_scale)))
        if self.mutant == "scale_kept_on_one_gate":                  # gate 1 (LSTM f, GRU z) keeps the weight scale
            G = out.shape[-1] // gates
            inv[G:2 * G] *= self.s
        return out * inv


def x3_matmul_f16(a, w, mutant=None, gates=1, a_scale=H_SCALE):
    """a [.., K] times w [G, K]^T in the mode's arithmetic (see the module docstring)"""
    return X3Weights(w, mutant, a_scale).matmul(a, gates)


def plain_matmul_f16(a, w):
    return x3_matmul_f16(a, w, mutant="plain_f16")


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward_ragged(prog, reads, mutant=None):
    """crnn_ref.forward_ragged with the scoped GEMMs in f16x3 arithmetic"""
    assert mutant is None or mutant in MUTANTS, mutant
    feats = [crnn_ref.conv_front(prog, np.asarray(r)[None])[0] for r in reads]
    T = np.array([f.shape[0] for f in feats])
    N, Tm = len(reads), int(T.max())
    h = np.zeros((N, Tm, feats[0].shape[1]))
    for i, f in enumerate(feats):
        h[i, Tm - T[i]:] = f
    layers = prog["layers"]
    for li, lay in enumerate(layers):
        last = li == len(layers) - 1
        H = lay["hidden"]
        ng = 4 if lay["cell"] == "lstm" else 3
        outs = []
        for d in range(2 if lay["bidirectional"] else 1):
            bih, bhh = lay["b_ih"][d].astype(np.float64), lay["b_hh"][d].astype(np.float64)
            whh = X3Weights(lay["w_hh"][d], mutant)
            if d == 1:
                x = np.zeros_like(h)
                for i in range(N):
                    x[i, Tm - T[i]:] = h[i, Tm - T[i]:][::-1]
            else:
                x = h
            if li > 0:
                xp = X3Weights(lay["w_ih"][d], mutant).matmul(x, ng) + bih
            elif mutant == "first_proj_split":               # conv outputs are not bounded by 1: no activation scale
                xp = X3Weights(lay["w_ih"][d], None, a_scale=1.0).matmul(x, ng) + bih
            else:
                xp = x @ lay["w_ih"][d].astype(np.float64).T + bih
            hs, cs = np.zeros((N, H)), np.zeros((N, H))
            o = np.zeros((N, Tm, H))
            steps = range(Tm - 1, Tm) if (last and d == 1) else range(Tm)
            for s in steps:
                live = (s >= Tm - T)[:, None]
                g = np.stack([xp[i, Tm - T[i]] for i in range(N)]) if (last and d == 1) else xp[:, s]
                hh = whh.matmul(hs, ng)
                if lay["cell"] == "lstm":
                    g = g + hh + bhh
                    i_, f_, g_, o_ = (g[:, j * H:(j + 1) * H] for j in range(4))
                    c2 = _sig(f_) * cs + _sig(i_) * np.tanh(g_)
                    h2 = _sig(o_) * np.tanh(c2)
                else:
                    r = _sig(g[:, :H] + hh[:, :H] + bhh[:H])
                    z = _sig(g[:, H:2 * H] + hh[:, H:2 * H] + bhh[H:2 * H])
                    n = np.tanh(g[:, 2 * H:] + r * (hh[:, 2 * H:] + bhh[2 * H:]))
                    h2, c2 = (1.0 - z) * n + z * hs, cs
                hs, cs = np.where(live, h2, hs), np.where(live, c2, cs)
                o[:, s] = hs
            o[np.arange(Tm)[None, :] < (Tm - T)[:, None]] = 0.0
            if d == 1 and not last:
                for i in range(N):
                    o[i, Tm - T[i]:] = o[i, Tm - T[i]:][::-1].copy()
            outs.append(o)
        h = np.concatenate(outs, axis=2)
        if lay["relu_after"]:
            h = np.maximum(h, 0.0)
    return h[:, -1, :] @ prog["fc_w"].astype(np.float64).T + prog["fc_b"].astype(np.float64)


def forward(prog, x, mutant=None):
    """reads x [B, L] of one length"""
    return forward_ragged(prog, list(np.asarray(x)), mutant)
