"""Layer by layer: the buffers of an f16xf8 model (F8 rows decoded: hi16 + lo8 x scale, and hi8 x scale against hi16) against
those of an f16x3 model on the same reads.  python tools/f8_debug.py [n_reads] [length]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from riser_amd import synth
from riser_amd.model import Model
from riser_amd.preprocess import pack_reads
from tests import h16_ref as H

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
L = int(sys.argv[2]) if len(sys.argv) > 2 else 16000
dev = torch.device("cuda", 0)
sigs = synth.make_signals(20260103, B, L)
sig, off, ln, lens = pack_reads(list(sigs), dev)


models = {dt: Model(synth.make_state_dict(1), synth.Config(), None, "m", dtype=dt, device=dev) for dt in ("f16x3", "f16xf8")}
info = {dt: m.layer_info() for dt, m in models.items()}
n_layers = models["f16x3"].n_layers
for i in range(3, n_layers):
    out = {}
    for dt, m in models.items():
        rows, cp, _ = m.layer_rows(lens, i)
        cap = torch.zeros(rows * cp * 2 + 256 + (cp // 64) * (rows + 4) * 4 + 1024, dtype=torch.uint8, device=dev)
        with m.capture_layer(i, cap):
            p = m.classify_raw(sig, off, ln, lens).cpu().numpy()
        out[dt] = (cap.cpu().numpy(), rows, cp, p)
    C = info["f16x3"][i]["c_out"]
    raw, rows, cp, p3 = out["f16x3"]
    hi3, lo3 = H.decode_split(raw, rows, cp, C, "f16x3")
    v3 = hi3 + lo3
    raw, rows8, cp8, p8 = out["f16xf8"]
    assert rows8 == rows
    f8rows = cp8 != cp or (i + 1 < n_layers and info["f16xf8"][i]["cp_out"] % 128 == 0 and cp8 == 128 * ((C + 63) // 64) and i >= 4 and i < n_layers - 1)
    scale = np.abs(v3).max()
    if f8rows:
        hi, lo8, hi8, sc = H.decode_f8(raw, rows, cp8, C)
        v8 = hi + lo8
        Cp = (C + 31) // 32 * 32
        def blkmax(x):
            xp = np.zeros((x.shape[0], Cp)); xp[:, :C] = np.abs(x)
            return np.repeat(xp.reshape(x.shape[0], Cp // 32, 32).max(axis=2), 32, axis=1)[:, :C]
        bm = np.maximum(blkmax(hi), 1e-30)
        print("          hi8 - hi16 over block max: %.3e (expect <= 2^-5 = 3.1e-2)   lo8 - (v3 - hi) over block max 2^-11: %.3e" % (
            (np.abs(hi8 - hi) / bm).max(), (np.abs(lo8 - (v3 - hi)) / (bm * 2.0 ** -11)).max()))
        print("layer %2d F8 rows cp %d: max|v - v(f16x3)| / max %.2e   hi16 vs f16x3 hi %.2e   hi8 vs hi16 rel %.2e   lo8 vs exact lo (of ulp) %.2e   scale bytes %d..%d" % (
            i, cp8, np.abs(v8 - v3).max() / scale, np.abs(hi - hi3).max() / scale, (np.abs(hi8 - hi) / np.maximum(np.abs(hi), 1e-30)).max(),
            (np.abs(lo8 - (v3 - hi)) / np.maximum(np.abs(hi) * 2.0 ** -11, 1e-30)).max(), sc.min(), sc.max()))
    else:
        hi, lo = H.decode_split(raw, rows, cp8, C, "f16x3")
        print("layer %2d x3 rows: max|v - v(f16x3)| / max %.2e" % (i, np.abs(hi + lo - v3).max() / scale))
    print("          max |dp| %.2e" % np.abs(p8 - p3).max())
