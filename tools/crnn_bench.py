#!/usr/bin/env python3
"""CNN-RNN (riser/nets/cnn_rnn.py, ConvRecNet) on csrc/crnn.hip: ms per call and reads/s for uniform 512 x 16000 and 512 x 4000
batches, the 357 x 8615 live shape with ragged lengths, and 1 / 16 / 64 reads; the forward alone (normalised input on the
device) and classify_raw (int16 reads: normalise + forward); program_macs per read and the MAC rate against the 157 TF f32
MFMA peak; the recurrent steps T of the longest read.  Nets: synth.CRNN_BENCH_CFG (4 conv layers 32/64/128/128, k 9/7/5/3,
2 x 2 bidirectional LSTM layers of 128) and its GRU twin.
    python tools/crnn_bench.py [steps] [--only LABEL] [--cell lstm|gru|both] [--dtype f32|f16x3|both]
--only runs one shape (for a profiler run of its own).  --dtype both builds the fp32 and the f16x3 model in ONE process and
times them shape by shape, interleaved; the f16x3 entries also carry the MAC rate of the split-precision parts (every
recurrence, the input projection of every layer but the first) against a third of the f16 MFMA peak, at the whole call's
time (an under-estimate: the fp32 parts run in that time too)."""
import json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from riser_amd import crnn as R
from riser_amd import synth
from riser_amd.model import Model
from riser_amd.preprocess import pack_reads

PEAK_TF = 157.3
PEAK_F16_TF = 2516.6                                 # dense f16 MFMA peak; a split product is three MFMAs
SHAPES = [("512x16000", 512, 16000, False), ("512x4000", 512, 4000, False), ("357x8615_ragged", 357, 8615, True),
          ("1x16000", 1, 16000, False), ("16x16000", 16, 16000, False), ("64x16000", 64, 16000, False)]


def _time(fn, steps, dev):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1) / steps


def x3_macs(prog, L: int) -> int:
    """multiply-adds of one read that the f16x3 mode runs in split precision"""
    T = R.steps(prog, L)
    total = 0
    for n, lay in enumerate(prog["layers"]):
        g = R.GATES[lay["cell"]] * lay["hidden"]
        per = g * (lay["hidden"] + (lay["in_dim"] if n > 0 else 0))
        for d in range(2 if lay["bidirectional"] else 1):
            total += (1 if (d == 1 and n == len(prog["layers"]) - 1) else T) * per
    return int(total)


def run(steps=5, only=None, cells=("lstm", "gru"), dtypes=("f32",)):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    pool = synth.make_signals(20260103, 64, 16000)
    out = {}
    for cell in cells:
        cfg = synth.CRNN_BENCH_CFG if cell == "lstm" else synth.CRNN_GRU_BENCH_CFG
        sd = synth.make_crnn_state_dict(11, cfg)
        ns = types.SimpleNamespace(**cfg)
        models = {dt: Model(sd, types.SimpleNamespace(model="cnn-rnn", cnn_rnn=ns), None, "x", dtype=dt, device=dev)
                  for dt in dtypes}
        prog = R.build_crnn_program(sd, ns)
        res = {"min_length": models[dtypes[0]].min_length, "layers": len(prog["layers"])}
        for label, B, L, ragged in SHAPES:
            if only and label != only:
                continue
            lens = rng.integers(1000, L + 1, B) if ragged else np.full(B, L)
            lens[0] = L
            sigs = [pool[i % 64][: int(n)] for i, n in enumerate(lens)]
            sig, off, ln, lh = pack_reads(sigs, dev)
            x = torch.zeros((B, L), dtype=torch.float32, device=dev)
            for i, s in enumerate(sigs):
                x[i, : len(s)] = torch.from_numpy(np.clip((s.astype(np.float32) - 500.0) / 60.0, -3.5, 3.5))
            lh = np.asarray(lh, dtype=np.int32)
            macs = sum(R.program_macs(prog, int(n)) for n in lens)
            macs3 = sum(x3_macs(prog, int(n)) for n in lens)
            for dt, m in models.items():
                ms_fwd = _time(lambda: m.forward_batch(x, lh, lens_dev=ln), steps, dev)
                ms_raw = _time(lambda: m.classify_raw(sig, off, ln, lh), steps, dev)
                r = dict(ms_forward=round(ms_fwd, 3), ms_classify_raw=round(ms_raw, 3),
                         reads_per_s=round(B / (ms_raw * 1e-3), 1), steps_T=R.steps(prog, L),
                         gmac_per_read=round(macs / B / 1e9, 4),
                         tflops_forward=round(2 * macs / (ms_fwd * 1e-3) / 1e12, 3),
                         frac_of_f32_mfma_peak=round(2 * macs / (ms_fwd * 1e-3) / 1e12 / PEAK_TF, 4))
                if dt == "f16x3":
                    r["x3_gmac_per_read"] = round(macs3 / B / 1e9, 4)
                    r["x3_frac_of_f16_mfma_peak_over_3"] = round(2 * macs3 / (ms_fwd * 1e-3) / 1e12 / (PEAK_F16_TF / 3), 5)
                res[label if len(dtypes) == 1 else f"{label}:{dt}"] = r
            if len(dtypes) == 2:
                a, b = res[f"{label}:{dtypes[0]}"], res[f"{label}:{dtypes[1]}"]
                res[f"{label}:{dtypes[0]}/{dtypes[1]}"] = round(a["ms_forward"] / b["ms_forward"], 3)
        for m in models.values():
            m.close()
        out[cell] = res
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[s[0] for s in SHAPES])
    ap.add_argument("--cell", choices=("lstm", "gru", "both"), default="both")
    ap.add_argument("--dtype", choices=("f32", "f16x3", "both"), default="f32")
    args = ap.parse_args()
    print(json.dumps(run(args.steps, args.only, ("lstm", "gru") if args.cell == "both" else (args.cell,),
                         ("f32", "f16x3") if args.dtype == "both" else (args.dtype,))))
