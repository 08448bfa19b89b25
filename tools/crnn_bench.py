#!/usr/bin/env python3
"""CNN-RNN (riser/nets/cnn_rnn.py, ConvRecNet) on csrc/crnn.hip: ms per call and reads/s for uniform 512 x 16000 and 512 x 4000
batches, the 357 x 8615 live shape with ragged lengths, and 1 / 16 / 64 reads; the forward alone (normalised input on the
device) and classify_raw (int16 reads: normalise + forward); program_macs per read and the MAC rate against the 157 TF f32
MFMA peak; the recurrent steps T of the longest read.  Nets: synth.CRNN_BENCH_CFG (4 conv layers 32/64/128/128, k 9/7/5/3,
2 x 2 bidirectional LSTM layers of 128) and its GRU twin.
    python tools/crnn_bench.py [steps] [--only LABEL] [--cell lstm|gru|both]
--only runs one shape (for a profiler run of its own)."""
import json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from riser_amd import crnn as R
from riser_amd import synth
from riser_amd.model import Model
from riser_amd.preprocess import pack_reads

PEAK_TF = 157.3
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


def run(steps=5, only=None, cells=("lstm", "gru")):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    pool = synth.make_signals(20260103, 64, 16000)
    out = {}
    for cell in cells:
        cfg = synth.CRNN_BENCH_CFG if cell == "lstm" else synth.CRNN_GRU_BENCH_CFG
        sd = synth.make_crnn_state_dict(11, cfg)
        ns = types.SimpleNamespace(**cfg)
        m = Model(sd, types.SimpleNamespace(model="cnn-rnn", cnn_rnn=ns), None, "x", device=dev)
        prog = R.build_crnn_program(sd, ns)
        res = {"min_length": m.min_length, "layers": len(prog["layers"])}
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
            ms_fwd = _time(lambda: m.forward_batch(x, lh, lens_dev=ln), steps, dev)
            ms_raw = _time(lambda: m.classify_raw(sig, off, ln, lh), steps, dev)
            res[label] = dict(ms_forward=round(ms_fwd, 3), ms_classify_raw=round(ms_raw, 3),
                              reads_per_s=round(B / (ms_raw * 1e-3), 1), steps_T=R.steps(prog, L),
                              gmac_per_read=round(macs / B / 1e9, 4),
                              tflops_forward=round(2 * macs / (ms_fwd * 1e-3) / 1e12, 3),
                              frac_of_f32_mfma_peak=round(2 * macs / (ms_fwd * 1e-3) / 1e12 / PEAK_TF, 4))
        m.close()
        out[cell] = res
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[s[0] for s in SHAPES])
    ap.add_argument("--cell", choices=("lstm", "gru", "both"), default="both")
    args = ap.parse_args()
    print(json.dumps(run(args.steps, args.only, ("lstm", "gru") if args.cell == "both" else (args.cell,))))
