#!/usr/bin/env python3
"""TCN / TCNBot (riser/nets/tcn.py, tcn_bot.py) on the receptive-cone program (csrc/tcn.hip; bf16x3: csrc/tcn_x3.hip): ms per
call and reads/s for uniform 512 x 16000 and 512 x 4000 batches, the 357 x 8615 live shape with ragged lengths, and 1 / 16 / 64
reads; the forward alone (normalised input on the device) and classify_raw (int16 reads: normalise + forward); the MAC rate
(for fp32 also against the 157 TF f32 MFMA peak).  Config: 8 blocks, 64 filters, k 3, base 2 (synth.TCN_BENCH_CFG) and its
TCNBot twin.
    python tools/tcn_bench.py [steps] [--dtype f32|bf16x3|both]
--dtype both times the two modes interleaved, shape by shape, in one process (each figure the faster of two alternating
passes): {"tcn": {"receptive_field": .., "512x16000": {"f32": {..}, "bf16x3": {..}}, ..}, "tcnbot": ..}.  With one dtype the
line has the single-mode layout: {"tcn": {"receptive_field": .., "512x16000": {..}, ..}, ..}."""
import json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from riser_amd import synth
from riser_amd import tcn as T
from riser_amd.model import Model
from riser_amd.preprocess import pack_reads

PEAK_TF = 157.3


def _time(fn, steps, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1) / steps


def run(steps=20, dtype="f32"):
    dev = torch.device("cuda", 0)
    dtypes = ["f32", "bf16x3"] if dtype == "both" else [dtype]
    passes = 2 if len(dtypes) > 1 else 1
    rng = np.random.default_rng(5)
    pool = synth.make_signals(20260103, 64, 16000)
    shapes = [("512x16000", 512, 16000, False), ("512x4000", 512, 4000, False), ("357x8615_ragged", 357, 8615, True),
              ("1x16000", 1, 16000, False), ("16x16000", 16, 16000, False), ("64x16000", 64, 16000, False)]
    out = {}
    for bot in (False, True):
        cfg = dict(synth.TCN_BENCH_CFG)
        name = "tcnbot" if bot else "tcn"
        sd = synth.make_tcn_state_dict(11, cfg, bot)
        ns = types.SimpleNamespace(**cfg)
        config = types.SimpleNamespace(model="tcn-bot" if bot else "tcn", **{"tcnbot" if bot else "tcn": ns})
        models = {dt: Model(sd, config, None, "x", dtype=dt, device=dev) for dt in dtypes}
        blocks, _, _ = T.build_tcn_program(sd, ns, bot)
        res = {"receptive_field": T.receptive_field(blocks)}
        for label, B, L, ragged in shapes:
            lens = rng.integers(1000, L + 1, B) if ragged else np.full(B, L)
            lens[0] = L
            sigs = [pool[i % 64][: int(n)] for i, n in enumerate(lens)]
            sig, off, ln, lh = pack_reads(sigs, dev)
            x = torch.zeros((B, L), dtype=torch.float32, device=dev)
            for i, s in enumerate(sigs):
                x[i, : len(s)] = torch.from_numpy(np.clip((s.astype(np.float32) - 500.0) / 60.0, -3.5, 3.5))
            lh = np.asarray(lh, dtype=np.int32)
            macs = sum(T.program_macs(blocks, int(n)) for n in lens)
            best = {dt: [float("inf"), float("inf")] for dt in dtypes}
            for _ in range(passes):
                for dt in dtypes:
                    m = models[dt]
                    ms_fwd = _time(lambda: m.forward_batch(x, lh, lens_dev=ln), steps, dev)
                    ms_raw = _time(lambda: m.classify_raw(sig, off, ln, lh), steps, dev)
                    best[dt] = [min(best[dt][0], ms_fwd), min(best[dt][1], ms_raw)]
            row = {}
            for dt in dtypes:
                ms_fwd, ms_raw = best[dt]
                r = dict(ms_forward=round(ms_fwd, 4), ms_classify_raw=round(ms_raw, 4),
                         reads_per_s=round(B / (ms_raw * 1e-3), 1), mmac_per_read=round(macs / B / 1e6, 2),
                         tflops_forward=round(2 * macs / (ms_fwd * 1e-3) / 1e12, 3))
                if dt == "f32":
                    r["frac_of_f32_mfma_peak"] = round(2 * macs / (ms_fwd * 1e-3) / 1e12 / PEAK_TF, 4)
                row[dt] = r
            res[label] = row if len(dtypes) > 1 else row[dtypes[0]]
        for m in models.values():
            m.close()
        out[name] = res
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("--dtype", choices=("f32", "bf16x3", "both"), default="f32")
    args = ap.parse_args()
    print(json.dumps(run(args.steps, args.dtype)))
