#!/usr/bin/env python3
"""TCN / TCNBot (riser/nets/tcn.py, tcn_bot.py) on the receptive-cone program (csrc/tcn.hip): ms per call and reads/s for
uniform 512 x 16000 and 512 x 4000 batches, the 357 x 8615 live shape with ragged lengths, and 1 / 16 / 64 reads; the forward
alone (normalised input on the device) and classify_raw (int16 reads: normalise + forward); the MAC rate against the
157 TF f32 MFMA peak.  Config: 8 blocks, 64 filters, k 3, base 2 (synth.TCN_BENCH_CFG) and its TCNBot twin.
    python tools/tcn_bench.py [steps]"""
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


def run(steps=20):
    dev = torch.device("cuda", 0)
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
        m = Model(sd, config, None, "x", device=dev)
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
            ms_fwd = _time(lambda: m.forward_batch(x, lh, lens_dev=ln), steps, dev)
            ms_raw = _time(lambda: m.classify_raw(sig, off, ln, lh), steps, dev)
            macs = sum(T.program_macs(blocks, int(n)) for n in lens)
            res[label] = dict(ms_forward=round(ms_fwd, 4), ms_classify_raw=round(ms_raw, 4),
                              reads_per_s=round(B / (ms_raw * 1e-3), 1), mmac_per_read=round(macs / B / 1e6, 2),
                              tflops_forward=round(2 * macs / (ms_fwd * 1e-3) / 1e12, 3),
                              frac_of_f32_mfma_peak=round(2 * macs / (ms_fwd * 1e-3) / 1e12 / PEAK_TF, 4))
        m.close()
        out[name] = res
    return out


if __name__ == "__main__":
    print(json.dumps(run(int(sys.argv[1]) if len(sys.argv) > 1 else 20)))
