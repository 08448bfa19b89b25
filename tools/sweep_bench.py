"""Offline evaluation sweep, measured: rs_polya_coords at (500, 20) next to rs_polya_end on the same 512 raw
reads, in one process, and the pairs per second of one riser_amd.evaluate.sweep over 512 reads per kit.

    python tools/sweep_bench.py [--reads 512]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from riser_amd import evaluate, synth                                # noqa: E402
from riser_amd.model import Model                                    # noqa: E402
from riser_amd.preprocess import Kit, SignalProcessor, pack_reads    # noqa: E402


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=dev)
    reads = [synth.make_raw_read(93, rid, 9000 + 37 * (rid % 256), rid % 4 != 3) for rid in range(a.reads)]
    sig, off, ln, lens = pack_reads(reads, dev)
    B, lmax = len(reads), int(lens.max())
    live = proc.polyA_end_device(sig, off, ln, B).cpu().numpy()
    _, gen = proc.polyA_coords_device(sig, off, ln, B, lmax, 500, 20)
    assert np.array_equal(live, gen.cpu().numpy())
    t_live = timed(lambda: proc.polyA_end_device(sig, off, ln, B))
    t_gen = timed(lambda: proc.polyA_coords_device(sig, off, ln, B, lmax, 500, 20))
    print(f"POLYA_TIME {B} reads of {int(lens.min())}-{lmax} samples, ends found {int((live > 0).sum())}: "
          f"rs_polya_end {t_live * 1e3:.3f} ms, rs_polya_coords(500, 20) {t_gen * 1e3:.3f} ms, ratio {t_gen / t_live:.2f}")
    model = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", device=dev)
    for kit in ("RNA002", "RNA004"):
        hi = {"RNA002": 18000, "RNA004": 14000}[kit]
        rs = [synth.make_raw_read(93, rid, 7000 + (hi - 7000) * (rid % 64) // 63, rid % 4 != 3) for rid in range(a.reads)]
        evaluate.sweep(model, rs, kit)
        times = []
        for _ in range(9):                                             # whole sweeps, host work included: the median of nine
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = evaluate.sweep(model, rs, kit)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        times.sort()
        n, dt = int(res.valid.sum()), times[len(times) // 2]
        print(f"SWEEP_RATE {kit}: {len(rs)} reads, {n} pairs, median of 9 sweeps {dt * 1e3:.2f} ms (min {times[0] * 1e3:.2f}, "
              f"max {times[-1] * 1e3:.2f}) = {n / dt:.0f} pairs/s (upload, scan, classify, download)")
    model.close()


if __name__ == "__main__":
    main()
