"""Retraining preprocessing, measured: rs_retrain_prepare on raw int16 reads at three cutoffs next to the path
a user had before it - pA on the host, then rs_normalise_float on the float32 prefixes, once per cutoff - in one process,
alternating, on the same reads.

    python tools/retrain_bench.py [--reads 4096] [--samples 16000] [--repeats 7]

Two figures per path: the kernels alone between device events on resident data, and upload + kernels on a host clock that
ends in a synchronise (the downloads are the same bytes for both and are left out; so is the old path's host pA scaling,
which is printed on its own).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from riser_amd import _native as nv     # noqa: E402
from riser_amd import retrain           # noqa: E402

CUTOFFS = [8000, 12000, 16000]


def stat(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.samples >= CUTOFFS[-1]
    dev = torch.device("cuda", 0)
    B, n = a.reads, a.samples
    rng = np.random.default_rng(20260115)
    raw = (500 + rng.integers(-20, 21, size=(4, B, n), dtype=np.int16).sum(axis=0, dtype=np.int16)).astype(np.int16)
    spikes = rng.integers(0, n, size=(B, 24))
    np.put_along_axis(raw, spikes, rng.integers(-2000, 3000, size=spikes.shape).astype(np.int16), axis=1)
    cal = np.stack([rng.integers(-30, 31, size=B).astype(np.float64), (13000 + rng.integers(0, 3000, size=B)) / 10.0 / 8192.0], 1)
    t = time.perf_counter()
    pa = np.array(cal[:, 1:2] * (raw + cal[:, 0:1]), dtype=np.float32)
    t_pa = time.perf_counter() - t
    offs = np.arange(B, dtype=np.int64) * n
    lens = np.full(B, n, dtype=np.int32)
    rows = retrain.row_maps(lens, CUTOFFS)[0]
    L = nv.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    outs_new = [torch.empty((B, c), dtype=torch.float32, device=dev) for c in CUTOFFS]
    outs_old = [torch.empty((B, c), dtype=torch.float32, device=dev) for c in CUTOFFS]

    def new_upload():
        return (torch.from_numpy(raw.reshape(-1)).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev),
                torch.from_numpy(cal).to(dev), torch.from_numpy(rows).to(dev))

    def new_kernels(up):
        sig, off, ln, cal_d, rows_d = up
        retrain.launch(sig, 2, off, ln, cal_d, B, CUTOFFS, 3.5, rows_d, outs_new)

    def old_upload():
        ups = []
        for c in CUTOFFS:                                               # mad_normalise_float_batch: one upload per prefix set
            ups.append((torch.from_numpy(np.ascontiguousarray(pa[:, :c]).reshape(-1)).to(dev),
                        torch.from_numpy(np.arange(B, dtype=np.int64) * c).to(dev),
                        torch.from_numpy(np.full(B, c, dtype=np.int32)).to(dev)))
        return ups

    def old_kernels(ups):
        for (sig, off, ln), o, c in zip(ups, outs_old, CUTOFFS):
            nv.check(L.rs_normalise_float(sig.data_ptr(), 4, off.data_ptr(), ln.data_ptr(), B, o.data_ptr(), c, None, st),
                     "rs_normalise_float")

    def events(fn, arg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(arg)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(upload, kernels):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        kernels(upload())
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    up_new, up_old = new_upload(), old_upload()
    for _ in range(2):                                                  # warm-up, and the two paths agree (no zero MAD here)
        new_kernels(up_new)
        old_kernels(up_old)
    torch.cuda.synchronize(dev)
    for x, y in zip(outs_new, outs_old):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the two paths differ"
    k_new, k_old, w_new, w_old = [], [], [], []
    for _ in range(a.repeats):                                          # alternating
        k_new.append(events(new_kernels, up_new))
        k_old.append(events(old_kernels, up_old))
    del up_new, up_old
    wall(new_upload, new_kernels)
    wall(old_upload, old_kernels)
    for _ in range(a.repeats):
        w_new.append(wall(new_upload, new_kernels))
        w_old.append(wall(old_upload, old_kernels))
    print(f"RETRAIN_BENCH {B} reads x {n} int16 samples, cutoffs {CUTOFFS}, {a.repeats} alternating repeats, outputs bit-identical")
    for name, new, old in (("kernels alone (device events)", k_new, k_old), ("upload + kernels (host clock)", w_new, w_old)):
        (mn, lo_n, hi_n), (mo, lo_o, hi_o) = stat(new), stat(old)
        print(f"  {name}: rs_retrain_prepare {mn:.2f} ms (min {lo_n:.2f}, max {hi_n:.2f}) = {mn * 1e3 / B:.2f} us/read; "
              f"3 x rs_normalise_float {mo:.2f} ms (min {lo_o:.2f}, max {hi_o:.2f}) = {mo * 1e3 / B:.2f} us/read; "
              f"old / new {mo / mn:.2f}")
    print(f"  host pA scaling of the old path (not in either figure): {t_pa * 1e3:.0f} ms")
    up_b_new = raw.nbytes + offs.nbytes + lens.nbytes + cal.nbytes + rows.nbytes
    up_b_old = sum(4 * B * c + 12 * B for c in CUTOFFS)
    hbm = 2 * B * CUTOFFS[-1] + 4 * B * sum(CUTOFFS)
    visits = B * sum(CUTOFFS) * (2 * 4 + 3)                             # 4 counting passes per median, ~3 reads per output
    mk = stat(k_new)[0] * 1e-3
    print(f"  uploaded: {up_b_new / 1e6:.0f} MB against {up_b_old / 1e6:.0f} MB ({up_b_new / up_b_old:.2f})")
    print(f"  new kernel: {hbm / 1e6:.0f} MB of HBM traffic by shape = {hbm / mk / 1e9:.0f} GB/s; "
          f"about {visits / 1e9:.2f} G LDS element visits = {visits / mk / 1e9:.0f} G/s")


if __name__ == "__main__":
    main()
