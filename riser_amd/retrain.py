"""The reference's retraining preprocessing (riser/retrain/preprocess.py, riser/retrain/write_tensors.py) on the GPU.

The README's retraining recipe runs `preprocess.py N_SECS FREQ FAST5_DIR` three times (2 s, 3 s, 4 s): every read of at
least N_SECS * FREQ samples is scaled to pA, cut to that length, MAD-normalised in float32 and outlier-smoothed in a Python
loop; `write_tensors.py` then balances a positive and a negative set and saves them as `.pt` files for train.py.

`prepare` does the first for a list of reads and ALL requested lengths in one pass (rs_retrain_prepare,
csrc/retrain_prep.hip): raw int16 samples and the channel calibration go up once, every prefix comes back.  The results are
the script's bit for bit, its quirks included: it has NO guard for a MAD of zero (:42-44), so a read with more than half of
its first n samples equal comes back as NaN / +-inf, smoothed as the script smooths them - where the live rule
(`SignalProcessor.mad_normalise`, riser/preprocess.py:122-125) gives zeros; and the outlier limit is a parameter.

    python -m riser_amd.retrain preprocess N_SECS FREQ READS.npz [--out-dir D] [--outlier-lim X]
    python -m riser_amd.retrain write-tensors POS.npy NEG.npy OUT_DIR

N_SECS is one integer or a comma list (`2,3,4`: the README's three runs as one).  READS.npz holds `flat`, `lengths`,
`read_ids`, `filename` as riser_amd.evaluate takes them, plus `offset`, `range`, `digitisation` (one per read) when `flat`
is int16; a float `flat` is pA.  `preprocess` writes D/{name}_{cutoff}.npy, {name} being the .npz file's name without its
extension (the script: the last component of the fast5 directory), and prints the script's discard line per cutoff.

Deviations from the scripts: a result without reads has shape (0, cutoff) where the script saves np.array([]);
write_tensors.py's `build_dataset` (concatenation in glob order, unused by its main) is not reproduced.  Reading fast5 /
pod5 files is out of scope: reads arrive as arrays.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import NamedTuple

import numpy as np

from . import _native as nv

WORKGROUP_THREADS = 512          # csrc/retrain_prep.hip: kThreads
MAX_CUTOFFS = 4                  # cutoffs per call of rs_retrain_prepare
MAX_CUTOFF = 32768               # samples: a read's longest prefix is staged in LDS


class Prepared(NamedTuple):
    cutoff: int
    data: np.ndarray             # float32 [N_c, cutoff]: the reads of at least `cutoff` samples, in input order
    kept: np.ndarray             # int64 [N_c]: their indices in the input


def cutoffs_for(n_secs, freq: int) -> list:
    """freq * n_secs (riser/retrain/preprocess.py:53) for one N_SECS or each of several."""
    secs = [n_secs] if np.isscalar(n_secs) else list(n_secs)
    return [int(freq) * int(s) for s in secs]


def check_cutoffs(cutoffs) -> list:
    cuts = [int(c) for c in cutoffs]
    if not cuts:
        raise ValueError("no cutoff")
    if any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cutoffs must be strictly ascending, got {cuts}")
    if cuts[0] < 2 or cuts[-1] > MAX_CUTOFF:
        raise ValueError(f"cutoffs must lie in [2, {MAX_CUTOFF}], got {cuts}")
    return cuts


def scale_of(rng, digitisation) -> np.ndarray:
    """pA per ADC step, in float64 as the fast5 attributes are"""
    return np.asarray(rng, dtype=np.float64) / np.asarray(digitisation, dtype=np.float64)


def as_calibration(calibration, n_reads: int) -> np.ndarray:
    """-> float64 [N, 2] = (offset, scale) from that table or from the three arrays (offset, range, digitisation)"""
    if isinstance(calibration, (tuple, list)) and len(calibration) == 3 and np.ndim(calibration[0]) == 1:
        offset, rng, dig = calibration
        cal = np.stack([np.asarray(offset, dtype=np.float64), scale_of(rng, dig)], axis=1)
    else:
        cal = np.asarray(calibration, dtype=np.float64)
    if cal.shape != (n_reads, 2):
        raise ValueError(f"calibration of shape {cal.shape} for {n_reads} reads: expected [N, 2] = (offset, scale) "
                         "or the three arrays (offset, range, digitisation)")
    return np.ascontiguousarray(cal)


def row_maps(lens, cutoffs):
    """Where each read's row goes -> (rows int64 [n_cut, B], kept list of int64 index arrays): at cutoff c the reads with
    len >= cutoffs[c] take rows 0, 1, ... in input order, the others -1 (the script's `continue`, :83-85)."""
    lens = np.asarray(lens, dtype=np.int64)
    rows = np.full((len(cutoffs), lens.size), -1, dtype=np.int64)
    kept = []
    for c, n in enumerate(cutoffs):
        idx = np.nonzero(lens >= n)[0].astype(np.int64)
        rows[c, idx] = np.arange(idx.size, dtype=np.int64)
        kept.append(idx)
    return rows, kept


def launch(sig, elem_bytes: int, off, ln, calib, B: int, cutoffs, outlier_lim: float, rows, outs, stats=None, stream=None):
    """rs_retrain_prepare on torch device tensors (`calib`, `stats`: a tensor or None; `outs`: one tensor per cutoff)."""
    import torch
    cuts = (C.c_int32 * len(cutoffs))(*cutoffs)
    ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    if stream is None:
        stream = torch.cuda.current_stream(sig.device).cuda_stream
    nv.check(nv.lib().rs_retrain_prepare(sig.data_ptr(), elem_bytes, off.data_ptr(), ln.data_ptr(),
                                         calib.data_ptr() if calib is not None else None, B, cuts, len(cutoffs),
                                         float(outlier_lim), rows.data_ptr(), ptrs,
                                         stats.data_ptr() if stats is not None else None, stream), "rs_retrain_prepare")


def prepare(signals, cutoffs, calibration=None, outlier_lim: float = 3.5, device=None, sub_batch: int = 4096) -> list:
    """riser/retrain/preprocess.py:75-92 for a list of reads at every cutoff -> [Prepared(cutoff, data, kept), ...].

    `signals`: int16 reads with `calibration` (float64 [N, 2] = (offset, scale), or the three arrays offset / range /
    digitisation), or float32 pA reads without.  Reads go up `sub_batch` at a time, cut to the longest cutoff; device memory
    is bounded by sub_batch, and the rows come back through pinned memory."""
    import torch
    cuts = check_cutoffs(cutoffs)
    if len(cuts) > MAX_CUTOFFS:
        raise ValueError(f"at most {MAX_CUTOFFS} cutoffs per call, got {len(cuts)}")
    if sub_batch < 1:
        raise ValueError("sub_batch must be at least 1")
    arrs = [np.asarray(s) for s in signals]
    N = len(arrs)
    raw = calibration is not None
    want = np.int16 if raw else np.float32
    if any(a.dtype != want or a.ndim != 1 for a in arrs):
        raise TypeError("prepare takes int16 reads with a calibration, or float32 pA reads without one; got "
                        f"{sorted({str(a.dtype) for a in arrs})}")
    cal = as_calibration(calibration, N) if raw else None
    lens = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    _, kept = row_maps(lens, cuts)
    res = [np.empty((k.size, n), dtype=np.float32) for k, n in zip(kept, cuts)]
    if N == 0 or kept[0].size == 0:
        return [Prepared(n, r, k) for n, r, k in zip(cuts, res, kept)]
    nv.require_gpu()
    d = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
    done = [0] * len(cuts)
    for b0 in range(0, N, sub_batch):
        b1 = min(N, b0 + sub_batch)
        B = b1 - b0
        part = [a[: cuts[-1]] for a in arrs[b0:b1]]                    # nothing behind the longest cutoff is needed
        up = np.minimum(lens[b0:b1], cuts[-1])
        rows, sub_kept = row_maps(lens[b0:b1], cuts)
        if sub_kept[0].size == 0:
            continue
        offs = np.zeros(B, dtype=np.int64)
        offs[1:] = np.cumsum(up[:-1])
        flat = np.concatenate(part) if int(up.sum()) else np.zeros(1, dtype=want)
        with torch.cuda.device(dev):
            sig = torch.from_numpy(flat).to(dev)
            off_d = torch.from_numpy(offs).to(dev)
            len_d = torch.from_numpy(lens[b0:b1].astype(np.int32)).to(dev)
            cal_d = torch.from_numpy(cal[b0:b1]).to(dev) if raw else None
            rows_d = torch.from_numpy(rows).to(dev)
            outs = [torch.empty((max(k.size, 1), n), dtype=torch.float32, device=dev) for k, n in zip(sub_kept, cuts)]
            launch(sig, 2 if raw else 4, off_d, len_d, cal_d, B, cuts, outlier_lim, rows_d, outs)
            for c, (k, o) in enumerate(zip(sub_kept, outs)):
                if k.size == 0:
                    continue
                host = torch.empty((k.size, cuts[c]), dtype=torch.float32, pin_memory=True)
                host.copy_(o[: k.size], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()
                res[c][done[c]: done[c] + k.size] = host.numpy()
                done[c] += k.size
    return [Prepared(n, r, k) for n, r, k in zip(cuts, res, kept)]


def write_tensors(pos, neg, out_dir: str):
    """riser/retrain/write_tensors.py:43-57: the longer set is cut to the shorter one's length, both become float32 tensors
    and are saved as out_dir/positive.pt and out_dir/negative.pt.  Host only.  -> the two tensors."""
    import torch
    pos, neg = np.asarray(pos), np.asarray(neg)
    n = min(len(pos), len(neg))
    tensors = []
    for arr, name in ((pos[:n], "positive.pt"), (neg[:n], "negative.pt")):
        t = torch.from_numpy(np.ascontiguousarray(arr)).float()
        torch.save(t, os.path.join(out_dir, name))
        tensors.append(t)
    return tuple(tensors)


def load_reads(path: str):
    """READS.npz -> (signals, calibration | None, read_ids, filename)"""
    g = np.load(path, allow_pickle=False)
    lens = np.asarray(g["lengths"], dtype=np.int64)
    bounds = np.concatenate([[0], np.cumsum(lens)])
    flat = np.asarray(g["flat"])
    if flat.dtype == np.int16:
        missing = [k for k in ("offset", "range", "digitisation") if k not in g.files]
        if missing:
            raise ValueError(f"{path}: int16 `flat` needs the calibration arrays, {missing} missing")
        cal = as_calibration((g["offset"], g["range"], g["digitisation"]), lens.size)
    elif np.issubdtype(flat.dtype, np.floating):
        flat, cal = flat.astype(np.float32, copy=False), None
    else:
        raise TypeError(f"{path}: `flat` must be int16 (raw) or float (pA), got {flat.dtype}")
    signals = [flat[bounds[i]:bounds[i + 1]] for i in range(lens.size)]
    return signals, cal, [str(r) for r in g["read_ids"]], str(g["filename"])


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m riser_amd.retrain", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("preprocess", help="riser/retrain/preprocess.py for every N_SECS in one pass")
    p.add_argument("n_secs", type=lambda s: [int(v) for v in s.split(",")], help="seconds per signal: 4, or 2,3,4")
    p.add_argument("freq", type=int, help="sampling rate [Hz]")
    p.add_argument("reads", help=".npz with flat, lengths, read_ids, filename (+ offset, range, digitisation for int16)")
    p.add_argument("--out-dir", default=".")
    p.add_argument("--outlier-lim", type=float, default=3.5)
    w = sub.add_parser("write-tensors", help="riser/retrain/write_tensors.py")
    w.add_argument("pos_npy")
    w.add_argument("neg_npy")
    w.add_argument("out_dir")
    a = ap.parse_args(argv)
    if a.command == "preprocess":
        try:
            a.cutoffs = check_cutoffs(sorted(cutoffs_for(a.n_secs, a.freq)))
        except ValueError as e:
            ap.error(str(e))
        a.name = os.path.splitext(a.reads.rstrip("/").split("/")[-1])[0]
    return a


def output_paths(out_dir: str, name: str, cutoffs) -> list:
    return [os.path.join(out_dir, f"{name}_{n}.npy") for n in cutoffs]           # riser/retrain/preprocess.py:99


def main(argv=None) -> int:
    a = parse_args(argv)
    if a.command == "write-tensors":
        p_data, n_data = np.load(a.pos_npy, allow_pickle=True), np.load(a.neg_npy, allow_pickle=True)
        print(f"Dataset sizes before balancing:\npositive data shape: {p_data.shape}\nnegative data shape: {n_data.shape}")
        p, n = write_tensors(p_data, n_data, a.out_dir)
        print("Dataset sizes after balancing positive and negative sets:\n"
              f"positive data shape: {tuple(p.shape)}\nnegative data shape: {tuple(n.shape)}")
        return 0
    signals, cal, _, filename = load_reads(a.reads)
    paths = output_paths(a.out_dir, a.name, a.cutoffs)
    for i in range(0, len(a.cutoffs), MAX_CUTOFFS):
        for r, path in zip(prepare(signals, a.cutoffs[i:i + MAX_CUTOFFS], cal, a.outlier_lim), paths[i:]):
            print(f"# of discarded reads (< {r.cutoff} samples) in {filename}: {len(signals) - r.kept.size}")
            np.save(path, r.data)
    return 0


if __name__ == "__main__":
    sys.exit(main())
