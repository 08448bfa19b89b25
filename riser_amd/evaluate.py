"""The reference's offline evaluation sweep (riser/test.py) on the GPU.

The script is how a retrained model's thresholds and decision lengths are judged: for every read it finds the poly(A) with a
window rule whose window size and MAD threshold come from the command line (riser/test.py:80-117), trims at the found end or
by a fixed length, and classifies EVERY prefix of min, min + 1 s, ... up to the kit's maximum, each normalised on its own.
Its trim lengths and its maximum differ from the live path's (riser/preprocess.py): 6481 / 4634 samples against 6480 / 4633,
4 s / 2.15 s against 280 nt.

`sweep` does that for a batch of raw reads: one upload, one poly(A) scan (rs_polya_coords), and the prefixes of a read as
(offset, length) pairs that share one offset through `Model.classify_raw` - so any Model of any family and dtype works, and
every pair gets the bits a solo call gives it.  `SweepResult.lines` writes the script's TSV lines;

    python -m riser_amd.evaluate READS.npz MODEL.pth CONFIG.yaml KIT OUT_DIR Y|N [RESOLUTION MAD_THRESHOLD] [--dtype f32w]

takes the script's positional arguments with an .npz (`flat` int16, `lengths`, `read_ids`, `filename`) in place of the fast5
directory and writes OUT_DIR/<filename>_test_output.tsv.

One deviation: the script's `normalise` (riser/test.py:54-56) has no guard for a MAD of 0 and prints nan for a constant
prefix; the library's normalisation gives zeros there, as riser/preprocess.py does.  Real reads have no constant prefix.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass

import numpy as np

# riser/test.py:18-26: sampling rate [Hz], shortest and longest prefix [s], fixed trim [samples]
_MIN_SAMPLES = 4096
_KITS = {"RNA002": (3012, _MIN_SAMPLES / 3012, 4, 6481), "RNA004": (4000, _MIN_SAMPLES / 4000, 2.15, 4634)}


def sweep_plan(kit_version: str) -> dict:
    """-> {sampling_hz, lengths, fixed_trim}: the prefix lengths the script classifies (riser/test.py:202-224), built the way
    it builds them, in Python floats: ceil(min_sec * hz) stepping by hz up to floor(max_sec * hz)."""
    try:
        hz, min_sec, max_sec, fixed_trim = _KITS[kit_version]
    except KeyError:
        raise ValueError(f"Sequencing kit {kit_version!r} invalid (RNA002 / RNA004)") from None
    lengths, n = [], math.ceil(min_sec * hz)
    while n <= math.floor(max_sec * hz):
        lengths.append(n)
        n += hz
    return {"sampling_hz": hz, "lengths": lengths, "fixed_trim": fixed_trim}


def build_pairs(read_lens, ends, lengths, fixed_trim: int, already_trimmed: bool = False):
    """The script's trim and length rules (riser/test.py:190-211) for N reads -> (trims int64 [N], valid bool [N, K]).
    A read loses end + 1 samples where an end was found (the script tests `if polyA_end`: None and 0 are not one), else
    `fixed_trim`, a start alone included; nothing when `already_trimmed`.  Pair (n, k) exists where what is left has at
    least lengths[k] samples."""
    read_lens = np.asarray(read_lens, dtype=np.int64)
    ends = np.asarray(ends, dtype=np.int64)
    if already_trimmed:
        trims = np.zeros_like(read_lens)
    else:
        trims = np.where(ends > 0, ends + 1, int(fixed_trim))
    rest = np.maximum(read_lens - trims, 0)
    valid = rest[:, None] >= np.asarray(lengths, dtype=np.int64)[None, :]
    return trims, valid


@dataclass
class SweepResult:
    starts: np.ndarray              # int32 [N], -1: none
    ends: np.ndarray                # int32 [N], -1: none
    lengths: list                   # K prefix lengths
    probs: np.ndarray               # float32 [N, K, 2] as (p_n, p_p); NaN where the trimmed read is shorter than the prefix
    valid: np.ndarray               # bool [N, K]
    already_trimmed: bool = False

    def lines(self, model_id, dataset, filename, read_ids) -> list:
        """The script's output lines (riser/test.py:221,226), one per read, newline included: seven tab-separated fields,
        the poly(A) coordinates as an int, `None`, or `boostnano` for reads trimmed beforehand, the predictions as
        `L:p_n,p_p` joined by `;` - each probability the Python repr of the fp32 value widened to double, which is what
        the script's f-string makes of `tensor.item()`.  A read with no prediction keeps its line, with an empty field."""
        out = []
        for n, rid in enumerate(read_ids):
            if self.already_trimmed:
                start = end = "boostnano"
            else:
                start = "None" if self.starts[n] < 0 else str(int(self.starts[n]))
                end = "None" if self.ends[n] < 0 else str(int(self.ends[n]))
            preds = ";".join(f"{L}:{float(self.probs[n, k, 0])!r},{float(self.probs[n, k, 1])!r}"
                             for k, L in enumerate(self.lengths) if self.valid[n, k])
            out.append(f"{model_id}\t{dataset}\t{filename}\t{rid}\t{start}\t{end}\t{preds}\n")
        return out


def sweep(model, signals, kit_version: str, already_trimmed: bool = False, resolution: int = 500, mad_threshold: int = 20,
          pairs_per_call: int = 1024) -> SweepResult:
    """riser/test.py:187-224 for a list of raw int16 reads of any length, on `model`'s device."""
    import torch
    from .preprocess import Kit, SignalProcessor, pack_reads

    plan = sweep_plan(kit_version)
    lengths = plan["lengths"]
    if min(lengths) < model.min_length:
        raise ValueError(f"the sweep's shortest prefix, {min(lengths)} samples, is below the model's minimum {model.min_length}")
    if pairs_per_call < 1:
        raise ValueError("pairs_per_call must be at least 1")
    N, K = len(signals), len(lengths)
    starts = np.full(N, -1, dtype=np.int32)
    ends = np.full(N, -1, dtype=np.int32)
    probs = np.full((N, K, 2), np.nan, dtype=np.float32)
    if N == 0:
        return SweepResult(starts, ends, lengths, probs, np.zeros((0, K), dtype=bool), already_trimmed)
    dev = model.device
    sig, off, ln, lens = pack_reads(signals, dev)
    offs = np.zeros(N, dtype=np.int64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    if not already_trimmed:
        proc = SignalProcessor(Kit.create_from_version(kit_version), device=dev)
        s_dev, e_dev = proc.polyA_coords_device(sig, off, ln, N, int(lens.max()), resolution, mad_threshold)
        starts, ends = s_dev.cpu().numpy(), e_dev.cpu().numpy()
    trims, valid = build_pairs(lens, ends, lengths, plan["fixed_trim"], already_trimmed)
    rn, rk = np.nonzero(valid)                                         # (read, length) order
    pair_off = (offs + trims)[rn]
    pair_len = np.asarray(lengths, dtype=np.int32)[rk]
    flat = probs.reshape(N * K, 2)
    for p0 in range(0, rn.size, pairs_per_call):
        p1 = min(rn.size, p0 + pairs_per_call)
        h_len = np.ascontiguousarray(pair_len[p0:p1])
        d_off = torch.from_numpy(np.ascontiguousarray(pair_off[p0:p1])).to(dev)
        d_len = torch.from_numpy(h_len).to(dev)
        got = model.classify_raw(sig, d_off, d_len, h_len)
        flat[rn[p0:p1] * K + rk[p0:p1]] = got.cpu().numpy()
    if getattr(model, "is_half", False):
        model.warn_if_saturated("sweep()")
    return SweepResult(starts, ends, lengths, probs, valid, already_trimmed)


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m riser_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("reads", help=".npz with flat (int16), lengths, read_ids, filename")
    ap.add_argument("model_file")
    ap.add_argument("config_file")
    ap.add_argument("kit", help="RNA002 / RNA004")
    ap.add_argument("out_dir")
    ap.add_argument("already_trimmed", choices=["Y", "N"], help="were the signals trimmed by BoostNano already?")
    ap.add_argument("resolution", nargs="?", type=int)
    ap.add_argument("mad_threshold", nargs="?", type=int)
    ap.add_argument("--dtype", default="f32w")
    a = ap.parse_args(argv)
    trimmed = a.already_trimmed == "Y"
    if not trimmed and (a.resolution is None or a.mad_threshold is None):
        ap.error("RESOLUTION and MAD_THRESHOLD are needed with N (riser/test.py:153-154)")
    sweep_plan(a.kit)                                                  # an unknown kit: before anything is loaded
    from .model import Model
    from .modeldir import get_config
    g = np.load(a.reads, allow_pickle=False)
    lens = np.asarray(g["lengths"], dtype=np.int64)
    bounds = np.concatenate([[0], np.cumsum(lens)])
    flat = np.asarray(g["flat"], dtype=np.int16)
    signals = [flat[bounds[i]:bounds[i + 1]] for i in range(lens.size)]
    read_ids = [str(r) for r in g["read_ids"]]
    filename = str(g["filename"])
    model_id = a.model_file.split(".pth")[0].split("/")[-1]            # riser/test.py:163
    dataset = os.path.splitext(a.reads.rstrip("/").split("/")[-1])[0]  # the script: the last component of the fast5 directory
    model = Model(a.model_file, get_config(a.config_file), None, model_id, dtype=a.dtype)
    res = sweep(model, signals, a.kit, trimmed, a.resolution or 500, a.mad_threshold if a.mad_threshold is not None else 20)
    path = os.path.join(a.out_dir, f"{filename}_test_output.tsv")
    with open(path, "w") as f:
        f.writelines(res.lines(model_id, dataset, filename, read_ids))
    print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
