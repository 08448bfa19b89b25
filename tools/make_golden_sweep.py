#!/usr/bin/env python3
"""Generate tests/golden/polya_coords.npz and tests/golden/sweep.npz by running the REFERENCE's offline evaluation script.

Runs only in the build container: it imports /root/reference/riser/test.py at run time (with stub modules for the three
imports of that script that are not installed and that the functions used here never touch), which does not exist on the GPU
box and must never be copied.  The committed outputs are data: the integer seeds that rebuild every signal and the weights
through riser_amd.synth, the parameters, and the values the script's own functions returned.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sweep.py

Reference entry points exercised (riser/test.py):
  get_polyA_coords   :80-117   window rule at 12 (resolution, mad_threshold) rows on 36 reads, and on 24 reads at negative levels
  the loop of main() :187-224  get_polyA_coords(., 500, 20), the trim, then mad_normalise + classify per prefix length, both kits
"""
import importlib.util
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# riser/test.py:5,8,10 import these three (not installed; only main() and get_config use them): stub them.
sys.modules.setdefault("attridict", types.ModuleType("attridict"))
sys.modules.setdefault("torchinfo", types.SimpleNamespace(summary=None))
sys.modules.setdefault("ont_fast5_api", types.ModuleType("ont_fast5_api"))
sys.modules.setdefault("ont_fast5_api.fast5_interface", types.SimpleNamespace(get_fast5_file=None))
sys.path.insert(0, "/root/reference/riser")

import numpy as np          # noqa: E402
import torch                # noqa: E402

from riser_amd import synth  # noqa: E402

# the script is called test.py: load it under another name, the standard library has a `test` package
_spec = importlib.util.spec_from_file_location("riser_offline_test", "/root/reference/riser/test.py")
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

OUT = os.path.join(ROOT, "tests", "golden")
COORD_SEED, COORD_READS = 91, 24
COORD_ROWS = [(500, 20), (250, 20), (501, 20), (333, 12), (1000, 30), (64, 15), (7, 20), (2048, 25), (500, 60), (500, 5),
              (1, 20), (4096, 40)]
NEG_SHIFT, NEG_ROWS = 900, [(500, 20), (250, 20)]
SWEEP_SEED, SWEEP_READS, WEIGHTS_SEED = 93, 16, 1


def _i(v):
    return -1 if v is None else int(v)


def coords_reads():
    reads = [synth.make_raw_read(COORD_SEED, rid, 6000 + 523 * rid, rid % 4 != 3) for rid in range(COORD_READS)]
    return reads + [s for _, s in synth.polya_edge_cases()]


def polya_coords():
    reads = coords_reads()
    neg = [(r.astype(np.int32) - NEG_SHIFT).astype(np.int16) for r in reads[:COORD_READS]]

    def run(sigs, rows):
        st = np.zeros((len(rows), len(sigs)), dtype=np.int32)
        en = np.zeros_like(st)
        for k, (res, thr) in enumerate(rows):
            for j, s in enumerate(sigs):
                a, b = ref.get_polyA_coords(s, res, thr)
                st[k, j], en[k, j] = _i(a), _i(b)
        return st, en

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # x / 0 in the rolling-mean cases
        st, en = run(reads, COORD_ROWS)
        nst, nen = run(neg, NEG_ROWS)
    np.savez_compressed(os.path.join(OUT, "polya_coords.npz"), seed=np.int64(COORD_SEED), n_reads=np.int64(COORD_READS),
                        rows=np.array(COORD_ROWS, dtype=np.int32), starts=st, ends=en,
                        neg_shift=np.int64(NEG_SHIFT), neg_rows=np.array(NEG_ROWS, dtype=np.int32), neg_starts=nst, neg_ends=nen)
    for k, row in enumerate(COORD_ROWS):
        both = int(((st[k] >= 0) & (en[k] >= 0)).sum())
        only = int(((st[k] >= 0) & (en[k] < 0)).sum())
        same = int(((st[k] >= 0) & (st[k] == en[k])).sum())
        print(f"coords {row}: start+end {both}, start only {only}, none {len(reads) - both - only}, start == end {same}")
    print("coords neg:", [(int((nst[k] >= 0).sum()), int((nen[k] >= 0).sum())) for k in range(len(NEG_ROWS))])


def ref_convnet():
    from nets.cnn import ConvNet                                          # reference
    net = ConvNet(synth.Config().cnn)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(WEIGHTS_SEED).items()})
    return net.eval()


def sweep():
    net, dev = ref_convnet(), torch.device("cpu")
    reads = [synth.make_raw_read(SWEEP_SEED, rid, 7000 + 911 * rid, rid % 4 != 3) for rid in range(SWEEP_READS)]
    out = {"seed": np.int64(SWEEP_SEED), "n_reads": np.int64(SWEEP_READS), "weights_seed": np.int64(WEIGHTS_SEED)}
    kits = {"RNA002": (ref.SAMPLING_HZ_RNA002, ref.MIN_SIGNAL_SEC_RNA002, ref.MAX_SIGNAL_SEC_RNA002, ref.FIXED_TRIM_RNA002),
            "RNA004": (ref.SAMPLING_HZ_RNA004, ref.MIN_SIGNAL_SEC_RNA004, ref.MAX_SIGNAL_SEC_RNA004, ref.FIXED_TRIM_RNA004)}
    import math
    for kit, (hz, min_sec, max_sec, fixed_trim) in kits.items():
        lengths, n = [], math.ceil(min_sec * hz)
        while n <= math.floor(max_sec * hz):
            lengths.append(n)
            n += hz
        st = np.zeros(len(reads), dtype=np.int32)
        en = np.zeros_like(st)
        probs = np.full((len(reads), len(lengths), 2), np.nan, dtype=np.float32)
        for j, s in enumerate(reads):
            a, b = ref.get_polyA_coords(s, 500, 20)
            st[j], en[j] = _i(a), _i(b)
            rest = s[b + 1:] if b else s[fixed_trim:]
            for k, n in enumerate(lengths):
                if len(rest) < n:
                    continue
                p = ref.classify(ref.mad_normalise(rest[:n]), dev, net)
                probs[j, k] = (p[0][0].item(), p[0][1].item())
        out.update({f"{kit}_lengths": np.array(lengths, dtype=np.int32), f"{kit}_fixed_trim": np.int64(fixed_trim),
                    f"{kit}_starts": st, f"{kit}_ends": en, f"{kit}_probs": probs})
        print(f"sweep {kit}: lengths {lengths}, predictions per read {[int((~np.isnan(probs[j, :, 0])).sum()) for j in range(len(reads))]}, "
              f"fixed trims {int((en < 0).sum())}")
    np.savez_compressed(os.path.join(OUT, "sweep.npz"), **out)


if __name__ == "__main__":
    polya_coords()
    sweep()
