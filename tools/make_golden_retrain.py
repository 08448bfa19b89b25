#!/usr/bin/env python3
"""Generate tests/golden/retrain.npz by running the REFERENCE's retraining scripts.

Runs only in the build container: it imports /root/reference/riser/retrain/preprocess.py (with a stub for ont_fast5_api,
which is not installed and which the functions used here never touch) and write_tensors.py at run time; neither exists on the
GPU box and neither may be copied.  The committed output is data: the seed that rebuilds every read and calibration through
tests/retrain_ref.py, the parameters, and the values the scripts' own functions returned.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_retrain.py

Reference entry points exercised:
  retrain/preprocess.py     mad_normalise :8-15 (with calculate_mad, normalise, smooth_outliers) on the first `cutoff` pA samples
                            of every read that has them (main's :83-86), at every (limit, cutoffs) of retrain_ref.SETS
  retrain/write_tensors.py  main :29-57 on two .npy files of unequal length and dtype
"""
import importlib.util
import os
import sys
import tempfile
import types
import warnings

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.modules.setdefault("ont_fast5_api", types.ModuleType("ont_fast5_api"))
sys.modules.setdefault("ont_fast5_api.fast5_interface", types.SimpleNamespace(get_fast5_file=None))

import numpy as np          # noqa: E402
import torch                # noqa: E402

from tests import retrain_ref as R  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_prep = _load("riser_retrain_preprocess", "/root/reference/riser/retrain/preprocess.py")
ref_wt = _load("riser_retrain_write_tensors", "/root/reference/riser/retrain/write_tensors.py")

OUT = os.path.join(ROOT, "tests", "golden", "retrain.npz")
SEED = 97


def main():
    reads, offset, rng_pa, dig = R.build_reads(SEED)
    sig = [R.pa(r, o, g, d) for r, o, g, d in zip(reads, offset, rng_pa, dig)]
    out = {"seed": np.int64(SEED), "reads_crc": np.int64(R.reads_crc(reads)),
           "limits": np.array([s[0] for s in R.SETS], dtype=np.float64)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # 0 / 0 and x / 0: the script has no guard
        for k, (lim, cutoffs) in enumerate(R.SETS):
            out[f"cutoffs_{k}"] = np.array(cutoffs, dtype=np.int32)
            for n in cutoffs:
                kept = [i for i, s in enumerate(sig) if not len(s) < n]   # :83-85
                rows = [ref_prep.mad_normalise(sig[i][:n], lim) for i in kept]
                assert all(r.dtype == np.float32 for r in rows)
                out[R.key(lim, n)] = np.stack(rows)
                out[R.key(lim, n) + "_kept"] = np.array(kept, dtype=np.int64)
                print(f"limit {lim} cutoff {n}: {len(kept)} reads, {int(np.isnan(out[R.key(lim, n)]).all(axis=1).sum())} all NaN, "
                      f"{int(np.isinf(out[R.key(lim, n)]).any(axis=1).sum())} with inf")
    # write_tensors.py's main on files, as it is run
    pos, neg = R.write_tensor_inputs(out)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "pos.npy"), pos)
        np.save(os.path.join(d, "neg.npy"), neg)
        argv, sys.argv = sys.argv, ["write_tensors.py", os.path.join(d, "pos.npy"), os.path.join(d, "neg.npy"), d]
        try:
            ref_wt.main()
        finally:
            sys.argv = argv
        p = torch.load(os.path.join(d, "positive.pt"))
        n = torch.load(os.path.join(d, "negative.pt"))
    assert p.dtype == torch.float32 and n.dtype == torch.float32
    out["wt_positive"], out["wt_negative"] = p.numpy(), n.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
