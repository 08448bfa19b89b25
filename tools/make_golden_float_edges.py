#!/usr/bin/env python3
"""Generate tests/golden/float_edges.npz by running the REFERENCE's two MAD normalisers on the value-edge table.

Runs only in the build container: it loads /root/reference/riser/preprocess.py and riser/retrain/preprocess.py at run time
(with stubs for matplotlib and ont_fast5_api, which the functions used here never touch); neither exists on the GPU box and
neither may be copied.  The committed output is data: the seed that rebuilds every read through tests/float_edges_ref.py, a CRC
of those reads, and the arrays the reference's own functions returned for them, concatenated in the table's order (a zip member
per array would cost more than the arrays; float_edges_ref.unpack splits them again).  Nothing of an input is stored.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_float_edges.py

Reference entry points exercised:
  preprocess.py           SignalProcessor.mad_normalise :108-147 on every case of float16 / float32 / float64
  retrain/preprocess.py   mad_normalise :8-44 on every float32 case of two samples or more, and on the first CUTOFFS samples of
                          the int16 reads under every degenerate calibration (scaled by retrain_ref.pa), at outlier_lim 3.5 and 0.0

np.savez stamps its members with the time of day; the file is written member by member with a fixed stamp so that a second run
gives the same bytes.
"""
import importlib.util
import io
import os
import sys
import types
import warnings
import zipfile

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import matplotlib.pyplot  # noqa: F401  (preprocess.py:3 imports it and never draws)
except ImportError:
    sys.modules.setdefault("matplotlib", types.ModuleType("matplotlib"))
    sys.modules.setdefault("matplotlib.pyplot", types.ModuleType("matplotlib.pyplot"))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules.setdefault("ont_fast5_api", types.ModuleType("ont_fast5_api"))
sys.modules.setdefault("ont_fast5_api.fast5_interface", types.SimpleNamespace(get_fast5_file=None))

import numpy as np          # noqa: E402

from tests import float_edges_ref as F  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_live = _load("riser_preprocess", "/root/reference/riser/preprocess.py")
ref_prep = _load("riser_retrain_preprocess", "/root/reference/riser/retrain/preprocess.py")

OUT = os.path.join(ROOT, "tests", "golden", "float_edges.npz")


def save_npz(path, arrays):
    """np.savez_compressed with every member stamped 1980-01-01"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    proc = ref_live.SignalProcessor(ref_live.Kit.create_from_version("RNA004"))
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # neither script guards its arithmetic
        for dt in F.DTYPES:
            kinds = {}
            for name, x in F.edge_reads(dt, F.SEED):
                y = proc.mad_normalise(x.copy())
                kinds[str(y.dtype)] = kinds.get(str(y.dtype), 0) + 1
                out[F.live_key(dt, name)] = y
                if dt == "float32" and len(x) >= 2:
                    for lim in F.LIMITS:
                        y = ref_prep.mad_normalise(x.copy(), lim)
                        assert y.dtype == np.float32
                        out[F.retrain_key(name, lim)] = y
            print(f"live {dt}: {kinds}")
        for name, _, pa in F.calibrated(F.SEED):
            for lim in F.LIMITS:
                for n in F.CUTOFFS:
                    y = ref_prep.mad_normalise(pa[:n].copy(), lim)
                    assert y.dtype == np.float32
                    out[F.retrain_key("cal." + name, lim, n)] = y
    packed = {"seed": np.int64(F.SEED), "inputs_crc": np.int64(F.inputs_crc(F.SEED)), "limits": np.array(F.LIMITS),
              "cutoffs": np.array(F.CUTOFFS, dtype=np.int32)}
    for group, keys in F.golden_groups(F.SEED).items():
        rows = [out.pop(k) for k, _ in keys]
        zeros = np.array([r.dtype == np.int64 for r in rows])             # np.vectorize over `return 0`: int64, all zero
        assert all(not r.any() for r, z in zip(rows, zeros) if z) and len({r.dtype for r, z in zip(rows, zeros) if not z}) == 1
        packed[group + ".int64_zeros"] = zeros
        packed[group + ".flat"] = np.concatenate([r for r, z in zip(rows, zeros) if not z])
    assert not out
    save_npz(OUT, packed)
    print(OUT, len(packed), "arrays,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
