#!/usr/bin/env python3
"""Generic ConvNets (riser/nets/cnn.py at depth > 1 / kernels other than 3) on csrc/gconv.hip against the conv / max-pool
program of csrc/seqnet.hip (RS_GCONV=0: reads grouped by length, one forward per distinct length): ms per call and reads/s,
both paths built in ONE process and timed shape by shape, interleaved.  Nets: the depth-2 variant of
tests/golden/convnet_variants.npz (channels 6-20, kernels 5-3-7-3) and a net of the shipped widths (synth.CnnConfig's channel
list) with kernels 5.  Shapes: 512 x 16000, 512 x 4000, the live shape of 357 reads with distinct lengths around 8615, and
1 / 16 reads.
    python tools/gconv_bench.py [steps] [--only LABEL] [--net depth2|shipped_k5|both] [--path gconv|seqnet|both]
                                [--dtype f32|bf16x3|both]
--only / --path run one shape on one path (for a profiler run of its own).  --dtype bf16x3 / both times the family in split
precision on the bf16 MFMA (csrc/gconv_x3.hip) instead of / next to fp32: the seqnet path is left out, both modes are built
in one process and timed shape by shape, interleaved, and "<shape>:f32/bf16x3" is the ratio of their ms per call."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from riser_amd import gconv as G
from riser_amd import synth
from riser_amd.model import Model

PEAK_TF = 157.3
SHAPES = [("512x16000", 512, 16000, False), ("512x4000", 512, 4000, False), ("357x8615_ragged", 357, 8615, True),
          ("1x16000", 1, 16000, False), ("16x16000", 16, 16000, False)]


def _time(fn, steps, dev):
    fn()
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize(dev)
    return t0.elapsed_time(t1) / steps


def _state_dict(cnn, seed):
    rng = np.random.default_rng(seed)
    sd, c_in = {}, 1
    for i in range(int(cnn.n_layers)):
        co, k = int(cnn.channels[i]), int(cnn.kernels[i])
        for d in range(int(cnn.depth)):
            sd[f"layers.{i}.{2 * d}.weight"] = (rng.standard_normal((co, c_in, k)) * np.sqrt(2.0 / (k * c_in))).astype(np.float32)
            sd[f"layers.{i}.{2 * d}.bias"] = (rng.standard_normal(co) * 0.1).astype(np.float32)
            c_in = co
    sd["classifier.2.weight"] = rng.standard_normal((2, c_in)).astype(np.float32)
    sd["classifier.2.bias"] = rng.standard_normal(2).astype(np.float32)
    return sd


def nets():
    shipped = synth.CnnConfig()
    return {"depth2": synth.CnnConfig(channels=[6, 9, 14, 20], kernels=[5, 3, 7, 3], depth=2),
            "shipped_k5": synth.CnnConfig(channels=list(shipped.channels), kernels=[5] * int(shipped.n_layers))}


def _model(sd, cnn, dev, path):
    old = os.environ.pop("RS_GCONV", None)
    if path == "seqnet":
        os.environ["RS_GCONV"] = "0"
    try:
        return Model(sd, synth.Config(cnn), None, "x", device=dev, dtype="bf16x3" if path == "gconv_x3" else "f32w")
    finally:
        os.environ.pop("RS_GCONV", None)
        if old is not None:
            os.environ["RS_GCONV"] = old


def run(steps=3, only=None, which=("depth2", "shipped_k5"), paths=("seqnet", "gconv")):
    dev = torch.device("cuda", 0)
    out = {}
    for name in which:
        cnn = nets()[name]
        sd = _state_dict(cnn, 11)
        prog = G.build_gconv_program(sd, cnn)
        models = {p: _model(sd, cnn, dev, p) for p in paths}
        res = {"convs": len(prog["convs"])}
        for label, B, L, ragged in SHAPES:
            if only and label != only:
                continue
            if L < G.min_length(prog):              # 512 x 4000 under a 12-layer net: the reference's max_pool raises
                res[label] = "skipped: below the network minimum %d" % G.min_length(prog)
                continue
            rng = np.random.default_rng(5)
            lens = (L - 200 + rng.permutation(400)[:B]) if ragged else np.full(B, L)      # distinct lengths around L
            lens = np.asarray(lens, dtype=np.int32)
            ld = int(lens.max())
            x = torch.from_numpy(np.clip(rng.standard_normal((B, ld)), -3.5, 3.5).astype(np.float32)).to(dev)
            ln = torch.from_numpy(lens).to(dev)
            macs = sum(G.program_macs(prog, int(n)) for n in lens)
            for p, m in models.items():
                ms = _time(lambda: m.forward_batch(x, lens, lens_dev=ln), steps if p != "seqnet" or not ragged else 1, dev)
                res[f"{label}:{p}"] = dict(ms=round(ms, 3), reads_per_s=round(B / (ms * 1e-3), 1),
                                           tflops=round(2 * macs / (ms * 1e-3) / 1e12, 3),
                                           frac_of_f32_mfma_peak=round(2 * macs / (ms * 1e-3) / 1e12 / PEAK_TF, 4))
            if "seqnet" in paths and "gconv" in paths:
                res[f"{label}:seqnet/gconv"] = round(res[f"{label}:seqnet"]["ms"] / res[f"{label}:gconv"]["ms"], 3)
            if "gconv" in paths and "gconv_x3" in paths:
                res[f"{label}:f32/bf16x3"] = round(res[f"{label}:gconv"]["ms"] / res[f"{label}:gconv_x3"]["ms"], 3)
        for m in models.values():
            m.close()
        out[name] = res
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=3)
    ap.add_argument("--only", default=None, choices=[s[0] for s in SHAPES])
    ap.add_argument("--net", choices=("depth2", "shipped_k5", "both"), default="both")
    ap.add_argument("--path", choices=("gconv", "seqnet", "both"), default="both")
    ap.add_argument("--dtype", choices=("f32", "bf16x3", "both"), default="f32")
    args = ap.parse_args()
    paths = ("seqnet", "gconv") if args.path == "both" else (args.path,)
    if args.dtype != "f32":                  # the family alone, in the modes asked for
        paths = {"bf16x3": ("gconv_x3",), "both": ("gconv", "gconv_x3")}[args.dtype]
    print(json.dumps(run(args.steps, args.only, ("depth2", "shipped_k5") if args.net == "both" else (args.net,), paths)))
