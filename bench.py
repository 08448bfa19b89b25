#!/usr/bin/env python3
"""bench.py - chunks/s of the squiggle-classification hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config rna004_b512|promethion|progressive]
                    [--dtype f32|f32_direct|bf16|f16|bf16x3|f16x3] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of synthetic reads already resident in HBM:
MAD-normalise + 12-layer ConvNet forward + softmax, through the C ABI.

  --config rna004_b512   (default) BASELINE.json configs[1], the configuration the metric is quoted on: 512 RNA004
                         4 s chunks (512 x 16000 int16 samples) per GPU and step, fp32 (conv layers lowered to
                         Winograd F(2,3) / F(4,3) on the f32-input MFMA; --dtype f32_direct = exact fmaf chains)
  --config promethion    configs[3]: 18 000 x N concurrent 4 s chunks sharded by read id over the N ranks
                         (riser_amd.dist.shard_indices), every rank walks its HBM-resident shard in sub-batches of
                         --batch reads; one step = one pass over the shard
  --config progressive   configs[4]: mixed 2 s / 3 s / 4 s chunks (8000 / 12000 / 16000 samples in equal thirds of
                         each 512-read batch), fused normalise + conv, fp16 in split precision (f16x3: within 1e-3 of
                         the reference; --dtype f16 is the fast, approximate plain mode)
  --config promethion_live  configs[3] as a LIVE system: every rank runs the batched ReadUntil control loop
                         (riser_amd.SequencerControl) over its own range of 18 000 channels of an 18 000 x N-channel flow
                         cell (riser_amd.launch.rank_channel_range; scripted AccumulatingCache traffic).  One step = one
                         ReadUntil batch of the rank's channels: upload of the new samples, poly(A) scan, gating, normalise,
                         forward, decision, client calls, CSV rows.  value = reads ASSESSED per second over all ranks

Ranks: with WORLD_SIZE in the environment (torch.distributed.run, one rank per GPU) this process is one rank.  With
--gpus N > 1 and NO WORLD_SIZE the script starts the N ranks itself as child processes (before it makes any GPU
call) and prints rank 0's line; it fails if fewer than N devices are visible.  Reads are independent: every rank steps
its own shard, there is no data-path collective; the printed value is the whole-job aggregate over the
max-over-ranks time ("scaling": "weak").

--dump-outputs DIR: after the timed steps, what the last timed step returned, as DIR/probs.npy ([reads, 2] float32;
promethion_live: rejected.npy / finished.npy, float64 channels of the reads the client was sent).  Inputs and weights are
seeded, so two builds of the project run with the same arguments compare output for output.

Prints ONE JSON line on rank 0.  Extra objects:
  roofline      conv stack (layers 1..11, the MFMA kernel family): `achieved` = the TFLOP/s the matrix pipe really
                executes (padded tiles; Winograd issues 2/3 resp. 1/2 of the direct convolution's multiplications),
                from HIP events recorded on the launch stream inside the timed steps; `frac` = achieved / dense MFMA
                peak of the dtype; `algorithmic_tflops` = the direct convolution's FLOPs over the
                same time.  `traffic` is null: HBM bytes need rocprofv3 PMC passes (profiles/, named per round).
  cpu_baseline  the oracle's torch-CPU port timed on this box's host cores over a bounded sample, best of a sweep
                over thread counts (rank 0, N = 1 only)
  control_loop  scripted 512-channel ReadUntil batches through the batched SequencerControl: p50 / p99 per batch

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line; its `roofline` is what the
events inside the timed steps give.  --full adds everything that takes work of its own after the timed steps: the
per-launch pass (roofline.layers, the stage times), the batch latency, the sustained and host-fed figures, the variants,
the control loop, the CPU baseline and the verbose detail file (--no-latency / --no-variants / --no-control-loop /
--no-cpu-baseline drop single parts of it).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from riser_amd import supervise              # noqa: E402  (no torch inside)

supervise.apply_rank_limits()                # a spawned rank pins itself to its core slice BEFORE numpy / torch start pools

import numpy as np                           # noqa: E402
import torch                                 # noqa: E402

from riser_amd import dist as rdist          # noqa: E402
from riser_amd import synth                  # noqa: E402

supervise.apply_torch_threads()

SETTLE_STEPS = 25
BATCH = 512
CHUNK = 16000
SIG_SEED = 20260103
READS_PER_GPU = 18000         # BASELINE config 4: 144 k concurrent chunks over 8 GPUs
LAT_WARMUP, LAT_SAMPLES = 20, 200
PEAK_F32_MFMA_TF = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md:45
PEAK_BF16_MFMA_TF = 2500.0    # :46
PROFILE_ROUND = "r06"         # roofline.traffic comes from profiles/<round>_pmc_fetch_write_<mode>.json of THIS round only
LIB_DTYPE = {"f32": "f32w", "f32_direct": "f32"}
MFMA_PASSES = {"bf16x3": 3, "f16x3": 3, "f16xf8": 3}   # split-precision modes issue three 16-bit MFMAs per product (f16xf8: two
                                                         # instruction times on its wide layers; counted as three here)


def conv_flops_per_chunk(channels, L0):
    """Un-padded algorithmic FLOPs per chunk of each conv layer."""
    out = []
    c_in, L = 1, L0
    for c in channels:
        out.append(2.0 * c_in * c * 3 * L)
        c_in, L = c, L // 2
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", default="rna004_b512", choices=["rna004_b512", "promethion", "progressive", "promethion_live"])
    ap.add_argument("--dtype", default=None, choices=["f32", "f32_direct", "bf16", "f16", "bf16x3", "f16x3", "f16xf8"])
    ap.add_argument("--batch", type=int, default=None, help="reads per library call (sub-batch for promethion)")
    ap.add_argument("--chunk", type=int, default=CHUNK)
    ap.add_argument("--reads-per-gpu", type=int, default=READS_PER_GPU)
    ap.add_argument("--streams", type=int, default=1,
                    help="promethion: sub-batches in flight on separate HIP streams (2: idle CUs of one run the other)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=18.0)
    ap.add_argument("--no-latency", action="store_true", help="skip the per-batch latency loop (profiling runs)")
    ap.add_argument("--no-variants", action="store_true", help="skip the 16-bit / ensemble side measurements")
    ap.add_argument("--no-control-loop", action="store_true", help="skip the ReadUntil replay")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements after the timed steps (per-launch pass, latency, variants, control loop, "
                         "CPU baseline) and the detail file")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)   # CPU rehearsal of the rank plumbing (tests)
    ap.add_argument("--stub-fail-rank", type=int, default=None, help=argparse.SUPPRESS)   # tests: this rank dies before the rendezvous
    args = ap.parse_args(argv)
    if args.dtype is None:
        args.dtype = "f16x3" if args.config == "progressive" else "f32"   # the fp16 mode that meets the 1e-3 tolerance
    if args.batch is None:
        args.batch = 1024 if args.config == "promethion" else BATCH
    if args.steps is None:
        args.steps = {"promethion": 3, "promethion_live": 30}.get(args.config, 50)
    if args.warmup is None:
        args.warmup = {"promethion": 1, "promethion_live": 4}.get(args.config, 30)   # ~60 ms: the shader clock needs ~20 steps to settle
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ---------------------------------------------------------------------------------------------------------------
# rank launcher: --gpus N without torchrun
# ---------------------------------------------------------------------------------------------------------------
def spawn_ranks(args, argv):
    """Start N fresh child processes, one rank per GPU, and relay rank 0's JSON line.  The parent makes no GPU
    call (torch.cuda.device_count() does not initialise the runtime on this image).  The children are polled
    (riser_amd/supervise.py): a rank that dies - before the first barrier or after - ends the run at once with its
    stderr tail and a non-zero exit code instead of leaving its siblings in a collective until an outer timeout; every
    rank runs on its own slice of the host's cores with its thread pools sized to it."""
    n = args.gpus
    if not args.stub and not os.environ.get("RS_DIST_BACKEND"):          # RS_DIST_BACKEND=gloo: several ranks rehearse on one GPU
        ndev = torch.cuda.device_count()
        if ndev < n:
            raise SystemExit(f"bench.py: --gpus {n} but only {ndev} ROCm device(s) visible")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out0 = []

    def spawn(r):
        return subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv],
                                env=supervise.rank_env(r, n, master_port=port),
                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def on_line(r, line):
        if r == 0 and line.lstrip().startswith("{"):      # stdout carries the ONE JSON line of rank 0; anything else
            out0.append(line)                             # (library chatter such as gloo's connection notes) goes to stderr
        elif line.strip():
            print(f"[rank {r}] {line}", file=sys.stderr, flush=True)

    supervise.supervise(spawn, n, on_line, "bench.py")     # raises RankFailure (a SystemExit) on the first dead rank
    for line in out0:
        print(line, flush=True)
    if not out0:
        raise SystemExit("bench.py: every rank exited 0 but rank 0 printed no JSON line")
    return 0


def per_rank_object(elapsed_s, units, steps, world):
    """every rank's own rate and step time (all ranks call this; VERDICT round 5, item 8: what makes a first 8-GPU run
    diagnosable): {min, max, argmin} of units/s over the ranks and each rank's ms_per_step, in rank order"""
    import torch.distributed as dist
    mine = (float(units) / elapsed_s, elapsed_s / steps * 1e3)
    if world > 1 and dist.is_available() and dist.is_initialized():
        objs = [None] * world
        dist.all_gather_object(objs, mine)
    else:
        objs = [mine]
    rates = [o[0] for o in objs]
    return {"min": round(min(rates), 1), "max": round(max(rates), 1), "argmin": int(np.argmin(rates)),
            "ms_per_step": [round(o[1], 4) for o in objs]}


def run_stub(args, rank, world):
    """The rank plumbing without a GPU (tests/test_bench_cpu.py): gloo, a fixed-cost host step, the same barriers,
    reductions and JSON contract."""
    if args.stub_fail_rank is not None and args.stub_fail_rank == rank:
        print(f"rank {rank}: simulated failure before the rendezvous (--stub-fail-rank)", file=sys.stderr, flush=True)
        os._exit(3)
    rdist.init(backend="gloo")
    B = args.batch
    for _ in range(args.warmup):
        time.sleep(0.001)
    rdist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002)
    rdist.barrier()
    mine = time.perf_counter() - t0
    elapsed = rdist.reduce_scalar(mine, "max")
    total = rdist.reduce_scalar(B * args.steps, "sum")
    per_rank = per_rank_object(mine, B * args.steps, args.steps, world)
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": round(total / elapsed, 1), "unit": "chunks/s", "n_gpus": world,
                          "per_rank": per_rank,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none",
                          "data": "stub", "config": {"workload": "stub step (rank plumbing rehearsal, no GPU)"}}),
              flush=True)
    rdist.finalize()
    return 0


# ---------------------------------------------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------------------------------------------
class Workload:
    """Resident inputs of one rank + step()."""

    def __init__(self, args, model, device, rank, world):
        from riser_amd.preprocess import pack_reads
        self.args, self.model, self.device = args, model, device
        B, L = args.batch, args.chunk
        cfg = args.config
        if cfg == "promethion":
            # the population is 18 000 x N read ids; this rank owns the ids that hash to it (crc32(id) % N)
            ids = np.arange(args.reads_per_gpu * world, dtype=np.int64)
            self.mine = rdist.shard_indices(ids, rank, world)
            n = int(self.mine.shape[0])
            base = synth.make_signals(SIG_SEED, 512, L)                  # read i carries the signal of i mod 512
            sigs = base[self.mine % 512]
            self.sample_sigs = sigs[: min(n, 512)]
            self.sig = torch.from_numpy(np.ascontiguousarray(sigs.reshape(-1))).to(device)
            self.n_reads, self.sub = n, B
            self.lens_host = np.full(n, L, dtype=np.int32)
            self.probs = torch.empty((1, n, 2), dtype=torch.float32, device=device)
            self.calls_per_step = -(-n // B)
            self.reads_per_step = n
            self.workload = (f"PromethION-scale population of {args.reads_per_gpu * world} x {L}-sample (4 s) int16 chunks, "
                             f"sharded by read id over {world} GPU(s) ({n} on rank 0), HBM-resident, walked in sub-batches of "
                             f"{B}" + (f" with {args.streams} in flight on separate HIP streams" if args.streams > 1 else "") +
                             f": MAD-normalise + 12-layer ConvNet forward + softmax, {args.dtype}")
        else:
            sigs = synth.make_signals(SIG_SEED, B, L, first_read=rank * B)   # each rank owns a different shard
            self.sample_sigs = sigs
            self.sig, self.off, self.ln, self.lens_host = pack_reads(list(sigs), device)
            if cfg == "progressive":
                self.lens_host = np.array([(L // 2, 3 * L // 4, L)[i % 3] for i in range(B)], dtype=np.int32)
                self.off = torch.from_numpy(np.arange(B, dtype=np.int64) * L).to(device)
                self.ln = torch.from_numpy(self.lens_host).to(device)
            self.probs = torch.empty((B, 2), dtype=torch.float32, device=device)
            self.calls_per_step = 1
            self.reads_per_step = B
            what = (f"mixed {L // 2} / {3 * L // 4} / {L}-sample (2 s / 3 s / 4 s) chunks in equal thirds, fused "
                    f"normalise + conv" if cfg == "progressive" else f"{L}-sample (4 s) int16 chunks")
            self.workload = (f"mRNA RNA004 model, batch={B} x {what} resident in HBM, MAD-normalise + 12-layer ConvNet "
                             f"forward + softmax, {args.dtype}")

    def step(self):
        if self.args.config == "promethion":
            from riser_amd.stream import classify_resident
            classify_resident([self.model], self.sig, self.n_reads, self.args.chunk, self.lens_host, self.sub,
                              out=self.probs, streams=self.args.streams)
        else:
            self.model.classify_raw(self.sig, self.off, self.ln, self.lens_host, out=self.probs)

    def outputs(self):
        """what the last step returned to its caller: the class probabilities of every read of the step, [reads, 2]"""
        return {"probs": self.probs.reshape(-1, 2).cpu().numpy()}


def algorithmic_bytes_per_step(channels, lens, esize, fused01=True):
    """HBM bytes the conv stack must move per step if every layer reads its input and writes its pooled output once
    (layer-fused figure; layers 0+1 as one launch: the normalised signal in, layer 1's output out)."""
    tot = 0.0
    for n in lens:
        n = int(n)
        if fused01:
            tot += 4.0 * n + channels[1] * (n >> 2) * esize
            first = 2
        else:
            tot += 4.0 * n + channels[0] * (n >> 1) * esize
            first = 1
        for i in range(first, len(channels)):
            tot += (channels[i - 1] * (n >> i) + channels[i] * (n >> (i + 1))) * esize
    return tot


def traffic_object(args, model, wl):
    """HBM-side bytes of the conv stack per step from the TRACKED rocprofv3 PMC passes of this tree's kernels
    (profiles/rNN_pmc_fetch_write_<mode>.json: FETCH_SIZE and WRITE_SIZE in separate --pmc runs of this same command,
    KiB per dispatch, FETCH doubled for gfx950 as MI355X_MICROARCH.md prescribes).  Counters cannot be read from inside a
    run, so the figure is the profiled run's, valid for the same workload (config, dtype, batch, chunk)."""
    tag = {"f32": "f32", "bf16x3": "bf16x3", "f16xf8": "f16xf8"}.get(args.dtype) if args.config == "rna004_b512" else (
        "prog" if args.config == "progressive" and args.dtype == "f16x3" else None)
    if tag is None or args.batch != BATCH or args.chunk != CHUNK:
        return None
    path = os.path.join(ROOT, "profiles", f"{PROFILE_ROUND}_pmc_fetch_write_{tag}.json")    # this round's pass only
    if not os.path.exists(path):
        return None
    with open(path) as f:
        pmc = json.load(f)
    from riser_amd.build import csrc_sha16
    stamp = (pmc.get("_meta") or {}).get("csrc_sha16")
    fresh = stamp is not None and stamp == csrc_sha16()
    conv = {k: v for k, v in pmc.items() if k.startswith("conv_")}
    if not conv:
        return None
    steps = max(v["dispatches"] for k, v in conv.items() if "stream" in k) if any("stream" in k for k in conv) else None
    if not steps:
        return None
    fetched = sum(2.0 * v.get("FETCH_SIZE", 0.0) * 1024 * v["dispatches"] for v in conv.values()) / steps
    written = sum(v.get("WRITE_SIZE", 0.0) * 1024 * v["dispatches"] for v in conv.values()) / steps
    launches = sum(v["dispatches"] for v in conv.values()) / steps
    esize = 4 if args.dtype in ("f32", "f32_direct") else (4 if args.dtype in ("bf16x3", "f16x3", "f16xf8") else 2)
    alg = algorithmic_bytes_per_step(model.channels, wl.lens_host, esize, fused01=args.dtype == "f32")
    if args.dtype != "f32":                               # 16-bit modes: layers 0+1+2 are one launch
        alg = sum(4.0 * int(n) + model.channels[2] * (int(n) >> 3) * esize +
                  sum((model.channels[i - 1] * (int(n) >> i) + model.channels[i] * (int(n) >> (i + 1))) * esize
                      for i in range(3, model.n_layers)) for n in wl.lens_host)
    return {"bytes_per_launch": round((fetched + written) / launches, 1), "launches_per_step": round(launches, 2),
            "bytes_per_step": round(fetched + written, 1), "fetched_bytes_per_step": round(fetched, 1),
            "written_bytes_per_step": round(written, 1), "algorithmic_bytes_per_step": round(alg, 1),
            "ratio_to_algorithmic": round((fetched + written) / alg, 3), "fetch_doubled_for_gfx950": True,
            "source": os.path.relpath(path, ROOT), "profiled_csrc_sha16": stamp, "kernels_match_tree": fresh}


def roofline_object(args, model, wl, conv_ms_total, conv_calls, launches=None):
    """conv stack = layers 1..n-1.  conv_ms_total: HIP-event time of the conv stack summed over `conv_calls` library
    calls of the timed region; launches: (stage_ms, detail_calls) of the per-launch pass (--full), or None: no per-layer
    and per-stage figures."""
    lib_dtype = LIB_DTYPE.get(args.dtype, args.dtype)
    L = args.chunk
    nl = model.n_layers
    lens = wl.lens_host
    reads_per_call = wl.reads_per_step / wl.calls_per_step
    # algorithmic FLOPs of one step: per read, by its own length
    per_len = {int(n): conv_flops_per_chunk(model.channels, int(n)) for n in np.unique(lens)}
    layer_flop_step = [sum(per_len[int(n)][i] * int((lens == n).sum()) for n in per_len) for i in range(nl)]
    conv_flop_step = float(sum(layer_flop_step[1:]))
    steps_timed = conv_calls / wl.calls_per_step if wl.calls_per_step else 0
    conv_ms_step = conv_ms_total / steps_timed if steps_timed else 0.0
    info = model.layer_info()
    passes = MFMA_PASSES.get(args.dtype, 1)
    stage_ms, detail_calls = launches if launches is not None else (None, 0)
    per_layer, executed_step = [], 0.0
    for i in range(1, nl):
        U = info[i]["block_samples"]                                             # packed layout: len // U + 1 blocks per read,
        blocks_step = int((lens.astype(np.int64) // U + 1).sum())               # finer blocks below the last three layers
        rows = blocks_step * -(-(U >> i) // info[i]["gemm_row_div"])              # GEMM rows of a step
        ex = 2.0 * rows * info[i]["n_pad"] * info[i]["k_pad"] * passes
        executed_step += ex
        if stage_ms is None:
            continue
        ms = float(stage_ms[1 + i]) / max(detail_calls, 1)                       # per library call
        fl_call = layer_flop_step[i] / wl.calls_per_step
        per_layer.append({"layer": i, "ms": round(ms, 4),
                          "algorithmic_tflops": round(fl_call / (ms * 1e-3) / 1e12, 2) if ms > 0 else None,
                          "executed_tflops": round(ex / wl.calls_per_step / (ms * 1e-3) / 1e12, 2) if ms > 0 else None,
                          "tile": [info[i]["bm"], info[i]["bn"], info[i]["kc"]]})
    traffic = traffic_object(args, model, wl)
    alg_tf = conv_flop_step / (conv_ms_step * 1e-3) / 1e12 if conv_ms_step > 0 else 0.0
    exe_tf = executed_step / (conv_ms_step * 1e-3) / 1e12 if conv_ms_step > 0 else 0.0
    peak = PEAK_F32_MFMA_TF if args.dtype in ("f32", "f32_direct") else PEAK_BF16_MFMA_TF
    f23 = [str(i) for i in range(1, nl) if info[i]["gemm_row_div"] == 2]
    f43 = [str(i) for i in range(1, nl) if info[i]["gemm_row_div"] == 4]
    kname = {"f32w": "conv_stream_f32_kernel / conv_wino_kernel / conv_wino4_kernel (Winograd F(2,3) layers %s, F(4,3) "
                     "layers %s, f32-input MFMA)" % (",".join(f23), ",".join(f43)),
             "f32": "conv_f32_kernel (direct, f32-input MFMA)"}.get(lib_dtype, "16-bit MFMA conv kernels (%s)" % lib_dtype)
    overlap = ({"streams_note": f"{args.streams} sub-batches in flight: the per-call HIP-event times overlap, so `achieved` / `frac` "
                                "(FLOPs over the SUM of those times) understate the pipe's share; use --streams 1 for the roofline"}
               if getattr(args, "streams", 1) > 1 else {})
    roof = {**overlap, "bound": "mfma", "kernel": kname + f", {nl - 1} launches per call, layers 1-{nl - 1}",
            "achieved": round(exe_tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(exe_tf / peak, 4),
            # counters of OTHER kernel sources are not this tree's traffic: null, the stale figure stays in traffic_detail
            "traffic": traffic["bytes_per_launch"] if traffic and traffic["kernels_match_tree"] else None,
            "traffic_detail": traffic,
            "traffic_note": "HBM-side bytes per conv launch (FETCH_SIZE x 2 + WRITE_SIZE) from the tracked rocprofv3 PMC passes of "
                            "this same command (traffic_detail.source): counters cannot be collected from inside a run; null "
                            "for workloads without a tracked pass",
            "achieved_note": "MFMA FLOPs the kernels execute (tile padding included; Winograd F(2,3) issues 2/3, F(4,3) 1/2 "
                             "of the direct convolution's multiplications; split-precision modes three MFMAs per product) / "
                             "HIP-event time of the conv stack inside the timed steps",
            "algorithmic_tflops": round(alg_tf, 2),
            "algorithmic_note": f"direct-convolution FLOPs of layers 1-{nl - 1} (SURVEY.md 8(d): 582.95 MFLOP per 16000-sample "
                                "chunk) over the same time; can exceed the MFMA peak under Winograd, so it is not the fraction",
            "avg_launch_ms": round(conv_ms_step / wl.calls_per_step / (nl - 1), 4) if wl.calls_per_step else None,
            "conv_stack_ms_per_call": round(conv_ms_step / wl.calls_per_step, 4) if wl.calls_per_step else None,
            "reads_per_call": round(reads_per_call, 1),
            "timing_note": "achieved / avg_launch_ms: HIP events around the conv stack inside the timed steps; stage_ms and "
                           "layers[] (--full): a separate pass with one event per launch (each event adds ~4.5 us of stream "
                           "time)"}
    if stage_ms is not None:
        conv_ms_detail = float(stage_ms[2:2 + nl - 1].sum()) / max(detail_calls, 1)
        roof.update({"conv_stack_ms_per_launch_events": round(conv_ms_detail, 4),
                     "stage_ms": {"normalise": round(float(stage_ms[0]) / max(detail_calls, 1), 4),
                                  "conv0": round(float(stage_ms[1]) / max(detail_calls, 1), 4),
                                  "conv1_11": round(conv_ms_detail, 4),
                                  "head": round(float(stage_ms[nl + 1]) / max(detail_calls, 1), 4)},
                     "layers": per_layer})
    return roof


def _longest_run(sig: np.ndarray) -> int:
    """longest run of consecutive |y| > 3.5 samples of a raw read after MAD normalisation (numpy; a statistic for the JSON)"""
    x = sig.astype(np.float64)
    med = np.median(x)
    mad = np.median(np.abs(x - med))
    if mad == 0:
        return 0
    o = np.abs((x - med) / (1.4826 * mad)) > 3.5
    edges = np.flatnonzero(np.diff(np.concatenate([[0], o.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[0::2]).max()) if edges.size else 0


def sustained_object(step, device, B, headline):
    """the headline's step over a window of >= 2 s (the timed region is K steps = tens of milliseconds): chunks/s and its
    ratio to the K-step figure"""
    t1 = time.perf_counter()
    n = 0
    while True:
        for _ in range(100):
            step()
        n += 100
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t1
        if dt >= 2.0:
            break
    v = n * B / dt
    return {"value": round(v, 1), "window_s": round(dt, 2), "steps": n, "ratio_to_headline": round(v / headline, 4)}


def host_fed_object(args, device, model, wl, lib_dtype, headline):
    """the same 512 x 16000 batches fed from PINNED HOST memory through riser_amd.stream.StreamClassifier: the upload of batch
    k + 1 runs on a copy stream under the kernels of batch k, the probabilities come back to pinned memory ("from
    int16 batch resident in pinned host memory").  chunks/s over N_BATCH batches, per arithmetic mode."""
    from riser_amd.model import Model
    from riser_amd.stream import StreamClassifier
    B, L = args.batch, args.chunk
    n_batch = 48
    pop = torch.from_numpy(np.ascontiguousarray(wl.sample_sigs)).pin_memory()                  # one batch, walked n_batch times
    pinned = torch.empty((n_batch * B, L), dtype=torch.int16).pin_memory()
    for k in range(n_batch):
        pinned[k * B:(k + 1) * B].copy_(pop)
    out = {"batches": n_batch, "pinned_mb": round(pinned.numel() * 2 / 1e6, 1)}
    for dt in ("f32", "bf16x3", "f16xf8"):
        ldt = LIB_DTYPE.get(dt, dt)
        if ldt not in Model.dtypes():
            continue
        m = model if ldt == lib_dtype else Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=ldt, device=device)
        sc = StreamClassifier([m], sub_batch=B, max_len=L)
        sc.classify(pinned)                                            # one untimed pass: a pinned page's FIRST upload is slow (8.9 ms per
        torch.cuda.synchronize(device)                                 # 16 MB batch on a fresh allocation), the per-stream workspaces
        times = []
        for _ in range(3):                                             # median of three passes over the whole population
            t1 = time.perf_counter()
            probs = sc.classify(pinned)
            times.append(time.perf_counter() - t1)
        dtw = float(np.median(times))
        e = {"value": round(n_batch * B / dtw, 1), "ms_per_batch": round(dtw / n_batch * 1e3, 4),
             "passes_ms_per_batch": [round(t / n_batch * 1e3, 4) for t in times]}
        if ldt == lib_dtype:
            e["ratio_to_resident"] = round(e["value"] / headline, 4)
            e["bits_equal_resident"] = bool(np.array_equal(probs[0, :B], wl.probs.cpu().numpy()))
        out[dt] = e
        if m is not model:
            m.close()
    return out


def side_variants(args, device, wl, ref):
    """The same 512-read batch through the other arithmetic modes, the 3-model ensemble (config 3) and the mixed-length
    batch (config 5): throughput, and distance of the probabilities from the fp32 result of this run."""
    from riser_amd.model import Model, classify_raw_ensemble
    from riser_amd import _native as nv
    B, L = args.batch, args.chunk
    sig, off, ln, lens = wl.sig, wl.off, wl.ln, wl.lens_host
    variants = {}

    def timed(fn):
        for _ in range(max(3, min(args.warmup, 10))):
            fn()
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t1) / args.steps

    def versus_ref(p):
        return {"max_abs_dprob_vs_f32": float(np.abs(p - ref).max()),
                "label_flips_at_0.9_vs_f32": int(((p[:, 1] > 0.9) != (ref[:, 1] > 0.9)).sum())}

    for dt in ("f32", "bf16x3", "f16x3", "f16xf8", "f16", "bf16"):
        if dt not in Model.dtypes():
            continue
        mv = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=dt, device=device)
        if dt in ("f16", "bf16"):
            mv.autotune(sig, off, ln, lens)      # optional per-geometry tile tuning (fp32: the planner's picks stand)
        pv = torch.empty((B, 2), dtype=torch.float32, device=device)
        dtv = timed(lambda: mv.classify_raw(sig, off, ln, lens, out=pv))
        entry = {"chunks_per_s": round(B / dtv, 1), "ms_per_step": round(dtv * 1e3, 4), "batch": B, **versus_ref(pv.cpu().numpy())}
        if dt == "bf16x3":                       # thin batches in split precision too (the fp32 figures: thin_batches_f32 below)
            thin3 = {}
            for tb in (1, 16, 32, 64):
                t_lens = np.full(tb, L, dtype=np.int32)
                t_off = torch.from_numpy(np.arange(tb, dtype=np.int64) * L).to(device)
                t_len = torch.from_numpy(t_lens).to(device)
                pt = torch.empty((tb, 2), dtype=torch.float32, device=device)
                thin3[str(tb)] = round(timed(lambda: mv.classify_raw(sig, t_off, t_len, t_lens, out=pt)) * 1e3, 4)
            variants["thin_batches_bf16x3"] = {"ms_per_step_by_reads": thin3, "chunk_samples": L}
        if dt in ("f16", "bf16"):                # plain 16-bit: fast, outside the 1e-3 tolerance
            variants.setdefault("approximate", {})[dt] = entry
        else:
            variants["f32_direct" if dt == "f32" else dt] = entry
        mv.close()
    # two batches in flight: the same 512-read call alternately on two HIP streams (per-stream workspaces).  The idle CUs
    # of one batch's tile rounds, prologues and launch boundaries run the other's work; throughput-oriented callers
    # (stream.classify_resident(streams=2), BASELINE config 4) use it, the headline and the control loop do not
    for dt in ("f32", "bf16x3"):
        mv = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=LIB_DTYPE.get(dt, dt), device=device)
        pv2 = [torch.empty((B, 2), dtype=torch.float32, device=device) for _ in range(2)]
        side = [torch.cuda.Stream(device=device) for _ in range(2)]
        turn = [0]

        def two():
            k = turn[0] = turn[0] ^ 1
            with torch.cuda.stream(side[k]):
                mv.classify_raw(sig, off, ln, lens, out=pv2[k])
        for st_ in side:
            st_.wait_stream(torch.cuda.current_stream(device))
        dt2 = timed(two)
        for st_ in side:
            torch.cuda.current_stream(device).wait_stream(st_)
        variants["two_batches_in_flight_" + dt] = {"chunks_per_s": round(B / dt2, 1), "ms_per_step": round(dt2 * 1e3, 4),
                                                   "batch": B, "streams": 2, **versus_ref(pv2[0].cpu().numpy())}
        mv.close()
    # BASELINE config 3: three-model ensemble, normalise once + three forwards + decision on the device
    for dt in ("bf16x3", "f16xf8", "bf16"):
        if dt not in Model.dtypes():
            continue
        ens = [Model(synth.make_state_dict(sd_), synth.Config(), None, t_, dtype=dt, device=device)
               for sd_, t_ in ((1, "mRNA"), (2, "mtRNA"), (3, "globin"))]
        if dt == "bf16":
            for mk in ens:
                mk.autotune(sig, off, ln, lens)
        pe = torch.empty((3, B, 2), dtype=torch.float32, device=device)
        dec = torch.empty(B, dtype=torch.uint8, device=device)
        dte = timed(lambda: classify_raw_ensemble(ens, sig, off, ln, lens, out=pe, decision=dec, max_len=L,
                                                  threshold=0.9, mode=nv.RS_ENRICH))
        entry = {"reads_per_s": round(B / dte, 1), "model_forwards_per_s": round(3 * B / dte, 1),
                 "ms_per_step": round(dte * 1e3, 4), "batch": B, "accepted": int((dec == 1).sum().item()),
                 "model0": versus_ref(pe[0].cpu().numpy())}
        if dt in ("bf16x3", "f16xf8"):
            variants["ensemble3_" + dt] = entry                    # BASELINE config 3 (the modes that meet 1e-3)
        else:                                                      # plain bf16 misses the tolerance: not config 3
            variants.setdefault("approximate", {})["ensemble3_bf16"] = entry
        for mk in ens:
            mk.close()
    # BASELINE config 5: progressive 2 s / 3 s / 4 s chunks in equal thirds of one batch, f16: per-read lengths
    # are carried through every layer, no bucketing
    mix_lens = np.array([(L // 2, 3 * L // 4, L)[i % 3] for i in range(B)], dtype=np.int32)
    mix_off = torch.from_numpy((np.arange(B, dtype=np.int64) * L)).to(device)
    mix_len = torch.from_numpy(mix_lens).to(device)
    mm = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype="f16", device=device)
    pm = torch.empty((B, 2), dtype=torch.float32, device=device)
    mm.autotune(sig, mix_off, mix_len, mix_lens)
    dtm = timed(lambda: mm.classify_raw(sig, mix_off, mix_len, mix_lens, out=pm))
    variants.setdefault("approximate", {})["mixed_2s_3s_4s_f16"] = {
        "chunks_per_s": round(B / dtm, 1), "ms_per_step": round(dtm * 1e3, 4), "batch": B, "samples_per_step": int(mix_lens.sum())}
    mm.close()
    for dt in ("f16x3", "f16xf8"):
        mm = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=dt, device=device)
        dtm = timed(lambda: mm.classify_raw(sig, mix_off, mix_len, mix_lens, out=pm))
        variants["mixed_2s_3s_4s_" + dt] = {"chunks_per_s": round(B / dtm, 1), "ms_per_step": round(dtm * 1e3, 4), "batch": B,
                                            "samples_per_step": int(mix_lens.sum())}
        mm.close()
    # the live ReadUntil shape: ~357 assessable reads per 512-channel batch, capped at the RNA004 maximum of 8615 samples
    # (riser/preprocess.py:36-37): 3 blocks of 4096 per read in the packed layout
    lb, ll = 357, 8615
    live_lens = np.full(lb, ll, dtype=np.int32)
    live_off = torch.from_numpy(np.arange(lb, dtype=np.int64) * L).to(device)
    live_len = torch.from_numpy(live_lens).to(device)
    ml = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype="f32w", device=device)
    pl = torch.empty((lb, 2), dtype=torch.float32, device=device)
    dtl = timed(lambda: ml.classify_raw(sig, live_off, live_len, live_lens, out=pl))
    variants["live_357x8615_f32"] = {"reads_per_s": round(lb / dtl, 1), "ms_per_step": round(dtl * 1e3, 4), "batch": lb,
                                     "samples_per_read": ll}
    # thin batches (a chunk client delivers ~20 assessable reads per batch, riser/control.py:31-93; Model.classify is batch 1,
    # riser/model.py:22-28): whole-step time of 1 / 16 / 32 / 64 reads of 16000 samples
    thin = {}
    for tb in (1, 16, 32, 64):
        t_lens = np.full(tb, L, dtype=np.int32)
        t_off = torch.from_numpy(np.arange(tb, dtype=np.int64) * L).to(device)
        t_len = torch.from_numpy(t_lens).to(device)
        pt = torch.empty((tb, 2), dtype=torch.float32, device=device)
        thin[str(tb)] = round(timed(lambda: ml.classify_raw(sig, t_off, t_len, t_lens, out=pt)) * 1e3, 4)
    variants["thin_batches_f32"] = {"ms_per_step_by_reads": thin, "chunk_samples": L}
    # the same shape on the signals the control-loop replay carries (synth.make_raw_read: adapter + poly(A) plateau + squiggle,
    # trimmed as riser/control.py:36-60 trims: behind the poly(A) end, or at the fixed offset when none is found - which leaves a
    # plateau of ~3000 consecutive outliers in front of the squiggle).  Data-dependent only through the normalise kernel's walk
    # of outlier runs (one lane per run cost such a batch 0.8 ms until round 4)
    from riser_amd.preprocess import pack_reads
    from riser_amd import Kit, SignalProcessor
    whole = [synth.make_raw_read(4242, rid, 18000 + 11 * (rid % 97), polya=(rid % 5 != 0)) for rid in range(lb)]
    kit = SignalProcessor(Kit.create_from_version("RNA004"), device=device)
    ends = kit.get_polyA_end_batch(whole)                     # the GPU detector; -1 where the reference returns None
    raw = []
    for s, end in zip(whole, ends.tolist()):
        start = min(end + 1 if end > 0 else kit.get_fixed_trim_length(), s.shape[0] - ll)
        raw.append(np.ascontiguousarray(s[start: start + ll]))
    rsig, roff, rln, rlh = pack_reads(raw, device)
    dtp = timed(lambda: ml.classify_raw(rsig, roff, rln, rlh, out=pl))
    variants["live_357x8615_f32_replay_signals"] = {"reads_per_s": round(lb / dtp, 1), "ms_per_step": round(dtp * 1e3, 4),
                                                    "batch": lb, "samples_per_read": ll,
                                                    "reads_with_a_run_over_1000_outliers": int(sum(_longest_run(r) > 1000 for r in raw))}
    ml.close()
    # the reference's secondary architecture (riser/nets/resnet.py; no shipped config or weights): a SquiggleNet-like
    # basic-block ResNet through the generic conv program (csrc/seqnet.hip: f32-input MFMA, weights resident in LDS)
    import types
    from riser_amd.resnet import ResNetModel, build_program, program_flops, program_traffic_bytes
    rcfg = synth.RESNET_BENCH_CFG
    rsd = synth.make_resnet_state_dict(7)
    xr = torch.from_numpy(np.stack([np.clip((s.astype(np.float32) - 500.0) / 60.0, -3.5, 3.5)
                                    for s in wl.sample_sigs[:64]])).to(device).repeat(B // 64, 1).contiguous()
    rprog = build_program(rsd, types.SimpleNamespace(**rcfg))[0]
    fl = program_flops(rprog, L) * xr.shape[0]
    by = program_traffic_bytes(rprog, L, fused=True) * xr.shape[0]
    by_unfused = program_traffic_bytes(rprog, L, fused=False) * xr.shape[0]
    rprobs = {}
    for rdt, peak in (("f32", PEAK_F32_MFMA_TF), ("bf16x3", PEAK_BF16_MFMA_TF)):
        rm = ResNetModel(rsd, types.SimpleNamespace(resnet=types.SimpleNamespace(**rcfg)), None, "x", device=device, dtype=rdt)
        dtr = timed(lambda: rm._net.forward(xr))
        rprobs[rdt] = rm._net.forward(xr).cpu().numpy()
        entry = {"chunks_per_s": round(xr.shape[0] / dtr, 1), "ms_per_step": round(dtr * 1e3, 4),
                 "batch": int(xr.shape[0]), "config": rcfg,
                 "conv_tflops": round(fl / dtr / 1e12, 2),
                 "roofline_frac_mfma": round(fl / dtr / 1e12 / peak, 4),
                 "hbm_gb_per_step": round(by / 1e9, 3), "hbm_gb_per_step_unfused": round(by_unfused / 1e9, 3),
                 "hbm_tb_per_s": round(by / dtr / 1e12, 3), "roofline_frac_hbm": round(by / dtr / 8e12, 4)}
        if rdt == "f32":
            entry["roofline_frac_f32_mfma"] = entry["roofline_frac_mfma"]
            entry["note"] = ("one launch per residual block (conv-BN-ReLU, conv-BN, 1x1 shortcut, add, ReLU) and one for the stem "
                             "(conv-BN-ReLU-MaxPool): x in, y out per launch (hbm_gb_per_step, algorithmic); conv_tflops = un-padded "
                             "conv FLOPs / step time over the 157.3 TF f32 MFMA peak (channel widths of 20-67 pad to 32-80 columns)")
        else:
            entry["max_abs_dprob_vs_f32"] = float(np.abs(rprobs["bf16x3"] - rprobs["f32"]).max())
            entry["label_flips_at_0.9_vs_f32"] = int(((rprobs["bf16x3"][:, 1] > 0.9) != (rprobs["f32"][:, 1] > 0.9)).sum())
            entry["note"] = ("the same program with its stem and residual basic blocks in split precision on the bf16 MFMA "
                             "(rs_seqnet_set_mode): three v_mfma_f32_16x16x32_bf16 per product, activations fp32 between launches; "
                             "frac over the 2.5 PF bf16 peak - the blocks are bound by the split's VALU work and their epilogues")
        variants["resnet_basic_" + rdt] = entry
        if rdt == "bf16x3":
            # a live ReadUntil batch through the ResNet: 357 reads, lengths anywhere in [4096, 8615] (riser/control.py:36-60),
            # ONE ragged forward (rs_seqnet_forward_ragged) - against one forward per distinct length before round 5
            rng = np.random.default_rng(3)
            rl = rng.integers(4096, 8616, size=357).astype(np.int32)
            xl = xr[:357, :8615].contiguous()
            rl_dev = torch.from_numpy(rl).to(device)
            dtl_ = timed(lambda: rm._net.forward_ragged(xl, rl_dev))
            variants["resnet_live_ragged_357_bf16x3"] = {"reads_per_s": round(357 / dtl_, 1), "ms_per_step": round(dtl_ * 1e3, 4),
                                                         "batch": 357, "samples_per_step": int(rl.sum()),
                                                         "distinct_lengths": int(np.unique(rl).size)}
        rm.close()
    return variants


def control_loop_object(device, dtype):
    """ReadUntil replay (riser_amd/replay.py): scripted AccumulatingCache traffic through the batched SequencerControl
    with 1 and 3 models at 512 channels (MinION) and with 1 model at 18 000 channels (a PromethION-scale batch, the
    per-GPU share of BASELINE config 4); what the 1 s decision window has to cover."""
    from riser_amd.model import Model
    from riser_amd.preprocess import Kit, SignalProcessor
    from riser_amd.replay import run_replay, scripted_batches
    from riser_amd.fake_client import PlainFakeClient
    from riser_amd.replay import chunked_batches
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=device)
    batches = scripted_batches(260, 512)
    out = {"kit": "RNA004", "channels": 512, "dtype": dtype, "window_s": 1.0,
           "note": "p50 / p99 / max_ms: host wall time per ReadUntil batch from get_read_batch() to the reject / finish calls "
                   "(riser/control.py:31-106): upload of the new samples of every read, poly(A) scan, gating, normalise, one "
                   "forward per model, decision; loop_*: the whole iteration including the batch's CSV rows (written after "
                   "the calls); first 3 batches dropped as warm-up (first_ms lists them); the garbage collector is frozen over "
                   "the scripted batches (gc_frozen).  Traffic: every channel re-sends its read whole, 1600 samples longer per "
                   "batch (an accumulating client); models_1_chunk_traffic: a client that pops its cache, disjoint 2 s chunks "
                   "under one read id (what riser/client.py:44 delivers) - the signal store detects it and uploads whole reads"}
    spec = list(zip((1, 2, 3), ("mRNA", "mtRNA", "globin")))
    for n_models in (1, 3):
        models = [Model(synth.make_state_dict(s), synth.Config(), None, t, dtype=dtype, device=device) for s, t in spec[:n_models]]
        out[f"models_{n_models}"] = run_replay(models, proc, batches)
        if n_models == 1:
            # the same replay with every read re-uploaded whole each batch (no device-resident signals): what the
            # signal store saves (the part of it that pays)
            out["models_1_full_reupload"] = run_replay(models, proc, batches, signal_cache=False)
            # the eight-method duck type only (one get_raw_signal call per read) instead of the C host loops
            out["models_1_python_host_loops"] = run_replay(models, proc, batches, client_cls=PlainFakeClient)
            out["models_1_chunk_traffic"] = run_replay(models, proc, chunked_batches(260, 512))
        for m in models:
            m.close()
    # the same loop with the models in split precision (bf16x3: within 1e-3 of the reference, labels identical - the mode of
    # BASELINE config 3): the device share of a batch halves
    for n_models in (1, 3):
        models = [Model(synth.make_state_dict(s), synth.Config(), None, t, dtype="bf16x3", device=device) for s, t in spec[:n_models]]
        out[f"models_{n_models}_bf16x3"] = run_replay(models, proc, batches)
        for m in models:
            m.close()
    # the reference's second architecture behind the same loop (riser/nets/resnet.py; `Model` with a `resnet:` config): ragged
    # batches are one forward (rs_seqnet_forward_ragged), stem and residual blocks in split precision on the bf16 MFMA
    import types
    rcfg = types.SimpleNamespace(model="resnet", resnet=types.SimpleNamespace(**synth.RESNET_BENCH_CFG))
    models = [Model(synth.make_resnet_state_dict(7), rcfg, None, "mRNA", dtype="bf16x3", device=device)]
    out["models_1_resnet_bf16x3"] = run_replay(models, proc, batches)
    models[0].close()
    del batches
    big = scripted_batches(60, 18000)
    models = [Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=dtype, device=device)]
    out["promethion_18000_channels"] = run_replay(models, proc, big)
    out["promethion_18000_channels_full_reupload"] = run_replay(models, proc, big, signal_cache=False)
    models[0].close()
    return out


def run_promethion_live(args, model, lib_dtype, device, rank, world):
    """BASELINE config 4 as a running system: one control loop per rank, each on its own channel range."""
    import gc
    import logging
    import tempfile
    from riser_amd.control import PHASES, SequencerControl
    from riser_amd.fake_client import FakeClient
    from riser_amd.launch import rank_channel_range
    from riser_amd.preprocess import Kit, SignalProcessor
    from riser_amd.replay import scripted_batches
    per_rank = args.reads_per_gpu
    first, last = rank_channel_range(rank, world, per_rank * world)
    proc = SignalProcessor(Kit.create_from_version("RNA004"), device=device)
    W, K = max(args.warmup, 1), args.steps
    client = FakeClient(scripted_batches(W, per_rank, first_channel=first), first_channel=first, last_channel=last)
    timed = scripted_batches(K, per_rank, first_channel=first, first_batch=W)

    def csv_rows(path):
        with open(path) as f:
            return sum(1 for ln in f if not ln.startswith("batch_start"))

    with tempfile.TemporaryDirectory() as d:
        out_file = os.path.join(d, f"live.rank{rank}")
        ctl = SequencerControl(client, [model], proc, logging.getLogger("riser_amd.bench"), out_file)
        ctl.reserve(per_rank)
        ctl.start()
        gc.collect()
        gc.freeze()              # the scripted batches are ~1e6 long-lived objects a live run never holds (riser_amd/replay.py)
        try:
            ctl.target("enrich", 1.0, 0.9)                          # W untimed batches
            n_warm, rows_warm = len(ctl.batch_latencies), csv_rows(out_file + ".csv")
            client.extend(timed)
            torch.cuda.synchronize(device)
            rdist.barrier(device)
            t0 = time.perf_counter()
            ctl.target("enrich", 1.0, 0.9)                          # exactly K batches
            torch.cuda.synchronize(device)
            rdist.barrier(device)
            elapsed = time.perf_counter() - t0
        finally:
            gc.unfreeze()
        ctl.finish()
        rows_timed = csv_rows(out_file + ".csv") - rows_warm
    if args.dump_outputs:                     # what the client was sent for the last timed batch: the reads' channels
        write_outputs(args.dump_outputs, {k: np.array([ch for ch, _ in getattr(client, k)[-1]], dtype=np.float64)
                                          for k in ("rejected", "finished")}, rank)
    lat = np.asarray(list(ctl.batch_latencies)[n_warm:]) * 1e3
    loop = np.asarray(list(ctl.batch_loop_times)[n_warm:]) * 1e3
    phases = np.asarray(list(ctl.batch_phases)[n_warm:]).reshape(-1, len(PHASES)) * 1e3
    elapsed = rdist.reduce_scalar(elapsed, "max", device)
    received = rdist.reduce_scalar(per_rank * K, "sum", device)
    p99 = rdist.reduce_scalar(float(np.percentile(lat, 99)) if lat.size else 0.0, "max", device)
    rows_timed = rdist.reduce_scalar(rows_timed, "sum", device)
    if rank != 0:
        rdist.finalize()
        return 0
    out = {"metric": "reads assessed/sec through the live ReadUntil control loop (PromethION-scale flow cell, RNA004)",
           "value": round(rows_timed / elapsed, 1), "unit": "reads/s", "n_gpus": world, "steps": K, "warmup": W,
           "ms_per_step": round(elapsed / K * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32" if lib_dtype in ("f32", "f32w") else lib_dtype, "data": "synthetic",
           "config": {"workload": f"live control loop, {per_rank} channels per rank of a {per_rank * world}-channel flow cell "
                                  f"(rank r drives channels [r x {per_rank} + 1, (r + 1) x {per_rank}]), scripted AccumulatingCache "
                                  "traffic (every read re-sent whole, 1600 samples longer per batch), 1 model: upload of the new "
                                  "samples, poly(A) scan, gating, MAD-normalise + 12-layer ConvNet forward + softmax, decision, "
                                  f"client calls, CSV rows; {lib_dtype}",
                      "name": args.config, "channels_per_rank": per_rank, "sharding": "channel ranges across ranks, no collectives"},
           "reads_received_per_s": round(received / elapsed, 1),
           "p50_batch_latency_ms": round(float(np.percentile(lat, 50)), 3) if lat.size else None,
           "p99_batch_latency_ms": round(p99, 3), "latency_samples": int(lat.size),
           "loop_p50_ms": round(float(np.percentile(loop, 50)), 3) if loop.size else None,
           "latency_note": "rank 0's p50, max over ranks of p99: host wall time per ReadUntil batch from get_read_batch() to the "
                           "reject / finish calls (riser/control.py:31-106); loop_p50_ms includes the CSV rows; gc frozen over the "
                           "scripted batches",
           "phase_ms_median": {n: round(float(v), 3) for n, v in zip(PHASES, np.median(phases, axis=0))} if phases.size else {},
           "gc_frozen": True, "window_s": 1.0, "roofline": None,
           "roofline_note": "a host + PCIe + device pipeline, not one kernel: the device share is phase_ms_median.device_wait "
                            "(the kernels' own roofline is the rna004_b512 line)"}
    print(json.dumps(out), flush=True)
    rdist.finalize()
    return 0


def cpu_baseline_object(args, sigs):
    """The oracle's torch-CPU port (kind "port") on this box's host cores: (A) the reference's structure, one read at a
    time (riser/control.py:63-69), and (B) the same ops batched at 64; each at several thread counts, best reported."""
    from oracle import riser_oracle as ro
    from oracle import torch_path
    ncpu = os.cpu_count() or 1
    cpu_model = torch_path.TorchCpuModel(synth.make_state_dict(1))
    counts = sorted({c for c in (8, 32, ncpu) if 1 <= c <= ncpu})
    budget = max(args.cpu_seconds, 6.0)
    per_a, per_b = budget * 0.55 / len(counts), budget * 0.45 / len(counts)
    B = sigs.shape[0]
    sweep = {}
    torch_path.classify_per_read(cpu_model, sigs[:2])                    # warm-up
    for c in counts:
        torch.set_num_threads(c)
        torch_path.classify_per_read(cpu_model, sigs[:1])
        n_done, t1 = 0, time.perf_counter()
        while n_done < B and time.perf_counter() - t1 < per_a:
            torch_path.classify_per_read(cpu_model, sigs[n_done:n_done + 4])
            n_done += 4
        dt = time.perf_counter() - t1
        nb, tb0 = 0, time.perf_counter()
        while nb < B and time.perf_counter() - tb0 < per_b:
            xs = np.stack([ro.mad_normalise(s) for s in sigs[nb:nb + 64]]).astype(np.float32)
            torch.softmax(cpu_model.logits(torch.from_numpy(xs)), dim=1)
            nb += 64
        dtb = time.perf_counter() - tb0
        sweep[str(c)] = {"per_read": round(n_done / dt, 2), "per_read_chunks": n_done,
                         "batched64": round(nb / dtb, 2), "batched64_chunks": nb}
    best_a = max(sweep, key=lambda k: sweep[k]["per_read"])
    best_b = max(sweep, key=lambda k: sweep[k]["batched64"])
    return {"value": sweep[best_a]["per_read"], "unit": "chunks/s", "cores": int(best_a), "kind": "port",
            "batched64_value": sweep[best_b]["batched64"], "batched64_cores": int(best_b),
            "thread_sweep": sweep, "host_logical_cpus": ncpu,
            "sample": f"the first chunks of the step's batch ({sigs.shape[1]} samples each): per thread count "
                      f"{per_a:.1f} s one read at a time (numpy MAD-normalise + torch-CPU conv stack at batch 1, the structure "
                      f"of riser/control.py:63-69) and {per_b:.1f} s at batch 64; best thread count reported"}


# ---------------------------------------------------------------------------------------------------------------
def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args, argv)                    # before anything touches the GPU
    rank, local_rank, world = rdist.env_world()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if args.stub:
        return run_stub(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no ROCm device visible (there is no CPU fallback)")
    ndev = torch.cuda.device_count()
    if world > 1 and ndev < world and not os.environ.get("RS_DIST_BACKEND"):
        raise SystemExit(f"bench.py: {world} ranks but only {ndev} ROCm device(s) visible "
                         "(RS_DIST_BACKEND=gloo rehearses several ranks on one GPU)")
    device = torch.device("cuda", local_rank % ndev)
    torch.cuda.set_device(device)
    rdist.init(device=device)

    from riser_amd.model import Model

    B, L = args.batch, args.chunk
    lib_dtype = LIB_DTYPE.get(args.dtype, args.dtype)
    if lib_dtype not in Model.dtypes():
        raise SystemExit(f"bench.py: dtype {args.dtype} is not built into this library")
    model = Model(synth.make_state_dict(1), synth.Config(), None, "mRNA", dtype=lib_dtype, device=device)
    if args.config == "promethion_live":
        return run_promethion_live(args, model, lib_dtype, device, rank, world)
    wl = Workload(args, model, device, rank, world)
    step = wl.step

    # steady state is what the ReadUntil loop runs in: let the shader clock settle (~20 steps = 40 ms after an idle
    # period) before the W counted warm-up steps, whatever W the caller picked
    for _ in range(SETTLE_STEPS if args.config != "promethion" else 1):
        step()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(device)

    # ---- timed region: exactly K steps, barrier + sync on both sides ---------------------------
    # HIP events on the launch stream bracket the conv stack inside the timed steps (coarse level: 4 events per call;
    # one event per launch costs ~4.5 us of stream time each, 3 % of the step - that level runs in a separate pass below)
    model.profile(True, coarse=True)
    rdist.barrier(device)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(device)
    rdist.barrier(device)
    elapsed = time.perf_counter() - t0
    coarse_ms, conv_calls = model.profile_read()
    model.profile(False)
    if args.dump_outputs:                     # before the untimed passes below write into the same buffers
        write_outputs(args.dump_outputs, wl.outputs(), rank)
    per_rank = per_rank_object(elapsed, wl.reads_per_step * args.steps, args.steps, world)
    elapsed = rdist.reduce_scalar(elapsed, "max", device)
    total_chunks = rdist.reduce_scalar(wl.reads_per_step * args.steps, "sum", device)
    conv_ms_total = float(coarse_ms[model.n_layers])                       # layers 1..n-1 over the timed region

    # every pass from here on is --full only: a plain run goes straight to its line
    # per-launch detail (not timed): one event after every kernel
    launches = None
    if args.full:
        model.profile(True)
        for _ in range(max(5, min(args.steps, 20)) if args.config != "promethion" else 1):
            step()
        torch.cuda.synchronize(device)
        launches = model.profile_read()
        model.profile(False)

    # ---- per-batch latency incl. H2D of the int16 batch and D2H of the probabilities -----------
    p50 = p99 = 0.0
    n_lat = 0
    if args.full and not args.no_latency and args.config != "promethion":
        host_sig = torch.from_numpy(np.ascontiguousarray(wl.sample_sigs.reshape(-1))).pin_memory()
        host_probs = torch.empty((B, 2), dtype=torch.float32).pin_memory()
        lat = []
        for i in range(LAT_WARMUP + LAT_SAMPLES):
            t1 = time.perf_counter()
            wl.sig.copy_(host_sig, non_blocking=True)
            step()
            host_probs.copy_(wl.probs, non_blocking=True)
            torch.cuda.synchronize(device)
            if i >= LAT_WARMUP:
                lat.append(time.perf_counter() - t1)
        lat_ms = np.asarray(lat) * 1e3
        n_lat = len(lat)
        p50, p99 = float(np.percentile(lat_ms, 50)), float(np.percentile(lat_ms, 99))
    if args.full:
        p99 = rdist.reduce_scalar(p99, "max", device)

    if rank != 0:
        rdist.finalize()
        return 0

    ms_per_step = elapsed / args.steps * 1e3
    value = total_chunks / elapsed
    detail = {
        "metric": "signal chunks classified/sec (RNA004 4 s chunks, batch=512)",
        "value": round(value, 1), "unit": "chunks/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32" if lib_dtype in ("f32", "f32w") else lib_dtype,
        "data": "synthetic",
        "config": {"workload": wl.workload, "name": args.config,
                   "conv_algorithm": {"f32w": "winograd_f23_f43_fp32", "f32": "direct_fp32"}.get(lib_dtype, "direct_" + lib_dtype),
                   "batch_per_call": B, "reads_per_gpu_per_step": wl.reads_per_step, "chunk_samples": L,
                   "sharding": "reads by id across GPUs, no collectives"},
        "roofline": roofline_object(args, model, wl, conv_ms_total, conv_calls, launches),
    }
    if args.full:
        detail.update({
            "p50_batch_latency_ms": round(p50, 3), "p99_batch_latency_ms": round(p99, 3), "latency_samples": n_lat,
            "latency_note": f"host wall time per {B}-read batch incl. H2D of int16 signals from pinned memory and D2H of "
                            f"probabilities; {LAT_SAMPLES} batches after {LAT_WARMUP} warm-up (kernel loop + PCIe; the ReadUntil "
                            "loop's own latency is control_loop)"})

    detail["per_rank"] = per_rank
    single = args.full and world == 1 and args.config == "rna004_b512"
    # ---- the same step over a window of seconds, and fed from pinned host memory ----
    if single and not args.no_latency:
        detail["sustained"] = sustained_object(step, device, B, value)
        detail["host_fed"] = host_fed_object(args, device, model, wl, lib_dtype, value)
    # ---- side measurements on the same batch (rank 0, N = 1 only; not the headline) --------------
    if single and not args.no_variants and args.dtype == "f32":
        detail["variants"] = side_variants(args, device, wl, wl.probs.cpu().numpy().copy())
    if single and not args.no_control_loop:
        detail["control_loop"] = control_loop_object(device, lib_dtype)
    # ---- CPU baseline (rank 0, N = 1 only): oracle port timed on this box's host cores ---------
    if single and not args.no_cpu_baseline:
        detail["cpu_baseline"] = cpu_baseline_object(args, wl.sample_sigs)
    line = compact_line(detail, args, model, wl)
    if args.full:
        path = write_detail(detail, args)
        if path:
            line["detail_file"] = path
    print(json.dumps(line, separators=(",", ":")), flush=True)
    rdist.finalize()
    return 0


# ---------------------------------------------------------------------------------------------------------------
# the ONE line: everything a reader of the driver's record needs, under 6 KB; the verbose objects go to a file
# ---------------------------------------------------------------------------------------------------------------
LINE_LIMIT = 6000
MODE_OF_VARIANT = {            # variants key -> (name in roofline.modes, BASELINE config it carries)
    "bf16x3": ("bf16x3", "the 16-bit MFMA arithmetic of configs 3 / 5 at 512 x 16000"),
    "f16x3": ("f16x3", ""),
    "f16xf8": ("f16xf8", "f16x3 with the cross terms of the wide layers on the block-scaled e4m3 MFMA"),
    "mixed_2s_3s_4s_f16x3": ("mixed_f16x3", "config 5"),
    "mixed_2s_3s_4s_f16xf8": ("mixed_f16xf8", "config 5"),
    "ensemble3_bf16x3": ("ensemble3_bf16x3", "config 3"),
    "ensemble3_f16xf8": ("ensemble3_f16xf8", "config 3"),
    "live_357x8615_f32": ("live_357x8615_f32", "the live ReadUntil batch shape"),
    "resnet_basic_f32": ("resnet_basic_f32", "riser/nets/resnet.py"),
    "resnet_basic_bf16x3": ("resnet_basic_bf16x3", "riser/nets/resnet.py on the bf16 MFMA"),
    "resnet_live_ragged_357_bf16x3": ("resnet_live_ragged_357_bf16x3", "a live batch of ragged lengths through the ResNet"),
}


def modes_object(detail, model, wl):
    """roofline.modes: the side measurements that carry BASELINE configs 3 and 5, the live batch shape and the ResNet, each
    {value (chunks or reads per s), ms_per_step, frac, max_dp_vs_f32, flips}.  `frac` = direct-convolution FLOPs of the
    step's reads (un-padded, counted once per product whatever the mode issues) / the WHOLE step's time
    (normalise and head included) / the dense MFMA peak of the mode's matrix instruction (157.3 TF f32-input, 2.5 PF
    16-bit).  fp32 Winograd issues half to two thirds of those multiplications, so its frac can exceed what the pipe
    executes (roofline.frac is the executed share)."""
    v = detail.get("variants") or {}
    L = wl.args.chunk
    per_len = {}

    def flops(lens):
        tot = 0.0
        for n in lens:
            n = int(n)
            if n not in per_len:
                per_len[n] = float(sum(conv_flops_per_chunk(model.channels, n)[1:]))
            tot += per_len[n]
        return tot

    B = wl.args.batch
    mixed = [(L // 2, 3 * L // 4, L)[i % 3] for i in range(B)]
    lens_of = {"bf16x3": [L] * B, "f16x3": [L] * B, "f16xf8": [L] * B, "ensemble3_bf16x3": [L] * B * 3,
               "ensemble3_f16xf8": [L] * B * 3, "mixed_f16x3": mixed, "mixed_f16xf8": mixed, "live_357x8615_f32": [8615] * 357}
    modes = {}
    for key, (name, _) in MODE_OF_VARIANT.items():
        e = v.get(key)
        if not e:
            continue
        ms = e["ms_per_step"]
        vs = e.get("model0", e)
        m = {"value": e.get("chunks_per_s", e.get("reads_per_s")), "unit": "chunks/s" if "chunks_per_s" in e else "reads/s",
             "ms_per_step": ms}
        if name.startswith("resnet_basic"):
            m["frac"] = e.get("roofline_frac_mfma")
        elif name.startswith("resnet_live"):
            m["frac"] = None
        else:
            peak = PEAK_F32_MFMA_TF if name.endswith("f32") else PEAK_BF16_MFMA_TF
            m["frac"] = round(flops(lens_of[name]) / (ms * 1e-3) / 1e12 / peak, 4)
        if "max_abs_dprob_vs_f32" in vs:
            m["max_dp_vs_f32"] = float("%.3g" % vs["max_abs_dprob_vs_f32"])
            m["flips"] = vs["label_flips_at_0.9_vs_f32"]
        modes[name] = m
    return modes


def compact_line(detail, args, model, wl):
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data")
    line = {k: detail[k] for k in keep}
    c = detail["config"]
    line["config"] = {"workload": c["workload"], "name": c["name"], "conv_algorithm": c["conv_algorithm"],
                      "batch_per_call": c["batch_per_call"], "chunk_samples": c["chunk_samples"], "sharding": c["sharding"]}
    for k in ("p50_batch_latency_ms", "p99_batch_latency_ms", "latency_samples"):
        if k in detail:                                       # --full
            line[k] = detail[k]
    if detail.get("per_rank") and detail["n_gpus"] > 1:
        line["per_rank"] = detail["per_rank"]
    r = detail["roofline"]
    layers = [x for x in r.get("layers", []) if x["ms"]]
    dom = max(layers, key=lambda x: x["ms"]) if layers else None
    # the order matters: the driver's record keeps the head of this object (round 5's `parsed` ended behind slowest_layer_*), so
    # what the round is judged on comes first
    roof = {"bound": r["bound"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"],
            "traffic": r["traffic"]}
    modes = modes_object(detail, model, wl)
    sus, hf = detail.get("sustained"), detail.get("host_fed")
    if sus:
        roof["sustained_value"] = sus["value"]                     # chunks/s over >= 2 s of back-to-back steps
        roof["sustained_ratio"] = sus["ratio_to_headline"]
    if hf:
        for dt in ("f32", "bf16x3", "f16xf8"):                     # batches fed from pinned host memory, upload overlapped
            if dt in hf:
                roof["host_fed_value" if dt == "f32" else f"host_fed_{dt}_value"] = hf[dt]["value"]
        if "f32" in hf:
            roof["host_fed_ratio"] = hf["f32"].get("ratio_to_resident")
    for name in ("bf16x3", "f16xf8", "mixed_f16xf8", "ensemble3_f16xf8", "f16x3", "mixed_f16x3", "ensemble3_bf16x3"):
        if name in modes:                                          # flat scalars of the 16-bit modes (configs 3 / 5)
            roof[f"{name}_value"] = modes[name]["value"]
    for name in ("bf16x3", "f16xf8"):
        if name in modes:
            roof[f"{name}_frac"] = modes[name]["frac"]
            roof[f"{name}_max_dp"] = modes[name].get("max_dp_vs_f32")
            roof[f"{name}_flips"] = modes[name].get("flips")
    thin = (detail.get("variants") or {}).get("thin_batches_f32")
    if thin:
        roof["thin_batch_ms_f32"] = thin["ms_per_step_by_reads"]      # reads of 16000 samples per call -> ms per call
    thin3 = (detail.get("variants") or {}).get("thin_batches_bf16x3")
    if thin3:
        roof["thin_batch_ms_bf16x3"] = thin3["ms_per_step_by_reads"]
    roof.update({"traffic_source": (r["traffic_detail"] or {}).get("source"),
                 "traffic_kernels_match_tree": (r["traffic_detail"] or {}).get("kernels_match_tree"),
                 "traffic_ratio_to_algorithmic": (r["traffic_detail"] or {}).get("ratio_to_algorithmic"),
                 "kernel": r["kernel"][:100],
                 "achieved_is": "executed MFMA FLOPs (padded, Winograd-reduced) / HIP-event time of conv layers 1-11",
                 "algorithmic_tflops": r["algorithmic_tflops"],
                 "algorithmic_frac": round(r["algorithmic_tflops"] / r["peak"], 4),
                 "avg_launch_ms": r["avg_launch_ms"], "conv_stack_ms_per_call": r["conv_stack_ms_per_call"]})
    if "stage_ms" in r:                                            # --full: the per-launch pass and the latency loop
        roof.update({"normalise_ms": r["stage_ms"]["normalise"], "head_ms": r["stage_ms"]["head"],
                     "p50_batch_latency_ms": detail["p50_batch_latency_ms"],
                     "p99_batch_latency_ms": detail["p99_batch_latency_ms"], "latency_window_s": 1.0})
    if dom:
        roof.update({"slowest_layer": dom["layer"], "slowest_layer_ms": dom["ms"],
                     "slowest_layer_executed_tflops": dom["executed_tflops"],
                     "slowest_layer_algorithmic_tflops": dom["algorithmic_tflops"]})
    if sus:
        roof["sustained_window_s"] = sus["window_s"]
    if modes:
        roof["modes"] = modes
    line["roofline"] = roof
    cb = detail.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "batched64_value", "batched64_cores",
                                                   "host_logical_cpus")}
        line["cpu_baseline"]["sample"] = cb["sample"][:200]
    cl = detail.get("control_loop")
    if cl:
        rows = {}
        for name, e in cl.items():
            if not isinstance(e, dict):
                continue
            rows[name] = {"p50_ms": e["p50_ms"], "p99_ms": e["p99_ms"], "max_ms": e["max_ms"], "samples": e["latency_samples"],
                          "loop_p50_ms": e["loop_p50_ms"], "assessed_per_batch": e["assessed_per_batch"]}
        big = cl.get("promethion_18000_channels") or {}
        line["control_loop"] = {"kit": cl["kit"], "dtype": cl["dtype"], "window_s": cl["window_s"], "lines": rows,
                                "phase_ms_median_18000_channels": big.get("phase_ms_median")}
    blob = json.dumps(line, separators=(",", ":"))
    if len(blob) > LINE_LIMIT:                             # never let the line outgrow the driver's tail: drop the widest extras
        for k in ("control_loop", "modes"):
            (line if k in line else line["roofline"]).pop(k, None)
            if len(json.dumps(line, separators=(",", ":"))) <= LINE_LIMIT:
                break
    return line


def write_detail(detail, args):
    """the verbose objects (per-layer table, notes, variants, control-loop phases and counters, CPU thread sweep) as a
    file next to the run: gpurun_out/bench_detail_<config>_<dtype>.json (what profiles/rNN_bench_*.json are copies of)"""
    d = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"bench_detail_{args.config}_{args.dtype}.json")
        with open(path, "w") as f:
            json.dump(detail, f, indent=1)
        return os.path.relpath(path, ROOT)
    except OSError:
        return None


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def write_outputs(d, arrays, rank=0):
    """--dump-outputs: each array as d/<name>.npy (rank r > 0: <name>_rank<r>.npy), float64 if it is float64, else float32.
    Beyond DUMP_LIMIT_BYTES in all, every array keeps a fixed, seeded sample of its rows, sorted, and their indices go to
    <name>_rows.npy: the same rows in every run, so two builds compare output for output."""
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    suffix = f"_rank{rank}" if rank else ""
    if sum(a.nbytes for a in arrays.values()) <= DUMP_LIMIT_BYTES:
        scale = 1.0
    else:                                                  # sampled rows plus their float64 indices, 1 MB left for headers
        scale = (DUMP_LIMIT_BYTES - 10 ** 6) / sum(a.nbytes + 8 * (a.shape[0] if a.ndim else 1) for a in arrays.values())
    for name, a in arrays.items():
        if scale < 1.0 and a.ndim and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * scale))
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
            a = a[rows]
            np.save(os.path.join(d, f"{name}_rows{suffix}.npy"), rows.astype(np.float64))
        np.save(os.path.join(d, f"{name}{suffix}.npy"), a)


if __name__ == "__main__":
    sys.exit(main())
