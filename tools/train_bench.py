#!/usr/bin/env python3
"""One training step (forward + backward + Adam) of the shipped 12-layer ConvNet at 32 x 8000 / 12000 / 16000: riser_amd.train's
HIP kernels against the same net written in PyTorch and run eagerly on the same GPU in the same process.

    python tools/train_bench.py [--steps 20] [--rounds 3] [--lengths 8000,12000,16000] [--batch 32]
    python tools/train_bench.py --depth 2 --kernels 5 [--lengths 16000]
    python tools/train_bench.py --kernels [--lengths 16000]

--depth and --kernels K (one odd width for every layer, or a comma list of twelve) time a generic net on the shipped channel
list instead - riser_amd.train.GenericTrainer, torch's own initialisation under a fixed seed.

Step times come from device events around `--steps` steps after a warm-up of every shape; the two implementations are
interleaved round by round, and the median round is reported with the spread.  --kernels runs this family's steps alone in
a child process under `rocprofv3 --kernel-trace --stats` (kernel times belong to a run of their own) and prints the train_*
rows of its summary.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from riser_amd import synth  # noqa: E402


def config(kernels=None, depth=1):
    cnn = synth.CnnConfig(kernels=kernels or synth.KERNELS, depth=depth)
    return types.SimpleNamespace(model="cnn", learning_rate=1e-3, cnn=cnn)


def state_of(cfg):
    """the synthetic shipped state dict, or - for a generic net - torch's own initialisation under a fixed seed"""
    from riser_amd import train as T
    if T.is_shipped_class(cfg):
        return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(1).items()}
    torch.manual_seed(1)
    return T.init_state(*T.check_generic_config(cfg))


def torch_net(state, dev, cfg):
    layers, c_in = [], 1
    for i, (c, k) in enumerate(zip(cfg.cnn.channels, cfg.cnn.kernels)):
        for d in range(cfg.cnn.depth):
            conv = torch.nn.Conv1d(c_in, c, k, padding="same")
            conv.weight.data.copy_(state[f"layers.{i}.{2 * d}.weight"])
            conv.bias.data.copy_(state[f"layers.{i}.{2 * d}.bias"])
            layers += [conv, torch.nn.ReLU(inplace=True)]
            c_in = c
        layers.append(torch.nn.MaxPool1d(2, 2))
    fc = torch.nn.Linear(c_in, 2)
    fc.weight.data.copy_(state["classifier.2.weight"])
    fc.bias.data.copy_(state["classifier.2.bias"])
    return torch.nn.Sequential(*layers, torch.nn.AdaptiveAvgPool1d(1), torch.nn.Flatten(1), fc).to(dev)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def data(B, L, dev):
    g = torch.Generator().manual_seed(L)
    return torch.randn((B, L), generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).to(dev)


def steps_only(lengths, B, steps, cfg):
    from riser_amd.train import trainer_for
    dev = torch.device("cuda", 0)
    t = trainer_for(cfg, state_of(cfg), device=dev)
    for L in lengths:
        x, y = data(B, L, dev)
        for _ in range(steps):
            t.step(x, y)
    torch.cuda.synchronize()
    t.close()


def kernels(lengths, B, steps, net_args):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--steps-only", "--steps", str(steps), "--batch", str(B),
               "--lengths", ",".join(str(v) for v in lengths), *net_args]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("rocprofv3 failed:\n" + r.stderr[-2000:])
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            sys.exit("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(found[0])))
    print(f"per-kernel times of {steps} steps at {B} x {lengths} (rocprofv3 --kernel-trace --stats)")
    print(f"{'kernel':<64} {'calls':>7} {'total ms':>10} {'mean us':>10} {'share %':>8}")
    ours = [r for r in rows if "train_" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in ours)
    for r in sorted(ours, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].replace("rs::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        ns = float(r["TotalDurationNs"])
        print(f"{name:<64} {int(r['Calls']):>7} {ns / 1e6:>10.2f} {ns / int(r['Calls']) / 1e3:>10.1f} {100 * ns / total:>8.1f}")
    print(f"{'all train_* kernels':<64} {'':>7} {total / 1e6:>10.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lengths", type=lambda s: [int(v) for v in s.split(",")], default=[8000, 12000, 16000])
    ap.add_argument("--depth", type=int, default=1, help="convs per layer (default 1)")
    ap.add_argument("--kernels", nargs="?", const="profile", default=None, metavar="K[,K...]",
                    help="with a value: the conv kernel width(s) of the net; without: per-kernel times under rocprofv3")
    ap.add_argument("--profile", action="store_true", help="per-kernel times under rocprofv3 (what a bare --kernels asks for)")
    ap.add_argument("--steps-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    widths = None
    if a.kernels == "profile":
        a.profile = True
    elif a.kernels is not None:
        widths = [int(v) for v in a.kernels.split(",")]
        widths = widths * len(synth.CHANNELS) if len(widths) == 1 else widths
    cfg = config(widths, a.depth)
    net_args = ["--depth", str(a.depth)] + (["--kernels", a.kernels] if widths else [])
    if a.profile:
        return kernels(a.lengths, a.batch, min(a.steps, 5), net_args)
    if a.steps_only:
        return steps_only(a.lengths, a.batch, a.steps, cfg)
    from riser_amd.train import trainer_for
    assert torch.cuda.is_available(), "train_bench.py needs an MI355X"
    dev = torch.device("cuda", 0)
    state = state_of(cfg)
    ours = trainer_for(cfg, state, device=dev)
    net = torch_net(state, dev, cfg)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    loss_fn = torch.nn.CrossEntropyLoss()
    print(f"{torch.cuda.get_device_name(0)}; {type(ours).__name__}, {len(cfg.cnn.channels)} layers, depth {cfg.cnn.depth}, "
          f"kernels {sorted(set(cfg.cnn.kernels[:cfg.cnn.n_layers]))}; batch {a.batch}; {a.steps} steps per window, "
          f"{a.rounds} interleaved rounds; ms per step (forward + backward + Adam), median [min .. max]")
    for L in a.lengths:
        x, y = data(a.batch, L, dev)

        def step_ours():
            ours.step(x, y)

        def step_torch():
            loss = loss_fn(net(x.unsqueeze(1)), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.item()                              # the reference's loop reads the loss every step (riser/train.py:61)

        for fn in (step_ours, step_torch):                  # warm up this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {"riser_amd": [], "eager PyTorch": []}
        for _ in range(a.rounds):
            times["riser_amd"].append(timed(step_ours, a.steps))
            times["eager PyTorch"].append(timed(step_torch, a.steps))
        for name, ts in times.items():
            med = statistics.median(ts)
            print(f"{a.batch} x {L:>5}  {name:<14} {med:9.2f} ms [{min(ts):.2f} .. {max(ts):.2f}]  {1e3 / med:8.2f} steps/s  "
                  f"{a.batch * 1e3 / med:9.1f} reads/s")
    ours.close()


if __name__ == "__main__":
    main()
