#!/usr/bin/env python3
"""One training step (forward + backward + Adam) of the bench TCN - 8 blocks, 64 filters, kernel 3, dilation base 2, dropout
0.2, receptive field 1021 - at 32 x 4000 / 8000 / 16000: riser_amd.tcn_train's HIP kernels, which run the receptive cone of
the last sample alone, against the same net written in PyTorch (weight norm, dropout, Adam) and run eagerly over every
position on the same GPU in the same process.

    python tools/tcn_train_bench.py [--steps 20] [--rounds 3] [--lengths 4000,8000,16000] [--batch 32]

Step times come from device events around `--steps` steps after a warm-up of every shape; the two implementations are
interleaved round by round, and the median round is reported with the spread.
"""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

NET = dict(in_channels=1, n_filters=64, kernel=3, dilation=2, n_layers=8, dropout=0.2, n_classes=2)


def config():
    return types.SimpleNamespace(model="tcn", learning_rate=1e-3, tcn=types.SimpleNamespace(**NET))


class TorchTcn(torch.nn.Module):
    """riser/nets/tcn.py from torch ops on the parameters of a state dict: weight-normed causal convs, ReLU, dropout, the
    shortcut where the channels change, Linear on the last position"""

    def __init__(self, state):
        super().__init__()
        self.p = torch.nn.ParameterDict({k.replace(".", "_"): torch.nn.Parameter(v.clone()) for k, v in state.items()})

    def forward(self, x):
        p, k, base = self.p, NET["kernel"], NET["dilation"]
        h = x.unsqueeze(1)
        for i in range(NET["n_layers"]):
            d, a = base ** i, h
            for j in (0, 1):
                cp = f"layers_{i}_blocks_{j}_0"
                w = torch._weight_norm(p[cp + "_weight_v"], p[cp + "_weight_g"], 0)
                a = F.conv1d(a, w, p[cp + "_bias"], padding=(k - 1) * d, dilation=d)[:, :, :-(k - 1) * d]
                a = F.dropout(F.relu(a), NET["dropout"], self.training)
            res = F.conv1d(h, p[f"layers_{i}_shortcut_weight"], p[f"layers_{i}_shortcut_bias"]) if h.shape[1] != a.shape[1] else h
            h = F.relu(a + res)
        return F.linear(h[:, :, -1], p["linear_weight"], p["linear_bias"])


def launches_per_step(net) -> int:
    """kernel launches of one TcnTrainer.step: per block two forward convs, per conv a weight-gradient contraction and its
    reduction (three convs where the shortcut is applied), two data gradients (one in block 0); head, loss, head backward,
    weight-norm backward, Adam, fold"""
    n = 0
    for i in range(net["n_layers"]):
        applied = (1 if i == 0 else net["n_filters"]) != net["n_filters"]
        n += 2 + 2 * (3 if applied else 2) + (1 if i == 0 else 2)
    return n + 6


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lengths", type=lambda s: [int(v) for v in s.split(",")], default=[4000, 8000, 16000])
    a = ap.parse_args()
    from riser_amd import tcn as cone
    from riser_amd import tcn_train as T
    assert torch.cuda.is_available(), "tcn_train_bench.py needs an MI355X"
    dev = torch.device("cuda", 0)
    cfg = config()
    net = T.check_tcn_config(cfg)
    torch.manual_seed(1)
    state = T.init_state(net)
    ours = T.TcnTrainer(cfg, state, device=dev, seed=1)
    model = TorchTcn(state).to(dev).train()
    params = [p for k, p in model.p.items() if "shortcut" not in k or k.startswith("layers_0_")]
    opt = torch.optim.Adam(params, lr=1e-3)
    loss_fn = torch.nn.CrossEntropyLoss()
    blocks, _, _ = cone.build_tcn_program({k: v.numpy() for k, v in state.items()}, cfg.tcn, False)
    print(f"{torch.cuda.get_device_name(0)}; TcnTrainer, {net['n_layers']} blocks, {net['n_filters']} filters, kernel "
          f"{net['kernel']}, base {net['dilation']}, dropout {net['dropout']}, receptive field {cone.receptive_field(blocks)}; "
          f"{launches_per_step(net)} kernel launches per step; batch {a.batch}; {a.steps} steps per window, {a.rounds} "
          f"interleaved rounds; ms per step (forward + backward + Adam), median [min .. max]")
    for L in a.lengths:
        x, y = data(a.batch, L, dev)
        print(f"{a.batch} x {L:>5}  cone {cone.program_macs(blocks, L) / 1e6:.1f} M MAC per read forward")

        def step_ours():
            ours.step(x, y)

        def step_torch():
            loss = loss_fn(model(x), y)
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
