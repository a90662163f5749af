"""Samples per ray of the bench workload's train step (the serial length of
the per-ray compositing chain).

Runs bench.py's trainer for the warm-up plus the timed steps and, for each of
the last 16 steps, prints the distribution of nat.rays[:, 2] (mean, 90th and
99th percentile, maximum), the same in 16-sample windows, the share of rays
whose samples fit in K windows, and the longest ray of each 64-ray workgroup
of the ray chain.  For the last step also the samples the compositing loop
takes before its T < 1e-4 break (from sigma and delta, log-space prefix
products: statistics, not bit-exact).

    python tools/ray_lengths.py [--res 128] [--warmup 20] [--steps 100]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "single-stable-dreamfusion_amd")]


def pct(x, q):
    return float(torch.quantile(x.float(), q))


def describe(name, x):
    print(f"  {name}: mean {float(x.float().mean()):.2f}  p50 {pct(x, 0.5):.0f}  "
          f"p90 {pct(x, 0.9):.0f}  p99 {pct(x, 0.99):.0f}  max {int(x.max())}")


def taken_counts(nat):
    """Samples per ray the compositing loop reaches (its break included)."""
    rays = nat.rays.long()
    off, num = rays[:, 1], rays[:, 2]
    m = int(nat.counter[0])
    alpha = 1 - torch.exp(-nat.sigma[:m].double() * nat.deltas[:m, 0].double())
    logt = torch.log1p(-alpha.clamp(max=1 - 1e-300))
    cs = torch.cat([logt.new_zeros(1), torch.cumsum(logt, 0)])
    ray_of = torch.repeat_interleave(torch.arange(len(num), device=num.device), num)
    # T before sample i of its ray; the loop reaches i while that T >= 1e-4
    before = cs[:m] - cs[off[ray_of]]
    reached = before >= float(torch.log(torch.tensor(1e-4, dtype=torch.float64)))
    return torch.zeros_like(num).index_add_(0, ray_of, reached.long())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=int, default=128)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--steps", type=int, default=100)
    args = p.parse_args()
    import bench
    import _dfhip
    _dfhip.load()
    torch.cuda.set_device(0)
    trainer, data = bench.make_trainer(args.res, 0, 0, 1, True, graph=True)
    total = args.warmup + args.steps
    for i in range(total):
        trainer.train_iteration(data.collate([0]))
        if i < total - 16:
            continue
        torch.cuda.synchronize()
        nat = next(iter(trainer._graphs.values())).native
        num = nat.rays[:, 2].clone()
        print(f"step {i}: {int(num.sum())} samples, {len(num)} rays")
        describe("samples per ray", num)
        win = (num + 15) // 16
        describe("windows per ray", win)
        print("  share of rays within K windows: " +
              "  ".join(f"K={k} {float((win <= k).float().mean()):.3f}" for k in range(1, 9)))
        pad = (-len(win)) % 64
        wg = torch.cat([win, win.new_zeros(pad)]).view(-1, 64).max(dim=1).values
        describe("longest ray per 64-ray workgroup (windows)", wg)
    taken = taken_counts(nat)
    print("last step, samples taken before the T < 1e-4 break:")
    describe("taken per ray", taken)
    tw = (taken + 15) // 16
    describe("taken windows per ray", tw)
    print("  share of rays within K taken windows: " +
          "  ".join(f"K={k} {float((tw <= k).float().mean()):.3f}" for k in range(1, 9)))
    wg = torch.cat([tw, tw.new_zeros((-len(tw)) % 64)]).view(-1, 64).max(dim=1).values
    describe("longest taken ray per workgroup (windows)", wg)


if __name__ == "__main__":
    main()
