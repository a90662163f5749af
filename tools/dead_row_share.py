"""Share of dead field rows in the bench workload's native train step.

A field row is dead when its incoming output gradient is exactly zero:
grad_sigma == 0 and all three grad_albedo == 0 (the samples past a ray's
T < 1e-4 break in composite_rays_train, and what the shading backward makes
of them).  The field backward turns such a row into an all-zero d_enc row,
which the embedding backward need not file (BinnedOpts.row_live).

Runs bench.py's trainer (same options, seed 0) for the warm-up plus the timed
steps and, after each replay of the timed window, counts the dead rows below
the live count in the step's own buffers.  Prints the per-step share and the
mean; with the mask on (the default) also the share the step's own row_live
mask gives, which must agree.

    python tools/dead_row_share.py [--shade albedo|textureless|lambertian]
                                   [--res 128] [--warmup 20] [--steps 100]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "single-stable-dreamfusion_amd")]


def dead_rows(nat):
    """(live field rows, dead rows among them, dead rows by the step's mask or None)."""
    m = int(nat.m_field[0])
    gs, ga = nat.grad_sigma_field[:m], nat.grad_albedo[:m]
    is_dead = (gs == 0) & (ga == 0).all(dim=1)
    dead = int(is_dead.sum())
    # rows in aligned 64-row blocks that are dead throughout: what a field
    # backward that skipped its all-dead rounds (4 tiles of 16 rows) could save
    full = is_dead[:m - m % 64].view(-1, 64).all(dim=1)
    dead_rounds = 64 * int(full.sum())
    by_mask = None
    if nat.live_mask and m:
        words = nat.row_live[:(m + 31) // 32].cpu().numpy().view("uint32")
        import numpy as np
        bits = np.unpackbits(words.view("uint8"), bitorder="little")[:m]
        by_mask = m - int(bits.sum())
    return m, dead, by_mask, dead_rounds


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shade", default="albedo", choices=("albedo", "textureless", "lambertian"))
    p.add_argument("--res", type=int, default=128)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--steps", type=int, default=100)
    args = p.parse_args()
    import bench
    import _dfhip
    _dfhip.load()
    torch.cuda.set_device(0)
    trainer, data = bench.make_trainer(args.res, 0, 0, 1, True, graph=True)
    if args.shade != "albedo":
        trainer.pick_shading = (lambda k: (lambda: (k, 0.1)))(args.shade)
    shares, round_shares = [], []
    for i in range(args.warmup + args.steps):
        trainer.train_iteration(data.collate([0]))
        if i < args.warmup:
            continue
        torch.cuda.synchronize()
        nat = next(iter(trainer._graphs.values())).native
        m, dead, by_mask, dead_rounds = dead_rows(nat)
        shares.append(dead / max(m, 1))
        round_shares.append(dead_rounds / max(m, 1))
        note = "" if by_mask is None else f"  mask {by_mask}" + ("" if by_mask == dead else " (!)")
        print(f"step {i}: {m} field rows, {dead} dead, share {shares[-1]:.4f}, in all-dead "
              f"64-row rounds {round_shares[-1]:.4f}{note}")
    print(f"{args.shade}: mean dead share over steps {args.warmup}..{args.warmup + args.steps - 1}:"
          f" {sum(shares) / len(shares):.4f}  (min {min(shares):.4f}, max {max(shares):.4f});"
          f" in all-dead 64-row rounds {sum(round_shares) / len(round_shares):.4f}")


if __name__ == "__main__":
    main()
