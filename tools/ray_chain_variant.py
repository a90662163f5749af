"""bench.py with Trainer.fused_ray_chain set (bench.py's own environment
switches are fixed): the headline run of one variant.

    python tools/ray_chain_variant.py --chain 0|1 -- <bench.py arguments>

--chain 0 keeps the three launches (compositing forward, ray head,
compositing backward).  Prints bench.py's JSON line.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "single-stable-dreamfusion_amd")]


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        k = argv.index("--")
        argv, rest = argv[:k], argv[k + 1:]
    p = argparse.ArgumentParser()
    p.add_argument("--chain", type=int, default=1)
    args = p.parse_args(argv)
    import bench
    make = bench.make_trainer

    def make_trainer(*a, **kw):
        trainer, data = make(*a, **kw)
        trainer.fused_ray_chain = bool(args.chain)
        return trainer, data
    bench.make_trainer = make_trainer
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    bench.main()


if __name__ == "__main__":
    main()
