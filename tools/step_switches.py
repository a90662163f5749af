"""bench.py with Trainer switches of the native step set (bench.py's own
environment switches are fixed): the headline run of one variant.

    python tools/step_switches.py --set chain_live_mask=0 --set live_mask=1 -- <bench.py arguments>

Each --set NAME=0|1 assigns bool to trainer.NAME before the first step (the
switch must exist on the Trainer).  Prints bench.py's JSON line.
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
    p.add_argument("--set", action="append", default=[], metavar="NAME=0|1")
    args = p.parse_args(argv)
    switches = [(s.split("=")[0], bool(int(s.split("=")[1]))) for s in args.set]
    import bench
    make = bench.make_trainer

    def make_trainer(*a, **kw):
        trainer, data = make(*a, **kw)
        for name, on in switches:
            if not hasattr(trainer, name):
                raise SystemExit(f"step_switches.py: the Trainer has no switch {name}")
            setattr(trainer, name, on)
        return trainer, data
    bench.make_trainer = make_trainer
    sys.argv = [os.path.join(ROOT, "bench.py")] + rest
    bench.main()


if __name__ == "__main__":
    main()
