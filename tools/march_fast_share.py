"""Share of the C2 workload's rays (one 128x128 view of the radius-0.56
occupied sphere, as tools/bench_kernels.py) that the train march's count pass
finishes chain-free, restarts on the exact path, or never starts chain-free,
from the stats counter of dfhip_march_rays_train_count_opts; and the staged
count pass alone (HIP events, median) in the default mode and with mode 1
(the exact path for every ray).  Prints one JSON object.

    python tools/march_fast_share.py [--reps 30]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "single-stable-dreamfusion_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import _dfhip
    import _raymarching
    from scenes import march_inputs
    _dfhip.load()
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    o, d, ne, fa, no, b = map(T, march_inputs(128, 128, seed=0, radius=0.56, noise=0.0))
    n = o.shape[0]
    rays = torch.empty(n, 3, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    bs = torch.empty(_raymarching.march_rays_train_scratch_ints(n), dtype=torch.int32, device=dev)
    stage = torch.empty(_raymarching.march_rays_train_stage_floats(n, 512), device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)

    def count(**kw):
        _raymarching.march_rays_train_count_staged(o, d, b, 1.0, 0.0, 512, n, 1, 128, ne, fa, rays,
                                                   counter, no, bs, stage, **kw)

    count(stats=stats)
    restarted, chain_free = stats.cpu().tolist()
    with_samples = int((rays[:, 2] > 0).sum())
    out = {"rays": n, "rays_with_samples": with_samples, "samples": int(counter[0]),
           "chain_free": chain_free, "restarted": restarted,
           "never_chain_free": n - chain_free - restarted}

    def median_us(**kw):
        ts = []
        for i in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            count(**kw)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts))

    out["count_staged_default_us"] = median_us()
    out["count_staged_exact_us"] = median_us(mode=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
