#!/usr/bin/env python
"""Time the vanilla backbone's albedo eval frames: the fused persistent launch
(csrc/resmlprender.hip) against the host loop of the same commit
(NeRFRenderer._infer_loop with its default schedule on the native field).

    python tools/bench_vanilla_render.py [--hw 800] [--rounds 4] [--out FILE]

The parent starts one child process under `timeout`.  The child builds a
seeded vanilla net (torch.manual_seed(0), the module's own initialisation; the
density head's bias is lowered by `--bias` so that the Gaussian blob at the
origin stands out of a thin haze, as a trained scene's object does), refreshes
the occupancy grid until mean_density settles, and renders hw x hw rays of one
orbit camera (tests/scenes.camera_rays) with infer_tile_w = hw through
net.render (run_cuda's eval branch, as test_step).  3 warm-up frames of each
path, then `rounds` rounds of 5 fused frames and 1 loop frame, interleaved, so
drift of the shared machine hits both alike.  A frame is timed by HIP events
around the render call on the current stream (the loop's host syncs leave the
GPU idle inside that interval: that idle time is the loop's cost) and by the
host clock around a synchronise.  It reports medians, spread, the ratio, the
samples per frame and samples/s, the largest difference between the two
paths' images, and k_resmlp_fwd's stand-alone rate at the frame's sample
count: the MLP dominates this backbone, so that rate is the fused frame's
ceiling.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "single-stable-dreamfusion_amd"


def child(hw, rounds, warmup, max_steps, bias):
    for p in (str(ROOT), str(PKG), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    import _resmlp
    import main
    from nerf.network import NeRFNetwork
    from scenes import camera_rays
    dev = torch.device("cuda:0")
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla"])
    torch.manual_seed(0)
    net = NeRFNetwork(opt).to(dev)
    with torch.no_grad():
        net.sigma_net.net[4].bias[0] += bias
    net.train()
    last = None
    with torch.autocast("cuda", dtype=torch.float16):
        for it in range(64):
            net.update_extra_state()
            mean = float(net.mean_density)
            if last is not None and abs(mean - last) <= 1e-3 * abs(mean):
                break
            last = mean
    net.eval()
    occupied = int(np.unpackbits(net.density_bitfield.cpu().numpy()).sum())
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"net: vanilla 39 -> 128 x4 -> 4, seed 0, density bias {bias:+g}  frame: {hw} x {hw}  "
          f"max_steps {max_steps}  occupancy: {occupied} of {net.density_bitfield.numel() * 8} "
          f"cells after {it + 1} refreshes (mean_density {mean:.4f})")
    o, d = camera_rays(hw, hw, seed=0, radius=1.3)
    rays_o, rays_d = torch.from_numpy(o).to(dev)[None], torch.from_numpy(d).to(dev)[None]
    net.infer_tile_w = hw

    def frame(native):
        net.native_infer = native
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = net.render(rays_o, rays_d, staged=True, perturb=False, shading="albedo",
                             max_steps=max_steps, bg_color=None)
        e1.record()
        torch.cuda.synchronize()
        net.native_infer = True
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    for _ in range(warmup):
        frame(True), frame(False)
    before = net.native_render_calls
    ev, host = {True: [], False: []}, {True: [], False: []}
    for _ in range(rounds):
        for native in (True,) * 5 + (False,):
            e, h, out = frame(native)
            ev[native].append(e)
            host[native].append(h)
            if native:
                work = net.last_infer_work.cpu().numpy().view(np.uint32)
                samples = int(work[1]) + (int(work[2]) << 32)
                img = out["image"].float()
            else:
                diff = float((out["image"].float() - img).abs().max())
    assert net.native_render_calls - before == 5 * rounds, "the fused path did not run"
    med = {k: statistics.median(v) for k, v in ev.items()}
    for k, label in ((True, "fused"), (False, "loop ")):
        v, h = ev[k], host[k]
        print(f"albedo: {label} events median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f} ms "
              f"(spread {max(v) - min(v):.3f}) over {len(v)} frames; host clock median "
              f"{statistics.median(h):.3f} ms")
    spread = max(max(v) - min(v) for v in ev.values())
    print(f"albedo: ratio loop / fused {med[False] / med[True]:.2f}  loop - fused "
          f"{med[False] - med[True]:.3f} ms against the larger spread {spread:.3f} ms  "
          f"samples per frame {samples}  ({samples / med[True] * 1e-6:.3f} G samples/s fused, "
          f"{samples / med[False] * 1e-6:.3f} loop)  max |loop - fused| image {diff:.2e}")

    # the field alone on as many positions as the frame evaluated
    M = max(samples, 1 << 16)
    x = torch.rand(M, 3, device=dev) * 2 - 1
    ps = [p.detach() for p in net.sigma_net.parameters()]
    sigma = torch.empty(M, device=dev)
    albedo = torch.empty(M, 3, device=dev, dtype=torch.float16)
    times = []
    for i in range(warmup + 10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _resmlp.field_forward(x, ps, sigma, albedo)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    t = statistics.median(times)
    print(f"k_resmlp_fwd alone: M {M}  median {t:.3f}  min {min(times):.3f}  max {max(times):.3f} "
          f"ms  ({M / t * 1e-6:.3f} G samples/s)")


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=4, help="rounds of 5 fused + 1 loop frames")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max_steps", type=int, default=1024)
    ap.add_argument("--bias", type=float, default=-3.0, help="added to the density head's bias")
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.hw, a.rounds, a.warmup, a.max_steps, a.bias)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--hw", str(a.hw), "--rounds", str(a.rounds), "--warmup", str(a.warmup),
           "--max_steps", str(a.max_steps), "--bias", str(a.bias)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
