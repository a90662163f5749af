#!/usr/bin/env python
"""Time the DVGO backbone's eval frames: the fused persistent launch
(csrc/voxelrender.hip) against the host loop of the same commit
(NeRFRenderer._infer_loop on the native field), for the four shadings.

    python tools/bench_voxel_render.py [--world 160] [--hw 800] [--rounds 4] [--out FILE]

The parent starts one child process under `timeout`.  The child writes
tools/bench_voxel.py's synthetic checkpoint (a dense blob in a world^3 volume,
C = 12, dim0 = 72), refreshes the occupancy grid until mean_density settles,
and renders hw x hw rays of one orbit camera (tests/scenes.camera_rays) with
infer_tile_w = hw through net.render (run_cuda's eval branch, as test_step).
Per shading: 3 warm-up frames of each path, then `rounds` rounds of 5 fused
frames and 1 loop frame, interleaved, so drift of the shared machine hits both
alike.  A frame is timed by HIP events around the render call on the current
stream (the loop's host syncs leave the GPU idle inside that interval: that
idle time is the loop's cost) and by the host clock around a synchronise.  It
reports medians, spread, the ratio, the samples per frame and the largest
difference between the two paths' images.
"""
import argparse
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "single-stable-dreamfusion_amd"
SHADINGS = ["albedo", "textureless", "lambertian", "normal"]


def child(world, hw, rounds, warmup, max_steps):
    for p in (str(ROOT), str(PKG), str(ROOT / "tests"), str(ROOT / "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.nn.functional as F

    import main
    from bench_voxel import synthetic_checkpoint
    from scenes import camera_rays
    dev = torch.device("cuda:0")
    ckpt = str(Path(tempfile.mkdtemp()) / "bench.dvgo")
    synthetic_checkpoint(ckpt, world)
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", ckpt])
    torch.manual_seed(0)
    net = main.network_class(opt)(opt).to(dev)
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
    print(f"world: {world}^3  C 12  dim0 72  frame: {hw} x {hw}  max_steps {max_steps}  "
          f"occupancy: {occupied} of {net.density_bitfield.numel() * 8} cells after {it + 1} "
          f"refreshes (mean_density {mean:.4f})")
    o, d = camera_rays(hw, hw, seed=0, radius=1.3)
    rays_o, rays_d = torch.from_numpy(o).to(dev)[None], torch.from_numpy(d).to(dev)[None]
    light = F.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0).to(dev)
    net.infer_tile_w = hw

    def frame(shading, native):
        net.native_infer = native
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = net.render(rays_o, rays_d, staged=True, perturb=False, shading=shading,
                             light_d=light, ambient_ratio=0.1, max_steps=max_steps,
                             bg_color=None)
        e1.record()
        torch.cuda.synchronize()
        net.native_infer = True
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    for shading in SHADINGS:
        for _ in range(warmup):
            frame(shading, True), frame(shading, False)
        before = net.native_render_calls
        ev, host = {True: [], False: []}, {True: [], False: []}
        for _ in range(rounds):
            for native in (True,) * 5 + (False,):
                e, h, out = frame(shading, native)
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
            print(f"{shading}: {label} events median {med[k]:.3f}  min {min(v):.3f}  max "
                  f"{max(v):.3f} ms over {len(v)} frames; host clock median "
                  f"{statistics.median(h):.3f} ms")
        print(f"{shading}: ratio loop / fused {med[False] / med[True]:.2f}  samples per frame "
              f"{samples}  ({samples / med[True] * 1e-6:.2f} G samples/s fused)  "
              f"max |loop - fused| image {diff:.2e}")


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=160)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=4, help="rounds of 5 fused + 1 loop frames")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max_steps", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=500, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.world, a.hw, a.rounds, a.warmup, a.max_steps)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--world", str(a.world), "--hw", str(a.hw), "--rounds", str(a.rounds),
           "--warmup", str(a.warmup), "--max_steps", str(a.max_steps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
