#!/usr/bin/env python
"""Time the vanilla field's common_forward forward + backward on the native
path (csrc/resmlp.hip) and on the torch path of the same module.

    python tools/bench_vanilla.py [--rows 262144] [--pairs 20] [--out FILE]

The parent starts one child process under `timeout`; the child builds the
module, warms both paths up and times them as interleaved pairs (native,
torch, native, torch, ...) with HIP events around each forward + backward, so
drift of the shared machine hits both sides alike.  It reports the medians,
the spread and the ratio, and checks once that the two paths' outputs agree.
"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "single-stable-dreamfusion_amd"


def child(rows, pairs, warmup):
    for p in (str(ROOT), str(PKG)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import main
    from nerf.network import NeRFNetwork
    dev = torch.device("cuda:0")
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla"])
    torch.manual_seed(0)
    net = NeRFNetwork(opt).to(dev)
    x = torch.rand(rows, 3, device=dev) * 2 - 1
    gs = torch.randn(rows, device=dev) * 1e-3
    ga = (torch.randn(rows, 3, device=dev) * 1e-3).half()

    def step(fused):
        net.fused_field = fused
        net.zero_grad(set_to_none=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.autocast("cuda", dtype=torch.float16):
            sigma, albedo = net.common_forward(x)
        torch.autograd.backward([sigma, albedo], [gs, ga])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), sigma.detach(), albedo.detach()

    for _ in range(warmup):
        step(True)
        step(False)
    before = (net.native_calls, net.torch_calls)
    times = {True: [], False: []}
    for _ in range(pairs):
        for fused in (True, False):
            times[fused].append(step(fused)[0])
    assert (net.native_calls - before[0], net.torch_calls - before[1]) == (pairs, pairs)
    _, s1, a1 = step(True)
    _, s0, a0 = step(False)
    rel = float(((s1 - s0).abs() / (s0.abs() + s0.abs().mean())).max())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"rows: {rows}  pairs: {pairs}  warmup: {warmup}  (forward + backward, ms)")
    for k, name in ((True, "native"), (False, "torch ")):
        v = times[k]
        print(f"{name}: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}")
    print(f"ratio torch / native: {med[False] / med[True]:.2f}")
    print(f"sigma native vs torch, max relative difference: {rel:.2e}")
    print(f"albedo native vs torch, max difference: {float((a1.float() - a0.float()).abs().max()):.2e}")


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.rows, a.pairs, a.warmup)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--rows", str(a.rows), "--pairs", str(a.pairs), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
