#!/usr/bin/env python
"""Time NeRFRenderer.run() with its glue as native kernels (csrc/hiersample.hip,
`native_run = True`) against the torch glue of the same commit.

    python tools/bench_run_path.py [--legs abc] [--pairs 20] [--out FILE]

The parent starts one child process under `timeout`; the child warms both
paths up and times them as interleaved pairs (native, torch, native, torch,
...) with HIP events, so drift of a shared machine hits both sides alike, and
reports median, min and max per leg:

  a  the glue alone, forward + backward: run() of a stub field that returns
     fixed sigma and rgbs tensors, N = 4096 rays, 64 + 64 steps, perturbed
  b  one -O2 vanilla fp16 render with backward at 64 x 64
  c  one staged 800 x 800 eval frame (chunks of 4096 rays) of the same model

`--only native|torch` runs one path alone (no pairs), for a kernel trace of
leg b:  rocprofv3 --kernel-trace --stats -- python tools/bench_run_path.py
--child --legs b --only native
"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "single-stable-dreamfusion_amd"


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _glue_leg(dev, N=4096, T=64, t=64):
    """run() around a field of fixed tensors: what is timed is the glue."""
    import torch

    import main
    from nerf.renderer import NeRFRenderer

    class Stub(NeRFRenderer):
        def __init__(self, opt):
            super().__init__(opt)
            g = torch.Generator().manual_seed(0)
            # a bump of density around the middle of each ray, as a scene has
            i = torch.linspace(-1, 1, T + t)
            bump = 30 * torch.exp(-0.5 * (i / 0.2) ** 2) * torch.rand(N, 1, generator=g)
            self.sig = torch.nn.Parameter(bump[:, :T].contiguous())
            self.new_sig = torch.nn.Parameter(bump[:, T:].contiguous())
            self.rgbs = torch.nn.Parameter(torch.rand(N * (T + t), 3, generator=g))
            self.register_buffer("bg", torch.rand(N, 3, generator=g))
            self.calls = 0

        def density(self, x):
            self.calls += 1
            return {"sigma": (self.sig if self.calls % 2 else self.new_sig).reshape(-1)}

        def forward(self, x, d, l=None, ratio=1, shading="albedo"):
            return None, self.rgbs, None

        def background(self, d):
            return self.bg

    opt = main.parse_opt(["--text", "x", "-O2"])
    net = Stub(opt).to(dev).train()
    g = torch.Generator().manual_seed(1)
    o = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1) * 1.8
    d = torch.nn.functional.normalize((torch.rand(N, 3, generator=g) - 0.5) * 0.8 - o, dim=-1)
    o, d = o.to(dev)[None], d.to(dev)[None]
    gi = torch.randn(1, N, 3, device=dev)

    def step(native):
        net.native_run = native
        net.zero_grad(set_to_none=True)
        out = net.render(o, d, staged=False, perturb=True, num_steps=T, upsample_steps=t)
        torch.autograd.backward([out["image"], out["weights_sum"]],
                                [gi, torch.ones_like(out["weights_sum"])])
    return net, step


def _vanilla(dev):
    import torch

    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "-O2", "--backbone", "vanilla"])
    torch.manual_seed(0)
    return opt, NeRFNetwork(opt).to(dev)


def _rays(opt, dev, size, kind):
    from nerf.provider import NeRFDataset
    data = NeRFDataset(opt, device=dev, type=kind, H=size, W=size, size=8).collate([1])
    return data["rays_o"], data["rays_d"]


def _train_leg(dev, size=64):
    import torch
    opt, net = _vanilla(dev)
    net.train()
    o, d = _rays(opt, dev, size, "train")
    gi = torch.randn(1, size * size, 3, device=dev) * 1e-2

    def step(native):
        net.native_run = native
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.render(o, d, staged=False, perturb=True, ambient_ratio=1.0,
                             shading="albedo", num_steps=opt.num_steps,
                             upsample_steps=opt.upsample_steps)
        torch.autograd.backward([out["image"], out["weights_sum"]],
                                [gi, torch.ones_like(out["weights_sum"])])
    return net, step


def _frame_leg(dev, size=800):
    import torch
    opt, net = _vanilla(dev)
    net.eval()
    o, d = _rays(opt, dev, size, "test")

    def step(native):
        net.native_run = native
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            net.render(o, d, staged=True, max_ray_batch=opt.max_ray_batch, perturb=False,
                       ambient_ratio=1.0, shading="albedo", num_steps=opt.num_steps,
                       upsample_steps=opt.upsample_steps)
    return net, step


LEGS = {"a": ("glue alone, forward + backward, N = 4096, 64 + 64 steps", _glue_leg),
        "b": ("-O2 vanilla fp16 render + backward, 64 x 64", _train_leg),
        "c": ("staged 800 x 800 eval frame, chunks of 4096 rays", _frame_leg)}


def child(legs, pairs, warmup, only):
    for p in (str(ROOT), str(PKG)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}")
    for leg in legs:
        title, make = LEGS[leg]
        net, step = make(dev)
        n = max(2, pairs // 5) if leg == "c" else pairs  # a frame is 157 chunks
        w = 1 if leg == "c" else warmup
        if only:
            native = only == "native"
            before = (net.native_run_calls, net.torch_run_calls)
            ms = [_timed(lambda: step(native)) for _ in range(w + n)][w:]
            ran = (net.native_run_calls - before[0], net.torch_run_calls - before[1])
            assert (ran[0] > 0, ran[1] > 0) == (native, not native), ran
            print(f"leg {leg}: {title}\n  {only} alone: {w + n} iterations, median "
                  f"{statistics.median(ms):.3f} ms")
            continue
        for _ in range(w):
            step(True)
            step(False)
        before = (net.native_run_calls, net.torch_run_calls)
        times = {True: [], False: []}
        for _ in range(n):
            for native in (True, False):
                times[native].append(_timed(lambda: step(native)))
        ran = (net.native_run_calls - before[0], net.torch_run_calls - before[1])
        assert ran[0] == ran[1] and ran[0] >= n, ran
        med = {k: statistics.median(v) for k, v in times.items()}
        diffs = sorted(b - a for a, b in zip(times[True], times[False]))
        print(f"leg {leg}: {title}  ({n} pairs, warmup {w}, ms)")
        for k, name in ((True, "native"), (False, "torch ")):
            v = times[k]
            print(f"  {name}: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}")
        print(f"  torch - native per pair: median {statistics.median(diffs):.3f}  "
              f"min {diffs[0]:.3f}  max {diffs[-1]:.3f}")
        print(f"  ratio torch / native: {med[False] / med[True]:.3f}")


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=str, default="abc")
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["native", "torch"], default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if not a.legs or set(a.legs) - set(LEGS):
        ap.error("--legs takes letters of 'abc'")
    if a.child:
        child(a.legs, a.pairs, a.warmup, a.only)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--legs", a.legs, "--pairs", str(a.pairs), "--warmup", str(a.warmup)]
    if a.only:
        cmd += ["--only", a.only]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
