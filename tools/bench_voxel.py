#!/usr/bin/env python
"""Time the DVGO voxel field on the native path (csrc/voxelfield.hip) and on
the torch path of the same module (nerf/network_dvgo.py).

    python tools/bench_voxel.py [--world 160] [--rows 262144] [--pairs 20] [--out FILE]

The parent starts one child process under `timeout`; the child writes a
synthetic checkpoint (a dense blob in a world^3 volume, C = 12, posbase_pe 5,
viewbase_pe 4: dim0 = 72), warms both paths up and times them as interleaved
pairs (native, torch, native, torch, ...), so drift of the shared machine hits
both sides alike:

  forward            common_forward, no grad, `rows` positions in [-1, 1]^3
  forward+backward   common_forward and the backward of a random albedo gradient
  normal             net.normal on the samples of one 128 x 128 -O step (the
                     march's own positions, recorded from a render)
  train step         one 16 x 16 -O albedo step: render, SDS gradient, backward,
                     optimizer (host clock around a device synchronise)

Kernel cases use HIP events around the call.  It reports medians, spread and
ratios, and checks once that the two paths' outputs agree.
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


def synthetic_checkpoint(path, world):
    import torch
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ax = torch.linspace(-1, 1, world)
    rad = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt()
    density = ((0.7 - rad) * 40).clamp(-8, 8) + r(world, world, world) * 0.5
    dims, names = [72, 128, 128, 3], ["0", "2.0", "3"]
    sd = {"density": density[None, None], "k0": r(1, 12, world, world, world),
          "xyz_min": torch.tensor([-1.0, -1.0, -1.0]), "xyz_max": torch.tensor([1.0, 1.0, 1.0]),
          "posfreq": torch.tensor([2.0 ** i for i in range(5)]),
          "viewfreq": torch.tensor([2.0 ** i for i in range(4)])}
    for n, i, o in zip(names, dims[:-1], dims[1:]):
        sd[f"rgbnet.net.{n}.weight"] = r(o, i) * (2.0 / i) ** 0.5
        sd[f"rgbnet.net.{n}.bias"] = r(o) * 0.1
    hyper = {"cfg": {"fine_model_and_render": {"alpha_init": 1e-2}}}
    torch.save({"state_dict": sd, "hyper_parameters": hyper}, path)


def child(world, rows, pairs, warmup):
    for p in (str(ROOT), str(PKG)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp()
    ckpt = str(Path(tmp) / "bench.dvgo")
    synthetic_checkpoint(ckpt, world)

    def trainer_of(hw):
        opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", ckpt,
                              "--h", str(hw), "--w", str(hw), "--guidance", "synthetic"])
        seed_everything(0)
        model = main.network_class(opt)(opt)
        optim = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
        t = Trainer("df", opt, model, InjectedSDS(dev, text_dim=768), device=dev, workspace=None,
                    optimizer=optim, ema_decay=None, fp16=True, use_checkpoint="scratch", mute=True)
        t.model.train()
        with torch.autocast("cuda", dtype=torch.float16):
            for _ in range(4):
                t.model.update_extra_state()
        return t, NeRFDataset(opt, device=dev, type="train", H=hw, W=hw, size=100)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def pairs_of(name, net, fn, clock=timed):
        def run(fused):
            net.fused_field = fused
            with torch.autocast("cuda", dtype=torch.float16):
                return clock(lambda: fn(fused))
        for _ in range(warmup):
            run(True), run(False)
        before = (net.native_calls + net.native_normal_calls, net.torch_calls)
        times = {True: [], False: []}
        for _ in range(pairs):
            for fused in (True, False):
                times[fused].append(run(fused)[0])
        after = (net.native_calls + net.native_normal_calls, net.torch_calls)
        assert after[0] > before[0] and after[1] > before[1], "a path did not run"
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, label in ((True, "native"), (False, "torch ")):
            v = times[k]
            print(f"{name}: {label} median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f} ms")
        print(f"{name}: ratio torch / native {med[False] / med[True]:.2f}")
        net.fused_field = True
        return run(True)[1], run(False)[1]

    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"world: {world}^3  C 12  dim0 72  rows: {rows}  pairs: {pairs}  warmup: {warmup}")
    big, data = trainer_of(128)
    net = big.model
    x = torch.rand(rows, 3, device=dev) * 2 - 1
    ga = torch.randn(rows, 3, device=dev) * 1e-3

    def forward(_):
        with torch.no_grad():
            return net.common_forward(x)

    def forward_backward(_):
        net.zero_grad(set_to_none=True)
        sigma, albedo = net.common_forward(x)
        albedo.backward(ga.to(albedo.dtype))
        return [p.grad for p in net.main_net.rgbnet.parameters()]

    (s1, a1), (s0, a0) = pairs_of("forward", net, forward)
    rel = float(((s1 - s0).abs() / (s0.abs() + s0.abs().mean())).max())
    print(f"forward: sigma native vs torch, max relative difference {rel:.2e}; albedo max "
          f"difference {float((a1.float() - a0.float()).abs().max()):.2e}")
    g1, g0 = pairs_of("forward+backward", net, forward_backward)
    print("forward+backward: gradients native vs torch, |difference| / |torch| "
          + " ".join(f"{float((a - b).norm() / b.norm()):.1e}" for a, b in zip(g1, g0)))

    # the samples of one 128 x 128 -O step, as the march emits them
    seen = []
    orig = net.common_forward
    net.common_forward = lambda p, *a, **k: (seen.append(p.detach().clone()), orig(p, *a, **k))[1]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        big.train_step(data.collate([0]), "albedo", 1.0)
    del net.common_forward
    big._pending_sds = None
    xs = max(seen, key=len)
    print(f"normal: {xs.shape[0]} samples of one 128 x 128 step")

    def normal(_):
        with torch.no_grad():
            return net.normal(xs.clone())
    n1, n0 = pairs_of("normal", net, normal)
    print(f"normal: native vs torch, max difference {float((n1 - n0).abs().max()):.2e}")

    small, sdata = trainer_of(16)

    def train_step(_):
        small.optimizer.zero_grad(set_to_none=True)
        pred_rgb, pred_ws, loss = small.train_step(sdata.collate([0]), "albedo", 1.0)
        small.backward_and_step(loss)
        return pred_rgb.detach()
    pairs_of("train step 16x16", small.model, train_step, clock=wall)


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=160)
    ap.add_argument("--rows", type=int, default=1 << 18)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.world, a.rows, a.pairs, a.warmup)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--world", str(a.world), "--rows", str(a.rows), "--pairs", str(a.pairs),
           "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
