#!/usr/bin/env python
"""Time the DVGO backbone's train step: the replayed native step
(nerf/native_voxel_step.py, one HIP graph per shading and resolution) against
the eager autograd step of the same commit (Trainer.native_step = False).

    python tools/bench_voxel_step.py [--world 160] [--pairs 20] [--out FILE]

The parent starts one child process under `timeout`; the child writes the
synthetic checkpoint of tools/bench_voxel.py (world^3, C = 12, dim0 = 72),
refreshes the occupancy grid (update_extra_state) until mean_density
settles, and for albedo, lambertian and textureless steps at 16 x 16,
64 x 64 and 128 x 128 times interleaved pairs (native, eager, native, ...) on
the same camera, so drift of the shared machine hits both sides alike.  Both
sides include making the rays from the host pose and the optimizer step.
Per case: medians and spread on the host clock (around a device synchronise)
and by HIP events, the live sample count of the last native step and the
bytes of the field backward's capacity-sized scratch.
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
CASES = [("albedo", 1.0), ("lambertian", 0.1), ("textureless", 0.1)]


def child(world, pairs, warmup, sizes):
    for p in (str(ROOT), str(PKG), str(ROOT / "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import main
    from bench_voxel import synthetic_checkpoint
    from nerf.graph import GraphedTrainStep
    from nerf.native_voxel_step import NativeVoxelStep, eligible
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    dev = torch.device("cuda:0")
    ckpt = str(Path(tempfile.mkdtemp()) / "bench.dvgo")
    synthetic_checkpoint(ckpt, world)

    def trainer_of(hw):
        opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", ckpt,
                              "--h", str(hw), "--w", str(hw), "--guidance", "synthetic"])
        seed_everything(0)
        model = main.network_class(opt)(opt)
        optim = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
        t = Trainer("df", opt, model, InjectedSDS(dev, text_dim=768), device=dev, workspace=None,
                    optimizer=optim, ema_decay=None, fp16=True, use_checkpoint="scratch",
                    mute=True, graph_step=True)
        t.model.train()
        last = None
        with torch.autocast("cuda", dtype=torch.float16):
            for it in range(64):  # as tools/bench_voxel_render.py settles it
                t.model.update_extra_state()
                mean = float(t.model.mean_density)
                if last is not None and abs(mean - last) <= 1e-3 * abs(mean):
                    break
                last = mean
        bits = int(sum(bin(v).count("1") for v in t.model.density_bitfield.cpu().tolist()))
        print(f"{hw} x {hw}: occupancy {bits} of {t.model.density_bitfield.numel() * 8} cells "
              f"after {it + 1} refreshes (mean_density {mean:.4f})")
        return t, NeRFDataset(opt, device=dev, type="train", H=hw, W=hw, size=100)

    def clocks(fn):
        """(host ms around a synchronise, HIP-event ms) of fn()."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"world: {world}^3  C 12  dim0 72  pairs: {pairs}  warmup: {warmup}")
    slower = []
    for hw in sizes:
        t, data = trainer_of(hw)
        stream = torch.cuda.Stream(device=dev)
        for shading, ratio in CASES:
            assert eligible(t, shading), (hw, shading)
            batch = data.collate([0])
            g = GraphedTrainStep(t, batch, shading, ratio, t.text_z[batch["dir"]], stream)
            g.capture(batch)
            nat = g.native
            assert isinstance(nat, NativeVoxelStep) and g.optimizer_in_graph

            def native(b):
                g.load(b, None, row=0)
                g.replay()
                t.optimizer_step(stepped=True)

            def eager(b):
                t.optimizer.zero_grad(set_to_none=True)
                rays = {"H": hw, "W": hw, "dir": b["dir"], "pose": b["pose"],
                        "intrinsics": b["intrinsics"], "device": b["device"]}
                with torch.autocast("cuda", dtype=torch.float16):
                    _, _, loss = t.train_step(type(b)(rays), shading, ratio)
                t.backward_and_step(loss)

            times = {"native": ([], []), "eager": ([], [])}
            before = (t.model.native_step_calls, t.model.torch_calls)
            for i in range(warmup + pairs):
                b = data.collate([i])
                for name, fn in (("native", native), ("eager", eager)):
                    host, events = clocks(lambda: fn(b))
                    if i >= warmup:
                        times[name][0].append(host)
                        times[name][1].append(events)
            assert t.model.native_step_calls == before[0] + warmup + pairs
            assert t.model.torch_calls == before[1], "the eager step left the native field"
            live = int(nat.counter[0].item())
            med = {}
            for name in ("native", "eager"):
                for k, clock in enumerate(("host", "events")):
                    v = times[name][k]
                    med[name, clock] = statistics.median(v)
                    print(f"{hw} x {hw} {shading}: {name:6s} {clock:6s} median "
                          f"{med[name, clock]:.3f}  min {min(v):.3f}  max {max(v):.3f} ms")
            print(f"{hw} x {hw} {shading}: ratio eager / native host "
                  f"{med['eager', 'host'] / med['native', 'host']:.2f}  events "
                  f"{med['eager', 'events'] / med['native', 'events']:.2f}  live samples {live}  "
                  f"capacity {nat.cap}  backward scratch {nat.scratch_bytes} bytes")
            if med["native", "host"] >= med["eager", "host"]:
                slower.append((hw, shading))
            t.optimizer.zero_grad(set_to_none=True)
            del g, nat, native, eager
            torch.cuda.empty_cache()
        del t, data
        torch.cuda.empty_cache()
    print("native slower than eager (host clock): "
          + (", ".join(f"{h} x {h} {s}" for h, s in slower) if slower else "no case"))


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=160)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=str, default="16,64,128")
    ap.add_argument("--timeout", type=int, default=500, help="seconds for the GPU step")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.world, a.pairs, a.warmup, [int(s) for s in a.sizes.split(",")])
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, str(Path(__file__).resolve()),
           "--child", "--world", str(a.world), "--pairs", str(a.pairs), "--warmup",
           str(a.warmup), "--sizes", a.sizes]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(r.stdout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main_())
