#!/usr/bin/env python
"""Time the vanilla backbone's albedo train step: (a) the replayed native step
(nerf/native_vanilla_step.py, one HIP graph per resolution) against (b) the
eager autograd step and (c) the autograd-form graph_step capture
(Trainer.native_step = False) of the same commit.  The native step changes
neither (b) nor (c): they are what the backbone ran before it existed.

    python tools/bench_vanilla_step.py [--pairs 20] [--sizes 16,64,128] [--out FILE]

The backbone's defaults (lambda_opacity 1e-3, lambda_entropy 0, max_steps
512).  Per size the parent starts two child processes, each under `timeout`:
one refreshes the occupancy grid (update_extra_state) until mean_density
settles and times interleaved pairs (native, eager, native, ...) on the same
camera, so drift of the shared machine hits both sides alike; the other
captures the autograd form and times a few replays (expected slow: its
device-count march sends the field down the torch path on all N * max_steps
capacity rows; it has a time limit of its own and may fail without failing
the run).  Every side includes making the rays from the host pose and the
optimizer step.  Per case: medians and spread on the host clock (around a
device synchronise) and by HIP events, the live sample count of the last
native step, the capacity and the bytes of the field backward's
capacity-sized scratch.

The last line names the sizes at which the native median is above the eager
median by more than the run-to-run spread the file itself shows (the larger of
the two sides' min-max bands).
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "single-stable-dreamfusion_amd"


def child(hw, mode, pairs, warmup):
    for p in (str(ROOT), str(PKG), str(ROOT / "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch

    import main
    from nerf.graph import GraphedTrainStep
    from nerf.native_vanilla_step import NativeVanillaStep, eligible
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    dev = torch.device("cuda:0")
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla", "--h", str(hw), "--w",
                          str(hw), "--guidance", "synthetic"])
    seed_everything(0)
    model = main.network_class(opt)(opt)
    optim = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    t = Trainer("df", opt, model, InjectedSDS(dev, text_dim=768), device=dev, workspace=None,
                optimizer=optim, ema_decay=None, fp16=True, use_checkpoint="scratch",
                mute=True, graph_step=True)
    t.model.train()
    last = None
    with torch.autocast("cuda", dtype=torch.float16):
        for it in range(16):
            t.model.update_extra_state()
            mean = float(t.model.mean_density)
            if last is not None and abs(mean - last) <= 1e-3 * abs(mean):
                break
            last = mean
    data = NeRFDataset(opt, device=dev, type="train", H=hw, W=hw, size=100)
    bits = int(sum(bin(v).count("1") for v in t.model.density_bitfield.cpu().tolist()))
    if mode == "pair":
        print(f"{hw} x {hw}: lambda_opacity {opt.lambda_opacity} lambda_entropy "
              f"{opt.lambda_entropy} max_steps {opt.max_steps}; occupancy {bits} of "
              f"{t.model.density_bitfield.numel() * 8} cells after {it + 1} refreshes "
              f"(mean_density {mean:.4f})")

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

    def report(name, v_host, v_events):
        for clock, v in (("host", v_host), ("events", v_events)):
            print(f"{hw} x {hw} albedo: {name:8s} {clock:6s} median {statistics.median(v):.3f}  "
                  f"min {min(v):.3f}  max {max(v):.3f} ms")

    stream = torch.cuda.Stream(device=dev)
    batch = data.collate([0])
    if mode == "autograd":
        t.native_step = False
        text_z = t.text_z[batch["dir"]]
        g = GraphedTrainStep(t, batch, "albedo", 1.0, text_z, stream)
        g.capture(batch)
        assert g.native is None

        def captured(b):
            g.load(b, t.text_z[b["dir"]])
            g.replay()
            t.model.step_counter[0].copy_(g.counter)
            t.optimizer_step(stepped=False)
        host, events = [], []
        for i in range(warmup + pairs):
            b = data.collate([i])
            h, e = clocks(lambda: captured(b))
            if i >= warmup:
                host.append(h)
                events.append(e)
        report("autograd", host, events)
        print(f"{hw} x {hw} albedo: autograd-form capture: field rows per step {hw * hw * opt.max_steps} "
              f"(the capacity), torch_calls {t.model.torch_calls}")
        return
    assert eligible(t, "albedo"), hw
    g = GraphedTrainStep(t, batch, "albedo", 1.0, t.text_z[batch["dir"]], stream)
    g.capture(batch)
    nat = g.native
    assert isinstance(nat, NativeVanillaStep)
    print(f"{hw} x {hw} albedo: optimizer in the graph: {g.optimizer_in_graph}")

    def native(b):
        g.load(b, None, row=0)
        g.replay()
        t.optimizer_step(stepped=g.optimizer_in_graph)

    def eager(b):
        t.optimizer.zero_grad(set_to_none=True)
        rays = {"H": hw, "W": hw, "dir": b["dir"], "pose": b["pose"],
                "intrinsics": b["intrinsics"], "device": b["device"]}
        with torch.autocast("cuda", dtype=torch.float16):
            _, _, loss = t.train_step(type(b)(rays), "albedo", 1.0)
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
    for name in ("native", "eager"):
        report(name, *times[name])
    med = {n: statistics.median(times[n][0]) for n in times}
    band = max(max(times[n][0]) - min(times[n][0]) for n in times)
    print(f"{hw} x {hw} albedo: ratio eager / native host {med['eager'] / med['native']:.2f}  "
          f"events {statistics.median(times['eager'][1]) / statistics.median(times['native'][1]):.2f}"
          f"  live samples {live}  capacity {nat.cap}  backward scratch {nat.scratch_bytes} bytes")
    verdict = "SLOWER" if med["native"] > med["eager"] + band else "not slower"
    print(f"{hw} x {hw} albedo: native - eager host median {med['native'] - med['eager']:+.3f} ms, "
          f"min-max band {band:.3f} ms: {verdict}")


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--autograd_pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=str, default="16,64,128")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per paired child")
    ap.add_argument("--autograd_timeout", type=int, default=120,
                    help="seconds per autograd-form child")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", type=str, default=None, help="(internal) pair or autograd")
    ap.add_argument("--size", type=int, default=16)
    a = ap.parse_args()
    if a.child:
        child(a.size, a.child, a.pairs, a.warmup)
        return 0
    sys.path.insert(0, str(PKG))
    text, slower, rc = [], [], 0
    for hw in (int(s) for s in a.sizes.split(",")):
        for mode, pairs, warmup, limit in (("pair", a.pairs, a.warmup, a.timeout),
                                           ("autograd", a.autograd_pairs, 1, a.autograd_timeout)):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()),
                   "--child", mode, "--size", str(hw), "--pairs", str(pairs), "--warmup",
                   str(warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if mode == "pair":
                if not text:
                    import torch
                    text.append(f"pairs: {a.pairs}  warmup: {a.warmup}  autograd-form pairs: "
                                f"{a.autograd_pairs}  torch {torch.__version__}\n")
                text.append(r.stdout)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    rc = r.returncode  # the measurement itself failed: stop, start nothing more
                    break
                if f"{hw} x {hw} albedo: native - eager" in r.stdout and "SLOWER" in r.stdout:
                    slower.append(hw)
            elif r.returncode == 0:
                text.append(r.stdout)
            elif r.returncode in (124, 137):
                text.append(f"{hw} x {hw} albedo: autograd-form capture: no figure, the time limit "
                            f"of {limit} s ran out\n")
                rc = r.returncode  # a hung GPU process: start nothing more
                break
            else:
                tail = r.stderr.strip().splitlines()[-1:] or [""]
                text.append(f"{hw} x {hw} albedo: autograd-form capture: no figure, exit "
                            f"{r.returncode}: {tail[0][:160]}\n")
                if r.returncode < 0 or r.returncode in (134, 139):
                    rc = r.returncode
                    break
        if rc:
            break
    text.append("native slower than eager (host median beyond the min-max band): "
                + (", ".join(f"{h} x {h}" for h in slower) if slower else "no size") + "\n")
    out = "".join(text)
    sys.stdout.write(out)
    if rc == 0 and a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(out)
    return rc


if __name__ == "__main__":
    sys.exit(main_())
