"""GPU tests of the DVGO backbone's fused persistent inference renderer
(csrc/voxelrender.hip, dfhip_voxel_render_rays_infer[_shaded], dispatched by
NeRFRenderer._infer_fused on nerf/voxel_field.py's InferField).

The yardstick is the renderer's own host loop at n_step = 1 on the native
field (`_infer_loop(..., n_step_max=1)`): the kernel runs the same device
functions in the same order (-ffp-contract=off, MFMA rows independent), so
weights_sum and depth of all four shadings, the albedo image and the sample
count must be the loop's bits.  Each link of that loop is pinned elsewhere: the
field and the normal to the float64 restatement (tests/test_gpu_voxel.py), the
march and the compositing to oracle/ (tests/test_gpu_raymarching.py,
tests/test_gpu_march_settings.py).

Shaded images go through NeRFNetwork.forward in the loop (torch ops on the
native normal), whose f16 `normal @ l` may round one f16 ulp apart from the
kernel's: the project's bounds for that construct (DESIGN.md "C4 renderer:
shaded frames"): textureless and lambertian <= 2^-9 absolute, the normal
view <= 1e-5.

Counters.  A fused frame raises `native_render_calls` by one and leaves
`torch_calls` alone.  It also counts ONCE in `native_calls` (shaded: and once
in `native_normal_calls`), where the loop counts one per iteration: the
pre-existing tests/test_gpu_voxel.py::test_o2_step_and_test_view requires an
eval view to show in those two counters, so "unchanged" cannot hold for them;
"+1 for the whole frame" still tells the fused frame from the loop.
"""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scenes
import voxel_cases as vc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SHADINGS = ["albedo", "textureless", "lambertian", "normal"]
CKPTS = {"small": dict(world=vc.WORLD_SMALL),                     # dim0 72
         "padded": dict(world=vc.WORLD_SMALL, C=4, posbase=0),    # dim0 31
         "large": dict(world=vc.WORLD_LARGE),
         "deep": dict(world=vc.WORLD_SMALL, depth=4),             # not served natively
         # sigma = 10 softplus(20 - 4.6) ~ 154: T < 1e-4 after ~ 20 samples of dt_min
         "dense": dict(world=vc.WORLD_SMALL, density=torch.full((1, 1, *vc.WORLD_SMALL), 20.0)),
         "flat": dict(world=vc.WORLD_SMALL, density=torch.full((1, 1, *vc.WORLD_SMALL), 1.5))}
LIGHT = F.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
B_TL, B_N = 2.0 ** -9, 1e-5  # textureless / lambertian, normal view


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def nets(gpu, tmp_path_factory):
    import main
    tmp = tmp_path_factory.mktemp("dvgo_render")
    out = {}
    for name, kw in CKPTS.items():
        sd, dim0 = vc.make_state(seed=len(out), **kw)
        path = vc.save_checkpoint(tmp / f"{name}.dvgo", sd)
        opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
        net = main.network_class(opt)(opt).to(gpu)
        net.eval()
        out[name] = (net, sd, path)
    assert out["small"][0].main_net.dim0 == 72 and out["padded"][0].main_net.dim0 == 31
    return out


def set_bits(net, kind, seed=0):
    if kind == "ones":
        net.density_bitfield.fill_(255)
    else:  # one cell in eight: empty-space skips
        bits = scenes.random_bitfield(net.cascade, net.grid_size, seed)
        assert bits.shape == tuple(net.density_bitfield.shape)
        net.density_bitfield.copy_(torch.from_numpy(bits).to(net.density_bitfield.device))


def rays(gpu, h, w, seed=0, radius=1.3):
    o, d = scenes.camera_rays(h, w, seed, radius=radius)
    return torch.from_numpy(o).to(gpu), torch.from_numpy(d).to(gpu)


def samples_of(net):
    work = net.last_infer_work.cpu().numpy().view(np.uint32)
    return int(work[1]) + (int(work[2]) << 32)


class Recorder:
    """Wraps raymarching.march_rays: keeps what the loop marched."""

    def __init__(self, keep=False):
        import raymarching
        self.mod, self.orig, self.keep = raymarching, raymarching.march_rays, keep
        self.samples, self.steps = 0, []

    def __enter__(self):
        def march(n_alive, n_step, rays_alive, *a, **k):
            xyzs, dirs, deltas = self.orig(n_alive, n_step, rays_alive, *a, **k)
            self.samples += int((deltas[:n_alive * n_step, 0] > 0).sum())
            if self.keep:
                assert n_step == 1
                self.steps.append((rays_alive[:n_alive].clone(), xyzs[:n_alive].clone(),
                                   deltas[:n_alive].clone()))
            return xyzs, dirs, deltas
        self.mod.march_rays = march
        return self

    def __exit__(self, *exc):
        self.mod.march_rays = self.orig


def near_far(net, rays_o, rays_d):
    import raymarching
    return raymarching.near_far_from_aabb(rays_o, rays_d, net.aabb_infer)


def fused(net, rays_o, rays_d, shading="albedo", perturb=False, T_thresh=1e-4, max_steps=128,
          dt_gamma=0.0, ratio=1.0, seed=7):
    """(weights_sum, depth, image) numpy and the sample count of one fused frame."""
    nears, fars = near_far(net, rays_o, rays_d)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        field = net.native_infer_field(shading, rays_o)
        assert field is not None
        torch.manual_seed(seed)
        out = net._infer_fused(rays_o, rays_d, nears, fars, field, perturb, dt_gamma, max_steps,
                               T_thresh, shading=shading, light_d=LIGHT.to(rays_o.device),
                               ambient_ratio=ratio)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], samples_of(net)


def loop(net, rays_o, rays_d, shading="albedo", perturb=False, T_thresh=1e-4, max_steps=128,
         dt_gamma=0.0, ratio=1.0, seed=7, fused_field=True, keep=False):
    """The host loop at n_step = 1 on the native (or the torch) field."""
    nears, fars = near_far(net, rays_o, rays_d)
    net.fused_field = fused_field
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), Recorder(keep) as rec:
            torch.manual_seed(seed)
            out = net._infer_loop(rays_o, rays_d, nears, fars, LIGHT.to(rays_o.device), ratio,
                                  shading, perturb, dt_gamma, max_steps, T_thresh, n_step_max=1)
    finally:
        net.fused_field = True
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], rec.samples, rec.steps


def assert_bits(got, want, what):
    for name, a, b in zip(("weights_sum", "depth", "image"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")


# ---------------------------------------------------------------- 1. the path runs
def test_eval_frame_runs_the_kernel(gpu, nets):
    net = nets["small"][0]
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert net.native_infer_field("albedo", rays_o) is not None
        before = (net.native_render_calls, net.native_calls, net.native_normal_calls,
                  net.torch_calls)
        out = net.render(rays_o[None], rays_d[None], staged=True, perturb=False, max_steps=128)
    after = (net.native_render_calls, net.native_calls, net.native_normal_calls, net.torch_calls)
    # one frame: one fused launch, counted once as a native field evaluation
    # (the loop would count ~ 70 of them), no normal, no torch path
    assert after == (before[0] + 1, before[1] + 1, before[2], before[3])
    assert out["image"].shape == (1, 256, 3) and torch.isfinite(out["image"]).all()
    (lw, ld, li), want, _ = loop(net, rays_o, rays_d)
    assert samples_of(net) == want and want > 256 * 10
    np.testing.assert_array_equal(out["weights_sum"].reshape(-1).cpu().numpy(), lw)


# ---------------------------------------------------------------- 2. bit identity
def special_rays(gpu):
    """40 camera rays, 40 looking away from the box (they miss the aabb), and 48
    that cross the aabb outside the volume's 0.8 box (|x| = |z| = 0.9)."""
    o, d = rays(gpu, 8, 5, seed=3)
    ys = torch.linspace(-0.95, 0.95, 48, device=gpu)
    oo = torch.stack([torch.full_like(ys, 0.9), torch.full_like(ys, -2.0), 0.9 * torch.sign(ys)
                      + 0.05 * ys], -1)
    dd = torch.tensor([0.0, 1.0, 0.0], device=gpu).expand(48, 3)
    return (torch.cat([o, o, oo]).contiguous(), torch.cat([d, -d, dd]).contiguous())


CASES = [("small", "ones", n, {}) for n in (0, 1, 63, 64, 65, 1024)] + [
    ("small", "random", 1024, {}), ("padded", "ones", 256, {}), ("padded", "random", 1024, {}),
    ("large", "ones", 256, {}), ("large", "random", 1024, {}),
    ("small", "ones", 256, dict(perturb=True)),
    ("small", "random", 1024, dict(perturb=True, dt_gamma=1 / 128)),
    ("large", "ones", 256, dict(dt_gamma=1 / 128)),
    ("small", "ones", -1, {}),                       # the special rays
    ("small", "ones", 256, dict(max_steps=4)),       # fewer than kK = 8 samples per ray
    ("dense", "ones", 256, {}),                      # T_thresh retirement
]


@pytest.mark.parametrize("ckpt, bits, n, kw", CASES,
                         ids=[f"{c}-{b}-{n}-{'-'.join(k) or 'plain'}" for c, b, n, k in CASES])
def test_bit_identity_with_the_loop(gpu, nets, ckpt, bits, n, kw):
    net = nets[ckpt][0]
    set_bits(net, bits, seed=5)
    if n < 0:
        rays_o, rays_d = special_rays(gpu)
    else:
        side = 16 if n == 256 else 32
        o, d = rays(gpu, side, side, seed=2)
        rays_o, rays_d = o[:n].contiguous(), d[:n].contiguous()
    want, want_samples, _ = loop(net, rays_o, rays_d, **kw)
    for shading in SHADINGS:
        got, samples = fused(net, rays_o, rays_d, shading=shading, ratio=0.1, **kw)
        assert samples == want_samples, shading
        np.testing.assert_array_equal(got[0], want[0], err_msg=f"{shading}: weights_sum")
        np.testing.assert_array_equal(got[1], want[1], err_msg=f"{shading}: depth")
        if shading == "albedo":
            np.testing.assert_array_equal(got[2], want[2], err_msg="albedo: image")
        assert np.isfinite(got[2]).all()
    if n < 0:
        nears, fars = (t.cpu().numpy() for t in near_far(net, rays_o, rays_d))
        miss = slice(40, 80)
        assert (want[0][miss] == 0).all() and (want[2][miss] == 0).all()
        # outside the 0.8 box: sigma = 10 softplus(act_shift), albedo exactly 0.5
        out = slice(80, 128)
        assert (want[0][out] > 0).all()
        np.testing.assert_allclose(want[2][out], np.repeat(0.5 * want[0][out, None], 3, 1),
                                   rtol=2e-6, atol=0)
    elif n >= 64:
        assert (want[0] > 0).sum() >= n // 2
    if ckpt == "dense":  # rays through the volume retire on T_thresh
        assert (want[0] > 1 - 1e-3).sum() > n // 2
    if kw.get("max_steps") == 4:
        assert 0 < want_samples <= 4 * n


# ---------------------------------------------------------------- 3. queue layouts
def test_queue_layouts(gpu, nets):
    net = nets["large"][0]
    set_bits(net, "random", seed=9)
    rays_o, rays_d = rays(gpu, 32, 32, seed=4)
    keep = (net.infer_order, net.infer_chunk_log2, net.infer_tile_w)
    runs = []
    variants = [(0, 6, 0), (1, 0, 0), (1, 3, 0), (1, 6, 0), (1, 6, 32), (2, 6, 32), (2, 6, 0)]
    try:
        for shading in ("albedo", "lambertian", "normal"):
            for flag, cl, tile in variants:
                net.infer_order, net.infer_chunk_log2, net.infer_tile_w = flag, cl, tile
                runs.append((shading, (flag, cl, tile),
                             *fused(net, rays_o, rays_d, shading=shading, ratio=0.1)))
    finally:
        net.infer_order, net.infer_chunk_log2, net.infer_tile_w = keep
    first = {}
    for shading, v, got, samples in runs:
        ref = first.setdefault(shading, (got, samples))
        assert samples == ref[1] and samples > 0, (shading, v)
        assert_bits(got, ref[0], f"{shading} {v}")


# ---------------------------------------------------------------- 4. shaded images
@pytest.mark.parametrize("ckpt, bits, ratio", [("small", "ones", 0.1), ("small", "random", 0.0),
                                               ("large", "ones", 0.1), ("padded", "ones", 0.0),
                                               ("flat", "ones", 0.1), ("flat", "ones", 0.0)])
def test_shaded_images_against_the_loop(gpu, nets, ckpt, bits, ratio):
    net = nets[ckpt][0]
    set_bits(net, bits, seed=6)
    rays_o, rays_d = rays(gpu, 16, 16, seed=5)
    albedo, _ = fused(net, rays_o, rays_d)
    for shading in SHADINGS[1:]:
        want, want_samples, _ = loop(net, rays_o, rays_d, shading=shading, ratio=ratio)
        got, samples = fused(net, rays_o, rays_d, shading=shading, ratio=ratio)
        err = float(np.abs(got[2] - want[2]).max())
        print(f"parity: shaded {ckpt} {bits} ratio {ratio} {shading}: max |fused - loop| {err:.3e}")
        assert samples == want_samples
        # density, depth and weights_sum are the albedo frame's and the loop's bits
        for k in (0, 1):
            np.testing.assert_array_equal(got[k], want[k])
            np.testing.assert_array_equal(got[k], albedo[k])
        assert err <= (B_N if shading == "normal" else B_TL), (shading, err)
        if ckpt == "flat":  # every normal is exactly 0
            if shading == "textureless":
                lam = float(torch.tensor(ratio).half())
                np.testing.assert_allclose(got[2], np.repeat(lam * got[0][:, None], 3, 1), rtol=0,
                                           atol=2e-6)
                if ratio == 0.0:
                    assert (got[2] == 0).all()
            if shading == "normal":
                np.testing.assert_allclose(got[2], np.repeat(0.5 * got[0][:, None], 3, 1), rtol=0,
                                           atol=2e-6)
    assert (albedo[0] > 0).sum() > 128


# ---------------------------------------------------------------- 5. float64 end to end
def composite64(steps, sigma, rgb, nears, N):
    """Front-to-back compositing of the recorded samples in float64 (no
    T_thresh: the run uses 0): w = alpha T, T = prod (1 - alpha), t = near +
    the sum of deltas[:, 1]."""
    ws, dp, img = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    T, t = np.ones(N), nears.astype(np.float64).copy()
    pos = 0
    for ids, _, deltas in steps:
        n = len(ids)
        live = deltas[:, 0] > 0
        i = ids[live]
        s, c = sigma[pos:pos + n][live], rgb[pos:pos + n][live]
        dt, dl = deltas[live, 0].astype(np.float64), deltas[live, 1].astype(np.float64)
        alpha = 1 - np.exp(-s * dt)
        w = alpha * T[i]
        t[i] += dl
        ws[i] += w
        dp[i] += w * t[i]
        img[i] += w[:, None] * c
        T[i] *= 1 - alpha
        pos += n
    return ws, dp, img, t


def test_end_to_end_against_float64(gpu, nets):
    """T_thresh = 0 (no retirement depends on rounding).  The loop's samples
    at n_step = 1 are recorded, the float64 field of tests/voxel_cases.py is
    evaluated on them and composited in float64.  Sticks: the torch-path loop
    (fused_field = False).  The image follows the 2x rule on row_err.
    weights_sum and depth: |y - r| <= max(2 |t - r|, W) per ray, with W the
    field's float32 window propagated through the compositing plus the
    compositing's own float32 roundings:
      ws = 1 - exp(-sum sigma_i dt_i) is 1-Lipschitz in D = sum_i dt_i dsigma_i;
      every sample adds an f32 product, the fast exp (one rounding of its
      argument, relative error sigma dt 2^-24, and ~ 2 ulp of the result), a
      subtraction, a product and an add on values <= 1: (sigma_i dt_i + 6) 2^-24;
          W_ws = sum_i dt_i w_sigma_i + sum_i (sigma_i dt_i + 6) 2^-24
      depth = sum_i w_i t_i with sum_i |dw_i| <= 2 D (dw_i = T_i dt_i (1 -
      alpha_i) dsigma_i - w_i sum_{j<i} dt_j dsigma_j) and t_i <= t_last, and one
      more rounding per sample for t itself and the fma:
          W_depth = 2 t_last W_ws + 2 n 2^-24 t_last."""
    lines = []
    for ckpt, bits in (("small", "ones"), ("large", "random")):
        net, sd, _ = nets[ckpt]
        set_bits(net, bits, seed=8)
        rays_o, rays_d = rays(gpu, 16, 16, seed=6)
        N = rays_o.shape[0]
        kw = dict(T_thresh=0.0, max_steps=128)
        got, samples = fused(net, rays_o, rays_d, **kw)
        nat, nat_samples, steps = loop(net, rays_o, rays_d, keep=True, **kw)
        stick, stick_samples, _ = loop(net, rays_o, rays_d, fused_field=False, **kw)
        assert samples == nat_samples == stick_samples
        assert_bits(got, nat, "fused vs native loop")
        steps = [(a.cpu().numpy().astype(np.int64), x.cpu(), d.cpu().numpy()) for a, x, d in steps]
        x = torch.cat([s[1] for s in steps])
        rs, ra, _, aux = vc.truth(sd, x)
        w_sigma, _ = vc.windows(rs, aux)
        sigma, rgb, w_sigma = rs.detach().numpy(), ra.detach().numpy(), w_sigma.numpy()
        nears = near_far(net, rays_o, rays_d)[0].cpu().numpy()
        ws, dp, img, t_last = composite64(steps, sigma, rgb, nears, N)
        # the windows, accumulated per ray
        W_ws, count, pos = np.zeros(N), np.zeros(N), 0
        for ids, _, deltas in steps:
            n = len(ids)
            live = deltas[:, 0] > 0
            i, dt = ids[live], deltas[live, 0].astype(np.float64)
            sg, wg = sigma[pos:pos + n][live], w_sigma[pos:pos + n][live]
            W_ws[i] += dt * wg + (sg * dt + 6) * vc.EPS
            count[i] += 1
            pos += n
        W_dp = 2 * t_last * W_ws + 2 * count * vc.EPS * t_last

        def row_err(y, r):
            return float((np.abs(y - r) / (np.abs(r) + np.abs(r).mean())).max())
        ey, et = row_err(got[2], img), row_err(stick[2], img)
        lines.append(f"parity: render {ckpt} {bits} image: fused {ey:.3e} torch-loop {et:.3e} "
                     f"({samples} samples)")
        checks = [("image", ey <= 2 * et)]
        for name, k, r, W in (("weights_sum", 0, ws, W_ws), ("depth", 1, dp, W_dp)):
            dy, dt_ = np.abs(got[k] - r), np.abs(stick[k] - r)
            lines.append(f"parity: render {ckpt} {bits} {name}: fused {dy.max():.3e} "
                         f"({(dy / np.maximum(W, 1e-300)).max():.3f} W) torch-loop {dt_.max():.3e} "
                         f"({(dt_ / np.maximum(W, 1e-300)).max():.3f} W)")
            checks.append((name, bool((dy <= np.maximum(2 * dt_, W)).all())))
        print("\n".join(lines[-3:]))
        assert (ws > 0).sum() > 64
        for name, ok in checks:
            assert ok, (ckpt, name, lines[-3:])
    out = ROOT / "profiles" / "voxel" / "render_parity.txt"
    try:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text("\n".join(lines) + "\n")
    except OSError:
        pass  # a read-only checkout: the figures are on stdout


# ---------------------------------------------------------------- 6. determinism, cache
def test_two_frames_are_equal(gpu, nets):
    net = nets["small"][0]
    set_bits(net, "random", seed=3)
    rays_o, rays_d = rays(gpu, 32, 32, seed=7)
    for shading in SHADINGS:
        a, sa = fused(net, rays_o, rays_d, shading=shading, ratio=0.1)
        b, sb = fused(net, rays_o, rays_d, shading=shading, ratio=0.1)
        assert sa == sb
        assert_bits(a, b, shading)


def make_trainer(gpu, nets, seed):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt",
                          nets["small"][2], "--h", "16", "--w", "16", "--guidance", "synthetic",
                          "--seed", str(seed)])
    seed_everything(seed)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=None, optimizer=optimizer, ema_decay=None, fp16=True,
                      use_checkpoint="scratch", mute=True)
    data = NeRFDataset(opt, device=gpu, type="train", H=16, W=16, size=100)
    return trainer, data


def test_no_stale_operands_after_a_train_step(gpu, nets):
    """A frame, one Trainer step (the native Adam writes rgbnet in place), a
    frame: the second equals the loop on the updated weights and differs from
    the first."""
    trainer, data = make_trainer(gpu, nets, 5)
    model = trainer.model
    model.density_bitfield.fill_(255)
    rays_o, rays_d = rays(gpu, 16, 16, seed=8)
    model.eval()
    first, _ = fused(model, rays_o, rays_d)
    model.train()
    before = copy.deepcopy(model.main_net.rgbnet.state_dict())
    torch.manual_seed(11)
    trainer.optimizer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        _, _, loss = trainer.train_step(data.collate([0]), "albedo", 1.0)
    trainer.backward_only(loss)
    trainer.optimizer_step()
    after = model.main_net.rgbnet.state_dict()
    assert any(not torch.equal(after[k], before[k]) for k in before)
    model.eval()
    model.density_bitfield.fill_(255)
    second, samples = fused(model, rays_o, rays_d)
    want, want_samples, _ = loop(model, rays_o, rays_d)
    assert samples == want_samples
    assert_bits(second, want, "after the step")
    assert not np.array_equal(first[2], second[2])


# ---------------------------------------------------------------- 7. dispatch
def render(net, rays_o, rays_d, shading, autocast=torch.float16, ratio=0.1):
    counts = (net.native_render_calls, net.native_calls + net.native_normal_calls, net.torch_calls)
    ctx = (torch.autocast("cuda", dtype=autocast) if autocast is not None
           else torch.autocast("cuda", enabled=False))
    with torch.no_grad(), ctx:
        out = net.render(rays_o[None], rays_d[None], staged=True, perturb=False, max_steps=64,
                         shading=shading, light_d=LIGHT.to(rays_o.device), ambient_ratio=ratio)
    torch.cuda.synchronize()
    delta = (net.native_render_calls - counts[0],
             net.native_calls + net.native_normal_calls - counts[1], net.torch_calls - counts[2])
    return {k: out[k].float().reshape(rays_o.shape[0], -1).cpu().numpy()
            for k in ("image", "depth", "weights_sum")}, delta


def test_dispatch(gpu, nets):
    net, deep = nets["small"][0], nets["deep"][0]
    set_bits(net, "ones")
    set_bits(deep, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=9)
    ref = {}
    for shading in SHADINGS:
        ref[shading], d = render(net, rays_o, rays_d, shading)
        assert d == (1, 1 if shading == "albedo" else 2, 0), (shading, d)
    # the loop: many native field calls, no fused frame; the same frame to the
    # bounds of the shaded test.  The albedo view has none there (it is bit-exact
    # against n_step = 1): 1e-4 as tests/test_gpu_render.py allows the default
    # schedule; on the torch field one f16 ulp of an albedo below 1 per sample,
    # 2^-11, composited with weights summing to <= 1, doubled: 2^-10
    bounds = {"albedo": 1e-4, "textureless": B_TL, "lambertian": B_TL, "normal": B_N}
    for switch in ("native_infer", "fused_field"):
        for shading in SHADINGS:
            setattr(net, switch, False)
            try:
                out, d = render(net, rays_o, rays_d, shading)
            finally:
                setattr(net, switch, True)
            assert d[0] == 0, (switch, shading)
            bound = bounds[shading]
            if switch == "native_infer":
                assert d[1] > 2 and d[2] == 0
            else:  # the torch field: f16 albedo of another summation order
                assert d[1] == 0 and d[2] > 2
                if shading == "albedo":
                    bound = 2.0 ** -10
            err = {k: float(np.abs(out[k] - ref[shading][k]).max()) for k in out}
            print(f"parity: dispatch {switch} = False {shading}: {err}")
            assert err["image"] <= bound, (switch, shading, err)
            assert max(err["weights_sum"], err["depth"]) <= 1e-4, (switch, shading, err)
    # bf16 and no autocast, a depth-4 rgbnet, an unknown shading: the loop
    for autocast in (torch.bfloat16, None):
        out, d = render(net, rays_o, rays_d, "albedo", autocast=autocast)
        assert d[0] == 0 and d[2] > 2
        assert np.abs(out["weights_sum"] - ref["albedo"]["weights_sum"]).max() <= 1e-3
        # bf16 activations: 2^-8 relative per layer, three layers, 1/4 through the sigmoid
        assert np.abs(out["image"] - ref["albedo"]["image"]).max() <= 2.0 ** -6
    out, d = render(deep, rays_o, rays_d, "lambertian")
    assert d[0] == 0 and d[2] > 2 and np.isfinite(out["image"]).all()
    with torch.autocast("cuda", dtype=torch.float16):
        assert net.native_infer_field("phong", rays_o) is None
        assert deep.native_infer_field("albedo", rays_o) is None
        assert net.native_infer_field("albedo", rays_o.cpu()) is None


# ---------------------------------------------------------------- 8. the Trainer's views
def test_trainer_views_go_through_the_kernel(gpu, nets):
    from nerf.provider import NeRFDataset
    trainer, _ = make_trainer(gpu, nets, 6)
    model = trainer.model
    model.density_bitfield.fill_(255)
    model.eval()
    ds = NeRFDataset(trainer.opt, device=gpu, type="test", H=32, W=32, size=4)
    for shading in ("albedo", "lambertian"):
        batch = ds.collate([1])
        batch["shading"], batch["ambient_ratio"] = shading, 0.1
        batch["light_d"] = LIGHT.to(gpu)
        outs = {}
        for native in (True, False):
            model.native_infer = native
            n0 = model.native_render_calls
            try:
                with torch.autocast("cuda", dtype=torch.float16):
                    img, depth = trainer.test_step(batch)
                    img2, depth2, loss = trainer.eval_step(batch)
            finally:
                model.native_infer = True
            assert model.native_render_calls - n0 == (2 if native else 0)
            if native:
                assert model.infer_tile_w == 32
            assert img.shape == (1, 32, 32, 3) and torch.isfinite(loss)
            outs[native] = [t.float().cpu().numpy() for t in (img, depth, img2, depth2)]
        for a, b in zip(outs[True], outs[False]):
            # the default schedule's 1e-4 (tests/test_gpu_render.py), the f16 light product
            assert np.abs(a - b).max() <= (1e-4 if shading == "albedo" else B_TL), shading
