"""GPU tests of the vanilla backbone's fused persistent inference renderer
(csrc/resmlprender.hip, dfhip_resmlp_render_rays_infer, dispatched by
NeRFRenderer._infer_fused on nerf/vanilla_field.py's InferField; albedo only).

The yardstick is the renderer's own host loop at n_step = 1 on the native
field (`_infer_loop(..., n_step_max=1)`): the kernel runs the same device
functions in the same order (-ffp-contract=off, MFMA columns independent), so
weights_sum, depth, the image and the sample count must be the loop's bits:
assert_array_equal everywhere, no tolerance.  Each link of that loop is pinned
elsewhere: the field to the float64 restatement (tests/test_gpu_vanilla.py),
the march and the compositing to oracle/ (tests/test_gpu_raymarching.py,
tests/test_gpu_march_settings.py).

Counters.  A fused frame raises `native_render_calls` by one, counts ONCE in
`native_calls` (the loop counts one per iteration) and leaves `torch_calls`
alone.

The nets are seeded 39 -> 128 x4 -> 4 networks with randomised LayerNorm
weights and biases; the field's density is about 1 away from the Gaussian
blob, so at max_steps = 128 (dt ~ 0.027) a ray through the box takes about 70
samples and retires at far.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scenes

pytestmark = pytest.mark.gpu

LIGHT = F.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
SHADED = ["textureless", "lambertian", "normal"]


# ---------------------------------------------------------------- helpers
def make_net(gpu, seed=0, args=(), **kw):
    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla", *args])
    torch.manual_seed(seed)
    net = NeRFNetwork(opt, **kw).to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.sigma_net.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    net.eval()
    return net


@pytest.fixture(scope="module")
def nets(gpu):
    base = make_net(gpu)
    dense = copy.deepcopy(base)
    with torch.no_grad():  # sigma ~ e^6: T < 1e-4 after a sample or two
        dense.sigma_net.net[4].bias[0] += 6.0
    # the trained-like head of tests/field_head_cases.py: h0 + gaussian spans
    # about [-70, 70] and a third of the albedo entries are exactly 0 or 1
    import field_head_cases as fc
    trained = fc.load_params(make_net(gpu), fc.vanilla_case()["trained"])
    out = {"base": base, "dense": dense, "bound2": make_net(gpu, 1, args=("--bound", "2")),
           "narrow": make_net(gpu, 2, hidden_dim=64), "trained": trained}
    assert out["base"].cascade == 1 and out["bound2"].cascade == 2
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
    """Wraps raymarching.march_rays: counts what the loop marched."""

    def __init__(self):
        import raymarching
        self.mod, self.orig, self.samples = raymarching, raymarching.march_rays, 0

    def __enter__(self):
        def march(n_alive, n_step, rays_alive, *a, **k):
            xyzs, dirs, deltas = self.orig(n_alive, n_step, rays_alive, *a, **k)
            self.samples += int((deltas[:n_alive * n_step, 0] > 0).sum())
            return xyzs, dirs, deltas
        self.mod.march_rays = march
        return self

    def __exit__(self, *exc):
        self.mod.march_rays = self.orig


def near_far(net, rays_o, rays_d):
    import raymarching
    return raymarching.near_far_from_aabb(rays_o, rays_d, net.aabb_infer)


def fused(net, rays_o, rays_d, perturb=False, T_thresh=1e-4, max_steps=128, dt_gamma=0.0, seed=7):
    """(weights_sum, depth, image) numpy and the sample count of one fused frame."""
    nears, fars = near_far(net, rays_o, rays_d)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        field = net.native_infer_field("albedo", rays_o)
        assert field is not None and field.kind == "vanilla"
        torch.manual_seed(seed)
        out = net._infer_fused(rays_o, rays_d, nears, fars, field, perturb, dt_gamma, max_steps,
                               T_thresh, shading="albedo")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out], samples_of(net)


def loop(net, rays_o, rays_d, perturb=False, T_thresh=1e-4, max_steps=128, dt_gamma=0.0, seed=7):
    """The host loop at n_step = 1 on the native field."""
    nears, fars = near_far(net, rays_o, rays_d)
    before = (net.native_calls, net.torch_calls)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), Recorder() as rec:
        torch.manual_seed(seed)
        out = net._infer_loop(rays_o, rays_d, nears, fars, LIGHT.to(rays_o.device), 1.0, "albedo",
                              perturb, dt_gamma, max_steps, T_thresh, n_step_max=1)
    torch.cuda.synchronize()
    if rays_o.shape[0]:
        assert net.native_calls > before[0] and net.torch_calls == before[1]
    return [t.cpu().numpy() for t in out], rec.samples


def assert_bits(got, want, what):
    for name, a, b in zip(("weights_sum", "depth", "image"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")


def both(net, rays_o, rays_d, what, **kw):
    """One fused frame against the loop: the same bits and sample count."""
    want, want_samples = loop(net, rays_o, rays_d, **kw)
    got, samples = fused(net, rays_o, rays_d, **kw)
    assert samples == want_samples, what
    assert_bits(got, want, what)
    assert all(np.isfinite(a).all() for a in got)
    return got, samples


# ---------------------------------------------------------------- 1, 2: full / sparse grid
def test_full_bitfield_and_counters(gpu, nets):
    net = nets["base"]
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16)
    got, samples = both(net, rays_o, rays_d, "full")
    assert samples > 10 * 256
    assert (got[0] > 0).all()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        before = (net.native_render_calls, net.native_calls, net.native_normal_calls,
                  net.torch_calls)
        out = net.render(rays_o[None], rays_d[None], staged=True, perturb=False, max_steps=128,
                         bg_color=None)
    after = (net.native_render_calls, net.native_calls, net.native_normal_calls, net.torch_calls)
    assert after == (before[0] + 1, before[1] + 1, before[2], before[3])
    assert samples_of(net) == samples
    np.testing.assert_array_equal(out["weights_sum"].reshape(-1).cpu().numpy(), got[0])
    assert out["image"].shape == (1, 256, 3) and torch.isfinite(out["image"]).all()


def test_random_bitfield(gpu, nets):
    net = nets["base"]
    set_bits(net, "random", seed=5)
    rays_o, rays_d = rays(gpu, 16, 16, seed=2)
    _, samples = both(net, rays_o, rays_d, "random")
    set_bits(net, "ones")
    _, full = fused(net, rays_o, rays_d)
    assert 0 < samples < full // 2  # most of the box is skipped


def test_trained_head_frame(gpu, nets):
    """A frame through a field whose density spans e^-70 .. e^70 (empty space
    beside solid cells along one ray) and whose colours saturate: the loop's
    bits all the same."""
    net = nets["trained"]
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=8)
    got, samples = both(net, rays_o, rays_d, "trained head")
    assert samples > 256
    assert (got[0] > 0.99).any()  # some ray met a solid cell


# ---------------------------------------------------------------- 3, 4: ray counts
@pytest.mark.parametrize("n", [1, 15, 65, 257])
def test_ray_counts(gpu, nets, n):
    net = nets["base"]
    set_bits(net, "random", seed=3)
    o, d = rays(gpu, 20, 20, seed=1)
    _, samples = both(net, o[:n].contiguous(), d[:n].contiguous(), f"N = {n}")
    assert samples > 0


def test_no_rays(gpu, nets):
    net = nets["base"]
    set_bits(net, "ones")
    o, d = rays(gpu, 4, 4)
    fused(net, o, d)  # leaves a count behind
    assert samples_of(net) > 0
    got, samples = fused(net, o[:0].contiguous(), d[:0].contiguous())
    assert samples == 0 and (net.last_infer_work.cpu().numpy() == 0).all()
    assert [a.shape for a in got] == [(0,), (0,), (0, 3)]


# ---------------------------------------------------------------- 5, 6: noises, cascades
def test_perturbed_march(gpu, nets):
    net = nets["base"]
    set_bits(net, "random", seed=4)
    rays_o, rays_d = rays(gpu, 16, 16, seed=3)
    got, _ = both(net, rays_o, rays_d, "perturb", perturb=True)
    plain, _ = fused(net, rays_o, rays_d)
    assert not np.array_equal(got[1], plain[1])  # the noises moved the samples


def test_dt_gamma_and_two_cascades(gpu, nets):
    rays_o, rays_d = rays(gpu, 16, 16, seed=4)
    net = nets["base"]
    set_bits(net, "ones")
    both(net, rays_o, rays_d, "dt_gamma", dt_gamma=1 / 128)
    wide = nets["bound2"]
    for bits in ("ones", "random"):
        set_bits(wide, bits, seed=6)
        for dt_gamma in (0.0, 1 / 128):
            _, samples = both(wide, rays_o, rays_d, f"bound 2 {bits} {dt_gamma}", dt_gamma=dt_gamma,
                              perturb=bits == "random")
            assert samples > 0


# ---------------------------------------------------------------- 7, 8, 9: retirement
def test_retirement_on_T_thresh(gpu, nets):
    rays_o, rays_d = rays(gpu, 16, 16, seed=5)
    for name in ("base", "dense"):
        set_bits(nets[name], "ones")
    _, default = fused(nets["base"], rays_o, rays_d)
    got, samples = both(nets["dense"], rays_o, rays_d, "dense")
    assert samples < default // 8
    assert (got[0] > 1 - 1e-3).all()


def test_retirement_on_the_step_cap(gpu, nets):
    net = nets["base"]
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=6)
    _, samples = both(net, rays_o, rays_d, "max_steps 8", max_steps=8)
    assert 0 < samples <= 8 * 256


def test_marching_to_far(gpu, nets):
    rays_o, rays_d = rays(gpu, 16, 16, seed=7)
    for name in ("base", "dense"):
        set_bits(nets[name], "ones")
    _, capped = fused(nets["dense"], rays_o, rays_d)
    _, samples = both(nets["dense"], rays_o, rays_d, "T_thresh 0", T_thresh=0.0)
    assert samples > 8 * capped  # no ray retires before far
    both(nets["base"], rays_o, rays_d, "T_thresh 0 base", T_thresh=0.0)


# ---------------------------------------------------------------- 10, 11, 12
def test_queue_layouts(gpu, nets):
    net = nets["base"]
    set_bits(net, "random", seed=9)
    rays_o, rays_d = rays(gpu, 32, 32, seed=4)
    keep = (net.infer_order, net.infer_chunk_log2, net.infer_tile_w)
    variants = [(0, 6, 0), (1, 0, 0), (1, 6, 0), (1, 6, 32), (2, 0, 0), (2, 6, 0), (2, 6, 32)]
    runs = []
    try:
        for flag, cl, tile in variants:
            net.infer_order, net.infer_chunk_log2, net.infer_tile_w = flag, cl, tile
            runs.append(((flag, cl, tile), *fused(net, rays_o, rays_d)))
    finally:
        net.infer_order, net.infer_chunk_log2, net.infer_tile_w = keep
    _, ref, ref_samples = runs[0]  # pixel order
    assert ref_samples > 0
    for v, got, samples in runs[1:]:
        assert samples == ref_samples, v
        assert_bits(got, ref, str(v))


def test_two_frames_are_equal(gpu, nets):
    net = nets["base"]
    set_bits(net, "random", seed=3)
    rays_o, rays_d = rays(gpu, 32, 32, seed=7)
    a, sa = fused(net, rays_o, rays_d)
    b, sb = fused(net, rays_o, rays_d)
    assert sa == sb and sa > 0
    assert_bits(a, b, "second frame")


def test_no_stale_operands_after_an_in_place_update(gpu, nets):
    """Every parameter changes in place between two frames (as an optimizer
    step writes them): the second frame equals the loop on the new weights."""
    net = copy.deepcopy(nets["base"])
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=8)
    first, _ = fused(net, rays_o, rays_d)
    with torch.no_grad():
        for p in net.sigma_net.parameters():
            p.mul_(1.03).add_(0.002)
    second, _ = both(net, rays_o, rays_d, "after the update")
    assert not np.array_equal(first[2], second[2])


# ---------------------------------------------------------------- dispatch
def render(net, rays_o, rays_d, shading, autocast=torch.float16):
    counts = (net.native_render_calls, net.native_calls + net.native_normal_calls, net.torch_calls)
    ctx = (torch.autocast("cuda", dtype=autocast) if autocast is not None
           else torch.autocast("cuda", enabled=False))
    with torch.no_grad(), ctx:
        assert net.native_infer_field(shading, rays_o) is None
        out = net.render(rays_o[None], rays_d[None], staged=True, perturb=False, max_steps=64,
                         shading=shading, light_d=LIGHT.to(rays_o.device), ambient_ratio=0.1,
                         bg_color=None)
    torch.cuda.synchronize()
    delta = (net.native_render_calls - counts[0],
             net.native_calls + net.native_normal_calls - counts[1], net.torch_calls - counts[2])
    assert out["image"].shape == (1, rays_o.shape[0], 3) and torch.isfinite(out["image"]).all()
    return delta


def test_dispatch_negatives(gpu, nets):
    net, narrow = nets["base"], nets["narrow"]
    set_bits(net, "ones")
    set_bits(narrow, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=9)
    for switch in ("native_infer", "fused_field"):
        setattr(net, switch, False)
        try:
            d = render(net, rays_o, rays_d, "albedo")
        finally:
            setattr(net, switch, True)
        assert d[0] == 0, switch
        # the loop: on the native field, or on the torch path
        assert (d[1] > 2 and d[2] == 0) if switch == "native_infer" else (d[1] == 0 and d[2] > 2)
    for autocast in (torch.bfloat16, None):
        d = render(net, rays_o, rays_d, "albedo", autocast=autocast)
        assert d[0] == 0 and d[1] == 0 and d[2] > 2, autocast
    d = render(narrow, rays_o, rays_d, "albedo")
    assert d[0] == 0 and d[1] == 0 and d[2] > 2
    for shading in SHADED:  # the loop with the native field and normal
        d = render(net, rays_o, rays_d, shading)
        assert d[0] == 0 and d[1] > 2 and d[2] == 0, shading
    with torch.autocast("cuda", dtype=torch.float16):
        assert net.native_infer_field("albedo", rays_o) is not None
        assert net.native_infer_field("albedo", rays_o.cpu()) is None


# ---------------------------------------------------------------- end to end
def test_render_and_trainer_views_go_through_the_kernel(gpu, nets):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    net = nets["base"]
    set_bits(net, "ones")
    rays_o, rays_d = rays(gpu, 16, 16, seed=10)
    n0 = net.native_render_calls
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = net.render(rays_o[None], rays_d[None], staged=True, perturb=False, max_steps=64)
    assert net.native_render_calls == n0 + 1
    assert out["image"].shape == (1, 256, 3) and out["depth"].shape == (1, 256)
    assert out["weights_sum"].shape == (1, 256)
    assert all(torch.isfinite(out[k].float()).all() for k in ("image", "depth", "weights_sum"))

    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla", "--h", "16", "--w", "16",
                          "--guidance", "synthetic", "--seed", "3"])
    seed_everything(3)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=None, optimizer=optimizer, ema_decay=None, fp16=True,
                      use_checkpoint="scratch", mute=True)
    model = trainer.model
    model.density_bitfield.fill_(255)
    model.eval()
    ds = NeRFDataset(opt, device=gpu, type="test", H=16, W=16, size=4)
    for shading, frames in (("albedo", 1), ("lambertian", 0)):
        batch = ds.collate([1])
        batch["shading"] = shading
        batch["ambient_ratio"] = 1.0 if shading == "albedo" else 0.1
        batch["light_d"] = LIGHT.to(gpu)
        n0 = model.native_render_calls
        with torch.autocast("cuda", dtype=torch.float16):
            img, depth = trainer.test_step(batch)
        assert model.native_render_calls - n0 == frames, shading
        assert img.shape == (1, 16, 16, 3) and torch.isfinite(img).all(), shading
        assert depth.shape == (1, 16, 16) and torch.isfinite(depth).all(), shading
