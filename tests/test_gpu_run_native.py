"""The native glue of NeRFRenderer.run (csrc/hiersample.hip: coarse samples,
sample_pdf importance samples, the sort of their union, compositing forward
and closed-form backward) against the same arithmetic in torch f64 on the CPU,
and run() / the -O2 trainer on both settings of `native_run`.

Tolerance rule (tests/test_gpu_run.py): the native result's relative L2 error
against the f64 truth is at most 3 x the error of the torch f32 ops on the same
inputs on the same GPU, plus 1e-6.  The coarse samples and the sort are
bit-equal to torch instead.

N = 67 rays (not a multiple of the 4 rays of a workgroup): ray 0 misses the
box (near = far = FLT_MAX), ray 1 starts inside it.  Densities are a Gaussian
bump along each ray, at a "soft" scale (ray opacities spread over (0, 1)) and
a "hard" one (most rays opaque, alpha rounding to 1 on several samples)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 67
SIZES = [(3, 1), (16, 16), (17, 30), (33, 32), (64, 64), (100, 93), (256, 256), (64, 0)]
MIN_NEAR = 0.1


def rel_err(a, e):
    a, e = a.detach().double().cpu(), e.detach().double().cpu()
    return float((a - e).norm() / e.norm().clamp(min=1e-30))


def check_rule(what, native, torch32, exact):
    en, et = rel_err(native, exact), rel_err(torch32, exact)
    print(f"{what}: native {en:.3e} torch-f32 {et:.3e}")
    assert math.isfinite(en) and en <= 3 * et + 1e-6, (what, en, et)


# ------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def rays(gpu):
    import raymarching
    g = torch.Generator().manual_seed(7)
    o = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1) * 1.8
    target = (torch.rand(N, 3, generator=g) - 0.5) * 0.8
    d = torch.nn.functional.normalize(target - o, dim=-1)
    o[0] = torch.tensor([0.3, 0.2, 1.8])  # passes beside the box
    d[0] = torch.nn.functional.normalize(torch.tensor([1.0, 0.1, 0.05]), dim=-1)
    o[1] = torch.tensor([0.1, 0.2, -0.3])  # inside the box
    o, d = o.to(gpu).contiguous(), d.to(gpu).contiguous()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device=gpu)
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, MIN_NEAR)
    hit = nears < fars
    assert not bool(hit[0]) and bool(hit[1:].all()) and float(nears[0]) == float(fars[0])
    assert float(nears[1]) == pytest.approx(MIN_NEAR)
    return dict(o=o, d=d, aabb=aabb, nears=nears, fars=fars, hit=hit.cpu())


class Bumps:
    """sigma(z) = height exp(-((z - centre) / width)^2 / 2) per ray, in f64.

    "soft": the bump's optical depth tau is log-uniform over 0.05 .. 3, so ray
    opacities spread over (0, 1).  "hard": of the rays, taken in a random
    order, 7 are saturated (tau 1000 .. 4000, narrow: sigma dz > 17 and alpha
    rounds to 1 on their central samples at every size tested), 36 opaque (tau
    5 .. 15, opacity > 0.99) and the rest soft (tau 0.05 .. 2).

    The opaque rays' bumps are wide (0.08 .. 0.15 of the ray) and sit in its
    far half.  A bin of weight < 1e-6 on a ray of opacity W > 0.9 has a pdf span
    of 1e-5 / (W + (T - 2) 1e-5), inside the coin-toss class of
    test_importance_samples, and a uniform u falls into it with that
    probability: a ray whose bins are mostly empty puts up to (T - 2) 1e-5 of
    its samples there, 0.25 % at T = 256.  The class may hold 0.1 % of a
    case's samples, so the opaque rays must keep most of their bins above
    1e-6, which a wide bump reaching back to the ray's start does, with the
    bins behind it still seeing a transmittance of e^-15 = 3e-7 or more.
    Expected share at T = 256: (36 x 0.25 + 7 x 0.85) / 66 empty bins per bin
    x 0.25 % = 0.06 %."""

    def __init__(self, rays, mode, seed):
        g = torch.Generator().manual_seed(seed)
        rand = lambda: torch.rand(N, generator=g, dtype=torch.float64)  # noqa: E731
        near, far = rays["nears"].double().cpu(), rays["fars"].double().cpu()
        near, far = torch.where(rays["hit"], near, torch.zeros(())), torch.where(
            rays["hit"], far, torch.ones(()))
        span = far - near
        log_uniform = lambda lo, hi: lo * (hi / lo) ** rand()  # noqa: E731
        centre, width, tau = 0.15 + 0.7 * rand(), 0.02 + 0.13 * rand(), log_uniform(0.05, 3.0)
        if mode == "hard":
            rank = torch.argsort(torch.argsort(rand()))
            saturated, opaque = rank < 7, (rank >= 7) & (rank < 43)
            tau = torch.where(saturated, log_uniform(1000.0, 4000.0),
                              torch.where(opaque, log_uniform(5.0, 15.0), log_uniform(0.05, 2.0)))
            width = torch.where(saturated, 0.03 + 0.05 * rand(),
                                torch.where(opaque, 0.08 + 0.07 * rand(), width))
            centre = torch.where(opaque, 0.5 + 0.3 * rand(), centre)
        self.centre = near + span * centre
        self.width = span * width
        self.height = tau / (self.width * math.sqrt(2 * math.pi))

    def __call__(self, z):
        zc = z.double().cpu()
        s = self.height[:, None] * torch.exp(-0.5 * ((zc - self.centre[:, None])
                                                     / self.width[:, None]) ** 2)
        return s.float()


def coarse(rays, T, seed):
    import raymarching
    gpu = rays["o"].device
    lin = torch.linspace(0.0, 1.0, T, device=gpu)
    noise = torch.rand(N, T, device=gpu, generator=torch.Generator(gpu).manual_seed(seed))
    z, xyzs = raymarching.uniform_samples(rays["o"], rays["d"], rays["aabb"], rays["nears"],
                                          rays["fars"], lin, noise)
    return lin, noise, z, xyzs


def positions(rays, z):
    x = rays["o"].unsqueeze(-2) + rays["d"].unsqueeze(-2) * z.unsqueeze(-1)
    return torch.min(torch.max(x, rays["aabb"][:3]), rays["aabb"][3:])


# ----------------------------------------------------------- coarse samples
@pytest.mark.parametrize("T", sorted({T for T, _ in SIZES}))
def test_uniform_samples_are_bit_equal_to_torch(gpu, rays, T):
    import raymarching
    lin, noise, z, xyzs = coarse(rays, T, seed=T)
    nears, fars = rays["nears"].unsqueeze(-1), rays["fars"].unsqueeze(-1)
    want = nears + (fars - nears) * lin.unsqueeze(0).expand((N, T))
    sample_dist = (fars - nears) / T
    z0, xyzs0 = raymarching.uniform_samples(rays["o"], rays["d"], rays["aabb"], rays["nears"],
                                            rays["fars"], lin)
    assert torch.equal(z0, want) and torch.equal(xyzs0, positions(rays, want))
    want = want + (noise - 0.5) * sample_dist
    assert torch.equal(z, want) and torch.equal(xyzs, positions(rays, want))
    assert torch.isfinite(xyzs).all()


# ------------------------------------------------------- importance samples
def ref_importance(z, sigma, nears, fars, T, t, u):
    """renderer.py:358-370 and sample_pdf in the dtype of its inputs (f64 on the
    CPU: the truth; f32 on the GPU: the torch path).  Returns new_z, and the
    span and bin edges of every sample."""
    nears, fars = nears.unsqueeze(-1), fars.unsqueeze(-1)
    sample_dist = (fars - nears) / T
    dz = z[..., 1:] - z[..., :-1]
    dz = torch.cat([dz, sample_dist * torch.ones_like(dz[..., :1])], dim=-1)
    alphas = 1 - torch.exp(-dz * sigma)
    trans = torch.cumprod(torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15],
                                    dim=-1), dim=-1)[..., :-1]
    weights = alphas * trans
    bins = z[..., :-1] + 0.5 * dz[..., :-1]
    w = weights[:, 1:-1] + 1e-5
    pdf = w / w.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)
    u = u.contiguous()
    hi_idx = torch.searchsorted(cdf, u, right=True)
    lo = (hi_idx - 1).clamp(min=0)
    hi = hi_idx.clamp(max=cdf.shape[-1] - 1)
    span = torch.gather(cdf, 1, hi) - torch.gather(cdf, 1, lo)
    den = torch.where(span < 1e-5, torch.ones_like(span), span)
    b_lo, b_hi = torch.gather(bins, 1, lo), torch.gather(bins, 1, hi)
    return b_lo + (u - torch.gather(cdf, 1, lo)) / den * (b_hi - b_lo), span, b_lo, b_hi


@pytest.mark.parametrize("scale", ["soft", "hard"])
@pytest.mark.parametrize("T,t", [s for s in SIZES if s[1] > 0])
def test_importance_samples(gpu, rays, T, t, scale):
    """new_z against the f64 truth under the rule, for given and deterministic u.

    The share of coin-toss samples follows from the inputs' f64 arithmetic
    alone (see Bumps).  Measured on an MI355X with u given: 1.63e-4 at soft
    100+93, 3.26e-4 at hard 100+93, 5.33e-4 at hard 256+256, 0 in every other
    case."""
    import raymarching
    _, _, z, _ = coarse(rays, T, seed=100 + T)
    sigma = Bumps(rays, scale, seed=T + t)(z).to(gpu)
    hit = rays["hit"]
    cpu64 = lambda a: a.double().cpu()  # noqa: E731
    u_rand = torch.rand(N, t, device=gpu, generator=torch.Generator(gpu).manual_seed(t))
    u_det32 = torch.linspace(0.5 / t, 1.0 - 0.5 / t, t, device=gpu).expand(N, t)
    u_det64 = ((torch.arange(t, dtype=torch.float64) + 0.5) / t).expand(N, t)
    shares = []
    for what, u_native, u32, u64 in (("u given", u_rand, u_rand, cpu64(u_rand)),
                                     ("deterministic u", None, u_det32, u_det64)):
        new_z, new_xyzs = raymarching.importance_samples(
            rays["o"], rays["d"], rays["aabb"], rays["nears"], rays["fars"], z, sigma, t, u_native)
        assert new_z.shape == (N, t) and new_xyzs.shape == (N, t, 3)
        assert torch.equal(new_xyzs, positions(rays, new_z))
        exact, span, b_lo, b_hi = ref_importance(cpu64(z), cpu64(sigma), cpu64(rays["nears"]),
                                                 cpu64(rays["fars"]), T, t, u64)
        torch32 = ref_importance(z, sigma, rays["nears"], rays["fars"], T, t, u32)[0]
        # the span < 1e-5 switch is a coin toss in f32 where the exact span is
        # within 1e-6 of it: such a sample only has to lie inside its bin
        toss = ((span - 1e-5).abs() < 1e-6) & hit[:, None]
        share = float(toss.sum()) / (int(hit.sum()) * t)
        print(f"{scale} {T}+{t} {what}: coin-toss share {share:.2e}")
        shares.append(share)
        got = cpu64(new_z)
        slack = 1e-6 * b_hi.abs()  # f32 rounding of the bin edges
        assert ((got >= b_lo - slack) & (got <= b_hi + slack))[toss].all()
        keep = hit[:, None] & ~toss
        pick = lambda a: torch.where(keep, cpu64(a), torch.zeros((), dtype=torch.float64))  # noqa
        check_rule(f"{scale} {T}+{t} {what}", pick(new_z), pick(torch32), pick(exact))
        # the ray that misses: every depth is its near = far, as in torch
        assert torch.equal(new_z[0], torch32[0])
    # at most 0.1 % of a case's samples may take the weaker check
    assert max(shares) <= 1e-3, shares


# -------------------------------------------------------------------- merge
def check_merge(z, new_z, xyzs, new_xyzs):
    import raymarching
    T, t = z.shape[1], new_z.shape[1]
    z_all, order, xyzs_all = raymarching.merge_samples(z, new_z, xyzs, new_xyzs)
    both = torch.cat([z, new_z], 1)
    assert order.dtype == torch.int32 and order.shape == (N, T + t)
    assert torch.equal(z_all, torch.sort(both, dim=1)[0])
    idx = order.long()
    assert torch.equal(torch.sort(idx, dim=1)[0], torch.arange(T + t, device=z.device).expand(N, -1))
    assert torch.equal(torch.gather(both, 1, idx), z_all)
    both_xyzs = torch.cat([xyzs, new_xyzs], 1)
    assert torch.equal(xyzs_all, torch.gather(both_xyzs, 1, idx.unsqueeze(-1).expand(-1, -1, 3)))
    return z_all, order


@pytest.mark.parametrize("T,t", [s for s in SIZES if s[1] > 0])
def test_merge_samples(gpu, rays, T, t):
    import raymarching
    _, _, z, xyzs = coarse(rays, T, seed=200 + T)
    sigma = Bumps(rays, "soft", seed=T)(z).to(gpu)
    u = torch.rand(N, t, device=gpu, generator=torch.Generator(gpu).manual_seed(3))
    new_z, new_xyzs = raymarching.importance_samples(
        rays["o"], rays["d"], rays["aabb"], rays["nears"], rays["fars"], z, sigma, t, u)
    check_merge(z, new_z, xyzs, new_xyzs)


def test_merge_orders_ties_by_concatenation_index(gpu, rays):
    T, t = 33, 32
    _, _, z, xyzs = coarse(rays, T, seed=5)
    pick = torch.randint(0, T, (N, t), device=gpu, generator=torch.Generator(gpu).manual_seed(9))
    new_z = torch.gather(z, 1, pick)  # every new depth ties with a coarse one (and some twice)
    new_xyzs = torch.rand(N, t, 3, device=gpu, generator=torch.Generator(gpu).manual_seed(2))
    z_all, order = check_merge(z, new_z, xyzs, new_xyzs)
    assert bool((z_all[0] == z_all[0, 0]).all())  # the ray that misses: all depths equal
    assert torch.equal(order[0], torch.arange(T + t, device=gpu, dtype=torch.int32))
    # among equal depths the concatenation index ascends
    tie = z_all[:, 1:] == z_all[:, :-1]
    assert int(tie.sum()) >= N * t
    assert bool((order[:, 1:] > order[:, :-1])[tie].all())


# ---------------------------------------------------------------- composite
def ref_composite(sigma_c, sigma_n, order, z_all, nears, fars, sample_dist, rgbs):
    """renderer.py:387-393, 414-421 in the dtype of its inputs."""
    sig = sigma_c if sigma_n is None else torch.gather(torch.cat([sigma_c, sigma_n], 1), 1, order)
    nears, fars, sample_dist = nears.unsqueeze(-1), fars.unsqueeze(-1), sample_dist.unsqueeze(-1)
    dz = z_all[..., 1:] - z_all[..., :-1]
    dz = torch.cat([dz, sample_dist * torch.ones_like(dz[..., :1])], dim=-1)
    alphas = 1 - torch.exp(-dz * sig)
    trans = torch.cumprod(torch.cat([torch.ones_like(alphas[..., :1]), 1 - alphas + 1e-15],
                                    dim=-1), dim=-1)[..., :-1]
    weights = alphas * trans
    weights_sum = weights.sum(dim=-1)
    depth = torch.sum(weights * ((z_all - nears) / (fars - nears)).clamp(0, 1), dim=-1)
    image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2)
    return weights_sum, depth, image, weights


COMPOSITE_CASES = {}


def composite_case(gpu, rays, T, t, scale):
    """Inputs of one (T, t, scale), with the f64 truth and the torch f32 result
    of the forward and of both backward runs: computed once, then only read."""
    key = (T, t, scale)
    if key in COMPOSITE_CASES:
        return COMPOSITE_CASES[key]
    import raymarching
    _, _, z, xyzs = coarse(rays, T, seed=300 + T)
    bumps = Bumps(rays, scale, seed=2 * T + t)
    sigma_c = bumps(z).to(gpu)
    if t > 0:
        u = torch.rand(N, t, device=gpu, generator=torch.Generator(gpu).manual_seed(T))
        new_z, new_xyzs = raymarching.importance_samples(
            rays["o"], rays["d"], rays["aabb"], rays["nears"], rays["fars"], z, sigma_c, t, u)
        sigma_n = bumps(new_z).to(gpu)
        z_all, order, _ = raymarching.merge_samples(z, new_z, xyzs, new_xyzs)
    else:
        sigma_n, order, z_all = None, None, z
    gen = torch.Generator(gpu).manual_seed(T + 3 * t)
    M = T + t
    rgbs = torch.rand(N, M, 3, device=gpu, generator=gen)
    sample_dist = (rays["fars"] - rays["nears"]) / T
    inputs = dict(sigma_c=sigma_c, sigma_n=sigma_n, order=order, z_all=z_all, nears=rays["nears"],
                  fars=rays["fars"], sample_dist=sample_dist)
    ups = dict(ws=torch.randn(N, device=gpu, generator=gen),
               depth=torch.randn(N, device=gpu, generator=gen),
               image=torch.randn(N, 3, device=gpu, generator=gen))

    def reference(dtype, device, rgbs_in):
        cast = lambda a: None if a is None else (  # noqa: E731
            a.to(device) if a.dtype in (torch.int32, torch.int64) else a.to(device, dtype))
        leaves = [cast(sigma_c).requires_grad_(), None if t == 0 else cast(sigma_n).requires_grad_(),
                  cast(rgbs_in.float()).requires_grad_()]
        out = ref_composite(leaves[0], leaves[1], None if t == 0 else cast(order.long()),
                            cast(z_all), cast(inputs["nears"]), cast(inputs["fars"]),
                            cast(sample_dist), leaves[2])
        hit = rays["hit"].to(device)
        grads = {}
        # all three outputs (the ray that misses has a NaN depth: left out of
        # this run), then image and weights_sum only (every ray)
        ins = [x for x in leaves if x is not None]
        loss = ((out[0] * cast(ups["ws"]))[hit].sum() + (out[1] * cast(ups["depth"]))[hit].sum()
                + (out[2] * cast(ups["image"]))[hit].sum())
        grads["all"] = torch.autograd.grad(loss, ins, retain_graph=True)
        loss = (out[0] * cast(ups["ws"])).sum() + (out[2] * cast(ups["image"])).sum()
        grads["no_depth"] = torch.autograd.grad(loss, ins)
        return [o.detach() for o in out], grads

    case = dict(inputs=inputs, rgbs=rgbs, ups=ups,
                exact=reference(torch.float64, "cpu", rgbs),
                torch32=reference(torch.float32, gpu, rgbs),
                exact_h=reference(torch.float64, "cpu", rgbs.half()))
    COMPOSITE_CASES[key] = case
    return case


def native_composite(case, rgbs):
    import raymarching
    i = case["inputs"]
    sigma_c = i["sigma_c"].clone().requires_grad_()
    sigma_n = None if i["sigma_n"] is None else i["sigma_n"].clone().requires_grad_()
    rgbs = rgbs.clone().requires_grad_()
    out = raymarching.composite_uniform(sigma_c, sigma_n, i["order"], i["z_all"], i["nears"],
                                        i["fars"], i["sample_dist"], rgbs)
    return out, [x for x in (sigma_c, sigma_n, rgbs) if x is not None]


@pytest.mark.parametrize("scale", ["soft", "hard"])
@pytest.mark.parametrize("T,t", SIZES)
def test_composite_forward(gpu, rays, T, t, scale):
    case = composite_case(gpu, rays, T, t, scale)
    hit = rays["hit"]
    for half in (False, True):
        rgbs = case["rgbs"].half() if half else case["rgbs"]
        (ws, depth, image, weights), _ = native_composite(case, rgbs)
        assert not weights.requires_grad and ws.dtype == depth.dtype == image.dtype == torch.float32
        exact = (case["exact_h"] if half else case["exact"])[0]
        t32 = case["torch32"][0]
        tag = f"{scale} {T}+{t} {'f16' if half else 'f32'}"
        check_rule(f"{tag} weights", weights, t32[3], exact[3])
        check_rule(f"{tag} weights_sum", ws, t32[0], exact[0])
        check_rule(f"{tag} depth", depth.cpu()[hit], t32[1].cpu()[hit], exact[1][hit])
        if half:  # the torch path reads the same f16 colours (cast to f32)
            t32_image = ref_composite(*[case["inputs"][k] if k != "order" or t == 0
                                        else case["inputs"][k].long() for k in (
                "sigma_c", "sigma_n", "order", "z_all", "nears", "fars", "sample_dist")],
                rgbs.float())[2]
        else:
            t32_image = t32[2]
        check_rule(f"{tag} image", image, t32_image, exact[2])
        # the ray that misses the box: nothing composited, a NaN depth as in torch
        assert float(ws[0].detach()) == 0 and bool((image[0] == 0).all()) and bool((weights[0] == 0).all())
        assert bool(torch.isnan(depth[0])) and torch.equal(torch.isnan(depth), torch.isnan(t32[1]))
        assert torch.allclose(ws[:1], t32[0][:1], equal_nan=True)
        assert torch.allclose(depth[:1], t32[1][:1], equal_nan=True)


@pytest.mark.parametrize("scale", ["soft", "hard"])
@pytest.mark.parametrize("T,t", SIZES)
def test_composite_backward(gpu, rays, T, t, scale):
    case = composite_case(gpu, rays, T, t, scale)
    ups = case["ups"]
    hit = rays["hit"].to(gpu)
    names = ["sigma_coarse"] + (["sigma_new"] if t > 0 else []) + ["rgbs"]
    # random upstream gradients on all three outputs: the rays that hit
    (ws, depth, image, _), leaves = native_composite(case, case["rgbs"])
    loss = ((ws * ups["ws"])[hit].sum() + (depth * ups["depth"])[hit].sum()
            + (image * ups["image"])[hit].sum())
    got = torch.autograd.grad(loss, leaves)
    for n, g, g32, g64 in zip(names, got, case["torch32"][1]["all"], case["exact"][1]["all"]):
        assert torch.isfinite(g[1:]).all(), n
        check_rule(f"{scale} {T}+{t} all outputs, {n}", g[1:], g32[1:], g64[1:])
    # image and weights_sum only, every ray: depth's NaN stays out
    (ws, depth, image, _), leaves = native_composite(case, case["rgbs"])
    loss = (ws * ups["ws"]).sum() + (image * ups["image"]).sum()
    got = torch.autograd.grad(loss, leaves)
    for n, g, g32, g64 in zip(names, got, case["torch32"][1]["no_depth"],
                              case["exact"][1]["no_depth"]):
        assert torch.isfinite(g).all(), n
        assert bool((g[0] == 0).all()), n  # the ray that misses
        check_rule(f"{scale} {T}+{t} image + weights_sum, {n}", g, g32, g64)
    # f16 colours: the gradient comes back in f16
    (ws, depth, image, _), leaves = native_composite(case, case["rgbs"].half())
    got = torch.autograd.grad((image * ups["image"]).sum() + (ws * ups["ws"]).sum(), leaves)
    assert got[-1].dtype == torch.float16 and got[0].dtype == torch.float32
    exact = case["exact_h"][1]["no_depth"]
    for n, g, g64 in zip(names, got, exact):
        assert torch.isfinite(g).all(), n
    # against the f64 truth on the same f16 colours: f16 rounding of the result
    assert rel_err(got[-1], exact[-1]) < 2.0 ** -10


# --------------------------------------------------------------- run() paths
def _models(gpu, seed=0, emb_scale=0.5):
    """The grid field in f32 with the CPU oracle holding the same weights
    (as tests/test_gpu_run.py)."""
    import main
    import oracle.cpu_render as cr
    from nerf.network_grid import NeRFNetwork
    opt = main.parse_opt(["--text", "a hamburger", "--h", "32", "--w", "32"])
    assert not opt.cuda_ray and not opt.fp16
    torch.manual_seed(seed)
    net = NeRFNetwork(opt).to(gpu)
    with torch.no_grad():
        net.encoder.embeddings.uniform_(-emb_scale, emb_scale)
    ref = cr.CPUNeRF(bound=opt.bound, min_near=opt.min_near)
    with torch.no_grad():
        ref.encoder.embeddings.copy_(net.encoder.embeddings.cpu())
        for dst, src in ((ref.sigma_net, net.sigma_net.net), (ref.bg_net, net.bg_net.net)):
            lins = [m for m in dst if isinstance(m, torch.nn.Linear)]
            for a, b in zip(lins, src):
                a.weight.copy_(b.weight.cpu())
                a.bias.copy_(b.bias.cpu())
        ref.aabb = net.aabb_infer.detach().cpu().clone()
    return opt, net, ref


@pytest.fixture(scope="module")
def grid_models(gpu):
    from nerf.provider import NeRFDataset
    opt, net, ref = _models(gpu)
    data = NeRFDataset(opt, device=gpu, type="test", H=24, W=24, size=8).collate([2])
    with torch.no_grad():
        img_ref, ws_ref = ref.run(data["rays_o"][0].cpu(), data["rays_d"][0].cpu(), opt.num_steps,
                                  opt.upsample_steps, perturb=False, det=True)
    return opt, net, data, img_ref, ws_ref


@pytest.mark.parametrize("native", [True, False])
def test_run_eval_matches_cpu_oracle(gpu, grid_models, native):
    opt, net, data, img_ref, ws_ref = grid_models
    net.eval()
    net.native_run = native
    before = (net.native_run_calls, net.torch_run_calls)
    light = torch.tensor([0.0, 0.0, 1.0], device=gpu)
    with torch.no_grad():
        out = net.render(data["rays_o"], data["rays_d"], staged=False, perturb=False,
                         light_d=light, ambient_ratio=1.0, shading="albedo", bg_color=None,
                         num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
    after = (net.native_run_calls, net.torch_run_calls)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if native else (0, 1))
    img = out["image"].reshape(-1, 3).cpu()
    ws = out["weights_sum"].reshape(-1).cpu()
    assert torch.isfinite(img).all() and float(ws.max()) > 0.05
    np.testing.assert_allclose(ws.numpy(), ws_ref.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(img.numpy(), img_ref.numpy(), rtol=1e-4, atol=2e-5)


def test_run_train_draws_the_same_samples_on_both_paths(gpu, grid_models):
    opt, net, data, _, _ = grid_models
    net.train()
    seen, states = {}, {}
    try:
        for native in (True, False):
            net.native_run = native
            net.zero_grad(set_to_none=True)
            first = []
            orig = net.density

            def recording(x, orig=orig, first=first):
                if not first:
                    first.append(x.detach().clone())
                return orig(x)
            net.density = recording
            torch.manual_seed(21)
            try:
                out = net.render(data["rays_o"], data["rays_d"], staged=False, perturb=True,
                                 ambient_ratio=0.1, shading="lambertian", bg_color=None,
                                 num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
            finally:
                del net.density
            states[native] = torch.cuda.get_rng_state(gpu).clone()
            seen[native] = first[0]
            assert torch.isfinite(out["image"]).all()
            loss = out["image"].sum() + out["weights_sum"].sum() + out["loss_orient"]
            loss.backward()
            grads = [p.grad for p in net.parameters() if p.grad is not None]
            assert grads and all(torch.isfinite(g).all() for g in grads)
            assert float(net.encoder.embeddings.grad.abs().sum()) > 0
    finally:
        net.native_run = True
        net.eval()
    assert seen[True].shape == (24 * 24 * opt.num_steps, 3)
    assert torch.equal(seen[True], seen[False])
    assert torch.equal(states[True], states[False])


def make_o2_trainer(gpu, extra=()):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", "-O2", "--num_steps", "16", "--upsample_steps", "16",
                          "--backbone", "vanilla", "--h", "16", "--w", "16", "--guidance",
                          "synthetic", "--seed", "3", *extra])
    seed_everything(3)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=None, optimizer=optimizer, ema_decay=None, fp16=True,
                      use_checkpoint="scratch", mute=True)
    return trainer, NeRFDataset


def test_o2_vanilla_train_step(gpu):
    trainer, NeRFDataset = make_o2_trainer(gpu)
    model = trainer.model
    assert not model.cuda_ray and model.native_run
    model.train()
    data = NeRFDataset(trainer.opt, device=gpu, type="train", H=16, W=16, size=100)
    torch.manual_seed(1)
    with torch.autocast("cuda", dtype=torch.float16):
        pred_rgb, pred_ws, loss = trainer.train_step(data.collate([0]), "lambertian", 0.1)
    assert pred_rgb.shape == (1, 3, 16, 16) and torch.isfinite(pred_rgb).all()
    assert torch.isfinite(loss).all()
    trainer._pending_sds = None
    torch.autograd.backward([pred_rgb, loss], [torch.ones_like(pred_rgb) * 1e-3, None])
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert all(p.grad is not None for p in model.sigma_net.parameters())
    assert model.native_run_calls > 0 and model.torch_run_calls == 0
    assert model.native_calls > 0


def test_staged_test_step_with_a_short_last_chunk(gpu):
    trainer, NeRFDataset = make_o2_trainer(gpu, extra=("--max_ray_batch", "100"))
    model = trainer.model
    model.eval()
    ds = NeRFDataset(trainer.opt, device=gpu, type="test", H=16, W=16, size=4)
    for k, shading in enumerate(("albedo", "textureless", "lambertian", "normal")):
        batch = ds.collate([1])
        batch["shading"] = shading
        batch["ambient_ratio"] = 1.0 if shading == "albedo" else 0.1
        with torch.autocast("cuda", dtype=torch.float16):
            img, depth = trainer.test_step(batch)
        assert img.shape == (1, 16, 16, 3) and torch.isfinite(img).all(), shading
        assert depth.shape == (1, 16, 16) and torch.isfinite(depth).all(), shading
        # 256 rays in chunks of 100, 100 and 56
        assert model.native_run_calls == 3 * (k + 1) and model.torch_run_calls == 0
