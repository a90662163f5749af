"""GPU tests of the DVGO voxel backbone (nerf/network_dvgo.py) and its fused
native field (csrc/voxelfield.hip, nerf/voxel_field.py).

Set-up of every parity test, as in tests/test_gpu_vanilla.py: truth `r` is the
float64 restatement of tests/voxel_cases.py; stick `t` is the module's own
torch path under fp16 autocast (fused_field = False); candidate `y` is the
native path, whose call counters prove it ran.  Each check prints a `parity:`
line.

f16-rounded quantities (albedo, shaded colours, the six parameter gradients):
the native error may not exceed twice the stick's error on the same inputs;
both round at the same f16 points.  Per-row outputs use max |y - r| /
(|r| + mean |r|), a parameter gradient |g - r|_2 / |r|_2.

f32-only quantities (sigma, -d sigma / d x): the stick's error is a few ulp,
so a pure 2x rule would test summation order.  Per row and component,
    |y - r| <= max(2 |t - r|, w),
with w the propagated float32 window of tests/voxel_cases.py (its docstring
derives it: roundings on the path x 2^-24 x the magnitudes they act on, that
is sum |weight x value| over the eight corners plus the rounding of the mapped
coordinate x the local corner-value differences, passed through the
10-Lipschitz activation and, for the normal, the chain factors).  The stick
itself must lie inside w in the same test.  For unit normals the window of a
row is 2 |w_n|_2 / |n|_2 + 8 x 2^-24 (normalising a vector n known to |w_n|).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import voxel_cases as vc

pytestmark = pytest.mark.gpu

import _voxelfield  # noqa: E402

R, W = _voxelfield.ROW_TILE, _voxelfield.WORKGROUP_ROWS
SIZES = [1, R - 1, R, R + 1, 2 * W + 1, 1000]
CKPTS = {"small": dict(world=vc.WORLD_SMALL), "large": dict(world=vc.WORLD_LARGE),
         "padded": dict(world=vc.WORLD_SMALL, C=4, posbase=0),  # dim0 = 31: padded K
         "deep": dict(world=vc.WORLD_SMALL, depth=4)}            # not served natively


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def nets(gpu, tmp_path_factory):
    import main
    tmp = tmp_path_factory.mktemp("dvgo")
    out = {}
    for name, kw in CKPTS.items():
        sd, dim0 = vc.make_state(seed=len(out), **kw)
        path = vc.save_checkpoint(tmp / f"{name}.dvgo", sd)
        opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
        out[name] = (main.network_class(opt)(opt).to(gpu), sd, path)
    assert out["small"][0].main_net.dim0 == 72 and out["padded"][0].main_net.dim0 == 31
    return out


_TRUTH = {}


def truth(nets, ckpt, M, seed=0):
    """The float64 reference of one case, computed once and shared."""
    key = (ckpt, M, seed)
    if key not in _TRUTH:
        sd = nets[ckpt][1]
        x = vc.positions(M, tuple(sd["density"].shape[2:]), seed)
        rs, ra, ps, aux = vc.truth(sd, x)
        rn = vc.normal_of(rs, aux)
        w_sigma, w_n = vc.windows(rs, aux)
        _TRUTH[key] = dict(x=x, sigma=rs.detach(), albedo=ra, ps=ps, aux=aux, normal=rn,
                           w_sigma=w_sigma, w_n=w_n)
    return _TRUTH[key]


def row_err(y, r):
    y, r = y.detach().double().cpu(), r.detach().double().cpu()
    return float(((y - r).abs() / (r.abs() + r.abs().mean())).max()) if r.numel() else 0.0


def norm_err(g, r):
    g, r = g.detach().double().cpu(), r.detach().double().cpu()
    if float(r.norm()) == 0.0:
        return float(g.norm())
    return float((g - r).norm() / r.norm())


def run_path(net, fused, fn):
    """fn() under fp16 autocast on the native (fused) or the torch path; the
    counters prove which one ran."""
    net.fused_field = fused
    before = (net.native_calls + net.native_normal_calls, net.torch_calls)
    with torch.autocast("cuda", dtype=torch.float16):
        out = fn()
    after = (net.native_calls + net.native_normal_calls, net.torch_calls)
    if fused:
        assert after[0] > before[0] and after[1] == before[1], "the native path did not run"
    else:
        assert after[0] == before[0] and after[1] > before[1], "the torch path did not run"
    net.fused_field = True
    return out


def check(name, y, t, r, err=row_err):
    """The 2x rule of the f16-rounded quantities."""
    ey, et = err(y, r), err(t, r)
    print(f"parity: {name}: native {ey:.3e} torch {et:.3e}")
    assert torch.isfinite(t).all() and torch.isfinite(y).all(), name
    assert ey <= 2 * et, (name, ey, et)


def check_window(name, y, t, r, w):
    """The rule of the f32-only quantities, per row and component."""
    y, t = y.detach().double().cpu(), t.detach().double().cpu()
    ey, et = (y - r).abs(), (t - r).abs()
    rel = lambda e: float((e / w.clamp(min=1e-300)).max()) if e.numel() else 0.0  # noqa: E731
    print(f"parity: {name}: native {float(ey.max()) if ey.numel() else 0:.3e} "
          f"({rel(ey):.3f} w) torch {float(et.max()) if et.numel() else 0:.3e} ({rel(et):.3f} w)")
    assert (et <= w).all(), (name, "the stick leaves the window")
    assert (ey <= torch.maximum(2 * et, w)).all(), name


def unit_window(rn, w_n):
    return 2 * w_n.norm(dim=-1, keepdim=True) / rn.norm(dim=-1, keepdim=True).clamp(min=1e-300) \
        + 8 * vc.EPS


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("ckpt, M", [("small", m) for m in SIZES] + [("padded", R + 1),
                                                                   ("padded", 1000),
                                                                   ("large", 1000)])
def test_forward(gpu, nets, ckpt, M):
    net = nets[ckpt][0]
    ref = truth(nets, ckpt, M)
    x = ref["x"].to(gpu)
    with torch.no_grad():
        ys, ya = run_path(net, True, lambda: net.common_forward(x))
        ts, ta = run_path(net, False, lambda: net.common_forward(x))
    assert ys.dtype == torch.float32 and ya.dtype == torch.float16 and ya.shape == (M, 3)
    assert ts.dtype == torch.float32
    check_window(f"forward {ckpt} M={M} sigma", ys, ts, ref["sigma"], ref["w_sigma"])
    check(f"forward {ckpt} M={M} albedo", ya, ta, ref["albedo"])
    outside = ~ref["aux"]["inside"]
    assert torch.equal(ya.cpu()[outside], torch.full((int(outside.sum()), 3), 0.5).half())
    if M == 1000:
        assert 0.3 < float(outside.float().mean()) < 0.7


def test_forward_all_outside_and_empty(gpu, nets):
    net = nets["small"][0]
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2 * W + 1, 3, generator=g) * 0.15 + 0.84).to(gpu)  # beyond 0.8 of the bound
    assert not vc.restate32(x.cpu().numpy(), vc.WORLD_SMALL)["inside"].any()
    want = 10 * F.softplus(torch.tensor(vc.act_shift(), dtype=torch.float64))
    for fused in (True, False):
        with torch.no_grad():
            s, a = run_path(net, fused, lambda: net.common_forward(x))
            n = run_path(net, fused, lambda: net.normal(x.clone()))
        assert torch.equal(a.float(), torch.full_like(a.float(), 0.5))
        assert torch.equal(n, torch.zeros_like(n))
        assert float((s.double().cpu() - want).abs().max()) <= 8 * vc.EPS * float(want)
    empty = torch.zeros(0, 3, device=gpu)
    with torch.no_grad():
        s, a = run_path(net, True, lambda: net.common_forward(empty))
        n = run_path(net, True, lambda: net.normal(empty))
    assert s.shape == (0,) and a.shape == (0, 3) and n.shape == (0, 3)


def test_density_only_entry(gpu, nets):
    """albedo NULL: the density branch alone, the same bits as the fused launch."""
    net = nets["small"][0]
    x = truth(nets, "small", 2 * W + 1)["x"].to(gpu)
    with torch.no_grad():
        ys, _ = run_path(net, True, lambda: net.common_forward(x))
    vol, _ = _operands(net)
    sigma = torch.full_like(ys, float("nan"))
    _voxelfield.field_forward(x, vol, 1.0, net.main_net.act_shift, None, sigma)
    assert torch.equal(sigma, ys)


# ---------------------------------------------------------------- backward
def field_grads(net, x, ga, fused):
    net.zero_grad(set_to_none=True)

    def fn():
        sigma, albedo = net.common_forward(x)
        assert sigma.requires_grad is False  # frozen density, leaf positions
        albedo.backward(ga.to(albedo.dtype))
    run_path(net, fused, fn)
    m = net.main_net
    assert m.density.grad is None and m.k0.grad is None
    return [p.grad.detach().clone() for p in m.rgbnet.parameters()]


@pytest.mark.parametrize("ckpt, M", [("small", m) for m in SIZES] + [("padded", 2 * W + 1),
                                                                   ("large", 1000)])
def test_backward(gpu, nets, ckpt, M):
    net = nets[ckpt][0]
    ref = truth(nets, ckpt, M, seed=1)
    x = ref["x"].to(gpu)
    g = torch.Generator().manual_seed(7 + M)
    ga = torch.randn(M, 3, generator=g)
    y = field_grads(net, x, ga.to(gpu), True)
    t = field_grads(net, x, ga.to(gpu), False)
    # the stick's albedo gradient arrives rounded to f16; the truth takes it exact
    rg = torch.autograd.grad(ref["albedo"], ref["ps"], ga.double(), retain_graph=True)
    names = [n for n, _ in net.main_net.rgbnet.named_parameters()]
    assert len(names) == 6
    for n, gy, gt, r in zip(names, y, t, rg):
        assert gy.dtype == torch.float32 and gy.shape == r.shape
        check(f"backward {ckpt} M={M} {n}", gy, gt, r, err=norm_err)


def _operands(net):
    from nerf import voxel_field as vf
    m = net.main_net
    return vf.volume(net)[0], [p.detach().contiguous() for p in m.rgbnet.parameters()]


def test_backward_accumulate_grad_dtypes_and_determinism(gpu, nets):
    """accumulate adds onto a preset gradient exactly (preset + overwrite run,
    one f32 add per element); grad_albedo is taken as f16 and as f32; two
    runs give the same bits."""
    net = nets["small"][0]
    M = 2 * W + 1
    x = vc.positions(M, vc.WORLD_SMALL, seed=2).to(gpu)
    vol, ws = _operands(net)
    g = torch.Generator().manual_seed(3)
    ga32 = torch.randn(M, 3, generator=g).to(gpu).half().float()  # f16-representable
    over = [torch.full_like(w, float("nan")) for w in ws]
    _voxelfield.field_backward(x, vol, 1.0, ws, ga32, over)
    assert all(torch.isfinite(o).all() for o in over)
    assert all(float(o.abs().sum()) > 0 for o in over)
    again = [torch.empty_like(w) for w in ws]
    _voxelfield.field_backward(x, vol, 1.0, ws, ga32, again)
    for a, o in zip(again, over):
        assert torch.equal(a, o)
    preset = [torch.randn(w.shape, generator=g).to(gpu) for w in ws]
    acc = [p.clone() for p in preset]
    _voxelfield.field_backward(x, vol, 1.0, ws, ga32, acc, accumulate=True)
    for a, p, o in zip(acc, preset, over):
        assert torch.equal(a, p + o)
    half = [torch.empty_like(w) for w in ws]
    _voxelfield.field_backward(x, vol, 1.0, ws, ga32.half(), half)
    for h, o in zip(half, over):
        assert torch.equal(h, o)
    # no rows: zeros, or the preset untouched
    none = [torch.full_like(w, float("nan")) for w in ws]
    _voxelfield.field_backward(x[:0], vol, 1.0, ws, ga32[:0], none)
    assert all(torch.equal(n, torch.zeros_like(n)) for n in none)


# ---------------------------------------------------------------- normal
@pytest.mark.parametrize("ckpt, M", [("small", m) for m in SIZES] + [("large", 1000)])
def test_normal(gpu, nets, ckpt, M):
    from nerf import voxel_field as vf
    net = nets[ckpt][0]
    ref = truth(nets, ckpt, M)
    x = ref["x"].to(gpu)
    yn = run_path(net, True, lambda: vf.input_gradient(net, x))

    def stick():
        xs = x.clone().requires_grad_(True)
        return -torch.autograd.grad(net.common_forward(xs)[0].sum(), xs)[0]
    tn = run_path(net, False, stick)
    check_window(f"normal {ckpt} M={M} raw", yn, tn, ref["normal"], ref["w_n"])
    outside = ~ref["aux"]["inside"]
    assert torch.equal(yn.cpu()[outside], torch.zeros(int(outside.sum()), 3))
    # unit normals, with and without grad: the native path serves both
    ru, wu = vc.unit(ref["normal"]), unit_window(ref["normal"], ref["w_n"])
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            yu = run_path(net, True, lambda: net.normal(x.clone()))
            tu = run_path(net, False, lambda: net.normal(x.clone()))
        assert yu.requires_grad is False
        check_window(f"normal {ckpt} M={M} unit grad={grad}", yu, tu, ru, wu)
        zero = (ref["normal"] == 0).all(-1)
        assert torch.equal(yu.cpu()[zero], torch.zeros(int(zero.sum()), 3))
        assert torch.isfinite(yu).all()


def test_flat_density_gives_exactly_zero_normals(gpu, tmp_path):
    import main
    sd, _ = vc.make_state(density=torch.full((1, 1, *vc.WORLD_SMALL), 1.5))
    path = vc.save_checkpoint(tmp_path / "flat.dvgo", sd)
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
    net = main.network_class(opt)(opt).to(gpu)
    x = vc.positions(R + 1 + 40, vc.WORLD_SMALL, seed=4).to(gpu)
    with torch.no_grad():
        n = run_path(net, True, lambda: net.normal(x.clone()))
    assert torch.equal(n, torch.zeros_like(n))


# ---------------------------------------------------------------- module
def test_dispatch(gpu, nets):
    net, deep = nets["small"][0], nets["deep"][0]
    x = vc.positions(100, vc.WORLD_SMALL, seed=6).to(gpu)

    def counts(n):
        return n.native_calls + n.native_normal_calls, n.torch_calls
    with torch.no_grad():
        c0 = counts(net)
        s, a = net.common_forward(x)  # no autocast
        assert counts(net) == (c0[0], c0[1] + 1) and a.dtype == torch.float32
        with torch.autocast("cuda", dtype=torch.bfloat16):
            s, a = net.common_forward(x)
        assert counts(net) == (c0[0], c0[1] + 2) and torch.isfinite(s).all()
        with torch.autocast("cuda", dtype=torch.float16):
            s, a = net.common_forward(x, torch.ones(100, device=gpu))  # a weight argument
            assert counts(net) == (c0[0], c0[1] + 3)
            s, a = net.common_forward(x)
            assert counts(net) == (c0[0] + 1, c0[1] + 3) and a.dtype == torch.float16
            # a depth-4 rgbnet is not the native shape
            c1 = counts(deep)
            s, a = deep.common_forward(x)
            n = deep.normal(x.clone())
            assert counts(deep) == (c1[0], c1[1] + 2)
            assert torch.isfinite(s).all() and torch.isfinite(a).all() and torch.isfinite(n).all()


@pytest.mark.parametrize("shading", ["albedo", "textureless", "lambertian", "normal"])
def test_shadings(gpu, nets, shading):
    net = nets["small"][0]
    M = 1000
    ref = truth(nets, "small", M)
    x = ref["x"].to(gpu)
    d = F.normalize(vc.positions(M, vc.WORLD_SMALL, seed=8, edges=False) + 0.01, dim=-1).to(gpu)
    light = F.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
    out = {}
    for fused in (True, False):
        with torch.no_grad():
            out[fused] = run_path(net, fused, lambda: net(x.clone(), d, light.to(gpu), ratio=0.1,
                                                          shading=shading))
    rn = vc.unit(ref["normal"])
    lam = 0.1 + 0.9 * (rn @ light.double()).clamp(min=0)
    ra = ref["albedo"].detach()
    rc = {"albedo": ra, "textureless": lam[:, None].repeat(1, 3), "normal": (rn + 1) / 2,
          "lambertian": ra * lam[:, None]}[shading]
    (ys, yc, yn), (ts, tc, tn) = out[True], out[False]
    check_window(f"{shading} sigma", ys, ts, ref["sigma"], ref["w_sigma"])
    if shading == "normal":  # an f32-only colour
        check_window(f"{shading} colour", yc, tc, rc, unit_window(ref["normal"], ref["w_n"]) / 2)
    else:
        check(f"{shading} colour", yc, tc, rc)
    if shading == "albedo":
        assert yn is None and tn is None
    else:
        check_window(f"{shading} normal", yn, tn, rn, unit_window(ref["normal"], ref["w_n"]))


# ---------------------------------------------------------------- trainer
def make_trainer(gpu, nets, seed, args=("-O",), tmp=None):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", *args, "--backbone", "dvgo", "--dvgo_ckpt",
                          nets["small"][2], "--h", "16", "--w", "16", "--guidance", "synthetic",
                          "--seed", str(seed)])
    seed_everything(seed)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=tmp, optimizer=optimizer, ema_decay=None, fp16=True,
                      use_checkpoint="scratch", mute=True)
    data = NeRFDataset(opt, device=gpu, type="train", H=16, W=16, size=100)
    trainer.model.train()
    return trainer, data


@pytest.fixture(scope="module")
def trainer_state(gpu, nets):
    trainer, _ = make_trainer(gpu, nets, 3)
    torch.manual_seed(4)
    with torch.autocast("cuda", dtype=torch.float16):
        trainer.model.update_extra_state()
    assert int(trainer.model.density_bitfield.count_nonzero()) > 0
    return copy.deepcopy(trainer.model.state_dict())


@pytest.mark.parametrize("shading", ["albedo", "lambertian"])
def test_train_step(gpu, nets, trainer_state, shading):
    """One 16 x 16 -O step: the native field (and, shaded, the native normal)
    ran and the torch path did not; only rgbnet and bg_net change; the volumes
    stay bit-identical."""
    trainer, data = make_trainer(gpu, nets, 3)
    model = trainer.model
    model.load_state_dict(trainer_state)
    before = copy.deepcopy(model.state_dict())
    torch.manual_seed(11)
    trainer.opt.light_d = F.normalize(torch.tensor([0.2, 0.9, 0.4], device=gpu), dim=0)
    trainer.optimizer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        pred_rgb, pred_ws, loss = trainer.train_step(data.collate([0]), shading,
                                                     1.0 if shading == "albedo" else 0.1)
    assert pred_rgb.shape == (1, 3, 16, 16) and torch.isfinite(pred_rgb).all()
    trainer.backward_only(loss)
    assert model.native_calls > 0 and model.torch_calls == 0
    assert (model.native_normal_calls > 0) == (shading != "albedo")
    m = model.main_net
    assert m.density.grad is None and m.k0.grad is None
    for p in list(m.rgbnet.parameters()) + list(model.bg_net.parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    trainer.optimizer_step()
    after = model.state_dict()
    trained = ("main_net.rgbnet.", "bg_net.")
    for k in before:
        if k.startswith(trained):
            assert not torch.equal(after[k], before[k]), k
        elif k.startswith("main_net."):
            assert torch.equal(after[k], before[k]), k
    assert torch.equal(after["main_net.density"], trainer_state["main_net.density"])
    assert torch.equal(after["main_net.k0"], trainer_state["main_net.k0"])


def test_o2_step_and_test_view(gpu, nets, trainer_state):
    """One -O2 (no cuda_ray) step with gradients and one lambertian test view
    at 16 x 16: finite images of the right shape, from the native field."""
    trainer, data = make_trainer(gpu, nets, 3, args=("-O2", "--num_steps", "16",
                                                     "--upsample_steps", "16"))
    assert not trainer.model.cuda_ray
    torch.manual_seed(1)
    with torch.autocast("cuda", dtype=torch.float16):
        pred_rgb, pred_ws, loss = trainer.train_step(data.collate([0]), "lambertian", 0.1)
    assert pred_rgb.shape == (1, 3, 16, 16) and torch.isfinite(pred_rgb).all()
    trainer.backward_only(loss)
    assert all(torch.isfinite(p.grad).all() for p in trainer.model.main_net.rgbnet.parameters())
    assert trainer.model.native_calls > 0 and trainer.model.torch_calls == 0

    from nerf.provider import NeRFDataset
    trainer, _ = make_trainer(gpu, nets, 3)
    trainer.model.load_state_dict(trainer_state)
    trainer.model.eval()
    ds = NeRFDataset(trainer.opt, device=gpu, type="test", H=16, W=16, size=4)
    batch = ds.collate([1])
    batch["shading"], batch["ambient_ratio"] = "lambertian", 0.1
    with torch.autocast("cuda", dtype=torch.float16):  # as the Trainer's test loop does
        img, depth = trainer.test_step(batch)
    assert img.shape == (1, 16, 16, 3) and torch.isfinite(img).all()
    assert depth.shape == (1, 16, 16) and torch.isfinite(depth).all()
    assert trainer.model.native_calls > 0 and trainer.model.native_normal_calls > 0


def test_checkpoint_round_trip(gpu, nets, trainer_state, tmp_path):
    trainer, _ = make_trainer(gpu, nets, 3, tmp=str(tmp_path))
    trainer.model.load_state_dict(trainer_state)
    with torch.no_grad():  # other weights and volumes than the file the models start from
        for p in trainer.model.main_net.parameters():
            p.add_(0.01)
    trainer.ckpt_path = str(tmp_path)
    trainer.save_checkpoint("ck", full=True)
    fresh, _ = make_trainer(gpu, nets, 4, tmp=str(tmp_path))
    x = vc.positions(50, vc.WORLD_SMALL).to(gpu)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fresh.model.common_forward(x)  # the native operands exist before the load replaces k0
    fresh.ckpt_path = str(tmp_path)
    fresh.load_checkpoint(str(tmp_path / "ck.pth"))
    want, got = trainer.model.state_dict(), fresh.model.state_dict()
    assert want.keys() == got.keys()
    assert "main_net.rgbnet.net.2.0.weight" in want and "main_net.k0" in want
    for k in want:
        assert torch.equal(want[k], got[k]), k
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a, b = trainer.model.common_forward(x), fresh.model.common_forward(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
