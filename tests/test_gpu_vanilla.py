"""GPU tests of the vanilla backbone (nerf/network.py) and its fused native
field (csrc/resmlp.hip, nerf/vanilla_field.py).

Set-up of every parity test: truth `r` is a float64 restatement of the field
in plain torch (`truth_field` below, gradients by autograd in f64); stick `t`
is the module's own torch path under fp16 autocast (fused_field = False);
candidate `y` is the native path, whose call counters prove it ran.

Criterion: for per-row outputs (sigma, albedo, dx) the error is
max |y - r| / (|r| + mean |r|); for a parameter gradient it is
|g - r|_2 / |r|_2.  The native error may not exceed twice the stick's error on
the same inputs: both round at the same f16 points and differ in f32 summation
order only.  Each test prints `parity:` lines with both errors.

sigma_net has 19 parameter tensors (5 in block 0, 4 in blocks 1..3, 2 in the
output layer); every one of them is checked.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _resmlp  # noqa: E402

R, W = _resmlp.ROW_TILE, _resmlp.WORKGROUP_ROWS
SIZES = [1, R - 1, R, R + 1, 2 * W + 1, 1000]


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
    return net


def positions(gpu, M, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.rand(M, 3, generator=g) * 2 - 1
    x[0] = 0.0
    if M > 2:
        x[1] = 1.0
        x[2] = -1.0
    return x.to(gpu)


def truth_field(net, x):
    """The field in float64: sigma [M], albedo [M, 3] of x [M, 3] (f64, may
    require grad), and the f64 copies of sigma_net's parameters in order."""
    ps = [p.detach().double().requires_grad_(True) for p in net.sigma_net.parameters()]
    feats = [x]
    for k in range(6):
        feats += [torch.sin(2.0 ** k * x), torch.cos(2.0 ** k * x)]
    h = torch.cat(feats, -1)
    i = 0
    for l in range(4):
        w, b, gamma, beta = ps[i:i + 4]
        i += 4
        idn = h
        if l == 0:
            idn = h @ ps[i].T
            i += 1
        h = F.silu(F.layer_norm(h @ w.T + b, (128,), gamma, beta, 1e-5) + idn)
    o = h @ ps[i].T + ps[i + 1]
    sigma = torch.exp(o[:, 0] + 5 * torch.exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2)))
    return sigma, torch.sigmoid(o[:, 1:]), ps


def row_err(y, r):
    y, r = y.detach().double(), r.detach().double()
    return float(((y - r).abs() / (r.abs() + r.abs().mean())).max()) if r.numel() else 0.0


def norm_err(g, r):
    g, r = g.detach().double(), r.detach().double()
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
    ey, et = err(y, r), err(t, r)
    print(f"parity: {name}: native {ey:.3e} torch {et:.3e}")
    assert torch.isfinite(t).all(), name
    assert ey <= 2 * et, (name, ey, et)
    return ey, et


def field_grads(net, x, gs, ga, fused):
    net.zero_grad(set_to_none=True)

    def fn():
        sigma, albedo = net.common_forward(x)
        torch.autograd.backward([sigma, albedo], [gs, ga.to(albedo.dtype)])
    run_path(net, fused, fn)
    return [p.grad.detach().clone() for p in net.sigma_net.parameters()]


# ---------------------------------------------------------------- kernels
@pytest.fixture(scope="module")
def net(gpu):
    return make_net(gpu)


@pytest.mark.parametrize("M", SIZES)
def test_forward(gpu, net, M):
    x = positions(gpu, M)
    with torch.no_grad():
        ys, ya = run_path(net, True, lambda: net.common_forward(x))
        ts, ta = run_path(net, False, lambda: net.common_forward(x))
        rs, ra, _ = truth_field(net, x.double())
    assert ys.dtype == torch.float32 and ya.dtype == torch.float16
    assert ts.dtype == torch.float32 and ta.dtype == torch.float16
    assert float(rs.max()) < 1100.0  # sigma < e^7: no f16 gradient of the stick overflows
    check(f"forward M={M} sigma", ys, ts, rs)
    check(f"forward M={M} albedo", ya, ta, ra)


def test_forward_empty(gpu, net):
    x = torch.zeros(0, 3, device=gpu)
    with torch.no_grad():
        s, a = run_path(net, True, lambda: net.common_forward(x))
        n = run_path(net, True, lambda: net.normal(x))
    assert s.shape == (0,) and a.shape == (0, 3) and n.shape == (0, 3)


@pytest.mark.parametrize("M", SIZES)
def test_backward(gpu, net, M):
    x = positions(gpu, M, seed=1)
    g = torch.Generator().manual_seed(7 + M)
    gs = (torch.randn(M, generator=g) * 1e-2).to(gpu)
    ga = torch.randn(M, 3, generator=g).to(gpu)
    y = field_grads(net, x, gs, ga, True)
    t = field_grads(net, x, gs, ga, False)
    rs, ra, ps = truth_field(net, x.double())
    # the stick's albedo gradient arrives rounded to f16; the truth takes it exact
    torch.autograd.backward([rs, ra], [gs.double(), ga.double()])
    names = [n for n, _ in net.sigma_net.named_parameters()]
    assert len(names) == 19
    for n, gy, gt, p in zip(names, y, t, ps):
        assert gy.dtype == torch.float32 and gy.shape == p.shape
        check(f"backward M={M} {n}", gy, gt, p.grad, err=norm_err)


def test_backward_accumulate_and_grad_dtypes(gpu, net):
    """accumulate adds onto a preset gradient exactly (preset + overwrite run,
    one f32 add per element); grad_albedo is taken as f16 and as f32."""
    M = 2 * W + 1
    x = positions(gpu, M, seed=2)
    ws = [p.detach().contiguous() for p in net.sigma_net.parameters()]
    g = torch.Generator().manual_seed(3)
    gs = (torch.randn(M, generator=g) * 1e-2).to(gpu)
    ga32 = torch.randn(M, 3, generator=g).to(gpu).half().float()  # f16-representable
    over = [torch.full_like(w, float("nan")) for w in ws]
    _resmlp.field_backward(x, ws, gs, ga32, grads=over)
    assert all(torch.isfinite(o).all() for o in over)
    preset = [torch.randn(w.shape, generator=g).to(gpu) for w in ws]
    acc = [p.clone() for p in preset]
    _resmlp.field_backward(x, ws, gs, ga32, grads=acc, accumulate=True)
    for a, p, o in zip(acc, preset, over):
        assert torch.equal(a, p + o)
    half = [torch.empty_like(w) for w in ws]
    _resmlp.field_backward(x, ws, gs, ga32.half(), grads=half)
    for h, o in zip(half, over):
        assert torch.equal(h, o)
    # parameter gradients and dx in one call equal the separate calls
    both, dx = [torch.empty_like(w) for w in ws], torch.empty(M, 3, device=gpu)
    _resmlp.field_backward(x, ws, gs, ga32, dx=dx, grads=both)
    only = torch.empty(M, 3, device=gpu)
    _resmlp.field_backward(x, ws, gs, ga32, dx=only)
    assert torch.equal(dx, only)
    # (the LayerNorm sums are taken per wave, and this form runs 4 waves per
    # workgroup instead of 8: f32 summation order differs)
    for b, o in zip(both, over):
        torch.testing.assert_close(b, o, rtol=1e-4, atol=1e-6 * float(o.abs().max()))


@pytest.mark.parametrize("M", SIZES)
def test_input_gradient_and_normal(gpu, net, M):
    from nerf import vanilla_field as vf
    x = positions(gpu, M, seed=3)
    ydx = run_path(net, True, lambda: vf.input_gradient(net, x))
    x64 = x.double().requires_grad_(True)
    rs, _, _ = truth_field(net, x64)
    rdx = torch.autograd.grad(rs.sum(), x64)[0]

    def stick_dx():
        xs = x.clone().requires_grad_(True)
        sigma, _ = net.common_forward(xs)
        return torch.autograd.grad(sigma.sum(), xs)[0]
    tdx = run_path(net, False, stick_dx)
    check(f"dx M={M}", ydx, tdx, rdx)
    with torch.no_grad():
        yn = run_path(net, True, lambda: net.normal(x.clone()))
        tn = run_path(net, False, lambda: net.normal(x.clone()))
    assert yn.requires_grad is False and tn.requires_grad is False
    rn = -rdx / torch.sqrt(torch.clamp((rdx * rdx).sum(-1, keepdim=True), min=1e-20))
    check(f"normal M={M}", yn, tn, rn)


def test_grad_enabled_normal_carries_a_graph(gpu, net):
    """The pin of the dispatch: with grad enabled the autograd normal of the
    torch path requires grad (sigma enters its own input gradient through the
    Gaussian blob and trunc_exp's backward), so the module serves grad-enabled
    normals and shaded steps from the torch path and the native, graph-free
    input gradient serves no-grad calls only."""
    x = positions(gpu, R + 1, seed=9)
    tn = run_path(net, False, lambda: net.normal(x.clone()))
    assert tn.requires_grad is True
    # fused_field on, grad on: still the torch path, the same bits
    before = (net.native_normal_calls, net.torch_calls)
    with torch.autocast("cuda", dtype=torch.float16):
        yn = net.normal(x.clone())
    assert (net.native_normal_calls, net.torch_calls) == (before[0], before[1] + 1)
    assert yn.requires_grad is True and torch.equal(yn, tn)
    light = torch.tensor([0.0, 0.0, 1.0], device=gpu)
    with torch.autocast("cuda", dtype=torch.float16):
        sigma, color, normal = net(x.clone(), x, light, ratio=0.1, shading="lambertian")
    assert normal.requires_grad and net.native_normal_calls == before[0]


def test_zero_input_gradient_row(gpu):
    """A row whose input gradient is exactly zero: x = 0 (the Gaussian's
    gradient vanishes) with the density output's weights zeroed.  Its normal is
    0 on both paths.  safe_normalize divides by sqrt(clamp(|n|^2, 1e-20)), so a
    zero gradient gives 0, not NaN: the NaN -> 0 rule only ever acts on
    non-finite gradients, which these inputs cannot produce."""
    net = make_net(gpu, seed=5)
    with torch.no_grad():
        net.sigma_net.net[4].weight[0].zero_()
    x = positions(gpu, R + 1, seed=4)
    from nerf import vanilla_field as vf
    dx = run_path(net, True, lambda: vf.input_gradient(net, x))
    assert torch.equal(dx[0], torch.zeros(3, device=gpu))
    for fused in (True, False):
        with torch.no_grad():
            n = run_path(net, fused, lambda: net.normal(x.clone()))
        assert torch.equal(n[0], torch.zeros(3, device=gpu))
        assert torch.isfinite(n).all()


def test_determinism(gpu, net):
    M = 2 * W + 1
    x = positions(gpu, M, seed=5)
    ws = [p.detach().contiguous() for p in net.sigma_net.parameters()]
    g = torch.Generator().manual_seed(9)
    gs = (torch.randn(M, generator=g) * 1e-2).to(gpu)
    ga = torch.randn(M, 3, generator=g).to(gpu).half()
    runs = []
    for _ in range(2):
        grads, dx = [torch.empty_like(w) for w in ws], torch.empty(M, 3, device=gpu)
        _resmlp.field_backward(x, ws, gs, ga, dx=dx, grads=grads)
        runs.append(grads + [dx])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_dispatch(gpu, net):
    x = positions(gpu, 100, seed=6)

    def counts():
        return net.native_calls, net.torch_calls
    with torch.no_grad():
        c0 = counts()
        s, a = net.common_forward(x)  # no autocast
        assert counts() == (c0[0], c0[1] + 1) and torch.isfinite(s).all()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            s, a = net.common_forward(x)
        assert counts() == (c0[0], c0[1] + 2) and torch.isfinite(s).all()
        assert torch.isfinite(a.float()).all()
        s, a = run_path(net, False, lambda: net.common_forward(x))
        assert torch.isfinite(s).all() and torch.isfinite(a.float()).all()
        c1 = counts()
        with torch.autocast("cuda", dtype=torch.float16):
            s, a = net.common_forward(x)
        assert counts() == (c1[0] + 1, c1[1]) and torch.isfinite(s).all()
        narrow = make_net(gpu, seed=2, hidden_dim=64)
        with torch.autocast("cuda", dtype=torch.float16):
            s, a = narrow.common_forward(x)
        assert (narrow.native_calls, narrow.torch_calls) == (0, 1)
        assert torch.isfinite(s).all() and torch.isfinite(a.float()).all()


@pytest.mark.parametrize("shading", ["albedo", "textureless", "lambertian", "normal"])
def test_shadings(gpu, net, shading):
    M = 1000
    x = positions(gpu, M, seed=7)
    d = F.normalize(positions(gpu, M, seed=8) + 0.01, dim=-1)
    light = F.normalize(torch.tensor([0.3, 0.5, 0.8], device=gpu), dim=0)
    out = {}
    for fused in (True, False):
        with torch.no_grad():  # an eval frame: the native normal serves no-grad calls
            out[fused] = run_path(net, fused, lambda: net(x.clone(), d, light, ratio=0.1,
                                                          shading=shading))
    x64 = x.double().requires_grad_(True)
    rs, ra, _ = truth_field(net, x64)
    rdx = torch.autograd.grad(rs.sum(), x64)[0]
    rn = -rdx / torch.sqrt(torch.clamp((rdx * rdx).sum(-1, keepdim=True), min=1e-20))
    lam = 0.1 + 0.9 * (rn @ light.double()).clamp(min=0)
    rc = {"albedo": ra, "textureless": lam[:, None].repeat(1, 3), "normal": (rn + 1) / 2,
          "lambertian": ra * lam[:, None]}[shading]
    (ys, yc, yn), (ts, tc, tn) = out[True], out[False]
    check(f"{shading} sigma", ys, ts, rs)
    check(f"{shading} colour", yc, tc, rc)
    if shading == "albedo":
        assert yn is None and tn is None
    else:
        check(f"{shading} normal", yn, tn, rn)


# ---------------------------------------------------------------- trainer
def make_trainer(gpu, seed, args=("-O",), tmp=None):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", *args, "--backbone", "vanilla", "--h", "16", "--w", "16",
                          "--guidance", "synthetic", "--seed", str(seed)])
    seed_everything(seed)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=tmp, optimizer=optimizer, ema_decay=None, fp16=True,
                      use_checkpoint="scratch", mute=True)
    data = NeRFDataset(opt, device=gpu, type="train", H=16, W=16, size=100)
    trainer.model.train()
    return trainer, data


def _step(gpu, fused, shading, state):
    """One train_step + backward on a fresh trainer from `state` (shared model
    weights and density grid); records the field call's samples and incoming
    gradients."""
    trainer, data = make_trainer(gpu, 3)
    model = trainer.model
    model.load_state_dict(state)
    model.fused_field = fused
    rec = []
    orig = model.common_forward

    def recording(x, *args, **kw):
        s, a = orig(x, *args, **kw)
        if s.requires_grad and not rec:
            r = {"x": x.detach().clone(), "ga": torch.zeros(x.shape[0], 3, device=gpu)}
            s.register_hook(lambda g: r.__setitem__("gs", g.detach().clone()))
            a.register_hook(lambda g: r.__setitem__("ga", g.detach().float().clone()))
            rec.append(r)
        return s, a
    model.common_forward = recording
    torch.manual_seed(11)
    batch = data.collate([0])
    model.march_noises = torch.rand(256, device=gpu, generator=torch.Generator(gpu).manual_seed(5))
    trainer.opt.light_d = F.normalize(torch.tensor([0.2, 0.9, 0.4], device=gpu), dim=0)
    trainer.optimizer.zero_grad(set_to_none=True)
    torch.manual_seed(12)
    with torch.autocast("cuda", dtype=torch.float16):
        pred_rgb, pred_ws, loss = trainer.train_step(batch, shading, 1.0 if shading == "albedo"
                                                     else 0.1)
    g = torch.randn(pred_rgb.shape, device=gpu, generator=torch.Generator(gpu).manual_seed(1))
    trainer._pending_sds = None
    torch.autograd.backward([pred_rgb, loss], [g * 1e-2, None])
    del model.common_forward
    calls = (model.native_calls, model.torch_calls)
    if fused and shading == "albedo":
        assert calls[0] > 0 and calls[1] == 0
    else:  # shaded steps carry a graph through the normal: the torch path
        assert calls[0] == 0 and calls[1] > 0
    assert torch.isfinite(loss).all() and torch.isfinite(pred_rgb).all()
    grads = [p.grad.detach().clone() for p in model.sigma_net.parameters()]
    before = [p.detach().clone() for p in model.sigma_net.parameters()]
    trainer.optimizer.step()
    for p, b in zip(model.sigma_net.parameters(), before):
        assert torch.isfinite(p).all() and not torch.equal(p, b)
    model.load_state_dict(state)  # the truth below reads the step's own weights
    return model, rec[0], grads


@pytest.fixture(scope="module")
def trainer_state(gpu):
    trainer, _ = make_trainer(gpu, 3)
    torch.manual_seed(4)
    with torch.autocast("cuda", dtype=torch.float16):
        trainer.model.update_extra_state()
    assert int(trainer.model.density_bitfield.count_nonzero()) > 0
    return copy.deepcopy(trainer.model.state_dict())


@pytest.mark.parametrize("shading", ["albedo", "lambertian"])
def test_train_step(gpu, trainer_state, shading):
    """One 16 x 16 train_step per path from the same state, seeds and march
    noises (the lambertian step runs the torch path under either setting: its
    normal carries a graph, whose share of the gradient the restatement below
    does not model, so there both errors are large and equal).  The f64 truth of the sigma_net gradients is the restatement on
    the step's own samples with the step's own incoming (sigma, albedo)
    gradients, recorded by hooks on each path's field call."""
    errs = {}
    xs = {}
    for fused in (True, False):
        model, rec, grads = _step(gpu, fused, shading, trainer_state)
        xs[fused] = rec["x"]
        rs, ra, ps = truth_field(model, rec["x"].double())
        torch.autograd.backward([rs, ra], [rec["gs"].double(), rec["ga"].double()])
        errs[fused] = [(norm_err(g, p.grad), torch.isfinite(g).all()) for g, p in zip(grads, ps)]
    assert torch.equal(xs[True], xs[False])  # the march is bit-identical
    assert xs[True].shape[0] > 0
    names = [n for n, _ in model.sigma_net.named_parameters()]
    for n, (ey, fy), (et, ft) in zip(names, errs[True], errs[False]):
        print(f"parity: train_step {shading} {n}: native {ey:.3e} torch {et:.3e}")
        assert fy and ft, n
        assert ey <= 2 * et, (n, ey, et)


def test_o2_step_and_test_views(gpu, trainer_state):
    """One -O2 (no cuda_ray) render with gradients and one test_step per
    shading at 16 x 16: finite images of the right shape."""
    trainer, data = make_trainer(gpu, 3, args=("-O2", "--num_steps", "16", "--upsample_steps",
                                               "16"))
    assert not trainer.model.cuda_ray
    torch.manual_seed(1)
    with torch.autocast("cuda", dtype=torch.float16):
        pred_rgb, pred_ws, loss = trainer.train_step(data.collate([0]), "lambertian", 0.1)
    assert pred_rgb.shape == (1, 3, 16, 16) and torch.isfinite(pred_rgb).all()
    assert torch.isfinite(loss).all()
    trainer._pending_sds = None
    torch.autograd.backward([pred_rgb, loss], [torch.ones_like(pred_rgb) * 1e-3, None])
    assert all(torch.isfinite(p.grad).all() for p in trainer.model.sigma_net.parameters())
    assert trainer.model.native_calls > 0

    from nerf.provider import NeRFDataset
    trainer, _ = make_trainer(gpu, 3)
    trainer.model.load_state_dict(trainer_state)
    trainer.model.eval()
    ds = NeRFDataset(trainer.opt, device=gpu, type="test", H=16, W=16, size=4)
    for shading in ("albedo", "textureless", "lambertian", "normal"):
        batch = ds.collate([1])
        batch["shading"] = shading
        batch["ambient_ratio"] = 1.0 if shading == "albedo" else 0.1
        with torch.autocast("cuda", dtype=torch.float16):  # as the Trainer's test loop does
            img, depth = trainer.test_step(batch)
        assert img.shape == (1, 16, 16, 3) and torch.isfinite(img).all(), shading
        assert depth.shape == (1, 16, 16) and torch.isfinite(depth).all()
    assert trainer.model.native_calls > 0


def test_checkpoint_round_trip(gpu, trainer_state, tmp_path):
    trainer, _ = make_trainer(gpu, 3, tmp=str(tmp_path))
    trainer.model.load_state_dict(trainer_state)
    trainer.ckpt_path = str(tmp_path)
    trainer.save_checkpoint("ck", full=True)
    fresh, _ = make_trainer(gpu, 4, tmp=str(tmp_path))
    fresh.ckpt_path = str(tmp_path)
    fresh.load_checkpoint(str(tmp_path / "ck.pth"))
    want, got = trainer.model.state_dict(), fresh.model.state_dict()
    assert want.keys() == got.keys()
    assert "sigma_net.net.0.skip.weight" in want and "bg_net.net.0.norm.weight" in want
    for k in want:
        assert torch.equal(want[k], got[k]), k
