"""GPU tests of the device-count forms of the voxel field
(dfhip_voxel_field_forward_dev, dfhip_voxel_normal_dev,
dfhip_voxel_field_backward_dev) and of the training shading entries
(dfhip_voxel_shade_train_forward / _backward; csrc/voxelstep.hip), the kernels
of the DVGO backbone's native train step.

Device count against host count, bit for bit (torch.equal): the buffers hold
`cap` rows, the live count sits in a device int32, rows at or past it hold NaN
in every input and must be neither read nor written.  The backward sums over
Me = min(cap, align_up(live, align)) rows and equals the host-count backward on
Me rows whose tail holds position 0 and gradient 0.

Shading entry: the rules of tests/test_gpu_voxel.py::test_shadings.  Colours
and the lambertian factor (f16-rounded) may not err more than twice the
module's torch path does against the float64 truth of tests/voxel_cases.py;
the unit normal (f32) obeys the window rule |y - r| <= max(2 |t - r|, w).  The
orientation term may lie no farther from a float64 evaluation of its formula
on the entry's own buffers than twice the torch float32 expression does.
"""
import pytest
import torch
import torch.nn.functional as F

import voxel_cases as vc

pytestmark = pytest.mark.gpu

import _voxelfield  # noqa: E402

LIVE = [0, 1, 15, 16, 17, 257, 1000, 65536, 65537]
SLACK = 300 + 37  # capacity = live + SLACK: no multiple of the 32-row padding
CKPTS = {"small": dict(world=vc.WORLD_SMALL), "padded": dict(world=vc.WORLD_SMALL, C=4, posbase=0)}
NAN = float("nan")


# ---------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def nets(gpu, tmp_path_factory):
    import main
    tmp = tmp_path_factory.mktemp("dvgo_step")
    out = {}
    for name, kw in CKPTS.items():
        sd, _ = vc.make_state(seed=len(out), **kw)
        path = vc.save_checkpoint(tmp / f"{name}.dvgo", sd)
        opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
        out[name] = (main.network_class(opt)(opt).to(gpu), sd)
    return out


def operands(net):
    from nerf import voxel_field as vf
    m = net.main_net
    return (vf.volume(net)[0], float(m.act_shift),
            [p.detach().contiguous() for p in m.rgbnet.parameters()])


_POS = {}


def positions(gpu, n):
    """n positions (the edge rows first), drawn once and shared."""
    if "x" not in _POS:
        _POS["x"] = vc.positions(max(LIVE) + 8, vc.WORLD_SMALL, seed=21).to(gpu)
    return _POS["x"][:n]


def count(gpu, live):
    return torch.tensor([live], dtype=torch.int32, device=gpu)


def poisoned(gpu, cap, live, rows, dtype=torch.float32):
    """[cap, 3] holding `rows` in its first `live` rows, NaN past them."""
    t = torch.full((cap, 3), NAN, device=gpu, dtype=dtype)
    t[:live] = rows.to(dtype)
    return t


def effective(live, cap, align):
    return min(cap, -(-live // align) * align)


def row_err(y, r):
    y, r = y.detach().double().cpu(), r.detach().double().cpu()
    return float(((y - r).abs() / (r.abs() + r.abs().mean())).max()) if r.numel() else 0.0


def check(name, y, t, r):
    """The 2x rule of the f16-rounded quantities."""
    ey, et = row_err(y, r), row_err(t, r)
    print(f"parity: {name}: native {ey:.3e} torch {et:.3e}")
    assert torch.isfinite(t).all() and torch.isfinite(y).all(), name
    assert ey <= 2 * et, (name, ey, et)


def check_window(name, y, t, r, w):
    """The rule of the f32-only quantities, per row and component."""
    y, t = y.detach().double().cpu(), t.detach().double().cpu()
    ey, et = (y - r).abs(), (t - r).abs()
    print(f"parity: {name}: native {float(ey.max()):.3e} torch {float(et.max()):.3e}")
    assert (et <= w).all(), (name, "the stick leaves the window")
    assert (ey <= torch.maximum(2 * et, w)).all(), name


def unit_window(rn, w_n):
    return 2 * w_n.norm(dim=-1, keepdim=True) / rn.norm(dim=-1, keepdim=True).clamp(min=1e-300) \
        + 8 * vc.EPS


# ---------------------------------------------------------------- device count
@pytest.mark.parametrize("align", [1, 128])
@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("ckpt", list(CKPTS))
def test_forward_and_normal_dev(gpu, nets, ckpt, live, align):
    net = nets[ckpt][0]
    vol, shift, ws = operands(net)
    cap = live + SLACK
    x = poisoned(gpu, cap, live, positions(gpu, live))
    m_dev = count(gpu, live)
    xs = x[:live].contiguous()
    want_s = torch.empty(live, device=gpu)
    want_a = torch.empty(live, 3, device=gpu, dtype=torch.float16)
    want_n = torch.empty(live, 3, device=gpu)
    _voxelfield.field_forward(xs, vol, 1.0, shift, ws, want_s, want_a)
    _voxelfield.normal(xs, vol, 1.0, shift, want_n)
    sigma = torch.full((cap,), NAN, device=gpu)
    albedo = torch.full((cap, 3), NAN, device=gpu, dtype=torch.float16)
    normal = torch.full((cap, 3), NAN, device=gpu)
    _voxelfield.field_forward_dev(x, vol, 1.0, shift, ws, sigma, albedo, m_dev, align)
    _voxelfield.normal_dev(x, vol, 1.0, shift, normal, m_dev, align)
    assert torch.equal(sigma[:live], want_s) and torch.equal(albedo[:live], want_a)
    assert torch.equal(normal[:live], want_n)
    if live:
        assert torch.isfinite(sigma[:live]).all() and torch.isfinite(albedo[:live]).all()
    # rows past the live count keep the poison of the output buffers
    assert torch.isnan(sigma[live:]).all() and torch.isnan(albedo[live:]).all()
    assert torch.isnan(normal[live:]).all()
    # the density branch alone
    only = torch.full((cap,), NAN, device=gpu)
    _voxelfield.field_forward_dev(x, vol, 1.0, shift, None, only, None, m_dev, align)
    assert torch.equal(only[:live], want_s) and torch.isnan(only[live:]).all()


def backward_case(gpu, net, live, cap, align):
    vol, _, ws = operands(net)
    Me = effective(live, cap, align)
    g = torch.Generator().manual_seed(5 + live)
    ga_live = torch.randn(live, 3, generator=g).to(gpu).half().float()  # f16-representable
    x = poisoned(gpu, cap, live, positions(gpu, live))
    ga = poisoned(gpu, cap, live, ga_live)
    m_dev = count(gpu, live)
    # the host-count backward on Me rows with zeroed tail rows
    xr = torch.zeros(Me, 3, device=gpu)
    gr = torch.zeros(Me, 3, device=gpu)
    xr[:live], gr[:live] = x[:live], ga_live
    want = [torch.full_like(w, NAN) for w in ws]
    _voxelfield.field_backward(xr, vol, 1.0, ws, gr, want)
    assert all(torch.isfinite(w).all() for w in want)
    if live > 16:
        assert all(float(w.abs().sum()) > 0 for w in want)
    scratch = torch.empty(_voxelfield.backward_dev_scratch_bytes(cap, vol.dim0),
                          dtype=torch.uint8, device=gpu)
    got = [torch.full_like(w, NAN) for w in ws]
    _voxelfield.field_backward_dev(x, vol, 1.0, ws, ga, got, m_dev, align, scratch=scratch)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    again = [torch.full_like(w, NAN) for w in ws]  # two runs, the same bits
    _voxelfield.field_backward_dev(x, vol, 1.0, ws, ga, again, m_dev, align, scratch=scratch)
    for a, b in zip(again, got):
        assert torch.equal(a, b)
    half = [torch.full_like(w, NAN) for w in ws]  # an f16 gradient
    _voxelfield.field_backward_dev(x, vol, 1.0, ws, ga.half(), half, m_dev, align,
                                   scratch=scratch)
    for a, b in zip(half, want):
        assert torch.equal(a, b)
    preset = [torch.randn(w.shape, generator=g).to(gpu) for w in ws]
    acc, acc_want = [p.clone() for p in preset], [p.clone() for p in preset]
    _voxelfield.field_backward(xr, vol, 1.0, ws, gr, acc_want, accumulate=True)
    _voxelfield.field_backward_dev(x, vol, 1.0, ws, ga, acc, m_dev, align, accumulate=True,
                                   scratch=scratch)
    for a, b, p in zip(acc, acc_want, preset):
        assert torch.equal(a, b)
        if Me == 0:
            assert torch.equal(a, p)
    if Me == 0:
        assert all(torch.equal(a, torch.zeros_like(a)) for a in got)


@pytest.mark.parametrize("align", [1, 128])
@pytest.mark.parametrize("live", LIVE)
@pytest.mark.parametrize("ckpt", list(CKPTS))
def test_backward_dev(gpu, nets, ckpt, live, align):
    backward_case(gpu, nets[ckpt][0], live, live + SLACK, align)


def test_backward_dev_effective_rows_stop_at_the_capacity(gpu, nets):
    """align_up(live, 128) beyond the capacity: Me = cap."""
    backward_case(gpu, nets["small"][0], 1000, 1010, 128)
    assert effective(1000, 1010, 128) == 1010


def test_dev_scratch_bytes(gpu):
    rows, per_chunk = 616 * 2, 64 * 4 * (128 * 72 + 17027)
    assert _voxelfield.backward_dev_scratch_bytes(64 * 64 * 512, 72) == \
        rows * 64 * 64 * 512 + 32 * per_chunk == 2798673920
    assert _voxelfield.backward_dev_scratch_bytes(128 * 128 * 512, 72) == 11194695680
    assert _voxelfield.backward_dev_scratch_bytes(33, 72) == rows * 64 + per_chunk


# ---------------------------------------------------------------- shading entry
M_SHADE = 1000
LIGHT = F.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
_REF = {}


def shade_truth(nets):
    """The float64 reference of the shading case, computed once and shared."""
    if not _REF:
        sd = nets["small"][1]
        x = vc.positions(M_SHADE, vc.WORLD_SMALL, seed=0)
        rs, ra, _, aux = vc.truth(sd, x)
        rn = vc.normal_of(rs, aux)
        _, w_n = vc.windows(rs, aux)
        d = F.normalize(vc.positions(M_SHADE, vc.WORLD_SMALL, seed=8, edges=False) + 0.01, dim=-1)
        _REF.update(x=x, d=d, albedo=ra.detach(), normal=rn, w_n=w_n)
    return _REF


def shade(gpu, net, x, d, shading, ratio, live, cap, align=128):
    """The entry on capacity-sized, poisoned buffers; albedo from the field."""
    vol, shift, ws = operands(net)
    xs, ds = poisoned(gpu, cap, live, x[:live]), poisoned(gpu, cap, live, d[:live])
    m_dev = count(gpu, live)
    sigma = torch.full((cap,), NAN, device=gpu)
    albedo = torch.full((cap, 3), NAN, device=gpu, dtype=torch.float16)
    _voxelfield.field_forward_dev(xs, vol, 1.0, shift, ws, sigma, albedo, m_dev, align)
    normal = torch.full((cap, 3), NAN, device=gpu)
    lam = torch.full((cap,), NAN, device=gpu, dtype=torch.float16)
    color = torch.full((cap, 3), NAN, device=gpu, dtype=torch.float16)
    orient = torch.full((1,), NAN, device=gpu)
    partial = torch.empty(_voxelfield.shade_partial_doubles(cap), device=gpu, dtype=torch.float64)
    _voxelfield.shade_train_forward(xs, ds, vol, 1.0, shift,
                                    albedo if shading == "lambertian" else None, LIGHT.to(gpu),
                                    ratio, shading, m_dev, align, normal, lam, color, partial,
                                    orient)
    return dict(sigma=sigma, albedo=albedo, normal=normal, lam=lam, color=color, orient=orient,
                m_dev=m_dev, dirs=ds)


@pytest.mark.parametrize("ratio", [0.1, 0.0])
@pytest.mark.parametrize("shading", ["textureless", "lambertian"])
def test_shading_forward(gpu, nets, shading, ratio):
    net = nets["small"][0]
    ref = shade_truth(nets)
    x, d = ref["x"].to(gpu), ref["d"].to(gpu)
    live, cap = M_SHADE, M_SHADE + SLACK
    out = shade(gpu, net, x, d, shading, ratio, live, cap)
    # the stick: the module's torch path under fp16 autocast
    net.fused_field = False
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            ts, tc, tn = net(x.clone(), d, LIGHT.to(gpu), ratio=ratio, shading=shading)
            _, tl, _ = net(x.clone(), d, LIGHT.to(gpu), ratio=ratio, shading="textureless")
    finally:
        net.fused_field = True
    rn = vc.unit(ref["normal"])
    lam = ratio + (1 - ratio) * (rn @ LIGHT.double()).clamp(min=0)
    rc = lam[:, None].repeat(1, 3) if shading == "textureless" else ref["albedo"] * lam[:, None]
    assert out["color"].dtype == torch.float16 and out["lam"].dtype == torch.float16
    check(f"{shading} ratio={ratio} colour", out["color"][:live], tc, rc)
    check(f"{shading} ratio={ratio} factor", out["lam"][:live], tl[:, 0], lam)
    check_window(f"{shading} ratio={ratio} normal", out["normal"][:live], tn, rn,
                 unit_window(ref["normal"], ref["w_n"]))
    for k in ("normal", "lam", "color"):
        assert torch.isnan(out[k][live:]).all(), k
    # the orientation term against float64 on the entry's own buffers
    Me = effective(live, cap, 128)
    n64, d64, s64 = (out[k][:live].double() for k in ("normal", "dirs", "sigma"))
    r = float(((1 - torch.exp(-s64)) * (n64 * d64).sum(-1).clamp(min=0) ** 2).sum() / Me)
    n32, d32, s32 = (out[k][:live] for k in ("normal", "dirs", "sigma"))
    terms = torch.zeros(Me, device=gpu)
    terms[:live] = (1 - torch.exp(-s32)) * (n32 * d32).sum(-1).clamp(min=0) ** 2
    t, y = float(terms.mean()), float(out["orient"])
    print(f"parity: {shading} ratio={ratio} orient: native {abs(y - r):.3e} torch {abs(t - r):.3e} "
          f"of {r:.6e}")
    assert r > 0 and abs(y - r) <= 2 * abs(t - r)


def test_shading_flat_density_gives_exactly_zero_normals(gpu, tmp_path):
    import main
    sd, _ = vc.make_state(density=torch.full((1, 1, *vc.WORLD_SMALL), 1.5))
    path = vc.save_checkpoint(tmp_path / "flat.dvgo", sd)
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
    net = main.network_class(opt)(opt).to(gpu)
    live = 57
    x = vc.positions(live, vc.WORLD_SMALL, seed=4).to(gpu)
    d = F.normalize(torch.ones(live, 3), dim=-1).to(gpu)
    out = shade(gpu, net, x, d, "textureless", 0.1, live, live + SLACK, align=1)
    assert torch.equal(out["normal"][:live], torch.zeros(live, 3, device=gpu))
    assert torch.equal(out["lam"][:live], torch.full((live,), 0.1, device=gpu).half())
    assert float(out["orient"]) == 0.0


def test_shading_no_live_rows(gpu, nets):
    ref = shade_truth(nets)
    out = shade(gpu, nets["small"][0], ref["x"].to(gpu), ref["d"].to(gpu), "lambertian", 0.1, 0,
                SLACK)
    assert float(out["orient"]) == 0.0
    assert torch.isnan(out["color"]).all() and torch.isnan(out["normal"]).all()


def test_shading_backward(gpu, nets):
    ref = shade_truth(nets)
    live, cap = M_SHADE, M_SHADE + SLACK
    out = shade(gpu, nets["small"][0], ref["x"].to(gpu), ref["d"].to(gpu), "lambertian", 0.1,
                live, cap)
    g = torch.Generator().manual_seed(9)
    gc = poisoned(gpu, cap, live, torch.randn(live, 3, generator=g).to(gpu), torch.float16)
    ga = torch.full((cap, 3), NAN, device=gpu, dtype=torch.float16)
    _voxelfield.shade_train_backward(gc, out["lam"], "lambertian", out["m_dev"], 128, ga)
    want = gc[:live] * out["lam"][:live, None]  # torch half operations
    assert want.dtype == torch.float16 and float(want.float().abs().sum()) > 0
    assert torch.equal(ga[:live], want)
    assert torch.isnan(ga[live:]).all()
    # a textureless step has no albedo gradient: nothing is written
    none = torch.full((cap, 3), NAN, device=gpu, dtype=torch.float16)
    _voxelfield.shade_train_backward(gc, out["lam"], "textureless", out["m_dev"], 128, none)
    assert torch.isnan(none).all()
