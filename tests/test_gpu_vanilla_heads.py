"""The native vanilla field (csrc/resmlp.hip) on a trained-like head and at
an overflowing input gradient (cases: tests/field_head_cases.py, held to their
names on the CPU by tests/test_field_head_cases_host.py).

Rule of tests/test_gpu_vanilla.py: truth `r` in float64 (field_head_cases.
truth_field: the density head through an f64 trunc_exp, backward g *
exp(clamp(y, -15, 15))), stick `t` the module's torch path under fp16
autocast, candidate `y` the native path; the native error may not exceed twice
the stick's, and every test prints `parity:` lines with both.

* forward: sigma as max |log y - log r| (y spans e^-70 .. e^70: the row
  metric's mean |r| term would hide every small density), albedo by the row
  metric;
* backward: all 19 gradients by |g - r|_2 / |r|_2, with the class-scaled gs on
  all rows and ga ~ N(0, 1), then with gs on the low class (y < -16) only and
  on the high class (y > 16) only and ga = 0 (the density head alone);
* saturated albedo: ga non-zero only where the native f16 albedo is exactly 0
  or 1, gs = 0: all 19 gradients are exactly zero on both paths, which pins
  (1 - a) a on the ROUNDED a;
* overflowing input gradient: where f16(exp(y)) is inf the normal is exactly
  (0, 0, 0) on both paths and dx is not finite;
* the device-count entries give the host-count entries' bits on this head.
"""
import pytest
import torch

import field_head_cases as fc
from test_gpu_vanilla import check, field_grads, make_net, norm_err, run_path

pytestmark = pytest.mark.gpu

import _resmlp  # noqa: E402

W = _resmlp.WORKGROUP_ROWS


def log_err(y, r):
    return float((torch.log(y.detach().double()) - torch.log(r.detach().double())).abs().max())


@pytest.fixture(scope="module")
def trained(gpu):
    assert fc.SHAPES == [tuple(s) for s in _resmlp.SHAPES]
    return fc.load_params(make_net(gpu), fc.vanilla_case()["trained"])


@pytest.fixture(scope="module")
def overflow(gpu):
    return fc.load_params(make_net(gpu), fc.vanilla_case()["overflow"])


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("M", [2 * W + 1, 1000])
def test_forward(gpu, trained, M):
    x = fc.vanilla_case()["xs"][M].to(gpu)
    with torch.no_grad():
        ys, ya = run_path(trained, True, lambda: trained.common_forward(x))
        ts, ta = run_path(trained, False, lambda: trained.common_forward(x))
        rs, ra, _, ry = fc.truth_field(trained.sigma_net.parameters(), x.double())
    assert ys.dtype == torch.float32 and ya.dtype == torch.float16
    s = fc.class_shares(ry.cpu().numpy())
    assert s["low"] >= 0.15 and s["high"] >= 0.08 and s["max_abs"] <= fc.Y_MAX
    assert torch.isfinite(ys).all() and bool((ys > 0).all())
    check(f"heads forward M={M} log sigma", ys, ts, rs, err=log_err)
    check(f"heads forward M={M} albedo", ya, ta, ra)
    ones, zeros = float((ya == 1).float().mean()), float((ya == 0).float().mean())
    print(f"heads: forward M={M}: {s} native albedo == 1 {ones:.3f} == 0 {zeros:.3f}")
    assert ones >= 0.05 and zeros >= 0.02


# ---------------------------------------------------------------- backward
@pytest.mark.parametrize("side", [None, "low", "high"], ids=["all", "low", "high"])
def test_backward(gpu, trained, side):
    M = 1000
    x = fc.vanilla_case()["xs"][M].to(gpu)
    gs, ga = fc.vanilla_upstream(M)
    if side is not None:  # the density head of one class alone: no colour gradient beside it
        gs = fc.only(gs, fc.vanilla_truth_y(M)[1].numpy(), side)
        assert int(gs.count_nonzero()) >= 2
        ga = torch.zeros_like(ga)
    gs, ga = gs.to(gpu), ga.to(gpu)
    y = field_grads(trained, x, gs, ga, True)
    t = field_grads(trained, x, gs, ga, False)
    rs, ra, ps, _ = fc.truth_field(trained.sigma_net.parameters(), x.double())
    torch.autograd.backward([rs, ra], [gs.double(), ga.double()])
    names = [n for n, _ in trained.sigma_net.named_parameters()]
    assert len(names) == 19
    for n, gy, gt, p in zip(names, y, t, ps):
        assert gy.dtype == torch.float32 and gy.shape == p.shape
        assert torch.isfinite(gy).all(), n
        check(f"heads backward gs={side or 'all'} {n}", gy, gt, p.grad, err=norm_err)


def test_saturated_albedo_has_exactly_zero_gradient(gpu, trained):
    """sigmoid_backward on the rounded albedo: a == 0 or a == 1 in f16 gives
    (1 - a) a == 0 exactly, so a gradient that arrives only at those entries
    (and gs = 0) leaves all 19 parameter gradients exactly zero."""
    M = 1000
    x = fc.vanilla_case()["xs"][M].to(gpu)
    with torch.no_grad():
        _, ya = run_path(trained, True, lambda: trained.common_forward(x))
        _, ta = run_path(trained, False, lambda: trained.common_forward(x))
    sat = (ya == 0) | (ya == 1)
    assert float(sat.float().mean()) >= 0.07
    # the torch path saturates on the same entries (else its zero would not be owed)
    sat = sat & ((ta == 0) | (ta == 1))
    assert float(sat.float().mean()) >= 0.07
    _, ga = fc.vanilla_upstream(M)
    ga = torch.where(sat, ga.to(gpu), torch.zeros((), device=gpu))
    assert int(ga.count_nonzero()) == int(sat.sum())
    gs = torch.zeros(M, device=gpu)
    for fused in (True, False):
        grads = field_grads(trained, x, gs, ga, fused)
        for n, g in zip([n for n, _ in trained.sigma_net.named_parameters()], grads):
            assert int(g.count_nonzero()) == 0, (fused, n, float(g.abs().max()))
    # the control: the same gradient on the unsaturated entries does arrive
    ga = torch.where(sat, torch.zeros((), device=gpu), fc.vanilla_upstream(M)[1].to(gpu))
    grads = field_grads(trained, x, gs, ga, True)
    assert all(int(g.count_nonzero()) > 0 for g in grads)


# ---------------------------------------------------------------- overflowing dx
def test_overflowing_input_gradient_and_normal(gpu, overflow):
    """The base net with net.4.bias[0] raised: f16(exp(y)), where the
    density's gradient enters the f16 tensor h0, is the only overflow point.
    y > ln 65520 + 0.1: dx is not finite and the normal is exactly 0 on both
    paths; y < 7 (the range tests/test_gpu_vanilla.py covers): finite and under
    the usual rule; in between, where neither path is predictable without
    running it, the native normal is finite and zero or of unit length."""
    from nerf import vanilla_field as vf
    net = overflow
    x = fc.vanilla_case()["x_overflow"].to(gpu)
    x64 = x.double().requires_grad_(True)
    rs, _, _, ry = fc.truth_field(net.sigma_net.parameters(), x64)
    rdx = torch.autograd.grad(rs.sum(), x64)[0]
    ry = ry.detach()
    hi, lo = ry > fc.LN_F16_MAX + 0.1, ry < 7
    mid = ~hi & ~lo
    assert float(hi.float().mean()) >= 0.10 and float(lo.float().mean()) >= 0.30
    with torch.no_grad():
        ydx = run_path(net, True, lambda: vf.input_gradient(net, x))
        yn = run_path(net, True, lambda: net.normal(x.clone()))
        tn = run_path(net, False, lambda: net.normal(x.clone()))
    assert yn.requires_grad is False and tn.requires_grad is False
    # the overflowing rows
    assert bool((~torch.isfinite(ydx[hi])).any(1).all())
    assert int(yn[hi].count_nonzero()) == 0 and int(tn[hi].count_nonzero()) == 0
    # the covered range

    def stick_dx():
        xs = x.clone().requires_grad_(True)
        sigma, _ = net.common_forward(xs)
        return torch.autograd.grad(sigma.sum(), xs)[0]
    tdx = run_path(net, False, stick_dx)
    assert torch.isfinite(ydx[lo]).all() and torch.isfinite(tdx[lo]).all()
    check("heads overflow dx, y < 7", ydx[lo], tdx[lo], rdx[lo])
    rn = -rdx / torch.sqrt(torch.clamp((rdx * rdx).sum(-1, keepdim=True), min=1e-20))
    check("heads overflow normal, y < 7", yn[lo], tn[lo], rn[lo])
    # in between
    assert torch.isfinite(yn).all()
    length = yn[mid].norm(dim=-1)
    assert bool(((length == 0) | ((length - 1).abs() <= 1e-3)).all())
    print(f"heads: overflow rows {int(hi.sum())}, covered {int(lo.sum())}, between "
          f"{int(mid.sum())} of which native zero normals {int((length == 0).sum())}")


# ---------------------------------------------------------------- device-count forms
def test_device_count_forms_equal_host_count_on_trained_head(gpu):
    """One case of tests/test_gpu_resmlp_dev.py's comparison (m = 2049, align
    = 128) with the trained parameters and the class-scaled gs: the forward and
    the 19 gradients of the device-count entries are the host-count entries'
    bits."""
    import test_gpu_resmlp_dev as dev
    m, align = 2049, 128
    cap = -(-m // align) * align + 256
    ps = [p.to(gpu).contiguous() for p in fc.vanilla_case()["trained"]]
    xyz = torch.zeros(cap, 3)
    xyz[:m] = fc.vanilla_case()["xs"][m]
    gs, ga = torch.zeros(cap), torch.zeros(cap, 3)
    gs[:m], ga[:m] = fc.vanilla_upstream(m)
    case = dict(ps=ps, xyz=xyz.to(gpu), gs=gs.to(gpu), ga=(ga * 1e-2).to(gpu).half(),
                scratch=torch.empty(_resmlp.backward_dev_scratch_bytes(cap), dtype=torch.uint8,
                                    device=gpu))
    want_s = torch.empty(cap, device=gpu)
    want_a = torch.empty(cap, 3, device=gpu, dtype=torch.float16)
    _resmlp.field_forward(case["xyz"], ps, want_s, want_a)
    sigma = torch.full((cap,), dev.SENTINEL, device=gpu)
    albedo = torch.full((cap, 3), dev.SENTINEL, device=gpu, dtype=torch.float16)
    _resmlp.field_forward_dev(dev.nan_tail(case["xyz"], m), ps, sigma, albedo, dev.count(gpu, m),
                              align)
    torch.cuda.synchronize()
    assert torch.equal(sigma[:m], want_s[:m]) and torch.equal(albedo[:m], want_a[:m])
    assert bool((sigma[m:] == dev.SENTINEL).all()) and bool((albedo[m:] == dev.SENTINEL).all())
    s = fc.class_shares(torch.log(sigma[:m].double()).cpu().numpy())
    assert s["low"] >= 0.15 and s["high"] >= 0.08
    Me = -(-m // align) * align
    want = [torch.empty_like(p) for p in ps]
    dev.host_backward(case, Me, m, want)
    got = [torch.full_like(p, float("nan")) for p in ps]
    dev.dev_backward(gpu, case, m, align, got)
    torch.cuda.synchronize()
    dev.assert_equal_grads(got, want, ("trained head", m, align))
    assert all(float(w.abs().sum()) > 0 for w in want)
