"""GPU tests of the device-count forms of the vanilla field
(dfhip_resmlp_field_forward_dev / _backward_dev, csrc/resmlp.hip) and of the
opacity regulariser's entries (dfhip_opacity_forward / _backward_accumulate,
csrc/head.hip).

The device-count entries are compared bit for bit with the host-count entries:
the forward on the live rows (rows past the count hold NaN positions and a
sentinel that must survive), the backward's 19 gradients with
dfhip_resmlp_field_backward on Me = min(cap, align_up(m, align)) rows of
zero-padded copies, where the device-count buffers hold NaN from row m on.
The capacity 65536 + 256 spans two backward chunks; the counts sit around the
16-row tile, the 32-row k-step, the 128-row workgroup pass and slice, the
2048 rows at which a chunk takes all 64 splits, and the chunk edge.

The opacity forward is compared with a float64 sum in numpy (one f32 ulp: the
kernel rounds a f64 value once), the backward with the documented f32
expression evaluated operation by operation in numpy f32.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _dfhip  # noqa: E402
import _resmlp  # noqa: E402

CAP = 65536 + 256
FWD_M = [0, 1, 15, 16, 17, 127, 128, 129, 65536, 65537, CAP]
BWD_M = [1, 31, 32, 33, 128, 2049, 65536, 65537, 65536 + 129]
SENTINEL = -7.25


def make_params(gpu, seed=0):
    """Seeded random sigma_net parameters with the reference's shapes."""
    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla"])
    torch.manual_seed(seed)
    net = NeRFNetwork(opt).to(gpu)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in net.sigma_net.named_parameters():
            if name.endswith("norm.weight"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return [p.detach().contiguous() for p in net.sigma_net.parameters()]


@pytest.fixture(scope="module")
def case(gpu):
    """Parameters, positions in [-1, 1], upstream gradients, the host-count
    forward of every row and the device-count scratch: made once, read only."""
    ps = make_params(gpu)
    g = torch.Generator().manual_seed(7)
    xyz = (torch.rand(CAP, 3, generator=g) * 2 - 1).to(gpu)
    xyz[0] = 0.0
    gs = (torch.randn(CAP, generator=g) * 1e-2).to(gpu)
    ga = (torch.randn(CAP, 3, generator=g) * 1e-2).to(gpu).half()
    sigma = torch.empty(CAP, device=gpu)
    albedo = torch.empty(CAP, 3, device=gpu, dtype=torch.float16)
    _resmlp.field_forward(xyz, ps, sigma, albedo)
    scratch = torch.empty(_resmlp.backward_dev_scratch_bytes(CAP), dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    return dict(ps=ps, xyz=xyz, gs=gs, ga=ga, sigma=sigma, albedo=albedo, scratch=scratch)


def count(gpu, m):
    return torch.tensor([m], dtype=torch.int32, device=gpu)


def nan_tail(t, m):
    t = t.clone()
    t[m:] = float("nan")
    return t


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("m_dev", FWD_M + [CAP + 1000])
def test_forward_dev_equals_host_count_on_live_rows(gpu, case, m_dev):
    m = min(m_dev, CAP)  # the kernels clamp the count to the capacity
    xyz = nan_tail(case["xyz"], m)
    sigma = torch.full((CAP,), SENTINEL, device=gpu)
    albedo = torch.full((CAP, 3), SENTINEL, device=gpu, dtype=torch.float16)
    _resmlp.field_forward_dev(xyz, case["ps"], sigma, albedo, count(gpu, m_dev), 128)
    torch.cuda.synchronize()
    assert torch.equal(sigma[:m], case["sigma"][:m])
    assert torch.equal(albedo[:m], case["albedo"][:m])
    assert bool((sigma[m:] == SENTINEL).all()) and bool((albedo[m:] == SENTINEL).all())
    if 0 < m < 1000:  # literally the host-count entry on the same rows
        s2 = torch.empty(m, device=gpu)
        a2 = torch.empty(m, 3, device=gpu, dtype=torch.float16)
        _resmlp.field_forward(xyz[:m].contiguous(), case["ps"], s2, a2)
        assert torch.equal(sigma[:m], s2) and torch.equal(albedo[:m], a2)


def test_forward_dev_negative_count_is_empty(gpu, case):
    sigma = torch.full((CAP,), SENTINEL, device=gpu)
    albedo = torch.full((CAP, 3), SENTINEL, device=gpu, dtype=torch.float16)
    _resmlp.field_forward_dev(nan_tail(case["xyz"], 0), case["ps"], sigma, albedo,
                              count(gpu, -5), 1)
    assert bool((sigma == SENTINEL).all()) and bool((albedo == SENTINEL).all())


# ---------------------------------------------------------------- backward
def host_backward(case, Me, m, grads, accumulate=False, ga=None):
    """dfhip_resmlp_field_backward on Me rows of copies whose rows [m, Me) are zero."""
    ga = case["ga"] if ga is None else ga
    x, gs, ga = case["xyz"][:Me].clone(), case["gs"][:Me].clone(), ga[:Me].clone()
    x[m:], gs[m:], ga[m:] = 0, 0, 0
    _resmlp.field_backward(x, case["ps"], gs, ga, grads=grads, accumulate=accumulate)


def dev_backward(gpu, case, m, align, grads, accumulate=False, ga=None):
    ga = case["ga"] if ga is None else ga
    _resmlp.field_backward_dev(nan_tail(case["xyz"], m), case["ps"], nan_tail(case["gs"], m),
                               nan_tail(ga, m), grads, count(gpu, m), align,
                               accumulate=accumulate, scratch=case["scratch"])


def assert_equal_grads(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(w).all(), (what, i)
        assert torch.equal(g, w), (what, i, float((g - w).abs().max()))


@pytest.mark.parametrize("align", [1, 128])
@pytest.mark.parametrize("m", BWD_M)
def test_backward_dev_equals_host_count_on_padded_rows(gpu, case, m, align):
    Me = min(CAP, -(-m // align) * align)
    want = [torch.empty_like(p) for p in case["ps"]]
    host_backward(case, Me, m, want)
    got = [torch.full_like(p, float("nan")) for p in case["ps"]]
    dev_backward(gpu, case, m, align, got)
    torch.cuda.synchronize()
    assert_equal_grads(got, want, (m, align))
    assert any(float(w.abs().sum()) > 0 for w in want)
    # two runs give equal bits
    again = [torch.full_like(p, float("nan")) for p in case["ps"]]
    dev_backward(gpu, case, m, align, again)
    assert_equal_grads(again, got, ("rerun", m, align))


@pytest.mark.parametrize("m, align", [(2049, 128), (65536 + 129, 128), (33, 1)])
def test_backward_dev_accumulates_as_the_host_count_entry(gpu, case, m, align):
    Me = min(CAP, -(-m // align) * align)
    g = torch.Generator().manual_seed(m)
    base = [torch.randn(p.shape, generator=g).to(gpu) * 1e-3 for p in case["ps"]]
    want = [b.clone() for b in base]
    host_backward(case, Me, m, want, accumulate=True)
    got = [b.clone() for b in base]
    dev_backward(gpu, case, m, align, got, accumulate=True)
    assert_equal_grads(got, want, ("accumulate", m, align))
    assert not torch.equal(got[0], base[0])


def test_backward_dev_f32_albedo_gradient(gpu, case):
    m, align = 65537, 128
    Me = min(CAP, -(-m // align) * align)
    ga = case["ga"].float() * 1.0009765625  # not f16 values: the kernels round them
    want = [torch.empty_like(p) for p in case["ps"]]
    host_backward(case, Me, m, want, ga=ga)
    got = [torch.full_like(p, float("nan")) for p in case["ps"]]
    dev_backward(gpu, case, m, align, got, ga=ga)
    assert_equal_grads(got, want, "f32 grad_albedo")


def test_backward_dev_empty_count(gpu, case):
    got = [torch.full_like(p, float("nan")) for p in case["ps"]]
    dev_backward(gpu, case, 0, 128, got)
    assert all(bool((g == 0).all()) for g in got)  # zeros written from the kernel
    base = [torch.full_like(p, 0.375) for p in case["ps"]]
    dev_backward(gpu, case, 0, 128, base, accumulate=True)
    assert all(bool((g == 0.375).all()) for g in base)  # left untouched


# ---------------------------------------------------------------- opacity
def opacity_ws(N, seed):
    rng = np.random.default_rng(seed)
    ws = rng.random(N, dtype=np.float32)
    ws[0] = 1.0
    if N > 1:
        ws[-1] = 0.0
    return ws


@pytest.mark.parametrize("N", [1, 63, 64, 65, 256])
def test_opacity_forward(gpu, N):
    lam = np.float32(1e-3)
    ws = opacity_ws(N, N)
    d_ws = torch.from_numpy(ws).to(gpu)
    loss = torch.full((1,), float("nan"), device=gpu)
    _dfhip.call("dfhip_opacity_forward", N, _dfhip.ptr(d_ws), float(lam), _dfhip.ptr(loss), 0,
                _dfhip.stream())
    got = np.float32(loss.item())
    want = np.float64(lam) * np.sum(ws.astype(np.float64) ** 2) / N
    print(f"parity: opacity forward N={N}: got {got!r} f64 {want!r}")
    assert abs(np.float64(got) - want) <= np.spacing(np.float32(want))
    # accumulate adds the same f32 value onto a preset loss
    preset = np.float32(0.3141592)
    loss.fill_(float(preset))
    _dfhip.call("dfhip_opacity_forward", N, _dfhip.ptr(d_ws), float(lam), _dfhip.ptr(loss), 1,
                _dfhip.stream())
    assert np.float32(loss.item()) == np.float32(preset + got)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 256])
def test_opacity_backward_accumulate(gpu, N):
    lam, g = np.float32(1e-3), np.float32(3.7 * 65536)
    ws = opacity_ws(N, 100 + N)
    pre = np.random.default_rng(N).standard_normal(N).astype(np.float32)
    scale = np.float32(np.float32(g * lam) / np.float32(N))
    want = pre + scale * (np.float32(2) * ws)
    assert want.dtype == np.float32
    d_ws, d_pre = torch.from_numpy(ws).to(gpu), torch.from_numpy(pre).to(gpu)
    d_g = torch.tensor([float(g)], device=gpu)
    _dfhip.call("dfhip_opacity_backward_accumulate", N, _dfhip.ptr(d_ws), _dfhip.ptr(d_g),
                float(lam), _dfhip.ptr(d_pre), _dfhip.stream())
    assert np.array_equal(d_pre.cpu().numpy(), want)
