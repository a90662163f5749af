"""The per-ray head and the entropy regulariser (csrc/head.hip) at their edges,
against the float64 / f16-graph oracle of oracle/field.py (bg_forward,
bg_backward, bg_bounds, ray_tail, entropy): ray counts that are no multiple of
the 64 rays of a workgroup (dead rays staged, every path of k_head_wsum's
loops), edge values of ws / nears / fars / directions, the mix without a
background network, the entropy kernels around their clamp thresholds and
loop limits, and the fused C-ABI entries against their parts bit for bit.

u = 2^-24 throughout.  Tests print `parity:` lines with the worst error /
bound ratios (kept in profiles/head/parity.txt)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import oracle.field as of
from oracle_checks import check_ray_head, ray_head_inputs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
LO, HI = F32(1e-5), F32(1) - F32(1e-5)
_UP, _DN = F32(np.inf), F32(-np.inf)
# 0, 1, 0.5, the two clamp thresholds and their float32 neighbours; then a
# negative value and one above 1
SPECIAL = np.array([0, 1, 0.5, LO, HI, np.nextafter(LO, _DN), np.nextafter(HI, _DN),
                    np.nextafter(LO, _UP), np.nextafter(HI, _UP), -0.25, 1.5], F32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _net(gpu, seed=3):
    torch.manual_seed(seed)
    return nn.Linear(39, 64).to(gpu), nn.Linear(64, 3).to(gpu)


# ---------------------------------------------------------------- a. ray counts

# 1, 63: one partial workgroup; 65: a full one and one ray; 130: three; 7700:
# 121 workgroups (only waves 0..8 of k_head_wsum take the eight-wide loop);
# 15983: 250 (eight-wide once or twice, then a tail)
@pytest.mark.parametrize("N", [1, 63, 65, 130, 7700, 15983])
def test_ray_head_ray_counts(gpu, N):
    l1, l2 = _net(gpu)
    check_ray_head(gpu, N, l1, l2, ray_head_inputs(N, 40 + N))


# ---------------------------------------------------------------- b. edge values

def test_ray_head_edge_values(gpu):
    """N = 130 with ws in {0, 1, 1 + 2^-23}, fars == nears (finite, and both
    FLT_MAX as the step prologue writes for a miss), fars < nears, depth <
    nears, axis directions, a -0.0 and a 1e-30 component: inside the same
    windows, depth and mask bit-equal to ray_tail with NaNs in the same
    places."""
    N = 130
    inp = ray_head_inputs(N, 7)
    inp["ws"][0:3] = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -23])
    inp["nears"][3], inp["fars"][3] = 0.5, 0.5
    inp["nears"][4], inp["fars"][4] = FLT_MAX, FLT_MAX
    inp["nears"][5], inp["fars"][5] = 0.9, 0.4
    inp["depth"][6], inp["nears"][6], inp["fars"][6] = 0.1, 0.3, 1.0
    # the last two rays: alone in the third workgroup, next to 62 dead rays
    inp["nears"][129], inp["fars"][129] = FLT_MAX, FLT_MAX
    inp["ws"][128] = 1.0
    e = torch.eye(3)
    inp["d"][7:10], inp["d"][10:13] = e, -e
    inp["d"][13] = torch.tensor([-0.0, 1.0, 0.0])
    inp["d"][14] = torch.tensor([1e-30, 0.0, -1.0])
    l1, l2 = _net(gpu)
    r = check_ray_head(gpu, N, l1, l2, inp)
    nan = np.isnan(r["want_depth"])
    assert nan[3] or np.isinf(r["want_depth"][3])
    assert nan[4] and nan[129] and r["want_depth"][6] == 0.0 and r["want_depth"][5] <= 0.0
    assert np.array_equal(np.isnan(r["depth"]), nan)
    assert np.array_equal(_bits(r["depth"])[~nan], _bits(r["want_depth"])[~nan])
    assert np.array_equal(r["mask"], r["want_mask"]) and r["mask"].dtype == np.bool_
    assert not r["mask"][[3, 4, 5, 129]].any() and r["mask"][6]


# ---------------------------------------------------------------- c. no background network

@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("with_bg", [False, True])
def test_ray_head_plain_mix(gpu, N, with_bg):
    """bg_color None (white) or an [N, 3] tensor that requires grad: image
    within 2u (|image| + |(1 - ws) bg|) of the float64 value (1 - ws, its
    product and the sum round), grad_image bit-equal to the upstream, grad_bg
    within 1u of g (1 - ws) with 1 - ws the float32 value autograd saves (one
    product), grad_ws within 3u sum|g bg| of the float64 -sum g bg (three
    products, three sums; not bit-equal: the compiler may contract)."""
    from nerf import head as _head
    inp = ray_head_inputs(N, 90 + N)
    g = torch.Generator(device="cpu").manual_seed(N)
    bg = torch.rand(N, 3, generator=g) if with_bg else None
    ws = inp["ws"].to(gpu).requires_grad_()
    image = inp["image"].to(gpu).requires_grad_()
    bg_t = bg.to(gpu).requires_grad_() if with_bg else None
    gimg = inp["gimg"].to(gpu)
    out_img, out_depth, mask = _head.ray_head(ws, inp["depth"].to(gpu), image, None,
                                              inp["nears"].to(gpu), inp["fars"].to(gpu), bg_t, None)
    grads = torch.autograd.grad(out_img, [ws, image] + ([bg_t] if with_bg else []), gimg)
    ws_np, img_np = inp["ws"].numpy(), inp["image"].numpy()
    bg_np = bg.numpy() if with_bg else np.ones((N, 3), F32)
    mix = (1.0 - ws_np.astype(np.float64))[:, None] * bg_np
    want = img_np.astype(np.float64) + mix
    err = np.abs(out_img.detach().t().cpu().numpy().astype(np.float64) - want)
    bound = 2 * U * (np.abs(img_np) + np.abs(mix))
    r_img = float((err / bound).max())
    _, ed, em = of.ray_tail(ws_np, inp["depth"].numpy(), img_np, inp["nears"].numpy(),
                            inp["fars"].numpy(), bg_np)
    np.testing.assert_array_equal(out_depth.detach().cpu().numpy(), ed)
    np.testing.assert_array_equal(mask.cpu().numpy(), em)
    g_np = inp["gimg"].t().numpy().astype(F32)
    assert np.array_equal(_bits(grads[1].cpu().numpy()), _bits(np.ascontiguousarray(g_np)))
    gb = g_np.astype(np.float64) * bg_np
    err_ws = np.abs(grads[0].cpu().numpy().astype(np.float64) + gb.sum(1))
    r_ws = float((err_ws / (3 * U * np.abs(gb).sum(1))).max())
    r_bg = 0.0
    if with_bg:
        t32 = (F32(1) - ws_np).astype(np.float64)[:, None]
        want_bg = g_np.astype(np.float64) * t32
        r_bg = float((np.abs(grads[2].cpu().numpy() - want_bg) / (U * np.abs(want_bg))).max())
    print(f"\nparity: plain mix N={N} bg={'tensor' if with_bg else 'white'}: worst error / bound: "
          f"image {r_img:.3f} grad_ws {r_ws:.3f} grad_bg {r_bg:.3f}")
    assert r_img <= 1.0 and r_ws <= 1.0 and r_bg <= 1.0


# ---------------------------------------------------------------- d. entropy

def _entropy_ws(N, seed=0):
    rng = np.random.default_rng(seed + N)
    ws = rng.uniform(0.0, 1.0, N).astype(F32)
    k = min(N, len(SPECIAL))
    ws[:k] = SPECIAL[:k]
    return ws


# 1023 / 1025: one element per thread of the 1024-thread block, and one more;
# 7169: the first N at which thread 0 takes the eight-wide loop (7 * 1024 < N);
# 8193: eight-wide once and one tail element; 16384: eight-wide twice
@pytest.mark.parametrize("N", [1, 1023, 1025, 7169, 8193, 16384])
def test_entropy_matches_oracle(gpu, N):
    """lambda * mean(entropy(clamp(ws))) and its gradient (nerf.head.ray_entropy)
    against oracle.field.entropy.

    Loss, per element with t1 = a log2 a, t2 = (1 - a) log2(1 - a) (both < 0,
    the term is |t1| + |t2|), float32 with log2f at 1 ulp = 2u (HIP math API):
      t1: log2f 2u, the product u                         3u |t1|
      t2: 1 - a rounds (u), which moves the factor (u |t2|) and the
          logarithm by u / ln 2 absolutely; log2f 2u, the product u:
                                              4u |t2| + 1.4427 u (1 - a)
      -t1 - t2: one rounding                              u (|t1| + |t2|)
    then a double sum (exact at this size), the division by N, one cast and the
    product with lambda: 2u of the mean.  In all at most
    7u mean(|t1| + |t2|) + 1.4427 u mean(1 - a); twice that is allowed.  (The
    second part is no multiple of the term: at a = 1e-5 the rounding of 1 - a
    alone moves t2 by 3e-3 of itself.)
    Gradient: zero exactly where the oracle's is (the clamp's mask; 0.5, whose
    gradient is 0 inside the mask, is checked by value); values within
    |g lambda / N| 1e-5 (|log2 a| + |log2(1 - a)|), the form and constant
    test_gpu_step_structures.py uses for this term."""
    from nerf import head as _head
    lam = float(F32(1e-3))
    up = 3.0
    ws_np = _entropy_ws(N)
    ws = torch.from_numpy(ws_np).to(gpu).requires_grad_()
    loss = _head.ray_entropy(ws, lam)
    (grad,) = torch.autograd.grad(loss, ws, torch.tensor(up, device=gpu))
    want_loss, want_g = of.entropy(ws_np, lam)
    a = np.clip(ws_np.astype(np.float64), float(LO), float(HI))
    t1, t2 = np.abs(a * np.log2(a)), np.abs((1 - a) * np.log2(1 - a))
    bound = 2 * lam * U * (7 * (t1 + t2).mean() + 1.4427 * (1 - a).mean())
    r_loss = abs(float(loss.detach()) - want_loss) / bound
    got = grad.cpu().numpy().astype(np.float64)
    want_g = want_g * up
    inside = (ws_np >= LO) & (ws_np <= HI)
    zero = got == 0
    ok = ws_np != F32(0.5)
    assert np.array_equal(zero[ok], ~inside[ok]), "gradient mask differs from the clamp's"
    assert np.array_equal(want_g[ok] == 0, ~inside[ok])
    gb = abs(up * lam / N) * 1e-5 * (np.abs(np.log2(a)) + np.abs(np.log2(1 - a)))
    r_g = float((np.abs(got - want_g) / gb).max())
    print(f"\nparity: entropy N={N}: worst error / bound: loss {r_loss:.3f} gradient {r_g:.3f}")
    assert r_loss <= 1.0 and r_g <= 1.0


@pytest.mark.parametrize("N", [1, 1025])
def test_entropy_backward_overwrites_and_accumulates(gpu, N):
    import _dfhip
    from _dfhip import ptr
    lam = float(F32(1e-3))
    ws = torch.from_numpy(_entropy_ws(N)).to(gpu)
    up = torch.tensor([3.0], device=gpu)
    plain = torch.full((N,), float("nan"), device=gpu)
    _dfhip.call("dfhip_entropy_backward", N, ptr(ws), ptr(up), lam, ptr(plain), _dfhip.stream())
    assert torch.isfinite(plain).all()
    pre = torch.from_numpy(np.random.default_rng(N).standard_normal(N).astype(F32) * 1e-6).to(gpu)
    acc = pre.clone()
    _dfhip.call("dfhip_entropy_backward_accumulate", N, ptr(ws), ptr(up), lam, ptr(acc),
                _dfhip.stream())
    p64, v64 = pre.cpu().numpy().astype(np.float64), plain.cpu().numpy().astype(np.float64)
    larger = np.maximum(np.abs(p64), np.abs(v64)).astype(F32)
    assert np.all(np.abs(acc.cpu().numpy() - (p64 + v64)) <= np.spacing(larger))
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits((pre + plain).cpu().numpy()))


def test_entropy_of_no_rays(gpu):
    """N = 0: the loss is NaN, as torch.mean of an empty tensor is; no
    gradient element is written."""
    import _dfhip
    from _dfhip import ptr
    ws = torch.full((4,), 0.5, device=gpu)
    loss = torch.zeros((), device=gpu)
    _dfhip.call("dfhip_entropy_forward", 0, ptr(ws), 1e-3, ptr(loss), _dfhip.stream())
    assert torch.isnan(loss) and torch.isnan(torch.empty(0).mean())
    grad = torch.full((4,), 7.0, device=gpu)
    up = torch.ones(1, device=gpu)
    for name in ("dfhip_entropy_backward", "dfhip_entropy_backward_accumulate"):
        _dfhip.call(name, 0, ptr(ws), ptr(up), 1e-3, ptr(grad), _dfhip.stream())
    assert (grad == 7.0).all() and (ws == 0.5).all()


# ---------------------------------------------------------------- e. fused entries

class _Head:
    """Device buffers of one head call through the C ABI."""

    def __init__(self, gpu, N, seed):
        import _dfhip
        inp = ray_head_inputs(N, seed)
        k = min(N, len(SPECIAL))
        inp["ws"][:k] = torch.from_numpy(SPECIAL[:k])
        self.N = N
        self.inp = {k_: v.to(gpu).contiguous() for k_, v in inp.items()}
        l1, l2 = _net(gpu)
        self.w = [t.detach().float().contiguous() for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
        self.up = torch.tensor([65536.0], device=gpu)
        self.lam = float(F32(1e-3))
        self.parts = int(_dfhip.load().dfhip_ray_head_partial_floats(N))
        self.gpu = gpu

    def outputs(self):
        """Fresh NaN-filled gradient outputs: grad_image, grad_ws, partial, gw1, gb1, gw2, gb2."""
        nan = lambda *s: torch.full(s, float("nan"), device=self.gpu)  # noqa: E731
        return [nan(self.N, 3), nan(self.N), nan(self.parts)] + [nan(*w.shape) for w in self.w]

    def fwd_outputs(self):
        return [torch.full((3, self.N), float("nan"), device=self.gpu),
                torch.full((self.N,), float("nan"), device=self.gpu),
                torch.full((self.N,), 9, dtype=torch.uint8, device=self.gpu)]

    def backward_args(self, o):
        from _dfhip import ptr
        i = self.inp
        return [self.N, ptr(i["gimg"]), ptr(i["ws"]), ptr(i["d"]), *[ptr(w) for w in self.w], None,
                ptr(o[0]), ptr(o[1]), None, ptr(o[2]), *[ptr(g) for g in o[3:]]]


def _same(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert not np.isnan(x).any(), f"{what}: output {k} not fully written"
        assert np.array_equal(_bits(x), _bits(y)), f"{what}: output {k} differs"


@pytest.mark.parametrize("N", [65, 15983])
def test_fused_head_entries_equal_their_parts(gpu, N):
    """head.hip documents the fused entries as giving their parts' values bit
    for bit; the native step's equality tests rest on it."""
    import _dfhip
    from _dfhip import ptr
    h = _Head(gpu, N, 11)
    i, st = h.inp, _dfhip.stream()
    # the parts
    parts = h.outputs()
    _dfhip.call("dfhip_ray_head_backward", *h.backward_args(parts), st)
    _dfhip.call("dfhip_entropy_backward_accumulate", N, ptr(i["ws"]), ptr(h.up), h.lam,
                ptr(parts[1]), st)
    loss = torch.full((), float("nan"), device=gpu)
    _dfhip.call("dfhip_entropy_forward", N, ptr(i["ws"]), h.lam, ptr(loss), st)
    fwd = h.fwd_outputs()
    _dfhip.call("dfhip_ray_head_forward", N, ptr(i["ws"]), ptr(i["depth"]), ptr(i["image"]),
                ptr(i["d"]), ptr(i["nears"]), ptr(i["fars"]), *[ptr(w) for w in h.w], None,
                *[ptr(t) for t in fwd], st)
    assert torch.isfinite(loss)
    grads = lambda o: [o[0], o[1]] + o[3:]  # noqa: E731 - all but the partials' scratch
    # backward + entropy gradient
    a = h.outputs()
    _dfhip.call("dfhip_ray_head_backward_entropy", *h.backward_args(a), ptr(h.up), h.lam, st)
    _same(grads(a), grads(parts), "backward_entropy")
    # ... + loss
    b, loss_b = h.outputs(), torch.full((), float("nan"), device=gpu)
    _dfhip.call("dfhip_ray_head_backward_entropy_loss", *h.backward_args(b), ptr(h.up), h.lam,
                ptr(loss_b), st)
    _same(grads(b), grads(parts), "backward_entropy_loss")
    _same([loss_b], [loss], "backward_entropy_loss: loss")
    # forward + backward + entropy gradient + loss
    c, fwd_c, loss_c = h.outputs(), h.fwd_outputs(), torch.full((), float("nan"), device=gpu)
    _dfhip.call("dfhip_ray_head_forward_backward_entropy_loss", N, ptr(i["ws"]), ptr(i["depth"]),
                ptr(i["image"]), ptr(i["d"]), ptr(i["nears"]), ptr(i["fars"]),
                *[ptr(w) for w in h.w], *[ptr(t) for t in fwd_c], ptr(i["gimg"]), ptr(c[0]),
                ptr(c[1]), ptr(c[2]), *[ptr(g) for g in c[3:]], ptr(h.up), h.lam, ptr(loss_c), st)
    _same(grads(c), grads(parts), "forward_backward_entropy_loss")
    _same([loss_c], [loss], "forward_backward_entropy_loss: loss")
    for k, (x, y) in enumerate(zip(fwd_c, fwd)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy())), f"forward output {k}"
    assert set(np.unique(fwd[2].cpu().numpy())) <= {0, 1}


def test_fused_head_entries_of_no_rays(gpu):
    """N = 0: the two loss-writing entries write dfhip_entropy_forward's value."""
    import _dfhip
    from _dfhip import ptr
    ws = torch.full((4,), 0.5, device=gpu)
    up = torch.ones(1, device=gpu)
    st = _dfhip.stream()
    want = torch.zeros((), device=gpu)
    _dfhip.call("dfhip_entropy_forward", 0, ptr(ws), 1e-3, ptr(want), st)
    a, b = torch.zeros((), device=gpu), torch.zeros((), device=gpu)
    _dfhip.call("dfhip_ray_head_backward_entropy_loss", 0, None, ptr(ws), *[None] * 14, ptr(up),
                1e-3, ptr(a), st)
    _dfhip.call("dfhip_ray_head_forward_backward_entropy_loss", 0, ptr(ws), *[None] * 20, ptr(up),
                1e-3, ptr(b), st)
    assert torch.isnan(want)
    for got in (a, b):
        assert np.array_equal(_bits(got.cpu().numpy().reshape(1)), _bits(want.cpu().numpy().reshape(1)))
