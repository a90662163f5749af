"""Train and inference compositing against the float64 truth of
tests/composite_cases.py at the edges of the 16-sample window: every entry of
csrc/raymarching.hip that composites (dfhip_composite_rays_train_forward,
_backward, _backward_dense, _forward_mixed, _backward_mixed,
dfhip_composite_rays), the raymarching.composite_rays_train autograd function
on its memset-plus-reference-form route, and the compositing halves of the
fused chain (dfhip_ray_chain_train, csrc/head.hip), which run the same
chain_common.h code.

With r the truth, t the f32 C oracle and y the kernel (composite_cases.check_bounds):

    per tensor and case   |y - r|_2 / |r|_2 <= 3 |t - r|_2 / |r|_2 + 1e-6
    per element           |y - r| <= 1e-4 |r| + a
                          a = 1e-6 (weights_sum, image, grad_rgb), 1e-5 (depth, grad_sigma)

the constants of tests/test_gpu_raymarching.py (upstream gradients from
N(0, 1), dt <= 0.03).  A result stored as f16 gains 2^-10 |r| + 2^-24 (one
rounding, doubled; bf16 colour gradients 2^-7 |r|), with truth and oracle
computed on the rounded inputs and the oracle's result rounded to the stored
type; f64 entries keep the f32 bounds (the kernels take __expf in f32).
tests/test_composite_cases_host.py shows on the CPU that every break decision of
the cases has a factor 2 to spare and that the oracle alone meets a third of
these bounds.

Exact (sentinel-filled buffers): rows past M and rows a backward does not own
are untouched, skipped rays write 0, the dense backward writes 0 past a break,
over the clipped rows of a ray past the capacity and (zero_tail) over
[total, M); at T_thresh 0 the samples behind an opaque one get a colour
gradient of exactly 0; the NaN ray's NaN pattern is the truth's.  The tests
print `edges:` lines for the 70-ray cases (kept in profiles/composite/edges.txt).
"""
import numpy as np
import pytest
import torch

import composite_cases as cc

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f16": torch.float16, "f64": torch.float64,
         "bf16": torch.bfloat16}
LAM = 1e-3


def _dev(gpu, a, elem):
    """A float64 array of values already rounded to `elem`, on the device."""
    return torch.tensor(np.ascontiguousarray(a), dtype=TORCH[elem], device=gpu)


def _sent(gpu, elem, *shape):
    return torch.full(shape, cc.SENT, dtype=TORCH[elem], device=gpu)


def _np(t):
    return t.double().cpu().numpy()


def _tag(c, T_thresh, what):
    return f"[{what} N {c.N} {c.layout} {c.order} T {T_thresh:g}]"


def _say(line):
    print("\n" + line, end="")


def _log(c):
    return _say if c.N == 70 else None


class _Train:
    """Device operands of one case at one element type pair."""

    def __init__(self, gpu, c, elem, rgb_elem=None):
        self.c, self.gpu, self.elem = c, gpu, elem
        self.ce = elem if rgb_elem is None else rgb_elem
        sg, cl, dl, gw, gi = c.inputs(elem, self.ce)
        self.sigma, self.rgbs = _dev(gpu, sg, elem), _dev(gpu, cl, self.ce)
        self.deltas = _dev(gpu, dl, elem)
        self.g_ws, self.g_image = _dev(gpu, gw, elem), _dev(gpu, gi, elem)
        self.rays = torch.from_numpy(c.rays).to(gpu)

    def forward_outputs(self):
        """ws, depth, image with PAD rows of slack past N."""
        n = self.c.N + cc.PAD
        return (_sent(self.gpu, self.elem, n), _sent(self.gpu, self.elem, n),
                _sent(self.gpu, self.elem, n, 3))

    def grad_outputs(self):
        c = self.c
        return _sent(self.gpu, self.elem, c.rows), _sent(self.gpu, self.ce, c.rows, 3)


def _check_forward(c, ref, T_thresh, what, ws, depth, image):
    """Bounds of the three per-ray outputs; zeros of the skipped rays."""
    tag, t, o = _tag(c, T_thresh, what), ref["truth"], ref["oracle"]
    skipped = torch.from_numpy(c.rays[ref["taken"] == 0, 0].astype(np.int64))
    for name, y in (("ws", ws), ("depth", depth), ("image", image)):
        y = y.cpu()
        assert bool((y[c.N:] == cc.SENT).all()), f"{tag} {name}: rows past N were written"
        y = y[:c.N]
        assert bool((y[skipped] == 0).all()), f"{tag} {name}: a skipped ray did not write 0"
        cc.check_bounds(name, _np(y), t[name], o[name], ref["elem"], tag=tag, log=_log(c))
    _nan_neighbours_finite(c, ws[:c.N].cpu(), image[:c.N].cpu(), tag)


def _nan_neighbours_finite(c, ws, image, tag):
    row = c.row_of(cc.NAN_RAY)
    if row is None:
        return
    assert bool(torch.isnan(ws[int(c.rays[row, 0])]))
    for ray in cc.WAVE_OF_NAN:
        index = int(c.rays[c.row_of(ray), 0])
        assert bool(torch.isfinite(ws[index])) and bool(torch.isfinite(image[index]).all()), \
            f"{tag}: ray {ray}, in the NaN ray's wave, is not finite"


def _check_backward(c, ref, T_thresh, what, gs, gc, mode, zero_tail=True):
    """mode "reference": rows the backward does not own keep the sentinel;
    "dense": they are exactly 0 up to min(total, M), and [total, M) is 0 with
    zero_tail and untouched without; "memset": 0 everywhere unowned below M."""
    tag, t, o = _tag(c, T_thresh, what), ref["truth"], ref["oracle"]
    gs, gc = gs.cpu(), gc.cpu()
    owned = torch.from_numpy(ref["owned"])
    M, total = c.M, min(c.total, c.M)
    rows = torch.arange(c.rows)
    for name, y in (("grad_sigma", gs), ("grad_rgb", gc)):
        y2 = y.reshape(c.rows, -1)
        assert bool((y2[M:] == cc.SENT).all()), f"{tag} {name}: rows past M were written"
        assert not bool((y2[owned] == cc.SENT).any()), f"{tag} {name}: a taken row was not written"
        free = ~owned & (rows < M)
        if mode == "reference":
            assert bool((y2[free] == cc.SENT).all()), \
                f"{tag} {name}: a row the reference-form backward does not own was written"
        else:
            inside = free & (rows < total)
            bad = torch.nonzero(~(y2[inside] == 0).all(1)).flatten()
            assert bad.numel() == 0, (f"{tag} {name}: rows past a break or clipped rows are not "
                                      f"0: {rows[inside][bad][:6].tolist()}")
            tail = y2[total:M]
            want = 0.0 if (zero_tail or mode == "memset") else cc.SENT
            assert bool((tail == want).all()), f"{tag} {name}: rows [total, M) are not {want}"
    own = ref["owned"]
    cc.check_bounds("grad_sigma", _np(gs)[own], t["grad_sigma"][own], o["grad_sigma"][own],
                    ref["elem"], tag=tag, log=_log(c))
    cc.check_bounds("grad_rgb", _np(gc)[own], t["grad_rgb"][own], o["grad_rgb"][own],
                    ref["rgb_elem"], tag=tag, log=_log(c))
    if T_thresh == 0.0:   # behind an opaque sample T is exactly 0
        for ray, (num, at) in cc._OPAQUE.items():
            row = c.row_of(ray)
            if row is None or ref["taken"][row] == 0:
                continue
            off = int(c.rays[row, 1])
            assert bool((gc[off + at + 1:off + num] == 0).all()), \
                f"{tag}: colour gradient behind the opaque sample of ray {ray} is not exactly 0"
            assert bool((gc[off + at] != 0).any())


# ---------------------------------------------------------------- generic entries

@pytest.mark.parametrize("elem", ["f32", "f16", "f64"])
@pytest.mark.parametrize("order,layout", [("ordered", "B"), ("scattered", "T")])
@pytest.mark.parametrize("N", cc.RAY_COUNTS)
def test_train_forward_and_reference_form_backward(gpu, N, order, layout, elem):
    import _raymarching
    c = cc.train_case(N, layout, order)
    b = _Train(gpu, c, elem)
    for T_thresh in cc.T_THRESH:
        ref = cc.train_reference(c, T_thresh, elem)
        ws, depth, image = b.forward_outputs()
        _raymarching.composite_rays_train_forward(b.sigma, b.rgbs, b.deltas, b.rays, c.M, N,
                                                  T_thresh, ws, depth, image)
        _check_forward(c, ref, T_thresh, f"forward {elem}", ws, depth, image)
        gs, gc = b.grad_outputs()
        _raymarching.composite_rays_train_backward(
            b.g_ws, b.g_image, b.sigma, b.rgbs, b.deltas, b.rays, _dev(gpu, ref["ws_in"], elem),
            _dev(gpu, ref["image_in"], elem), c.M, N, T_thresh, gs, gc)
        _check_backward(c, ref, T_thresh, f"backward {elem}", gs, gc, "reference")


DENSE_CASES = [(70, "A"), (70, "B"), (70, "T"), (17, "A"), (1, "B"), (15, "B"), (16, "B"),
               (17, "B")]


@pytest.mark.parametrize("elem", ["f32", "f64"])
@pytest.mark.parametrize("N,layout", DENSE_CASES)
def test_train_backward_dense(gpu, N, layout, elem):
    import _raymarching
    c = cc.train_case(N, layout, "ordered")
    b = _Train(gpu, c, elem)
    for T_thresh in cc.T_THRESH:
        ref = cc.train_reference(c, T_thresh, elem)
        gs, gc = b.grad_outputs()
        _raymarching.composite_rays_train_backward_dense(
            b.g_ws, b.g_image, b.sigma, b.rgbs, b.deltas, b.rays, _dev(gpu, ref["ws_in"], elem),
            _dev(gpu, ref["image_in"], elem), c.M, N, T_thresh, gs, gc)
        _check_backward(c, ref, T_thresh, f"dense {elem}", gs, gc, "dense")


@pytest.mark.parametrize("zero_tail", [0, 1])
@pytest.mark.parametrize("rgb_elem", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("N,layout", DENSE_CASES)
def test_train_mixed_entries(gpu, N, layout, rgb_elem, zero_tail):
    import _raymarching
    c = cc.train_case(N, layout, "ordered")
    b = _Train(gpu, c, "f32", rgb_elem)
    for T_thresh in cc.T_THRESH:
        ref = cc.train_reference(c, T_thresh, "f32", rgb_elem)
        what = f"mixed {rgb_elem} tail {zero_tail}"
        ws, depth, image = b.forward_outputs()
        _raymarching.composite_rays_train_forward_mixed(b.sigma, b.rgbs, b.deltas, b.rays, c.M, N,
                                                        T_thresh, ws, depth, image)
        _check_forward(c, ref, T_thresh, what, ws, depth, image)
        gs, gc = b.grad_outputs()
        _raymarching.composite_rays_train_backward_mixed(
            b.g_ws, b.g_image, b.sigma, b.rgbs, b.deltas, b.rays, _dev(gpu, ref["ws_in"], "f32"),
            _dev(gpu, ref["image_in"], "f32"), c.M, N, T_thresh, gs, gc, bool(zero_tail))
        _check_backward(c, ref, T_thresh, what, gs, gc, "dense", zero_tail=bool(zero_tail))


@pytest.mark.parametrize("T_thresh", cc.T_THRESH)
def test_autograd_function_on_scattered_rays(gpu, T_thresh):
    """raymarching.composite_rays_train without the ordered attribute: the
    generic forward, then a memset and the reference-form backward."""
    import raymarching
    c = cc.train_case(70, "T", "scattered")
    b = _Train(gpu, c, "f32")
    ref = cc.train_reference(c, T_thresh, "f32")
    s = b.sigma[:c.M].clone().requires_grad_(True)
    col = b.rgbs[:c.M].clone().requires_grad_(True)
    ws, depth, image = raymarching.composite_rays_train(s, col, b.deltas[:c.M].contiguous(),
                                                        b.rays, T_thresh)
    _check_forward(c, ref, T_thresh, "autograd", ws.detach(), depth.detach(), image.detach())
    # the NaN ray makes the sum NaN; the upstream gradients are g all the same
    ((ws * b.g_ws).sum() + (image * b.g_image).sum()).backward()
    pad = lambda g, *tail: torch.cat([g, _sent(gpu, "f32", cc.PAD, *tail)])  # noqa: E731
    # the backward reads the forward's own ws / image: f32 roundings of the
    # truth's, like the operands the reference was computed on
    _check_backward(c, ref, T_thresh, "autograd", pad(s.grad), pad(col.grad, 3), "memset")


# ---------------------------------------------------------------- the fused chain

@pytest.mark.parametrize("rgb_elem", ["f16", "bf16"])
def test_ray_chain_compositing_halves(gpu, rgb_elem):
    """dfhip_ray_chain_train on the ordered layout A: ws / depth / image
    against the truth, grad_sigma / grad_rgb against the truth's backward of
    the grad_ws / grad_image (and ws / image) the chain itself wrote."""
    import _dfhip
    import oracle
    from _dfhip import call, ptr, stream
    c = cc.train_case(70, "A", "ordered")
    N, M = c.N, c.M
    b = _Train(gpu, c, "f32", rgb_elem)
    gen = torch.Generator(device="cpu").manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    d = r(N, 3)
    d = (d / d.norm(dim=1, keepdim=True)).to(gpu)
    nears, fars = torch.full((N,), 0.2, device=gpu), torch.full((N,), 2.0, device=gpu)
    w = [(r(64, 39) * 0.2).to(gpu), (r(64) * 0.1).to(gpu), (r(3, 64) * 0.2).to(gpu),
         (r(3) * 0.1).to(gpu)]
    g_image = b.g_image.t().contiguous()   # [3, N], N(0, 1)
    scale = torch.full((1,), 1.0, device=gpu)
    sg, cl, dl, _, _ = c.inputs("f32", rgb_elem)
    f = lambda a: a[:M].astype(np.float32)  # noqa: E731
    for T_thresh in cc.T_THRESH:
        ref = cc.train_reference(c, T_thresh, "f32", rgb_elem)
        ws, depth, image = b.forward_outputs()
        gs, gc = b.grad_outputs()
        s32 = lambda *s: _sent(gpu, "f32", *s)  # noqa: E731
        out_image, out_depth, grad_image, grad_ws = s32(3, N), s32(N), s32(N, 3), s32(N)
        mask = torch.full((N,), 77, dtype=torch.uint8, device=gpu)
        partial = s32(int(_dfhip.load().dfhip_ray_head_partial_floats(N)))
        grads = [torch.full_like(x, cc.SENT) for x in w]
        loss, found_inf = s32(), torch.zeros(1, device=gpu)
        call("dfhip_ray_chain_train", _dfhip._DTYPE[TORCH[rgb_elem]], ptr(b.sigma), ptr(b.rgbs),
             ptr(b.deltas), ptr(b.rays), M, N, T_thresh, ptr(ws), ptr(depth), ptr(image), ptr(d),
             ptr(nears), ptr(fars), *[ptr(x) for x in w], ptr(out_image), ptr(out_depth),
             ptr(mask), ptr(g_image), ptr(grad_image), ptr(grad_ws), ptr(partial),
             *[ptr(x) for x in grads], ptr(scale), LAM, ptr(loss), ptr(found_inf), 0,
             ptr(gs), ptr(gc), stream())
        torch.cuda.synchronize()
        what = f"chain {rgb_elem}"
        _check_forward(c, ref, T_thresh, what, ws, depth, image)
        assert torch.equal(grad_image, b.g_image)
        gw, gi = _np(grad_ws), _np(grad_image)
        fin = np.isfinite(gw)
        assert np.abs(gw[fin]).max() < 8.0   # the floors assume upstream gradients of order 1
        ws, image = ws[:N], image[:N]
        tb = cc.train_truth_backward(gw, gi, sg, cl, dl, c.rays, M, T_thresh, _np(ws), _np(image))
        o_gs, o_gc = oracle.composite_rays_train_backward(
            gw.astype(np.float32), gi.astype(np.float32), f(sg), f(cl), f(dl), c.rays,
            ws.cpu().numpy(), image.cpu().numpy(), T_thresh)
        zs = lambda a: np.concatenate([a, np.zeros((cc.PAD,) + a.shape[1:], a.dtype)])  # noqa: E731
        mine = dict(ref, owned=tb["owned"],
                    truth=dict(grad_sigma=tb["grad_sigma"], grad_rgb=tb["grad_rgb"]),
                    oracle=dict(grad_sigma=zs(o_gs).astype(np.float64),
                                grad_rgb=cc.round_to(zs(o_gc), rgb_elem)))
        assert np.array_equal(tb["taken"], ref["taken"])
        _check_backward(c, mine, T_thresh, what, gs, gc, "dense", zero_tail=False)


# ---------------------------------------------------------------- inference

@pytest.mark.parametrize("elem", ["f32", "f16", "f64"])
@pytest.mark.parametrize("n_step", cc.INFER_STEPS)
@pytest.mark.parametrize("n_alive", cc.INFER_ALIVE)
def test_composite_infer(gpu, n_alive, n_step, elem):
    import _raymarching
    c = cc.infer_case(n_alive, n_step)
    rt, sg, cl, dl, ws0, dp0, im0 = c.inputs(elem)
    for T_thresh in cc.INFER_THRESH:
        ref = cc.infer_reference(c, T_thresh, elem)
        t, o = ref["truth"], ref["oracle"]
        tag = f"[infer {elem} {n_alive} x {n_step} T {T_thresh:g}]"
        alive = torch.from_numpy(c.rays_alive.copy()).to(gpu)
        rays_t, ws, depth, image = (_dev(gpu, a, elem) for a in (rt, ws0, dp0, im0))
        before = [x.clone() for x in (rays_t, ws, depth, image)]
        _raymarching.composite_rays(n_alive, n_step, T_thresh, alive, rays_t, _dev(gpu, sg, elem),
                                    _dev(gpu, cl, elem), _dev(gpu, dl, elem), ws, depth, image)
        torch.cuda.synchronize()
        got_alive = alive.cpu().numpy()
        assert np.array_equal(got_alive, t["rays_alive"]), (tag, got_alive, t["rays_alive"])
        listed = torch.from_numpy(c.rays_alive[:n_alive].astype(np.int64)).to(gpu)
        retired = listed[torch.from_numpy(t["rays_alive"][:n_alive] < 0).to(gpu)]
        assert torch.equal(rays_t[retired], before[0][retired]), f"{tag}: rays_t of a retired ray"
        others = torch.ones(c.n_rays, dtype=torch.bool, device=gpu)
        others[listed] = False
        for x, x0 in zip((rays_t, ws, depth, image), before):
            assert torch.equal(x[others], x0[others]), f"{tag}: a ray that is not listed changed"
        log = _say if n_alive == 65 else None
        for name, y in (("ws", ws), ("depth", depth), ("image", image), ("rays_t", rays_t)):
            cc.check_bounds(name, _np(y), t[name], o[name], elem, tag=tag, log=log)
