"""GPU tests of the fused per-ray chain (dfhip_ray_chain_train): compositing
forward, ray head and compositing backward as one launch.  Every comparison is
exact (torch.equal) against the three entries it replaces, run on the same
inputs into sentinel-filled buffers:

    dfhip_composite_rays_train_forward_mixed
    dfhip_ray_head_forward_backward_entropy_loss_check
    dfhip_composite_rays_train_backward_mixed (zero_tail = 0)

* the kernel on 70 rays (two workgroups, the second with 6 live rays) whose
  sample counts sit around multiples of the 16-sample window, with rays that
  break early, at a window's last sample and deep into a long ray, and a last
  ray past the capacity;
* the whole graph-replayed step with Trainer.fused_ray_chain on against off.

The entry has no per-call options: the two that were built (loading a window
ahead; keeping six windows' backward state on chip) passed these same
comparisons off and on, measured within the run-to-run spread and were
removed.  The counts around 96 samples are the boundary
the second of them had.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 70
LAM = 1e-3


def _case(gpu, dtype):
    """Inputs of the 70-ray case (built once per colour dtype)."""
    K = 6  # sample counts around the sixth window as well as the first two
    gen = torch.Generator(device="cpu").manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    u = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    special = [0, 1, 15, 16, 17, 31, 32, 33, 16 * K - 1, 16 * K, 16 * K + 1, 16 * K + 17, 300]
    # (count, sample whose density ends the ray): after 5 samples; exactly at a
    # window's last sample; at the sixth window's last sample; inside the seventh
    breaks = [(40, 4), (40, 15), (16 * K + 24, 16 * K - 1), (16 * K + 34, 16 * K + 4)]
    counts = special + [c for c, _ in breaks]
    counts += [int(v) for v in torch.randint(0, 41, (N - 1 - len(counts),), generator=gen)]
    counts.append(20)  # the final ray: past the capacity
    assert len(counts) == N
    num = torch.tensor(counts, dtype=torch.int64)
    off = torch.cumsum(num, 0) - num
    M = int(off[-1]) + 7  # offset + num > M for the final ray only
    rows = M + 16         # rows past M must stay untouched
    rays = torch.stack([torch.arange(N), off, num], 1).to(torch.int32)
    # sigma * delta ~ 0.02: a 300-sample ray keeps T > 1e-4
    sigma = u(rows) * 2.0
    deltas = torch.stack([0.01 + 0.02 * u(rows), 0.01 + 0.02 * u(rows)], 1)
    for k, (_, at) in enumerate(breaks):
        o = int(off[len(special) + k])
        if k == 0:  # five dense samples: T = e^-8 after four, e^-10 < 1e-4 after five
            sigma[o:o + 5], deltas[o:o + 5, 0] = 100.0, 0.02
        else:       # empty space, then one opaque sample
            sigma[o:o + at], sigma[o + at] = 0.0, 1e6
    # the reference loop must break where the case says it does
    for k, (c, at) in enumerate(breaks):
        o = int(off[len(special) + k])
        T = torch.cumprod(torch.exp(-sigma[o:o + c].double() * deltas[o:o + c, 0].double()), 0)
        assert float(T[at]) < 1e-4 and (at == 0 or float(T[at - 1]) >= 1e-4)
    rgbs = u(rows, 3).to(dtype)
    d = r(N, 3)
    d = d / d.norm(dim=1, keepdim=True)
    nears, fars = torch.full((N,), 0.2), torch.full((N,), 2.0)
    nears[3], fars[3] = 1.5, 1.0  # a ray that misses the box: mask 0
    w = [r(64, 39) * 0.2, r(64) * 0.1, r(3, 64) * 0.2, r(3) * 0.1]
    g_image = r(3, N) * 0.1
    t = lambda x: x.to(gpu)  # noqa: E731
    return dict(M=M, rows=rows, rays=t(rays), sigma=t(sigma), deltas=t(deltas), rgbs=t(rgbs),
                d=t(d), nears=t(nears), fars=t(fars), w=[t(x) for x in w], g_image=t(g_image),
                scale=torch.full((1,), 512.0, device=gpu), dtype=dtype, off=off, num=num)


def _buffers(c, gpu):
    """Every output of the chain, sentinel-filled."""
    import _dfhip
    f = lambda *s: torch.full(s, -7.0, device=gpu)  # noqa: E731
    return dict(
        ws=f(N), depth=f(N), image=f(N, 3), out_image=f(3, N), out_depth=f(N),
        mask=torch.full((N,), 77, dtype=torch.uint8, device=gpu), grad_image=f(N, 3),
        grad_ws=f(N), partial=f(int(_dfhip.load().dfhip_ray_head_partial_floats(N))),
        grads=[torch.full_like(x, -7.0) for x in c["w"]], loss=f(),
        found_inf=torch.zeros(1, device=gpu), grad_sigma=f(c["rows"]),
        grad_rgb=torch.full((c["rows"], 3), -7.0, dtype=c["dtype"], device=gpu))


def _three_launches(c, gpu, defer):
    import _raymarching
    from _dfhip import call, ptr, stream
    b = _buffers(c, gpu)
    _raymarching.composite_rays_train_forward_mixed(
        c["sigma"], c["rgbs"], c["deltas"], c["rays"], c["M"], N, 1e-4, b["ws"], b["depth"],
        b["image"])
    call("dfhip_ray_head_forward_backward_entropy_loss_check", N, ptr(b["ws"]), ptr(b["depth"]),
         ptr(b["image"]), ptr(c["d"]), ptr(c["nears"]), ptr(c["fars"]),
         *[ptr(x) for x in c["w"]], ptr(b["out_image"]), ptr(b["out_depth"]), ptr(b["mask"]),
         ptr(c["g_image"]), ptr(b["grad_image"]), ptr(b["grad_ws"]), ptr(b["partial"]),
         *[ptr(x) for x in b["grads"]], ptr(c["scale"]), LAM, ptr(b["loss"]),
         ptr(b["found_inf"]), int(defer), stream())
    _raymarching.composite_rays_train_backward_mixed(
        b["grad_ws"], b["grad_image"], c["sigma"], c["rgbs"], c["deltas"], c["rays"], b["ws"],
        b["image"], c["M"], N, 1e-4, b["grad_sigma"], b["grad_rgb"], False)
    torch.cuda.synchronize()
    return b


def _one_launch(c, gpu, defer):
    import _dfhip
    from _dfhip import call, ptr, stream
    b = _buffers(c, gpu)
    call("dfhip_ray_chain_train", _dfhip._DTYPE[c["dtype"]], ptr(c["sigma"]), ptr(c["rgbs"]),
         ptr(c["deltas"]), ptr(c["rays"]), c["M"], N, 1e-4, ptr(b["ws"]), ptr(b["depth"]),
         ptr(b["image"]), ptr(c["d"]), ptr(c["nears"]), ptr(c["fars"]),
         *[ptr(x) for x in c["w"]], ptr(b["out_image"]), ptr(b["out_depth"]), ptr(b["mask"]),
         ptr(c["g_image"]), ptr(b["grad_image"]), ptr(b["grad_ws"]), ptr(b["partial"]),
         *[ptr(x) for x in b["grads"]], ptr(c["scale"]), LAM, ptr(b["loss"]),
         ptr(b["found_inf"]), int(defer), ptr(b["grad_sigma"]), ptr(b["grad_rgb"]), stream())
    torch.cuda.synchronize()
    return b


_CACHE = {}


def _reference(gpu, dtype, defer):
    """The case and the three launches' outputs, computed once and shared."""
    if dtype not in _CACHE:
        _CACHE[dtype] = _case(gpu, dtype)
    key = (dtype, defer)
    if key not in _CACHE:
        _CACHE[key] = _three_launches(_CACHE[dtype], gpu, defer)
    return _CACHE[dtype], _CACHE[key]


def test_reference_case_is_what_it_claims(gpu):
    """The three launches on the case: finite everywhere, the sentinel left in
    the rows past M, zeros in the rows the dense fill owns (past each break and
    the clipped rows of the skipped final ray), gradients in the rows taken."""
    c, want = _reference(gpu, torch.float16, 0)
    gs, off, num = want["grad_sigma"].cpu(), c["off"], c["num"]
    assert bool((gs[c["M"]:] == -7.0).all()) and not bool((gs[:c["M"]] == -7.0).any())
    assert bool((gs[int(off[-1]):c["M"]] == 0.0).all())           # final ray: skipped, clipped
    assert float(want["ws"][-1]) == 0.0
    gc = want["grad_rgb"].float().cpu()
    o, e = int(off[13]), int(off[13] + num[13])                    # breaks after 5 samples
    assert bool((gc[o:o + 5] != 0.0).all()) and bool((gc[o + 5:e] == 0.0).all())
    assert bool((gs[o + 5:e] == 0.0).all())
    o, e = int(off[14]), int(off[14] + num[14])                    # at a window's last sample
    assert bool((gc[o + 15] != 0.0).all()) and bool((gc[o + 16:e] == 0.0).all())
    assert bool((gs[o + 16:e] == 0.0).all())
    for t in (want["ws"], want["out_image"], want["grad_ws"], want["partial"], *want["grads"]):
        assert bool(torch.isfinite(t).all())
    assert int(want["mask"][3]) == 0 and int(want["mask"][2]) == 1
    assert float(want["loss"]) != -7.0 and float(want["found_inf"]) == 0.0


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_ray_chain_equals_three_launches(gpu, dtype, defer):
    """Every buffer the three launches write, bit for bit, with the weight sum
    inside (defer 0: gradients, loss, found_inf) and left to the caller (defer
    1: those stay untouched in both)."""
    c, want = _reference(gpu, dtype, defer)
    got = _one_launch(c, gpu, defer)
    for name in want:
        if name == "grads":
            for k, (x, y) in enumerate(zip(want[name], got[name])):
                assert torch.equal(x, y), (name, k)
        elif name == "grad_rgb":
            assert torch.equal(want[name].view(torch.int16), got[name].view(torch.int16)), name
        else:
            assert torch.equal(want[name], got[name]), name
    if defer:
        assert float(got["loss"]) == -7.0 and float(got["grads"][0][0, 0]) == -7.0


def test_ray_chain_reports_a_non_finite_gradient(gpu):
    """found_inf as the head's entry sets it: an inf upstream gradient of ray 0
    makes the background network's gradients non-finite."""
    c, _ = _reference(gpu, torch.float16, 0)
    bad = dict(c, g_image=c["g_image"].clone())
    bad["g_image"][1, 0] = float("inf")
    want, got = _three_launches(bad, gpu, 0), _one_launch(bad, gpu, 0)
    assert float(want["found_inf"]) == 1.0 == float(got["found_inf"])


def test_ray_chain_refuses_bad_arguments(gpu):
    c, _ = _reference(gpu, torch.float16, 0)
    with pytest.raises(RuntimeError, match="rgb dtype"):
        _one_launch(dict(c, dtype=torch.float64), gpu, 0)
    with pytest.raises(RuntimeError, match="null pointer"):
        _one_launch(dict(c, scale=None), gpu, 0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
def test_whole_step_ray_chain_on_equal_off(gpu, bf16):
    """Twin 16 x 16 trainers, three graph-replayed steps, the fused chain on
    against the three launches: parameters, density grid, loss and the
    rendered image are equal."""
    import bench

    def run(on):
        tr, dt = bench.make_trainer(16, 5, 0, 1, True, graph=True, bf16=bf16)
        tr.opt.iters = 50
        assert tr.fused_ray_chain is True  # default on
        tr.fused_ray_chain = on
        for i in range(3):
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        return tr, next(iter(tr._graphs.values()))
    (a, ga), (b, gb) = run(True), run(False)
    assert ga.native is not None and ga.native.ray_chain and not gb.native.ray_chain
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb)
    assert torch.equal(a.model.density_grid, b.model.density_grid)
    assert torch.equal(ga.loss, gb.loss)
    na, nb = ga.native, gb.native
    assert int(na.counter[0]) > 0
    for name in ("out_image", "out_depth", "mask", "image", "ws", "depth", "grad_ws",
                 "grad_image"):
        assert torch.equal(getattr(na, name), getattr(nb, name)), name
    m = int(na.counter[0])
    assert torch.equal(na.grad_sigma[:m], nb.grad_sigma[:m])
    assert torch.equal(na.grad_albedo[:m].view(torch.int16), nb.grad_albedo[:m].view(torch.int16))
