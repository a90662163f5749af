"""Native GradScaler + Adam step (csrc/optim.hip, nerf/optim.py) against
torch's GradScaler.step / update with a fused torch.optim.Adam on the same
parameters and gradients: same parameters, moments, step counts and scale
(f32 tolerance: torch's kernel is compiled with FMA contraction, ours is not),
including a skipped non-finite step and a scale growth."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(gpu, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    shapes = [(1000, 2), (64, 32), (64,), (4, 64), (4,), (3, 64)]
    ps = [torch.randn(s, device=gpu, generator=g).requires_grad_() for s in shapes]
    groups = [{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:], "lr": 1e-3}]
    opt = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15, fused=True)
    sc = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3)
    return ps, opt, sc, g


def test_native_adam_amp_matches_torch(gpu):
    from nerf.optim import NativeAdamAmp, eligible
    pa, oa, sa, g = _setup(gpu, 0)
    pb, ob, sb, _ = _setup(gpu, 0)
    assert eligible(ob, sb)
    nat = NativeAdamAmp(ob, sb)
    for it in range(8):
        grads = [torch.randn(p.shape, device=gpu, generator=g) * 100 for p in pa]
        if it == 4:
            grads[2][3] = float("inf")
        for (p, q, gr) in zip(pa, pb, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        sa.scale(torch.ones((), device=gpu))  # lazy scale init, as backward would
        sb.scale(torch.ones((), device=gpu))
        sa.step(oa)
        sa.update()
        nat.step()
        torch.cuda.synchronize()
        assert float(sa._scale) == float(sb._scale), it
        assert int(sa._growth_tracker) == int(sb._growth_tracker), it
        for p, q in zip(pa, pb):
            torch.testing.assert_close(q, p, rtol=2e-6, atol=1e-7)
            st_a, st_b = oa.state[p], ob.state[q]
            assert float(st_a["step"]) == float(st_b["step"])
            sc = float(st_a["exp_avg"].abs().max())
            torch.testing.assert_close(st_b["exp_avg"], st_a["exp_avg"], rtol=2e-6, atol=1e-6 * sc)
            sq = float(st_a["exp_avg_sq"].abs().max())
            torch.testing.assert_close(st_b["exp_avg_sq"], st_a["exp_avg_sq"], rtol=2e-6,
                                       atol=1e-6 * sq)
    # the inf step was skipped (7 updates) and the scale backed off then grew
    assert float(oa.state[pa[0]]["step"]) == 7.0



# ---------------------------------------------------------------- edge cases
# Shapes around kPerBlock, two groups with different hyper-parameters, mixed
# gradient magnitudes (tests/optim_cases.py); float64 oracle: oracle/optim.py.
import copy  # noqa: E402

import numpy as np  # noqa: E402

import optim_cases as oc  # noqa: E402
import oracle.optim as oo  # noqa: E402


def _case(gpu, init_scale=oc.INIT_SCALE, growth_interval=oc.GROWTH_INTERVAL, enabled=True,
          params=None):
    """The case's parameters in one fused torch Adam with groups A and B, and
    its GradScaler (scale initialised, as backward would)."""
    src = oc.params() if params is None else params
    ps = [torch.from_numpy(np.array(p)).to(gpu).requires_grad_() for p in src]
    groups = [{"params": [p for p, gi in zip(ps, oc.GROUP) if gi == k], **oc.GROUPS[k]}
              for k in range(len(oc.GROUPS))]
    opt = torch.optim.Adam(groups, fused=True)
    sc = torch.amp.GradScaler("cuda", init_scale=init_scale, growth_interval=growth_interval,
                              enabled=enabled)
    if enabled:
        sc.scale(torch.ones((), device=gpu))
    return ps, opt, sc


def _set_grads(ps, grads, gpu, in_place=False):
    """New gradient tensors, or (in_place) the values written into the
    gradient buffers that exist, as the graph-replayed train step does."""
    for p, g in zip(ps, grads):
        if g is None:
            p.grad = None
        elif in_place and p.grad is not None:
            p.grad.copy_(torch.from_numpy(np.array(g)))
        else:
            p.grad = torch.from_numpy(np.array(g)).to(gpu)


def _snap(ps, opt):
    """(p, exp_avg, exp_avg_sq, step) per parameter as numpy (zeros before the
    state exists)."""
    out = []
    for p in ps:
        st = opt.state.get(p, {})
        z = np.zeros(tuple(p.shape), np.float32)
        out.append((p.detach().cpu().numpy().copy(),
                    st["exp_avg"].cpu().numpy().copy() if st else z,
                    st["exp_avg_sq"].cpu().numpy().copy() if st else z.copy(),
                    float(st["step"]) if st else 0.0))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_identical(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
            assert np.array_equal(_bits(x[q]), _bits(y[q])), f"{what} tensor {k} {name} differs"
        assert x[3] == y[3], f"{what} tensor {k} step {x[3]} != {y[3]}"


def _assert_close(pa, oa, sa, pb, ob, sb, what=""):
    """The existing test's tolerances: native (b) against torch (a)."""
    torch.cuda.synchronize()
    if sa is not None and sa.is_enabled():
        assert float(sa._scale) == float(sb._scale), what
        assert int(sa._growth_tracker) == int(sb._growth_tracker), what
    for k, (p, q) in enumerate(zip(pa, pb)):
        st_a, st_b = oa.state.get(p, {}), ob.state.get(q, {})
        assert bool(st_a) == bool(st_b), (what, k)
        torch.testing.assert_close(q, p, rtol=2e-6, atol=1e-7, msg=lambda m: f"{what} p{k}: {m}")
        if not st_a:
            continue
        assert float(st_a["step"]) == float(st_b["step"]), (what, k)
        if p.numel() == 0:
            continue
        for name in ("exp_avg", "exp_avg_sq"):
            mx = float(st_a[name].abs().max())
            torch.testing.assert_close(st_b[name], st_a[name], rtol=2e-6, atol=1e-6 * mx,
                                       msg=lambda m: f"{what} {name}{k}: {m}")


def _torch_step(opt, sc):
    sc.step(opt)
    sc.update()


def test_adam_step_within_rounding_bounds(gpu):
    """Every step of six (t = 1..6) against the float64 oracle started from
    the native path's own float32 state of the previous step, at the float32-
    rounded hyper-parameters the C ABI receives: exp_avg, exp_avg_sq and the
    update d = p_new - p_old (difference taken in float64).

    Bounds: count of roundings of adam1 (csrc/optim.hip), u = 2^-24, first
    order in u (x 1.001 for the products of roundings) plus a few 2^-149 for
    roundings in the subnormal range.  g0 = grad / scale, G = |g0| + |wd p|
    (= |g| without weight decay; with it the sum may cancel, and the roundings
    are relative to the addends).  g carries cg roundings relative to G: the
    division (1), and with weight decay the product and the sum (2 in all,
    since |g| <= G).
      m = b1 m0 + (1 - b1) g: the product b1 m0 and the sum, 2 u |b1 m0|;
        1 - b1, its product with g, g itself and the sum, (3 + cg) u (1 - b1) G:
          |dm| <= c_m u (|b1 m0| + (1 - b1) G),  c_m = 3 + cg;
      v = b2 v0 + ((1 - b2) g) g: 2 u |b2 v0|; 1 - b2, two products, g twice
        and the sum, (4 + 2 cg) u (1 - b2) G^2:
          |dv| <= c_v u (b2 v0 + (1 - b2) G^2),  c_v = 4 + 2 cg;
      step_size = lr / (1 - powf(b1, t)): powf is P = 1 ulp = 2 u relative
        (HIP math API), which the subtraction magnifies by the cancellation
        factor k1 = b1^t / (1 - b1^t); the subtraction and the division round:
        c_s = 2 + 2 k1 P;
      bc2s = sqrtf(1 - powf(b2, t)): (1 + 2 k2 P) / 2 through the root plus
        its rounding, c_bc = 1.5 + k2 P;
      denom = sqrtf(v) / bc2s + eps: dD = |d sqrt(v)| / bc + (sqrt(v) / bc) u
        (2 + c_bc) + u D, where |d sqrt(v)| <= |dv| / (sqrt(v) + sqrt(v - |dv|));
      d = -(step_size m) / denom, then p - (.): with d_abs = step_size (|b1 m0|
        + (1 - b1) G) / D >= |d|,
          |dd| <= d_abs (u (c_m + c_s + 2) + dD / (D - dD)) + u |p_new|
        — the relative term on the un-cancelled update plus the final
        subtraction's rounding.
    tests/test_oracle_kat.py evaluates the same formula in np.float32, one
    rounding per operation, on these inputs: it lies inside these bounds and
    needs more than a quarter of every constant.  A kernel outside a bound
    that evaluation meets computes something else than the formula."""
    from nerf.optim import NativeAdamAmp, eligible
    ps, opt, sc = _case(gpu)
    assert eligible(opt, sc)
    nat = NativeAdamAmp(opt, sc)
    worst = [dict(m=0.0, v=0.0, d=0.0, ds=0.0) for _ in ps]
    for it in range(oc.STEPS):
        scale = float(sc._scale)
        G = oc.grads(it, scale)
        before = _snap(ps, opt)
        _set_grads(ps, G, gpu)
        nat.step()
        torch.cuda.synchronize()
        after = _snap(ps, opt)
        for k, gi in enumerate(oc.GROUP):
            p0, m0, v0, s0 = before[k]
            assert s0 == it and after[k][3] == it + 1
            bd = oc.bounds(p0, G[k], m0, v0, s0, scale, *oc.hyper32(gi))
            for q, r in oc.ratios(bd, p0, *after[k][:3]).items():
                worst[k][q] = max(worst[k][q], r)
    for k, w in enumerate(worst):
        print(f"\nparity: adam n={oc.SIZES[k]} group {'AB'[oc.GROUP[k]]}: worst error / bound over "
              f"{oc.STEPS} steps: exp_avg {w['m']:.3f} exp_avg_sq {w['v']:.3f} update {w['d']:.3f} "
              f"(elements with |p| ~ lr: {w['ds']:.3f})", end="")
    for k, w in enumerate(worst):
        assert max(w.values()) <= 1.0, (oc.SIZES[k], w)


def test_adam_edge_shapes_match_torch(gpu):
    """The same inputs, torch's fused Adam + GradScaler and the native step
    both running freely for six steps (two scale growths)."""
    from nerf.optim import NativeAdamAmp
    pa, oa, sa = _case(gpu)
    pb, ob, sb = _case(gpu)
    nat = NativeAdamAmp(ob, sb)
    for it in range(oc.STEPS):
        G = oc.grads(it, float(sa._scale))
        _set_grads(pa, G, gpu)
        _set_grads(pb, G, gpu)
        _torch_step(oa, sa)
        nat.step()
        _assert_close(pa, oa, sa, pb, ob, sb, f"step {it}")
    assert float(sa._scale) == oc.INIT_SCALE * 4


def test_adam_misaligned_gradients_are_bit_identical(gpu):
    """Gradients as views into one flat buffer at a one-float offset (the
    flat-bucket layout: the element-by-element path) against gradients that
    are each their own allocation (float4 path on whole chunks)."""
    from nerf.optim import NativeAdamAmp
    runs = []
    for flat in (False, True):
        ps, opt, sc = _case(gpu)
        nat = NativeAdamAmp(opt, sc)
        starts = np.cumsum([0] + [(n + 3) // 4 * 4 for n in oc.SIZES])
        buf = torch.zeros(int(starts[-1]) + 1, device=gpu)
        for it in range(3):
            G = oc.grads(it, float(sc._scale))
            _set_grads(ps, G, gpu)
            if flat:
                for p, s0 in zip(ps, starts):
                    view = buf[1 + int(s0):1 + int(s0) + p.numel()]
                    view.copy_(p.grad)
                    p.grad = view
                    assert p.numel() == 0 or view.data_ptr() % 16 == 4
            else:
                assert all(p.grad.data_ptr() % 16 == 0 for p in ps)
            nat.step()
        torch.cuda.synchronize()
        runs.append(_snap(ps, opt))
    _assert_identical(runs[0], runs[1])
    assert runs[0][-1][3] == 3.0


# tensor (index into oc.SIZES) and element of the planted value: the .w lane of
# a float4 inside the 4096 tensor's second whole chunk; the last element of the
# 5000 tensor's tail; the last tensor
_BAD_AT = {"float4": (oc.SIZES.index(4096), 2048 + 1027), "tail": (oc.SIZES.index(5000), 4999),
           "last": (len(oc.SIZES) - 1, 8 * 2048 + 4)}


@pytest.mark.parametrize("place", list(_BAD_AT))
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_adam_skips_nonfinite_step(gpu, bad, place):
    from nerf.optim import NativeAdamAmp
    ps, opt, sc = _case(gpu)
    nat = NativeAdamAmp(opt, sc)
    _set_grads(ps, oc.grads(0, oc.INIT_SCALE), gpu)
    nat.step()
    torch.cuda.synchronize()
    before = _snap(ps, opt)
    G = oc.grads(1, oc.INIT_SCALE)
    k, j = _BAD_AT[place]
    assert oc.SIZES[k] > j
    G[k][j] = bad
    _set_grads(ps, G, gpu)
    nat.step()
    torch.cuda.synchronize()
    _assert_identical(before, _snap(ps, opt), "skipped step:")
    assert float(sc._scale) == oc.INIT_SCALE / 2 and int(sc._growth_tracker) == 0
    # found_inf was cleared: the next finite step updates every tensor
    _set_grads(ps, oc.grads(2, oc.INIT_SCALE / 2), gpu)
    nat.step()
    torch.cuda.synchronize()
    after = _snap(ps, opt)
    assert float(sc._scale) == oc.INIT_SCALE / 2 and int(sc._growth_tracker) == 1
    for n, b, a in zip(oc.SIZES, before, after):
        assert a[3] == 2.0
        for q in range(3):
            assert n == 0 or not np.array_equal(_bits(a[q]), _bits(b[q]))


def test_scale_growth_does_not_overflow(gpu):
    """init_scale 2^127, growth_interval 1: 2^128 is not a float32, so the
    scale stays and the tracker resets (torch._amp_update_scale_)."""
    from nerf.optim import NativeAdamAmp
    big = 2.0 ** 127
    pa, oa, sa = _case(gpu, init_scale=big, growth_interval=1)
    pb, ob, sb = _case(gpu, init_scale=big, growth_interval=1)
    nat = NativeAdamAmp(ob, sb)
    G = oc.grads(0, 1.0)
    _set_grads(pa, G, gpu)
    _set_grads(pb, G, gpu)
    _torch_step(oa, sa)
    nat.step()
    torch.cuda.synchronize()
    assert float(sb._scale) == big == float(sa._scale)
    assert int(sb._growth_tracker) == 0 == int(sa._growth_tracker)
    assert oo.update_scale(big, 0, False, 1) == (big, 0)
    assert float(ob.state[pb[1]]["step"]) == 1.0


class _Pair:
    """torch's fused Adam + GradScaler (a) and the native step (b) on the same
    values, stepped together.  Gradient buffers stay in place from step to
    step, so NativeAdamAmp's cached descriptors are reused unless something
    else tells it to rebuild them."""

    def __init__(self, gpu):
        from nerf.optim import NativeAdamAmp
        self.gpu = gpu
        self.pa, self.oa, self.sa = _case(gpu)
        self.pb, self.ob, self.sb = _case(gpu)
        self.nat = NativeAdamAmp(self.ob, self.sb)

    def grads(self, it):
        G = oc.grads(it, float(self.sa._scale))
        rng = np.random.default_rng(100 + it)
        G += [rng.standard_normal(tuple(p.shape)).astype(np.float32) * float(self.sa._scale)
              for p in self.pa[len(G):]]
        return G

    def step(self, it, drop=None):
        G = self.grads(it)
        if drop is not None:
            G[drop] = None
        _set_grads(self.pa, G, self.gpu, in_place=True)
        _set_grads(self.pb, G, self.gpu, in_place=True)
        _torch_step(self.oa, self.sa)
        self.nat.step()
        _assert_close(self.pa, self.oa, self.sa, self.pb, self.ob, self.sb, f"step {it}")


def test_adam_rereads_group_hyperparameters(gpu):
    """weight_decay, betas and eps of a group changed after the first steps
    are used from the next step on, as torch's optimizer re-reads them."""
    pr = _Pair(gpu)
    pr.step(0)
    pr.step(1)
    for opt in (pr.oa, pr.ob):
        opt.param_groups[1].update(weight_decay=0.1, betas=(0.5, 0.9), eps=1e-3)
    pr.step(2)
    pr.step(3)


def test_adam_parameter_without_gradient_lags(gpu):
    pr = _Pair(gpu)
    pr.step(0)
    pr.step(1, drop=3)
    pr.step(2)
    assert float(pr.ob.state[pr.pb[3]]["step"]) == 2.0
    assert float(pr.ob.state[pr.pb[4]]["step"]) == 3.0


def test_adam_add_param_group(gpu):
    pr = _Pair(gpu)
    pr.step(0)
    pr.step(1)
    new = np.random.default_rng(9).standard_normal((25, 4)).astype(np.float32)
    for ps, opt in ((pr.pa, pr.oa), (pr.pb, pr.ob)):
        ps.append(torch.from_numpy(new.copy()).to(gpu).requires_grad_())
        opt.add_param_group({"params": [ps[-1]], "lr": 5e-3, "betas": (0.7, 0.9), "eps": 1e-6,
                             "weight_decay": 0.0})
    pr.step(2)
    pr.step(3)
    assert float(pr.ob.state[pr.pb[-1]]["step"]) == 2.0
    assert float(pr.ob.state[pr.pb[1]]["step"]) == 4.0


def _restore(ps, opt, sc, saved):
    p_saved, opt_sd, sc_sd = saved
    with torch.no_grad():
        for p, q in zip(ps, p_saved):
            p.copy_(q)
    opt.load_state_dict(copy.deepcopy(opt_sd))
    sc.load_state_dict(sc_sd)


def test_adam_load_state_dict_replays(gpu):
    """optimizer.load_state_dict of a state saved two steps earlier, on the
    same optimizer and the same NativeAdamAmp object: the continuation equals
    the first run of those two steps bit for bit (and torch doing the same)."""
    pr = _Pair(gpu)
    pr.step(0)
    pr.step(1)
    saved = {s: ([p.detach().clone() for p in ps], copy.deepcopy(opt.state_dict()), sc.state_dict())
             for s, (ps, opt, sc) in {"a": (pr.pa, pr.oa, pr.sa), "b": (pr.pb, pr.ob, pr.sb)}.items()}
    pr.step(2)
    pr.step(3)
    torch.cuda.synchronize()
    first = _snap(pr.pb, pr.ob)
    _restore(pr.pa, pr.oa, pr.sa, saved["a"])
    _restore(pr.pb, pr.ob, pr.sb, saved["b"])
    assert float(pr.ob.state[pr.pb[1]]["step"]) == 2.0
    pr.step(2)
    pr.step(3)
    torch.cuda.synchronize()
    _assert_identical(first, _snap(pr.pb, pr.ob), "replay:")


def test_adam_state_dict_into_fresh_objects(gpu):
    """state_dict into a fresh optimizer, GradScaler and NativeAdamAmp
    continues bit-identically to the uninterrupted run."""
    from nerf.optim import NativeAdamAmp

    def run(ps, opt, sc, nat, its):
        for it in its:
            _set_grads(ps, oc.grads(it, float(sc._scale)), gpu)
            nat.step()
        torch.cuda.synchronize()

    ps, opt, sc = _case(gpu)
    run(ps, opt, sc, NativeAdamAmp(opt, sc), range(4))
    want = _snap(ps, opt)
    ps, opt, sc = _case(gpu)
    run(ps, opt, sc, NativeAdamAmp(opt, sc), range(2))
    ps2, opt2, sc2 = _case(gpu, params=[p.detach().cpu().numpy() for p in ps])
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    sc2.load_state_dict(sc.state_dict())
    run(ps2, opt2, sc2, NativeAdamAmp(opt2, sc2), range(2, 4))
    _assert_identical(want, _snap(ps2, opt2))
    assert float(sc2._scale) == float(sc._scale) * 2  # grew at the third clean step


def test_adam_unit_scale_without_scaler(gpu):
    """Disabled GradScaler, unit_scale=True (the bf16 trainer): finite steps
    are torch's fused Adam without a scaler; a non-finite step changes nothing,
    step counts included."""
    from nerf.optim import NativeAdamAmp, eligible
    pa, oa, sa = _case(gpu, enabled=False)
    pb, ob, sb = _case(gpu, enabled=False)
    assert eligible(ob, sb, unit_scale=True) and not eligible(ob, sb)
    nat = NativeAdamAmp(ob, sb)
    for it in range(3):
        G = oc.grads(it, 1.0)
        _set_grads(pa, G, gpu)
        _set_grads(pb, G, gpu)
        oa.step()
        nat.step()
        _assert_close(pa, oa, None, pb, ob, None, f"step {it}")
    before = _snap(pb, ob)
    G = oc.grads(3, 1.0)
    G[3][2048 + 1027] = float("nan")
    _set_grads(pb, G, gpu)
    nat.step()
    torch.cuda.synchronize()
    _assert_identical(before, _snap(pb, ob), "non-finite step:")
    _set_grads(pb, oc.grads(3, 1.0), gpu)
    nat.step()
    torch.cuda.synchronize()
    assert all(s[3] == 4.0 for s in _snap(pb, ob))


def test_eligible_refuses_what_the_kernel_does_not_do(gpu):
    from nerf.optim import eligible
    sc = torch.amp.GradScaler("cuda")
    mk = lambda n=1, **kw: torch.optim.Adam(  # noqa: E731
        [torch.zeros(8, device=gpu, requires_grad=True) for _ in range(n)], lr=1e-3, **kw)
    assert eligible(mk(), sc) and eligible(mk(24), sc)
    assert not eligible(mk(25), sc)
    assert not eligible(mk(amsgrad=True), sc)
    assert not eligible(mk(maximize=True), sc)
    assert not eligible(torch.optim.Adam([torch.zeros(8, device=gpu, requires_grad=True)],
                                         lr=torch.tensor(1e-3)), sc)
    assert not eligible(torch.optim.AdamW([torch.zeros(8, device=gpu, requires_grad=True)]), sc)
    assert not eligible(torch.optim.Adam(
        [torch.zeros(8, device=gpu, dtype=torch.float16, requires_grad=True)]), sc)
    assert not eligible(torch.optim.Adam([torch.zeros(8, requires_grad=True)]), sc)
    assert not eligible(mk(), torch.amp.GradScaler("cuda", growth_factor=3.0))
    assert not eligible(mk(), torch.amp.GradScaler("cuda", backoff_factor=0.25))
    noncontig = torch.zeros(8, 4, device=gpu).t().requires_grad_()
    assert not noncontig.is_contiguous()
    assert not eligible(torch.optim.Adam([noncontig]), sc)


def test_step_refuses_noncontiguous_gradient(gpu):
    from nerf.optim import NativeAdamAmp
    p = torch.zeros(8, 4, device=gpu, requires_grad=True)
    opt = torch.optim.Adam([p], fused=True)
    sc = torch.amp.GradScaler("cuda")
    sc.scale(torch.ones((), device=gpu))
    p.grad = torch.ones(4, 8, device=gpu).t()
    assert not p.grad.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous float32"):
        NativeAdamAmp(opt, sc).step()
    assert not opt.state.get(p)
