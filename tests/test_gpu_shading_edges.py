"""The shading entries of csrc/shade.hip called directly (dfhip_shading_forward,
dfhip_shading_backward, their _bf16 forms, dfhip_shading_light) on the
synthetic rows of tests/shading_cases.py: flat, tiny and non-finite stencils,
n . l and n . d exactly 0, ratio 0 and 1, live counts at 0, at multiples of
128, at cap and outside [0, cap], the grid-stride second pass, and a non-null
loss pointer.

* against oracle/field.py (shade_forward / shade_backward), which rounds where
  the kernels round: bit-equal normals on the edge rows, the existing
  tolerances of test_gpu_shading.py on the bulk rows;
* against torch CPU f32 autograd of the reference expression for the pattern of
  non-finite gradients on the rows with a non-finite stencil;
* against the float64 truth (shading_cases.truth): the f32 quantities by the
  project's rule (relative L2 error <= 3 x the torch f32 error + 1e-6), the
  element-type quantities within 8 u on the rows away from the clamp's kink.
  tests/test_shading_cases_host.py shows the oracle alone meets these bounds.

Every output buffer has slack rows past cap and is prefilled with a sentinel
bit pattern; rows at or past the live count must keep it, so a wrong clamp of
the count fails an assertion.  Tests print `edges:` lines with the measured
errors (kept in profiles/shading/edges.txt)."""
import numpy as np
import pytest
import torch

import oracle.field as of
import shading_cases as sc

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = [torch.float16, torch.bfloat16]
ELEM = {torch.float16: "f16", torch.bfloat16: "bf16"}
ULP1 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}  # spacing at 1.0
CODE = {"textureless": 1, "lambertian": 2}  # DFHIP_SHADING_*
PAT32, PAT16 = 0x5EA7BEEF, 0x5A5A
SLACK = 64
# rows past 1024 x 256 are reached only by the second pass of the grid-stride loops
BIG = 1024 * 256 + 293

# (cap, M, ratio, lambda_orient, grad_loss)
CASES = [
    (1, 1, 0.1, 1e-2, 128.0),
    (63, 63, 0.0, 1e-2, 1.0),
    (256, 256, 1.0, 0.0, 65536.0),
    (257, 257, 0.7, 1e-2, 128.0),
    (1000, 0, 0.1, 1e-2, 128.0),
    (1000, 1, 0.7, 0.0, 1.0),
    (1000, 127, 0.0, 1e-2, 65536.0),
    (1000, 128, 1.0, 1e-2, 128.0),
    (1000, 999, 0.1, 1e-2, 128.0),
    (1000, 2000, 0.7, 1e-2, 65536.0),  # treated as 1000
    (1000, -3, 0.1, 1e-2, 1.0),        # treated as 0
    (BIG, BIG - 5, 0.1, 1e-2, 128.0),
]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _np(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


class _Buffers:
    """Device inputs of one case and sentinel-filled outputs.  Every buffer
    has `slack` rows past cap; a count above cap gets that many more, so that
    even an unclamped count stays inside the allocations."""

    def __init__(self, gpu, c, dtype):
        import _dfhip
        self.c, self.gpu, self.dtype = c, gpu, dtype
        self.rows = c.cap + SLACK + max(0, c.M - c.cap)
        pad = self.rows - c.cap
        dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(dt)  # noqa: E731
        grow = lambda a: np.concatenate([a, np.zeros((pad,) + a.shape[1:], a.dtype)])  # noqa: E731
        alb7 = np.full((c.cap, 7, 3), np.nan, F32)  # the stencil rows' albedo is never read
        alb7[:, 0] = c.albedo
        self.sigma7 = dev(grow(c.sigma7))
        self.albedo7 = dev(grow(alb7), dtype)
        self.dirs = dev(grow(c.dirs))
        self.light = dev(c.light)
        self.grad_sigma = dev(grow(c.grad_sigma))
        self.m_dev = torch.tensor([c.M], dtype=torch.int32, device=gpu)
        self.partial = torch.zeros(int(_dfhip.load().dfhip_shading_partial_doubles(c.cap)),
                                   dtype=torch.float64, device=gpu)
        self._grow, self._dev = grow, dev

    def out32(self, per_row):
        return torch.full((self.rows * per_row,), PAT32, dtype=torch.int32, device=self.gpu)

    def out16(self, per_row):
        return torch.full((self.rows * per_row,), PAT16, dtype=torch.int16, device=self.gpu)

    def untouched(self, buf, per_row, what):
        tail = buf[self.c.live * per_row:]
        pat = PAT32 if buf.dtype == torch.int32 else PAT16
        assert bool((tail == pat).all()), f"{what}: rows at or past the live count were written"

    def forward(self, shading, ratio, lam, orient=True, loss=None):
        import _dfhip
        from _dfhip import ptr
        c, bf = self.c, self.dtype == torch.bfloat16
        sigma, color, normal = self.out32(1), self.out16(3), self.out32(3)
        orient_t = torch.full((1,), float("nan"), device=self.gpu) if orient else None
        _dfhip.call("dfhip_shading_forward_bf16" if bf else "dfhip_shading_forward",
                    ptr(self.sigma7), ptr(self.albedo7), ptr(self.dirs), ptr(self.light),
                    float(F32(ratio)), sc.EPS, CODE[shading], ptr(self.m_dev), c.cap, ptr(sigma),
                    ptr(color), ptr(normal), ptr(self.partial), float(F32(lam)), ptr(orient_t),
                    ptr(loss), _dfhip.stream())
        torch.cuda.synchronize()
        for buf, k, what in ((sigma, 1, "sigma"), (color, 3, "color"), (normal, 3, "normal")):
            self.untouched(buf, k, what)
        M = c.live
        return {"sigma": sigma.view(torch.float32)[:M].cpu().numpy(),
                "color": _np(color.view(self.dtype)[:3 * M].view(M, 3)),
                "normal": normal.view(torch.float32)[:3 * M].view(M, 3).cpu().numpy(),
                "orient": None if orient_t is None else float(orient_t)}

    def backward(self, shading, ratio, lam, grad_loss, grad_color=None):
        import _dfhip
        from _dfhip import ptr
        c, bf = self.c, self.dtype == torch.bfloat16
        gcol = self._dev(self._grow(c.grad_color if grad_color is None else grad_color), self.dtype)
        scale = torch.tensor([grad_loss], dtype=torch.float32, device=self.gpu)
        gs7, ga7 = self.out32(7), self.out16(21)
        _dfhip.call("dfhip_shading_backward_bf16" if bf else "dfhip_shading_backward",
                    ptr(self.sigma7), ptr(self.albedo7), ptr(self.dirs), ptr(self.light),
                    float(F32(ratio)), sc.EPS, CODE[shading], ptr(self.m_dev), c.cap,
                    ptr(self.grad_sigma), ptr(gcol), ptr(scale), float(F32(lam)), ptr(gs7),
                    ptr(ga7), _dfhip.stream())
        torch.cuda.synchronize()
        self.untouched(gs7, 7, "grad_sigma7")
        self.untouched(ga7, 21, "grad_albedo7")
        M = c.live
        return (gs7.view(torch.float32)[:7 * M].view(M, 7).cpu().numpy(),
                _np(ga7.view(self.dtype)[:21 * M].view(M, 7, 3)))


def _close(got, want, rows, what):
    """rtol 1e-4, atol 1e-6 of the largest wanted magnitude among `rows`."""
    if rows.any():
        np.testing.assert_allclose(got[rows], want[rows], rtol=1e-4,
                                   atol=1e-6 * np.abs(want[rows]).max(), err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shading", ["textureless", "lambertian"])
@pytest.mark.parametrize("cap,M,ratio,lam,grad_loss", CASES,
                         ids=[f"cap{c[0]}-M{c[1]}" for c in CASES])
def test_shading_entries_at_their_edges(gpu, cap, M, ratio, lam, grad_loss, shading, dtype):
    elem = ELEM[dtype]
    with of.precision(elem):
        _shading_entries(gpu, sc.make(cap, M, 5, elem), ratio, lam, grad_loss, shading, dtype)


def _shading_entries(gpu, c, ratio, lam, grad_loss, shading, dtype):
    elem, u, L = c.elem, sc.U[c.elem], c.live
    tag = f"edges: [{elem} {shading} cap {c.cap} M {c.M} ratio {ratio}]"
    b = _Buffers(gpu, c, dtype)
    fo, gsp, ga = sc.oracle_pair(c, ratio, shading, lam, grad_loss)
    bulk, edge = sc.rows_of(c, "bulk"), ~sc.rows_of(c, "bulk")
    bad = sc.rows_of(c, "c", "d", "e")  # a non-finite stencil value

    # ---------------------------------------------------------------- forward
    f = b.forward(shading, ratio, lam)
    assert np.array_equal(_bits(f["sigma"]), _bits(c.sigma7[:L, 0]))
    want_n = fo["normal"].reshape(L, 3)
    differ = np.flatnonzero(edge & (_bits(f["normal"]) != _bits(want_n)).any(1))
    assert differ.size == 0, (
        f"normals of edge rows {differ[:6]} (kinds {[sc.KINDS[k] for k in c.kind[differ[:6]]]}) "
        f"differ from the oracle's: got {f['normal'][differ[:3]].tolist()}, "
        f"want {want_n[differ[:3]].tolist()}")
    nan_axis = sc.rows_of(c, "d", "e")
    assert not f["normal"][nan_axis].any(), f["normal"][nan_axis]
    r16 = sc.round_elem(F32(ratio), elem)
    want_bad = (np.broadcast_to(r16, (L, 3)) if shading == "textureless"
                else sc.round_elem(c.albedo[:L] * r16, elem))
    assert np.isfinite(f["color"]).all()
    assert np.array_equal(f["color"][bad], want_bad[bad]), (f["color"][bad], want_bad[bad])
    np.testing.assert_allclose(f["normal"][bulk], want_n[bulk], rtol=2e-6, atol=2e-7)
    want_col = np.asarray(fo["color"], F32).reshape(L, 3)
    flips = (f["color"] != want_col).any(1)
    if bulk.any():
        assert flips[bulk].mean() <= 1e-3, flips[bulk].mean()
    np.testing.assert_allclose(f["color"], want_col, atol=2 * ULP1[dtype], rtol=0)
    want_orient = fo["orient"].astype(np.float64).sum() / sc.padded_rows(L)
    np.testing.assert_allclose(f["orient"], want_orient, rtol=1e-5)
    assert np.isfinite(f["orient"]) and (L > 0 or f["orient"] == 0.0)  # M = 0: 0 / 128
    # a loss pointer: *loss += lambda * orient in f32; no orient pointer
    loss = torch.full((1,), 3.25, device=gpu)
    f2 = b.forward(shading, ratio, lam, orient=False, loss=loss)
    assert float(loss) == float(F32(3.25) + F32(lam) * F32(f["orient"])), (float(loss), f["orient"])
    for k in ("sigma", "color", "normal"):
        assert np.array_equal(_bits(f2[k].astype(F32)), _bits(f[k].astype(F32))), k

    # ---------------------------------------------------------------- backward
    g7, ga7 = b.backward(shading, ratio, lam, grad_loss)
    assert np.array_equal(_bits(g7[:, 0]), _bits(c.grad_sigma[:L]))
    assert not ga7[:, 1:].any(), "stencil rows carry an albedo gradient"
    clean = ~flips
    if shading == "lambertian":
        np.testing.assert_allclose(ga7[:, 0][clean], np.asarray(ga, F32)[clean],
                                   rtol=2 * ULP1[dtype], atol=1e-7)
    else:
        assert not ga7[:, 0].any()
    got = g7[:, 1:]
    _close(got, gsp, bulk & clean, "stencil gradient, bulk rows")
    for k in ("a", "b", "f", "g", "h0", "h1"):
        rows = sc.rows_of(c, k)
        assert np.isfinite(gsp[rows]).all()
        _close(got, gsp, rows, f"stencil gradient, rows ({k})")
    if bad.any():
        t32 = sc.truth(c, torch.float32, ratio, shading, lam, grad_loss)
        assert np.isnan(t32["grad_stencil"][bad]).all()
        assert np.array_equal(np.isfinite(got[bad]), np.isfinite(t32["grad_stencil"][bad])), got[bad]
        assert np.isnan(got[bad]).all()

    # ---------------------------------------------------------------- float64 truth
    if L < 999:
        return
    t64 = sc.truth(c, torch.float64, ratio, shading, lam, 0.0)
    t32 = sc.truth(c, torch.float32, ratio, shading, lam, 0.0)
    kept, share = sc.kept_rows(c, t64)
    print(f"\n{tag} excluded share {share:.4%} (cap {sc.EXCLUDED_CAP[elem]:.0%}) of "
          f"{int(bulk.sum())} bulk rows")
    assert share < sc.EXCLUDED_CAP[elem]
    g7c, ga7c = b.backward(shading, ratio, lam, 0.0)  # the colour path alone
    errs = {"colour": sc.rel_l2(f["color"][kept], t64["color"][kept]),
            "stencil gradient": sc.rel_l2(g7c[:, 1:][kept], t64["grad_stencil"][kept])}
    if shading == "lambertian":
        errs["albedo gradient"] = sc.rel_l2(ga7c[:, 0][kept], t64["grad_albedo"][kept])
    for what, e in errs.items():
        print(f"{tag} {what}: native vs f64 {e:.3e} (bound 8u = {8 * u:.3e})")
    zero = np.zeros_like(c.grad_color)
    g7o, _ = b.backward(shading, ratio, lam, grad_loss, grad_color=zero)  # orientation alone
    o64 = sc.truth(c, torch.float64, ratio, shading, lam, grad_loss, grad_color=zero)
    o32 = sc.truth(c, torch.float32, ratio, shading, lam, grad_loss, grad_color=zero)
    rule = []
    for what, nat, t, e in (("normal", f["normal"], t32["normal"], t64["normal"]),
                            ("orientation gradient", g7o[:, 1:], o32["grad_stencil"],
                             o64["grad_stencil"])):
        en, et = sc.rel_l2(nat[bulk], e[bulk]), sc.rel_l2(t[bulk], e[bulk])
        print(f"{tag} {what}: native {en:.3e} torch-f32 {et:.3e} ratio {en / et:.3f}")
        rule.append((what, en, et))
    for what, e in errs.items():
        assert e <= 8 * u, (what, e)
    for what, en, et in rule:
        assert np.isfinite(en) and en <= 3 * et + 1e-6, (what, en, et)


# ---------------------------------------------------------------- dfhip_shading_light

def _light_pairs(n, seed):
    """(seed, step) pairs below 2^64, both halves in use; then pairs that
    differ from pair 0 in one high half only, or in one low half only."""
    rng = np.random.default_rng(seed)
    w = lambda: rng.integers(0, 2 ** 32, n, dtype=np.uint64)  # noqa: E731
    seeds = [int(h) << 32 | int(l) for h, l in zip(w(), w())]
    steps = [int(h) << 32 | int(l) for h, l in zip(w(), w())]
    # the values training uses: a small seed, a small step
    seeds[1:5], steps[1:5] = [0, 0, 11, 11], [0, 1234, 0, 1234]
    s0, t0 = seeds[0], steps[0]
    near = [(s0 ^ (1 << 32), t0), (s0, t0 ^ (1 << 32)), (s0 ^ (1 << 63), t0), (s0, t0 ^ (1 << 63)),
            (s0 ^ 1, t0), (s0, t0 ^ 1), (t0, s0)]
    for k, (s, t) in enumerate(near):
        seeds[5 + k], steps[5 + k] = s, t
    return seeds, steps, [0] + list(range(5, 5 + len(near)))


def _lights(gpu, seeds, steps, rays_o):
    import _dfhip
    from _dfhip import ptr
    n = len(seeds)
    ro = torch.from_numpy(rays_o.astype(F32)).to(gpu).contiguous()
    out = torch.full((n + 1, 3), float("nan"), device=gpu)
    st = _dfhip.stream()
    for i in range(n):
        _dfhip.call("dfhip_shading_light", ptr(ro) + 12 * i, seeds[i], steps[i], ptr(out) + 12 * i, st)
    torch.cuda.synchronize()
    assert torch.isnan(out[n]).all()
    return out[:n].cpu().numpy()


def test_shading_light_follows_its_documented_draw(gpu):
    """include/dfhip.h documents the draw; shading_cases.light_draw restates it.
    The allowance is 4 x the largest error of that restatement evaluated in
    numpy f32 (the device's operations: logf, sincosf and sqrtf at a few ulp)
    against its f64 evaluation, + 2^-23, where |rays_o + z| >= 0.25 (the
    normalisation divides every error by that length)."""
    n = 4096
    seeds, steps, near = _light_pairs(n, 17)
    rng = np.random.default_rng(18)
    rays_o = (sc._unit(rng, n) * rng.uniform(1.0, 1.5, (n, 1))).astype(F32)
    got = _lights(gpu, seeds, steps, rays_o)
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6, rtol=0)
    length, want = sc.light_draw(seeds, steps, rays_o, np.float64)
    _, want32 = sc.light_draw(seeds, steps, rays_o, np.float32)
    ok = length >= 0.25
    assert ok.mean() >= 0.95, ok.mean()
    e32 = float(np.abs(want32.astype(np.float64) - want)[ok].max())
    err = float(np.abs(got.astype(np.float64) - want)[ok].max())
    print(f"\nedges: light: {ok.mean():.2%} of {n} cases qualify; native vs f64 restatement "
          f"{err:.3e}, numpy f32 restatement vs f64 {e32:.3e}, allowed {4 * e32 + 2.0 ** -23:.3e}")
    assert err <= 4 * e32 + 2.0 ** -23, (err, e32)
    # every half of (seed, step) reaches the key / counter
    for k in near[1:]:
        assert np.abs(got[k] - got[near[0]]).max() > 1e-3, (k, got[k], got[near[0]])


def test_shading_light_is_isotropic_about_the_origin(gpu):
    n = 4096
    seeds, steps, _ = _light_pairs(n, 19)
    got = _lights(gpu, seeds, steps, np.zeros((n, 3), F32)).astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6, rtol=0)
    mean = got.mean(0)
    print(f"\nedges: light: mean direction over {n} draws at rays_o = 0: {mean}")
    assert np.all(np.abs(mean) < 4 / np.sqrt(3 * n)), mean
