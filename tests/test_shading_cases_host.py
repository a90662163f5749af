"""CPU checks of what test_gpu_shading_edges.py relies on (tests/shading_cases.py):
the numpy Philox restatement against the published vectors, the edge rows
against the properties they are named for, the oracle's behaviour on them
against torch f32 autograd of the reference expression, and the oracle alone
against every bound the GPU test sets for the kernels against the float64
truth."""
import numpy as np
import pytest
import torch

import oracle.field as of
import shading_cases as sc

F32 = np.float32
ROWS = 20000
LAM, SCALE = 1e-2, 128.0


def test_philox_published_vectors():
    """Random123's known-answer vectors of Philox4x32-10."""
    got = sc.philox4x32_10(np.zeros(4, np.uint64), np.zeros(2, np.uint64))
    assert [f"{int(x):08x}" for x in got] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    got = sc.philox4x32_10(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], np.uint64),
                           np.array([0xa4093822, 0x299f31d0], np.uint64))
    assert [f"{int(x):08x}" for x in got] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    ones = np.full(4, 0xFFFFFFFF, np.uint64)
    got = sc.philox4x32_10(ones, ones[:2])
    assert [f"{int(x):08x}" for x in got] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_light_draw_is_a_unit_normal_draw():
    n = 4096
    seeds, steps = list(range(n)), [7] * n
    _, l64 = sc.light_draw(seeds, steps, np.zeros((n, 3)), np.float64)
    _, l32 = sc.light_draw(seeds, steps, np.zeros((n, 3)), np.float32)
    np.testing.assert_allclose(np.linalg.norm(l64, axis=1), 1.0, rtol=1e-12)
    assert np.abs(l32 - l64).max() < 1e-5
    assert np.all(np.abs(l64.mean(0)) < 4 / np.sqrt(3 * n))


@pytest.mark.parametrize("elem", ["f16", "bf16"])
def test_edge_rows_are_what_they_are_named(elem):
    c = sc.make(1000, 999, 1, elem)
    for k in sc.KINDS:
        assert sc.rows_of(c, k).sum() == sc.REPEATS
    assert sc.rows_of(c, "bulk").sum() == 999 - sc.EDGE_ROWS
    np.testing.assert_allclose(np.linalg.norm(c.light.astype(np.float64)), 1.0, atol=2e-7)
    with of.precision(elem):
        fo, _, _ = sc.oracle_pair(c, 0.1, "lambertian", LAM, SCALE)
    ss, v = fo["ss"], fo["v"]
    assert np.all(ss[sc.rows_of(c, "a")] == 0)
    b = sc.rows_of(c, "b")
    assert np.all(ss[b] < F32(1e-20)) and np.all(ss[b] > 0) and np.all(np.abs(v[b]).max(1) > 0)
    assert np.all(np.isinf(c.sigma7[:999][sc.rows_of(c, "c")]).sum(1) == 1)
    for k in ("d", "e"):
        r = sc.rows_of(c, k)
        assert np.all(np.isnan(v[r]).sum(1) == 1) and np.all(np.isnan(ss[r]))
        fin = np.where(np.isnan(v[r]), 1.0, v[r])
        assert np.all(np.isfinite(fin)) and np.all(fin != 0)
    f = sc.rows_of(c, "f")
    assert np.all(fo["d16"][f].astype(F32) == 0) and np.all(np.abs(fo["normal"][f, :2]) > 0.4)
    g = sc.rows_of(c, "g")
    assert np.all(fo["nd"][g] == 0) and np.all(np.abs(fo["normal"][g]).max(1) == 1)
    assert np.all(fo["w"][sc.rows_of(c, "h0")] == 0) and np.all(fo["w"][sc.rows_of(c, "h1")] == 1)


@pytest.mark.parametrize("elem", ["f16", "bf16"])
@pytest.mark.parametrize("shading", ["textureless", "lambertian"])
def test_oracle_follows_torch_on_edge_rows(elem, shading):
    """torch CPU f32 autograd of the reference expression is the arbiter of
    the edge rows: the oracle has the same normals there (bit for bit: both
    are f32), all-zero normals on (c), (d), (e), the same non-finite pattern
    of the stencil gradient, and a sub-gradient of 1 where n . l = 0."""
    c = sc.make(1000, 999, 2, elem)
    edge = ~sc.rows_of(c, "bulk")
    t32 = sc.truth(c, torch.float32, 0.1, shading, LAM, SCALE)
    with of.precision(elem):
        fo, gsp, _ = sc.oracle_pair(c, 0.1, shading, LAM, SCALE)
    n32 = t32["normal"].astype(F32)
    assert np.array_equal(n32[edge] == 0, fo["normal"][edge] == 0)
    np.testing.assert_allclose(fo["normal"][edge], n32[edge], rtol=3e-7, atol=0)
    bad = sc.rows_of(c, "c", "d", "e")
    assert not fo["normal"][bad].any() and not n32[bad].any()
    assert np.array_equal(np.isfinite(gsp[edge]), np.isfinite(t32["grad_stencil"][edge]))
    assert np.isnan(t32["grad_stencil"][bad]).all() and np.isnan(gsp[bad]).all()
    assert np.isfinite(gsp[~bad]).all()
    # (f): clamp(min=0) passes the gradient at 0 (the colour path alone)
    f = sc.rows_of(c, "f")
    t0 = sc.truth(c, torch.float32, 0.1, shading, 0.0, SCALE)
    with of.precision(elem):
        _, g0, _ = sc.oracle_pair(c, 0.1, shading, 0.0, SCALE)
    assert np.all(t0["nl"][f] == 0)
    assert np.all(np.abs(t0["grad_stencil"][f]).max(1) > 0) and np.all(np.abs(g0[f]).max(1) > 0)
    np.testing.assert_allclose(g0[f], t0["grad_stencil"][f], rtol=16 * sc.U[elem],
                               atol=1e-3 * np.abs(t0["grad_stencil"][f]).max())


@pytest.mark.parametrize("elem", ["f16", "bf16"])
@pytest.mark.parametrize("shading,ratio", [("textureless", 0.1), ("lambertian", 0.1),
                                           ("lambertian", 0.7), ("textureless", 0.0)])
def test_oracle_meets_the_gpu_bounds(elem, shading, ratio):
    """The oracle alone, on 20 000 rows, against the float64 truth: the bounds
    of test_gpu_shading_edges.py hold for the documented rounding points, so a
    kernel that follows them can meet them."""
    c = sc.make(ROWS, ROWS, 3, elem)
    u = sc.U[elem]
    t64 = sc.truth(c, torch.float64, ratio, shading, LAM, 0.0)
    t32 = sc.truth(c, torch.float32, ratio, shading, LAM, 0.0)
    kept, share = sc.kept_rows(c, t64)
    bulk = sc.rows_of(c, "bulk")
    with of.precision(elem):
        fo, gsp, ga = sc.oracle_pair(c, ratio, shading, LAM, 0.0)
    print(f"\nshading host [{elem} {shading} ratio {ratio}]: excluded share {share:.4%}")
    assert share < sc.EXCLUDED_CAP[elem]
    errs = {"colour": sc.rel_l2(fo["color"].astype(F32)[kept], t64["color"][kept]),
            "stencil gradient": sc.rel_l2(gsp[kept], t64["grad_stencil"][kept])}
    if shading == "lambertian":
        errs["albedo gradient"] = sc.rel_l2(np.asarray(ga, F32)[kept], t64["grad_albedo"][kept])
    for what, e in errs.items():
        print(f"  {what}: oracle vs f64 {e:.3e} (bound {sc.COLOUR_ROUNDINGS * u:.3e})")
        assert e <= sc.COLOUR_ROUNDINGS * u, (what, e)
    # f32 quantities: the project's rule (3 x the torch f32 error + 1e-6)
    zero = np.zeros_like(c.grad_color)
    o64 = sc.truth(c, torch.float64, ratio, shading, LAM, SCALE, grad_color=zero)
    o32 = sc.truth(c, torch.float32, ratio, shading, LAM, SCALE, grad_color=zero)
    with of.precision(elem):
        _, go, _ = sc.oracle_pair(c, ratio, shading, LAM, SCALE, grad_color=zero)
    for what, got, t, e in (("normal", fo["normal"], t32["normal"], t64["normal"]),
                            ("orientation gradient", go, o32["grad_stencil"], o64["grad_stencil"])):
        en, et = sc.rel_l2(got[bulk], e[bulk]), sc.rel_l2(t[bulk], e[bulk])
        print(f"  {what}: oracle {en:.3e} torch-f32 {et:.3e}")
        assert np.isfinite(en) and en <= 3 * et + 1e-6, (what, en, et)
    want_orient = fo["orient"].astype(np.float64).sum() / sc.padded_rows(ROWS)
    np.testing.assert_allclose(want_orient, o64["orient"], rtol=1e-6)
