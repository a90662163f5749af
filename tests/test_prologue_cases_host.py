"""CPU checks of tests/prologue_cases.py: the fixed cases contain what they are
named for, the f32 restatements alone stay within half of the bounds the GPU
tests allow the kernels (so half of each bound is left for the device's own
logf / sincosf / sqrtf), and the restated draws have the properties the
project states: one Philox word per output, t over the whole of [min_step,
max_step], every half of (seed, step) in use."""
import itertools

import numpy as np
import pytest

import oracle
import prologue_cases as pc

F32, F64 = np.float32, np.float64
CASES = pc.cases()


def _host_rays(c):
    o, d = pc.pixel_rays32(c.pose, *c.intr(), c.H, c.W)
    with np.errstate(divide="ignore", invalid="ignore"):
        ne, fa = oracle.near_far_from_aabb(o, d, c.aabb, c.min_near)
    return o, d, ne, fa


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_case_contains_what_it_is_named_for(c):
    assert c.H <= 257 and c.W <= 255 and c.N <= 64 * 64
    o, d, ne, fa = _host_rays(c)
    census = pc.slab_census(o, d, c.aabb, c.min_near, ne, fa)
    for what in c.named:
        if what.startswith("t="):
            t = int(pc.t_draw(c.seed, [c.step], c.min_step, c.max_step)[0])
            assert t == int(what[2:]) and t in (c.min_step, c.max_step)
        else:
            assert census[what] >= 1, (c.name, what, census)
    if "inside" in c.named:
        assert census["inside"] == c.N and census["miss"] == 0
    if not c.named:
        assert census["miss"] < c.N  # a random pose sees the box


def test_cases_cover_the_issue_list():
    shapes = {(c.H, c.W) for c in CASES if c.name.startswith("random")}
    assert shapes == set(pc.SHAPES)
    fovs = {c.name.rsplit("fov", 1)[1] for c in CASES if c.name.startswith("random")}
    assert fovs == {"20", "55", "120"}
    named = set(itertools.chain.from_iterable(c.named for c in CASES))
    assert {"zero", "nan", "inside", "inverted", "miss", "t=20", "t=21", "t=999"} <= named
    assert {(c.min_step, c.max_step) for c in CASES} == set(pc.SPANS)
    assert any(c.seed >= 2 ** 32 for c in CASES) and any(c.seed == 2 ** 64 - 1 for c in CASES)
    assert any(c.step >= 2 ** 32 for c in CASES) and any(c.step == 2 ** 64 - 1 for c in CASES)
    a, b = pc.prefix_pair()
    assert (a.H, a.W, b.H, b.W) == (16, 16, 17, 16)
    assert (a.seed, a.step) == (b.seed, b.step) and np.array_equal(a.pose, b.pose)


def test_f32_draws_stay_within_half_the_value_bound():
    worst = 0.0
    for seed, step in ((0, 0), (2 ** 64 - 1, 2 ** 32 + 3), (11, 1234)):
        d64 = pc.draws(seed, step, 200_000, 1, 20, 999, F64)
        d32 = pc.draws(seed, step, 200_000, 1, 20, 999, F32)
        assert d32["t"] == d64["t"] and d32["w"] == d64["w"] == (d64["t"] + 1) / 1024
        assert np.array_equal(d32["noise"], d64["noise"]) and np.array_equal(d32["bg"], d64["bg"])
        assert 0 <= d64["noise"].min() and d64["noise"].max() < 1
        assert 0 <= d64["bg"].min() and d64["bg"].max() < 1
        assert np.isfinite(d64["eps"]).all()  # the log's argument is never 0
        ratio = np.abs(d32["g_image"].astype(F64) - d64["g_image"]) / pc.g_image_bound(d64)
        worst = max(worst, float(ratio.max()))
    print(f"\nprologue: numpy f32 draws reach {worst * pc.VALUE_UNITS:.2f} of the allowed "
          f"{pc.VALUE_UNITS} units of 2^-24 * w * max(r, 2^-12)")
    assert worst <= 0.5, worst


def test_f32_directions_stay_within_half_the_direction_bound():
    worst = 0.0
    pairs = CASES + list(pc.prefix_pair())
    assert len(pairs) >= 30
    for c in pairs:
        o64, d64 = pc.pixel_rays64(c.pose, *c.intr(), c.H, c.W)
        o32, d32 = pc.pixel_rays32(c.pose, *c.intr(), c.H, c.W)
        assert np.array_equal(o32.astype(F64), o64)
        np.testing.assert_allclose(np.linalg.norm(d64, axis=1), 1.0, atol=1e-6, rtol=0)
        worst = max(worst, float(np.abs(d32.astype(F64) - d64).max()) / pc.U24)
    print(f"\nprologue: numpy f32 directions reach {worst:.2f} of the allowed {pc.DIR_UNITS} "
          f"units of 2^-24 over {len(pairs)} pose / shape pairs")
    assert worst <= pc.DIR_UNITS / 2, worst


def test_no_two_outputs_read_the_same_word():
    uni = list(pc.UNIFORM_WORDS.values())
    assert len(set(uni)) == len(uni) == 4
    pair_a, pair_b = pc.NORMAL_WORDS["eps0"], pc.NORMAL_WORDS["eps2"]
    assert pc.NORMAL_WORDS["eps1"] == pair_a  # the sine of eps0's pair
    normal = [*pair_a, *pair_b]
    assert len(set(normal)) == 4 and not set(normal) & set(uni)
    assert set(uni) | set(normal) == {(s, w) for s in (0, 1) for w in range(4)}
    # and in the values: no output is a copy of another
    d = pc.draws(5, 6, 4096, 1, 20, 999)
    outs = [d["noise"], *d["bg"].T, *d["eps"]]
    assert len(outs) == 7
    for a, b in itertools.combinations(outs, 2):
        assert np.abs(np.corrcoef(a, b)[0, 1]) < 0.1


def test_t_covers_both_ends_of_its_range():
    t = pc.t_draw(11, list(range(4096)), 5, 7)
    assert set(t.tolist()) == {5, 6, 7}
    assert set(pc.t_draw(11, list(range(64)), 9, 9).tolist()) == {9}


def test_every_half_of_seed_and_step_reaches_the_draw():
    seed, step = 0x1234, 77
    planes = [pc.draws(s, t, 1024, 1, 20, 999)["noise"]
              for s, t in ((seed, step), (seed + 2 ** 32, step), (seed, step + 2 ** 32))]
    for a, b in itertools.combinations(planes, 2):
        assert (a != b).mean() > 0.99


def test_draws_do_not_depend_on_the_ray_count():
    a, b = pc.draws(3, 4, 256, 1, 20, 999), pc.draws(3, 4, 272, 1, 20, 999)
    assert a["t"] == b["t"]
    for k in ("noise", "bg"):
        assert np.array_equal(a[k], b[k][:256])
    assert np.array_equal(a["g_image"], b["g_image"][:, :256])


@pytest.mark.parametrize("degenerate", [False, True])
def test_near_far_rows_contain_their_kinds(degenerate):
    o, d, aabb, kind = pc.near_far_rows(257, 3, degenerate)
    assert np.array_equal(o, o.astype(np.float16).astype(F32))
    assert np.array_equal(d, d.astype(np.float16).astype(F32))
    for min_near in (0.05, 0.2, 0.0):
        with np.errstate(divide="ignore", invalid="ignore"):
            ne, fa = oracle.near_far_from_aabb(o, d, aabb, min_near)
        rows = lambda k: kind == pc.NEAR_FAR_KINDS.index(k)  # noqa: E731
        census = pc.slab_census(o, d, aabb, min_near, ne, fa)
        assert census["nan"] >= 1 and census["miss"] >= 1 and census["zero"] >= 1
        miss = ne == F32(pc.FLT_MAX)
        assert (ne[rows("inside")] == F32(min_near)).all()
        if min_near > 0.0625:
            # the exit (t = 0.0625) lies before min_near: near = min_near > far
            assert (ne[rows("exit")] == F32(min_near)).all() and (fa[rows("exit")] == F32(0.0625)).all()
        g = rows("graze") & ~miss
        assert g.any() and (ne[g] == fa[g]).all()  # entry == exit on the edge
        assert not miss[rows("axis") & ~np.isnan(ne) & ~np.isnan(fa)].all()


def test_sph_rows_stay_clear_of_a_zero_discriminant():
    o, d, kind = pc.sph_rows(257, 4)
    assert set(kind.tolist()) == set(range(len(pc.SPH_KINDS)))
    radius = np.linalg.norm(o.astype(F64), axis=1) / pc.SPH_RADIUS
    assert (radius[0::3] == 0).all() and (np.abs(radius[1::3] - 0.5) < 0.01).all()
    assert (radius[2::3] > 0.97).all() and (radius < 1).all()
    want, margin = pc.sph_truth(o, d, pc.SPH_RADIUS)
    assert (margin > 1e-6).all(), margin.min()
    assert np.isfinite(want).all()
    assert (np.abs(want[kind == 1, 0] + 1) < 1e-2).all()      # theta = 0
    assert (np.abs(want[kind == 2, 0] - 1) < 1e-2).all()      # theta = pi
    assert (np.abs(np.abs(want[kind == 3, 1]) - 1) < 1e-2).all()  # phi = +-pi
    # the C oracle itself against the formula
    e = pc.sph_errors(oracle.sph_from_ray(o, d, pc.SPH_RADIUS), want, kind)
    print(f"\nsph_from_ray: C oracle vs f64, theta {e[0]:.3e} phi {e[1]:.3e}")
    assert max(e) < 1e-5
    assert pc.sph_phi_rows(kind).sum() >= 128 and (~pc.sph_phi_rows(kind)).sum() >= 64
