"""The occupancy-grid marchers away from the one setting every other test
uses (bound 1, one cascade, dt_gamma 0, H 128): several cascades, a growing
dt, other grid sizes, dt ties and a zero start, against the CPU oracle
(oracle.c march_one_, the serial restatement of raymarching.cu:42-54,
337-400).  Bit-exact throughout: a wrong level, cell or successor lane shows
as different sample counts, not as a small error.

Matrix (DESIGN.md "March settings"); every row at seed 0, rays 24 x 24
(16 x 16 at H = 512), bitfield random_bitfield(C, H, 0) unless noted:

  case   C bound  H   dt_gamma max_steps radius min_near
  a      2 2.0    128 0        512       1.8    0.2
  b      2 2.0    128 1/128    512       2.6    0.05
  c      3 4.0    128 0        1024      3.0    0.05
  c_dt   3 4.0    128 1/64     1024      3.0    0.05
  d      2 1.5    128 1/128    512       1.4    0.05
  e1028  2 2.0    128 0        1028      1.8    0.2    dt tie for t in [1, 2)
  e514   2 2.0    128 0        514       1.8    0.2    dt tie for t in [2, 4)
  f      1 1.0    128 0        431       1.3    0.2    dt tie for t in [0.5, 1)
  g      2 2.0    256 1/256    1024      1.8    0.05
  h      1 1.0    512 0        1024      1.3    0.2
  i      4 8.0    64  1/32     256       6.0    0.05
  j      2 2.0    16  0        64        1.8    0.05
  k_*    2 2.0    128 0, 1/128 64        1.8    0.2    bitfield all 0xFF / 0x00,
                                                       first 50 origins at (9, 9, 9)
  l      2 2.0    128 0        512       1.2    -      nears all zero; the noise of
                                                       the even rays is zero too, so
                                                       their first window starts at
                                                       t = 0 (the other rays start at
                                                       noise * dt_min)
"""
import functools

import numpy as np
import pytest
import torch

import oracle
from scenes import march_inputs_general, random_bitfield
from test_gpu_raymarching import T, _march_gpu, assert_close

gpu_test = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max

# name: C, bound, H, dt_gamma, max_steps, camera radius, min_near, bitfield
CASES = {
    "a": (2, 2.0, 128, 0.0, 512, 1.8, 0.2, "random"),
    "b": (2, 2.0, 128, 1 / 128, 512, 2.6, 0.05, "random"),
    "c": (3, 4.0, 128, 0.0, 1024, 3.0, 0.05, "random"),
    "c_dt": (3, 4.0, 128, 1 / 64, 1024, 3.0, 0.05, "random"),
    "d": (2, 1.5, 128, 1 / 128, 512, 1.4, 0.05, "random"),
    "e1028": (2, 2.0, 128, 0.0, 1028, 1.8, 0.2, "random"),
    "e514": (2, 2.0, 128, 0.0, 514, 1.8, 0.2, "random"),
    "f": (1, 1.0, 128, 0.0, 431, 1.3, 0.2, "random"),
    "g": (2, 2.0, 256, 1 / 256, 1024, 1.8, 0.05, "random"),
    "h": (1, 1.0, 512, 0.0, 1024, 1.3, 0.2, "random"),
    "i": (4, 8.0, 64, 1 / 32, 256, 6.0, 0.05, "random"),
    "j": (2, 2.0, 16, 0.0, 64, 1.8, 0.05, "random"),
    "k_full": (2, 2.0, 128, 0.0, 64, 1.8, 0.2, "full"),
    "k_full_dt": (2, 2.0, 128, 1 / 128, 64, 1.8, 0.2, "full"),
    "k_empty": (2, 2.0, 128, 0.0, 64, 1.8, 0.2, "empty"),
    "k_empty_dt": (2, 2.0, 128, 1 / 128, 64, 1.8, 0.2, "empty"),
    "l": (2, 2.0, 128, 0.0, 512, 1.2, None, "random"),
}
# max_steps: binade exponent e of the t for which dt is a tie in ulps of t
TIES = {"e1028": 0, "e514": 1, "f": -1}
SEED = 0


class Case:
    """Inputs of one matrix row and the oracle's march of them (computed once,
    shared by every test of the row, never modified)."""

    def __init__(self, name):
        (self.C, self.bound, self.H, self.dt_gamma, self.max_steps, radius, min_near,
         kind) = CASES[name]
        self.name = name
        side = 16 if self.H == 512 else 24
        o, d, nears, fars, noises = march_inputs_general(
            side, side, SEED, self.bound, radius, 0.2 if min_near is None else min_near)
        if name.startswith("k_"):
            o[:50] = [9.0, 9.0, 9.0]  # these miss the box: near = far = FLT_MAX
            aabb = np.array([-self.bound] * 3 + [self.bound] * 3, np.float32)
            nears, fars = oracle.near_far_from_aabb(o, d, aabb, min_near)
        if name == "l":
            nears = np.zeros_like(nears)
            noises[::2] = 0.0
        n_bytes = self.C * self.H ** 3 // 8
        if kind == "random":
            bf = random_bitfield(self.C, self.H, SEED)
        else:
            bf = np.full(n_bytes, 255 if kind == "full" else 0, np.uint8)
        assert bf.shape == (n_bytes,) and bf.dtype == np.uint8
        self.kind = kind
        self.inputs = (o, d, nears, fars, noises, bf)
        self.counts, self.xyzs, self.dirs, self.deltas = oracle.march_rays_train(
            o, d, bf, self.bound, self.dt_gamma, self.max_steps, self.C, self.H, nears, fars,
            noises)
        for a in (self.counts, self.xyzs, self.dirs, self.deltas):
            a.setflags(write=False)
        self.total = int(self.counts.sum())
        self.kw = dict(max_steps=self.max_steps, bound=self.bound, dt_gamma=self.dt_gamma,
                       C=self.C, H=self.H)

    def dt_consts(self):
        """dt_min, dt_max as the kernels' f32 arithmetic gives them."""
        two_sqrt3 = np.float32(2.0) * np.float32(1.7320508075688772)
        dt_min = two_sqrt3 / np.float32(self.max_steps)
        dt_max = two_sqrt3 * np.float32(1 << (self.C - 1)) / np.float32(self.H)
        assert dt_min.dtype == np.float32 and dt_max.dtype == np.float32
        return dt_min, dt_max

    def levels(self):
        """Per-sample cascade level from the position and from dt
        (oracle.c mip_from_pos_ / mip_from_dt_ restated in numpy)."""
        mx = np.abs(self.xyzs).max(1) if self.total else np.zeros(0, np.float32)
        lp = np.clip(np.frexp(mx)[1], 0, self.C - 1)
        md = ((self.deltas[:, 0] * np.float32(self.H)).astype(np.float64) * 0.5).astype(np.float32)
        ld = np.clip(np.frexp(md)[1], 0, self.C - 1)
        return lp, ld

    def sample_t(self):
        """t of every sample before its step, rebuilt per ray from deltas[:, 1]
        (f64 sums of the f32 differences; exact to a few ulps, enough to
        name the binade)."""
        o, d, nears, fars, noises, _ = self.inputs
        dt_min, dt_max = self.dt_consts()
        t0 = nears.astype(np.float64) + noises.astype(np.float64) * np.clip(
            nears.astype(np.float64) * self.dt_gamma, dt_min, dt_max)
        offs = oracle.rays_from_counts(self.counts)[:, 1]
        t_after = np.cumsum(self.deltas[:, 1].astype(np.float64))
        ray = np.repeat(np.arange(len(self.counts)), self.counts)
        before = np.concatenate([[0.0], t_after])[offs][ray]  # the sum up to the ray's start
        return t0[ray] + (t_after - before) - self.deltas[:, 0].astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def check_conditions(c):
    """What keeps a row from degenerating, from the oracle's output alone."""
    dt_min, dt_max = c.dt_consts()
    lp, ld = c.levels()
    level = np.maximum(lp, ld)
    if c.kind == "empty":
        assert c.total == 0
        return
    assert c.total > 4000, c.total
    if c.name in TIES:
        e = TIES[c.name]
        assert dt_min <= dt_max  # dt is dt_min
        D = np.float64(dt_min) * 2.0 ** (23 - e)
        assert abs(D - np.rint(D)) == 0.5, D  # dt is a tie in ulps of t in [2^e, 2^(e+1))
        t = c.sample_t()
        in_binade = (t >= 2.0 ** e) & (t < 2.0 ** (e + 1))
        assert in_binade.sum() >= 2000, in_binade.sum()
    if c.dt_gamma == 0 and c.C > 1 and c.kind == "random":
        share = np.bincount(level, minlength=c.C) / c.total
        assert share.min() >= 0.05, share
    if c.dt_gamma > 0 and c.kind == "random":
        assert (ld > lp).sum() >= 1000, (ld > lp).sum()
        assert len(np.unique(c.deltas[:, 0])) > 1000
    if c.name.startswith("k_"):
        assert np.all(c.inputs[2][:50] == FLT_MAX) and np.all(c.counts[:50] == 0)
        if c.dt_gamma == 0:
            assert (c.counts == c.max_steps).sum() >= 10
        assert c.counts.max() <= c.max_steps
    if c.name == "l":
        o = c.inputs[0]
        assert np.all(np.abs(o) < c.bound)  # the camera is inside the box
        assert np.all(c.inputs[2] == 0) and (c.counts[::2] > 0).sum() > 100


@pytest.mark.parametrize("name", list(CASES))
def test_case_inputs_not_degenerate(name):
    """No GPU: the conditions on every row's inputs hold on the oracle."""
    check_conditions(case(name))


# ------------------------------------------------------------------ march (train)

def _check_ordered(c, xyzs, dirs, deltas, rays, counter, cap):
    rays = rays.cpu().numpy()
    n, total = len(c.counts), c.total
    np.testing.assert_array_equal(rays[:, 0], np.arange(n))
    np.testing.assert_array_equal(rays[:, 2], c.counts)
    np.testing.assert_array_equal(rays[:, 1], oracle.rays_from_counts(c.counts)[:, 1])
    assert counter.cpu().tolist() == [total, n]
    np.testing.assert_array_equal(xyzs[:total].cpu().numpy(), c.xyzs)
    np.testing.assert_array_equal(dirs[:total].cpu().numpy(), c.dirs)
    np.testing.assert_array_equal(deltas[:total].cpu().numpy(), c.deltas)
    # align tail (reference rule: m + 128 - m % 128 rows) zero, poison beyond
    m_al = total + 128 - total % 128
    assert m_al + 4 <= cap
    for a in (xyzs, dirs, deltas):
        assert torch.all(a[total:m_al] == 0)
        assert torch.all(a[m_al:m_al + 4] == 7.0)


@gpu_test
@pytest.mark.parametrize("path", ["split", "staged", "abi"])
@pytest.mark.parametrize("name", list(CASES))
def test_march_rays_train_settings(gpu, name, path):
    import _raymarching
    c = case(name)
    check_conditions(c)
    o, d, nears, fars, noises, bf = c.inputs
    n = o.shape[0]
    if path != "abi":
        cap = n * c.max_steps + 256
        out = _march_gpu(gpu, o, d, nears, fars, noises, bf, staged=(path == "staged"), cap=cap,
                         **c.kw)
        _check_ordered(c, *out, cap)
        return
    # the reference-signature entry: caller-zeroed N * max_steps rows, rows in
    # arrival order; compared per ray id
    M = n * c.max_steps
    xyzs = torch.zeros(M, 3, device=gpu)
    dirs = torch.zeros(M, 3, device=gpu)
    deltas = torch.zeros(M, 2, device=gpu)
    rays = torch.full((n, 3), -1, dtype=torch.int32, device=gpu)
    counter = torch.zeros(2, dtype=torch.int32, device=gpu)
    _raymarching.march_rays_train(T(o, gpu), T(d, gpu), T(bf, gpu), c.bound, c.dt_gamma,
                                  c.max_steps, n, c.C, c.H, M, T(nears, gpu), T(fars, gpu), xyzs,
                                  dirs, deltas, rays, counter, T(noises, gpu))
    assert counter.cpu().tolist() == [c.total, n]
    r = rays.cpu().numpy()
    order = np.argsort(r[:, 0], kind="stable")
    np.testing.assert_array_equal(r[order, 0], np.arange(n))  # every ray once
    r = r[order]
    np.testing.assert_array_equal(r[:, 2], c.counts)
    # the offsets tile [0, total) without overlap
    by_off = np.argsort(r[:, 1], kind="stable")
    live = by_off[c.counts[by_off] > 0]
    np.testing.assert_array_equal(r[live, 1], np.cumsum(np.r_[0, c.counts[live]])[:-1])
    want_off = oracle.rays_from_counts(c.counts)[:, 1]
    rows = np.repeat(r[:, 1].astype(np.int64) - want_off, c.counts) + np.arange(c.total)
    np.testing.assert_array_equal(xyzs.cpu().numpy()[rows], c.xyzs)
    np.testing.assert_array_equal(dirs.cpu().numpy()[rows], c.dirs)
    np.testing.assert_array_equal(deltas.cpu().numpy()[rows], c.deltas)
    for a in (xyzs, dirs, deltas):
        assert torch.all(a[c.total:] == 0)


@gpu_test
@pytest.mark.parametrize("staged", [False, True])
def test_march_rays_train_settings_capacity_overflow(gpu, staged):
    """test_march_rays_train_capacity_overflow at row b (two cascades, growing
    dt): rays that do not fit in half the total are not written and their rows
    read as zero."""
    c = case("b")
    o, d, nears, fars, noises, bf = c.inputs
    cap = c.total // 2
    xyzs, _, deltas, rays, _ = _march_gpu(gpu, o, d, nears, fars, noises, bf, cap=cap,
                                          zero_tail=-1, staged=staged, **c.kw)
    offs = oracle.rays_from_counts(c.counts)[:, 1]
    fit = offs + c.counts <= cap
    written = int((offs + c.counts)[fit].max())
    assert 0 < written < cap
    np.testing.assert_array_equal(xyzs[:written].cpu().numpy(), c.xyzs[:written])
    assert torch.all(xyzs[written:] == 0) and torch.all(deltas[written:] == 0)


# ------------------------------------------------------------------ inference

def _infer_loop(gpu, c, schedule, perturb=False):
    """test_march_and_composite_infer's loop at the row's setting: the
    inference marcher and the compositing step on the GPU beside the same loop
    on the oracle, with an analytic field of the position scaled by 1 / bound."""
    import raymarching
    o, d, nears, fars, _, bf = c.inputs
    n = o.shape[0]

    def field(x):
        x = x / np.float32(c.bound)
        sig = 30.0 * np.exp(-4 * (x ** 2).sum(-1))
        return sig.astype(np.float32), (0.5 + 0.5 * np.sin(3 * x)).astype(np.float32)

    o_alive = np.arange(n, dtype=np.int32)
    o_t = nears.copy()
    o_ws, o_d, o_img = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    g_alive = torch.arange(n, dtype=torch.int32, device=gpu)
    g_t = T(nears, gpu).clone()
    g_ws, g_d = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    g_img = torch.zeros(n, 3, device=gpu)
    go, gd, gbf, gne, gfa = (T(a, gpu) for a in (o, d, bf, nears, fars))
    step = marched = 0
    while step < c.max_steps and len(o_alive) > 0:
        k = len(o_alive)
        n_step = max(min(n // k, 8), 1) if schedule == "reference" else 1
        if perturb:
            # the wrapper draws torch.rand(n_alive) on the rays' device: the
            # same draw under the same seed feeds the oracle
            torch.manual_seed(100 + step)
            noise = torch.rand(k, dtype=torch.float32, device=gpu).cpu().numpy()
            assert np.count_nonzero(noise) >= k - 1
            torch.manual_seed(100 + step)
        else:
            noise = np.zeros(k, np.float32)
        ox, _, odl = oracle.march_rays(k, n_step, o_alive, o_t, o, d, c.bound, c.dt_gamma,
                                       c.max_steps, c.C, c.H, bf, fars, noise)
        gx, _, gdl = raymarching.march_rays(k, n_step, g_alive, g_t, go, gd, c.bound, gbf, c.C,
                                            c.H, gne, gfa, 128, perturb, c.dt_gamma, c.max_steps)
        rows = k * n_step
        np.testing.assert_array_equal(gx[:rows].cpu().numpy(), ox)
        np.testing.assert_array_equal(gdl[:rows].cpu().numpy(), odl)
        assert torch.all(gx[rows:] == 0)
        marched += int((odl[:, 0] > 0).sum())
        sig, rgb = field(ox)
        oracle.composite_rays(k, n_step, 1e-2, o_alive, o_t, sig, rgb, odl, o_ws, o_d, o_img)
        raymarching.composite_rays(k, n_step, g_alive, g_t, T(sig, gpu), T(rgb, gpu), gdl[:rows],
                                   g_ws, g_d, g_img, 1e-2)
        np.testing.assert_array_equal(g_alive.cpu().numpy(), o_alive)
        o_alive = o_alive[o_alive >= 0].copy()
        g_alive = g_alive[g_alive >= 0]
        step += n_step
    assert marched > 2000 and (o_ws > 0).sum() > 100  # the loop composited a real scene
    assert_close(g_ws, o_ws, atol=1e-5)
    assert_close(g_img, o_img, atol=1e-5)


@gpu_test
@pytest.mark.parametrize("schedule", ["reference", "one"])
@pytest.mark.parametrize("name", ["b", "c_dt", "e1028"])
def test_march_and_composite_infer_settings(gpu, name, schedule):
    _infer_loop(gpu, case(name), schedule)


@gpu_test
def test_march_infer_perturbed_growing_dt(gpu):
    """perturb=True at row b: the first step of every call moves by
    noise * clamp(t * dt_gamma), not noise * dt_min."""
    _infer_loop(gpu, case("b"), "reference", perturb=True)
