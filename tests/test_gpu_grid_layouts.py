"""Grid encoder off its default operating point, against the float64 oracle.

Every embedding backward (atomic, LDS-sliced, binned rows, binned 7-point
stencil groups) and the forward at align_corners=True, at bounds other than 1
(raw positions mapped (x + bound) / (2 bound) by the kernels, powers of two and
not), on levels of more than 64 slices, on hand-built layouts whose levels wrap
by modulo, on a level so small that the tiled index stops before z, with f16 /
bf16 gradients at C = 1 / 2 / 4, and at the batch sizes and device counts where
the tile loops change path.

Every case is built on the CPU first (`_case_*`: inputs, gradients, the
oracle's answer) and asserts that at least 90 % of its samples are in range and
that the expected gradient has non-zeros inside every level's row block, so no
case passes because a level or the whole batch dropped out.  Tolerances are the
ones the tests of each path in test_gpu_encoders.py use: binned and sliced
rtol 1e-5 / atol 1e-6 max|want|, atomic f32 rtol 1e-4 / atol 1e-6 max|want|,
atomic f16 4e-3 max|want| + 1e-3, forward bit-exact.

Which test runs which kernel variant (csrc/gridbin.hip, csrc/gridencoder.hip):

* align_corners in k_grid_bwd, k_grid_bwd_sliced, k_bin, k_bin_fast, k_walk,
  k_walk_flat and the host's make_fast_levels / uniform_mode:
  test_align_corners_* (stencil groups: tiled only — a hashed level is not the
  mask form the groups need, the call raises as in test_wide_levels_refuse_*);
* POW2 = false (bounds 1.5 and 3: dyn_map's division) and POW2 = true with
  inv != 0.5 (bounds 0.5 and 2) of k_bin (fast_bin=0, and the hashed grid),
  k_bin_fast, k_walk, k_walk_flat, groups of 1 and 7; grid_encode_forward_dyn,
  grid_encode_backward_sliced_dyn: test_bound_*;
* W = 2 mask words of k_bin: test_wide_levels;
* MODE 1, MODE 2 with LevelRows::modulo, kModeAny, lead < 3:
  test_hand_built_layouts;
* f16 / bf16 gradients at C = 1, 2, 4 and k_sum's accumulate:
  test_binned_f16_gradients_and_accumulate, test_binned_bf16_*;
* the `tile += gridDim.x` loops and the 1,024-sample tile edge:
  test_binned_more_tiles_than_blocks, test_binned_tile_edge_sizes;
* dyn_count's clamps: test_binned_device_counts.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import oracle
from test_gpu_encoders import T, _samples

pytestmark = pytest.mark.gpu

Lay = namedtuple("Lay", "offs L C H S align")


def _lay_ref(align=False):
    """The 16-level reference layout (C = 2, 16 -> 2048, 2^16 rows)."""
    from gridencoder.grid import level_offsets
    pls = np.exp2(np.log2(2048 / 16) / 15)
    return Lay(level_offsets(16, 2, 3, 16, pls, 16, align), 16, 2, 16, float(np.log2(pls)), align)


def _lay_small(align=False):
    from gridencoder.grid import level_offsets
    return Lay(level_offsets(6, 2, 3, 4, 1.5, 12, align), 6, 2, 4, float(np.log2(1.5)), align)


def _lay_offsets(L, C, H, scale, log2T, align=False):
    from gridencoder.grid import level_offsets
    return Lay(level_offsets(L, C, 3, H, scale, log2T, align), L, C, H, float(np.log2(scale)),
               align)


def _lay_hand(rows, C=2):
    """Hand-built offsets, L = 3, H = 16, S = 1: the level spans are 17^3 =
    4,913, 33^3 = 35,937 and 65^3 = 274,625 rows."""
    offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return Lay(offs, len(rows), C, 16, 1.0, False)


LAYOUTS = {"ref": _lay_ref, "small": _lay_small}
HAND = {"modulo": [4000, 30000, 100000], "mixed": [4920, 30000, 65536],
        "no_z": [200, 35944, 65536]}


def _checks(x01, want, offs):
    """The two conditions of every case (module docstring)."""
    inside = np.all((x01 >= 0) & (x01 <= 1), axis=1)
    assert inside.mean() >= 0.9, inside.mean()
    for lvl in range(len(offs) - 1):
        assert np.count_nonzero(want[offs[lvl]:offs[lvl + 1]]) > 0, lvl


def _grads(B, lay, seed, dtype=np.float16):
    """[B, L*C] gradients (the oracle's blc form)."""
    return (np.random.default_rng(seed).normal(size=(B, lay.L * lay.C)) * 0.1).astype(dtype)


def _lbc(g, lay, gpu):
    """[B, L*C] host -> [L, B, C] device (the sliced / binned layout)."""
    B = g.shape[0]
    return T(g, gpu).view(B, lay.L, lay.C).transpose(0, 1).contiguous()


def _raw_samples(n, seed, bound):
    """Raw positions in [-bound, bound] with the edge rows of _samples, box
    faces and corners, and points just outside the box."""
    b = np.float32(bound)
    xr = (_samples(n, seed) * (2 * b) - b).astype(np.float32)
    up, down = np.nextafter(b, np.float32(np.inf)), np.nextafter(-b, np.float32(-np.inf))
    xr[8:14] = [[b, b, b], [-b, -b, -b], [b, 0, -b], [up, 0, 0], [0, down, 0],
                [b / 2, -b / 4, b / 8]]
    return xr


def _map01(xr, bound):
    """(x + bound) / (2 bound) in float32: the kernels' map, correctly rounded."""
    return ((xr + np.float32(bound)) / np.float32(2 * bound)).astype(np.float32)


def _stencil_rows(xr, eps, bound):
    """The seven rows per sample dfhip_shading_stencil lays out (f32): the
    sample, then clamp(x +- eps e_axis, -bound, bound), +eps first."""
    e, b = np.float32(eps), np.float32(bound)
    out = np.repeat(xr[:, None, :], 7, axis=1)
    for s in range(6):
        out[:, 1 + s, s >> 1] += -e if s & 1 else e
    out[:, 1:] = np.clip(out[:, 1:], -b, b)  # every coordinate of a moved point is clamped
    return out.reshape(-1, 3)


def _want(g, x01, lay, gt, blc=True, bf16=False):
    want = oracle.grid_encode_backward(g, x01, lay.offs, lay.C, lay.S, lay.H, gridtype=gt,
                                       align_corners=lay.align, blc=blc, bf16=bf16)
    _checks(x01, want, lay.offs)
    return want


def _close(got, want, rtol, atol_rel=1e-6):
    np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=rtol,
                               atol=atol_rel * np.abs(want).max())


def _binned(glbc, x, bound, lay, gt, B, m_dev, gpu, opts=None, accumulate=False, gemb=None,
            stencil_eps=None):
    """One binned backward call on fresh NaN-filled scratch; B counts samples
    (stencil groups: glbc holds 7 B rows per level)."""
    import _gridencoder
    rows = int(lay.offs[-1])
    ne, nc, npf = _gridencoder.grid_backward_binned_scratch(
        B, lay.offs, lay.L, lay.C, opts, group=1 if stencil_eps is None else 7)
    ent = torch.empty(ne, dtype=torch.int32, device=gpu)
    cnt = torch.empty(nc, dtype=torch.int32, device=gpu)
    part = torch.full((npf,), float("nan"), device=gpu)
    if gemb is None:
        gemb = torch.full((rows, lay.C), float("nan"), device=gpu)  # overwritten
    _gridencoder.grid_encode_backward_binned(glbc, x, bound, T(lay.offs, gpu), lay.offs, gemb, B,
                                             m_dev, 3, lay.C, lay.L, lay.S, lay.H, gt, lay.align,
                                             ent, cnt, part, accumulate,
                                             stencil_eps=stencil_eps, opts=opts)
    return gemb


def _sliced(glbc, x, bound, lay, gt, B, m_dev, gpu, dyn):
    import _gridencoder
    rows = int(lay.offs[-1])
    parts = 3
    partial = torch.full((_gridencoder.grid_backward_partial_floats(rows, lay.C, parts),),
                         float("nan"), device=gpu)
    gemb = torch.full((rows, lay.C), float("nan"), device=gpu)  # overwritten
    if dyn:
        _gridencoder.grid_encode_backward_sliced_dyn(glbc, x, bound, T(lay.offs, gpu), gemb, rows,
                                                     B, m_dev, 3, lay.C, lay.L, lay.S, lay.H, gt,
                                                     lay.align, partial, parts)
    else:
        _gridencoder.grid_encode_backward_sliced(glbc, x, T(lay.offs, gpu), gemb, rows, B, 3,
                                                 lay.C, lay.L, lay.S, lay.H, gt, lay.align,
                                                 partial, parts)
    return gemb


def _atomic(g, x01, lay, gt, gpu, acc=torch.float32):
    import _gridencoder
    B = x01.shape[0]
    gemb = torch.zeros(int(lay.offs[-1]), lay.C, dtype=acc, device=gpu)
    _gridencoder.grid_encode_backward_blc(T(g, gpu), T(x01, gpu), T(lay.offs, gpu), gemb, B, 3,
                                          lay.C, lay.L, lay.S, lay.H, None, None, gt, lay.align)
    return gemb


def _forward_exact(x01, lay, gt, gpu, seed, dtype=np.float32):
    """grid_encode_forward_blc on a random table, bit for bit."""
    import _gridencoder
    B = x01.shape[0]
    emb = (np.random.default_rng(seed).random((int(lay.offs[-1]), lay.C)) * 2 - 1).astype(dtype)
    out = torch.empty(B, lay.L * lay.C, device=gpu,
                      dtype=torch.float16 if dtype == np.float16 else torch.float32)
    _gridencoder.grid_encode_forward_blc(T(x01, gpu), T(emb, gpu), T(lay.offs, gpu), out, B, 3,
                                         lay.C, lay.L, lay.S, lay.H, None, gt, lay.align)
    want, _ = oracle.grid_encode_forward(x01, emb, lay.offs, lay.S, lay.H, gridtype=gt,
                                         align_corners=lay.align)
    assert np.count_nonzero(want) > 0.85 * want.size
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def _stencil_gpu(xr, m, eps, bound, gpu):
    """dfhip_shading_stencil's rows of the first m samples (checked against the
    f32 restatement the case was built from) and the device tensors."""
    import _dfhip
    cap = xr.shape[0]
    xt = T(xr, gpu)
    m_dev = torch.tensor([m], dtype=torch.int32, device=gpu)
    x7 = torch.full((7 * cap, 3), float("nan"), device=gpu)
    m7 = torch.zeros(1, dtype=torch.int32, device=gpu)
    _dfhip.call("dfhip_shading_stencil", xt.data_ptr(), m_dev.data_ptr(), cap, eps, bound,
                x7.data_ptr(), m7.data_ptr(), _dfhip.stream())
    assert int(m7.item()) == 7 * m
    np.testing.assert_array_equal(x7[:7 * m].cpu().numpy(), _stencil_rows(xr[:m], eps, bound))
    return xt, m_dev


def _opts(**kw):
    import _gridencoder
    return _gridencoder.BinnedOpts(**kw)


# ------------------------------------------------------------ a. align_corners

@functools.lru_cache(maxsize=None)
def _case_align(layout, gt):
    lay = LAYOUTS[layout](True)
    x = _samples(8000, 101)
    g = _grads(8000, lay, 102)
    return lay, x, g, _want(g, x, lay, gt)


@pytest.mark.parametrize("gt", [1, 0])
@pytest.mark.parametrize("layout", ["ref", "small"])
def test_align_corners_backward_paths(gpu, layout, gt):
    """align_corners=True through the forward, the atomic scatter (f32 table),
    the sliced backward and the binned rows (fast and generic binning, both
    walk forms) on level_offsets(..., True) layouts."""
    lay, x, g, want = _case_align(layout, gt)
    B = x.shape[0]
    _forward_exact(x, lay, gt, gpu, 103)
    _close(_atomic(g, x, lay, gt, gpu), want, 1e-4)
    glbc, xt = _lbc(g, lay, gpu), T(x, gpu)
    _close(_sliced(glbc, xt, 0.0, lay, gt, B, None, gpu, dyn=False), want, 1e-5)
    for kw in ({"fast_bin": 1}, {"fast_bin": 0}, {"walk_mode": 0}, {"walk_mode": 1}):
        _close(_binned(glbc, xt, 0.0, lay, gt, B, None, gpu, opts=_opts(**kw)), want, 1e-5)


@functools.lru_cache(maxsize=None)
def _case_align_f16(layout, gt):
    lay, x, g, want = _case_align(layout, gt)
    if layout == "small":
        x, g = x[:170], g[:170]
        want = _want(g, x, lay, gt)
    return lay, x, g, want


@pytest.mark.parametrize("gt", [1, 0])
@pytest.mark.parametrize("layout", ["ref", "small"])
def test_align_corners_atomic_f16_table(gpu, layout, gt):
    """The reference's half2 atomics at align_corners=True.  The bound is the
    one test_grid_backward derives for running half sums of about 50 adds per
    coarse row (30,000 samples on 17^3 lattice points): every add rounds the
    running sum to half, an error of about |sum| 2^-11 sqrt(adds / 3).  The
    reference layout keeps to that at 8,000 samples.  The small layout's
    coarsest level has 4^3 lattice points: 8,000 samples are about 1,800 adds
    on an inner row, and the measured error there (0.019 tiled, 0.018 hashed,
    all of it in levels 0 and 1, against a bound of 0.0106) is that rounding,
    not the kernel, so here the batch is the point: the first 170 samples of
    the case, about 50 adds per row, under the same bound."""
    lay, x, g, want = _case_align_f16(layout, gt)
    got = _atomic(g, x, lay, gt, gpu, acc=torch.float16).double().cpu().numpy()
    assert np.abs(got - want).max() <= 4e-3 * np.abs(want).max() + 1e-3


@functools.lru_cache(maxsize=None)
def _case_align_stencil(layout):
    lay = LAYOUTS[layout](True)
    cap, m, eps, bound = 6000, 5321, 1e-2, 1.0
    xr = _raw_samples(cap, 111, bound)
    xr[20:70, 0] = np.float32(bound)    # on the +x face: the +x stencil point clamps
    xr[70:120, 2] = np.float32(-bound)
    g7 = _grads(7 * cap, lay, 112)
    x01 = _map01(_stencil_rows(xr[:m], eps, bound), bound)
    return lay, xr, m, eps, bound, g7, _want(g7[:7 * m], x01, lay, 1)


@pytest.mark.parametrize("layout", ["ref", "small"])
def test_align_corners_stencil_groups(gpu, layout):
    """Binned 7-point stencil groups at align_corners=True (tiled: the mask
    form the groups need), both walk forms, against the oracle over the seven
    rows per sample dfhip_shading_stencil lays out."""
    lay, xr, m, eps, bound, g7, want = _case_align_stencil(layout)
    cap = xr.shape[0]
    xt, m_dev = _stencil_gpu(xr, m, eps, bound, gpu)
    glbc = _lbc(g7, lay, gpu)
    for kw in ({}, {"walk_mode": 0}, {"walk_mode": 1}):
        got = _binned(glbc, xt, bound, lay, 1, cap, m_dev, gpu, opts=_opts(**kw),
                      stencil_eps=eps)
        _close(got, want, 1e-5)
    # the hashed grid's capped levels are not the mask form: refused, not walked
    with pytest.raises(RuntimeError, match="mask-form level layout"):
        _binned(glbc, xt, bound, lay, 0, cap, m_dev, gpu, stencil_eps=eps)


@pytest.mark.parametrize("gt", [1, 0])
def test_align_corners_fast_bins_equal_generic(gpu, gt):
    """test_grid_backward_fast_bins_equal_generic with align_corners on: the
    fast and the generic binning file the same counts and id sets."""
    import _gridencoder
    lay = _lay_ref(True)
    rows = int(lay.offs[-1])
    x = _samples(9000, 121)
    x[8:72] = np.float32(1.0)
    x[72:136] = np.float32(0.0)
    B = x.shape[0]
    glbc, xt = _lbc(_grads(B, lay, 122), lay, gpu), T(x, gpu)
    ne, nc, npf = _gridencoder.grid_backward_binned_scratch(B, lay.offs, 16, 2)
    got = {}
    for fast in (0, 1):
        ent = torch.zeros(ne, dtype=torch.int32, device=gpu)
        cnt = torch.zeros(nc, dtype=torch.int32, device=gpu)
        part = torch.empty(npf, device=gpu)
        gemb = torch.empty(rows, 2, device=gpu)
        _gridencoder.binned_launcher(glbc, xt, 0.0, T(lay.offs, gpu), lay.offs, gemb, B, None, 3,
                                     2, 16, lay.S, 16, gt, True, ent, cnt, part,
                                     opts=_opts(fast_bin=fast))()
        torch.cuda.synchronize()
        got[fast] = (ent.cpu().numpy().view(np.uint16), cnt.cpu().numpy(), gemb.cpu().numpy())
    tsz = _gridencoder.grid_backward_binned_tile()
    tiles = -(-B // tsz)
    (e0, c0, g0), (e1, c1, g1) = got[0], got[1]
    nb = int(sum(-(-int(lay.offs[l + 1] - lay.offs[l]) // 8192) for l in range(16)))
    assert np.array_equal(c0[:tiles * nb], c1[:tiles * nb])
    assert c0[:tiles * nb].sum() >= 16 * (B - 2)  # every in-range sample, every level
    for t in range(tiles):
        for b in range(nb):
            n = int(c0[t * nb + b])
            base = (t * nb + b) * tsz
            assert np.array_equal(np.sort(e0[base:base + n]), np.sort(e1[base:base + n])), (t, b)
    np.testing.assert_allclose(g1, g0, rtol=1e-6, atol=1e-9)


@functools.lru_cache(maxsize=None)
def _case_align_edge(gt):
    # Level 0: scale 19 (an integer) and 20^3 = 8,000 rows, dense and no power
    # of two.  With align_corners a sample at x = 1 sits on the last lattice
    # point and its +1 corner (weight exactly 0) has coordinate 20 = the stride,
    # so on the z = 1 face the tiled index reaches 8,000 + 20 y + x: past the
    # level's rows, and from y = 10 on past its one 8,192-row slice.  The
    # reference wraps it (% 8,000); a slice number taken from the unwrapped
    # index names a bin of level 1 (one slice of 8,192 rows, where the sample
    # is filed anyway: walked twice there).  The face samples sit in the last,
    # partly filled tile.
    lay = _lay_offsets(2, 2, 20, 2.0, 13, True)
    assert lay.offs.tolist() == [0, 8000, 16192]
    x = _samples(7000, 131)
    x[1] = [1, 1, 0.5]
    face = np.random.default_rng(132).random((24, 3), dtype=np.float32)
    face[:, 2] = 1
    face[:4] = [[1, 1, 1], [0, 1, 1], [1, 0.5, 1], [0.75, 1, 1]]
    x[-24:] = face
    g = _grads(7000, lay, 133)
    return lay, x, g, _want(g, x, lay, gt)


@pytest.mark.parametrize("gt", [1, 0])
def test_align_corners_zero_weight_corner_past_level(gpu, gt):
    """align_corners=True on a dense level with an integer scale: samples on
    the far faces have zero-weight corners whose tiled index lies past the
    level's rows; every path wraps them as the reference does."""
    lay, x, g, want = _case_align_edge(gt)
    B = x.shape[0]
    _forward_exact(x, lay, gt, gpu, 134)
    _close(_atomic(g, x, lay, gt, gpu), want, 1e-4)
    glbc, xt = _lbc(g, lay, gpu), T(x, gpu)
    _close(_sliced(glbc, xt, 0.0, lay, gt, B, None, gpu, dyn=False), want, 1e-5)
    for kw in ({"fast_bin": 1}, {"fast_bin": 0}, {"walk_mode": 0}, {"walk_mode": 1}):
        _close(_binned(glbc, xt, 0.0, lay, gt, B, None, gpu, opts=_opts(**kw)), want, 1e-5)


# ------------------------------------------------------------ b. bounds != 1

BOUNDS = [0.5, 1.5, 2.0, 3.0]


@functools.lru_cache(maxsize=None)
def _case_bound(bound, counted, align=False):
    lay = _lay_ref(align)
    cap = 8000
    m = 6789 if counted else cap
    xr = _raw_samples(cap, 201, bound)
    x01 = _map01(xr, bound)
    g = _grads(cap, lay, 202)
    return lay, xr, x01, m, g, {gt: _want(g[:m], x01[:m], lay, gt) for gt in (1, 0)}


def _forward_dyn_exact(lay, xr, x01, m, bound, counted, gpu):
    import _gridencoder
    cap = xr.shape[0]
    m_dev = torch.tensor([m], dtype=torch.int32, device=gpu) if counted else None
    for dtype, gt in ((np.float32, 1), (np.float16, 1), (np.float32, 0), (np.float16, 0)):
        emb = (np.random.default_rng(203).random((int(lay.offs[-1]), 2)) * 2 - 1).astype(dtype)
        td = torch.float16 if dtype == np.float16 else torch.float32
        out = torch.full((cap, 32), float("nan"), dtype=td, device=gpu)
        _gridencoder.grid_encode_forward_dyn(T(xr, gpu), bound, T(emb, gpu), T(lay.offs, gpu),
                                             out, cap, m_dev, 3, 2, 16, lay.S, 16, None, gt,
                                             lay.align)
        want, _ = oracle.grid_encode_forward(x01[:m], emb, lay.offs, lay.S, 16, gridtype=gt,
                                             align_corners=lay.align)
        got = out.cpu().numpy()
        assert np.count_nonzero(want) > 0.85 * want.size
        np.testing.assert_array_equal(got[:m], want)
        assert np.all(got[m:] == 0)  # rows past the count: exactly zero


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("bound", BOUNDS)
def test_bound_forward_dyn(gpu, bound, counted):
    """grid_encode_forward_dyn maps raw positions (x + bound) / (2 bound) bit
    for bit (the correctly rounded f32 operations), f32 and f16 tables, tiled
    and hashed; rows past the device count are exactly zero."""
    lay, xr, x01, m, _, _ = _case_bound(bound, counted)
    _forward_dyn_exact(lay, xr, x01, m, bound, counted, gpu)


def _bound_backwards(lay, xr, m, g, wants, bound, counted, gpu):
    cap = xr.shape[0]
    m_dev = torch.tensor([m], dtype=torch.int32, device=gpu) if counted else None
    glbc, xt = _lbc(g, lay, gpu), T(xr, gpu)
    for gt in (1, 0):
        _close(_sliced(glbc, xt, bound, lay, gt, cap, m_dev, gpu, dyn=True), wants[gt], 1e-5)
    # tiled: fast binning + per-segment walk (default), generic binning, both
    # walk forms; hashed: the generic binning and the any-mode walk
    for gt, kw in ((1, {}), (1, {"fast_bin": 0}), (1, {"walk_mode": 0}), (1, {"walk_mode": 1}),
                   (0, {})):
        got = _binned(glbc, xt, bound, lay, gt, cap, m_dev, gpu, opts=_opts(**kw))
        _close(got, wants[gt], 1e-5)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("bound", BOUNDS)
def test_bound_backward_paths(gpu, bound, counted):
    """grid_encode_backward_sliced_dyn and the binned rows on raw positions in
    [-bound, bound], with and without a device count."""
    lay, xr, _, m, g, wants = _case_bound(bound, counted)
    _bound_backwards(lay, xr, m, g, wants, bound, counted, gpu)


@functools.lru_cache(maxsize=None)
def _case_bound_stencil(bound, counted, align=False):
    lay = _lay_ref(align)
    cap, eps = 6000, 1e-2
    m = 5321 if counted else cap
    xr = _raw_samples(cap, 211, bound)
    xr[20:70, 1] = np.float32(bound)    # on the box faces: the outward point clamps
    xr[70:120, 0] = np.float32(-bound)
    g7 = _grads(7 * cap, lay, 212)
    x01 = _map01(_stencil_rows(xr[:m], eps, bound), bound)
    return lay, xr, m, eps, g7, _want(g7[:7 * m], x01, lay, 1)


def _bound_stencil(lay, xr, m, eps, g7, want, bound, counted, gpu):
    cap = xr.shape[0]
    xt, m_dev = _stencil_gpu(xr, m, eps, bound, gpu)
    glbc = _lbc(g7, lay, gpu)
    for kw in ({"walk_mode": 0}, {"walk_mode": 1}):
        got = _binned(glbc, xt, bound, lay, 1, cap, m_dev if counted else None, gpu,
                      opts=_opts(**kw), stencil_eps=eps)
        _close(got, want, 1e-5)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("bound", BOUNDS)
def test_bound_stencil_groups(gpu, bound, counted):
    """Binned stencil groups with dfhip_shading_stencil called at the same
    bound, samples on the box faces, both walk forms."""
    lay, xr, m, eps, g7, want = _case_bound_stencil(bound, counted)
    _bound_stencil(lay, xr, m, eps, g7, want, bound, counted, gpu)


def test_bound_with_align_corners(gpu):
    """Bound 1.5 (a division, no exact reciprocal) with align_corners=True
    through every dynamic entry point."""
    lay, xr, x01, m, g, wants = _case_bound(1.5, True, True)
    _forward_dyn_exact(lay, xr, x01, m, 1.5, True, gpu)
    _bound_backwards(lay, xr, m, g, wants, 1.5, True, gpu)
    lay, xr, m, eps, g7, want = _case_bound_stencil(1.5, True, True)
    _bound_stencil(lay, xr, m, eps, g7, want, 1.5, True, gpu)


# ------------------------------------------------------------ c. wide levels

@functools.lru_cache(maxsize=1)
def _case_wide(C, gt):
    # C = 2: 8,192-row slices, 2^20 rows; C = 4: 4,096-row slices, 2^19 rows:
    # levels 1 to 3 have 128 slices (the two-word slice masks of k_bin)
    lay = _lay_offsets(4, C, 64, 2.0, 20 if C == 2 else 19)
    assert (int(lay.offs[2] - lay.offs[1]) * C * 8) // (128 * 1024) == 128
    x = _samples(7000, 301)
    g = _grads(7000, lay, 302)
    return lay, x, g, _want(g, x, lay, gt)


@pytest.mark.parametrize("gt", [1, 0])
@pytest.mark.parametrize("C", [2, 4])
def test_wide_levels(gpu, C, gt):
    lay, x, g, want = _case_wide(C, gt)
    _forward_exact(x, lay, gt, gpu, 303)
    _close(_binned(_lbc(g, lay, gpu), T(x, gpu), 0.0, lay, gt, x.shape[0], None, gpu), want, 1e-5)


def test_wide_levels_refuse_stencil_groups(gpu):
    """Stencil groups need the mask-form fast layout (at most 64 slices per
    level): the call raises, and the next default call is unaffected."""
    lay, x, g, want = _case_wide(2, 1)
    cap = 1000
    xr = (x[:cap] * 2 - 1).astype(np.float32)
    g7 = _lbc(_grads(7 * cap, lay, 304), lay, gpu)
    with pytest.raises(RuntimeError, match="mask-form level layout"):
        _binned(g7, T(xr, gpu), 1.0, lay, 1, cap, None, gpu, stencil_eps=1e-2)
    _close(_binned(_lbc(g, lay, gpu), T(x, gpu), 0.0, lay, 1, x.shape[0], None, gpu), want, 1e-5)


# ------------------------------------------------------------ d. hand-built layouts

@functools.lru_cache(maxsize=None)
def _case_hand(name, gt):
    lay = _lay_hand(HAND[name])
    x = _samples(7000, 401)
    g = _grads(7000, lay, 402)
    return lay, x, g, _want(g, x, lay, gt)


@pytest.mark.parametrize("gt", [1, 0])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_layouts(gpu, name, gt):
    """Offsets level_offsets never produces: levels smaller than their tiled
    span and no power of two wrap by modulo ("modulo": every level; "mixed":
    one dense, one modulo, one masked level, so the walk takes its any-mode
    form; "no_z": a 200-row level whose tiled index stops before z)."""
    lay, x, g, want = _case_hand(name, gt)
    B = x.shape[0]
    _forward_exact(x, lay, gt, gpu, 403)
    _close(_atomic(g, x, lay, gt, gpu), want, 1e-4)
    glbc, xt = _lbc(g, lay, gpu), T(x, gpu)
    _close(_sliced(glbc, xt, 0.0, lay, gt, B, None, gpu, dyn=False), want, 1e-5)
    for kw in ({}, {"fast_bin": 0, "walk_mode": 1}):
        _close(_binned(glbc, xt, 0.0, lay, gt, B, None, gpu, opts=_opts(**kw)), want, 1e-5)


# ------------------------------------------------------------ e. channels and types

def _lay_channels(C):
    return _lay_offsets(8, 1, 4, 2.0, 17) if C == 1 else _lay_offsets(6, 4, 8, 2.0, 15)


@functools.lru_cache(maxsize=None)
def _case_channels(C):
    lay = _lay_channels(C)
    x = _samples(7000, 501)
    g = _grads(7000, lay, 502)
    return lay, x, g, _want(g, x, lay, 1)


@pytest.mark.parametrize("C", [1, 4])
def test_binned_f16_gradients_and_accumulate(gpu, C):
    """f16 gradients through the C = 1 and C = 4 walks, and accumulate=True
    through k_sum (C != 2): the second call gives twice the oracle."""
    lay, x, g, want = _case_channels(C)
    B = x.shape[0]
    glbc, xt = _lbc(g, lay, gpu), T(x, gpu)
    gemb = _binned(glbc, xt, 0.0, lay, 1, B, None, gpu)
    _close(gemb, want, 1e-5)
    _binned(glbc, xt, 0.0, lay, 1, B, None, gpu, accumulate=True, gemb=gemb)
    _close(gemb, 2 * want, 1e-5)
    # f32 gradients accumulate the same way
    g32 = g.astype(np.float32)
    gemb = torch.zeros(int(lay.offs[-1]), C, device=gpu)
    for k in (1, 2):
        _binned(_lbc(g32, lay, gpu), xt, 0.0, lay, 1, B, None, gpu, accumulate=True, gemb=gemb)
        _close(gemb, k * want, 1e-5)


@functools.lru_cache(maxsize=None)
def _case_bf16():
    lay = _lay_ref(True)
    x = _samples(8000, 511)
    bits = oracle.to_bf16_bits(_grads(8000, lay, 512, np.float32))
    return lay, x, bits, _want(bits, x, lay, 1, bf16=True)


def _bf16(bits, gpu):
    return torch.from_numpy(bits.view(np.int16)).to(gpu).view(torch.bfloat16)


def test_binned_bf16_gradients_align_corners(gpu):
    lay, x, bits, want = _case_bf16()
    B = x.shape[0]
    glbc = _bf16(bits, gpu).view(B, 16, 2).transpose(0, 1).contiguous()
    for kw in ({}, {"walk_mode": 1}):
        _close(_binned(glbc, T(x, gpu), 0.0, lay, 1, B, None, gpu, opts=_opts(**kw)), want, 1e-5)


def test_binned_bf16_four_channels_raises(gpu):
    lay = _lay_channels(4)
    B = 500
    g = torch.zeros(lay.L, B, 4, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError, match="bf16 gradients are supported for C = 2"):
        _binned(g, T(_samples(B, 521), gpu), 0.0, lay, 1, B, None, gpu)


# ------------------------------------------------------------ f. sizes and counts

@functools.lru_cache(maxsize=None)
def _case_sizes():
    lay = _lay_ref()
    x = _samples(3000, 601, edge=False)
    x[2048:2056] = _samples(8, 0)[:8]  # the edge rows, past every tile-edge size below
    xr = (x * np.float32(4) - np.float32(2)).astype(np.float32)  # raw positions at bound 2
    g = _grads(3000, lay, 602)
    return lay, _map01(xr, 2.0), xr, g


@functools.lru_cache(maxsize=None)
def _want_first(m):
    lay, x, _, g = _case_sizes()
    return _want(g[:m], x[:m], lay, 1)


@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 2048])
def test_binned_tile_edge_sizes(gpu, B):
    """Batches at the 1,024-sample binning tile edge."""
    lay, x, _, g = _case_sizes()
    got = _binned(_lbc(g[:B], lay, gpu), T(x[:B], gpu), 0.0, lay, 1, B, None, gpu)
    _close(got, _want_first(B), 1e-5)


@pytest.mark.parametrize("m", [0, 1, 3000, 3005, -3])
def test_binned_device_counts(gpu, m):
    """Device counts on a capacity of 3,000: 0 and a negative count walk
    nothing (the output is all zero), a count above the capacity is clamped."""
    lay, _, xr, g = _case_sizes()
    cap = xr.shape[0]
    live = min(max(m, 0), cap)
    m_dev = torch.tensor([m], dtype=torch.int32, device=gpu)
    bound = 2.0
    for kw in ({}, {"fast_bin": 0}):
        got = _binned(_lbc(g, lay, gpu), T(xr, gpu), bound, lay, 1, cap, m_dev, gpu,
                      opts=_opts(**kw))
        if live == 0:
            assert torch.all(got == 0)
        else:
            _close(got, _want_first(live), 1e-5)


def _case_many_tiles():
    # two bins (128 + 736 rows), 4,098 tiles: past the 4,096-block grid of the
    # binning kernels, so their `tile += gridDim.x` loops take a second trip
    lay = _lay_offsets(2, 2, 4, 2.0, 12)
    B = 4096 * 1024 + 1500
    rng = np.random.default_rng(611)
    x = rng.random((B, 3), dtype=np.float32)
    x[:8] = _samples(8, 0)
    x[-3:] = [[1, 1, 1], [0, 0, 0], [0.5, 1, 0]]
    g = (rng.standard_normal((lay.L, B, 2), dtype=np.float32) * 0.1).astype(np.float16)
    want = oracle.grid_encode_backward(g, x, lay.offs, 2, lay.S, lay.H, blc=False)
    _checks(x, want, lay.offs)
    return lay, x, g, want


def test_binned_more_tiles_than_blocks(gpu):
    lay, x, g, want = _case_many_tiles()
    B = x.shape[0]
    glbc, xt = T(g, gpu), T(x, gpu)
    for fast in (1, 0):
        _close(_binned(glbc, xt, 0.0, lay, 1, B, None, gpu, opts=_opts(fast_bin=fast)), want, 1e-5)


# ------------------------------------------------------------ g. module level

ENCODERS = {"tiled_align": dict(align_corners=True, gridtype="tiled"),
            "hash_2p16": dict(gridtype="hash", log2_hashmap_size=16)}


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("bound", [2.0, 1.5])
@pytest.mark.parametrize("name", sorted(ENCODERS))
def test_module_bound_and_align(gpu, name, bound, half):
    """GridEncoder(x, bound=...) with raw positions: the output bit for bit,
    embeddings.grad of both backward modes against the oracle, and the two
    modes against each other; f32 and under f16 autocast (half table; the
    atomic mode then accumulates in half)."""
    from gridencoder import GridEncoder
    torch.manual_seed(700)
    enc = GridEncoder(**ENCODERS[name]).to(gpu)
    with torch.no_grad():
        enc.embeddings.uniform_(-0.5, 0.5)
    lay = Lay(enc.offsets_host, 16, 2, 16, float(np.log2(enc.per_level_scale)),
              enc.align_corners)
    gt = enc.gridtype_id
    xr = _raw_samples(8000, 701, bound)
    x01 = _map01(xr, bound)
    emb = enc.embeddings.detach()
    emb = (emb.half() if half else emb).cpu().numpy()
    want, _ = oracle.grid_encode_forward(x01, emb, lay.offs, lay.S, 16, gridtype=gt,
                                         align_corners=lay.align)
    gout = _grads(8000, lay, 702, np.float16 if half else np.float32)
    wantg = _want(gout, x01, lay, gt)
    scale = np.abs(wantg).max()
    grads = {}
    for mode in ("binned", "atomic"):
        enc.backward_mode = mode
        enc.embeddings.grad = None
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            y = enc(T(xr, gpu), bound=bound)
        assert y.dtype == (torch.float16 if half else torch.float32)
        np.testing.assert_array_equal(y.detach().cpu().numpy(), want)
        (y.float() * T(gout, gpu).float()).sum().backward()
        assert enc.embeddings.grad.dtype == torch.float32
        grads[mode] = enc.embeddings.grad.double().cpu().numpy()
    np.testing.assert_allclose(grads["binned"], wantg, rtol=1e-5, atol=1e-6 * scale)
    if half:
        assert np.abs(grads["atomic"] - wantg).max() <= 4e-3 * scale + 1e-3
        assert np.abs(grads["atomic"] - grads["binned"]).max() <= 4e-3 * scale + 1e-3
    else:
        np.testing.assert_allclose(grads["atomic"], wantg, rtol=1e-4, atol=1e-6 * scale)
        np.testing.assert_allclose(grads["atomic"], grads["binned"], rtol=1e-4, atol=1e-6 * scale)
