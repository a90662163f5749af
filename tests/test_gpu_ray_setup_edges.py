"""The three small ray entries at their edges, against a truth that is not GPU
code (tests/prologue_cases.py):

* dfhip_get_rays (csrc/camera.hip) on the prologue's cases: rays_d within
  8 * 2^-24 of the float64 camera and of unit length, rays_o exact, an empty
  image and a zero focal length;
* dfhip_near_far_from_aabb in f32, f16 and f64: bit-equal to the C oracle on
  the inputs as f32, rounded to the storage type (a NaN equals a NaN); misses
  are the storage type's largest finite value;
* dfhip_sph_from_ray in f32 against the documented formula at float64, allowed
  3 x the C oracle's own error on the same rows (atan2f / sqrtf differ between
  libm and the device library; the ratio test_gpu_run_native.py uses), phi
  compared on the circle; f16 / f64 storage is the f32 result rounded / widened.

Outputs carry 64 sentinel elements of padding that must survive.  Tests print
`edges:` lines (kept in profiles/prologue/edges.txt)."""
import numpy as np
import pytest
import torch

import oracle
import prologue_cases as pc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SLACK = 64
CASES = pc.cases()
DTYPES = [torch.float32, torch.float16, torch.float64]
IDS = ["f32", "f16", "f64"]
NP = {torch.float32: np.float32, torch.float16: np.float16, torch.float64: np.float64}
INT = {torch.float32: (torch.int32, 0x5EA7BEEF), torch.float16: (torch.int16, 0x5A5A),
       torch.float64: (torch.int64, 0x5EA7BEEF5EA7BEEF)}
MISS = {torch.float32: pc.FLT_MAX, torch.float16: 65504.0, torch.float64: float(np.finfo(F64).max)}


def _sentinel(n, dtype, gpu):
    it, pat = INT[dtype]
    return torch.full((n + SLACK,), pat, dtype=it, device=gpu)


def _read(buf, n, dtype):
    """(the first n elements as numpy values of `dtype`, padding intact?)"""
    raw = buf.cpu().numpy()
    return raw[:n].view(NP[dtype]), bool((raw[n:] == INT[dtype][1]).all())


def _same(a, b):
    """Bit-equal, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------- dfhip_get_rays

def _get_rays(gpu, c, H=None, W=None, fx=None, n_alloc=None):
    import _dfhip
    n = c.N if n_alloc is None else n_alloc
    o, d = _sentinel(3 * n, torch.float32, gpu), _sentinel(3 * n, torch.float32, gpu)
    _dfhip.call("dfhip_get_rays", c.pose.ctypes.data, c.fx if fx is None else fx, c.fy, c.cx,
                c.cy, c.H if H is None else H, c.W if W is None else W, o.data_ptr(),
                d.data_ptr(), _dfhip.stream())
    torch.cuda.synchronize()
    return o, d


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_get_rays_against_the_f64_camera(gpu, c):
    bo, bd = _get_rays(gpu, c)
    (o, ok_o), (d, ok_d) = _read(bo, 3 * c.N, torch.float32), _read(bd, 3 * c.N, torch.float32)
    assert ok_o and ok_d, "written past H * W rays"
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    o64, d64 = pc.pixel_rays64(c.pose, *c.intr(), c.H, c.W)
    assert np.array_equal(o.astype(F64), o64)
    err = float(np.abs(d.astype(F64) - d64).max()) / pc.U24
    length = float(np.abs(np.linalg.norm(d.astype(F64), axis=1) - 1).max()) / pc.U24
    print(f"\nedges: [get_rays {c.name}] rays_d {err:.2f} of {pc.DIR_UNITS} units of 2^-24, "
          f"| |rays_d| - 1 | {length:.2f} of 4 units")
    assert err <= pc.DIR_UNITS, err
    assert length <= 4, length
    if "zero" in c.named:
        assert (d == 0).any()


def test_get_rays_empty_image_and_zero_focal(gpu):
    c = next(x for x in CASES if x.name == "random-16x16-fov120")
    for kw in (dict(H=0), dict(W=0)):
        bo, bd = _get_rays(gpu, c, n_alloc=1, **kw)
        assert _read(bo, 0, torch.float32)[1] and _read(bd, 0, torch.float32)[1]
    for fx in (0.0, -0.0):
        with pytest.raises(RuntimeError, match=r"dfhip_get_rays failed \(1\): get_rays: focal "
                                               r"lengths must be non-zero"):
            _get_rays(gpu, c, fx=fx)


# ---------------------------------------------------------------- dfhip_near_far_from_aabb

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("degenerate", [False, True], ids=["box", "flatbox"])
@pytest.mark.parametrize("min_near", [0.05, 0.2, 0.0])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_near_far_is_the_oracle_in_every_storage_type(gpu, N, min_near, degenerate, dtype):
    import _dfhip
    o, d, aabb, kind = pc.near_far_rows(N, 3, degenerate)   # f32 values, exact in f16
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ne, fa = oracle.near_far_from_aabb(o, d, aabb, min_near)
        miss = (ne == F32(pc.FLT_MAX)) & (fa == F32(pc.FLT_MAX))
        want_ne, want_fa = ne.astype(NP[dtype]), fa.astype(NP[dtype])
    want_ne[miss] = want_fa[miss] = MISS[dtype]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(dtype).contiguous()  # noqa: E731
    to, td, tb = dev(o), dev(d), dev(aabb)
    assert np.array_equal(to.cpu().numpy().astype(F32), o)   # the storage type holds the rows
    bn, bf = _sentinel(N, dtype, gpu), _sentinel(N, dtype, gpu)
    _dfhip.call("dfhip_near_far_from_aabb", _dfhip._DTYPE[dtype], to.data_ptr(), td.data_ptr(),
                tb.data_ptr(), N, min_near, bn.data_ptr(), bf.data_ptr(), _dfhip.stream())
    torch.cuda.synchronize()
    (got_ne, ok_n), (got_fa, ok_f) = _read(bn, N, dtype), _read(bf, N, dtype)
    assert ok_n and ok_f, "written past N rays"
    bad = np.flatnonzero(~(_same(got_ne, want_ne) & _same(got_fa, want_fa)))
    assert bad.size == 0, (f"rows {bad[:5]} (kinds {[pc.NEAR_FAR_KINDS[k] for k in kind[bad[:5]]]}): "
                           f"got {got_ne[bad[:5]]} / {got_fa[bad[:5]]}, want {want_ne[bad[:5]]} / "
                           f"{want_fa[bad[:5]]}")
    if N >= 255:
        assert miss.any() and (got_ne[miss] == NP[dtype](MISS[dtype])).all()
        assert np.isnan(got_ne).any() or np.isnan(got_fa).any()   # the 0 * inf slabs
        hit = ~miss & ~np.isnan(got_ne) & ~np.isnan(got_fa)
        if min_near > 0.0625:
            assert (got_ne[hit] > got_fa[hit]).any()   # near = min_near past the exit


def test_near_far_no_rays(gpu):
    import _dfhip
    bn, bf = _sentinel(0, torch.float32, gpu), _sentinel(0, torch.float32, gpu)
    x = torch.zeros(6, device=gpu)
    _dfhip.call("dfhip_near_far_from_aabb", _dfhip.F32, x.data_ptr(), x.data_ptr(), x.data_ptr(),
                0, 0.2, bn.data_ptr(), bf.data_ptr(), _dfhip.stream())
    torch.cuda.synchronize()
    assert _read(bn, 0, torch.float32)[1] and _read(bf, 0, torch.float32)[1]


# ---------------------------------------------------------------- dfhip_sph_from_ray

def _sph(gpu, o, d, dtype):
    import _dfhip
    N = o.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(dtype).contiguous()  # noqa: E731
    to, td = dev(o), dev(d)
    out = _sentinel(2 * N, dtype, gpu)
    _dfhip.call("dfhip_sph_from_ray", _dfhip._DTYPE[dtype], to.data_ptr(), td.data_ptr(),
                pc.SPH_RADIUS, N, out.data_ptr(), _dfhip.stream())
    torch.cuda.synchronize()
    got, ok = _read(out, 2 * N, dtype)
    assert ok, "written past N rays"
    return got.reshape(N, 2)


_SPH = {}


def _sph_reference():
    """The 257 rows, their float64 truth and the C oracle's error on them,
    computed once.  Smaller launches take a prefix of the same rows, so the
    one measured allowance holds for all of them."""
    if not _SPH:
        o, d, kind = pc.sph_rows(257, 4)
        want, margin = pc.sph_truth(o, d, pc.SPH_RADIUS)
        assert (margin > 1e-6).all()
        orc = oracle.sph_from_ray(o, d, pc.SPH_RADIUS)
        _SPH.update(o=o, d=d, kind=kind, want=want, orc=orc, e_orc=pc.sph_errors(orc, want, kind))
    return _SPH


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_sph_from_ray_against_the_f64_formula(gpu, N):
    ref = _sph_reference()
    o, d, want, kind, e_orc = (ref["o"][:N], ref["d"][:N], ref["want"][:N], ref["kind"][:N],
                               ref["e_orc"])
    got = _sph(gpu, o, d, torch.float32)
    assert np.isfinite(got).all() and (np.abs(got) <= 1).all()
    e_got = pc.sph_errors(got, want, kind)
    # rows aimed at a pole: their phi is compared with the C oracle's, which
    # performs the same f32 operations on the same x and z up to atan2f, at
    # most 2 ulp of pi from the exact value on either side: 4 * 2^-23
    pole = ~pc.sph_phi_rows(kind)
    e_pole = float(pc.circle_distance(got[pole, 1], ref["orc"][:N][pole, 1]).max()) if pole.any() else 0.0
    print(f"\nedges: [sph_from_ray N {N}] theta: native {e_got[0]:.3e} oracle {e_orc[0]:.3e}; "
          f"phi (on the circle): native {e_got[1]:.3e} oracle {e_orc[1]:.3e}; allowed 3 x oracle; "
          f"phi of the pole rows, native vs oracle {e_pole:.3e} (allowed {4 * 2.0 ** -23:.3e})")
    for what, g, r in zip(("theta", "phi"), e_got, e_orc):
        assert g <= 3 * r, (what, g, r)
    assert e_pole <= 4 * 2.0 ** -23, e_pole
    # f16 / f64 storage: the f32 result rounded / widened
    with np.errstate(over="ignore"):
        want16 = got.astype(np.float16)
    assert _same(_sph(gpu, o, d, torch.float16), want16).all()
    assert _same(_sph(gpu, o, d, torch.float64), got.astype(F64)).all()
