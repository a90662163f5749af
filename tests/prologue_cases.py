"""The truth of the train-step prologue (csrc/step.hip, k_step_prologue) and of
the three small ray entries (dfhip_get_rays, dfhip_near_far_from_aabb,
dfhip_sph_from_ray) in numpy, with the cases both test files run: the CPU check
(test_prologue_cases_host.py) and the GPU comparisons
(test_gpu_prologue_edges.py, test_gpu_ray_setup_edges.py).

Draws (include/dfhip.h writes them out): Philox4x32-10 with key (seed_lo,
seed_hi) and counter (ray, step_lo, step_hi, stream); r0 is stream 0, r1 stream
1 of a ray, and counter (0xFFFFFFFF, step_lo, step_hi, 2) gives the step's t.
unit(v) = (v >> 8) * 2^-24 is exact in f32, so noise and bg have one value in
every precision; the Box-Muller values are evaluated at float64 (the
specification) and at float32 (the device's operations, its f32 2 pi).

Camera: cam::pixel_ray (csrc/camera_common.h) at float64 from the f32 pose and
intrinsics, and at float32 in the kernel's operation order.
"""
import numpy as np

from shading_cases import philox4x32_10

F32, F64 = np.float32, np.float64
_MASK = 0xFFFFFFFF
U24 = 2.0 ** -24
TWO_PI_F32 = F32(6.2831855)     # the device's 6.283185307179586f
FLT_MAX = float(np.finfo(F32).max)

# The Philox words (stream, word) behind the seven per-ray outputs; draws()
# reads the words through this table.  A uniform output reads one word; a
# normal output reads (radius word, angle word).  eps0 / eps1 are the cosine and
# the sine of ONE Box-Muller pair and so share their two words by construction;
# eps2 is the cosine of a second pair (its sine is not used), and r1's pair is
# (r1.x, r1.y).
UNIFORM_WORDS = {"noise": (0, 0), "bg0": (0, 3), "bg1": (1, 2), "bg2": (1, 3)}
NORMAL_WORDS = {"eps0": ((0, 1), (0, 2)), "eps1": ((0, 1), (0, 2)), "eps2": ((1, 0), (1, 1))}
T_ALPHAS = 1024
VALUE_UNITS = 16                # g_image: 16 * 2^-24 * w * max(r, 2^-12)
DIR_UNITS = 8                   # rays_d: 8 * 2^-24 absolute
R_FLOOR = 2.0 ** -12


def alphas():
    """alphas[t] = 1 - (t + 1) / 1024: w = 1 - alphas[t] = (t + 1) / 1024 is
    exact in f32, and a wrong t is a gross mismatch."""
    return (1.0 - (np.arange(T_ALPHAS, dtype=F64) + 1.0) / T_ALPHAS).astype(F32)


def _halves(v):
    v = int(v)
    assert 0 <= v < 2 ** 64
    return v & _MASK, (v >> 32) & _MASK


def ray_words(seed, step, n, stream):
    """Philox words [n, 4] (uint64 holding 32-bit words) of rays 0..n-1."""
    s_lo, s_hi = _halves(seed)
    t_lo, t_hi = _halves(step)
    ctr = np.empty((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = t_lo, t_hi, stream
    key = np.broadcast_to(np.array([s_lo, s_hi], np.uint64), (n, 2))
    return philox4x32_10(ctr, key)


def t_draw(seed, steps, min_step, max_step):
    """t of each step in `steps` (Python ints < 2^64): min_step + x % span with
    x the first word of counter (0xFFFFFFFF, step_lo, step_hi, 2).  The modulo
    bias towards small t is part of the draw."""
    steps = [int(s) for s in np.atleast_1d(np.asarray(steps, dtype=object))]
    s_lo, s_hi = _halves(seed)
    ctr = np.array([[0xFFFFFFFF, *_halves(s), 2] for s in steps], np.uint64)
    key = np.broadcast_to(np.array([s_lo, s_hi], np.uint64), (len(steps), 2))
    x = philox4x32_10(ctr, key)[:, 0]
    span = np.uint64(max_step - min_step + 1)
    return (np.uint64(min_step) + x % span).astype(np.int64)


def find_step(seed, min_step, max_step, want_t, start=0, limit=1 << 16):
    """The first step >= start whose t is want_t."""
    for base in range(start, start + limit, 4096):
        t = t_draw(seed, list(range(base, base + 4096)), min_step, max_step)
        hit = np.flatnonzero(t == want_t)
        if hit.size:
            return base + int(hit[0])
    raise AssertionError(f"no step in [{start}, {start + limit}) draws t = {want_t}")


def _unit(v):
    """(v >> 8) * 2^-24: exact in f32 and f64."""
    return (v >> np.uint64(8)).astype(F64) * U24


def _normal2(a, b, T):
    """Box-Muller pair of the words (a, b) at dtype T: (radius, z0, z1)."""
    arg = (((a >> np.uint64(8)) + np.uint64(1)).astype(T) * T(U24)).astype(T)
    r = np.sqrt(T(-2) * np.log(arg)).astype(T)
    two_pi = TWO_PI_F32 if T is F32 else F64(2 * np.pi)
    ang = (two_pi * ((b >> np.uint64(8)).astype(T) * T(U24))).astype(T)
    return r, (r * np.cos(ang)).astype(T), (r * np.sin(ang)).astype(T)


def draws(seed, step, n, perturb, min_step, max_step, dtype=F64):
    """Every drawn output of one launch over n rays at `dtype`:
    noise [n] f32, bg [n, 3] f32 (exact in every precision), eps [3, n] and the
    Box-Muller radius of each eps [3, n], t, w and g_image [3, n]."""
    T = dtype
    r = (ray_words(seed, step, n, 0), ray_words(seed, step, n, 1))
    word = lambda sw: r[sw[0]][:, sw[1]]  # noqa: E731
    uni = {k: _unit(word(sw)) for k, sw in UNIFORM_WORDS.items()}
    noise = (uni["noise"] if perturb else np.zeros(n)).astype(F32)
    bg = np.stack([uni["bg0"], uni["bg1"], uni["bg2"]], -1).astype(F32)
    ra, z0, _ = _normal2(*map(word, NORMAL_WORDS["eps0"]), T)
    _, _, z1 = _normal2(*map(word, NORMAL_WORDS["eps1"]), T)
    rb, z2, _ = _normal2(*map(word, NORMAL_WORDS["eps2"]), T)
    t = int(t_draw(seed, [step], min_step, max_step)[0])
    w = T(1) - T(alphas()[t])
    eps = np.stack([z0, z1, z2]).astype(T)
    return {"noise": noise, "bg": bg, "eps": eps, "radius": np.stack([ra, ra, rb]).astype(T),
            "t": t, "w": float(w), "g_image": (w * eps).astype(T)}


def g_image_bound(d64):
    """16 * 2^-24 * w * max(r, 2^-12) per element, from the float64 draws: the
    angle's absolute error is at most |2pi_f32 - 2pi| + ulp(6.28) / 2 = 11
    units of 2^-24 (times r in the value), and logf, sincosf, the two products
    and 1 - alphas[t] add about one ulp each, 5 in all."""
    return VALUE_UNITS * U24 * d64["w"] * np.maximum(d64["radius"], R_FLOOR)


# ---------------------------------------------------------------- camera

def pixel_rays64(pose, fx, fy, cx, cy, H, W):
    """cam::pixel_ray at float64 from the f32 pose and intrinsics:
    (rays_o [N, 3], rays_d [N, 3])."""
    pose = np.asarray(pose, F32).astype(F64).reshape(3, 4)
    fx, fy, cx, cy = (float(F32(v)) for v in (fx, fy, cx, cy))
    n = np.arange(H * W)
    h, w = n // max(W, 1), n % max(W, 1)
    x, y = (w + 0.5 - cx) / fx, (h + 0.5 - cy) / fy
    v = np.stack([x, y, np.ones_like(x)], -1) / np.sqrt(np.maximum(x * x + y * y + 1.0, 1e-20))[:, None]
    return np.broadcast_to(pose[:, 3], (H * W, 3)).copy(), v @ pose[:, :3].T


def _fma32(a, b, c):
    """fmaf on f32 arrays: the product is exact in f64; the sum's rounding to
    53 bits before the one to 24 can move a tie, which the tests' half-bound
    absorbs."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def pixel_rays32(pose, fx, fy, cx, cy, H, W):
    """The kernel's own f32 operations in its order: a multiply by the f32
    reciprocal of the focal length, (x*x + y*y) + 1, the two nested fmas."""
    pose = np.asarray(pose, F32).reshape(3, 4)
    fx, fy, cx, cy = (F32(v) for v in (fx, fy, cx, cy))
    n = np.arange(H * W)
    h, w = (n // max(W, 1)).astype(F32), (n % max(W, 1)).astype(F32)
    x = ((w + F32(0.5)) - cx) * (F32(1) / fx)
    y = ((h + F32(0.5)) - cy) * (F32(1) / fy)
    s = (x * x + y * y) + F32(1)
    inv = np.sqrt(np.maximum(s, F32(1e-20)))
    d0, d1, d2 = x / inv, y / inv, F32(1) / inv
    d = np.stack([_fma32(d2, np.full_like(d2, pose[k, 2]),
                         _fma32(d1, np.full_like(d1, pose[k, 1]), d0 * pose[k, 0]))
                  for k in range(3)], -1)
    return np.broadcast_to(pose[:, 3], (H * W, 3)).astype(F32), d.astype(F32)


# ---------------------------------------------------------------- the cases

SHAPES = [(1, 1), (1, 255), (16, 16), (257, 1), (33, 17), (17, 33), (48, 48), (64, 64)]
FOVS = (20.0, 55.0, 120.0)
BOX1 = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
BOX03 = (-0.3, -0.3, -0.3, 0.3, 0.3, 0.3)
SEEDS = (0, 11, 2 ** 32 + 5, 2 ** 64 - 1, 0xDEADBEEF12345678, 3)
STEPS = (0, 1234, 2 ** 32, 2 ** 64 - 1, 2 ** 40 + 17, 7)
SPANS = ((500, 500), (20, 21), (20, 999))   # min_step == max_step, a span of 2, a span of 980


class Case:
    def __init__(self, name, H, W, pose, focal, box=BOX1, min_near=0.2, seed=0, step=0,
                 span=SPANS[2], named=(), cx=None, cy=None, fy_scale=1.0):
        self.name, self.H, self.W, self.N = name, H, W, H * W
        self.pose = np.ascontiguousarray(pose, F32).reshape(3, 4)
        self.fx, self.fy = float(F32(focal)), float(F32(focal * fy_scale))
        self.cx = float(F32(W / 2 if cx is None else cx))
        self.cy = float(F32(H / 2 if cy is None else cy))
        self.aabb = np.array(box, F32)
        self.min_near = float(F32(min_near))
        self.seed, self.step = int(seed), int(step)
        self.min_step, self.max_step = span
        self.named = tuple(named)   # what the case is named for: miss, zero, nan, inverted

    def intr(self):
        return self.fx, self.fy, self.cx, self.cy

    def __repr__(self):
        return self.name


def _focal(H, fov):
    return H / (2 * np.tan(np.deg2rad(fov) / 2))


def _look_at_origin(rng, radius):
    """A camera at `radius` looking roughly at the origin, as a 3x4 pose."""
    c = rng.standard_normal(3)
    c *= radius / np.linalg.norm(c)
    fwd = -c / np.linalg.norm(c) + 0.05 * rng.standard_normal(3)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(rng.standard_normal(3), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    return np.concatenate([np.stack([right, up, fwd], 1), c[:, None]], 1)


def _identity(centre):
    return np.concatenate([np.eye(3), np.asarray(centre, F64)[:, None]], 1)


def cases():
    """The fixed cases, in a fixed order (seeded; no state is kept)."""
    rng = np.random.default_rng(20240607)
    out = []
    k = 0

    def draw_args():
        nonlocal k
        a = dict(seed=SEEDS[k % len(SEEDS)], step=STEPS[(k // 2) % len(STEPS)], span=SPANS[k % 3])
        k += 1
        return a

    # random poses: every shape at every field of view once the shapes cycle
    for i, (H, W) in enumerate(SHAPES):
        for fov in (FOVS if (H, W) in ((33, 17), (64, 64)) else (FOVS[i % 3],)):
            out.append(Case(f"random-{H}x{W}-fov{fov:g}", H, W,
                            _look_at_origin(rng, rng.uniform(1.2, 1.6)), _focal(max(H, 2), fov),
                            cx=W / 2 + rng.uniform(-0.3, 0.3), cy=H / 2 + rng.uniform(-0.3, 0.3),
                            fy_scale=1.1, **draw_args()))
    # identity rotation, odd W and H, the principal point on a pixel centre: the
    # centre row / column have a direction component of exactly 0
    for H, W in ((33, 17), (17, 33), (1, 255), (257, 1), (1, 1)):
        f = _focal(max(H, W), 55.0)
        out.append(Case(f"zero-{H}x{W}", H, W, _identity((0.25, -0.125, -1.5)), f, named=("zero",),
                        **draw_args()))
    for H, W in ((33, 17), (17, 33)):
        f = _focal(max(H, W), 55.0)
        # the centre on the face planes x = 1 and y = -1: 0 * inf in those slabs
        out.append(Case(f"face-{H}x{W}", H, W, _identity((1.0, -1.0, -1.5)), f,
                        named=("zero", "nan"), **draw_args()))
        # a centre inside the box: near = min_near
        out.append(Case(f"inside-{H}x{W}", H, W, _identity((0.1, -0.2, 0.0)), f,
                        named=("zero", "inside"), **draw_args()))
        # ... and close to the face it looks at: the exit lies before min_near
        out.append(Case(f"exit-{H}x{W}", H, W, _identity((0.0, 0.0, 0.9)), f,
                        named=("zero", "inverted"), **draw_args()))
        # a small box: the border pixels miss
        out.append(Case(f"smallbox-{H}x{W}", H, W, _identity((0.0, 0.0, -1.5)), f, box=BOX03,
                        named=("zero", "miss"), **draw_args()))
    # both ends of t for the spans of 2 and 980 (the steps found by t_draw)
    pose = _look_at_origin(rng, 1.4)
    for lo, hi in SPANS[1:]:
        for want in (lo, hi):
            seed = 11
            out.append(Case(f"t{want}-of-{lo}..{hi}", 16, 16, pose, _focal(16, 55.0), seed=seed,
                            step=find_step(seed, lo, hi, want), span=(lo, hi), named=(f"t={want}",)))
    return out


def prefix_pair():
    """The same pose, seed and step at (16, 16) and (17, 16): the draws of the
    first 256 rays must not depend on the launch shape."""
    rng = np.random.default_rng(77)
    pose = _look_at_origin(rng, 1.3)
    mk = lambda H: Case(f"prefix-{H}x16", H, 16, pose, _focal(16, 55.0), seed=2 ** 33 + 1,  # noqa: E731
                        step=2 ** 32 + 99, span=SPANS[2])
    return mk(16), mk(17)


def slab_census(rays_o, rays_d, aabb, min_near, nears, fars):
    """Counts of what a case can be named for, from f32 rays and their
    near / far: misses, exact-zero direction components, rays with a NaN slab
    bound ((b - o) * (1 / d) = 0 * inf), rays with near > far that hit, rays
    whose near is min_near."""
    o, d, b = np.asarray(rays_o, F32), np.asarray(rays_d, F32), np.asarray(aabb, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = F32(1) / d
        slabs = np.concatenate([(b[:3] - o) * rd, (b[3:] - o) * rd], -1)
    miss = (nears == F32(FLT_MAX)) & (fars == F32(FLT_MAX))
    return {"miss": int(miss.sum()), "zero": int((d == 0).sum()),
            "nan": int(np.isnan(slabs).any(-1).sum()),
            "inverted": int((~miss & (nears > fars)).sum()),
            "inside": int((~miss & (nears == F32(min_near))).sum())}


# ---------------------------------------------------------------- near_far rows

NEAR_FAR_KINDS = ("random", "axis", "face", "inside", "exit", "graze")


def near_far_rows(N, seed, degenerate=False):
    """(rays_o, rays_d, aabb, kind) as f32 arrays whose values are exact in
    f16, so that every storage type sees the same numbers.  Row j is of kind
    j % 6: random; axis-parallel (two zero components); an origin on a face
    with a zero component (0 * inf); an origin inside the box; an origin inside
    whose exit lies before min_near; a ray grazing an edge of the box.
    degenerate: the box has x0 == x1."""
    rng = np.random.default_rng([seed, N])
    h = lambda a: np.asarray(a, F32).astype(np.float16).astype(F32)  # noqa: E731
    o = h(rng.uniform(-2, 2, (N, 3)))
    d = rng.standard_normal((N, 3))
    d = h(d / np.linalg.norm(d, axis=1, keepdims=True))
    kind = np.arange(N) % len(NEAR_FAR_KINDS)
    x0 = 0.25 if degenerate else -1.0
    x1 = 0.25 if degenerate else 1.0
    for j in range(N):
        k, rep = NEAR_FAR_KINDS[kind[j]], j // len(NEAR_FAR_KINDS)
        a = rep % 3
        sgn = F32(-1 if rep & 1 else 1)
        if k == "axis":
            d[j] = 0
            d[j, a] = sgn
            if rep & 2:
                d[j, (a + 1) % 3] = -0.0    # 1 / -0 = -inf
            o[j, a] = -2 * sgn
            o[j, (a + 1) % 3], o[j, (a + 2) % 3] = h(rng.uniform(-0.9, 0.9, 2))
            if a != 0 and degenerate:
                o[j, 0] = 0.25
        elif k == "face":
            o[j, a] = (x1 if sgn > 0 else x0) if a == 0 else sgn
            d[j, a] = 0.0 if rep & 2 else -0.0
        elif k == "inside":
            o[j] = h(rng.uniform(-0.9, 0.9, 3))
            if degenerate:
                o[j, 0] = 0.25
        elif k == "exit":
            # 0.0625 before the face along a unit axis direction: far = 0.0625
            o[j], d[j] = h(rng.uniform(-0.5, 0.5, 3)), 0
            if degenerate:
                o[j, 0], d[j, 0] = 0.21875, 0.5   # crosses the plane x = 0.25 at t = 0.0625 too
                a = 1 + rep % 2
            o[j, a], d[j, a] = sgn * F32(0.9375), sgn
        elif k == "graze":
            # from (-2, 0) along (1, 1) in the (a, a + 1) plane: through the
            # edge (-1, 1), entry t == exit t
            b = (a + 1) % 3
            if degenerate:
                a, b = 1, 2
            o[j, a], o[j, b] = -2.0, 0.0
            d[j, a], d[j, b] = 0.5, 0.5
            if degenerate:
                o[j, 0], d[j, 0] = 0.0, 0.125   # in the plane x = 0.25 at that t = 2
    aabb = np.array([x0, -1, -1, x1, 1, 1], F32)
    return o, d, aabb, kind


# ---------------------------------------------------------------- sph_from_ray rows

SPH_KINDS = ("random", "pole+", "pole-", "minus_x")
SPH_RADIUS = 1.5


def sph_rows(N, seed):
    """(rays_o, rays_d, kind) f32, values exact in f16.  Origins at radius 0,
    0.5 r and 0.99 r (j % 3); directions random, towards the poles (0, +-r, 0)
    where theta = 0 / pi, or towards (-r, 0, 0) where phi = +-1."""
    rng = np.random.default_rng([seed, N, 5])
    h = lambda a: np.asarray(a, F32).astype(np.float16).astype(F32)  # noqa: E731
    u = rng.standard_normal((N, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    frac = np.array([0.0, 0.5, 0.99])[np.arange(N) % 3]
    # rounding to f16 must not push a 0.99 r origin out of the sphere
    o = h(u * (frac * SPH_RADIUS)[:, None] * (1 - 2.0 ** -9))
    kind = (np.arange(N) // 3) % len(SPH_KINDS)
    d = rng.standard_normal((N, 3))
    target = {1: (0, SPH_RADIUS, 0), 2: (0, -SPH_RADIUS, 0), 3: (-SPH_RADIUS, 0, 0)}
    for k, p in target.items():
        d[kind == k] = np.asarray(p, F64) - o[kind == k]
    d = h(d / np.linalg.norm(d, axis=1, keepdims=True))
    return o, d, kind


def sph_truth(rays_o, rays_d, radius):
    """raymarching.cu:162-198 at float64: (coords [N, 2], discriminant margin
    (B^2 - A C) / B^2 per row, inf where B = 0)."""
    o, d = np.asarray(rays_o, F64), np.asarray(rays_d, F64)
    A = (d * d).sum(-1)
    B = (o * d).sum(-1)
    C = (o * o).sum(-1) - float(F32(radius)) ** 2
    disc = B * B - A * C
    t = (-B + np.sqrt(disc)) / A
    p = o + t[:, None] * d
    theta = np.arctan2(np.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2), p[:, 1])
    phi = np.arctan2(p[:, 2], p[:, 0])
    with np.errstate(divide="ignore"):
        margin = np.where(B != 0, np.abs(disc) / (B * B), np.inf)
    return np.stack([2 * theta / np.pi - 1, phi / np.pi], -1), margin


def sph_phi_rows(kind):
    """Rows whose phi the inputs determine: not those aimed at a pole, where
    phi = atan2(z, x) of two rounding residues (x, z ~ 1e-7) is any angle at
    all, in float64 as much as in f32, and names the same point whatever it is."""
    return (np.asarray(kind) != 1) & (np.asarray(kind) != 2)


def circle_distance(a, b):
    """|a - b| for coordinates in [-1, 1] whose ends +1 and -1 are one point."""
    d = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
    return np.minimum(d, 2 - d)


def sph_errors(got, want, kind):
    """Largest absolute error of theta's coordinate over all rows, and of
    phi's, as a distance on the circle, over sph_phi_rows."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    e_theta = np.abs(got[:, 0] - want[:, 0])
    rows = sph_phi_rows(kind)
    e_phi = circle_distance(got[rows, 1], want[rows, 1])
    return float(e_theta.max()), float(e_phi.max()) if rows.any() else 0.0
