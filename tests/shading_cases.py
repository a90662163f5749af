"""Synthetic inputs of the non-albedo shading kernels (csrc/shade.hip), their
float64 truth and the numpy restatement of the light draw, shared by the CPU
check of the oracle (test_shading_cases_host.py) and the GPU comparison
(test_gpu_shading_edges.py).

One case is `cap` rows of field outputs as the shading entries read them:
sigma7 [cap, 7] (column 0 the sample, columns 1..6 its stencil +x, -x, +y, -y,
+z, -z), the samples' albedo, view directions, one light, and the upstream
gradients of the backward.  The first rows are edge rows (kind j % 9 for row
j < 36, so every kind is present four times once cap >= 36, and the small
caps still see several kinds); all later rows are bulk rows.

truth() restates network_grid.py:90-144 and renderer.py:485-489 in torch
autograd on the CPU with no f16 rounding point and without oracle/field.py: at
float64 it is the truth, at float32 the reference's own f32 arithmetic.
"""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = 1e-2                      # finite_difference_normal's epsilon
EPS32 = float(F32(EPS))         # as the kernels (and torch f32 tensors) see it
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}            # unit roundoff of the element type
EXCLUDED_CAP = {"f16": 0.01, "bf16": 0.03}            # share of bulk rows with |n.l| <= 4u
COLOUR_ROUNDINGS = 8            # the colour path has fewer than 8 roundings of u / 2... u each

# edge kinds (see make()); h0 / h1 are the two sample densities of (h)
KINDS = ("a", "b", "c", "d", "e", "f", "g", "h0", "h1")
REPEATS = 4
EDGE_ROWS = len(KINDS) * REPEATS
BULK = -1


def round_elem(x, elem):
    """Round f32 values to the element type; the result is an f32 array."""
    x = np.asarray(x, F32)
    if elem == "bf16":
        from oracle import round_bf16
        return round_bf16(x).reshape(x.shape)
    return x.astype(np.float16).astype(F32)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class Case:
    pass


def make(cap, M, seed, elem="f16"):
    """Inputs for `cap` rows (all of them filled: rows at or past the live
    count must not reach any output).  `M` is the row count handed to the
    kernel as it is; `live` is what the kernel must make of it."""
    rng = np.random.default_rng([seed, cap])
    c = Case()
    c.cap, c.M, c.live, c.elem = cap, M, min(max(M, 0), cap), elem
    # ---- bulk
    s = np.exp(rng.normal(0.0, 1.5, cap))
    g = _unit(rng, cap) * (10.0 ** rng.uniform(-2, 3, cap))[:, None]
    sig7 = np.empty((cap, 7), F64)
    sig7[:, 0] = s
    for a in range(3):
        sig7[:, 1 + 2 * a] = s + EPS * g[:, a]
        sig7[:, 2 + 2 * a] = s - EPS * g[:, a]
    sig7 = sig7.astype(F32)
    dirs = _unit(rng, cap).astype(F32)
    # the light: l_x = 2 l_y exactly, so that a normal along (1, -2, 0) is
    # exactly orthogonal to it in every precision (kind f)
    ly, lz = rng.uniform(0.2, 0.4) * rng.choice([-1, 1]), rng.uniform(0.3, 0.9) * rng.choice([-1, 1])
    nrm = np.sqrt(5 * ly * ly + lz * lz)
    l1 = F32(ly / nrm)
    c.light = np.array([F32(2) * l1, l1, F32(lz / nrm)], F32)
    # ---- edge rows
    kind = np.full(cap, BULK, np.int32)
    skew = rng.uniform(-1, 1, (cap, 6))
    for j in range(min(cap, EDGE_ROWS)):
        k, rep = KINDS[j % len(KINDS)], j // len(KINDS)
        kind[j] = j % len(KINDS)
        a = rep % 3
        sj = sig7[j, 0]
        if k == "a":    # flat: |v|^2 = 0
            sig7[j, 1:] = sj
        elif k == "b":  # tiny: 0 < |v|^2 < 1e-20 (|v| = 0.5 t / eps <= 5e-11)
            sig7[j, 1:] = 0.0
            sig7[j, 1 + 2 * a] = (1e-13, -1e-13, 3e-14, 1e-12)[rep]
        elif k in ("c", "d", "e"):
            # finite, clearly different stencil values on every axis first
            sig7[j, 1:] = sj * F32(1.0 + 0.5 * skew[j])
            if k == "c":    # one value +inf
                sig7[j, 1 + (rep * 5) % 6] = np.inf
            elif k == "d":  # inf - inf on one axis
                sig7[j, 1 + 2 * a] = sig7[j, 2 + 2 * a] = np.inf
            else:           # a NaN on one axis (the + point, then the - point)
                sig7[j, 1 + 2 * a + (rep & 1)] = np.nan
        elif k == "f":  # v = (t, -2 t, 0): n . l = 0 exactly, also after rounding to f16 / bf16
            d = F32(2.0 ** -(3 + rep // 2)) * F32(-1 if rep & 1 else 1)
            sig7[j, 1:] = (1 - d, 1 + d, 1 + 2 * d, 1 - 2 * d, 1, 1)
        elif k == "g":  # n = +-e_a, the view direction has no a component: n . d = 0
            d = F32(-0.25 if rep & 1 else 0.25)
            sig7[j, 1:] = 1.0
            sig7[j, 1 + 2 * a], sig7[j, 2 + 2 * a] = 1 + d, 1 - d
            th = rng.uniform(0, 2 * np.pi)
            dirs[j] = 0.0
            dirs[j, (a + 1) % 3], dirs[j, (a + 2) % 3] = np.cos(th), np.sin(th)
        elif k == "h0":  # w = 1 - exp(-sigma) = 0
            sig7[j, 0] = 0.0
        elif k == "h1":  # w = 1
            sig7[j, 0] = 1e4
    c.kind, c.sigma7, c.dirs = kind, sig7, dirs
    c.albedo = round_elem(rng.uniform(0, 1, (cap, 3)), elem)
    c.grad_color = round_elem(1e-2 * rng.standard_normal((cap, 3)), elem)
    # (f) is about the sub-gradient at n . l = 0: an upstream that cannot cancel
    c.grad_color[kind == KINDS.index("f")] = (2.0 ** -7, 2.0 ** -8, 2.0 ** -6)
    c.grad_sigma = rng.standard_normal(cap).astype(F32)
    return c


def rows_of(case, *kinds):
    """Mask of the live rows of the given edge kinds ("bulk" for the rest)."""
    m = np.zeros(case.live, bool)
    for k in kinds:
        m |= case.kind[:case.live] == (BULK if k == "bulk" else KINDS.index(k))
    return m


def padded_rows(m):
    """The march's returned row count (raymarching.py:224-227)."""
    return m + 128 - m % 128


def truth(case, dtype, ratio, shading, lam_orient, grad_loss, grad_color=None):
    """The reference's shading of the live rows and its autograd gradients in
    torch on the CPU at `dtype`.  ratio / lam_orient are taken as the f32
    values the kernels receive.  Returns numpy arrays (float64)."""
    M = case.live
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[:M])).to(dtype)  # noqa: E731
    s7 = t(case.sigma7).requires_grad_()
    alb = t(case.albedo).requires_grad_()
    d, l = t(case.dirs), torch.from_numpy(case.light).to(dtype)
    gc = t(case.grad_color if grad_color is None else grad_color)
    ratio, lam_orient = float(F32(ratio)), float(F32(lam_orient))
    # finite_difference_normal (epsilon meets f32 tensors: its f32 value)
    raw = -torch.stack([0.5 * (s7[:, 1] - s7[:, 2]) / EPS32, 0.5 * (s7[:, 3] - s7[:, 4]) / EPS32,
                        0.5 * (s7[:, 5] - s7[:, 6]) / EPS32], -1)
    # safe_normalize, then normal[isnan] = 0
    normal = raw / torch.sqrt(torch.clamp(torch.sum(raw * raw, -1, keepdim=True), min=1e-20))
    normal[torch.isnan(normal)] = 0
    nl = (normal * l).sum(-1)  # normal @ l, written so that no product is fused into the sum
    lamb = ratio + (1 - ratio) * nl.clamp(min=0)
    color = lamb.unsqueeze(-1).repeat(1, 3) if shading == "textureless" else alb * lamb.unsqueeze(-1)
    weights = 1 - torch.exp(-s7[:, 0])
    nd = (normal * d).sum(-1)
    loss_orient = weights.detach() * nd.clamp(min=0) ** 2
    orient = loss_orient.sum() / padded_rows(M)  # the mean over the march's rows (zeros past M)
    ((color * gc).sum() + float(grad_loss) * (lam_orient * orient)).backward()
    n64 = lambda x: x.detach().double().numpy()  # noqa: E731
    return {"normal": n64(normal), "color": n64(color), "orient": float(orient.detach()), "nl": n64(nl),
            "nd": n64(nd), "grad_stencil": n64(s7.grad[:, 1:]), "grad_sample": n64(s7.grad[:, 0]),
            "grad_albedo": n64(alb.grad) if alb.grad is not None else np.zeros((M, 3))}


def oracle_pair(case, ratio, shading, lam_orient, grad_loss, grad_color=None):
    """oracle/field.py's forward dict and (stencil gradient [M, 6], albedo
    gradient [M, 3] or None) on the live rows, under the current
    of.precision()."""
    import oracle.field as of
    M = case.live
    r32 = float(F32(ratio))
    s7 = case.sigma7[:M]
    gcol = (case.grad_color if grad_color is None else grad_color)[:M]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # the edge rows
        fo = of.shade_forward(s7[:, 0], s7[:, 1:].T, case.albedo[:M], case.dirs[:M], case.light,
                              r32, shading, eps=EPS)
        gsp, ga = of.shade_backward(fo, case.albedo[:M], case.dirs[:M], gcol, grad_loss,
                                    float(F32(lam_orient)), padded_rows(M), r32, shading, eps=EPS)
    return fo, gsp.T, ga


def rel_l2(a, e):
    a, e = np.asarray(a, F64), np.asarray(e, F64)
    return float(np.linalg.norm(a - e) / max(np.linalg.norm(e), 1e-300))


def kept_rows(case, tr):
    """(kept, excluded share): bulk rows whose |n . l| exceeds 4u.  Nearer the
    clamp's kink one rounding of the product decides the branch."""
    bulk = rows_of(case, "bulk")
    near = np.abs(tr["nl"]) <= 4 * U[case.elem]
    return bulk & ~near, float((bulk & near).sum() / max(int(bulk.sum()), 1))


# ---------------------------------------------------------------- the light draw

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit
    words: counter [..., 4], key [..., 2] -> [..., 4]."""
    c = [np.asarray(counter, np.uint64)[..., i] & np.uint64(_MASK) for i in range(4)]
    k0, k1 = (np.asarray(key, np.uint64)[..., i] & np.uint64(_MASK) for i in range(2))
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)  # 32 x 32 -> 64 bits, exact
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(_W0)) & np.uint64(_MASK)
        k1 = (k1 + np.uint64(_W1)) & np.uint64(_MASK)
    return np.stack(c, -1)


def light_draw(seeds, steps, rays_o, dtype):
    """dfhip_shading_light's documented draw for (seed, step) pairs (Python
    ints < 2^64) and rays_o [n, 3], evaluated at `dtype` (float64: the
    specification; float32: the same operations as the device performs them).
    Returns (|rays_o + z| [n], light [n, 3])."""
    n = len(seeds)
    lo = lambda v: [int(x) & _MASK for x in v]  # noqa: E731
    hi = lambda v: [(int(x) >> 32) & _MASK for x in v]  # noqa: E731
    ctr = np.stack([np.full(n, 0xFFFFFFFE, np.uint64), np.array(lo(steps), np.uint64),
                    np.array(hi(steps), np.uint64), np.full(n, 3, np.uint64)], -1)
    key = np.stack([np.array(lo(seeds), np.uint64), np.array(hi(seeds), np.uint64)], -1)
    r = philox4x32_10(ctr, key)
    T = dtype
    two24 = T(2.0 ** -24)
    log_arg = lambda x: ((x >> np.uint64(8)) + np.uint64(1)).astype(T) * two24  # noqa: E731
    angle = lambda x: T(2 * np.pi) * ((x >> np.uint64(8)).astype(T) * two24)  # noqa: E731
    ra = np.sqrt(T(-2) * np.log(log_arg(r[:, 0])))
    rb = np.sqrt(T(-2) * np.log(log_arg(r[:, 2])))
    a0, a1 = angle(r[:, 1]), angle(r[:, 3])
    z = np.stack([ra * np.cos(a0), ra * np.sin(a0), rb * np.cos(a1)], -1).astype(T)
    v = (np.asarray(rays_o, T) + z).astype(T)
    ss = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(T)
    rr = np.sqrt(np.maximum(ss, T(1e-20))).astype(T)
    return np.sqrt(ss.astype(F64)), (v / rr[:, None]).astype(T)
