"""Inputs, the float32 model and the rounding-count bounds of the native
GradScaler + Adam step (csrc/optim.hip), shared by the CPU check of the bounds
(test_oracle_kat.py) and the GPU comparison (test_gpu_optim.py).  The bounds
are derived in test_gpu_optim.test_adam_step_within_rounding_bounds."""
import numpy as np

import oracle.optim as oo

F32, F64 = np.float32, np.float64
U = 2.0 ** -24        # unit roundoff of float32
TINY = 2.0 ** -149    # a rounding in the subnormal range: absolute, not relative
POWF_ULPS = 1.0       # device powf: 1 ulp (HIP math API, single precision table)
SLACK = 1.001         # the counts are first order in u; products of roundings are < 1e-5 of them

# one optimizer, two groups; sizes around kPerBlock = 2048 (none, one element,
# a scalar-path tail only, one chunk less one, exactly one, one plus a tail,
# two whole chunks, two and a tail, eight and a tail)
SIZES = [0, 1, 2047, 4096, 5000, 3, 2048, 2049, 8 * 2048 + 5]
GROUP = [0, 0, 0, 0, 0, 1, 1, 1, 1]
# (lr, betas, eps, weight_decay): A = the reference's settings, B = others
GROUPS = [dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.0),
          dict(lr=1e-3, betas=(0.8, 0.95), eps=1e-8, weight_decay=0.01)]
STEPS = 6
INIT_SCALE = 3000.0   # not a power of two: grad / scale rounds
GROWTH_INTERVAL = 3


def hyper32(gi):
    """(lr, b1, b2, eps, wd) of group gi as the C ABI receives them: float32."""
    g = GROUPS[gi]
    return tuple(float(F32(x)) for x in (g["lr"], *g["betas"], g["eps"], g["weight_decay"]))


def params(seed=0):
    """Initial parameters: even elements |p| ~ lr (the update is not hidden
    under the parameter's rounding), odd elements N(0, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for n, gi in zip(SIZES, GROUP):
        p = rng.standard_normal(n)
        p[0::2] *= GROUPS[gi]["lr"]
        out.append(p.astype(F32))
    return out


def grads(it, scale, seed=0):
    """Scaled gradients of step `it`: unscaled they are N(0, 1), except
    elements 3 mod 7 (always +-[1e-17, 1e-13], log-uniform: eps = 1e-15
    matters) and elements 0 mod 11 on odd steps (exact zeros)."""
    rng = np.random.default_rng([seed, 1000 + it])
    out = []
    for n in SIZES:
        g = rng.standard_normal(n)
        i = np.arange(n)
        small = i % 7 == 3
        g[small] = np.sign(g[small]) * 10.0 ** rng.uniform(-17, -13, int(small.sum()))
        if it % 2 == 1:
            g[i % 11 == 0] = 0.0
        out.append((g * scale).astype(F32))
    return out


def adam_f32(p, g, m, v, step, scale, lr, b1, b2, eps, wd, pow_fn=np.power):
    """The step's formula in np.float32, one rounding per operation, in the
    order of the comment at the head of csrc/optim.hip.  Independent of the
    kernel; used to check that the bounds are neither too tight nor loose."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, s = (F32(a) for a in (lr, b1, b2, eps, wd, scale))
    one, t = F32(1), F32(step + 1)
    g = g / s
    if wd != 0:
        g = g + wd * p
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    step_size = lr / (one - F32(pow_fn(b1, t)))
    bc2s = np.sqrt(one - F32(pow_fn(b2, t)))
    denom = np.sqrt(v) / bc2s + eps
    p = p - step_size * m / denom
    assert all(a.dtype == F32 for a in (p, m, v))
    return p, m, v


def pow_ulps(b, t, fn=np.power):
    """Error of fn(float32 b, float32 t) against float64 pow, in float32 ulps."""
    got, want = F64(F32(fn(F32(b), F32(t)))), F64(F32(b)) ** F64(t)
    return abs(got - want) / np.spacing(F32(want)).astype(F64)


def bounds(p, g, m, v, step, scale, lr, b1, b2, eps, wd, pow_ulps1=POWF_ULPS,
           pow_ulps2=POWF_ULPS):
    """One step from the float32 state (p, m, v): the float64 oracle's m, v and
    update d = p_new - p, with the bound of a float32 evaluation's error on
    each.  Returns {"m", "v", "d", "p": oracle values, "Em", "Ev", "Ed": bounds}."""
    p0, m0, v0 = (np.asarray(a, F64) for a in (p, m, v))
    P, M, V = oo.adam_element(p0, g, m0, v0, step, scale, lr, b1, b2, eps, wd)
    t = step + 1.0
    g0 = np.asarray(g, F64) / scale
    cg = 2.0 if wd != 0 else 1.0             # roundings on g, relative to G
    G = np.abs(g0) + np.abs(wd * p0)         # |g| when wd = 0
    tm = np.abs(b1 * m0) + (1 - b1) * G
    tv = np.abs(b2 * v0) + (1 - b2) * G * G
    c_m, c_v = 3 + cg, 4 + 2 * cg
    Em = SLACK * c_m * U * tm + 4 * TINY
    Ev = SLACK * c_v * U * tv + 6 * TINY
    k1, k2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
    c_s = 2 + 2 * k1 * pow_ulps1             # step_size
    c_bc = 1.5 + k2 * pow_ulps2              # sqrt(1 - b2^t)
    S, bc = lr / (1 - b1 ** t), np.sqrt(1 - b2 ** t)
    sv = np.sqrt(V)
    dsqrt = np.where(V > 0, Ev / np.maximum(sv + np.sqrt(np.maximum(V - Ev, 0)), 1e-300),
                     np.sqrt(Ev))
    D = sv / bc + eps
    dD = dsqrt / bc + sv / bc * U * (2 + c_bc) + U * D
    with np.errstate(divide="ignore", invalid="ignore"):
        relD = np.where(dD < D, dD / (D - dD), np.inf)
        d_abs = np.where(tm > 0, S * tm / D, 0.0)
        Ed = SLACK * d_abs * (U * (c_m + c_s + 2) + relD)
    Ed = np.where(d_abs > 0, Ed, 0.0) + U * np.abs(P) + 4 * TINY
    return {"p": P, "m": M, "v": V, "d": P - p0, "Em": Em, "Ev": Ev, "Ed": Ed,
            "c": {"m": c_m, "v": c_v, "d": c_m + c_s + 2}}


def ratios(bd, p_old, p_new, m_new, v_new):
    """Worst error / bound of m, v, the update, and ("ds") the update of the
    even elements alone, whose |p| ~ lr leaves the final subtraction's u |p|
    a small part of the bound (0 for an empty tensor)."""
    if bd["m"].size == 0:
        return {"m": 0.0, "v": 0.0, "d": 0.0, "ds": 0.0}
    d = np.asarray(p_new, F64) - np.asarray(p_old, F64)
    with np.errstate(invalid="ignore"):
        out = {"m": np.abs(np.asarray(m_new, F64) - bd["m"]) / bd["Em"],
               "v": np.abs(np.asarray(v_new, F64) - bd["v"]) / bd["Ev"],
               "d": np.abs(d - bd["d"]) / bd["Ed"]}
    out["ds"] = out["d"][0::2]
    # a nan (non-finite result on either side) must count as outside
    return {k: float(np.where(np.isnan(r), np.inf, r).max()) for k, r in out.items()}
