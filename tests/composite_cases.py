"""Shared cases of the compositing edge tests and their float64 truth.

Imports nothing of the package under test and nothing of the C oracle: the
truth below is plain numpy, written from the formulas.

Train compositing, per ray (index, offset, num) of `rays`:

    skipped if num == 0 or offset + num > M: its outputs are 0
    alpha_i = 1 - exp(-sigma_i dt_i),  T_0 = 1,  w_i = alpha_i T_i,
    T_{i+1} = T_i (1 - alpha_i);  sample i is the last one taken if
    T_{i+1} < T_thresh;  t_i = running sum of deltas[:, 1]
    ws = sum w,  depth = sum w t,  image = sum w c
    backward (the taken length is a constant):
        grad_rgb_i   = g_image w_i
        grad_sigma_i = dt_i (g_image . (T_{i+1} c_i - (image - C_i)) + g_ws (1 - ws))
    with C_i the colour sum through sample i; rows past the last taken sample
    get no gradient.

The inference step (`infer_truth`) restates k_composite_infer: per alive slot n,
index = rays_alive[n]; loop step < n_step; stop on dt == 0; otherwise
T = 1 - wsum, w = alpha T, accumulate wsum, t, depth and colour, then stop
without advancing step if T < T_thresh.  A loop that stopped early sets
rays_alive[n] = -1 and leaves rays_t; otherwise rays_t[index] = t.

Every truth call also returns the per-ray count of samples taken and the
smallest |log(T / T_thresh)| over the break decisions it took (`margin`): the
inputs are built so that it is at least log 2, so an f32 evaluation cannot
decide differently (tests/test_composite_cases_host.py asserts it).

The 70-ray case (base list; a ray's id is its position in it):

    0 .. 12   sample counts 17, 0, 1, 15, 16, 31, 32, 33, 95, 96, 97, 113, 300
    13        first sample opaque (breaks at sample 0 of 40)
    14        optical depth 1, 2, 3, 7, 11 after samples 0 .. 4 of 40: breaks
              after 4 samples at T_thresh 1e-2, after 5 at 1e-4
    15, 16    empty space, then an opaque sample 15 (a window's last) / 16 (the
              next window's first) of 40
    17, 18    the same at sample 95 of 120 and sample 100 of 130
    19        all-zero sigma           20  sigma dt = 2e4 at sample 2
    21        sigma = inf at sample 5
    28 .. 31  one wave: ray 29 holds a single NaN sigma (sample 9 of 30)
    32 .. 35  one wave, 50 samples each: opaque at sample 7 (window 0), 20
              (window 1), 40 (window 2), never
    69        the final ray (20 samples)
    others    0 .. 40 samples

Rays 4 j .. 4 j + 3 share a wave in the compositing kernels (16 rays per
workgroup) and in the fused chain (64 per workgroup).  Ray counts 1, 15, 16, 17
are prefixes of the list.  Layout "A": the final ray does not fit
(offset + num > M); "B": it ends exactly at M; "T": M = total + 5, so rows
[total, M) belong to no ray.  Order "ordered": index = n, offsets monotone;
"scattered": the rows of `rays` shuffled, index a permutation and one mid-list
ray moved past the capacity (its former rows belong to no ray).
"""
import numpy as np
import torch

F32, F64 = np.float32, np.float64
SENT = -7.0          # prefill of every output buffer
PAD = 16             # rows past M: never to be written
T_THRESH = (1e-4, 1e-2, 0.0)
RAY_COUNTS = (1, 15, 16, 17, 70)
LOG2 = float(np.log(2.0))

# per-element floors of tests/test_gpu_raymarching.py (rtol 1e-4 everywhere)
RTOL = 1e-4
ATOL = {"ws": 1e-6, "image": 1e-6, "grad_rgb": 1e-6, "depth": 1e-5, "grad_sigma": 1e-5,
        "rays_t": 0.0}
# one rounding of the stored result, doubled: (relative, absolute)
GAIN = {"f32": (0.0, 0.0), "f64": (0.0, 0.0), "f16": (2.0 ** -10, 2.0 ** -24),
        "bf16": (2.0 ** -7, 0.0)}

_SPECIAL = [17, 0, 1, 15, 16, 31, 32, 33, 95, 96, 97, 113, 300]
# ray id -> (count, opaque sample)
_OPAQUE = {13: (40, 0), 15: (40, 15), 16: (40, 16), 17: (120, 95), 18: (130, 100),
           32: (50, 7), 33: (50, 20), 34: (50, 40)}
GRADUAL, ZERO_RAY, BIG_RAY, INF_RAY, NAN_RAY, NEVER_RAY, LAST_RAY = 14, 19, 20, 21, 29, 35, 69
NAN_AT = 9
WAVE_OF_NAN = (28, 30, 31)
_VICTIM = {70: 40, 17: 5, 16: 5, 15: 5}   # scattered: the ray moved past the capacity


def round_to(x, elem):
    """x (float array) rounded to the element type, returned as float64."""
    x = np.asarray(x)
    with np.errstate(over="ignore", invalid="ignore"):
        if elem == "f16":
            return x.astype(np.float16).astype(F64)
        if elem == "bf16":
            return torch.from_numpy(x.astype(F32)).to(torch.bfloat16).double().numpy()
        if elem == "f32":
            return x.astype(F32).astype(F64)
    return x.astype(F64)


class TrainCase:
    """Inputs of one train-compositing case (float32 numpy arrays)."""

    def __init__(self, N, layout, order):
        self.N, self.layout, self.order = N, layout, order
        gen = np.random.default_rng(31)
        counts = list(_SPECIAL)
        counts += [40, 40, 40, 40, 120, 130, 24, 24, 24]            # rays 13 .. 21
        counts += [int(v) for v in gen.integers(0, 41, 6)]          # 22 .. 27
        counts += [20, 30, 33, 18, 50, 50, 50, 50]                  # 28 .. 35
        counts += [int(v) for v in gen.integers(0, 41, 33)]         # 36 .. 68
        counts.append(20)                                           # 69
        assert len(counts) == 70
        counts[40] = max(counts[40], 8)                             # the scattered victim
        num = np.asarray(counts[:N], np.int64)
        off = np.cumsum(num) - num
        total = int(num.sum())
        all_total = int(np.sum(counts))
        # samples: drawn for the whole 70-ray list, so that prefixes share them
        rows_all = all_total + 5 + PAD
        sigma = (gen.random(rows_all) * 2.0).astype(F32)
        deltas = np.stack([0.01 + 0.02 * gen.random(rows_all),
                           0.01 + 0.02 * gen.random(rows_all)], 1).astype(F32)
        rgbs = gen.random((rows_all, 3)).astype(F32)
        off_all = np.cumsum(counts) - np.asarray(counts)
        for k, c in enumerate(counts):
            o = int(off_all[k])
            if c > 96:      # optical depth about 0.02 per sample: keep T above 2e-2
                sigma[o:o + c] *= F32(96.0 / c)
        for k, (c, at) in _OPAQUE.items():
            o = int(off_all[k])
            sigma[o:o + at], sigma[o + at] = 0.0, 1e6
        o = int(off_all[GRADUAL])
        sigma[o:o + 5], deltas[o:o + 5, 0] = [50.0, 50.0, 50.0, 200.0, 200.0], 0.02
        o = int(off_all[ZERO_RAY])
        sigma[o:o + counts[ZERO_RAY]] = 0.0
        o = int(off_all[BIG_RAY])
        sigma[o + 2], deltas[o + 2, 0] = 1e6, 0.02
        sigma[int(off_all[INF_RAY]) + 5] = np.inf
        sigma[int(off_all[NAN_RAY]) + NAN_AT] = np.nan

        if layout == "A":       # the final ray does not fit
            assert num[-1] > 7 or N == 1
            M = int(off[-1]) + min(7, int(num[-1]) - 1)
        elif layout == "B":     # the final ray ends exactly at M
            M = total
        else:                   # "T": rows [total, M) belong to no ray
            M = total + 5
        self.M, self.rows, self.total = M, M + PAD, total
        self.sigma = sigma[:self.rows].copy()
        self.deltas = deltas[:self.rows].copy()
        self.rgbs = rgbs[:self.rows].copy()
        index = np.arange(N)
        self.victim = None
        if order == "scattered":
            g2 = np.random.default_rng(77)
            index = g2.permutation(N)
            if N in _VICTIM:
                self.victim = _VICTIM[N]
                off = off.copy()
                off[self.victim] = M - 3
                assert num[self.victim] > 3
            shuffle = g2.permutation(N)
        else:
            shuffle = np.arange(N)
        self.ray_id = shuffle                       # row n of rays is base ray ray_id[n]
        self.rays = np.stack([index, off, num], 1)[shuffle].astype(np.int32)
        g3 = np.random.default_rng(9)
        self.g_ws = g3.normal(size=N).astype(F32)
        self.g_image = g3.normal(size=(N, 3)).astype(F32)

    def row_of(self, ray_id):
        """Row of `rays` that holds base ray `ray_id` (None outside a prefix)."""
        hit = np.flatnonzero(self.ray_id == ray_id)
        return int(hit[0]) if hit.size else None

    def inputs(self, elem="f32", rgb_elem=None):
        """(sigma, rgbs, deltas, g_ws, g_image) rounded to the element types,
        as float64 arrays (the truth's operands)."""
        ce = elem if rgb_elem is None else rgb_elem
        return (round_to(self.sigma, elem), round_to(self.rgbs, ce), round_to(self.deltas, elem),
                round_to(self.g_ws, elem), round_to(self.g_image, elem))


_CASES = {}


def train_case(N=70, layout="A", order="ordered"):
    key = (N, layout, order)
    if key not in _CASES:
        _CASES[key] = TrainCase(N, layout, order)
    return _CASES[key]


def _log_margin(T, thresh):
    """|log(T / thresh)| of each decision; inf where it cannot flip (thresh 0,
    T 0) and for the NaN comparisons, which are false in every precision."""
    if thresh == 0.0:
        return np.full(T.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.abs(np.log(T / thresh))
    return np.where(np.isnan(m), np.inf, m)


def _ray_chain(sigma, deltas, offset, num, T_thresh):
    """One ray's taken samples: weights, T after each, t, taken count, margin."""
    s = slice(offset, offset + num)
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = 1.0 - np.exp(-(sigma[s] * deltas[s, 0]))
        T_after = np.cumprod(1.0 - alpha)
        stop = np.flatnonzero(T_after < T_thresh)
        taken = int(stop[0]) + 1 if stop.size else num
        T_before = np.concatenate([[1.0], T_after[:-1]])
        w = (alpha * T_before)[:taken]
    t = np.cumsum(deltas[s, 1])[:taken]
    margin = float(_log_margin(T_after[:taken], T_thresh).min())
    return w, T_after[:taken], t, taken, margin


def train_truth_forward(sigma, rgbs, deltas, rays, M, T_thresh):
    """float64 forward.  Returns dict ws [N], depth [N], image [N, 3] (by ray
    index), taken [N] (by row of `rays`), margin."""
    sigma, rgbs, deltas = (np.asarray(a, F64) for a in (sigma, rgbs, deltas))
    N = rays.shape[0]
    ws, depth, image = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    taken, margin = np.zeros(N, np.int64), np.inf
    for n in range(N):
        index, offset, num = (int(v) for v in rays[n])
        if num == 0 or offset + num > M:
            continue
        w, _, t, taken[n], m = _ray_chain(sigma, deltas, offset, num, T_thresh)
        margin = min(margin, m)
        with np.errstate(invalid="ignore"):
            ws[index] = w.sum()
            depth[index] = (w * t).sum()
            image[index] = (w[:, None] * rgbs[offset:offset + taken[n]]).sum(0)
    return dict(ws=ws, depth=depth, image=image, taken=taken, margin=margin)


def train_truth_backward(g_ws, g_image, sigma, rgbs, deltas, rays, M, T_thresh, ws=None,
                         image=None):
    """float64 closed-form backward.  `ws` / `image` are the forward's outputs
    as the kernel under test is given them (default: this truth's own).
    Returns dict grad_sigma [rows], grad_rgb [rows, 3] (0 where no gradient),
    owned [rows] (True on the rows of taken samples), taken, margin."""
    sigma, rgbs, deltas = (np.asarray(a, F64) for a in (sigma, rgbs, deltas))
    g_ws, g_image = np.asarray(g_ws, F64), np.asarray(g_image, F64)
    if ws is None or image is None:
        f = train_truth_forward(sigma, rgbs, deltas, rays, M, T_thresh)
        ws, image = f["ws"], f["image"]
    ws, image = np.asarray(ws, F64), np.asarray(image, F64)
    rows, N = sigma.shape[0], rays.shape[0]
    gs, gc, owned = np.zeros(rows), np.zeros((rows, 3)), np.zeros(rows, bool)
    taken, margin = np.zeros(N, np.int64), np.inf
    for n in range(N):
        index, offset, num = (int(v) for v in rays[n])
        if num == 0 or offset + num > M:
            continue
        w, T_after, _, k, m = _ray_chain(sigma, deltas, offset, num, T_thresh)
        taken[n], margin = k, min(margin, m)
        s = slice(offset, offset + k)
        c = rgbs[s]
        with np.errstate(invalid="ignore"):
            C = np.cumsum(w[:, None] * c, 0)
            gc[s] = w[:, None] * g_image[index]
            inner = (T_after[:, None] * c - (image[index] - C)) @ g_image[index]
            gs[s] = deltas[s, 0] * (inner + g_ws[index] * (1.0 - ws[index]))
        owned[s] = True
    return dict(grad_sigma=gs, grad_rgb=gc, owned=owned, taken=taken, margin=margin)


_REF = {}


def train_reference(c, T_thresh, elem="f32", rgb_elem=None):
    """Truth and f32 C oracle of one case on the inputs rounded to the element
    types (`elem`: sigma, deltas, upstream gradients, per-ray outputs and
    grad_sigma; `rgb_elem`: colours and their gradient, default `elem`),
    computed once and shared.  The backward of the truth, of the oracle and of
    the kernel under test are all given the truth's forward `ws` / `image`
    rounded to `elem` (`ws_in`, `image_in`), so the backward is compared as a
    function of its own operands.  The oracle's results are rounded to the
    type they are stored in before their error is taken."""
    import oracle
    ce = elem if rgb_elem is None else rgb_elem
    key = (c.N, c.layout, c.order, T_thresh, elem, ce)
    if key in _REF:
        return _REF[key]
    sg, cl, dl, gw, gi = c.inputs(elem, ce)
    M = c.M
    tf = train_truth_forward(sg, cl, dl, c.rays, M, T_thresh)
    ws_in, image_in = round_to(tf["ws"], elem), round_to(tf["image"], elem)
    tb = train_truth_backward(gw, gi, sg, cl, dl, c.rays, M, T_thresh, ws_in, image_in)
    f = lambda a: np.asarray(a[:M] if a.shape[0] == c.rows else a).astype(F32)  # noqa: E731
    o_ws, o_depth, o_image = oracle.composite_rays_train_forward(f(sg), f(cl), f(dl), c.rays,
                                                                 T_thresh)
    o_gs, o_gc = oracle.composite_rays_train_backward(
        gw.astype(F32), gi.astype(F32), f(sg), f(cl), f(dl), c.rays, ws_in.astype(F32),
        image_in.astype(F32), T_thresh)
    pad = lambda a: np.concatenate([a, np.zeros((c.rows - M,) + a.shape[1:], a.dtype)])  # noqa: E731
    ref = dict(truth=dict(ws=tf["ws"], depth=tf["depth"], image=tf["image"],
                          grad_sigma=tb["grad_sigma"], grad_rgb=tb["grad_rgb"]),
               oracle=dict(ws=round_to(o_ws, elem), depth=round_to(o_depth, elem),
                           image=round_to(o_image, elem), grad_sigma=round_to(pad(o_gs), elem),
                           grad_rgb=round_to(pad(o_gc), ce)),
               ws_in=ws_in, image_in=image_in, owned=tb["owned"], taken=tf["taken"],
               margin=min(tf["margin"], tb["margin"]), elem=elem, rgb_elem=ce)
    _REF[key] = ref
    return ref


# ---------------------------------------------------------------- inference

INFER_ALIVE = (1, 63, 64, 65)
INFER_STEPS = (1, 2, 8, 9)
INFER_THRESH = (1e-2, 1e-4)
ALIVE_PAD = 4          # slots past n_alive: never to be written
ALIVE_SENT = 12345
KINDS = ("plain", "ends at step 0", "ends mid-way", "T_thresh at the first step",
         "T_thresh at the last step", "opaque last step")


class InferCase:
    """One call of the inference step: n_alive slots into 2 n_alive + 3 rays,
    every per-ray buffer preset to non-zero values."""

    def __init__(self, n_alive, n_step):
        self.n_alive, self.n_step = n_alive, n_step
        g = np.random.default_rng(1000 * n_alive + n_step)
        self.n_rays = R = 2 * n_alive + 3
        alive = g.permutation(R)[:n_alive].astype(np.int32)
        self.rays_alive = np.concatenate([alive, np.full(ALIVE_PAD, ALIVE_SENT, np.int32)])
        self.rays_t = (0.2 + 1.3 * g.random(R)).astype(F32)
        self.ws = (0.05 + 0.45 * g.random(R)).astype(F32)
        self.depth = (0.1 + 0.9 * g.random(R)).astype(F32)
        self.image = (0.05 + 0.45 * g.random((R, 3))).astype(F32)
        rows = n_alive * n_step
        # alpha <= 0.05 per step: nine steps keep T = 1 - wsum above 0.3
        self.sigma = (g.random(rows) * 1.7).astype(F32)
        self.deltas = np.stack([0.01 + 0.02 * g.random(rows),
                                0.01 + 0.02 * g.random(rows)], 1).astype(F32)
        self.rgbs = g.random((rows, 3)).astype(F32)
        self.kind = (np.arange(n_alive) + n_step) % len(KINDS)
        mid, last = n_step // 2, n_step - 1
        for n in range(n_alive):
            k, o = self.kind[n], n * n_step
            if k == 1:
                self.deltas[o:o + n_step] = 0.0
            elif k == 2 and n_step >= 2:
                self.deltas[o + mid:o + n_step] = 0.0
            elif k == 3 or (k == 4 and n_step == 1):
                self.ws[alive[n]] = 0.999
            elif k == 4:    # opaque at the step before the last: T = 0 at the last
                self.sigma[o:o + last - 1], self.sigma[o + last - 1] = 0.0, 1e6
            elif k == 5:
                self.sigma[o + last] = 1e6

    def inputs(self, elem):
        """(rays_t, sigma, rgbs, deltas, ws, depth, image) rounded to the
        element type, as float64 arrays."""
        return tuple(round_to(a, elem) for a in (self.rays_t, self.sigma, self.rgbs, self.deltas,
                                                 self.ws, self.depth, self.image))


def infer_case(n_alive, n_step):
    key = ("infer", n_alive, n_step)
    if key not in _CASES:
        _CASES[key] = InferCase(n_alive, n_step)
    return _CASES[key]


def infer_truth(n_alive, n_step, T_thresh, rays_alive, rays_t, sigma, rgbs, deltas, ws, depth,
                image):
    """float64 inference step on copies.  Returns dict rays_alive, rays_t, ws,
    depth, image, taken [n_alive] (samples accumulated), margin."""
    alive = np.array(rays_alive, np.int32)
    rays_t, ws, depth, image = (np.array(a, F64) for a in (rays_t, ws, depth, image))
    sigma, rgbs, deltas = (np.asarray(a, F64) for a in (sigma, rgbs, deltas))
    taken, margin = np.zeros(n_alive, np.int64), np.inf
    for n in range(n_alive):
        index = int(alive[n])
        t, wsum, d, c = rays_t[index], ws[index], depth[index], image[index].copy()
        step = 0
        while step < n_step:
            row = n * n_step + step
            dt = deltas[row, 0]
            if dt == 0.0:
                break
            with np.errstate(over="ignore"):
                alpha = 1.0 - np.exp(-(sigma[row] * dt))
            T = 1.0 - wsum
            w = alpha * T
            wsum += w
            t += deltas[row, 1]
            d += w * t
            c += w * rgbs[row]
            taken[n] += 1
            margin = min(margin, float(_log_margin(np.asarray([T]), T_thresh)[0]))
            if T < T_thresh:
                break
            step += 1
        if step < n_step:
            alive[n] = -1
        else:
            rays_t[index] = t
        ws[index], depth[index], image[index] = wsum, d, c
    return dict(rays_alive=alive, rays_t=rays_t, ws=ws, depth=depth, image=image, taken=taken,
                margin=margin)


def infer_reference(c, T_thresh, elem="f32"):
    """Truth and f32 C oracle of one inference call on the rounded inputs,
    computed once and shared; the oracle's results rounded to `elem`."""
    import oracle
    key = ("infer", c.n_alive, c.n_step, T_thresh, elem)
    if key in _REF:
        return _REF[key]
    rt, sg, cl, dl, ws, dp, im = c.inputs(elem)
    truth = infer_truth(c.n_alive, c.n_step, T_thresh, c.rays_alive, rt, sg, cl, dl, ws, dp, im)
    o = dict(rays_alive=c.rays_alive.copy(), rays_t=rt.astype(F32), ws=ws.astype(F32),
             depth=dp.astype(F32), image=im.astype(F32))
    oracle.composite_rays(c.n_alive, c.n_step, T_thresh, o["rays_alive"], o["rays_t"],
                          sg.astype(F32), cl.astype(F32), dl.astype(F32), o["ws"], o["depth"],
                          o["image"])
    for k in ("rays_t", "ws", "depth", "image"):
        o[k] = round_to(o[k], elem)
    ref = dict(truth=truth, oracle=o, margin=truth["margin"], elem=elem)
    _REF[key] = ref
    return ref


# ---------------------------------------------------------------- bounds

def rel_l2(y, r):
    """|y - r|_2 / |r|_2 over the finite entries of r (0 / 0 = 0)."""
    y, r = np.asarray(y, F64).ravel(), np.asarray(r, F64).ravel()
    ok = np.isfinite(r)
    num, den = np.linalg.norm(y[ok] - r[ok]), np.linalg.norm(r[ok])
    return float(num / den) if den > 0 else float(num)


def check_bounds(name, y, r, t, elem="f32", share=1.0, tag="", log=None):
    """The two bounds of one tensor: y the kernel's (or, with share = 1/3 and
    y = t, the oracle's own) result, r the truth, t the oracle.

        per tensor   |y - r|_2 <= share (3 |t - r|_2 + 1e-6 |r|_2) + gs |gain|_2
        per element  |y - r| <= share (1e-4 |r| + ATOL[name]) + gs gain

    gain = GAIN[elem] (relative, absolute) of the element type the result is
    stored in: one rounding of the result, doubled.  gs = 1 for the kernels.
    For the oracle's own check (share = 1/3) gs = 1/2: its result is rounded
    to that type once, an error of up to gain / 2 that no share of the
    arithmetic's allowance can absorb (2^-11 > 2^-10 / 3).  Non-finite entries
    of the truth must be matched exactly (NaN by NaN); they are left out of
    the norms."""
    y, r, t = (np.asarray(a, F64).reshape(-1) for a in (y, r, t))
    fin = np.isfinite(r)
    assert np.array_equal(y[~fin], r[~fin], equal_nan=True), \
        f"{tag} {name}: non-finite pattern differs from the truth's"
    assert np.isfinite(y[fin]).all(), f"{tag} {name}: non-finite where the truth is finite"
    y, r, t = y[fin], r[fin], t[fin]
    grel, gabs = GAIN[elem]
    gain = (1.0 if share == 1.0 else 0.5) * (grel * np.abs(r) + gabs)
    en, et, nr = np.linalg.norm(y - r), np.linalg.norm(t - r), np.linalg.norm(r)
    den = nr if nr > 0 else 1.0
    worst = float(np.abs(y - r).max()) if y.size else 0.0
    line = (f"edges: {tag} {name}: native {en / den:.3e} oracle {et / den:.3e} "
            f"max abs {worst:.3e}")
    if log is not None:
        log(line)
    assert en <= share * (3.0 * et + 1e-6 * nr) + np.linalg.norm(gain), line
    allowed = share * (RTOL * np.abs(r) + ATOL[name]) + gain
    bad = np.flatnonzero(np.abs(y - r) > allowed)
    assert bad.size == 0, (f"{line}; element {bad[0]}: got {y[bad[0]]!r} want {r[bad[0]]!r} "
                           f"allowed {allowed[bad[0]]:.3e}")
    return en / den, et / den
