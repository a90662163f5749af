"""dfhip_train_step_prologue_row (csrc/step.hip), the first launch of every
native train step, called directly on the cases of tests/prologue_cases.py and
compared with their numpy truth:

* bit for bit: the noise, bg_color, the counter reset, lr_dev, row_dev, rays_o,
  and nears / fars against the C oracle applied to the launch's own f32 rays
  (FLT_MAX on misses, the oracle's NaN on the 0 * inf slabs; a NaN equals a
  NaN, its sign and payload are not arithmetic);
* rays_d within 8 * 2^-24 of the float64 camera and bit-equal to dfhip_get_rays;
* g_image within 16 * 2^-24 * w * max(r, 2^-12) of the float64 Box-Muller
  values (prologue_cases.g_image_bound derives the 16;
  test_prologue_cases_host.py shows the numpy f32 restatement needs half of it);
* every optional output NULL alone, perturb = 0, H = 0, seeds and steps up to
  2^64 - 1, the launch-shape independence of the draws, the _lr and plain
  forms, and the refusals, which must not launch.

Every output is allocated 64 elements longer than its size and prefilled with a
sentinel; the padding must survive every call.  Tests print `edges:` lines with
the measured figures (kept in profiles/prologue/edges.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import prologue_cases as pc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PAT = 0x5EA7BEEF
SLACK = 64
MAX_LR = 8
CASES = pc.cases()
OUTPUTS = ("rays_o", "rays_d", "nears", "fars", "noises", "bg_color", "g_image", "counter",
           "lr_dev", "row_dev")
OPTIONAL = ("noises", "bg_color", "g_image", "counter", "row_dev")
LR = np.array([1e-3, 2.5e-4, 0.0, -1.0, 3.0e38, 1e-45, 7.0, 0.125, 99.0, 98.0], F32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


class Launch:
    """Sentinel-filled, padded outputs of one call and the call itself."""

    def __init__(self, gpu, c, n_alloc=None):
        n = c.N if n_alloc is None else n_alloc
        self.c, self.gpu = c, gpu
        self.size = {"rays_o": 3 * n, "rays_d": 3 * n, "nears": n, "fars": n, "noises": n,
                     "bg_color": 3 * n, "g_image": 3 * n, "counter": 2, "lr_dev": MAX_LR,
                     "row_dev": 1}
        self.buf = {k: torch.full((s + SLACK,), PAT, dtype=torch.int32, device=gpu)
                    for k, s in self.size.items()}
        self.alphas = torch.from_numpy(pc.alphas()).to(gpu)

    def call(self, form="row", null=(), n_lr=0, row=0, perturb=1, alphas=True, lr_host=True,
             H=None, W=None, fx=None, fy=None, span=None, pose=True, aabb=True):
        import _dfhip
        c, b = self.c, self.buf
        p = lambda k: None if k in null else b[k].data_ptr()  # noqa: E731
        lr = (ctypes.c_float * len(LR))(*LR.tolist())
        lo, hi = (c.min_step, c.max_step) if span is None else span
        args = [c.pose.ctypes.data if pose else None, c.fx if fx is None else fx,
                c.fy if fy is None else fy, c.cx, c.cy, c.H if H is None else H,
                c.W if W is None else W, c.aabb.ctypes.data if aabb else None, c.min_near,
                c.seed, c.step, perturb, self.alphas.data_ptr() if alphas else None, lo, hi,
                p("rays_o"), p("rays_d"), p("nears"), p("fars"), p("noises"), p("bg_color"),
                p("g_image"), p("counter")]
        if form in ("row", "lr"):
            args += [lr if lr_host else None, n_lr, p("lr_dev")]
        if form == "row":
            args += [row, p("row_dev")]
        name = {"row": "dfhip_train_step_prologue_row", "lr": "dfhip_train_step_prologue_lr",
                "plain": "dfhip_train_step_prologue"}[form]
        _dfhip.call(name, *args, _dfhip.stream())
        torch.cuda.synchronize()
        return self

    def raw(self):
        return {k: v.cpu().numpy() for k, v in self.buf.items()}

    def untouched(self, raw, written):
        """The padding of every buffer, and the whole of every buffer not in
        `written` (name -> element count), still hold the sentinel."""
        for k in OUTPUTS:
            n = written.get(k, 0)
            assert (raw[k][n:] == PAT).all(), f"{k}: written past element {n}"


def _written(c, n_lr, null=()):
    w = {"rays_o": 3 * c.N, "rays_d": 3 * c.N, "nears": c.N, "fars": c.N, "noises": c.N,
         "bg_color": 3 * c.N, "g_image": 3 * c.N, "counter": 2, "lr_dev": n_lr, "row_dev": 1}
    return {k: v for k, v in w.items() if k not in null}


def _f(raw, k, n):
    return raw[k][:n].view(F32)


_RUNS = {}


def _full_run(gpu, c):
    """The _row form with every output, memoised per case: (raw outputs, n_lr, row)."""
    if c.name not in _RUNS:
        i = [x.name for x in CASES].index(c.name) if c in CASES else 0
        n_lr, row = (0, 1, 8)[i % 3], 37 + i
        raw = Launch(gpu, c).call(n_lr=n_lr, row=row).raw()
        _RUNS[c.name] = (raw, n_lr, row)
    return _RUNS[c.name]


_WORST = {"dir": 0.0, "g": 0.0}


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_prologue_matches_its_truth(gpu, c):
    raw, n_lr, row = _full_run(gpu, c)
    N = c.N
    Launch(gpu, c).untouched(raw, _written(c, n_lr))
    # ---- the scalars
    assert (raw["counter"][:2] == 0).all()
    assert np.array_equal(raw["lr_dev"][:n_lr].view(np.uint32), LR[:n_lr].view(np.uint32))
    assert int(raw["row_dev"][0]) == row
    # ---- rays
    o, d = _f(raw, "rays_o", 3 * N).reshape(N, 3), _f(raw, "rays_d", 3 * N).reshape(N, 3)
    o64, d64 = pc.pixel_rays64(c.pose, *c.intr(), c.H, c.W)
    assert np.array_equal(o.astype(F64), o64), "rays_o is not the pose's centre"
    err = float(np.abs(d.astype(F64) - d64).max()) / pc.U24
    _WORST["dir"] = max(_WORST["dir"], err)
    assert err <= pc.DIR_UNITS, f"rays_d {err:.2f} units of 2^-24 from the f64 camera"
    # dfhip_get_rays: the same device function
    import _dfhip
    go = torch.full((3 * N + SLACK,), PAT, dtype=torch.int32, device=gpu)
    gd = go.clone()
    _dfhip.call("dfhip_get_rays", c.pose.ctypes.data, *c.intr(), c.H, c.W, go.data_ptr(),
                gd.data_ptr(), _dfhip.stream())
    torch.cuda.synchronize()
    assert np.array_equal(go.cpu().numpy(), raw["rays_o"]), "rays_o differs from dfhip_get_rays"
    assert np.array_equal(gd.cpu().numpy(), raw["rays_d"]), "rays_d differs from dfhip_get_rays"
    # ---- near / far: the C oracle on the launch's own rays
    with np.errstate(divide="ignore", invalid="ignore"):
        ne, fa = oracle.near_far_from_aabb(o, d, c.aabb, c.min_near)
    got_ne, got_fa = _f(raw, "nears", N), _f(raw, "fars", N)
    bad = np.flatnonzero(~(_same_bits(got_ne, ne) & _same_bits(got_fa, fa)))
    assert bad.size == 0, (f"near / far of rays {bad[:5]}: got {got_ne[bad[:5]]} / "
                           f"{got_fa[bad[:5]]}, oracle {ne[bad[:5]]} / {fa[bad[:5]]}")
    census = pc.slab_census(o, d, c.aabb, c.min_near, got_ne, got_fa)
    for what in c.named:
        if not what.startswith("t="):
            assert census[what] >= 1, (what, census)
    if "nan" in c.named:
        assert np.isnan(got_ne).any() or np.isnan(got_fa).any()
    if "miss" in c.named:
        miss = got_ne == F32(pc.FLT_MAX)
        assert miss.any() and (got_fa[miss] == F32(pc.FLT_MAX)).all()
    # ---- draws
    t64 = pc.draws(c.seed, c.step, N, 1, c.min_step, c.max_step)
    assert np.array_equal(_f(raw, "noises", N).view(np.uint32), t64["noise"].view(np.uint32))
    assert np.array_equal(_f(raw, "bg_color", 3 * N).view(np.uint32),
                          t64["bg"].reshape(-1).view(np.uint32))
    g = _f(raw, "g_image", 3 * N).reshape(3, N).astype(F64)
    ratio = np.abs(g - t64["g_image"]) / pc.g_image_bound(t64)
    worst = float(ratio.max())
    _WORST["g"] = max(_WORST["g"], worst)
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"\nedges: [{c.name} seed {c.seed:#x} step {c.step:#x} t {t64['t']}] rays_d {err:.2f} of "
          f"{pc.DIR_UNITS} units; g_image {worst * pc.VALUE_UNITS:.2f} of {pc.VALUE_UNITS} units")
    assert worst <= 1.0, (f"g_image[{k}] = {g[k]!r}, truth {t64['g_image'][k]!r} with t = "
                          f"{t64['t']}, w = {t64['w']}: {worst * pc.VALUE_UNITS:.1f} units of "
                          f"2^-24 w max(r, 2^-12), {pc.VALUE_UNITS} allowed")
    for what in c.named:
        if what.startswith("t="):
            assert t64["t"] == int(what[2:])


def test_distribution_of_all_draws_equals_the_truth(gpu):
    """Mean and variance of the noise, of bg and of g_image / w over every draw
    of the cases, against the same statistics of the float64 truth.  Not a
    statistical tolerance: with |x - x'| <= b per element, |mean - mean'| <=
    mean(b) =: B, |E x^2 - E x'^2| <= mean(b (2 |x'| + b)) and |mean^2 -
    mean'^2| <= B (2 |mean'| + B); b is 0 for the uniform outputs."""
    got = {"noise": [], "bg": [], "eps": []}
    want = {"noise": [], "bg": [], "eps": []}
    bound = []
    for c in CASES:
        raw, _, _ = _full_run(gpu, c)
        t64 = pc.draws(c.seed, c.step, c.N, 1, c.min_step, c.max_step)
        got["noise"].append(_f(raw, "noises", c.N).astype(F64))
        got["bg"].append(_f(raw, "bg_color", 3 * c.N).astype(F64))
        got["eps"].append(_f(raw, "g_image", 3 * c.N).astype(F64) / t64["w"])
        want["noise"].append(t64["noise"].astype(F64))
        want["bg"].append(t64["bg"].reshape(-1).astype(F64))
        want["eps"].append(t64["eps"].reshape(-1))
        bound.append((pc.g_image_bound(t64) / t64["w"]).reshape(-1))
    b_eps = np.concatenate(bound)
    for k in got:
        x, y = np.concatenate(got[k]), np.concatenate(want[k])
        b = b_eps if k == "eps" else np.zeros_like(y)
        B = b.mean()
        allow_mean = B + 1e-15
        allow_var = (b * (2 * np.abs(y) + b)).mean() + B * (2 * abs(y.mean()) + B) + 1e-15
        print(f"\nedges: distribution of {x.size} {k} values: mean {x.mean():.9f} (truth "
              f"{y.mean():.9f}, allowed {allow_mean:.2e}), variance {x.var():.9f} (truth "
              f"{y.var():.9f}, allowed {allow_var:.2e})")
        assert abs(x.mean() - y.mean()) <= allow_mean
        assert abs(x.var() - y.var()) <= allow_var
    n = sum(c.N for c in CASES)
    assert n > 20000
    print(f"edges: worst over the cases: rays_d {_WORST['dir']:.2f} of {pc.DIR_UNITS} units of "
          f"2^-24, g_image {_WORST['g'] * pc.VALUE_UNITS:.2f} of {pc.VALUE_UNITS} units")


# ---------------------------------------------------------------- options

def _case(name):
    return next(c for c in CASES if c.name == name)


def test_perturb_zero_gives_zero_noise(gpu):
    c = _case("random-33x17-fov55")
    full, n_lr, row = _full_run(gpu, c)
    raw = Launch(gpu, c).call(n_lr=n_lr, row=row, perturb=0).raw()
    assert (raw["noises"][:c.N] == 0).all()  # +0.0
    for k in OUTPUTS:
        if k != "noises":
            assert np.array_equal(raw[k], full[k]), k


@pytest.mark.parametrize("skip", OPTIONAL)
def test_each_optional_output_may_be_null_alone(gpu, skip):
    c = _case("random-17x33-fov120")
    full, n_lr, row = _full_run(gpu, c)
    la = Launch(gpu, c).call(null=(skip,), n_lr=n_lr, row=row)
    raw = la.raw()
    la.untouched(raw, _written(c, n_lr, null=(skip,)))
    for k in OUTPUTS:
        if k != skip:
            assert np.array_equal(raw[k], full[k]), f"{k} changed with {skip} = NULL"


def test_g_image_null_needs_no_alphas(gpu):
    c = _case("random-16x16-fov120")
    full, n_lr, row = _full_run(gpu, c)
    raw = Launch(gpu, c).call(null=("g_image",), alphas=False, n_lr=n_lr, row=row,
                              span=(5, 3)).raw()
    for k in OUTPUTS:
        if k != "g_image":
            assert np.array_equal(raw[k], full[k]), k


def test_lr_and_plain_forms_are_the_row_form_with_nulls(gpu):
    c = _case("random-48x48-fov20")
    a = Launch(gpu, c).call("row", null=("row_dev",), n_lr=1).raw()
    b = Launch(gpu, c).call("lr", n_lr=1).raw()
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    assert b["lr_dev"][:1].view(np.uint32) == LR[:1].view(np.uint32) and b["row_dev"][0] == PAT
    a = Launch(gpu, c).call("row", null=("row_dev", "lr_dev"), n_lr=0, lr_host=False).raw()
    b = Launch(gpu, c).call("plain").raw()
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    assert (b["lr_dev"] == PAT).all() and (b["counter"][:2] == 0).all()
    full, _, _ = _full_run(gpu, c)
    for k in ("rays_o", "rays_d", "nears", "fars", "noises", "bg_color", "g_image"):
        assert np.array_equal(b[k], full[k]), k


@pytest.mark.parametrize("n_lr", [0, 1, 8])
def test_no_rays_still_writes_counter_lr_and_row(gpu, n_lr):
    """H = 0: one block runs for the counter reset, the lr pack and the row;
    the ray buffers (non-null, one element) keep their sentinel."""
    c = _case("random-16x16-fov120")
    la = Launch(gpu, c, n_alloc=1).call(H=0, n_lr=n_lr, row=5)
    raw = la.raw()
    la.untouched(raw, {"counter": 2, "lr_dev": n_lr, "row_dev": 1})
    assert (raw["counter"][:2] == 0).all() and raw["row_dev"][0] == 5
    assert np.array_equal(raw["lr_dev"][:n_lr].view(np.uint32), LR[:n_lr].view(np.uint32))
    # W = 0 is the same launch
    raw = Launch(gpu, c, n_alloc=1).call(W=0, n_lr=n_lr, row=6).raw()
    la.untouched(raw, {"counter": 2, "lr_dev": n_lr, "row_dev": 1})
    assert (raw["counter"][:2] == 0).all() and raw["row_dev"][0] == 6


def test_draws_do_not_depend_on_the_launch_shape(gpu):
    a, b = pc.prefix_pair()
    ra, rb = Launch(gpu, a).call().raw(), Launch(gpu, b).call().raw()
    n = a.N
    assert np.array_equal(ra["noises"][:n], rb["noises"][:n])
    assert np.array_equal(ra["bg_color"][:3 * n], rb["bg_color"][:3 * n])
    ga = ra["g_image"][:3 * n].reshape(3, n)
    gb = rb["g_image"][:3 * b.N].reshape(3, b.N)[:, :n]
    assert np.array_equal(ga, gb)
    t64 = pc.draws(a.seed, a.step, n, 1, a.min_step, a.max_step)
    assert np.array_equal(ra["noises"][:n].view(np.uint32), t64["noise"].view(np.uint32))


def test_high_halves_of_seed_and_step_reach_the_draws(gpu):
    """Ranks are told apart by the seed alone, steps by the step alone: 2^32
    apart in either must draw other numbers."""
    import copy
    c = _case("random-16x16-fov120")
    planes = []
    for seed, step in ((c.seed, c.step), (c.seed ^ (1 << 32), c.step), (c.seed, c.step ^ (1 << 32)),
                       (c.seed ^ (1 << 63), c.step), (c.seed, c.step ^ (1 << 63))):
        v = copy.copy(c)
        v.seed, v.step = seed, step
        raw = Launch(gpu, v).call().raw()
        t64 = pc.draws(seed, step, v.N, 1, v.min_step, v.max_step)
        assert np.array_equal(raw["noises"][:v.N].view(np.uint32), t64["noise"].view(np.uint32))
        planes.append(raw["noises"][:v.N])
    for i in range(len(planes)):
        for j in range(i):
            assert (planes[i] != planes[j]).mean() > 0.95, (i, j)


# ---------------------------------------------------------------- refusals

REFUSALS = [
    ("n_lr-9", dict(n_lr=9), "at most 8 learning rates"),
    ("n_lr-1-null-lr_host", dict(n_lr=1, lr_host=False), "learning rates"),
    ("n_lr-1-null-lr_dev", dict(n_lr=1, null=("lr_dev",)), "learning rates"),
    ("g_image-without-alphas", dict(alphas=False), "needs alphas"),
    ("max_step-below-min_step", dict(span=(21, 20)), "min_step <= max_step"),
    ("fx-zero", dict(fx=0.0), "focal lengths must be non-zero"),
    ("fy-zero", dict(fy=-0.0), "focal lengths must be non-zero"),
    ("null-pose", dict(pose=False), "null pointer"),
    ("null-aabb", dict(aabb=False), "null pointer"),
    ("null-rays_o", dict(null=("rays_o",)), "null pointer"),
    ("null-rays_d", dict(null=("rays_d",)), "null pointer"),
    ("null-nears", dict(null=("nears",)), "null pointer"),
    ("null-fars", dict(null=("fars",)), "null pointer"),
]


@pytest.mark.parametrize("kw,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_return_einval_and_do_not_launch(gpu, kw, msg):
    c = _case("random-16x16-fov120")
    la = Launch(gpu, c)
    with pytest.raises(RuntimeError, match=r"dfhip_train_step_prologue_row failed \(1\): "
                                           r"train_step_prologue: .*" + msg):
        la.call(**kw)
    torch.cuda.synchronize()
    la.untouched(la.raw(), {})  # no launch: every buffer still holds the sentinel
