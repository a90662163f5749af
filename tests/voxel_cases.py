"""Shared cases of the DVGO voxel backbone's tests (tests/test_voxel_host.py,
tests/test_gpu_voxel.py): synthetic checkpoints, the edge rows, a float64
restatement of the field and the float32 windows.  Nothing here imports the
module under test.

The restatement is written from the reference's formulas (nerf/network.py:
245-268, osr_fine.py:559-673, dvgo_fine.py:45-54, modules/utils.py:129-131,
decoders/mlps.py:59-73).  The field is piecewise: which rows are inside the
box and which cell a row is sampled in are decisions the reference takes in
float32 (`<=` on the mapped point, `floor` of the grid coordinate).
`restate32` takes them with the same float32 operations in numpy; `truth`
evaluates the branch so chosen in float64.  Values are continuous across
cells (the weights are not clamped), the normal is not: on an integer voxel
coordinate it is the one-sided derivative of the chosen cell.

Windows (`windows`): a float32 evaluation of the path differs from the truth
by at most (number of roundings) x 2^-24 x (the magnitudes they act on):

  grid coordinate g_a: the map has 14 operations; 2^-24 relative on values of
    the size of u (<= 1.4) for eleven of them and of the size of the box
    coordinate for three (`* extent`, `+ min`, `- min`), all scaled by N_a - 1:
        dg_a = 2^-24 (N_a - 1) (12 + 4 B_a),  B_a = max(|min_a|, |max_a|) / extent_a
  raw = sum_i w_i v_i: two products per weight, one per term, seven adds, the
    weights' own subtraction: 12 roundings on S = sum_i |w_i v_i|, plus the
    position term sum_a dg_a D_a with D_a the largest |v(+1) - v(0)| along
    axis a among the cell's four edges:
        w_raw = 12 2^-24 S + sum_a dg_a D_a
  sigma = 10 softplus(raw + act_shift) is 10-Lipschitz in raw; the shift's add
    is one rounding on |y|, exp / log1p / the product by 10 a few ulp of sigma:
        w_sigma = 10 (w_raw + 2^-24 |y|) + 6 2^-24 sigma
  normal_a = -F_a ds G_a, ds = 10 sigmoid(y) (|d ds / dy| <= 2.5), G_a =
    sum_i (dw_i / dg_a) v_i, F_a = (N_a - 1) 1.25 / (2 bound) (seven factors):
        w_ds = 2.5 (w_raw + 2^-24 |y|) + 6 2^-24 ds
        w_G  = 12 2^-24 sum_i |dw_i / dg_a v_i| + sum_{b != a} dg_b M_ab
        w_n  = F_a (|G_a| w_ds + ds w_G) + 10 2^-24 |normal_a|
    with M_ab the largest mixed second difference of the cell's corner values
    along axes a and b.
  albedo in float32 (the CPU stick only; `aux["w_albedo"]`): a running bound
    through the MLP.  The feature row starts with the k0 samples' window (as
    w_raw, per channel), du_a = dg_a / (N_a - 1) for u, 2^i du + 2 ulp for
    sin / cos, 4 ulp x the largest frequency for the view encoding; a Linear
    with K inputs maps an error e to e |W|^T + (K + 2) 2^-24 (|h| |W|^T + |b|);
    ReLU is 1-Lipschitz, sigmoid 1/4-Lipschitz, plus 4 ulp of the output.
"""
import numpy as np
import torch

EPS = 2.0 ** -24
WORLD_SMALL, WORLD_LARGE = (5, 7, 6), (33, 20, 27)
# a dyadic box: the faces are hit exactly where the scaled coordinate is 0 or 1
BOX_MIN, BOX_MAX = (-1.0, -0.75, -0.5), (1.0, 1.25, 0.5)
ALPHA_INIT = 1e-2
VOXEL = 1  # the integer voxel coordinate of the edge rows


def expected_keys(posbase=5, viewbase=4, depth=3):
    keys = ["density", "k0", "xyz_min", "xyz_max", "voxel_size_each", "voxel_size_ratio",
            "voxel_size", "world_size"]
    keys += ["posfreq"] if posbase else []
    keys += ["viewfreq"] if viewbase else []
    layers = ["0"] + [f"{i}.0" for i in range(2, depth)] + [str(depth)]
    return keys + [f"rgbnet.net.{l}.{n}" for l in layers for n in ("weight", "bias")]


def make_state(world=WORLD_SMALL, C=12, posbase=5, viewbase=4, width=128, depth=3, seed=0,
               density=None):
    """A fine DVGO model's state_dict with the reference's keys and shapes."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    dim0 = C + (3 + 6 * posbase if posbase else 0) + (3 + 6 * viewbase if viewbase else 0)
    lo, hi = torch.tensor(BOX_MIN), torch.tensor(BOX_MAX)
    ws = torch.tensor(world)
    sd = {"density": r(1, 1, *world) * 3 + 2 if density is None else density,
          "k0": r(1, C, *world),
          "xyz_min": lo, "xyz_max": hi,
          "voxel_size_each": (hi - lo) / (ws - 1), "voxel_size_ratio": torch.tensor(1.0),
          "voxel_size": ((hi - lo).prod() / ws.prod()).pow(1 / 3), "world_size": ws.long()}
    if posbase:
        sd["posfreq"] = torch.tensor([2.0 ** i for i in range(posbase)])
    if viewbase:
        sd["viewfreq"] = torch.tensor([2.0 ** i for i in range(viewbase)])
    dims = [dim0] + [width] * (depth - 1) + [3]
    names = ["0"] + [f"{i}.0" for i in range(2, depth)] + [str(depth)]
    for name, i, o in zip(names, dims[:-1], dims[1:]):
        sd[f"rgbnet.net.{name}.weight"] = r(o, i) * (2.0 / i) ** 0.5
        sd[f"rgbnet.net.{name}.bias"] = r(o) * 0.1
    return sd, dim0


def save_checkpoint(path, sd, hyper="dicts", alpha_init=ALPHA_INIT):
    """hyper "dicts": Lightning style with alpha_init nested in plain dicts;
    None: the bare state_dict."""
    if hyper is None:
        torch.save(sd, path)
    else:
        cfg = {"fine_model_and_render": {"alpha_init": alpha_init, "rgbnet_dim": 12},
               "data": {"name": "synthetic"}}
        torch.save({"state_dict": sd, "hyper_parameters": {"cfg": cfg, "near": 0.1}}, path)
    return str(path)


def act_shift(alpha_init=ALPHA_INIT):
    return float(np.log(1 / (1 - alpha_init) - 1))


# ---------------------------------------------------------------- float32 decisions
def restate32(x, world, bound=1.0):
    """The map in float32 numpy, operation by operation.  x [M, 3] float32 ->
    dict(p, g: [M, 3] float32 mapped point and grid coordinate (grid axes),
    inside [M] bool, cell [M, 3] int64 = floor(g))."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    lo, hi = np.array(BOX_MIN, dtype=f), np.array(BOX_MAX, dtype=f)
    ext = hi - lo
    s = ((x + f(bound)) / f(2 * bound))[:, [0, 2, 1]]
    s = (s - f(0.5)) * f(1.25) + f(0.5)
    p = s * ext + lo
    u = (p - lo) / ext
    g = ((u * f(2) - f(1)) + f(1)) / f(2) * (np.array(world, dtype=f) - f(1))
    assert p.dtype == f and g.dtype == f
    inside = ((p <= hi) & (lo <= p)).all(-1)
    return {"p": p, "g": g, "inside": inside, "cell": np.floor(g).astype(np.int64)}


def _scan(x0, want, n=4096):
    """float32 values around x0 (n ulps each way) for which want(values) holds."""
    f = np.float32
    base = np.array([x0], dtype=f).view(np.int32)[0]
    cand = (base + np.arange(-n, n + 1, dtype=np.int32)).astype(np.int32).view(f)
    cand = cand[np.isfinite(cand)]
    return np.sort(cand[want(cand)])


def _axis_coordinate(values, axis, world):
    """Rows whose grid axis `axis` is driven by `values` (the other axes sit
    at the centre) -> (p, g) of that axis."""
    x = np.zeros((len(values), 3), dtype=np.float32)
    x[:, (0, 2, 1)[axis]] = values  # grid y is world z
    r = restate32(x, world)
    return r["p"][:, axis], r["g"][:, axis]


def edge_rows(world):
    """Edge positions [E, 3] float32 with their labels: x = 0; per grid axis
    the last float32 on the max face and the first one beyond, the first on
    the min face and the last one before it; the eight box corners; integer
    voxel coordinates (or, where no float32 maps onto the integer, the first
    one above it) and the last float32 below them, where the cell changes."""
    f = np.float32
    hi, lo = np.array(BOX_MAX, dtype=f), np.array(BOX_MIN, dtype=f)
    on_max, past_max, on_min, before_min, integer, below = [], [], [], [], [], []
    for a in range(3):
        hit = _scan(0.8, lambda v: _axis_coordinate(v, a, world)[0] == hi[a])
        assert len(hit), "no float32 maps exactly onto the max face"
        on_max.append(hit[-1])
        past_max.append(np.nextafter(hit[-1], f(np.inf)))
        hit = _scan(-0.8, lambda v: _axis_coordinate(v, a, world)[0] == lo[a])
        assert len(hit), "no float32 maps exactly onto the min face"
        on_min.append(hit[0])
        before_min.append(np.nextafter(hit[0], f(-np.inf)))
        # the voxel index itself where a float32 maps onto it exactly, else the
        # first float32 whose grid coordinate lies above it; and the last below
        k = VOXEL  # away from the centre: the scan walks float32 neighbours of a non-zero x
        x0 = (k / (world[a] - 1) - 0.5) / 1.25 * 2
        at = _scan(x0, lambda v: _axis_coordinate(v, a, world)[1] >= f(k), n=256)
        under = _scan(x0, lambda v: _axis_coordinate(v, a, world)[1] < f(k), n=256)
        assert len(at) and len(under) and under[-1] < at[0]
        integer.append(at[0])
        below.append(under[-1])
    world_of = lambda grid: [grid[0], grid[2], grid[1]]  # noqa: E731  grid xyz -> world xyz
    rows, labels = [[0.0, 0.0, 0.0]], ["zero"]
    mid = [0.1, -0.2, 0.3]
    for a in range(3):
        for name, vals in (("on_max", on_max), ("past_max", past_max), ("on_min", on_min),
                           ("before_min", before_min)):
            grid = list(mid)
            grid[a] = vals[a]
            rows.append(world_of(grid))
            labels.append(f"{name}{a}")
    for c in range(8):
        grid = [(on_max if c >> a & 1 else on_min)[a] for a in range(3)]
        rows.append(world_of(grid))
        labels.append(f"corner{c}")
    rows.append(world_of(integer))
    labels.append("integer")
    for a in range(3):  # on one axis only: the voxel index, and one float32 below it
        for name, vals in (("integer", integer), ("below", below)):
            grid = list(mid)
            grid[a] = vals[a]
            rows.append(world_of(grid))
            labels.append(f"{name}{a}")
    return np.array(rows, dtype=f), labels


def positions(M, world, seed=0, edges=True):
    """The edge rows, then positions drawn in [-1, 1]^3 (about half of them
    outside the box, which covers 0.8 of the bound), cut to M rows."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.rand(M, 3, generator=g) * 2 - 1
    if edges:
        x = torch.cat([torch.from_numpy(edge_rows(world)[0]), x])[:M]
    return x.contiguous()


# ---------------------------------------------------------------- float64 truth
def _pe(x, freqs):
    emb = (x[:, :, None] * freqs).flatten(1)
    return torch.cat([x, emb.sin(), emb.cos()], -1)


def truth(sd, x, alpha_init=ALPHA_INIT, bound=1.0):
    """sigma [M], albedo [M, 3], the float64 rgbnet parameters (requiring grad,
    state_dict order) and the terms the windows need, for x [M, 3] float32
    (CPU).  Gradients: torch.autograd on the outputs; `aux["x"]` is the
    float64 leaf the normal is taken against."""
    world = tuple(sd["density"].shape[2:])
    dec = restate32(x.detach().cpu().numpy(), world, bound)
    inside = torch.from_numpy(dec["inside"])
    cell = torch.from_numpy(dec["cell"])
    x64 = x.detach().cpu().double().requires_grad_(True)
    lo, hi = sd["xyz_min"].double(), sd["xyz_max"].double()
    n1 = torch.tensor(world).double() - 1
    s = ((x64 + bound) / (2 * bound))[:, [0, 2, 1]]
    p = ((s - 0.5) * 1.25 + 0.5) * (hi - lo) + lo
    u = (p - lo) / (hi - lo)
    g = u * n1
    up = g - cell.double()  # weight of the upper corner, lower: 1 - up
    last = torch.tensor(world) - 1
    idx = [torch.minimum(cell.clamp(min=0), last), torch.minimum((cell + 1).clamp(min=0), last)]

    def corner_values(vol):  # [C, Nx, Ny, Nz] -> [2, 2, 2, M, C] (x, y, z offsets)
        return torch.stack([torch.stack([torch.stack([
            vol[:, idx[dx][:, 0], idx[dy][:, 1], idx[dz][:, 2]].T
            for dz in (0, 1)]) for dy in (0, 1)]) for dx in (0, 1)])

    def weights():
        w = [torch.stack([1 - up[:, a], up[:, a]]) for a in range(3)]  # [2, M] per axis
        return w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]  # [2, 2, 2, M]

    wgt = weights()
    vd = corner_values(sd["density"][0].double())[..., 0]  # [2, 2, 2, M]
    raw = torch.where(inside, (wgt * vd).sum((0, 1, 2)), torch.zeros_like(up[:, 0]))
    shift = act_shift(alpha_init)
    sigma = 10 * torch.nn.functional.softplus(raw + shift)

    names = [k for k in sd if k.startswith("rgbnet.")]
    ps = [sd[k].detach().double().requires_grad_(True) for k in names]
    vk = corner_values(sd["k0"][0].double())  # [2, 2, 2, M, C]
    feats = [(wgt[..., None] * vk).sum((0, 1, 2))]
    # running float32 error bound of the feature row (module docstring: albedo)
    B = torch.maximum(lo.abs(), hi.abs()) / (hi - lo)
    du = EPS * (12 + 4 * B)
    err = [12 * EPS * (wgt[..., None] * vk).abs().sum((0, 1, 2)) + sum(
        du[a] * n1[a] * (vk.select(a, 1) - vk.select(a, 0)).abs().amax((0, 1)) for a in range(3))]
    if "posfreq" in sd:
        fr = sd["posfreq"].double()
        feats.append(_pe(u, fr))
        trig = (du[:, None] * fr).flatten().expand(len(u), -1) + 2 * EPS
        err.append(torch.cat([du.expand(len(u), -1), trig, trig], -1))
    if "viewfreq" in sd:
        feats.append(_pe(torch.full_like(u, 3 ** -0.5), sd["viewfreq"].double()))
        err.append(torch.full_like(feats[-1], 4 * EPS * float(sd["viewfreq"].max())))
    h = torch.cat(feats, -1)
    e = torch.cat(err, -1).detach()
    for i in range(0, len(ps), 2):
        W, b = ps[i].detach().abs(), ps[i + 1].detach().abs()
        e = e @ W.T + (W.shape[1] + 2) * EPS * (h.detach().abs() @ W.T + b)
        h = h @ ps[i].T + ps[i + 1]
        if i < len(ps) - 2:
            h = torch.relu(h)  # 1-Lipschitz
    out = h
    w_albedo = torch.where(inside[:, None], 0.25 * e + 4 * EPS, torch.zeros_like(e))
    albedo = torch.where(inside[:, None], torch.sigmoid(out), torch.full_like(out, 0.5))
    aux = {"x": x64, "inside": inside, "wgt": wgt.detach(), "vd": vd, "up": up.detach(),
           "y": (raw + shift).detach(), "world": world, "bound": bound, "w_albedo": w_albedo}
    return sigma, albedo, ps, aux


def normal_of(sigma, aux):
    """-d sigma.sum() / d x [M, 3] float64 (not normalised)."""
    return -torch.autograd.grad(sigma.sum(), aux["x"], retain_graph=True)[0]


def unit(n):
    return n / torch.sqrt(torch.clamp((n * n).sum(-1, keepdim=True), min=1e-20))


def windows(sigma, aux):
    """(w_sigma [M], w_normal [M, 3] in world axes) per the module docstring."""
    world, bound = aux["world"], aux["bound"]
    inside, wgt, vd, up, y = aux["inside"], aux["wgt"], aux["vd"], aux["up"], aux["y"]
    lo, hi = torch.tensor(BOX_MIN).double(), torch.tensor(BOX_MAX).double()
    n1 = torch.tensor(world).double() - 1
    B = torch.maximum(lo.abs(), hi.abs()) / (hi - lo)
    dg = EPS * n1 * (12 + 4 * B)  # [3]
    S = (wgt * vd).abs().sum((0, 1, 2))
    # largest first difference along each axis, mixed second differences
    D = [(vd.select(a, 1) - vd.select(a, 0)).abs().amax((0, 1)) for a in range(3)]
    w_raw = 12 * EPS * S + sum(dg[a] * D[a] for a in range(3))
    w_raw = torch.where(inside, w_raw, torch.zeros_like(w_raw))
    sig = sigma.detach()
    w_sigma = 10 * (w_raw + EPS * y.abs()) + 6 * EPS * sig
    ds = 10 * torch.sigmoid(y)
    w_ds = 2.5 * (w_raw + EPS * y.abs()) + 6 * EPS * ds
    w1 = [torch.stack([1 - up[:, a], up[:, a]]) for a in range(3)]
    sign = torch.tensor([-1.0, 1.0]).double()[:, None]
    w_n = []
    for a in range(3):
        parts = [w1[b] if b != a else sign.expand(2, up.shape[0]) for b in range(3)]
        dw = parts[0][:, None, None] * parts[1][None, :, None] * parts[2][None, None, :]
        G = (dw * vd).sum((0, 1, 2))
        w_G = 12 * EPS * (dw * vd).abs().sum((0, 1, 2))
        for b in range(3):
            if b == a:
                continue
            first = vd.select(a, 1) - vd.select(a, 0)  # axis a removed
            bb = b if b < a else b - 1
            M_ab = (first.select(bb, 1) - first.select(bb, 0)).abs().amax(0)
            w_G = w_G + dg[b] * M_ab
        F = n1[a] * 1.25 / (2 * bound)
        n_a = F * ds * G
        w = F * (G.abs() * w_ds + ds * w_G) + 10 * EPS * n_a.abs()
        w_n.append(torch.where(inside, w, torch.zeros_like(w)))
    return w_sigma, torch.stack([w_n[0], w_n[2], w_n[1]], -1)  # grid y is world z
