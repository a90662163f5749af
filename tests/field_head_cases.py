"""Trained-like heads of the two MLP fields and their upstream gradients
(imported by tests/test_field_head_cases_host.py, test_oracle_field.py,
test_gpu_field_heads.py, test_gpu_vanilla_heads.py and
test_gpu_vanilla_render.py; not collected itself).

Every field kernel of the train step ends in the same two heads:
sigma = trunc_exp(h0 + gaussian(x)), whose backward is g * exp(clamp(y, -15,
15)) rounded to the autocast type, and albedo = sigmoid(h[1:4]), whose backward
g (1 - a) a is taken on the rounded albedo.  A freshly initialised network
keeps |y| small and no albedo at 0 or 1, so neither the clamp nor the saturated
colour head is ever evaluated.  The cases here scale and centre the last
Linear layer of a seeded network so that y spans about [-60, 60] (empty
space below -16, the inside of an object above 16, the rest in between) and a
good share of the albedo entries round to exactly 0 or 1.  Everything is
seeded and built on the CPU; tests/test_field_head_cases_host.py checks, from
the restatements alone, that the cases hold what they are named for.

Upstream gradients: gs_i = 1e-2 n_i exp(-clip(y_i, -15, 15)), so every row
contributes alike to the parameter gradients (as under a GradScaler) and no
f16 gradient overflows; ga ~ 1e-2 N(0, 1) (grid) or N(0, 1) (vanilla, as
tests/test_gpu_vanilla.py::test_backward has it).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle.field as of

LOW, HIGH, MID = -16.0, 16.0, 14.0  # the classes: y < LOW, y > HIGH, |y| < MID
Y_MAX = 80.0  # every |y| stays below: sigma finite and positive in f32


def class_shares(y):
    y = np.asarray(y, np.float64)
    return {"low": float((y < LOW).mean()), "high": float((y > HIGH).mean()),
            "mid": float((np.abs(y) < MID).mean()), "max_abs": float(np.abs(y).max())}


def class_scaled_gs(y, seed):
    """gs_i = 1e-2 n_i exp(-clip(y_i, -15, 15)) as f32 (numpy)."""
    n = np.random.default_rng(seed).normal(size=np.shape(y))
    return (1e-2 * n * np.exp(-np.clip(np.asarray(y, np.float64), -15, 15))).astype(np.float32)


def only(gs, y, side):
    """gs zeroed outside one class ("low": y < -16, "high": y > 16)."""
    y = np.asarray(y, np.float64)
    keep = (y < LOW) if side == "low" else (y > HIGH)
    if isinstance(gs, torch.Tensor):
        return gs * torch.from_numpy(keep).to(gs)
    return np.where(keep, gs, 0).astype(np.float32)


# ---------------------------------------------------------------- f64 trunc_exp
class _TruncExp64(torch.autograd.Function):
    """activation.trunc_exp written out for float64: forward exp, backward
    g * exp(clamp(y, -15, 15))."""

    @staticmethod
    def forward(ctx, y):
        ctx.save_for_backward(y)
        return torch.exp(y)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(y, -15.0, 15.0))


trunc_exp64 = _TruncExp64.apply


# ---------------------------------------------------------------- grid field
GRID_A, GRID_K = 1300.0, 800.0  # scales of the density row and the colour rows (grid_case)
ORACLE_A, ORACLE_K = 400.0, 300.0  # the same for oracle_case, whose features span [-1, 1]
GRID_CENTRE = -3.0  # mean of y after the edit
GRID_SIZES = {4099: 11, 31: 5}  # M of the GPU tests -> seed of the positions


def train_head(w3, b3, z, a, k, centre, blob_mean=0.0):
    """The edit of a last Linear layer (w3 [4, K], b3 [4]) given its
    bias-free outputs z [M, 4] on the case's rows: row 0 and its bias scaled by
    a and the bias shifted so that the mean of y becomes `centre`; rows 1..3
    and their biases scaled by k and centred on 0."""
    w3, b3, z = (np.asarray(v, np.float64) for v in (w3, b3, z))
    w = np.concatenate([a * w3[:1], k * w3[1:]], 0)
    b = np.empty(4)
    b[0] = a * b3[0] - (a * (z[:, 0].mean() + b3[0]) + blob_mean - centre)
    b[1:] = k * b3[1:] - k * (z[:, 1:].mean(0) + b3[1:])
    assert np.abs(w).max() < 60000 and np.abs(b).max() < 60000  # inside f16 range
    return w.astype(np.float32), b.astype(np.float32)


def grid_positions(M):
    g = torch.Generator().manual_seed(GRID_SIZES[M])
    return (torch.rand(M, 3, generator=g) * 2 - 1).mul_(0.9)


_GRID = {}


def grid_case():
    """The grid field with the trained head, on the CPU: a dict with `enc`
    (GridEncoder, embeddings uniform in [-0.5, 0.5]), `layers` (32 -> 64 -> 64
    -> 4 nn.Linear stack, the last one edited), the numpy views `emb`,
    `offsets`, `S`, `H`, `ws` (the six f32 MLP tensors) and per M the
    positions.  Built once per process; callers copy what they move or change."""
    if _GRID:
        return _GRID
    import torch.nn as nn
    from gridencoder import GridEncoder
    torch.manual_seed(21)
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16,
                      log2_hashmap_size=16, desired_resolution=2048, gridtype="tiled")
    with torch.no_grad():
        enc.embeddings.uniform_(-0.5, 0.5)
    layers = nn.ModuleList([nn.Linear(32, 64), nn.Linear(64, 64), nn.Linear(64, 4)])
    emb = enc.embeddings.detach().numpy()
    offsets = enc.offsets.numpy()
    S, H = float(np.log2(enc.per_level_scale)), 16
    ws = [p.detach().numpy().copy() for p in layers.parameters()]
    xs = {M: grid_positions(M) for M in GRID_SIZES}
    # centre on the f16 restatement of the larger case
    x = xs[4099].numpy()
    fo = of.field_forward(x, ws, of.encode(x, 1.0, emb, offsets, S, H))
    z = fo["a2"].astype(np.float64) @ of.r16(ws[4]).astype(np.float64).T
    w3, b3 = train_head(ws[4], ws[5], z, GRID_A, GRID_K, GRID_CENTRE,
                        float(of.gaussian(x).mean()))
    with torch.no_grad():
        layers[2].weight.copy_(torch.from_numpy(w3))
        layers[2].bias.copy_(torch.from_numpy(b3))
    ws[4], ws[5] = w3, b3
    _GRID.update(enc=enc, layers=layers, emb=emb, offsets=offsets, S=S, H=H, ws=ws, xs=xs)
    return _GRID


def grid_restatement(M, bf16=False):
    """oracle.field's forward of the grid case on the M-row positions under
    f16 or bf16 autocast: the dict of field_forward (y, sigma, albedo, ...)."""
    c = grid_case()
    x = c["xs"][M].numpy()
    with of.precision("bf16" if bf16 else "f16"):
        x16 = (of.encode_bf16 if bf16 else of.encode)(x, 1.0, c["emb"], c["offsets"], c["S"],
                                                      c["H"])
        return of.field_forward(x, c["ws"], x16)


def grid_upstream(M, bf16=False):
    """(gs [M] f32, ga [M, 3] f32) of the grid case (numpy)."""
    fo = grid_restatement(M, bf16)
    gs = class_scaled_gs(fo["y"], 100 + M)
    ga = (np.random.default_rng(200 + M).normal(size=(M, 3)) * 1e-2).astype(np.float32)
    return gs, ga


def oracle_case(seed=3, M=4099):
    """tests/test_oracle_field.py::_case(seed, M) with the trained head: random
    f16 features, positions and nn.Linear-range weights, the last layer edited
    as above (400 / 300, centred).  Returns x16, xyz, ws."""
    r = np.random.default_rng(seed)
    x16 = (r.uniform(-1, 1, (M, 32))).astype(np.float16)
    xyz = r.uniform(-1, 1, (M, 3)).astype(np.float32)
    lim = lambda k: 1 / np.sqrt(k)  # noqa: E731
    ws = [r.uniform(-lim(32), lim(32), (64, 32)), r.uniform(-lim(32), lim(32), 64),
          r.uniform(-lim(64), lim(64), (64, 64)), r.uniform(-lim(64), lim(64), 64),
          r.uniform(-lim(64), lim(64), (4, 64)), r.uniform(-lim(64), lim(64), 4)]
    ws = [w.astype(np.float32) for w in ws]
    fo = of.field_forward(xyz, ws, x16)
    z = fo["a2"].astype(np.float64) @ of.r16(ws[4]).astype(np.float64).T
    ws[4], ws[5] = train_head(ws[4], ws[5], z, ORACLE_A, ORACLE_K, GRID_CENTRE,
                              float(of.gaussian(xyz).mean()))
    return x16, xyz, ws


# ---------------------------------------------------------------- vanilla field
IN, HIDDEN = 39, 128
# sigma_net.state_dict() order (csrc/resmlp_common.h; equal to _resmlp.SHAPES,
# which tests/test_field_head_cases_host.py asserts)
SHAPES = ([(HIDDEN, IN), (HIDDEN,), (HIDDEN,), (HIDDEN,), (HIDDEN, IN)]
          + [(HIDDEN, HIDDEN), (HIDDEN,), (HIDDEN,), (HIDDEN,)] * 3
          + [(4, HIDDEN), (4,)])
VAN_A, VAN_K = 42.0, 24.0
VAN_CENTRE = -3.0
VAN_SIZES = {257: 31, 1000: 32, 2049: 33}  # M -> seed of the positions
VAN_BIAS_UP = 6.25  # the overflow case: net.4.bias[0] raised by this much
VAN_OVERFLOW_M = 1000
LN_F16_MAX = math.log(65520.0)  # f16(exp(y)) is inf above


def base_params(seed=0):
    """The 19 sigma_net tensors (f32, CPU) from a seed and SHAPES: Linear
    weights uniform in +-1/sqrt(fan_in) (nn.Linear's range), LayerNorm weights
    in [0.5, 1.5), every bias 0.1 N(0, 1), as tests/test_gpu_vanilla.py::
    make_net randomises them."""
    g = torch.Generator().manual_seed(1000 + seed)
    ps = []
    for i, shp in enumerate(SHAPES):
        block, j = (0, i) if i < 5 else ((1 + (i - 5) // 4, (i - 5) % 4) if i < 17 else (4, i - 17))
        if len(shp) == 2:
            lim = 1 / math.sqrt(shp[1])
            ps.append((torch.rand(shp, generator=g) * 2 - 1) * lim)
        elif block < 4 and j == 2:  # norm.weight
            ps.append(torch.rand(shp, generator=g) + 0.5)
        else:
            ps.append(torch.randn(shp, generator=g) * 0.1)
    return ps


def positions(M, seed):
    """Positions in [-1, 1]^3 with the centre and two corners among them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, 3, generator=g) * 2 - 1
    x[0] = 0.0
    if M > 2:
        x[1] = 1.0
        x[2] = -1.0
    return x


def blob_positions(M, seed):
    """Positions of the overflow case: 30 % within 0.03 N(0, 1) of the centre
    (the Gaussian blob adds about 5 to y), 20 % within 0.15 N(0, 1) (it adds
    0..5), the rest uniform in the box (it adds about nothing)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(M, 3, generator=g) * 2 - 1
    a, b = (3 * M) // 10, M // 2
    x[:a] = torch.randn(a, 3, generator=g) * 0.03
    x[a:b] = (torch.randn(b - a, 3, generator=g) * 0.15).clamp_(-1, 1)
    x[0] = 0.0
    return x


def truth_outputs(ps, x):
    """The vanilla MLP in the dtype of ps (float64 for the truth): the four
    outputs o [M, 4] and y = o0 + gaussian(x)."""
    feats = [x]
    for k in range(6):
        feats += [torch.sin(2.0 ** k * x), torch.cos(2.0 ** k * x)]
    h = torch.cat(feats, -1)
    i = 0
    for l in range(4):
        w, b, gamma, beta = ps[i:i + 4]
        i += 4
        idn = h
        if l == 0:
            idn = h @ ps[i].T
            i += 1
        h = F.silu(F.layer_norm(h @ w.T + b, (HIDDEN,), gamma, beta, 1e-5) + idn)
    o = h @ ps[i].T + ps[i + 1]
    return o, o[:, 0] + 5 * torch.exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2))


def truth_field(params, x):
    """The field in float64 with the density head through trunc_exp64: sigma
    [M], albedo [M, 3] of x [M, 3] (f64, may require grad), the f64 leaf copies
    of the 19 parameters in order, and y.  For |y| < 15 identical, in value
    and gradient, to the exp form tests/test_gpu_vanilla.py::truth_field has."""
    ps = [p.detach().double().requires_grad_(True) for p in params]
    o, y = truth_outputs(ps, x)
    return trunc_exp64(y), torch.sigmoid(o[:, 1:]), ps, y


_VAN = {}


def vanilla_case():
    """`base`: base_params(0); `trained`: the same with net.4.weight / bias
    edited (42 / 24, centred on the 1000-row positions); `xs`: positions per
    M.  Built once per process, CPU tensors, read only."""
    if _VAN:
        return _VAN
    base = base_params(0)
    xs = {M: positions(M, s) for M, s in VAN_SIZES.items()}
    with torch.no_grad():
        ps = [p.double() for p in base]
        x = xs[1000].double()
        o, y = truth_outputs(ps, x)
        z = (o - ps[18]).numpy()
        blob = float((y - o[:, 0]).mean())
    w, b = train_head(base[17].numpy(), base[18].numpy(), z, VAN_A, VAN_K, VAN_CENTRE, blob)
    trained = [p.clone() for p in base]
    trained[17], trained[18] = torch.from_numpy(w), torch.from_numpy(b)
    over = [p.clone() for p in base]
    over[18][0] += VAN_BIAS_UP
    _VAN.update(base=base, trained=trained, overflow=over, xs=xs,
                x_overflow=blob_positions(VAN_OVERFLOW_M, 34))
    return _VAN


def vanilla_truth_y(M):
    c = vanilla_case()
    with torch.no_grad():
        return truth_outputs([p.double() for p in c["trained"]], c["xs"][M].double())


def vanilla_upstream(M):
    """(gs [M] f32, ga [M, 3] f32) CPU tensors of the vanilla case."""
    _, y = vanilla_truth_y(M)
    gs = torch.from_numpy(class_scaled_gs(y.numpy(), 300 + M))
    ga = torch.randn(M, 3, generator=torch.Generator().manual_seed(400 + M))
    return gs, ga


def load_params(net, params):
    """Copy the 19 tensors into net.sigma_net (state_dict order)."""
    own = list(net.sigma_net.parameters())
    assert [tuple(p.shape) for p in own] == SHAPES
    with torch.no_grad():
        for p, v in zip(own, params):
            p.copy_(v.to(p.device))
    return net
