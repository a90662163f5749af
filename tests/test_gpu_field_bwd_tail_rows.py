"""Rows past the live count give the field backward nothing.

k_field_bwd (csrc/fieldmlp.hip) prefetches every tile's inputs without a
bounds branch: a lane whose sample lies past the live count M loads the last
live row instead (row 0 when M = 0), and the chain zeroes what such a sample
contributes (features, output gradient).  So with a device-side live count
below the capacity, whatever the rows [M, cap) of the inputs hold — here NaN
in the features, positions and upstream gradients — the feature gradient, the
per-workgroup partial rows, the six summed weight gradients and the overflow
flag must be bit for bit what they are with zeros there, and finite.

Row counts (P = 64 * backward_parts(cap) rows per round of a full grid, read
from the library): 1 and 63 (one ragged tile, three lane groups of the last
live row's tile empty), P - 1 and P + 17 (a ragged tile at the end of the
first round / in the second), 2P + 83 (a third round in which only some waves
hold a tile), 0 (no round at all: every gradient is zero).

Inputs: a seeded tiled-grid table U(-0.5, 0.5) through the fused forward,
upstream gradients N(0, 1e-2).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


class Data:
    """Inputs at cap = 3 P rows, made once and never written again."""

    def __init__(self, gpu):
        import _fieldmlp
        from gridencoder import GridEncoder
        self.gpu = gpu
        self.P = 64 * _fieldmlp.backward_parts(1 << 22)
        self.cap = cap = 3 * self.P
        torch.manual_seed(1234)
        grid = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16,
                           log2_hashmap_size=16, desired_resolution=2048,
                           gridtype="tiled").to(gpu)
        with torch.no_grad():
            grid.embeddings.uniform_(-0.5, 0.5)
        layers = nn.ModuleList([nn.Linear(32, 64), nn.Linear(64, 64), nn.Linear(64, 4)])
        self.ws = [p.detach().float().contiguous().to(gpu)
                   for lin in layers for p in (lin.weight, lin.bias)]
        gen = torch.Generator(device="cpu").manual_seed(99)
        self.xyz = (torch.rand(cap, 3, generator=gen) * 2 - 1).to(gpu)
        S = float(np.log2(grid.per_level_scale))
        self.enc = {}
        for dt in (torch.float16, torch.bfloat16):
            table = grid.embeddings.detach().to(dt).contiguous()
            enc = torch.empty(cap, 32, device=gpu, dtype=dt)
            sigma = torch.empty(cap, device=gpu)
            rgb = torch.empty(cap, 3, device=gpu, dtype=dt)
            _fieldmlp.grid_field_forward(self.xyz, 1.0, table, grid.offsets, S,
                                         int(grid.base_resolution), grid.gridtype_id, False,
                                         self.ws, enc, sigma, rgb, None)
            self.enc[dt] = enc
        assert float(self.enc[torch.float16].float().abs().max()) > 0
        self.gs = (torch.randn(cap, generator=gen) * 1e-2).to(gpu)
        self.grgb = (torch.randn(cap, 3, generator=gen) * 1e-2).to(gpu)
        self.dh = (torch.randn(cap, 4, generator=gen) * 1e-2).to(gpu)
        self.offsets = torch.zeros(17, dtype=torch.int32, device=gpu)
        self.params = _fieldmlp.params_count()
        self.parts = _fieldmlp.backward_parts(cap)


@pytest.fixture(scope="module")
def data(gpu):
    return Data(gpu)


def _tail(t, M, value):
    """A copy of t with rows [M, cap) set to `value`."""
    out = t.clone()
    out[M:] = value
    return out


def _run(d, entry, elem, gdt, M, value):
    """One backward at capacity with live count M and `value` in the dead rows;
    returns every output."""
    import _fieldmlp
    gpu, cap = d.gpu, d.cap
    m_dev = torch.full((1,), M, dtype=torch.int32, device=gpu)
    enc = _tail(d.enc[elem], M, value)
    partial = torch.full((d.parts * d.params,), 7.0, device=gpu)
    grads = [torch.full_like(w, 7.0) for w in d.ws]
    flag = torch.zeros(1, device=gpu)
    if entry == "mlp":
        d_enc = torch.full((cap, 32), 7.0, dtype=elem, device=gpu)
        _fieldmlp.mlp_backward(enc, d.ws, _tail(d.dh, M, value).to(elem), d_enc, partial, grads,
                               m_dev=m_dev)
    else:
        d_enc = torch.full((16, cap, 2), 7.0, dtype=elem, device=gpu)
        _fieldmlp.grid_field_backward(enc, _tail(d.xyz, M, value), 1.0, d.ws,
                                      _tail(d.gs, M, value), _tail(d.grgb, M, value).to(gdt),
                                      d_enc, partial, grads, d.offsets, 0, 0.0, 0, 0, False, None,
                                      None, 0, m_dev, found_inf=flag)
    torch.cuda.synchronize()
    return [d_enc, partial, flag, *grads]


ENTRIES = [
    ("fused", torch.float16, torch.float16),
    ("fused", torch.float16, torch.float32),
    ("fused", torch.bfloat16, torch.bfloat16),
    ("fused", torch.bfloat16, torch.float32),
    ("mlp", torch.float16, None),
    ("mlp", torch.bfloat16, None),
]
IDS = [f"{e}-{str(a)[6:]}-{str(b)[6:] if b else 'dh'}" for e, a, b in ENTRIES]
NAMES = ["d_enc", "partial", "found_inf", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3"]


@pytest.mark.parametrize("entry,elem,gdt", ENTRIES, ids=IDS)
@pytest.mark.parametrize("mi", range(6))
def test_dead_rows_do_not_reach_the_gradients(data, entry, elem, gdt, mi):
    P = data.P
    M = [0, 1, 63, P - 1, P + 17, 2 * P + 83][mi]
    clean = _run(data, entry, elem, gdt, M, 0.0)
    dirty = _run(data, entry, elem, gdt, M, float("nan"))
    for n, a, b in zip(NAMES, clean, dirty):
        if n == "d_enc" and entry == "fused":
            a, b = a[:, :M], b[:, :M]    # [16, cap, 2]: only the live rows are written
        assert torch.equal(a, b), f"{entry} M={M}: {n} depends on the rows past the live count"
    assert float(dirty[2]) == 0.0
    for n, g in zip(NAMES[3:], dirty[3:]):
        assert bool(torch.isfinite(g).all()), f"{entry} M={M}: {n} is not finite"
    if M == 0:
        assert all(float(g.abs().max()) == 0.0 for g in dirty[3:])
    else:
        assert float(dirty[5].abs().sum()) > 0      # the case is live
    if entry == "mlp":
        assert float(dirty[0][M:].float().abs().max() if M < data.cap else 0.0) == 0.0
