"""The field backward's row-liveness mask (dfhip_grid_field_backward_check_live).

k_field_bwd (csrc/fieldmlp.hip) writes, beside its outputs, one bit per field
row for the binned embedding backward: row r is LIVE iff r < M (the device
live count) and grad_sigma[r] or one of the three grad_rgb[r] compares unequal
to zero, tested on the gradients as passed in.  -0.0 counts as zero, a NaN as
live.  Bit r & 31 of u32 word r >> 5; one u16 per 16-row tile.  The kernel
writes the tiles up to the end of the last u32 word that holds a row < M, so
the bits from M to the end of that word are zero whatever the buffer held.

Checked here, for the f16 and bf16 fields with both colour-gradient types:

* row counts M in {1, 15, 16, 17, 63, 65, P + 17} (P = 64 *
  backward_parts(cap) rows per round of a full grid, read from the library:
  the last is a ragged tile in the second round), on a mask buffer
  pre-filled with ones;
* gradient patterns per row, cycling: zero density gradient with a non-zero
  colour (one channel only, each channel in turn), the reverse, all zero,
  all -0.0, and a NaN in one component of an otherwise zero row;
* the mask bits equal the definition for rows < M and are 0 from M to the end
  of the last word; words past it keep their contents;
* d_enc, the partial rows, the six gradients and found_inf are bit-equal to
  the same call without a mask;
* a second call on the same buffers with a smaller live count.

The PERM = false instantiation (natural feature order) is reached through
dfhip_field_mlp_backward, which takes no mask and no device count; the mask
code does not depend on PERM.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

KINDS = 9  # gradient patterns (see _grads)


class Data:
    """Inputs at cap = P + 64 rows, made once and never written again."""

    def __init__(self, gpu):
        import _fieldmlp
        from gridencoder import GridEncoder
        self.gpu = gpu
        self.P = 64 * _fieldmlp.backward_parts(1 << 22)
        self.cap = cap = self.P + 64
        torch.manual_seed(4321)
        grid = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16,
                           log2_hashmap_size=16, desired_resolution=2048,
                           gridtype="tiled").to(gpu)
        with torch.no_grad():
            grid.embeddings.uniform_(-0.5, 0.5)
        layers = nn.ModuleList([nn.Linear(32, 64), nn.Linear(64, 64), nn.Linear(64, 4)])
        self.ws = [p.detach().float().contiguous().to(gpu)
                   for lin in layers for p in (lin.weight, lin.bias)]
        gen = torch.Generator(device="cpu").manual_seed(77)
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
        self.gs, self.grgb, self.live = _grads(cap, gen)
        self.gs, self.grgb = self.gs.to(gpu), self.grgb.to(gpu)
        self.offsets = torch.zeros(17, dtype=torch.int32, device=gpu)
        self.params = _fieldmlp.params_count()
        self.parts = _fieldmlp.backward_parts(cap)
        self.words = (cap + 31) // 32


def _grads(cap, gen):
    """grad_sigma [cap], grad_rgb [cap, 3] (f32; values exact in f16 and bf16,
    so a narrower colour type keeps every zero and every non-zero) and the
    rows' liveness by the definition.  Row r takes pattern r % KINDS."""
    gs = torch.zeros(cap)
    grgb = torch.zeros(cap, 3)
    val = (torch.randint(1, 64, (cap,), generator=gen).float() / 1024.0) * \
        (torch.randint(0, 2, (cap,), generator=gen).float() * 2 - 1)
    kind = torch.arange(cap) % KINDS
    for ch in range(3):                       # 0..2: colour channel ch only
        grgb[kind == ch, ch] = val[kind == ch]
    gs[kind == 3] = val[kind == 3]            # 3: density only
    gs[kind == 4] = val[kind == 4]            # 4: everything non-zero
    grgb[kind == 4] = val[kind == 4][:, None]
    # 5: all +0.0 (dead)
    gs[kind == 6] = -0.0                      # 6: all -0.0 (dead)
    grgb[kind == 6] = -0.0
    gs[kind == 7] = float("nan")              # 7: NaN density gradient (live)
    grgb[kind == 8, 1] = float("nan")         # 8: NaN in one colour channel (live)
    live = ~((kind == 5) | (kind == 6))
    assert bool(torch.signbit(gs[kind == 6]).all())
    return gs, grgb, live.numpy()


@pytest.fixture(scope="module")
def data(gpu):
    return Data(gpu)


def _run(d, elem, gdt, M, mask):
    """One backward at capacity with live count M; mask: the row_live buffer or
    None.  Returns every output."""
    import _fieldmlp
    gpu, cap = d.gpu, d.cap
    m_dev = torch.full((1,), M, dtype=torch.int32, device=gpu)
    partial = torch.full((d.parts * d.params,), 7.0, device=gpu)
    grads = [torch.full_like(w, 7.0) for w in d.ws]
    flag = torch.zeros(1, device=gpu)
    d_enc = torch.full((16, cap, 2), 7.0, dtype=elem, device=gpu)
    _fieldmlp.grid_field_backward(d.enc[elem], d.xyz, 1.0, d.ws, d.gs, d.grgb.to(gdt), d_enc,
                                  partial, grads, d.offsets, 0, 0.0, 0, 0, False, None, None, 0,
                                  m_dev, found_inf=flag, row_live=mask)
    torch.cuda.synchronize()
    return [d_enc, partial, flag, *grads]


def _bits(mask):
    """The mask buffer as one 0 / 1 byte per row."""
    words = mask.cpu().numpy().view(np.uint32)
    return np.unpackbits(words.view(np.uint8), bitorder="little")


def _check_mask(d, mask, M, before):
    got = _bits(mask)
    end = 32 * ((M + 31) // 32)  # end of the last word holding a row < M
    want = d.live[:M].astype(np.uint8)
    bad = np.flatnonzero(got[:M] != want)
    assert bad.size == 0, f"M={M}: liveness of rows {bad[:8]} (pattern {bad[:8] % KINDS}) is wrong"
    assert not got[M:end].any(), f"M={M}: bits past the live count in the last word"
    assert np.array_equal(got[end:], before[end:]), f"M={M}: words past the live count written"


ELEMS = [(torch.float16, torch.float16), (torch.float16, torch.float32),
         (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]
NAMES = ["d_enc", "partial", "found_inf", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3"]


@pytest.mark.parametrize("elem,gdt", ELEMS, ids=[f"{str(a)[6:]}-{str(b)[6:]}" for a, b in ELEMS])
@pytest.mark.parametrize("mi", range(7))
def test_mask_bits_and_unchanged_outputs(data, elem, gdt, mi):
    d = data
    M = [1, 15, 16, 17, 63, 65, d.P + 17][mi]
    mask = torch.full((d.words,), -1, dtype=torch.int32, device=d.gpu)
    before = _bits(mask)
    with_mask = _run(d, elem, gdt, M, mask)
    _check_mask(d, mask, M, before)
    plain = _run(d, elem, gdt, M, None)
    for n, a, b in zip(NAMES, with_mask, plain):
        if n == "d_enc":
            a, b = a[:, :M], b[:, :M]    # only the live rows are written
        # (NaN gradients flow into the outputs: compare the bits)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), \
            f"M={M}: {n} differs with a mask"
    if M > KINDS:
        assert (~d.live[:M]).any() and d.live[:M].any()  # the case has dead and live rows


@pytest.mark.parametrize("elem,gdt", ELEMS[::3], ids=["float16", "bfloat16-float32"])
def test_reused_buffer_smaller_count(data, elem, gdt):
    """A second call on the same mask buffer with a smaller live count: the
    bits of the new count's words are rewritten (zero from M to the end of its
    last word); the words past it still hold the previous call's bits."""
    d = data
    mask = torch.full((d.words,), -1, dtype=torch.int32, device=d.gpu)
    first = d.P + 17
    _run(d, elem, gdt, first, mask)
    _check_mask(d, mask, first, np.ones(32 * d.words, np.uint8))
    before = _bits(mask)
    for M in (65, 17):
        _run(d, elem, gdt, M, mask)
        _check_mask(d, mask, M, before)
        before = _bits(mask)
