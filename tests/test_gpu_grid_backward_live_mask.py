"""The binned embedding backward drops dead rows (BinnedOpts.row_live).

A row whose liveness bit is 0 (bit r & 31 of u32 word r >> 5; the field
backward writes it for rows whose incoming gradient is exactly zero) is not
filed by the binning (csrc/gridbin.hip k_bin / k_bin_fast), so the walk never
takes it.  On the reference grid layout (16 levels x 2 channels):

* case matrix: B in {1, 1023, 1024 + 17, 3 * 1024 + 1} samples with the device
  live count equal to B and below it (B - max(1, B // 3); 0 for B = 1), f16 and
  bf16 gradients, both walk forms, overwrite and accumulate;
* masks over the rows below the live count: all live, all dead, alternating, a
  dead run across the 1,024-sample tile boundary (rows 1000..1059, which also
  crosses a 32-bit word boundary) with another across the word boundary at 32
  (rows 20..39), only the last row dead.  The bits of rows at and past the
  live count are ones: the binning must not read them as rows;
* the mask is used: the masked rows carry non-zero random gradients and the
  result must match the f64 oracle computed with those rows zeroed, at the
  tolerance of tests/test_gpu_encoders.py::test_grid_backward_walk_forms
  (rtol 1e-5, atol 1e-7 max|want|).  With accumulate the call writes
  float(base + float(sum)) per element, so its result must be bit-equal to
  base + (the overwriting call's result), which is checked against the oracle;
* null-mask equivalence: with the masked rows' gradients zeroed, the call with
  the mask and the call with row_live = NULL give bit-equal results
  (torch.equal: the bin totals that deal out the walk parts count the dead
  rows' entries as before, so every part sums the same tiles, and the f64 sums
  of the exact products do not depend on the order, as in
  test_grid_backward_kept_clean_scratch);
* all dead: the gradient is all zero (with accumulate: unchanged), the bin
  totals are zero after the call and a following kept_clean call is correct;
* the generic binning kernel (fast_bin = 0) on the same masks;
* stencil groups (group = 7) take no mask: the call is rejected.  (A group
  files a centre entry whose seven points the walk reads from the gradient
  rows whatever a mask says, and dropping single points in the binning cost
  k_bin_fast<7> more than the walk gained: DESIGN.md, round 12.)
"""
import functools

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 1023, 1024 + 17, 3 * 1024 + 1]
DTYPES = [torch.float16, torch.bfloat16]
EPS = 1e-2


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _grid():
    from gridencoder.grid import level_offsets
    pls = np.exp2(np.log2(2048 / 16) / 15)
    offs = level_offsets(16, 2, 3, 16, pls, 16, False)
    return offs, float(np.log2(pls))


def _counts(B):
    return [B, B - max(1, B // 3)]


def _row_patterns(n):
    """name -> liveness [n] of the rows below the live count."""
    idx = np.arange(n)
    run = ((idx >= 20) & (idx < 40)) | ((idx >= 1000) & (idx < 1060))
    return {"all_live": np.ones(n, bool), "all_dead": np.zeros(n, bool),
            "alternating": idx % 2 == 0, "dead_run": ~run, "last_dead": idx != n - 1}


def _pack(live, rows, gpu):
    """The mask buffer for `rows` capacity rows: live for the leading rows,
    ones for the rest (they lie at and past the live count)."""
    bits = np.ones(32 * ((rows + 31) // 32), np.uint8)
    bits[:live.size] = live
    words = np.packbits(bits, bitorder="little").view(np.uint32)
    return T(words.view(np.int32), gpu)


class Case:
    """Inputs of one (B, dtype, group), made once; oracle results cached."""

    def __init__(self, gpu, B, dtype, group):
        import _dfhip
        import _gridencoder
        offs, S = _grid()
        self.gpu, self.B, self.group = gpu, B, group
        self.rows = int(offs[-1])
        r = np.random.default_rng(1000 + B + group)
        x = (r.random((B, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
        edge = np.array([[1, 1, 1], [-1, -1, -1], [1, -1, 0.5], [0.999999, 0.3, -0.999999]],
                        np.float32)
        n = min(B - 1, 4)
        x[1:1 + n] = edge[:n]  # (row 0 stays inside: B = 1 is a live case)
        self.x = T(x, gpu)
        self.g = (torch.randn(16, group * B, 2, generator=torch.Generator().manual_seed(B)) *
                  0.1).to(dtype).to(gpu)
        # no exact zeros among the gradients: a masked row is never dead by value
        self.g[self.g == 0] = 0.1
        if group == 7:
            x7 = torch.empty(7 * B, 3, device=gpu)
            m7 = torch.zeros(1, dtype=torch.int32, device=gpu)
            full = torch.tensor([B], dtype=torch.int32, device=gpu)
            _dfhip.call("dfhip_shading_stencil", self.x.data_ptr(), full.data_ptr(), B, EPS, 1.0,
                        x7.data_ptr(), m7.data_ptr(), _dfhip.stream())
            torch.cuda.synchronize()
            self.x01 = ((x7.cpu().numpy() + np.float32(1)) / np.float32(2)).astype(np.float32)
        else:
            self.x01 = ((x + np.float32(1)) / np.float32(2)).astype(np.float32)
        self.g_host = self.g.float().cpu().numpy()
        self.offs_dev = T(offs, gpu)
        ne, nc, npf = _gridencoder.grid_backward_binned_scratch(B, offs, 16, 2, group=group)
        self.scratch = (torch.empty(ne, dtype=torch.int32, device=gpu),
                        torch.empty(nc, dtype=torch.int32, device=gpu),
                        torch.empty(npf, device=gpu))
        self.base = torch.randn(self.rows, 2, generator=torch.Generator().manual_seed(3)).to(gpu)
        self._want = {}

    def want(self, m, name, live):
        """f64 oracle over the first m samples / groups with the dead rows zeroed."""
        key = (m, name)
        if key not in self._want:
            offs, S = _grid()
            n = self.group * m
            if n == 0:
                self._want[key] = np.zeros((self.rows, 2))
            else:
                g = self.g_host[:, :n] * live[None, :, None]
                self._want[key] = oracle.grid_encode_backward(g, self.x01[:n], offs, 2, S, 16,
                                                              gridtype=1, blc=False)
        return self._want[key]

    def zeroed(self, live):
        """The gradients with the dead rows zeroed."""
        g = self.g.clone()
        dead = np.flatnonzero(~live)
        if dead.size:
            g[:, T(dead, self.gpu)] = 0
        return g

    def run(self, g, m, mask, walk_mode, accumulate, fast_bin=-1, scratch=None, kept_clean=0):
        import _gridencoder
        offs, S = _grid()
        opts = _gridencoder.BinnedOpts(walk_mode=walk_mode, fast_bin=fast_bin, row_live=mask,
                                       kept_clean=kept_clean)
        m_dev = torch.tensor([m], dtype=torch.int32, device=self.gpu)
        out = self.base.clone() if accumulate else torch.full((self.rows, 2), float("nan"),
                                                              device=self.gpu)
        kw = {"stencil_eps": EPS} if self.group == 7 else {}
        _gridencoder.binned_launcher(g, self.x, 1.0, self.offs_dev, offs, out, self.B, m_dev, 3, 2,
                                     16, S, 16, 1, False, *(scratch or self.scratch),
                                     accumulate=bool(accumulate), opts=opts, **kw)()
        torch.cuda.synchronize()
        return out


_CASES = {}


def _case(gpu, B, dtype, group):
    key = (B, dtype, group)
    if key not in _CASES:
        _CASES[key] = Case(gpu, B, dtype, group)
    return _CASES[key]


def _check(c, m, name, live, mode, acc, fast_bin=-1):
    mask = _pack(live, c.group * c.B, c.gpu)
    want = c.want(m, name, live)
    tag = f"B={c.B} m={m} {name} mode={mode} acc={acc} group={c.group}"
    # the mask is used: non-zero gradients in the dead rows
    plain = c.run(c.g, m, mask, mode, 0, fast_bin)
    np.testing.assert_allclose(plain.double().cpu().numpy(), want, rtol=1e-5,
                               atol=1e-7 * np.abs(want).max(), err_msg=tag)
    got = plain
    if acc:
        got = c.run(c.g, m, mask, mode, 1, fast_bin)
        assert torch.equal(got, c.base + plain), tag
    # null-mask equivalence on zeroed gradients
    gz = c.zeroed(live)
    assert torch.equal(c.run(gz, m, None, mode, acc, fast_bin),
                       c.run(gz, m, mask, mode, acc, fast_bin)), tag
    if not live.any():
        assert torch.equal(got, c.base if acc else torch.zeros_like(got)), tag


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("B", SIZES)
def test_single_samples(gpu, B, dtype, mode, acc):
    c = _case(gpu, B, dtype, 1)
    for m in _counts(B):
        for name, live in _row_patterns(m).items():
            _check(c, m, name, live, mode, acc)


@pytest.mark.parametrize("B", SIZES)
def test_generic_binning_kernel(gpu, B):
    """k_bin (fast_bin = 0) takes the mask as k_bin_fast does."""
    c = _case(gpu, B, torch.float16, 1)
    for m in _counts(B):
        for name, live in _row_patterns(m).items():
            _check(c, m, name, live, 0, 0, fast_bin=0)


def test_stencil_groups_take_no_mask(gpu):
    """group = 7 with a mask is an error (and writes nothing)."""
    c = _case(gpu, 1023, torch.float16, 7)
    mask = _pack(np.ones(7 * c.B, bool), 7 * c.B, gpu)
    with pytest.raises(RuntimeError, match="row_live"):
        c.run(c.g, c.B, mask, -1, 0)
    assert int(c.run(c.g, c.B, None, -1, 0).count_nonzero()) > 0


def test_all_dead_keeps_the_scratch_clean(gpu, group=1):
    """kept_clean calls on one counts scratch zeroed once: all live, all dead,
    a partly dead one, all live again.  Every call equals the same call on a
    fresh scratch with the clearing launch, and leaves its bin totals zero."""
    import _gridencoder
    offs, S = _grid()
    B = 3 * 1024 + 1
    c = _case(gpu, B, torch.float16, group)
    ne, nc, npf = _gridencoder.grid_backward_binned_scratch(B, offs, 16, 2, group=group)
    kept = (torch.empty(ne, dtype=torch.int32, device=gpu),
            torch.zeros(nc, dtype=torch.int32, device=gpu), torch.empty(npf, device=gpu))
    nb = int(sum(-(-int(offs[l + 1] - offs[l]) // 8192) for l in range(16)))
    tiles = -(-B // _gridencoder.grid_backward_binned_tile(group=group))
    o_tot = (tiles * nb + 3) // 4 * 4
    n = group * B
    pats = _row_patterns(B)
    for name in ("all_live", "all_dead", "alternating", "all_dead", "all_live"):
        mask = _pack(pats[name], n, gpu)
        got = c.run(c.g, B, mask, -1, 0, scratch=kept, kept_clean=1)
        fresh = (torch.empty(ne, dtype=torch.int32, device=gpu),
                 torch.full((nc,), -1, dtype=torch.int32, device=gpu),
                 torch.empty(npf, device=gpu))
        assert torch.equal(got, c.run(c.g, B, mask, -1, 0, scratch=fresh)), (group, name)
        assert int(kept[1][o_tot:o_tot + nb * 16].abs().sum()) == 0, (group, name)
        if name == "all_dead":
            assert int(got.count_nonzero()) == 0
        else:
            assert int(got.count_nonzero()) > 0
