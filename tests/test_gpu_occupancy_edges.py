"""The occupancy-refresh entries of csrc/occupancy.hip called directly
(dfhip_density_grid_ema, dfhip_packbits_mean, dfhip_mean_count) with inputs
chosen for their branches; test_gpu_occupancy.py sees them only through a
trained model's refresh.  The specification is the reference's
update_extra_state (nerf/renderer.py:562-615): the EMA-max over the cells that
were valid (>= 0) before the update, their mean, `min(mean, density_thresh)`
as Python evaluates it (NaN when the mean is NaN), a strict > in the
bitfield, int(sum / total_step).

The grid is a view 64 floats into a larger tensor (16-byte aligned) with 64
more floats after it, all holding a valid-looking sentinel: an index that
escapes its guard changes a sentinel instead of foreign memory."""
import math

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

F32 = np.float32
CELLS, CAS = 8 ** 3, 2
PAD = 64
SENT = 12345.0   # >= 0: a stray access would treat it as a valid cell and rewrite it
DECAY = 0.75     # old * decay is exact for the old values used here


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _padded(gpu, values):
    buf = torch.full((PAD + len(values) + PAD,), SENT, device=gpu)
    grid = buf[PAD:PAD + len(values)]
    grid.copy_(torch.from_numpy(values))
    assert grid.data_ptr() % 16 == 0
    return buf, grid


def _pads_intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


# ---------------------------------------------------------------- dfhip_density_grid_ema

def _old_grid(rng):
    """Old values by cell index mod 8; every value is a small multiple of 2^-8
    or of 2^20, so old * 0.75 and every partial sum of the new values (multiples
    of 2^-12 below 2^40) are exact in f64 in any order, while an f32 sum of
    1e8-scale and 1e-3-scale values is not."""
    i = np.arange(CAS * CELLS)
    k = rng.integers(1, 200, i.size).astype(np.float64)
    old = np.select([i % 8 == 0, i % 8 == 1, i % 8 == 2, i % 8 == 3, i % 8 == 4, i % 8 == 5],
                    [-1.0 + 0 * k, -0.0 * k, 0.0 * k, np.nan * k, k * 2.0 ** 20, k * 2.0 ** -8],
                    k * 2.0 ** -6)
    return old.astype(F32)


def _sigma_for(rng, old):
    """One sigma per cell: below, equal to and above old * decay by turns,
    always > 0 (max(-0, +0) has no defined sign)."""
    od = (old * F32(DECAY)).astype(F32)
    k = rng.integers(1, 200, old.size).astype(np.float64)
    base = np.where(np.isfinite(od) & (od > 0), od, 1.0).astype(np.float64)
    turn = np.arange(old.size) // 8 % 4
    sig = np.select([turn == 0, turn == 1, turn == 2], [base, base / 2, base * 2], k * 2.0 ** -10)
    sig = sig.astype(F32)
    assert np.all(sig > 0) and np.all(sig.astype(np.float64) % 2.0 ** -12 == 0)
    return sig


@pytest.mark.parametrize("n,flavour", [(1, "finite"), (300, "finite"), (512, "finite"),
                                       (1, "inf"), (300, "inf"), (512, "inf"), (300, "nan")])
def test_density_grid_ema(gpu, n, flavour):
    import _dfhip
    from _dfhip import ptr
    rng = np.random.default_rng([n, len(flavour)])
    old = _old_grid(rng)
    sig_cell = _sigma_for(rng, old)
    buf, grid = _padded(gpu, old)
    acc = torch.tensor([3.5, 2.0], dtype=torch.float64, device=gpu)
    want = old.copy()
    new_valid = []
    for cas in range(CAS):
        # n distinct cells of this cascade (n = 1: a valid one), some of the
        # points pointed outside [0, cells) instead
        cells = rng.permutation(CELLS)[:n] if n > 1 else np.array([5 + 8 * cas])
        idx = (cells + cas * CELLS).astype(np.int64)
        sig = sig_cell[idx].copy()
        if n > 1:
            stray = rng.permutation(n)[:12]
            idx[stray[:6]] = -1 - rng.integers(0, PAD, 6)
            idx[stray[6:]] = CAS * CELLS + rng.integers(0, PAD, 6)
            idx[stray[0]], idx[stray[6]] = -1, CAS * CELLS
        inside = (idx >= 0) & (idx < CAS * CELLS)
        hit = np.flatnonzero(inside & (old[np.where(inside, idx, 0)] >= 0))  # points on valid cells
        if flavour != "finite":
            sig[hit[0]] = np.inf
        if flavour == "nan" and cas == 0:
            sig[hit[1]] = np.nan
        ci, si = idx[inside], sig[inside]
        v = want[ci] >= 0
        with np.errstate(invalid="ignore"):
            want[ci[v]] = np.maximum((want[ci[v]] * F32(DECAY)).astype(F32), si[v])
        new_valid += [float(x) for x in want[ci[v]]]
        sig_dev = torch.from_numpy(sig).to(gpu)
        idx_dev = torch.from_numpy(idx.astype(np.int32)).to(gpu)
        _dfhip.call("dfhip_density_grid_ema", ptr(sig_dev), ptr(idx_dev), n, CAS * CELLS, DECAY,
                    ptr(grid), ptr(acc), _dfhip.stream())
        torch.cuda.synchronize()
    got = grid.cpu().numpy()
    assert _pads_intact(buf), "a cell outside the grid was written"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), \
        np.flatnonzero(_bits(got) != _bits(want))[:8]
    untouched = np.isnan(old) | (old < 0)
    assert np.array_equal(_bits(got)[untouched], _bits(old)[untouched])
    a = acc.cpu().numpy()
    assert a[1] == 2 + len(new_valid), (a, len(new_valid))
    want_sum = math.fsum([3.5] + new_valid)
    if flavour == "nan":
        assert np.isnan(want).sum() == np.isnan(old).sum() + 1 and math.isnan(want_sum)
        assert math.isnan(a[0])
    else:
        assert math.isinf(want_sum) == (flavour == "inf")
        assert a[0] == want_sum, (a[0], want_sum)
        if flavour == "finite" and n > 1:  # an f32 accumulation would not be exact
            assert float(np.sum(np.array([3.5] + new_valid, F32), dtype=F32)) != want_sum


def test_density_grid_ema_of_no_points(gpu):
    import _dfhip
    from _dfhip import ptr
    buf, grid = _padded(gpu, _old_grid(np.random.default_rng(0)))
    before = grid.clone()
    acc = torch.tensor([3.5, 2.0], dtype=torch.float64, device=gpu)
    _dfhip.call("dfhip_density_grid_ema", None, None, 0, CAS * CELLS, DECAY, ptr(grid), ptr(acc),
                _dfhip.stream())
    torch.cuda.synchronize()
    assert torch.equal(grid.view(torch.int32), before.view(torch.int32))
    assert acc.tolist() == [3.5, 2.0]


# ---------------------------------------------------------------- dfhip_packbits_mean

# (acc[0], acc[1], density_thresh)
PACK = {
    "mean below the threshold": (1.0, 3.0, 0.5),
    "mean above the threshold": (7.0, 2.0, 0.5),
    "mean equal to the threshold": (1.0, 2.0, 0.5),
    "no valid cell": (5.0, 0.0, 0.5),
    "NaN sum": (float("nan"), 4.0, 0.5),
    "infinite sum": (float("inf"), 4.0, 0.5),
}


@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("case", list(PACK))
def test_packbits_mean(gpu, N, case):
    import _dfhip
    from _dfhip import ptr
    acc0, acc1, density_thresh = PACK[case]
    mean = F32(np.float64(acc0) / np.float64(acc1)) if acc1 > 0 else F32(np.nan)
    # renderer.py:606, as Python evaluates it: NaN when the mean is NaN
    thresh = min(float(mean), density_thresh)
    assert math.isnan(thresh) == (case in ("no valid cell", "NaN sum"))
    rng = np.random.default_rng(N)
    cells = rng.uniform(0, 1, 8 * N).astype(F32)
    t = F32(0.5 if math.isnan(thresh) else thresh)
    # the threshold itself (strict >: bit 0), its two neighbours, a value equal
    # to the mean, an invalid cell, a NaN, an infinity
    plant = np.array([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf)),
                      0.0 if math.isnan(float(mean)) else mean, -1.0, np.nan, np.inf, -0.0], F32)
    pos = rng.permutation(8 * N)[:8]
    cells[pos] = plant
    buf, grid = _padded(gpu, cells)
    want = oracle.packbits(cells, thresh)
    bit = lambda p: int(want[p // 8] >> (p % 8)) & 1  # noqa: E731
    if math.isnan(thresh):
        assert not want.any()
    else:
        assert [bit(p) for p in pos[:3]] == [0, 1, 0] and bit(pos[6]) == 1
        assert (bit(pos[3]) == 0) == (float(mean) <= thresh)
    acc = torch.tensor([acc0, acc1], dtype=torch.float64, device=gpu)
    for with_mean in (True, False):
        bits = torch.full((N + PAD,), 0xA5, dtype=torch.uint8, device=gpu)
        mean_out = torch.full((2,), -7.0, device=gpu) if with_mean else None
        _dfhip.call("dfhip_packbits_mean", ptr(grid), N, ptr(acc), density_thresh, ptr(bits),
                    ptr(mean_out), _dfhip.stream())
        torch.cuda.synchronize()
        got = bits.cpu().numpy()
        assert np.all(got[N:] == 0xA5), "bytes past N were written"
        assert np.array_equal(got[:N], want), \
            f"{case} (thresh {thresh}): {int((got[:N] != want).sum())} of {N} bitfield bytes differ"
        if with_mean:
            m = mean_out.cpu().numpy()
            assert m[1] == -7.0
            assert (np.isnan(m[0]) and np.isnan(mean)) or _bits(m[:1])[0] == _bits([mean])[0], (m, mean)
    assert _pads_intact(buf) and acc.cpu().numpy().tolist()[1] == acc1


def test_packbits_mean_rejects_a_misaligned_grid(gpu):
    import _dfhip
    from _dfhip import ptr
    buf, grid = _padded(gpu, np.zeros(64, F32))
    acc = torch.tensor([1.0, 2.0], dtype=torch.float64, device=gpu)
    bits = torch.full((8,), 0xA5, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="grid must be 16-byte aligned"):
        _dfhip.call("dfhip_packbits_mean", ptr(grid) + 4, 4, ptr(acc), 0.5, ptr(bits), None,
                    _dfhip.stream())
    torch.cuda.synchronize()
    assert bool((bits == 0xA5).all())


# ---------------------------------------------------------------- dfhip_mean_count

def _counter(gpu, seed):
    rng = np.random.default_rng(seed)
    sc = np.empty((64, 2), np.int32)
    sc[:, 0] = rng.integers(0, 2 ** 31, 64)
    sc[::5, 0] = 2 ** 31 - 1
    sc[1::7, 0] = 0
    sc[:, 1] = rng.integers(-2 ** 31, 2 ** 31, 64)  # the ray counts: not part of the mean
    return sc, torch.from_numpy(sc).to(gpu)


@pytest.mark.parametrize("total_step", [1, 15, 16, 64])
def test_mean_count(gpu, total_step):
    import _dfhip
    from _dfhip import ptr
    sc, dev = _counter(gpu, total_step)
    out = torch.full((2,), -99, dtype=torch.int64, device=gpu)
    _dfhip.call("dfhip_mean_count", ptr(dev), total_step, ptr(out), _dfhip.stream())
    torch.cuda.synchronize()
    total = sum(int(x) for x in sc[:total_step, 0])
    assert total_step in (1, 64) or total % total_step != 0  # a quotient that truncates
    assert out.tolist() == [int(total / total_step), -99]


def test_mean_count_limits(gpu):
    import _dfhip
    from _dfhip import ptr
    _, dev = _counter(gpu, 0)
    out = torch.full((2,), -99, dtype=torch.int64, device=gpu)
    _dfhip.call("dfhip_mean_count", ptr(dev), 0, ptr(out), _dfhip.stream())
    with pytest.raises(RuntimeError, match="total_step must be <= 64"):
        _dfhip.call("dfhip_mean_count", ptr(dev), 65, ptr(out), _dfhip.stream())
    torch.cuda.synchronize()
    assert out.tolist() == [-99, -99]
