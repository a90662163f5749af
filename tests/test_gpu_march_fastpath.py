"""The train marcher's chain-free path (csrc/march_common.h) against the CPU
oracle, with its per-call options (dfhip_march_rays_train_count_opts,
_emit_opts): rows of the settings matrix of test_gpu_march_settings (24 x 24
rays, seed 0), each run three ways:

  default   mode 0, guard 0: the product
  exact     mode 1: the exact path for every ray
  guard     mode 0, guard_ulps = 1 << 18 (about 4 dt at t in [1, 2)): conflicts
            are reported wholesale, so the restart on the exact path is what
            produces most rays' rows

through the count + re-marching emit pair and through the staged pair, at the
row's full N and at N = 1 and N = 17 (no multiple of the rays per workgroup).
Counts, offsets, xyzs, dirs and deltas are bit-equal to the oracle every way.

The counters (stats[0]: rays marched again on the exact path, stats[1]: rays
finished chain-free) are checked against a numpy restatement of which rays
may start chain-free at all (ray_all_arith: dt_gamma == 0, t0 positive and
normal, dt neither a tie nor out of range in ulps of any binade from t0's to
that of far + dt): every such ray is in exactly one counter, no other ray in
either.
  * guard 0: at most 1 % of the rays with samples restart (a numpy model of
    the candidate sequence found 0-4 of 16,384 rays with a conflict on a 50 %
    random bitfield, none on spheres and blobs).
  * guard 1 << 18 on the random-bitfield rows: at least half of the rays with
    samples restart: on rows a and c, where every ray starts chain-free.  Rows
    f, j and l cannot meet that over all their rays under any design, since
    their rays start in, or cross, a window that is not arithmetic (f: the tie
    binade [0.5, 1); j, at min_near 0.05, and l, at t0 = 0 or below 2^-7: dt
    above 2^23 ulps of t) and are on the exact path from their first window;
    there the share is taken over the rays that start chain-free (measured:
    none do, so on these rows the modes check only that nothing changes).
  * row b (dt_gamma > 0): both counters stay zero, in both passes.
"""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_march_settings import case
from test_gpu_raymarching import T

gpu_test = pytest.mark.gpu

ROWS = ["a", "c", "f", "j", "l", "k_full", "k_empty", "b"]
MODES = {"default": {}, "exact": {"mode": 1}, "guard": {"guard_ulps": 1 << 18}}
SIZES = [None, 1, 17]   # None: the whole row


def _starts_chain_free(c, n):
    """ray_all_arith of march_common.h restated in numpy f32, for the rays
    march_wave does not return from at once (t0 < far)."""
    _, _, nears, fars, noises, _ = c.inputs
    nears, fars, noises = nears[:n], fars[:n], noises[:n]
    dt_min, dt_max = c.dt_consts()
    step = np.clip(nears.astype(np.float64) * c.dt_gamma, dt_min, dt_max)
    with np.errstate(over="ignore"):
        t0 = (step * noises.astype(np.float64) + nears.astype(np.float64)).astype(np.float32)
    live = t0 < fars
    if c.dt_gamma != 0:
        return np.zeros(n, bool), live
    dt = np.float32(min(dt_max, max(dt_min, np.float32(0))))
    with np.errstate(over="ignore"):
        hi = (fars + dt).astype(np.float32)
    b0, b1 = t0.view(np.uint32), hi.view(np.uint32)
    ok = live & (b0 >= 0x00800000) & (b0 < 0x7F800000) & (b1 < 0x7F800000)
    for i in np.flatnonzero(ok):
        for ex in range(int(b0[i] >> 23), int(b1[i] >> 23) + 1):
            D = np.ldexp(np.float64(dt), 150 - ex)   # exact: a power-of-two scale
            if not (0.5 <= D < 8388608.0 and abs(D - np.rint(D)) != 0.5):
                ok[i] = False
                break
    return ok, live


def _run(gpu, c, n, staged, opts):
    import _raymarching
    o, d, nears, fars, noises, bf = c.inputs
    o, d = T(o[:n], gpu), T(d[:n], gpu)
    ne, fa, no, b = T(nears[:n], gpu), T(fars[:n], gpu), T(noises[:n], gpu), T(bf, gpu)
    cap = n * c.max_steps + 256
    rays = torch.empty(n, 3, dtype=torch.int32, device=gpu)
    counter = torch.zeros(2, dtype=torch.int32, device=gpu)
    bs = torch.empty(_raymarching.march_rays_train_scratch_ints(n), dtype=torch.int32, device=gpu)
    xyzs = torch.full((cap, 3), 7.0, device=gpu)
    dirs = torch.full((cap, 3), 7.0, device=gpu)
    deltas = torch.full((cap, 2), 7.0, device=gpu)
    st_count = torch.zeros(2, dtype=torch.int32, device=gpu)
    st_emit = torch.zeros(2, dtype=torch.int32, device=gpu)
    args = (o, d, b, c.bound, c.dt_gamma, c.max_steps, n, c.C, c.H)
    if staged:
        stage = torch.full((_raymarching.march_rays_train_stage_floats(n, c.max_steps),), 5.0,
                           device=gpu)
        _raymarching.march_rays_train_count_staged(*args, ne, fa, rays, counter, no, bs, stage,
                                                   stats=st_count, **opts)
        _raymarching.march_rays_train_emit_staged(d, c.max_steps, n, cap, xyzs, dirs, deltas,
                                                  rays, bs, 128, stage)
    else:
        _raymarching.march_rays_train_count(*args, ne, fa, rays, counter, no, bs,
                                            stats=st_count, **opts)
        _raymarching.march_rays_train_emit(*args, cap, ne, fa, xyzs, dirs, deltas, rays, no, bs,
                                           128, stats=st_emit, **opts)
    return xyzs, dirs, deltas, rays, counter, st_count.cpu().tolist(), st_emit.cpu().tolist()


@gpu_test
@pytest.mark.parametrize("staged", [False, True], ids=["split", "staged"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", SIZES, ids=["all", "n1", "n17"])
@pytest.mark.parametrize("name", ROWS)
def test_march_fastpath(gpu, name, size, mode, staged):
    c = case(name)
    n = len(c.counts) if size is None else size
    if name.startswith("k_") and size is not None:
        n += 50   # past the 50 rays that miss the box: 51 and 67, odd as well
    counts = c.counts[:n]
    total = int(counts.sum())
    xyzs, dirs, deltas, rays, counter, st_count, st_emit = _run(gpu, c, n, staged, MODES[mode])

    r = rays.cpu().numpy()
    np.testing.assert_array_equal(r[:, 0], np.arange(n))
    np.testing.assert_array_equal(r[:, 2], counts)
    np.testing.assert_array_equal(r[:, 1], oracle.rays_from_counts(counts)[:, 1])
    assert counter.cpu().tolist() == [total, n]
    np.testing.assert_array_equal(xyzs[:total].cpu().numpy(), c.xyzs[:total])
    np.testing.assert_array_equal(dirs[:total].cpu().numpy(), c.dirs[:total])
    np.testing.assert_array_equal(deltas[:total].cpu().numpy(), c.deltas[:total])
    m_al = total + 128 - total % 128
    for a in (xyzs, dirs, deltas):
        assert torch.all(a[total:m_al] == 0) and torch.all(a[m_al:m_al + 4] == 7.0)

    free, _ = _starts_chain_free(c, n)
    with_samples = int((counts > 0).sum())
    print(f"{name} n={n} {mode} staged={staged}: count pass restarted/chain-free {st_count}, "
          f"emit pass {st_emit}, start chain-free {int(free.sum())}, with samples {with_samples}")
    if mode == "exact" or name == "b":
        assert st_count == [0, 0] and st_emit == [0, 0]
        return
    assert sum(st_count) == int(free.sum())
    if not staged:   # the emit pass marches the rays with samples
        assert sum(st_emit) == int((free & (counts > 0)).sum())
    if mode == "default":
        assert st_count[0] <= 0.01 * with_samples and st_emit[0] <= 0.01 * with_samples
    elif c.kind == "random" and size is None:
        of = int((free & (counts > 0)).sum())
        if name in ("a", "c"):
            assert of == with_samples   # every ray with samples can restart
        assert 2 * st_count[0] >= of, (st_count, of)
