"""The lemma behind the train marcher's chain-free path (csrc/march_common.h,
"chain-free wave march"), on a pure-Python model of one 64-lane window.

Model: lane j is occupied or empty; an occupied lane's successor is j + 1, an
empty lane's is any lane in (j, 64] (64 = beyond the window: the model does
not even ask that skips be monotonic, which the kernel's are).  The visit
chain follows the successors from a start lane; the samples are the occupied
lanes on it.  A CONFLICT is an occupied lane o with j < o < nxt_j for some
empty lane j, visited or not: what the kernel tests per lane.

Lemma: without a conflict the samples are exactly the occupied lanes from the
start lane on.  No GPU.
"""
import numpy as np

LANES = 64
WINDOWS = 4000


def _window(r):
    # cells of 1-5 candidates, each occupied with the window's density; an
    # empty lane skips to the end of its cell, and now and then 1-3 lanes or
    # anywhere further (what rounding at a face, or nothing physical, would do)
    density = r.choice([0.05, 0.125, 0.5, 0.9])
    lanes = np.arange(LANES)
    cell_end = np.zeros(LANES, np.int64)
    occ = np.zeros(LANES, bool)
    j = 0
    while j < LANES:
        e = min(j + int(r.integers(1, 6)), LANES)
        cell_end[j:e] = e
        occ[j:e] = r.random() < density
        j = e
    wild = r.random(LANES) < r.choice([0.0, 0.02, 0.2])
    far = np.where(r.random(LANES) < 0.8, r.integers(1, 4, LANES), r.integers(1, LANES + 1, LANES))
    nxt = np.minimum(np.where(wild, cell_end + far, cell_end), LANES)
    nxt[occ] = lanes[occ] + 1
    return occ, nxt, int(r.integers(0, LANES))


def _chain_samples(occ, nxt, start):
    out, j = [], start
    while j < LANES:
        if occ[j]:
            out.append(j)
        j = int(nxt[j])
    return out


def _conflict(occ, nxt):
    """The kernel's test: every empty lane against the first occupied lane above it."""
    for j in np.flatnonzero(~occ):
        above = np.flatnonzero(occ[j + 1:])
        if len(above) and j + 1 + above[0] < nxt[j]:
            return True
    return False


def test_no_conflict_means_every_occupied_lane_is_sampled():
    r = np.random.default_rng(0)
    clean = dirty = differs = 0
    for _ in range(WINDOWS):
        occ, nxt, start = _window(r)
        assert np.all(nxt > np.arange(LANES))
        want = [j for j in range(start, LANES) if occ[j]]
        got = _chain_samples(occ, nxt, start)
        if _conflict(occ, nxt):
            dirty += 1
            differs += got != want
        else:
            clean += 1
            assert got == want, (occ, nxt, start)
    # both branches are exercised, and the condition is not idle: with a
    # conflict the chain does drop occupied lanes in some windows
    assert clean >= WINDOWS // 10, clean
    assert dirty >= WINDOWS // 10, dirty
    assert differs >= 10, differs
