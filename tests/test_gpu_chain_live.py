"""The ray chain writes the rows' liveness mask (dfhip_ray_chain_train_live:
one byte per sample row) and the binning reads it (BinnedOpts.row_live_bytes).

* The byte mask against the unpacked bit mask that
  dfhip_grid_field_backward_check_live makes of the gradients the same launch
  wrote: rays that break at T < 1e-4 in the first, a middle and the last
  window, a ray that never breaks, an empty ray, a ray past M, a ray whose
  upstream gradient is exactly zero (with lambda 0 every taken sample's four
  gradients are exactly zero: dead although taken), a ray whose colour
  gradients grad_cast rounds to zero in f16 (live by its density gradient), a
  ray whose one taken sample has an exactly zero density gradient and colour
  gradients of 1e-30 before the cast (zero in f16, non-zero in bf16 and f32:
  only a test made AFTER grad_cast calls the f16 row dead), and a NaN density
  (live).  f16, bf16 and f32 colours.  Every other output equals
  dfhip_ray_chain_train's.
* The binning with the byte mask against the binning with the same mask as
  bits: the entries (ids), the per-segment counts and the bin totals after a
  binning-only call, and the table gradient of the whole call.
* Twenty graph-replayed steps of twin 32 x 32 trainers with
  Trainer.chain_live_mask on against off: equal parameters, Adam moments,
  scaler state, loss and density grid.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 70
W = 16  # samples per window of the chain


def _case(gpu, dtype):
    gen = torch.Generator(device="cpu").manual_seed(47)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    u = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    # (count, sample at which T < 1e-4 first holds or None)
    named = {"first": (5 * W + 3, 4), "middle": (5 * W + 3, 2 * W + 7), "last": (5 * W + 3, 5 * W + 1),
             "window_end": (3 * W, W - 1), "never": (6 * W + 1, None), "empty": (0, None),
             "zero_g": (40, None), "tiny_g": (33, None), "nan_sigma": (20, None),
             # opaque at its first sample: w = 1, T = 0, the running colour equals the final
             # one and ws = 1, so the density gradient is dt * (+-0) whatever the upstream
             "cast_zero": (5, 0)}
    counts = [c for c, _ in named.values()]
    counts += [int(v) for v in torch.randint(0, 41, (N - 1 - len(counts),), generator=gen)]
    counts.append(20)  # the final ray: past the capacity
    num = torch.tensor(counts, dtype=torch.int64)
    off = torch.cumsum(num, 0) - num
    M = int(off[-1]) + 7
    rows = (M + 16 + 15) // 16 * 16
    idx = {k: i for i, k in enumerate(named)}
    sigma = u(rows) * 2.0
    deltas = torch.stack([0.01 + 0.02 * u(rows), 0.01 + 0.02 * u(rows)], 1)
    for k, (c, at) in named.items():
        if at is not None:  # empty space, then one opaque sample
            o = int(off[idx[k]])
            sigma[o:o + at], sigma[o + at] = 0.0, 1e6
    sigma[int(off[idx["nan_sigma"]]) + 3] = float("nan")
    g_image = r(3, N) * 0.1
    g_image[:, idx["zero_g"]] = 0.0
    g_image[:, idx["tiny_g"]] = 1e-9
    g_image[:, idx["cast_zero"]] = 1e-30  # g * w = 1e-30: 0 as f16, non-zero as bf16 / f32
    d = r(N, 3)
    t = lambda x: x.to(gpu)  # noqa: E731
    return dict(M=M, rows=rows, rays=t(torch.stack([torch.arange(N), off, num], 1).to(torch.int32)),
                sigma=t(sigma), deltas=t(deltas), rgbs=t(u(rows, 3).to(dtype)),
                d=t(d / d.norm(dim=1, keepdim=True)), nears=t(torch.full((N,), 0.2)),
                fars=t(torch.full((N,), 2.0)),
                w=[t(x) for x in (r(64, 39) * 0.2, r(64) * 0.1, r(3, 64) * 0.2, r(3) * 0.1)],
                g_image=t(g_image), scale=torch.full((1,), 512.0, device=gpu), dtype=dtype,
                off=off, num=num, idx=idx, named=named)


def _chain(c, gpu, lam, live):
    import _dfhip
    from _dfhip import call, ptr, stream
    f = lambda *s: torch.full(s, -7.0, device=gpu)  # noqa: E731
    b = dict(ws=f(N), depth=f(N), image=f(N, 3), out_image=f(3, N), out_depth=f(N),
             mask=torch.full((N,), 77, dtype=torch.uint8, device=gpu), grad_image=f(N, 3),
             grad_ws=f(N), partial=f(int(_dfhip.load().dfhip_ray_head_partial_floats(N))),
             grads=[torch.full_like(x, -7.0) for x in c["w"]], loss=f(),
             found_inf=torch.zeros(1, device=gpu), grad_sigma=f(c["rows"]),
             grad_rgb=torch.full((c["rows"], 3), -7.0, dtype=c["dtype"], device=gpu),
             live=torch.full((c["rows"],), 77, dtype=torch.uint8, device=gpu))
    call("dfhip_ray_chain_train" + ("_live" if live else ""), _dfhip._DTYPE[c["dtype"]],
         ptr(c["sigma"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), c["M"], N, 1e-4,
         ptr(b["ws"]), ptr(b["depth"]), ptr(b["image"]), ptr(c["d"]), ptr(c["nears"]),
         ptr(c["fars"]), *[ptr(x) for x in c["w"]], ptr(b["out_image"]), ptr(b["out_depth"]),
         ptr(b["mask"]), ptr(c["g_image"]), ptr(b["grad_image"]), ptr(b["grad_ws"]),
         ptr(b["partial"]), *[ptr(x) for x in b["grads"]], ptr(c["scale"]), lam, ptr(b["loss"]),
         ptr(b["found_inf"]), 0, ptr(b["grad_sigma"]), ptr(b["grad_rgb"]),
         *((ptr(b["live"]),) if live else ()), stream())
    torch.cuda.synchronize()
    return b


def _field_bits(c, gpu, grad_sigma, grad_rgb):
    """The bit mask dfhip_grid_field_backward_check_live makes of the
    gradients, unpacked to one byte per row."""
    import _fieldmlp
    rows = c["rows"]
    dtype = torch.float16 if c["dtype"] == torch.float32 else c["dtype"]  # the field's element
    gen = torch.Generator(device="cpu").manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    enc = (r(rows, 32) * 0.5).to(dtype).to(gpu)
    xyz = (torch.rand(rows, 3, generator=gen) * 2 - 1).to(gpu)
    ws = [(r(*s) * 0.2).to(gpu) for s in ((64, 32), (64,), (64, 64), (64,), (4, 64), (4,))]
    d_enc = torch.empty(16, rows, 2, dtype=dtype, device=gpu)
    partial = torch.empty(_fieldmlp.backward_parts(rows) * _fieldmlp.params_count(), device=gpu)
    grads = [torch.empty_like(w) for w in ws]
    words = torch.full(((rows + 31) // 32,), -1, dtype=torch.int32, device=gpu)
    m_dev = torch.tensor([c["M"]], dtype=torch.int32, device=gpu)
    _fieldmlp.grid_field_backward(enc, xyz, 1.0, ws, grad_sigma, grad_rgb, d_enc, partial, grads,
                                  torch.zeros(17, dtype=torch.int32, device=gpu), 0, 0.0, 0, 0,
                                  False, None, None, 0, m_dev, row_live=words)
    torch.cuda.synchronize()
    return np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:rows]


@pytest.mark.parametrize("lam", [1e-3, 0.0], ids=["entropy", "lambda0"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32],
                         ids=["f16", "bf16", "f32"])
def test_chain_bytes_equal_field_backward_bits(gpu, dtype, lam):
    c = _case(gpu, dtype)
    plain, got = _chain(c, gpu, lam, False), _chain(c, gpu, lam, True)
    for name in plain:  # the mask changes no other output (bits: the NaN ray)
        if name == "live":
            continue
        for x, y in zip(*[v if isinstance(v, list) else [v] for v in (plain[name], got[name])]):
            assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), name
    M, off, num, idx = c["M"], c["off"], c["num"], c["idx"]
    live = got["live"].cpu().numpy()
    assert set(np.unique(live[:M])) <= {0, 1} and (live[M:] == 77).all()
    bits = _field_bits(c, gpu, got["grad_sigma"], got["grad_rgb"])
    np.testing.assert_array_equal(live[:M], bits[:M])
    assert not bits[M:(M + 31) // 32 * 32].any()

    def ray(k):
        o = int(off[idx[k]])
        return live[o:o + int(num[idx[k]])]
    for k, (cnt, at) in c["named"].items():  # live up to the break, dead after it
        if at is not None and k != "cast_zero":
            assert ray(k)[:at + 1].all() and not ray(k)[at + 1:].any(), k
    assert ray("never").all() and ray("nan_sigma")[3:].all()
    assert not live[int(off[-1]):M].any()  # the ray past M: its clipped rows are zero-filled
    o = int(off[idx["tiny_g"]])
    if dtype == torch.float16:  # the colour gradients round to zero; live by the density's
        assert not got["grad_rgb"][o:o + 33].float().any() and ray("tiny_g").all()
    # the taken sample's density gradient is exactly zero and its colour gradients are 1e-30
    # before the cast: dead only where the cast rounds them to zero
    o = int(off[idx["cast_zero"]])
    assert float(got["grad_sigma"][o]) == 0.0
    assert bool(got["grad_rgb"][o].float().any()) == (dtype != torch.float16)
    assert ray("cast_zero")[0] == (dtype != torch.float16) and not ray("cast_zero")[1:].any()
    # exactly-zero gradients of taken samples: dead unless the entropy term feeds them
    assert ray("zero_g").all() == (lam != 0.0) and ray("zero_g").any() == (lam != 0.0)


# ---------------------------------------------------------------- the binning

@functools.lru_cache(maxsize=None)
def _grid():
    from gridencoder.grid import level_offsets
    pls = np.exp2(np.log2(2048 / 16) / 15)
    offs = level_offsets(16, 2, 3, 16, pls, 16, False)
    return offs, float(np.log2(pls))


@pytest.mark.parametrize("fast_bin", [-1, 0], ids=["k_bin_fast", "k_bin"])
@pytest.mark.parametrize("B,m", [(1, 1), (1024 + 17, 1024 + 17), (3 * 1024 + 1, 2 * 1024 + 5)])
def test_binning_with_bytes_equals_binning_with_bits(gpu, B, m, fast_bin):
    import _gridencoder
    offs, S = _grid()
    gen = torch.Generator().manual_seed(B)
    x = (torch.rand(B, 3, generator=gen) * 2 - 1).to(gpu)
    g = (torch.randn(16, B, 2, generator=gen) * 0.1).half().to(gpu)
    live = torch.rand(B, generator=gen) < 0.7
    live[1000:1060] = False  # a dead run across the tile and word boundaries
    g[:, ~live.to(gpu)] = 0
    by = live.to(torch.uint8).to(gpu) * 3  # any nonzero byte is live
    by[m:] = 1                             # (rows at and past the live count are not read)
    bits = np.ones(32 * ((B + 31) // 32), np.uint8)
    bits[:m] = live[:m].numpy()
    words = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).to(gpu)
    offs_dev = torch.from_numpy(np.ascontiguousarray(offs)).to(gpu)
    m_dev = torch.tensor([m], dtype=torch.int32, device=gpu)
    ne, nc, npf = _gridencoder.grid_backward_binned_scratch(B, offs, 16, 2)

    def run(phase, **mask):
        scratch = (torch.zeros(ne, dtype=torch.int32, device=gpu),
                   torch.zeros(nc, dtype=torch.int32, device=gpu), torch.zeros(npf, device=gpu))
        out = torch.full((int(offs[-1]), 2), float("nan"), device=gpu)
        opts = _gridencoder.BinnedOpts(fast_bin=fast_bin, **mask)
        _gridencoder.binned_launcher(g, x, 1.0, offs_dev, offs, out, B, m_dev, 3, 2, 16, S, 16, 1,
                                     False, *scratch, phase=phase, opts=opts)()
        torch.cuda.synchronize()
        return scratch, out
    (e1, c1, _), _ = run(1, row_live=words)
    (e2, c2, _), _ = run(1, row_live_bytes=by)
    T = _gridencoder.grid_backward_binned_tile()

    def ids(e):  # each (tile, slice) segment's ids as a set: waves append in arrival order
        e = e.view(torch.int16)
        return e[:e.numel() // T * T].view(-1, T).sort(dim=1).values
    assert torch.equal(ids(e1), ids(e2)) and torch.equal(c1, c2)  # ids; counts and totals
    assert int(c1.count_nonzero()) > 0
    _, t1 = run(3, row_live=words)
    _, t2 = run(3, row_live_bytes=by)
    _, t0 = run(3)
    assert torch.equal(t1, t2) and torch.equal(t0, t2) and bool(torch.isfinite(t2).all())
    with pytest.raises(RuntimeError, match="exclusive"):
        run(3, row_live=words, row_live_bytes=by)


# ---------------------------------------------------------------- the whole step

STEPS = 20  # crosses a density-grid refresh
SWITCHES = ("chain_live_mask",)
_RUNS = {}


def _trained(off):
    """The state after STEPS steps with switch `off` off (None: all on)."""
    if off not in _RUNS:
        import bench
        tr, dt = bench.make_trainer(32, 5, 0, 1, True, graph=True)
        tr.opt.iters = 50
        for name in SWITCHES:
            assert getattr(tr, name) is True  # default on
        if off is not None:
            setattr(tr, off, False)
        for i in range(STEPS):
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        g = next(iter(tr._graphs.values()))
        nat = g.native
        assert nat is not None and g.optimizer_in_graph and nat.ray_chain
        assert nat.chain_live == (off is None)
        m = int(nat.m_field[0])
        dead = int(((nat.grad_sigma[:m] == 0) & (nat.grad_albedo[:m] == 0).all(dim=1)).sum())
        if nat.chain_live:  # the mask the step used marks exactly the dead rows
            assert int((nat.row_live_bytes[:m] == 0).sum()) == dead
        assert 0.02 <= dead / m <= 0.98
        st = tr.optimizer.state_dict()["state"]
        _RUNS[off] = dict(
            loss=g.loss.clone(), params=[p.detach().clone() for p in tr.model.parameters()],
            moments=[st[i][k].clone() for i in st for k in ("step", "exp_avg", "exp_avg_sq")],
            scale=(float(tr.scaler.get_scale()), int(tr.scaler._growth_tracker)),
            grid=tr.model.density_grid.clone(), counter=tr.model.step_counter.clone(),
            emb_grad=tr.model.encoder.embeddings.grad.clone())
        del tr, dt, g, nat
    return _RUNS[off]


@pytest.mark.parametrize("switch", SWITCHES)
def test_twenty_steps_switch_on_equals_off(gpu, switch):
    a, b = _trained(None), _trained(switch)
    assert torch.equal(a["loss"], b["loss"]) and a["scale"] == b["scale"]
    for name in ("params", "moments"):
        for k, (x, y) in enumerate(zip(a[name], b[name])):
            assert torch.equal(x, y), (name, k)
    for name in ("grid", "counter", "emb_grad"):
        assert torch.equal(a[name], b[name]), name
