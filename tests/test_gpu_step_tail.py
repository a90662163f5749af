"""GPU tests of the train step's folded tail launches.  Every comparison is
exact (torch.equal): none of the folds changes an arithmetic operation or a
summation order.

* overflow check where the gradients are written (dfhip_binned_opts.found_inf,
  dfhip_grid_field_backward_check, dfhip_ray_head_backward_check) against the
  re-reading k_nonfinite of dfhip_adam_amp_step_lr_dev;
* the replayed step's optimizer entry (dfhip_adam_amp_step_tail: no check
  launch for covered tensors, the live count stored by the finalize) against
  dfhip_adam_amp_step_lr_dev;
* the merged parameter-gradient sums (dfhip_param_grad_sums) against the two
  separate sum launches;
* the corner quads built by rider workgroups of the march's count launch
  (dfhip_march_rays_train_count_staged_quads) against the two launches.  The
  quads kernels are fixed at the field's 16 levels (dfhip_grid_quads refuses
  any other L), so the layout is a small 16-level one with wrapped levels,
  not a 3-level one;
* the whole graph-replayed step with every switch on against every switch
  off.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INTERVAL = 7  # growth interval of the scaler in the optimizer tests


# ---------------------------------------------------------------- Adam state

class AdamState:
    """Tensors of one dfhip_adam_amp_step* call: per tensor p / g / m / v /
    step, the scaler's scale / growth tracker / found_inf, one device lr."""

    def __init__(self, sizes, gpu, seed=0, unaligned=(), step0=3.0, scale=1024.0, tracker=0):
        gen = torch.Generator(device="cpu").manual_seed(seed)

        def make(n, k, mul=1.0, positive=False):
            # a base that is 4-byte but not 16-byte aligned for tensors in `unaligned`
            t = torch.randn(n + 1, generator=gen) * mul
            if positive:
                t = t.abs()
            t = t.to(gpu)
            return t[1:] if k in unaligned else t[:n]
        self.p = [make(n, k) for k, n in enumerate(sizes)]
        self.g = [make(n, k, 5.0) for k, n in enumerate(sizes)]
        self.m = [make(n, k, 0.1) for k, n in enumerate(sizes)]
        self.v = [make(n, k, 0.01, True) for k, n in enumerate(sizes)]
        self.step = [torch.full((), step0 + k, device=gpu) for k in range(len(sizes))]
        self.scale = torch.full((1,), scale, device=gpu)
        self.tracker = torch.full((1,), tracker, dtype=torch.int32, device=gpu)
        self.found_inf = torch.zeros(1, device=gpu)
        self.lr = torch.tensor([1e-2, 3e-3], device=gpu)

    def clone(self):
        import copy
        c = copy.copy(self)
        # keep every tensor's alignment: clone the storage-backed base layout
        def cl(ts):
            out = []
            for t in ts:
                off = (t.data_ptr() % 16) // 4
                buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
                pad = (off - (buf.data_ptr() % 16) // 4) % 4
                v = buf[pad:pad + t.numel()]
                v.copy_(t)
                out.append(v)
            return out
        c.p, c.g, c.m, c.v = cl(self.p), cl(self.g), cl(self.m), cl(self.v)
        c.step = [t.clone() for t in self.step]
        c.scale, c.tracker = self.scale.clone(), self.tracker.clone()
        c.found_inf, c.lr = self.found_inf.clone(), self.lr.clone()
        return c

    def tensors(self):
        return (self.p + self.m + self.v + self.step +
                [self.scale, self.tracker, self.found_inf])


def _adam(st, tail=False, mask=0, live=None, live_rows=None, live_row=None):
    import _dfhip
    n = len(st.p)
    vp, f = ctypes.c_void_p * n, ctypes.c_float * n
    arr = lambda ts: vp(*[t.data_ptr() or None for t in ts])  # noqa: E731
    args = [n, arr(st.p), arr(st.g), arr(st.m), arr(st.v), arr(st.step),
            (ctypes.c_uint64 * n)(*[t.numel() for t in st.p]),
            (ctypes.c_int32 * n)(*[k % 2 for k in range(n)]), st.lr.data_ptr(),
            f(*[0.9] * n), f(*[0.99] * n), f(*[1e-15] * n),
            f(*[0.01 if k % 3 == 2 else 0.0 for k in range(n)]),  # weight decay on some
            st.scale.data_ptr(), st.tracker.data_ptr(), st.found_inf.data_ptr(), 2.0, 0.5,
            INTERVAL]
    if tail:
        _dfhip.call("dfhip_adam_amp_step_tail", *args, mask, _dfhip.ptr(live),
                    _dfhip.ptr(live_rows), _dfhip.ptr(live_row), _dfhip.stream())
    else:
        _dfhip.call("dfhip_adam_amp_step_lr_dev", *args, _dfhip.stream())


def _same(a, b):
    for k, (x, y) in enumerate(zip(a.tensors(), b.tensors())):
        assert torch.equal(x, y), k
    # NaNs compare unequal: the states here stay finite
    assert all(bool(torch.isfinite(t).all()) for t in a.p)


SIZES = [0, 1, 2047, 2048, 2049, 4100]


@pytest.mark.parametrize("found", [0, 1])
@pytest.mark.parametrize("tracker", [0, INTERVAL - 1])
def test_tail_entry_equals_three_launches(gpu, found, tracker):
    """dfhip_adam_amp_step_tail with nothing covered against
    dfhip_adam_amp_step_lr_dev on identical state: sizes around a workgroup's
    2,048-element chunk, an empty tensor, one tensor on a base that is not
    16-byte aligned; a raised and a clear found_inf; the growth tracker one
    step before the interval; three calls in a row."""
    a = AdamState(SIZES, gpu, seed=1, unaligned=(5,), tracker=tracker)
    assert a.p[5].data_ptr() % 16 != 0
    b = a.clone()
    assert b.p[5].data_ptr() % 16 != 0
    for call in range(3):
        for st in (a, b):
            st.found_inf.fill_(float(found if call == 0 else 0))
        if found and call == 0:  # the re-reading check must agree: a real inf
            a.g[3][17] = b.g[3][17] = float("inf")
        elif call == 1:
            a.g[3][17] = b.g[3][17] = 0.5
        _adam(a, tail=True)
        _adam(b)
        torch.cuda.synchronize()
        _same(a, b)
        assert float(a.found_inf) == 0.0
    if found:
        assert float(a.scale) == 512.0  # halved once; two clean steps do not reach the interval
    elif tracker == INTERVAL - 1:
        assert float(a.scale) == 2048.0  # grew on the first call


def test_finalize_stores_live_count(gpu):
    """The finalize launch also copies the sample counter into the row named
    by a device word; every other row stays."""
    a = AdamState([2049, 100], gpu, seed=2)
    live = torch.tensor([12345, 77], dtype=torch.int32, device=gpu)
    rows = torch.full((16, 2), -1, dtype=torch.int32, device=gpu)
    row = torch.tensor([5], dtype=torch.int32, device=gpu)
    _adam(a, tail=True, live=live, live_rows=rows, live_row=row)
    torch.cuda.synchronize()
    want = torch.full((16, 2), -1, dtype=torch.int32, device=gpu)
    want[5] = live
    assert torch.equal(rows, want)


def test_uncovered_tensors_are_still_checked(gpu):
    """A non-finite gradient in an uncovered tensor skips the step exactly as
    the three-launch entry does; in a covered one the tail trusts its writer
    (flag clear -> the step runs, as documented)."""
    a = AdamState([100, 3000, 50], gpu, seed=3)
    a.g[1][2999] = float("nan")
    b = a.clone()
    _adam(a, tail=True, mask=0b101)
    _adam(b)
    torch.cuda.synchronize()
    _same(a, b)
    assert float(a.scale) == 512.0


# ---------------------------------------------------------------- overflow fold

def _grid_case(gpu, accumulate, where, bad, flag):
    """The binned embedding backward of a 2-level dense layout (64 + 512 rows,
    align_corners: sample (0,0,0) owns the first row, (1,1,1) the last) on 70
    samples, reporting to `flag`.  where: None, "first" or "last"."""
    import _gridencoder
    from test_gpu_grid_layouts import Lay, _binned, _lbc
    from test_gpu_encoders import T
    lay = Lay(np.array([0, 64, 576], np.int32), 2, 2, 4, 1.0, True)
    rng = np.random.default_rng(11)
    x = rng.random((70, 3), dtype=np.float32)
    x[0], x[1] = 0.0, 1.0
    g = (rng.normal(size=(70, 4)) * 0.1).astype(np.float16)
    gemb = None
    if accumulate:
        gemb = T((rng.normal(size=(576, 2)) * 0.1).astype(np.float32), gpu)
    if where == "first":
        g[0, 0] = bad            # level 0, sample at the origin: row 0, weight 1
    elif where == "last":
        g[1, 2] = bad            # level 1, sample at (1,1,1): row 575, weight 1
    opts = _gridencoder.BinnedOpts(found_inf=flag)
    out = _binned(_lbc(g, lay, gpu), T(x, gpu), 0.0, lay, 1, 70, None, gpu, opts=opts,
                  accumulate=accumulate, gemb=gemb)
    if where == "first":
        assert not bool(torch.isfinite(out[0, 0]))
    elif where == "last":
        assert not bool(torch.isfinite(out[575, 0]))
    return out


def _field_case(gpu, accumulate, bad, flag, defer=False):
    """The field backward on 70 rows writing its six weight gradients; `bad`
    (None: finite) is the density gradient of row 3, so every partial that
    row's workgroup writes is non-finite."""
    import _fieldmlp
    gen = torch.Generator(device="cpu").manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    M = 70
    enc = (r(M, 32) * 0.5).half().to(gpu)
    xyz = (torch.rand(M, 3, generator=gen) * 2 - 1).to(gpu)
    ws = [(r(64, 32) * 0.2).to(gpu), (r(64) * 0.1).to(gpu), (r(64, 64) * 0.2).to(gpu),
          (r(64) * 0.1).to(gpu), (r(4, 64) * 0.2).to(gpu), (r(4) * 0.1).to(gpu)]
    gs = (r(M) * 0.1).to(gpu)
    if bad is not None:
        gs[3] = bad
    grgb = (r(M, 3) * 0.1).half().to(gpu)
    d_enc = torch.empty(16, M, 2, dtype=torch.float16, device=gpu)
    partial = torch.empty(_fieldmlp.backward_parts(M) * _fieldmlp.params_count(), device=gpu)
    grads = [(r(*w.shape) * 0.1).to(gpu) if accumulate else torch.full_like(w, float("nan"))
             for w in ws]
    _fieldmlp.grid_field_backward(enc, xyz, 1.0, ws, gs, grgb, d_enc, partial, grads,
                                  torch.zeros(17, dtype=torch.int32, device=gpu), 0, 0.0, 0, 0,
                                  False, None, None, 0, None, accumulate=accumulate,
                                  found_inf=flag, defer_sum=defer)
    return ws, grads, partial


def _head_case(gpu, N, bad, flag, combined=False, defer=False, entropy=True):
    """The ray head's backward on N rays writing the background network's four
    gradients; `bad` is the upstream colour gradient of ray 0."""
    import _dfhip
    from _dfhip import call, ptr, stream
    gen = torch.Generator(device="cpu").manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    d = r(N, 3)
    d = (d / d.norm(dim=1, keepdim=True)).to(gpu)
    ws = torch.rand(N, generator=gen).to(gpu)
    g_image = (r(3, N) * 0.1).to(gpu)
    if bad is not None:
        g_image[1, 0] = bad
    w = [(r(64, 39) * 0.2).to(gpu), (r(64) * 0.1).to(gpu), (r(3, 64) * 0.2).to(gpu),
         (r(3) * 0.1).to(gpu)]
    grads = [torch.full_like(t, float("nan")) for t in w]
    partial = torch.empty(int(_dfhip.load().dfhip_ray_head_partial_floats(N)), device=gpu)
    grad_image, grad_ws = torch.empty(N, 3, device=gpu), torch.empty(N, device=gpu)
    one = torch.ones(1, device=gpu)
    loss = torch.full((), -7.0, device=gpu)
    if not combined:
        call("dfhip_ray_head_backward_check", N, ptr(g_image), ptr(ws), ptr(d),
             *[ptr(t) for t in w], None, ptr(grad_image), ptr(grad_ws), None, ptr(partial),
             *[ptr(t) for t in grads], ptr(one) if entropy else None, 1e-3,
             ptr(loss) if entropy else None, ptr(flag), stream())
        return w, grads, partial, loss, (grad_image, grad_ws)
    depth, image = torch.rand(N, generator=gen).to(gpu), torch.rand(N, 3, generator=gen).to(gpu)
    nears, fars = torch.full((N,), 0.2, device=gpu), torch.full((N,), 2.0, device=gpu)
    outs = (torch.empty(3, N, device=gpu), torch.empty(N, device=gpu),
            torch.empty(N, dtype=torch.uint8, device=gpu))
    head = (N, ptr(ws), ptr(depth), ptr(image), ptr(d), ptr(nears), ptr(fars),
            *[ptr(t) for t in w], *[ptr(t) for t in outs], ptr(g_image), ptr(grad_image),
            ptr(grad_ws), ptr(partial), *[ptr(t) for t in grads], ptr(one), 1e-3, ptr(loss))
    if flag is None and not defer:
        call("dfhip_ray_head_forward_backward_entropy_loss", *head, stream())
    else:
        call("dfhip_ray_head_forward_backward_entropy_loss_check", *head, ptr(flag), int(defer),
             stream())
    return w, grads, partial, loss, (grad_image, grad_ws, *outs, ws)


CASES = [("none", None)] + [(w, b) for w in ("first", "last", "mlp", "head")
                            for b in (float("inf"), float("nan"))]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("where,bad", CASES)
def test_overflow_check_at_the_writers(gpu, accumulate, where, bad):
    """The writers' flag, fed to the tail entry with every tensor covered,
    against the three-launch entry re-reading the same gradients: flag 0 and
    an equal update for finite gradients; flag 1, p / m / v / step counts
    untouched and the scale halved for one inf or NaN in the first grid row,
    the last grid row, an MLP partial or a head partial."""
    flag = torch.zeros(1, device=gpu)
    gemb = _grid_case(gpu, accumulate, where if where in ("first", "last") else None, bad, flag)
    _, fgrads, _ = _field_case(gpu, accumulate, bad if where == "mlp" else None, flag)
    _, hgrads, _, _, _ = _head_case(gpu, 70, bad if where == "head" else None, flag)
    torch.cuda.synchronize()
    grads = [gemb] + fgrads + hgrads
    finite = all(bool(torch.isfinite(g).all()) for g in grads)
    assert finite == (where == "none")
    assert float(flag) == (0.0 if finite else 1.0)

    a = AdamState([g.numel() for g in grads], gpu, seed=4)
    a.g = [g.reshape(-1) for g in grads]
    b = a.clone()
    before = a.clone()
    a.found_inf.copy_(flag)
    _adam(a, tail=True, mask=(1 << len(grads)) - 1)
    _adam(b)
    torch.cuda.synchronize()
    _same(a, b)
    assert float(a.found_inf) == 0.0
    if finite:
        assert float(a.scale) == 1024.0 and not torch.equal(a.p[0], before.p[0])
    else:
        assert float(a.scale) == 512.0
        for x, y in zip(a.p + a.m + a.v + a.step, before.p + before.m + before.v + before.step):
            assert torch.equal(x, y)


# ---------------------------------------------------------------- merged sums

def _rows_with_parts(parts):
    import _fieldmlp
    M = 16
    while _fieldmlp.backward_parts(M) != parts:
        M += 16
        assert M < 1 << 16
    return M


@pytest.mark.parametrize("parts", [1, 16, 17])
@pytest.mark.parametrize("N,entropy", [(1, True), (64, False), (65, True)])
def test_merged_sums_equal_separate_launches(gpu, parts, N, entropy):
    """dfhip_param_grad_sums on the partials of a deferring field backward
    (1, 16 and 17 workgroups' partials) and a deferring head backward (1, 64
    and 65 rays: one and two workgroups; with and without the entropy block)
    against the two launches that sum by themselves."""
    import _fieldmlp
    from _dfhip import call, ptr, stream
    M = _rows_with_parts(parts)
    gen = torch.Generator(device="cpu").manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    enc = (r(M, 32) * 0.5).half().to(gpu)
    xyz = (torch.rand(M, 3, generator=gen) * 2 - 1).to(gpu)
    ws = [(r(64, 32) * 0.2).to(gpu), (r(64) * 0.1).to(gpu), (r(64, 64) * 0.2).to(gpu),
          (r(64) * 0.1).to(gpu), (r(4, 64) * 0.2).to(gpu), (r(4) * 0.1).to(gpu)]
    gs, grgb = (r(M) * 0.1).to(gpu), (r(M, 3) * 0.1).half().to(gpu)
    offs = torch.zeros(17, dtype=torch.int32, device=gpu)

    def field(defer):
        d_enc = torch.empty(16, M, 2, dtype=torch.float16, device=gpu)
        partial = torch.empty(parts * _fieldmlp.params_count(), device=gpu)
        grads = [torch.full_like(w, float("nan")) for w in ws]
        _fieldmlp.grid_field_backward(enc, xyz, 1.0, ws, gs, grgb, d_enc, partial, grads, offs, 0,
                                      0.0, 0, 0, False, None, None, 0, None, defer_sum=defer)
        return grads, partial, d_enc
    want_f, _, want_d = field(False)
    got_f, partial, got_d = field(True)
    _, want_h, _, want_loss, want_o = _head_case(gpu, N, None, None, combined=True)
    hw, got_h, hpartial, got_loss, got_o = _head_case(gpu, N, None, None, combined=True, defer=True)
    flag = torch.zeros(1, device=gpu)
    call("dfhip_param_grad_sums", ptr(partial), parts, *[ptr(g) for g in got_f], 0, N,
         ptr(hpartial), *[ptr(g) for g in got_h], ptr(got_o[-1]) if entropy else None, 1e-3,
         ptr(got_loss) if entropy else None, ptr(flag), stream())
    torch.cuda.synchronize()
    assert torch.equal(want_d, got_d)
    for k, (x, y) in enumerate(zip(want_f + want_h, got_f + got_h)):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), k
    for x, y in zip(want_o, got_o):
        assert torch.equal(x, y)
    assert float(got_loss) == (float(want_loss) if entropy else -7.0)
    assert float(want_loss) != -7.0 and float(flag) == 0.0


# ---------------------------------------------------------------- quads in the march

@pytest.mark.parametrize("N", [1, 16, 17])
def test_quads_in_march_equal_two_launches(gpu, N):
    """N = 1, 16, 17 rays (a march workgroup holds 16): counts, ray records,
    block totals and stage rows equal dfhip_march_rays_train_count_staged's;
    the table copy and the quads equal dfhip_grid_quads's, on a 16-level tiled
    layout whose upper levels wrap and whose row count is no multiple of the
    riders' 1,024-row span."""
    import _fieldmlp
    import _raymarching
    from gridencoder.grid import level_offsets
    from scenes import march_inputs
    from test_gpu_encoders import T
    rays_o, rays_d, nears, fars, noises, bf = march_inputs(8, 8, seed=0)
    sel = slice(27, 27 + N)  # centre rays: they hit the sphere
    ro, rd, ne, fa, no = (T(np.ascontiguousarray(a[sel]), gpu)
                          for a in (rays_o, rays_d, nears, fars, noises))
    grid = T(bf, gpu)
    pls, H, log2T = 1.4, 4, 11
    offs_host = level_offsets(16, 2, 3, H, pls, log2T, False)
    rows = int(offs_host[-1])
    assert rows % 1024 != 0 and rows > 4096
    sizes = np.diff(offs_host)
    assert sizes[0] < 2 ** log2T and (sizes == 2 ** log2T).sum() >= 3  # dense and wrapped levels
    offs = T(offs_host, gpu)
    emb = torch.empty(rows, 2, device=gpu).uniform_(-1, 1,
                                                    generator=torch.Generator(gpu).manual_seed(3))
    S, max_steps = float(np.log2(pls)), 64

    def run(fused):
        rays = torch.full((N, 3), -1, dtype=torch.int32, device=gpu)
        counter = torch.zeros(2, dtype=torch.int32, device=gpu)
        sums = torch.full((_raymarching.march_rays_train_scratch_ints(N),), -1, dtype=torch.int32,
                          device=gpu)
        stage = torch.zeros(_raymarching.march_rays_train_stage_floats(N, max_steps), device=gpu)
        table = torch.full((rows, 2), float("nan"), dtype=torch.float16, device=gpu)
        quads = torch.full((rows, 4), -1, dtype=torch.int32, device=gpu)
        args = (ro, rd, grid, 1.0, 0.0, max_steps, N, 1, 128, ne, fa, rays, counter, no, sums,
                stage)
        if fused:
            _raymarching.march_rays_train_count_staged_quads(*args, emb, offs, S, H, 1, False,
                                                             table, quads)
        else:
            _raymarching.march_rays_train_count_staged(*args)
            _fieldmlp.grid_quads(emb, offs, S, H, 1, False, table, quads)
        torch.cuda.synchronize()
        return rays, counter, sums, stage, table.view(torch.int16), quads
    want, got = run(False), run(True)
    assert int(want[1][0]) > 0 and int(want[1][1]) == N
    for k, (x, y) in enumerate(zip(want, got)):
        assert torch.equal(x, y), k


# ---------------------------------------------------------------- whole step

SWITCHES = ("fold_overflow_check", "merged_grad_sums", "store_live_count", "quads_in_march")


def test_whole_step_switches_on_equal_off(gpu):
    """Twin trainers at 32 x 32, every switch on against every switch off, 20
    graph-replayed steps crossing a density refresh: parameters, Adam state,
    scaler state, step_counter rows, density grid and bitfield are equal."""
    import bench

    def run(on):
        tr, dt = bench.make_trainer(32, 5, 0, 1, True, graph=True)
        tr.opt.iters = 50
        for s in SWITCHES:
            assert getattr(tr, s) is True  # default on
            setattr(tr, s, on)
        for i in range(20):
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        return tr
    a, b = run(True), run(False)
    ga, gb = next(iter(a._graphs.values())), next(iter(b._graphs.values()))
    assert ga.native is not None and ga.optimizer_in_graph and gb.optimizer_in_graph
    assert ga.stores_live_count() and not gb.stores_live_count()
    assert ga.native.found_inf is not None and ga.native.merged_sums and ga.native.quads_in_march
    assert gb.native.found_inf is None and not gb.native.merged_sums
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb)
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    for i in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][name], sb[i][name]), (i, name)
    assert float(a.scaler.get_scale()) == float(b.scaler.get_scale())
    assert int(a.scaler._growth_tracker) == int(b.scaler._growth_tracker)
    assert float(a._native_opt.found_inf) == 0.0 == float(b._native_opt.found_inf)
    assert torch.equal(a.model.step_counter, b.model.step_counter)
    assert int(a.model.step_counter[:, 0].min()) > 0  # every row written
    assert torch.equal(a.model.density_grid, b.model.density_grid)
    assert torch.equal(a.model.density_bitfield, b.model.density_bitfield)
    assert torch.equal(ga.loss, gb.loss)
