"""Shaded frames of the fused persistent inference renderer (csrc/render.hip,
dfhip_render_rays_infer_shaded): the textureless, lambertian and normal views
of test_step / test_gui (reference nerf/utils.py:414-418,616-671).

The pin is the n_step = 1 inference loop built here from the kernels the train
path already runs (march_rays -> dfhip_shading_stencil -> the grid field over
the 7 M rows -> dfhip_shading_forward -> composite_rays), each of which an
existing test pins to oracle/: the fused launch must equal it bit for bit.
There is no end-to-end CPU-oracle render: a central difference of two expf
densities amplifies last-bit differences between the device's and the host's
expf without bound where the two densities are close, so no tolerance for it
can be derived."""
import numpy as np
import pytest
import torch

from scenes import camera_rays, sphere_bitfield

pytestmark = pytest.mark.gpu

EPS = 1e-2  # network_grid.py:90 finite_difference_normal epsilon
MODES = ("textureless", "lambertian", "normal")
CODES = {"albedo": 0, "textureless": 1, "lambertian": 2, "normal": 3}


def _model(gpu, seed=0, scale=0.5, occupancy="sphere", quads=True):
    import main
    from nerf.network_grid import NeRFNetwork
    torch.manual_seed(seed)
    opt = main.parse_opt(["--text", "render", "-O"])
    m = NeRFNetwork(opt).to(gpu)
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-scale, scale)
    if occupancy == "sphere":
        m.density_bitfield.copy_(torch.from_numpy(sphere_bitfield(0.6, 0.003, seed)).to(gpu))
    elif occupancy == "full":
        m.density_bitfield.fill_(255)
    else:
        with torch.autocast("cuda", dtype=torch.float16):
            m.update_extra_state()
    m.infer_quads = quads
    m.eval()
    return m


_MODELS = {}


def _shared_model(gpu, seed, scale, occupancy, quads=True):
    """Models that tests only read (no test changes their state)."""
    key = (seed, scale, occupancy, quads)
    if key not in _MODELS:
        _MODELS[key] = _model(gpu, seed, scale, occupancy, quads)
    return _MODELS[key]


def _rays(gpu, h, w, seed, radius=1.6):
    o, d = camera_rays(h, w, seed, radius=radius)
    return torch.from_numpy(o).to(gpu), torch.from_numpy(d).to(gpu)


def _light(gpu, v=(0.3, 0.8, -0.5)):
    l = np.asarray(v, np.float32)
    return torch.from_numpy(l / np.linalg.norm(l)).to(gpu)


def _np(ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


def _fused(m, rays_o, rays_d, shading, light, ratio, perturb=False, T_thresh=1e-4,
           max_steps=128):
    import raymarching
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, m.aabb_infer)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        field = m.native_infer_field(shading, rays_o)
        assert field is not None
        torch.manual_seed(7)
        out = m._infer_fused(rays_o, rays_d, nears, fars, field, perturb, 0.0, max_steps,
                             T_thresh, shading=shading, light_d=light, ambient_ratio=ratio)
    return _np(out)


def _torch_loop(m, rays_o, rays_d, shading, light, ratio, n_step_max, max_steps=128):
    import raymarching
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, m.aabb_infer)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        torch.manual_seed(7)
        out = m._infer_loop(rays_o, rays_d, nears, fars, light, ratio, shading, False, 0.0,
                            max_steps, 1e-4, n_step_max=n_step_max)
    return _np(out)


def _kernel_loop(m, rays_o, rays_d, shading, light, ratio, perturb=False, T_thresh=1e-4,
                 max_steps=128, near_faces=None):
    """The n_step = 1 inference loop (renderer.py:496-532) of the existing
    kernels, through the bindings nerf/native_step.py uses, on the table, quads
    and weights the renderer caches (so after a fused frame).  near_faces: a
    list that receives the number of composited samples within EPS of +-bound."""
    import _dfhip
    import _fieldmlp
    import raymarching
    from _dfhip import call, ptr, stream
    _, weights, table, quads = m.__dict__["_infer_operands"]
    enc = m.encoder
    S, Hb = float(np.log2(enc.per_level_scale)), int(enc.base_resolution)
    dev = rays_o.device
    N = rays_o.shape[0]
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, m.aabb_infer)
    ws = torch.zeros(N, device=dev)
    depth = torch.zeros(N, device=dev)
    image = torch.zeros(N, 3, device=dev)
    alive = torch.arange(N, dtype=torch.int32, device=dev)
    rays_t = nears.clone()
    # the normal view takes the kernel's f32 normal; its colour output is unused
    code = CODES["textureless" if shading == "normal" else shading]
    faces = 0
    torch.manual_seed(7)
    step = 0
    while step < max_steps:
        n = alive.shape[0]
        if n <= 0:
            break
        xyzs, dirs, deltas = raymarching.march_rays(
            n, 1, alive, rays_t, rays_o, rays_d, m.bound, m.density_bitfield, m.cascade,
            m.grid_size, nears, fars, 128, perturb if step == 0 else False, 0.0, max_steps)
        cap = xyzs.shape[0]
        m_dev = torch.full((1,), cap, dtype=torch.int32, device=dev)
        m7 = torch.empty(1, dtype=torch.int32, device=dev)
        xyz7 = torch.empty(7 * cap, 3, device=dev)
        call("dfhip_shading_stencil", ptr(xyzs), ptr(m_dev), cap, EPS, float(m.bound), ptr(xyz7),
             ptr(m7), stream())
        sigma7 = torch.empty(7 * cap, device=dev)
        albedo7 = torch.empty(7 * cap, 3, dtype=torch.half, device=dev)
        _fieldmlp.grid_field_forward(xyz7, m.bound, table, enc.offsets, S, Hb, enc.gridtype_id,
                                     bool(enc.align_corners), weights, None, sigma7, albedo7, m7,
                                     quads=quads)
        sigma = torch.empty(cap, device=dev)
        color = torch.empty(cap, 3, dtype=torch.half, device=dev)
        normal = torch.empty(cap, 3, device=dev)
        partial = torch.empty(int(_dfhip.load().dfhip_shading_partial_doubles(cap)),
                              dtype=torch.float64, device=dev)
        call("dfhip_shading_forward", ptr(sigma7), ptr(albedo7), ptr(dirs), ptr(light),
             float(ratio), EPS, code, ptr(m_dev), cap, ptr(sigma), ptr(color), ptr(normal),
             ptr(partial), 0.0, None, None, stream())
        # composite_rays takes f32 colours (the loop's autocast casts them; exact)
        rgbs = (normal + 1) / 2 if shading == "normal" else color.float()
        if near_faces is not None:
            edge = xyzs.abs().amax(1) >= m.bound - EPS
            faces += int((edge & (deltas[:, 0] > 0)).sum())
        raymarching.composite_rays(n, 1, alive, rays_t, sigma, rgbs, deltas, ws, depth, image,
                                   T_thresh)
        alive = alive[alive >= 0]
        step += 1
    if near_faces is not None:
        near_faces.append(faces)
    return _np((ws, depth, image))


def _assert_same(got, want, msg=""):
    for g, w, name in zip(got, want, ("weights_sum", "depth", "image")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {msg}")


# ---- 1. bit-exact against the loop of the existing kernels

@pytest.mark.parametrize("shading,ratio,quads,occupancy,scale,seed,hw", [
    ("textureless", 0.1, True, "sphere", 0.5, 0, (48, 40)),
    ("lambertian", 0.1, False, "grid", 1.0, 2, (37, 29)),
    ("normal", 0.1, True, "grid", 1.0, 2, (48, 40)),
    ("lambertian", 0.0, True, "sphere", 2.0, 1, (37, 29)),
    ("textureless", 0.1, False, "sphere", 0.5, 0, (16, 16)),
    ("normal", 0.1, False, "sphere", 2.0, 1, (37, 29)),
])
def test_shaded_bit_exact_vs_kernel_loop(gpu, shading, ratio, quads, occupancy, scale, seed, hw):
    m = _shared_model(gpu, seed, scale, occupancy, quads)
    rays_o, rays_d = _rays(gpu, hw[0], hw[1], seed)
    light = _light(gpu)
    got = _fused(m, rays_o, rays_d, shading, light, ratio)
    assert (m.__dict__["_infer_operands"][3] is not None) == quads
    want = _kernel_loop(m, rays_o, rays_d, shading, light, ratio)
    assert (want[0] > 0).sum() > 100  # the scene is not empty
    _assert_same(got, want)


def test_shaded_perturbed_bit_exact(gpu):
    """perturb=True: the first march of each ray moves by the same torch.rand
    draw the loop makes (renderer.py:522)."""
    m = _shared_model(gpu, 3, 1.0, "sphere")
    rays_o, rays_d = _rays(gpu, 32, 32, 3)
    light = _light(gpu, (-0.6, 0.2, 0.7))
    got = _fused(m, rays_o, rays_d, "lambertian", light, 0.1, perturb=True)
    want = _kernel_loop(m, rays_o, rays_d, "lambertian", light, 0.1, perturb=True)
    assert (want[0] > 0).sum() > 100
    _assert_same(got, want)


# ---- 2. the stencil clamp at the box faces

@pytest.mark.parametrize("shading", ["lambertian", "normal"])
def test_shaded_stencil_clamp_at_box_faces(gpu, shading):
    """Every cell occupied: the rays are sampled from the box faces inward,
    so stencil points of the first samples leave the box and are clamped."""
    m = _shared_model(gpu, 4, 1.0, "full")
    rays_o, rays_d = _rays(gpu, 16, 16, 4)
    light = _light(gpu)
    got = _fused(m, rays_o, rays_d, shading, light, 0.1, max_steps=64)
    faces = []
    want = _kernel_loop(m, rays_o, rays_d, shading, light, 0.1, max_steps=64, near_faces=faces)
    assert faces[0] > 0  # composited samples within eps of +-bound
    assert (want[0] > 0).sum() > 100
    _assert_same(got, want)


# ---- 3. invariants that need no reference

def test_shaded_invariants(gpu):
    m = _shared_model(gpu, 0, 0.5, "sphere")
    rays_o, rays_d = _rays(gpu, 48, 40, 0)
    light = _light(gpu)
    aw, ad, ai = _fused(m, rays_o, rays_d, "albedo", None, 1.0)
    assert (aw > 0).sum() > 100
    for shading in MODES:
        w, d, i = _fused(m, rays_o, rays_d, shading, light, 0.1)
        np.testing.assert_array_equal(w, aw, err_msg=shading)
        np.testing.assert_array_equal(d, ad, err_msg=shading)
        if shading == "normal":
            hit = w > 0
            q = i[hit] / w[hit, None]
            assert q.min() >= 0.0 and q.max() <= 1.0
            assert np.all(i[~hit] == 0)
    # ambient ratio 1: the lambertian term is exactly 1
    w, d, i = _fused(m, rays_o, rays_d, "textureless", light, 1.0)
    for ch in range(3):
        np.testing.assert_array_equal(i[:, ch], aw)  # the fma order of weights_sum
    w, d, i = _fused(m, rays_o, rays_d, "lambertian", light, 1.0)
    np.testing.assert_array_equal(i, ai)


# ---- 4. against the torch loop (today's path for these frames)

# one f16 spacing of normal @ l moves lam16 and the colour by up to four
# spacings of 2^-11 below 1; the image is a convex sum of colours
IMG_TOL = {"textureless": 2.0 ** -9, "lambertian": 2.0 ** -9,
           "normal": 1e-5}  # f32 division against a reciprocal multiply


@pytest.mark.parametrize("shading", MODES)
def test_shaded_vs_torch_loop_nstep1(gpu, shading):
    m = _shared_model(gpu, 2, 1.0, "grid")
    rays_o, rays_d = _rays(gpu, 37, 29, 2)
    light = _light(gpu)
    fw, fd, fi = _fused(m, rays_o, rays_d, shading, light, 0.1)
    lw, ld, li = _torch_loop(m, rays_o, rays_d, shading, light, 0.1, n_step_max=1)
    assert (lw > 0).sum() > 100
    np.testing.assert_array_equal(fw, lw)  # the densities are the same field kernel's
    np.testing.assert_array_equal(fd, ld)
    err = np.abs(fi - li).max()
    print(f"\n{shading}: max |image - torch loop| = {err:.3e} (bound {IMG_TOL[shading]:.3e})")
    assert err <= IMG_TOL[shading]


def test_shaded_vs_torch_loop_default_schedule(gpu):
    """n_step up to 8: the schedule's 1-ulp sample shifts on top (the 1e-4 /
    1e-3 of test_fused_infer_vs_default_schedule)."""
    m = _shared_model(gpu, 2, 1.0, "grid")
    rays_o, rays_d = _rays(gpu, 37, 29, 2)
    light = _light(gpu)
    fw, fd, fi = _fused(m, rays_o, rays_d, "lambertian", light, 0.1)
    lw, ld, li = _torch_loop(m, rays_o, rays_d, "lambertian", light, 0.1, n_step_max=8)
    np.testing.assert_allclose(fw, lw, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(fi, li, rtol=1e-4, atol=1e-4 + IMG_TOL["lambertian"])
    np.testing.assert_allclose(fd, ld, rtol=1e-4, atol=1e-3)


# ---- 5. edge cases

def _direct(m, rays_o, rays_d, shading, light, ratio, fill, T_thresh=1e-4, max_steps=128,
            order=None, cl=6):
    """The binding itself on caller-owned outputs filled with `fill`."""
    import _fieldmlp
    import raymarching
    _, weights, table, quads = m.__dict__["_infer_operands"]
    enc = m.encoder
    dev = rays_o.device
    N = rays_o.shape[0]
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, m.aabb_infer)
    ws = torch.full((N,), fill, device=dev)
    depth = torch.full((N,), fill, device=dev)
    image = torch.full((N, 3), fill, device=dev)
    work = torch.empty(4, dtype=torch.int32, device=dev)
    _fieldmlp.render_rays_infer_shaded(
        rays_o, rays_d, nears, fars, None, m.bound, 0.0, max_steps, m.cascade, m.grid_size,
        m.density_bitfield, T_thresh, table, enc.offsets, float(np.log2(enc.per_level_scale)),
        int(enc.base_resolution), enc.gridtype_id, bool(enc.align_corners), weights, ws, depth,
        image, work, shading, light, ratio, EPS, quads=quads, order=order, chunk_log2=cl)
    return _np((ws, depth, image))


def test_shaded_edge_cases(gpu):
    """Rays that miss the box, an early T_thresh, a tiny max_steps and an
    empty bitfield; every ray is written (NaN-poisoned outputs)."""
    m = _model(gpu, 5, 2.0, "sphere")
    rays_o, rays_d = _rays(gpu, 16, 16, 5, radius=3.0)  # most rays miss the cube
    light = _light(gpu)
    nan = float("nan")
    for shading, T_thresh, max_steps in (("lambertian", 1e-4, 128), ("textureless", 0.5, 128),
                                         ("normal", 1e-4, 3), ("lambertian", 0.5, 3)):
        got = _fused(m, rays_o, rays_d, shading, light, 0.1, T_thresh=T_thresh,
                     max_steps=max_steps)
        want = _kernel_loop(m, rays_o, rays_d, shading, light, 0.1, T_thresh=T_thresh,
                            max_steps=max_steps)
        _assert_same(got, want, msg=f"{shading} {T_thresh} {max_steps}")
        poisoned = _direct(m, rays_o, rays_d, shading, light, 0.1, nan, T_thresh, max_steps)
        _assert_same(poisoned, want, msg=f"poisoned {shading}")  # no NaN left: all written
    assert (want[0] > 0).any() and (want[0] == 0).any()  # rays that hit and rays that miss
    m.density_bitfield.zero_()
    for shading in MODES:
        for out in _direct(m, rays_o, rays_d, shading, light, 0.1, nan):
            assert not out.any()  # all zero, none NaN


# ---- 6. queue layouts

def test_shaded_queue_layouts(gpu):
    """Pixel order, ordered chunks (cl 0, 3, 6) and 8 x 8 tiles give
    bit-identical shaded frames and equal sample counts."""
    m = _model(gpu, 3, 1.0, "sphere")
    h, w = 40, 48
    rays_o, rays_d = _rays(gpu, h, w, 3)
    light = _light(gpu)
    runs = []
    variants = [(0, 6, 0), (1, 0, 0), (1, 3, 0), (1, 6, 0), (1, 6, w), (2, 6, w)]
    for flag, cl, tile in variants:
        m.infer_order, m.infer_chunk_log2, m.infer_tile_w = flag, cl, tile
        out = _fused(m, rays_o, rays_d, "lambertian", light, 0.1)
        runs.append((out, m.last_infer_work.cpu().numpy()[:3].copy()))
    ref, ref_work = runs[0]
    assert (ref[0] > 0).sum() > 100 and ref_work[1] > 0
    for (got, work), v in zip(runs[1:], variants[1:]):
        _assert_same(got, ref, msg=str(v))
        np.testing.assert_array_equal(work[1:3], ref_work[1:3], err_msg=str(v))


# ---- 7. API

@pytest.mark.parametrize("shading", MODES)
def test_render_api_takes_the_fused_path(gpu, shading):
    m = _model(gpu, 6, 1.0, "sphere")
    rays_o, rays_d = _rays(gpu, 24, 24, 6)
    light = _light(gpu)
    kw = dict(staged=True, perturb=False, max_steps=128)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m.render(rays_o[None], rays_d[None], **kw)
        albedo_samples = m.last_infer_work.cpu().numpy().view(np.uint32)[1:3].copy()
        m.last_infer_work = None
        out = m.render(rays_o[None], rays_d[None], shading=shading, light_d=light,
                       ambient_ratio=0.1, **kw)
        assert m.last_infer_work is not None  # the fused launch ran
        samples = m.last_infer_work.cpu().numpy().view(np.uint32)[1:3]
        assert samples[0] > 0
        np.testing.assert_array_equal(samples, albedo_samples)
        m.native_infer = False
        m.last_infer_work = None
        ref = m.render(rays_o[None], rays_d[None], shading=shading, light_d=light,
                       ambient_ratio=0.1, **kw)
        assert m.last_infer_work is None  # the host loop
    g = {k: out[k].float().cpu().numpy() for k in ("image", "depth", "weights_sum")}
    r = {k: ref[k].float().cpu().numpy() for k in ("image", "depth", "weights_sum")}
    # the loop runs its default schedule (n_step up to 8)
    np.testing.assert_allclose(g["weights_sum"], r["weights_sum"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["image"], r["image"], rtol=1e-4, atol=1e-4 + IMG_TOL[shading])
    np.testing.assert_allclose(g["depth"], r["depth"], rtol=1e-4, atol=1e-3)


def test_render_api_bf16_keeps_the_host_loop(gpu):
    """The shaded kernels round at the f16 points: under bf16 autocast the
    shaded field is not offered (albedo still is)."""
    m = _shared_model(gpu, 0, 0.5, "sphere")
    x = torch.zeros(4, 3, device=gpu)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert m.native_infer_field("lambertian", x) is None
    with torch.autocast("cuda", dtype=torch.float16):
        assert m.native_infer_field("lambertian", x) is not None
        assert m.native_infer_field("phong", x) is None


def _trainer(gpu, seed=9):
    import main
    from nerf.network_grid import NeRFNetwork
    from nerf.utils import Trainer
    torch.manual_seed(seed)
    opt = main.parse_opt(["--text", "relight", "-O", "--max_steps", "128"])
    model = NeRFNetwork(opt)
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-1.0, 1.0)
    tr = Trainer("relight", opt, model, None, device=gpu, workspace=None, ema_decay=0.95,
                 fp16=True, use_checkpoint="scratch", mute=True)
    model.density_bitfield.copy_(torch.from_numpy(sphere_bitfield(0.6, 0.003, seed)).to(gpu))
    model.eval()
    return tr


def test_trainer_eval_entry_points(gpu):
    """test_step honours the batch's shading / ambient_ratio / light_d keys
    (absent: today's albedo frame, bit for bit); eval_step returns the entropy
    regulariser; test_gui returns numpy frames at full and half resolution."""
    tr = _trainer(gpu)
    m = tr.model
    h = w = 24
    rays_o, rays_d = _rays(gpu, h, w, 9)
    light = _light(gpu)
    data = {"rays_o": rays_o[None], "rays_d": rays_d[None], "H": h, "W": w}
    shaded = dict(data, shading="lambertian", ambient_ratio=0.1, light_d=light)
    opts = dict(vars(tr.opt))
    with torch.autocast("cuda", dtype=torch.float16):
        rgb, dep = tr.test_step(data)
        assert m.infer_tile_w == w
        with torch.no_grad():
            want = m.render(rays_o[None], rays_d[None], staged=True, perturb=False, light_d=None,
                            ambient_ratio=1.0, shading="albedo", force_all_rays=True,
                            bg_color=None, **opts)
        np.testing.assert_array_equal(rgb.cpu().numpy(),
                                      want["image"].reshape(1, h, w, 3).cpu().numpy())
        np.testing.assert_array_equal(dep.cpu().numpy(),
                                      want["depth"].reshape(1, h, w).cpu().numpy())
        m.last_infer_work = None
        rgb_s, dep_s = tr.test_step(shaded)
        assert m.last_infer_work is not None
        with torch.no_grad():
            want = m.render(rays_o[None], rays_d[None], staged=True, perturb=False,
                            light_d=light, ambient_ratio=0.1, shading="lambertian",
                            force_all_rays=True, bg_color=None, **opts)
        np.testing.assert_array_equal(rgb_s.cpu().numpy(),
                                      want["image"].reshape(1, h, w, 3).cpu().numpy())
        np.testing.assert_array_equal(dep_s.cpu().numpy(), dep.cpu().numpy())
        assert np.abs(rgb_s.cpu().numpy() - rgb.cpu().numpy()).max() > 1e-3  # relit
        # eval_step: lambda_entropy * mean binary entropy of the clamped weights_sum
        e_rgb, e_dep, loss = tr.eval_step(shaded)
        np.testing.assert_array_equal(e_rgb.cpu().numpy(), rgb_s.cpu().numpy())
        np.testing.assert_array_equal(e_dep.cpu().numpy(), dep_s.cpu().numpy())
        a = want["weights_sum"].reshape(1, h, w).clamp(1e-5, 1 - 1e-5)
        ent = (-a * torch.log2(a) - (1 - a) * torch.log2(1 - a)).mean()
        assert tr.opt.lambda_entropy > 0
        assert float(loss) == float(tr.opt.lambda_entropy * ent)
    # test_gui: pose [4, 4] numpy, light as (theta, phi) degrees, EMA restored
    o, d = camera_rays(1, 1, 9, radius=1.6)
    fwd = -o[0] / np.linalg.norm(o[0])
    right = np.cross(fwd, np.array([0.0, -1.0, 0.0]))
    right /= np.linalg.norm(right)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(right, fwd), fwd, o[0]
    H = W = 32
    intr = np.array([40.0, 40.0, W / 2, H / 2])
    before = [p.detach().clone() for p in m.parameters()]
    for p in tr.ema.shadow:  # an average that differs from the parameters
        p.mul_(0.5)
    for scale in (1, 0.5):
        out = tr.test_gui(pose, intr, W, H, downscale=scale, light_d=(60.0, 30.0),
                          ambient_ratio=0.1, shading="lambertian")
        assert out["image"].shape == (H, W, 3) and out["depth"].shape == (H, W)
        assert out["image"].dtype == np.float32 and np.isfinite(out["image"]).all()
        assert isinstance(out["image"], np.ndarray) and isinstance(out["depth"], np.ndarray)
    half = out["image"]  # nearest neighbour: 2 x 2 blocks of the 16 x 16 frame
    np.testing.assert_array_equal(half[0::2, 0::2], half[1::2, 1::2])
    for p, b in zip(m.parameters(), before):
        assert torch.equal(p, b)  # the trained parameters are back


def test_shaded_abi_errors(gpu):
    m = _shared_model(gpu, 0, 0.5, "sphere")
    rays_o, rays_d = _rays(gpu, 16, 16, 0)
    light = _light(gpu)
    _fused(m, rays_o, rays_d, "lambertian", light, 0.1)  # the cached operands
    with pytest.raises(RuntimeError, match="light is NULL"):
        _direct(m, rays_o, rays_d, "lambertian", None, 0.1, 0.0)
    with pytest.raises(RuntimeError, match="shading must be DFHIP_SHADING_TEXTURELESS"):
        _direct(m, rays_o, rays_d, 7, light, 0.1, 0.0)
    with pytest.raises(RuntimeError, match="albedo shading is dfhip_render_rays_infer_ordered"):
        _direct(m, rays_o, rays_d, "albedo", light, 0.1, 0.0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _direct(m, rays_o, rays_d, "lambertian", light.cpu(), 0.1, 0.0)
