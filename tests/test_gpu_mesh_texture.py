"""Texture bake of export_mesh on the GPU (csrc/texture.hip, nerf/mesh.py):
the UV rasteriser, the interpolation and the dilation against the f64 numpy
oracles of tests/test_mesh_texture_host.py, determinism, and the textured
export end to end."""
import numpy as np
import pytest
import torch

from nerf.mesh import BAKE_CHUNK, bake_texture, grid_atlas, rasterize_uv
from test_mesh_texture_host import (HAND_EXPECTED, dilate_ref, interp_f32_error, interp_np,
                                    raster_cases, raster_ref)

pytestmark = pytest.mark.gpu

CASES = raster_cases()
_REF = {}


def _ref(name):
    """The oracle's face ids, xyz and bary of a case (computed once, read-only)."""
    if name not in _REF:
        vt, ft, v, f, H, W = CASES[name]
        fid = raster_ref(vt, ft, H, W)
        xyz, bary = interp_np(vt, ft, v, f, fid, H, W, np.float64)
        for a in (fid, xyz, bary):
            a.setflags(write=False)
        _REF[name] = (fid, xyz, bary)
    return _REF[name]


@pytest.fixture(scope="module")
def f32_error():
    """(xyz, bary) error of the f32 restatement of the kernel's formula against
    the f64 oracle on the cases, measured on the CPU."""
    return interp_f32_error(CASES)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _raster(name, gpu, want_bary=True):
    import _texture
    vt, ft, v, f, H, W = CASES[name]
    vt, ft, v, f = (_dev(a, gpu) for a in (vt, ft, v, f))
    fid = _texture.raster_uv_faces(vt, ft, H, W)
    xyz, bary = _texture.raster_uv_interp(vt, ft, v, f, fid, H, W, want_bary=True)
    return fid, xyz, bary


@pytest.mark.parametrize("name", list(CASES))
def test_raster_face_ids_are_exact(gpu, name):
    fid = _raster(name, gpu)[0].cpu().numpy()
    H, W = CASES[name][4:]
    want = _ref(name)[0]
    assert fid.dtype == np.int32 and fid.shape == (H * W,)
    assert np.array_equal(fid.reshape(H, W), want)
    if name == "hand":
        assert np.array_equal(fid.reshape(H, W), HAND_EXPECTED)
    if name == "atlas5000_512":
        assert len(np.unique(fid)) == 5001  # every face, over many workgroups
    if name in ("empty",):
        assert (fid == -1).all()


def test_raster_walks_large_faces_with_the_whole_wave(gpu):
    """Faces whose bounding boxes exceed the lane-group limit take the
    wave-wide path: one face over 2048 x 2048 and four over 256 x 200."""
    import _texture
    for F, size in ((1, None), (4, (200, 256))):
        vt, ft, H, W = grid_atlas(F, size)
        fid = _texture.raster_uv_faces(_dev(vt, gpu), _dev(ft, gpu), H, W).cpu().numpy()
        assert np.array_equal(fid.reshape(H, W), raster_ref(vt, ft, H, W))


@pytest.mark.parametrize("name", list(CASES))
def test_interpolated_positions_match_the_f64_oracle(gpu, name, f32_error):
    """xyz and bary against the f64 oracle.  The tolerance is 4x the largest
    error of the f32 numpy restatement of the kernel's formula on these cases
    (measured on the CPU: xyz 3.553e-07, bary 1.788e-07, so 1.42e-06 and
    7.2e-07); the factor covers the compiler's freedom of operation order
    under -ffp-contract=off.  Uncovered texels are exactly zero."""
    _, xyz, bary = _raster(name, gpu)
    xyz, bary = xyz.cpu().numpy(), bary.cpu().numpy()
    fid, want_xyz, want_bary = _ref(name)
    ex, eb = f32_error
    err_x = float(np.abs(xyz - want_xyz).max())
    err_b = float(np.abs(bary - want_bary).max())
    print(f"{name}: xyz error {err_x:.3e} (allowed {4 * ex:.3e}), "
          f"bary error {err_b:.3e} (allowed {4 * eb:.3e})")
    assert err_x <= 4 * ex and err_b <= 4 * eb
    off = fid.reshape(-1) < 0
    assert not xyz[off].any() and not bary[off].any()
    if (~off).any():
        assert np.abs(xyz[~off]).max() > 0


def test_interp_without_bary_and_bad_indices(gpu):
    import _texture
    vt, ft, v, f, H, W = CASES["hand"]
    vt, ft, v, f = (_dev(a, gpu) for a in (vt, ft, v, f))
    fid = _texture.raster_uv_faces(vt, ft, H, W)
    xyz = _texture.raster_uv_interp(vt, ft, v, f, fid, H, W)
    assert torch.equal(xyz, _raster("hand", gpu)[1])
    with pytest.raises(RuntimeError, match="out of range"):
        _texture.raster_uv_faces(vt, ft + 1, H, W)
    with pytest.raises(RuntimeError, match="out of range"):
        _texture.raster_uv_interp(vt, ft, v, f - 1, fid, H, W)
    with pytest.raises(RuntimeError, match="2\\^31"):
        _texture.raster_uv_faces(vt, ft, 1 << 16, 1 << 15)


def _dilate_inputs(kind):
    rng = np.random.default_rng(5)
    H, W = 37, 53
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "random":
        mask = (rng.uniform(size=(H, W)) < 0.08).astype(np.uint8)
    elif kind == "full":
        mask = np.ones((H, W), np.uint8)
    else:
        mask = np.zeros((H, W), np.uint8)
    return rgb, mask


@pytest.mark.parametrize("kind,k", [("random", 0), ("random", 1), ("random", 3), ("full", 3),
                                    ("none", 3)])
def test_dilation_is_the_oracle_bit_for_bit(gpu, kind, k):
    import _texture
    rgb, mask = _dilate_inputs(kind)
    want_rgb, want_mask = dilate_ref(rgb, mask, k)
    src_rgb, src_mask = _dev(rgb, gpu), _dev(mask, gpu)
    out_rgb, out_mask = _texture.texture_dilate(src_rgb, src_mask, k)
    assert np.array_equal(out_rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(out_mask.cpu().numpy(), want_mask)
    # the inputs are left alone
    assert np.array_equal(src_rgb.cpu().numpy(), rgb)
    assert np.array_equal(src_mask.cpu().numpy(), mask)
    if kind == "random" and k == 3:
        assert want_mask.sum() > 4 * mask.sum()


def test_two_runs_are_bit_identical(gpu):
    import _texture

    def run():
        out = []
        for name in ("atlas5000_512", "overlap"):
            fid, xyz, bary = _raster(name, gpu)
            H, W = CASES[name][4:]
            rgb = (xyz.view(H, W, 3).abs() * 255).to(torch.uint8)
            mask = (fid.view(H, W) >= 0).to(torch.uint8)
            out += [fid, xyz, bary, *_texture.texture_dilate(rgb, mask, 3)]
        return out

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def trained(gpu):
    """A trainer after 17 native steps, as tests/test_mesh.py's export test."""
    import bench
    trainer, data = bench.make_trainer(64, 3, 0, 1, True, graph=True)
    with torch.no_grad():
        trainer.model.encoder.embeddings.uniform_(-0.5, 0.5)
    for i in range(17):
        trainer.train_iteration(data.collate([i % 4]))
    trainer.log_ptr = None
    return trainer


def _parse_obj(path):
    v, t, f = [], [], []
    for line in open(path):
        tok = line.split()
        if tok and tok[0] == "v":
            v.append([float(a) for a in tok[1:]])
        elif tok and tok[0] == "vt":
            t.append([float(a) for a in tok[1:]])
        elif tok and tok[0] == "f":
            f.append([[int(i) - 1 for i in a.split("/")] for a in tok[1:]])
    return np.array(v), np.array(t), np.array(f)


def test_textured_export_end_to_end(gpu, trained, tmp_path):
    from PIL import Image
    model = trained.model
    trained.workspace = str(tmp_path)
    trained.save_mesh(resolution=32, texture_size=None)
    out = tmp_path / "mesh"
    assert sorted(p.name for p in out.iterdir()) == ["albedo.png", "mesh.mtl", "mesh.obj"]
    v0, f0 = model.export_mesh(str(tmp_path / "plain"), resolution=32, texture_size=0)
    verts, faces = model.export_mesh(str(tmp_path / "tex"), resolution=32, texture_size=None)
    assert len(faces) > 0
    assert np.array_equal(verts, v0) and np.array_equal(faces, f0)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["mesh.obj"]
    assert (tmp_path / "tex" / "mesh.obj").read_bytes() == (out / "mesh.obj").read_bytes()

    vt, ft, H, W = grid_atlas(len(faces))
    with Image.open(tmp_path / "tex" / "albedo.png") as im:
        assert im.size == (W, H) and im.mode == "RGB"
        png = np.array(im)
    v, t, f = _parse_obj(tmp_path / "tex" / "mesh.obj")
    assert len(v) == len(verts) and len(t) == 3 * len(faces) and f.shape == (len(faces), 3, 2)
    assert np.array_equal(f[..., 0], faces)
    assert np.array_equal(f[..., 1], np.arange(3 * len(faces)).reshape(-1, 3))
    assert "map_Kd albedo.png" in (tmp_path / "tex" / "mesh.mtl").read_text()

    # the bake from the pipeline's own points: the same rows through the same
    # kernel, so the quantised colours are equal, not close
    face_id, xyz, mask = rasterize_uv(vt, ft, verts, faces, H, W)
    image, mask0 = bake_texture(model, xyz, mask, dilate=3)
    assert torch.equal(mask0, mask) and int(mask.sum()) >= 3 * len(faces)
    assert len(torch.unique(face_id[mask])) == len(faces)
    pts = xyz[mask]
    assert float(pts.abs().max()) <= 1.0 + 1e-6
    with torch.no_grad():
        cols = [model.density(pts[h:h + BAKE_CHUNK].contiguous())["albedo"].float()
                for h in range(0, len(pts), BAKE_CHUNK)]
    want = torch.floor(torch.cat(cols).clamp(0, 1) * 255).to(torch.uint8)
    assert torch.equal(image[mask], want)
    assert len(torch.unique(want)) > 8  # a trained field, not a constant
    image = image.cpu().numpy()
    assert np.array_equal(image, png)

    # dilation: covered texels keep their colour (checked above through
    # image[mask]); everything within Chebyshev distance 1 of the mask is filled
    # from a covered neighbour, which three steps can only extend
    undilated, _ = bake_texture(model, xyz, mask, dilate=0)
    undilated = undilated.cpu().numpy()
    m = mask.cpu().numpy()
    assert np.array_equal(undilated[m], image[m]) and not undilated[~m].any()
    ring_rgb, ring_mask = dilate_ref_fast(undilated, m)
    ring = ring_mask & ~m
    assert ring.any() and np.array_equal(image[ring], ring_rgb[ring])
    import _texture
    again, dilated = _texture.texture_dilate(_dev(undilated, gpu), mask.to(torch.uint8), 3)
    assert np.array_equal(again.cpu().numpy(), image)
    assert dilated.cpu().numpy().astype(bool)[ring_mask].all()


def dilate_ref_fast(rgb, mask):
    """One step of dilate_ref on a large image (vectorised; the neighbour order
    is applied backwards so the first in order is written last)."""
    from test_mesh_texture_host import NEIGHBOURS
    H, W = mask.shape
    out_rgb, out_mask = rgb.copy(), mask.copy()
    pm = np.pad(mask, 1)
    prgb = np.pad(rgb, ((1, 1), (1, 1), (0, 0)))
    for dr, dc in reversed(NEIGHBOURS):
        nm = pm[1 + dr:1 + dr + H, 1 + dc:1 + dc + W]
        take = nm & ~mask
        out_rgb[take] = prgb[1 + dr:1 + dr + H, 1 + dc:1 + dc + W][take]
        out_mask |= take
    return out_rgb, out_mask


def test_dilate_ref_fast_is_dilate_ref():
    rgb, mask = _dilate_inputs("random")
    a, am = dilate_ref_fast(rgb, mask.astype(bool))
    b, bm = dilate_ref(rgb, mask, 1)
    assert np.array_equal(a, b) and np.array_equal(am, bm.astype(bool))


def test_textured_export_of_an_empty_field(gpu, trained, tmp_path):
    """Nothing above the threshold: the export writes an OBJ without faces and
    a 1 x 1 black PNG and raises no launch error."""
    from PIL import Image
    model = trained.model
    saved = model.mean_density, model.density_thresh
    try:
        model.mean_density = model.density_thresh = 1e30
        verts, faces = model.export_mesh(str(tmp_path), resolution=32, texture_size=None)
    finally:
        model.mean_density, model.density_thresh = saved
    torch.cuda.synchronize()
    assert len(verts) == 0 and len(faces) == 0
    text = (tmp_path / "mesh.obj").read_text().splitlines()
    assert not [t for t in text if t.split()[0] in ("v", "vt", "f")]
    assert (tmp_path / "mesh.mtl").exists()
    with Image.open(tmp_path / "albedo.png") as im:
        assert im.size == (1, 1) and not np.array(im).any()
