"""Texture bake of export_mesh, host side (nerf/mesh.py): the regular atlas
`grid_atlas`, the textured OBJ / MTL / PNG writers, and the f64 numpy oracles
(`raster_ref`, `interp_np`, `dilate_ref`) with the raster cases that
tests/test_gpu_mesh_texture.py runs on the HIP kernels.

Parity with the reference's xatlas charts / nvdiffrast raster is unpinned
(neither library is importable); what is pinned are the properties a baked
atlas needs: faces that do not share or touch texels, coverage decided far
from every edge, and a writer a parser can read back."""
import numpy as np
import pytest

from nerf.mesh import grid_atlas, write_mtl, write_obj, write_obj_textured, write_png

MARGIN = 1.0 / 16  # texels between any texel centre and any edge line (R4)


# ---------------------------------------------------------------- oracles

def raster_ref(vt, ft, H, W, margin=MARGIN, want_count=False):
    """f64 oracle of dfhip_raster_uv_faces: face_id [H, W] int32, the lowest
    face covering each texel centre (u = (c + 0.5) / W, v = (r + 0.5) / H), -1
    where none; a centre is covered when the three edge functions have one
    sign or are zero, zero-area faces cover nothing.

    Asserts that no texel centre of a face's (one texel wider, clipped)
    bounding box is within `margin` texels of the line through any of its
    edges, so no f32 rounding can flip a decision.  With want_count also
    returns how many faces cover each texel."""
    vt = np.asarray(vt, np.float32).astype(np.float64).reshape(-1, 2)
    ft = np.asarray(ft).reshape(-1, 3)
    fid = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    for i in range(len(ft) - 1, -1, -1):  # descending: the lowest id is written last
        p = vt[ft[i]] * np.array([W, H], np.float64)
        d1, d2 = p[1] - p[0], p[2] - p[0]
        area = d1[0] * d2[1] - d1[1] * d2[0]
        if area == 0:
            continue
        x0 = int(max(0, np.floor(p[:, 0].min()) - 1))
        x1 = int(min(W, np.ceil(p[:, 0].max()) + 1))
        y0 = int(max(0, np.floor(p[:, 1].min()) - 1))
        y1 = int(min(H, np.ceil(p[:, 1].max()) + 1))
        if x1 <= x0 or y1 <= y0:
            continue
        qx = (np.arange(x0, x1) + 0.5 - p[0, 0])[None, :]
        qy = (np.arange(y0, y1) + 0.5 - p[0, 1])[:, None]
        e2 = d1[0] * qy - d1[1] * qx
        e1 = qx * d2[1] - qy * d2[0]
        e0 = area - e1 - e2
        for e, edge in ((e0, d2 - d1), (e1, d2), (e2, d1)):
            dist = np.abs(e).min() / np.hypot(*edge)
            assert dist >= margin, f"face {i}: a texel centre {dist} texels from an edge line"
        cov = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        fid[y0:y1, x0:x1][cov] = i
        count[y0:y1, x0:x1] += cov
    return (fid, count) if want_count else fid


def interp_np(vt, ft, v, f, face_id, H, W, dtype=np.float64):
    """dfhip_raster_uv_interp restated in numpy with every operation in
    `dtype`, in the kernel's order: float64 is the oracle, float32 the
    restatement whose distance from the oracle sets the GPU tolerance.
    Returns (xyz [H*W, 3], bary [H*W, 2]) in `dtype`, zeros where face_id < 0."""
    vt = np.asarray(vt, np.float32).reshape(-1, 2).astype(dtype)
    v = np.asarray(v, np.float32).reshape(-1, 3).astype(dtype)
    ft, f = np.asarray(ft).reshape(-1, 3), np.asarray(f).reshape(-1, 3)
    fid = np.asarray(face_id).reshape(-1)
    xyz, bary = np.zeros((H * W, 3), dtype), np.zeros((H * W, 2), dtype)
    t = np.nonzero(fid >= 0)[0]
    if len(t) == 0:
        return xyz, bary
    face = fid[t]
    fw, fh, half, one = dtype(W), dtype(H), dtype(0.5), dtype(1)
    i0, i1, i2 = ft[face].T
    p0x, p0y = vt[i0, 0] * fw, vt[i0, 1] * fh
    d1x, d1y = vt[i1, 0] * fw - p0x, vt[i1, 1] * fh - p0y
    d2x, d2y = vt[i2, 0] * fw - p0x, vt[i2, 1] * fh - p0y
    area = d1x * d2y - d1y * d2x
    qx = ((t % W).astype(dtype) + half) - p0x
    qy = ((t // W).astype(dtype) + half) - p0y
    e2 = d1x * qy - d1y * qx
    e1 = qx * d2y - qy * d2x
    w1, w2 = e1 / area, e2 / area
    w0 = (one - w1) - w2
    a, b, c = (v[j] for j in f[face].T)
    out = (w0[:, None] * a + w1[:, None] * b) + w2[:, None] * c
    assert out.dtype == dtype and w1.dtype == dtype
    xyz[t] = out
    bary[t] = np.stack([w1, w2], 1)
    return xyz, bary


NEIGHBOURS = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))  # N W E S ...


def dilate_ref(rgb, mask, k):
    """k steps of dfhip_texture_dilate: an uncovered texel takes the colour of
    its first covered neighbour in the order N, W, E, S, NW, NE, SW, SE and
    becomes covered (mask 1); every other texel is copied."""
    rgb, mask = np.array(rgb, np.uint8), np.array(mask, np.uint8)
    H, W = mask.shape
    for _ in range(k):
        out_rgb, out_mask = rgb.copy(), mask.copy()
        for r in range(H):
            for c in range(W):
                if mask[r, c]:
                    continue
                for dr, dc in NEIGHBOURS:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < H and 0 <= cc < W and mask[rr, cc]:
                        out_rgb[r, c], out_mask[r, c] = rgb[rr, cc], 1
                        break
        rgb, mask = out_rgb, out_mask
    return rgb, mask


# ---------------------------------------------------------------- raster cases

def _texels(points, H, W):
    """vt from (x, y) = (col, row) texel coordinates."""
    return (np.asarray(points, np.float64).reshape(-1, 2) / [W, H]).astype(np.float32)


def _tri_faces(n):
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def raster_cases():
    """name -> (vt, ft, v, f, H, W): the inputs of the GPU raster / interp
    tests.  Positions v are random in [-1, 1]^3 and f indexes them in another
    order than ft indexes vt, so swapping the two tables cannot pass."""
    cases = {}

    def add(name, vt, ft, H, W):
        vt, ft = np.asarray(vt, np.float32).reshape(-1, 2), np.asarray(ft, np.int32).reshape(-1, 3)
        rng = np.random.default_rng(len(cases))
        V = max(len(vt), 1)
        v = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
        f = (V - 1 - ft).astype(np.int32)
        cases[name] = (vt, ft, v, f, H, W)

    # two hand-placed faces of opposite orientation on 8 x 8
    add("hand", _texels([[0.25, 0.25], [4.25, 0.25], [0.25, 4.25],
                         [7.75, 7.75], [7.75, 3.75], [3.75, 7.75]], 8, 8), _tri_faces(2), 8, 8)
    vt, ft, H, W = grid_atlas(61, (64, 48))
    add("atlas61_64x48", vt, ft, H, W)
    vt, ft, H, W = grid_atlas(5000, 512)
    add("atlas5000_512", vt, ft, H, W)
    # overlap: the lowest face id wins; face 2 repeats face 0
    add("overlap", _texels([[0.25, 0.25], [6.25, 0.25], [0.25, 6.25],
                            [1.25, 1.25], [7.25, 1.25], [1.25, 7.25]], 8, 8),
        [[3, 4, 5], [0, 1, 2], [0, 1, 2]], 8, 8)
    # collinear vertices, a repeated vertex, far and near outside, partly outside
    add("degenerate", _texels([[2, 2], [4, 4], [6, 6],
                               [800, 800], [808, 800], [800, 808],
                               [12.25, 12.25], [20.25, 12.25], [12.25, 20.25],
                               [-2.25, -2.25], [4.75, -2.25], [-2.25, 4.75],
                               [5.25, 5.25], [7.5, 5.25], [5.25, 7.5]], 8, 8),
        [[0, 1, 2], [12, 12, 13], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14]], 8, 8)
    # vertices exactly on the image border
    add("border", np.array([[0, 0], [1, 0], [0.5, 1]], np.float32), _tri_faces(1), 8, 8)
    add("empty", np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), 8, 8)
    return cases


HAND_EXPECTED = np.array([
    [0, 0, 0, 0, -1, -1, -1, -1],
    [0, 0, 0, -1, -1, -1, -1, -1],
    [0, 0, -1, -1, -1, -1, -1, -1],
    [0, -1, -1, -1, -1, -1, -1, -1],
    [-1, -1, -1, -1, -1, -1, -1, 1],
    [-1, -1, -1, -1, -1, -1, 1, 1],
    [-1, -1, -1, -1, -1, 1, 1, 1],
    [-1, -1, -1, -1, 1, 1, 1, 1]], np.int32)


def interp_f32_error(cases=None):
    """Largest |f32 restatement - f64 oracle| of xyz and of bary over the
    raster cases (the GPU tolerance is 4x these)."""
    ex = eb = 0.0
    for vt, ft, v, f, H, W in (cases or raster_cases()).values():
        fid = raster_ref(vt, ft, H, W)
        x64, b64 = interp_np(vt, ft, v, f, fid, H, W, np.float64)
        x32, b32 = interp_np(vt, ft, v, f, fid, H, W, np.float32)
        ex = max(ex, float(np.abs(x32.astype(np.float64) - x64).max()))
        eb = max(eb, float(np.abs(b32.astype(np.float64) - b64).max()))
    return ex, eb


# ---------------------------------------------------------------- oracle self-checks

def test_oracle_on_the_hand_case_and_the_special_faces():
    cases = raster_cases()
    vt, ft, _, _, H, W = cases["hand"]
    assert np.array_equal(raster_ref(vt, ft, H, W), HAND_EXPECTED)
    vt, ft, _, _, H, W = cases["overlap"]
    fid = raster_ref(vt, ft, H, W)
    assert fid[0, 0] == 1 and fid[1, 1] == 0 and fid[6, 1] == 0 and not (fid == 2).any()
    vt, ft, _, _, H, W = cases["degenerate"]
    fid = raster_ref(vt, ft, H, W)
    assert set(np.unique(fid)) == {-1, 4, 5} and fid[0, 0] == 4 and fid[0, 2] == -1
    vt, ft, _, _, H, W = cases["border"]
    fid = raster_ref(vt, ft, H, W)
    assert fid[0, 0] == 0 and fid[0, 7] == 0 and fid[6, 3] == 0 and fid[7, 0] == -1
    vt, ft, _, _, H, W = cases["empty"]
    assert (raster_ref(vt, ft, H, W) == -1).all()


def test_oracle_refuses_an_edge_through_a_texel_centre():
    vt = _texels([[0, 0], [8, 0], [0, 8]], 8, 8)  # hypotenuse through the centres r + c = 7
    with pytest.raises(AssertionError, match="edge line"):
        raster_ref(vt, _tri_faces(1), 8, 8)


def test_interp_oracle_reproduces_the_vertices_plane():
    """The interpolated position is the affine map of the texel centre that
    takes the UV triangle to the 3D triangle; bary sums with w0 to 1."""
    vt, ft, v, f, H, W = raster_cases()["hand"]
    fid = raster_ref(vt, ft, H, W)
    xyz, bary = interp_np(vt, ft, v, f, fid, H, W)
    for r, c in ((0, 0), (1, 2), (7, 7), (5, 6)):
        face = fid[r, c]
        uv = np.array([(c + 0.5) / W, (r + 0.5) / H])
        tri = vt[ft[face]].astype(np.float64)
        A = np.stack([tri[1] - tri[0], tri[2] - tri[0]], 1)
        w1, w2 = np.linalg.solve(A, uv - tri[0])
        np.testing.assert_allclose(bary[r * W + c], [w1, w2], atol=1e-12)
        p = v[f[face]].astype(np.float64)
        np.testing.assert_allclose(xyz[r * W + c], (1 - w1 - w2) * p[0] + w1 * p[1] + w2 * p[2],
                                   atol=1e-12)
    assert not xyz[fid.reshape(-1) < 0].any()


def test_interp_f32_error_is_the_documented_one():
    """The f32 restatement is within 1.0e-6 (xyz) and 5.0e-7 (bary) of the f64
    oracle on the raster cases (measured 3.553e-07 and 1.788e-07): the figures the
    GPU test's 4x tolerance and DESIGN.md quote."""
    ex, eb = interp_f32_error()
    print(f"f32 restatement vs f64 oracle: xyz {ex:.3e}, bary {eb:.3e}")
    assert 0 < ex <= 1.0e-6 and 0 < eb <= 5.0e-7


def test_dilate_ref_by_hand():
    rgb = np.zeros((3, 4, 3), np.uint8)
    mask = np.zeros((3, 4), np.uint8)
    rgb[1, 1], mask[1, 1] = (10, 20, 30), 1
    rgb[1, 3], mask[1, 3] = (40, 50, 60), 1
    out, m = dilate_ref(rgb, mask, 1)
    assert m.all()
    # (1, 2): W neighbour (1, 1) comes before E neighbour (1, 3)
    assert tuple(out[1, 2]) == (10, 20, 30)
    # (0, 2): no N / W / E / S neighbour covered; SW (1, 1) comes before SE (1, 3)
    assert tuple(out[0, 2]) == (10, 20, 30)
    assert tuple(out[2, 3]) == (40, 50, 60) and tuple(out[0, 0]) == (10, 20, 30)
    same, m0 = dilate_ref(rgb, mask, 0)
    assert np.array_equal(same, rgb) and np.array_equal(m0, mask)


# ---------------------------------------------------------------- grid_atlas

ATLAS_CASES = [(1, None), (2, None), (3, None), (61, None), (5000, None), (61, 64), (61, (64, 48)),
               (5000, 512), (1, 6), (2, 5)]


@pytest.mark.parametrize("F,size", ATLAS_CASES)
def test_grid_atlas_properties(F, size):
    kw = {"min_cell": 5} if size == 5 else {}
    vt, ft, H, W = grid_atlas(F, size, **kw)
    assert vt.dtype == np.float32 and vt.shape == (3 * F, 2)
    assert ft.dtype == np.int32 and np.array_equal(ft, np.arange(3 * F).reshape(F, 3))
    if size is None:
        assert H == W == 2048
    else:
        assert (H, W) == ((size, size) if np.isscalar(size) else tuple(size))
    # R1
    assert vt.min() >= 0 and vt.max() <= 1
    # R4 is asserted inside the oracle for every texel of each face's cell
    fid, count = raster_ref(vt, ft, H, W, want_count=True)
    # R2
    covered = np.bincount(fid[fid >= 0], minlength=F)
    assert covered.min() >= 3
    # both triangles of a cell have the same number of texels
    assert len(np.unique(covered)) == 1
    # R3: no texel in two faces, and the 3 x 3 neighbourhood of a covered texel
    # holds that face or nothing, so two faces are >= 2 texels apart
    assert count.max() == 1
    pad = np.pad(fid, 1, constant_values=-1)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            nb = pad[dr:dr + H, dc:dc + W]
            assert np.all((fid < 0) | (nb < 0) | (nb == fid))
    # R5
    p = vt.astype(np.float64).reshape(F, 3, 2) * [W, H]
    d1, d2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    area = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    assert np.all(area > 0)
    assert np.allclose(area, area[0])


def test_grid_atlas_layout_and_auto_size():
    # two consecutive faces share a cell, cells run row-major
    vt, ft, H, W = grid_atlas(61, 64)
    s = 10  # 64 // 10 = 6 columns and rows: 36 >= 31 cells; s = 11 gives 25
    cell = np.floor(vt.reshape(61, 3, 2) * [W, H] / s).astype(int)
    assert np.all(cell == cell[:, :1])
    k = np.arange(61) // 2
    assert np.array_equal(cell[:, 0, 0], k % 6) and np.array_equal(cell[:, 0, 1], k // 6)
    # odd F: the second half of the last cell stays empty
    fid = raster_ref(vt, ft, H, W)
    last = fid[5 * s:6 * s, 0:s]
    assert set(np.unique(last)) == {-1, 60}
    full = fid[0:s, 0:s]
    assert set(np.unique(full)) == {-1, 0, 1}
    assert (last >= 0).sum() * 2 == (full >= 0).sum()
    # automatic size: 2048 until the cells fall below min_cell, then 4096
    assert grid_atlas(100000)[2:] == (2048, 2048)   # 227^2 cells of 9 texels
    assert grid_atlas(232562)[2:] == (2048, 2048)   # 341^2 = 116281 cells of 6 texels
    assert grid_atlas(232563)[2:] == (4096, 4096)
    assert grid_atlas(600000)[2:] == (4096, 4096)
    assert grid_atlas(0)[0].shape == (0, 2)


def test_grid_atlas_size_errors():
    with pytest.raises(ValueError, match="resolution.*texture size"):
        grid_atlas(61, 32)  # 31 cells of 6 texels need 36 texels a side
    with pytest.raises(ValueError, match="resolution.*texture size"):
        grid_atlas(232563, 2048)
    with pytest.raises(ValueError, match="resolution.*texture size"):
        grid_atlas(232563, max_size=2048)
    with pytest.raises(ValueError, match="resolution.*texture size"):
        grid_atlas(4_000_000)  # 1415^2 cells of 6 texels exceed 8192
    with pytest.raises(ValueError):
        grid_atlas(10, 16384)
    with pytest.raises(ValueError):
        grid_atlas(10, min_cell=4)


# ---------------------------------------------------------------- C entries

def test_texture_entries_validate_sizes_without_a_gpu():
    """H W < 2^31, F < 2^31, null and aliased buffers: the library's error
    codes, before any device work."""
    import _dfhip
    lib = _dfhip.load()
    assert lib.dfhip_raster_uv_faces(None, None, 0, 0, 1 << 16, 1 << 15, None, None) == 1
    assert b"2^31" in lib.dfhip_last_error()
    assert lib.dfhip_raster_uv_faces(None, None, 1 << 31, 1, 8, 8, None, None) == 1
    assert b"F must be below 2^31" in lib.dfhip_last_error()
    assert lib.dfhip_raster_uv_faces(None, None, 0, 0, 8, 8, None, None) == 1
    assert b"null pointer" in lib.dfhip_last_error()
    assert lib.dfhip_raster_uv_interp(None, None, None, None, None, 0, 0, 0, 0, 8, None, None,
                                      None) == 1
    assert b"H*W" in lib.dfhip_last_error()
    assert lib.dfhip_raster_uv_interp(None, None, None, None, None, 1 << 31, 0, 0, 8, 8, None,
                                      None, None) == 1
    assert lib.dfhip_texture_dilate(None, None, 8, 8, None, None, None) == 1
    assert lib.dfhip_texture_dilate(16, 32, 8, 8, 16, 48, None) == 1
    assert b"different buffers" in lib.dfhip_last_error()
    assert lib.dfhip_texture_dilate(16, 32, 1 << 16, 1 << 16, 48, 64, None) == 1


# ---------------------------------------------------------------- writers

def _tetrahedron():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * 0.5 - 0.1
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return verts, faces


def test_textured_obj_mtl_round_trip(tmp_path):
    verts, faces = _tetrahedron()
    vt, ft, H, W = grid_atlas(len(faces), 64)
    write_obj_textured(tmp_path / "xmesh.obj", verts, faces, vt, ft, "xmesh.mtl")
    write_mtl(tmp_path / "xmesh.mtl", "xalbedo.png")
    v, t, f, other = [], [], [], []
    for line in open(tmp_path / "xmesh.obj"):
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        if tok[0] == "v":
            v.append([float(a) for a in tok[1:]])
        elif tok[0] == "vt":
            t.append([float(a) for a in tok[1:]])
        elif tok[0] == "f":
            f.append([[int(i) - 1 for i in a.split("/")] for a in tok[1:]])
        else:
            other.append(tok)
    v, t, f = np.array(v), np.array(t), np.array(f)
    assert other == [["mtllib", "xmesh.mtl"], ["usemtl", "mat0"]]
    np.testing.assert_allclose(v, verts, rtol=1e-6, atol=1e-9)
    assert f.shape == (4, 3, 2)
    assert np.array_equal(f[..., 0], faces) and np.array_equal(f[..., 1], ft)
    assert f[..., 0].min() >= 0 and f[..., 0].max() < len(v)
    assert f[..., 1].min() >= 0 and f[..., 1].max() < len(t) == 3 * len(faces)
    # the flip: image row 0 is the top, OBJ v = 0 the bottom
    np.testing.assert_allclose(t[:, 0], vt[:, 0], rtol=1e-6)
    np.testing.assert_allclose(t[:, 1], 1 - vt[:, 1].astype(np.float64), rtol=1e-6)
    assert t[0, 1] > 0.9 > 0.1 > vt[0, 1]
    mtl = [line.split() for line in open(tmp_path / "xmesh.mtl") if not line.startswith("#")]
    assert mtl[0] == ["newmtl", "mat0"] and ["map_Kd", "xalbedo.png"] in mtl
    assert {m[0] for m in mtl} == {"newmtl", "Ka", "Kd", "Ks", "Tr", "illum", "Ns", "map_Kd"}


def test_png_round_trip_is_exact(tmp_path):
    from PIL import Image
    img = np.random.default_rng(0).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    write_png(tmp_path / "a.png", img)
    with Image.open(tmp_path / "a.png") as im:
        assert im.mode == "RGB" and im.size == (53, 37)  # (width, height)
        back = np.array(im)
    assert np.array_equal(back, img)  # row r = texel row r, RGB order


def test_vertex_colour_obj_is_unchanged(tmp_path):
    """texture_size = 0 goes through write_obj, whose output is today's text."""
    verts, faces = _tetrahedron()
    cols = np.linspace(0, 1, 12).reshape(4, 3)
    write_obj(tmp_path / "m.obj", verts, faces, cols)
    want = "# single-stable-dreamfusion_amd export_mesh (marching tetrahedra)\n"
    for (a, b, c), (r, g, bb) in zip(verts, cols):
        want += f"v {a} {b} {c} {r:.4f} {g:.4f} {bb:.4f}\n"
    for a, b, c in faces:
        want += f"f {a + 1} {b + 1} {c + 1}\n"
    assert (tmp_path / "m.obj").read_bytes() == want.encode()


def test_main_flag_maps_to_texture_size():
    """--mesh_texture_size: 0 (default) keeps the vertex colours, -1 is the
    automatic size, N a fixed one; the export methods default to 0."""
    import inspect
    import main
    from nerf.renderer import NeRFRenderer
    from nerf.utils import Trainer
    def size(*flags):
        return main.mesh_texture_size(main.parse_opt(["--text", "x", *flags]))

    assert size() == 0
    assert size("--mesh_texture_size", "-1") is None
    assert size("--mesh_texture_size", "4096") == 4096
    for fn in (NeRFRenderer.export_mesh, Trainer.save_mesh):
        assert inspect.signature(fn).parameters["texture_size"].default == 0


class _SphereModel:
    """export_mesh's view of a model: density() on the host (no kernel), a
    ball of radius 0.5 with a position-coloured albedo."""
    grid_size = 16
    mean_density = 1.0
    density_thresh = 10.0

    def __init__(self):
        import torch
        self.density_bitfield = torch.zeros(1, dtype=torch.uint8)

    def density(self, x):
        return {"sigma": (0.5 - x.norm(dim=-1)) * 10 + 1.0, "albedo": x * 0.5 + 0.5}


def test_export_mesh_texture_size_zero_is_todays_file(tmp_path):
    from nerf.mesh import export_mesh
    model = _SphereModel()
    verts, faces = export_mesh(model, str(tmp_path / "a"), resolution=16)
    v0, f0 = export_mesh(model, str(tmp_path / "b"), resolution=16, texture_size=0)
    assert np.array_equal(verts, v0) and np.array_equal(faces, f0) and len(faces) > 100
    import torch
    cols = np.clip(model.density(torch.from_numpy(verts))["albedo"].numpy(), 0, 1)
    want = "# single-stable-dreamfusion_amd export_mesh (marching tetrahedra)\n"
    for (a, b, c), (r, g, bb) in zip(verts, cols):
        want += f"v {a} {b} {c} {r:.4f} {g:.4f} {bb:.4f}\n"
    for a, b, c in faces:
        want += f"f {a + 1} {b + 1} {c + 1}\n"
    for d in "ab":
        assert (tmp_path / d / "mesh.obj").read_bytes() == want.encode()
        assert sorted(p.name for p in (tmp_path / d).iterdir()) == ["mesh.obj"]


def test_export_mesh_empty_isosurface_with_a_texture(tmp_path):
    """Nothing above the threshold: an OBJ without faces, the MTL and a 1 x 1
    black PNG, with no kernel launched (this runs without a GPU)."""
    from PIL import Image
    from nerf.mesh import export_mesh
    model = _SphereModel()
    model.mean_density = model.density_thresh = 1e9
    verts, faces = export_mesh(model, str(tmp_path), resolution=16, name="e_", texture_size=None)
    assert len(verts) == 0 and len(faces) == 0
    text = (tmp_path / "e_mesh.obj").read_text().splitlines()
    assert [t for t in text if not t.startswith("#")] == ["mtllib e_mesh.mtl", "usemtl mat0"]
    assert "map_Kd e_albedo.png" in (tmp_path / "e_mesh.mtl").read_text()
    with Image.open(tmp_path / "e_albedo.png") as im:
        assert im.size == (1, 1) and np.array_equal(np.array(im), np.zeros((1, 1, 3), np.uint8))
