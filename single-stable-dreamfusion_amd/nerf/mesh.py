"""Mesh export of the density field (reference nerf/renderer.py:121-299
`export_mesh`, nerf/utils.py:459-470 `save_mesh`).

The reference queries sigma on a resolution^3 lattice over [-1, 1]^3, runs
PyMCubes' marching cubes at min(mean_density, density_thresh), then unwraps
UVs with xatlas and bakes an albedo texture with nvdiffrast.  None of those
three libraries exists on this platform, so:

* the isosurface is extracted by marching tetrahedra (`isosurface`): every
  lattice cube is split into the six Kuhn tetrahedra around its 0-7
  diagonal (the same split in every cube, so neighbouring cubes share faces
  and the mesh is watertight), each tetrahedron contributes 0, 1 or 2
  triangles with vertices interpolated linearly on its edges at the
  threshold, and vertices on the same lattice edge are shared.  Triangles
  are oriented with the density decreasing along the normal (outward).
  The surface is the same level set marching cubes approximates; the
  triangulation differs (more, smaller triangles);
* with `texture_size=0` (the default) the albedo is queried at the vertices
  and written as OBJ vertex colours (`v x y z r g b`);
* with a texture size the albedo is baked into `albedo.png` as the reference
  does, without xatlas / nvdiffrast / cv2 / sklearn: `grid_atlas` gives every
  face its own right-angled triangle of a regular grid of cells (the
  marching-tetrahedra faces are near-uniform in size, so no chart solver is
  needed), the HIP rasteriser of csrc/texture.hip finds the face and position
  of every texel centre, `model.density` gives the albedo there, and a
  3x3 dilation pads the seams (the reference fills them from a kd-tree
  nearest neighbour).  See DESIGN.md "Texture bake".

Vertices are mapped to [-1, 1] exactly as the reference does
(`v / (resolution - 1) * 2 - 1`, renderer.py:149)."""
import os

import numpy as np
import torch

# the six tetrahedra of a cube, corner c = dx + 2 dy + 4 dz, all sharing the
# 0-7 diagonal (paths 0 -> 7 along the axes in each of the 3! orders)
TETS = np.array([[0, 1, 3, 7], [0, 2, 3, 7], [0, 2, 6, 7],
                 [0, 4, 6, 7], [0, 4, 5, 7], [0, 1, 5, 7]], np.int64)
CORNERS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)


def isosurface(values, thresh):
    """Marching tetrahedra of the level set values == thresh on a lattice.

    values: [X, Y, Z] float array (lattice point (i, j, k) at index space
    position (i, j, k)).  Returns (vertices [V, 3] float64 in index space,
    faces [F, 3] int64), faces oriented with `values` decreasing along the
    normal.  "Inside" is values > thresh."""
    v = np.asarray(values, np.float64)
    X, Y, Z = v.shape
    if min(X, Y, Z) < 2:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    inside = v > thresh
    # active cubes: corners not all on one side
    cnt = np.zeros((X - 1, Y - 1, Z - 1), np.int8)
    for dx, dy, dz in CORNERS:
        cnt += inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]
    cubes = np.argwhere((cnt > 0) & (cnt < 8))  # [C, 3]
    if len(cubes) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    # lattice points of the tetrahedra: [C, 6, 4, 3]
    pts = cubes[:, None, None, :] + CORNERS[TETS][None]
    pts = pts.reshape(-1, 4, 3)
    flat = (pts[..., 0] * Y + pts[..., 1]) * Z + pts[..., 2]  # [T, 4] lattice ids
    val = v.reshape(-1)[flat]
    ins = val > thresh
    n_in = ins.sum(1)
    keep = (n_in > 0) & (n_in < 4)
    flat, val, ins, n_in, pts = flat[keep], val[keep], ins[keep], n_in[keep], pts[keep]
    # order each tetrahedron's corners: inside ones first (stable)
    order = np.argsort(~ins, axis=1, kind="stable")
    flat = np.take_along_axis(flat, order, 1)
    val = np.take_along_axis(val, order, 1)
    pts = np.take_along_axis(pts, order[..., None], 1)

    edges_a, edges_b, tri_tet = [], [], []

    def emit(sel, pairs):
        # one triangle per selected tetrahedron over three (inside, outside) edges
        t = np.nonzero(sel)[0]
        if len(t) == 0:
            return
        a = np.stack([flat[t, p] for p, _ in pairs], 1)
        b = np.stack([flat[t, q] for _, q in pairs], 1)
        edges_a.append(a)
        edges_b.append(b)
        tri_tet.append(t)

    # one inside corner (0): edges 0-1, 0-2, 0-3
    emit(n_in == 1, [(0, 1), (0, 2), (0, 3)])
    # three inside (0, 1, 2), one outside (3): edges 0-3, 1-3, 2-3
    emit(n_in == 3, [(0, 3), (1, 3), (2, 3)])
    # two inside (0, 1), two outside (2, 3): quad 0-2, 0-3, 1-3, 1-2
    emit(n_in == 2, [(0, 2), (0, 3), (1, 3)])
    emit(n_in == 2, [(0, 2), (1, 3), (1, 2)])
    if not edges_a:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    ea = np.concatenate(edges_a)  # [F, 3] inside lattice ids
    eb = np.concatenate(edges_b)  # [F, 3] outside lattice ids
    # shared vertices: one per lattice edge
    npts = X * Y * Z
    key = ea.astype(np.int64) * npts + eb.astype(np.int64)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    ia, ib = uniq // npts, uniq % npts
    va, vb = v.reshape(-1)[ia], v.reshape(-1)[ib]
    t = (thresh - va) / (vb - va)  # va > thresh >= vb

    def coords(idx):
        return np.stack([idx // (Y * Z), (idx // Z) % Y, idx % Z], 1).astype(np.float64)

    verts = coords(ia) + t[:, None] * (coords(ib) - coords(ia))
    faces = inv.reshape(-1, 3).astype(np.int64)
    # orientation: the normal points from the inside corners to the outside
    # ones (the density decreases along it)
    p = verts[faces]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    out_dir = coords(eb.reshape(-1)).reshape(-1, 3, 3).mean(1) - \
        coords(ea.reshape(-1)).reshape(-1, 3, 3).mean(1)
    flip = (nrm * out_dir).sum(1) < 0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    # drop degenerate triangles (two vertices on one lattice point)
    good = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & \
        (faces[:, 0] != faces[:, 2])
    return verts, faces[good]


def query_lattice(density_fn, resolution, S, device):
    """sigma on the resolution^3 lattice over [-1, 1]^3 in S^3 chunks
    (renderer.py:130-143), [x, y, z] order."""
    from .utils import custom_meshgrid
    sig = np.zeros([resolution] * 3, np.float32)
    axes = torch.linspace(-1, 1, resolution).split(S)
    for xi, xs in enumerate(axes):
        for yi, ys in enumerate(axes):
            for zi, zs in enumerate(axes):
                xx, yy, zz = custom_meshgrid(xs, ys, zs)
                pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
                val = density_fn(pts.to(device).contiguous())["sigma"]
                sig[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys),
                    zi * S: zi * S + len(zs)] = \
                    val.reshape(len(xs), len(ys), len(zs)).float().cpu().numpy()
    return sig


def write_obj(path, vertices, faces, colors=None):
    """Wavefront OBJ; per-vertex colours as `v x y z r g b` when given."""
    with open(path, "w") as fp:
        fp.write("# single-stable-dreamfusion_amd export_mesh (marching tetrahedra)\n")
        if colors is None:
            fp.writelines(f"v {a} {b} {c}\n" for a, b, c in vertices)
        else:
            fp.writelines(f"v {a} {b} {c} {r:.4f} {g:.4f} {bb:.4f}\n"
                          for (a, b, c), (r, g, bb) in zip(vertices, colors))
        fp.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in faces)


# ---------------------------------------------------------------- texture bake

BAKE_CHUNK = 640000  # renderer.py:214 batch of the albedo query


def _atlas_cell(ncells, H, W):
    """Largest integer cell side s with (W // s) * (H // s) >= ncells (0 when
    even s = 1 does not fit); the product does not grow with s."""
    lo, hi = 0, min(H, W)
    while lo < hi:
        s = (lo + hi + 1) // 2
        if (W // s) * (H // s) >= ncells:
            lo = s
        else:
            hi = s - 1
    return lo


def grid_atlas(num_faces, size=None, min_cell=6, max_size=8192):
    """A regular UV atlas: every face gets its own right-angled triangle.

    The H x W texture (`size`: None = automatic, an int for a square, or
    (H, W)) is cut into square cells of s texels, laid out row-major; cell k
    holds faces 2k and 2k + 1.  Texel (row r, col c) has its centre at
    u = (c + 0.5) / W, v = (r + 0.5) / H.  With n = s - 3 and (x, y) = (col,
    row) texel coordinates relative to the cell's corner:

      face 2k     (0.25, 0.25), (0.25 + n, 0.25), (0.25, 0.25 + n)
                  covers the texels i, j >= 0, i + j <= n - 1
      face 2k + 1 (b, b), (b - n, b), (b, b - n) with b = s - 1.25
                  covers the texels i, j <= n + 1, i + j >= n + 3

    so both cover n (n + 1) / 2 texel centres, every centre is at least 1/4
    texel from the lines through the legs and 0.35 texel from the
    hypotenuses, the two triangles of a cell and those of neighbouring cells
    are 2 texels apart (Chebyshev), and both have the same orientation.

    The automatic size is the smallest power of two >= 2048 whose cells are at
    least `min_cell` texels.  Returns (vt [3 F, 2] float32 in [0, 1],
    ft [F, 3] int32 = [3 i, 3 i + 1, 3 i + 2], H, W)."""
    F = int(num_faces)
    if F < 0:
        raise ValueError("grid_atlas: num_faces must be >= 0")
    if min_cell < 5:
        raise ValueError("grid_atlas: min_cell must be >= 5 (3 texel centres per face)")
    ncells = max(1, (F + 1) // 2)
    trade = ("lower the mesh resolution or raise the texture size "
             f"({F} faces need cells of >= {min_cell} texels)")
    if size is None:
        H = W = 2048
        while _atlas_cell(ncells, H, W) < min_cell:
            H = W = 2 * H
            if H > max_size:
                raise ValueError(f"grid_atlas: no texture up to {max_size}^2 fits; {trade}")
    else:
        H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        if H <= 0 or W <= 0 or max(H, W) > max_size:
            raise ValueError(f"grid_atlas: texture size {H} x {W} outside [1, {max_size}]; {trade}")
        if _atlas_cell(ncells, H, W) < min_cell:
            raise ValueError(f"grid_atlas: a {H} x {W} texture is too small; {trade}")
    s = _atlas_cell(ncells, H, W)
    n, b = s - 3, s - 1.25
    cols = W // s
    cell = np.arange(F, dtype=np.int64) // 2
    origin = np.stack([(cell % cols) * s, (cell // cols) * s], 1).astype(np.float64)  # x, y
    lower = np.array([[0.25, 0.25], [0.25 + n, 0.25], [0.25, 0.25 + n]])
    upper = np.array([[b, b], [b - n, b], [b, b - n]])
    local = np.where((np.arange(F) % 2 == 0)[:, None, None], lower[None], upper[None])
    xy = origin[:, None, :] + local  # [F, 3, 2] texel coordinates
    vt = (xy / np.array([W, H], np.float64)).reshape(-1, 2).astype(np.float32)
    ft = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    return vt, ft, H, W


def rasterize_uv(vt, ft, v, f, H, W):
    """dr.rasterize + dr.interpolate of renderer.py:195-197 in UV space on the
    HIP rasteriser: vt [T, 2] UVs, ft [F, 3], v [V, 3] positions, f [F, 3]
    (arrays or device tensors) -> device tensors face_id [H, W] int32 (-1
    where no face covers the texel centre), xyz [H, W, 3] f32 and
    mask [H, W] bool."""
    import _texture
    dev = torch.device("cuda", torch.cuda.current_device())

    def dev_tensor(a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=dev, dtype=dtype).contiguous()

    vt, v = dev_tensor(vt, torch.float32), dev_tensor(v, torch.float32)
    ft, f = dev_tensor(ft, torch.int32), dev_tensor(f, torch.int32)
    face_id = _texture.raster_uv_faces(vt, ft, H, W)
    xyz = _texture.raster_uv_interp(vt, ft, v, f, face_id, H, W)
    face_id = face_id.view(H, W)
    return face_id, xyz.view(H, W, 3), face_id >= 0


@torch.no_grad()
def query_texels(model, xyz, mask):
    """The albedo of `model.density` at the masked texels of xyz [H, W, 3],
    quantised as the reference does (renderer.py:235 truncation, after a clamp
    to [0, 1]) -> [H, W, 3] uint8 image, zero where not masked."""
    H, W = mask.shape
    img = torch.zeros(H, W, 3, dtype=torch.uint8, device=xyz.device)
    pts = xyz[mask]
    if len(pts):
        cols = []
        for head in range(0, len(pts), BAKE_CHUNK):
            feats = model.density(pts[head:head + BAKE_CHUNK].contiguous())["albedo"].float()
            cols.append((feats.clamp(0, 1) * 255).to(torch.uint8))
        img[mask] = torch.cat(cols)
    return img


@torch.no_grad()
def bake_texture(model, xyz, mask, dilate=3):
    """renderer.py:199-256: albedo at the covered texels, then `dilate` 3x3
    dilation steps to pad the seams.  Returns (image [H, W, 3] uint8 on the
    device, the mask before dilation)."""
    import _texture
    img = query_texels(model, xyz, mask)
    img, _ = _texture.texture_dilate(img, mask.to(torch.uint8), dilate)
    return img, mask


def write_mtl(path, texture_name):
    """The material of the textured OBJ (renderer.py:289-297)."""
    with open(path, "w") as fp:
        fp.write("# single-stable-dreamfusion_amd export_mesh material\n")
        fp.write("newmtl mat0\n")
        fp.write("Ka 1.000000 1.000000 1.000000\n")
        fp.write("Kd 1.000000 1.000000 1.000000\n")
        fp.write("Ks 0.000000 0.000000 0.000000\n")
        fp.write("Tr 1.000000\n")
        fp.write("illum 1\n")
        fp.write("Ns 0.000000\n")
        fp.write(f"map_Kd {texture_name}\n")


def write_obj_textured(path, vertices, faces, vt, ft, mtl_name):
    """Wavefront OBJ with texture coordinates (renderer.py:273-287): image row
    0 is the top of the PNG, OBJ v = 0 the bottom, hence `vt u 1-v`."""
    with open(path, "w") as fp:
        fp.write("# single-stable-dreamfusion_amd export_mesh (marching tetrahedra, "
                 "grid atlas)\n")
        fp.write(f"mtllib {mtl_name}\n")
        fp.writelines(f"v {a} {b} {c}\n" for a, b, c in vertices)
        fp.writelines(f"vt {u} {1 - w}\n" for u, w in vt)
        fp.write("usemtl mat0\n")
        fp.writelines(f"f {a + 1}/{ta + 1} {b + 1}/{tb + 1} {c + 1}/{tc + 1}\n"
                      for (a, b, c), (ta, tb, tc) in zip(faces, ft))


def write_png(path, image):
    """[H, W, 3] uint8 RGB, image row r = texel row r."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image, np.uint8), "RGB").save(path)


def export_mesh(model, path, resolution=None, S=128, name="", texture_size=0):
    """NeRFRenderer.export_mesh (renderer.py:121-299) without mcubes / xatlas /
    nvdiffrast: lattice query, marching tetrahedra at
    min(mean_density, density_thresh), then

    * texture_size = 0: albedo at the vertices, `{name}mesh.obj` with vertex
      colours under `path`;
    * texture_size = None (automatic) or a positive size: `{name}mesh.obj`
      with UVs, `{name}mesh.mtl` and the baked `{name}albedo.png`.

    Returns (vertices [V, 3] float32 in [-1, 1], faces [F, 3])."""
    if resolution is None:
        resolution = model.grid_size
    mean = model.mean_density
    mean = float(mean) if not torch.is_tensor(mean) else float(mean.item())
    thresh = min(mean, float(model.density_thresh))
    device = model.density_bitfield.device
    sig = query_lattice(model.density, resolution, S, device)
    verts, faces = isosurface(sig, thresh)
    verts = (verts / (resolution - 1.0) * 2 - 1).astype(np.float32)
    faces = faces.astype(np.int32)
    os.makedirs(path, exist_ok=True)
    obj = os.path.join(path, f"{name}mesh.obj")
    if texture_size is not None and texture_size == 0:
        colors = None
        if len(verts):
            cols = []
            for head in range(0, len(verts), BAKE_CHUNK):
                chunk = torch.from_numpy(verts[head:head + BAKE_CHUNK]).to(device).contiguous()
                cols.append(model.density(chunk)["albedo"].float().cpu().numpy())
            colors = np.clip(np.concatenate(cols), 0, 1)
        write_obj(obj, verts, faces, colors)
        return verts, faces
    if len(faces) == 0:
        # nothing to bake (and nothing launched): an empty OBJ and a black texel
        vt, ft = np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32)
        image = np.zeros((1, 1, 3), np.uint8)
    else:
        vt, ft, H, W = grid_atlas(len(faces), texture_size)
        with torch.cuda.device(device):
            _, xyz, mask = rasterize_uv(vt, ft, verts, faces, H, W)
            image = bake_texture(model, xyz, mask)[0].cpu().numpy()
    write_png(os.path.join(path, f"{name}albedo.png"), image)
    write_mtl(os.path.join(path, f"{name}mesh.mtl"), f"{name}albedo.png")
    write_obj_textured(obj, verts, faces, vt, ft, f"{name}mesh.mtl")
    return verts, faces
