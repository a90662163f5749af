"""`_texture` backend module: the texture bake of export_mesh (UV rasteriser,
attribute interpolation, seam dilation) over the gfx950 C-ABI
(csrc/texture.hip).  No reference extension has these entries: they stand in
for nvdiffrast's dr.rasterize / dr.interpolate and the kd-tree seam fill of
nerf/renderer.py:195-256."""
import torch

from _dfhip import call, ptr, stream, checked


def _size(H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise RuntimeError(f"texture: H*W must be in [1, 2^31), got {H} x {W}")
    return H, W


def _faces(idx, what, rows):
    """An [F, 3] int32 index tensor whose entries are rows of a `rows`-row
    table (checked here: the kernels only skip faces with a bad index)."""
    checked(idx, what, "int")
    if idx.dim() != 2 or idx.shape[1] != 3:
        raise RuntimeError(f"{what} must be [F, 3]")
    if idx.shape[0] >= 2 ** 31:
        raise RuntimeError(f"{what}: F must be below 2^31")
    if idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= rows:
            raise RuntimeError(f"{what}: index out of range [0, {rows}) (min {lo}, max {hi})")
    return idx.shape[0]


def raster_uv_faces(vt, ft, H, W):
    """vt [T, 2] f32 UVs, ft [F, 3] int32 -> face_id [H*W] int32 (lowest
    covering face per texel centre, -1 where none)."""
    H, W = _size(H, W)
    checked(vt, "vt")
    if vt.dtype != torch.float32 or vt.dim() != 2 or vt.shape[1] != 2:
        raise RuntimeError("vt must be an [T, 2] float32 tensor")
    F = _faces(ft, "ft", vt.shape[0])
    face_id = torch.empty(H * W, dtype=torch.int32, device=vt.device)
    call("dfhip_raster_uv_faces", ptr(vt), ptr(ft), F, vt.shape[0], H, W, ptr(face_id), stream())
    return face_id


def raster_uv_interp(vt, ft, v, f, face_id, H, W, want_bary=False):
    """Positions v [V, 3] f32 of the faces f [F, 3] int32 interpolated at the
    covered texel centres -> xyz [H*W, 3] f32 (zeros where uncovered) and,
    with want_bary, bary [H*W, 2] = (w1, w2)."""
    H, W = _size(H, W)
    checked(vt, "vt")
    checked(v, "v")
    if vt.dtype != torch.float32 or v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise RuntimeError("vt / v must be [T, 2] / [V, 3] float32 tensors")
    F = _faces(ft, "ft", vt.shape[0])
    if _faces(f, "f", v.shape[0]) != F:
        raise RuntimeError("ft and f must have one row per face")
    checked(face_id, "face_id", "int")
    if face_id.numel() != H * W:
        raise RuntimeError("face_id must have H*W entries")
    xyz = torch.empty(H * W, 3, dtype=torch.float32, device=v.device)
    bary = torch.empty(H * W, 2, dtype=torch.float32, device=v.device) if want_bary else None
    call("dfhip_raster_uv_interp", ptr(vt), ptr(ft), ptr(v), ptr(f), ptr(face_id), F, vt.shape[0],
         v.shape[0], H, W, ptr(xyz), ptr(bary), stream())
    return (xyz, bary) if want_bary else xyz


def texture_dilate(rgb, mask, iterations=3):
    """`iterations` dilation steps of an [H, W, 3] uint8 image under an [H, W]
    uint8 mask (ping-pong between two buffer pairs).  Returns new (rgb, mask);
    the inputs are not written."""
    checked(rgb, "rgb", "u8")
    checked(mask, "mask", "u8")
    if rgb.dim() != 3 or rgb.shape[2] != 3 or tuple(mask.shape) != tuple(rgb.shape[:2]):
        raise RuntimeError("rgb must be [H, W, 3] and mask [H, W]")
    H, W = _size(*mask.shape)
    if iterations <= 0:
        return rgb.clone(), mask.clone()
    src = (rgb, mask)
    bufs = [(torch.empty_like(rgb), torch.empty_like(mask)) for _ in range(min(iterations, 2))]
    for i in range(iterations):
        dst = bufs[i % len(bufs)]
        call("dfhip_texture_dilate", ptr(src[0]), ptr(src[1]), H, W, ptr(dst[0]), ptr(dst[1]),
             stream())
        src = dst
    return src
