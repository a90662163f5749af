"""Native fused voxel field (csrc/voxelfield.hip): the DVGO backbone's
coordinate map, trilinear density / feature samples, position and view
encodings, colour MLP dim0 -> 128 -> 128 -> 3 and activations (reference
nerf/network.py:245-268 under fp16 autocast), its parameter-gradient backward
and the closed-form normal.  No reference pybind counterpart: the reference
runs this as torch ops."""
import ctypes

import torch

import _dfhip as _d
from _dfhip import call, checked, ptr, stream

HIDDEN, OUT, MAX_IN = 128, 3, 96
# rows of one MFMA tile (a wave's samples per pass) and rows a workgroup of
# the forward kernel takes per pass (8 waves)
ROW_TILE, WORKGROUP_ROWS = 16, 128


def shapes(dim0):
    """rgbnet.state_dict() order (include/dfhip.h)."""
    return [(HIDDEN, dim0), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (OUT, HIDDEN), (OUT,)]


class Volume:
    """The frozen operands of one checkpoint on one device: density
    [Nx, Ny, Nz] f32, k0 [Nx, Ny, Nz, C] f32 (channel last), the box (host
    floats: min xyz, max xyz), the number of position frequencies and the f32
    view encoding [view_dim] (or None)."""

    def __init__(self, density, k0, box, pos_freqs, view):
        checked(density, "density")
        checked(k0, "k0")
        if density.dtype != torch.float32 or k0.dtype != torch.float32:
            raise RuntimeError("density and k0 must be float32 tensors")
        if density.dim() != 3 or k0.dim() != 4 or tuple(k0.shape[:3]) != tuple(density.shape):
            raise RuntimeError("density [Nx, Ny, Nz] and k0 [Nx, Ny, Nz, C] expected")
        if view is not None:
            checked(view, "view")
            if view.dtype != torch.float32 or view.dim() != 1:
                raise RuntimeError("view must be a float32 vector")
        if len(box) != 6:
            raise RuntimeError("box must hold six floats: min xyz, max xyz")
        self.density, self.k0, self.view = density, k0, view
        self.box = (ctypes.c_float * 6)(*[float(v) for v in box])
        self.n = tuple(int(v) for v in density.shape)
        self.C, self.pos_freqs = int(k0.shape[3]), int(pos_freqs)
        self.view_dim = 0 if view is None else int(view.numel())
        self.dim0 = self.C + (3 + 6 * self.pos_freqs if self.pos_freqs else 0) + self.view_dim


def backward_scratch_bytes(M, dim0):
    return int(_d.load().dfhip_voxel_field_backward_scratch(int(M), int(dim0)))


def _f32(t, what):
    checked(t, what)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 tensor")


def _pointers(ts, dim0, what):
    want = shapes(dim0)
    if len(ts) != len(want):
        raise RuntimeError(f"expected the {len(want)} rgbnet tensors in state_dict order")
    for i, (t, shp) in enumerate(zip(ts, want)):
        _f32(t, f"{what}{i}")
        if tuple(t.shape) != shp:
            raise RuntimeError(f"{what}{i} must have shape {shp}, got {tuple(t.shape)}")
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _positions(xyz):
    _f32(xyz, "xyz")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError("xyz [M, 3] f32 expected")
    return xyz.shape[0]


def field_forward(xyz, vol, bound, act_shift, params, sigma, albedo=None):
    """xyz [M, 3] f32 -> sigma [M] f32, albedo [M, 3] f16 (None: density only,
    params may then be None)."""
    M = _positions(xyz)
    _f32(sigma, "sigma")
    if tuple(sigma.shape) != (M,):
        raise RuntimeError("sigma [M] f32 expected")
    pp = None
    if albedo is not None:
        checked(albedo, "albedo")
        if tuple(albedo.shape) != (M, 3) or albedo.dtype != torch.float16:
            raise RuntimeError("albedo [M, 3] f16 expected")
        pp = _pointers(params, vol.dim0, "param")
    call("dfhip_voxel_field_forward", ptr(xyz), ptr(vol.density), ptr(vol.k0), *vol.n, vol.C,
         vol.pos_freqs, ptr(vol.view), vol.view_dim, vol.box, float(bound), float(act_shift), pp,
         ptr(sigma), ptr(albedo), M, stream())


def field_backward(xyz, vol, bound, params, grad_albedo, grads, accumulate=False, scratch=None):
    """grads: the 6 f32 gradients shaped as params (overwritten, or added into
    with accumulate).  scratch: uint8 tensor of backward_scratch_bytes(M,
    dim0) or None (allocated)."""
    M = _positions(xyz)
    checked(grad_albedo, "grad_albedo")
    if grad_albedo.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("grad_albedo must be float16 or float32")
    if tuple(grad_albedo.shape) != (M, 3):
        raise RuntimeError("grad_albedo [M, 3] expected")
    need = backward_scratch_bytes(M, vol.dim0)
    if scratch is None:
        scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=xyz.device)
    checked(scratch, "scratch", "u8")
    if scratch.numel() < need:
        raise RuntimeError(f"scratch must hold {need} bytes")
    call("dfhip_voxel_field_backward", ptr(xyz), ptr(vol.k0), *vol.n, vol.C, vol.pos_freqs,
         ptr(vol.view), vol.view_dim, vol.box, float(bound), _pointers(params, vol.dim0, "param"),
         ptr(grad_albedo), _d.dtype_code(grad_albedo, "grad_albedo"), M, ptr(scratch),
         _pointers(grads, vol.dim0, "grad"), int(bool(accumulate)), stream())


def normal(xyz, vol, bound, act_shift, out):
    """xyz [M, 3] f32 -> out [M, 3] f32 = -d sigma / d x (not normalised)."""
    M = _positions(xyz)
    _f32(out, "normal")
    if tuple(out.shape) != (M, 3):
        raise RuntimeError("normal [M, 3] f32 expected")
    call("dfhip_voxel_normal", ptr(xyz), ptr(vol.density), *vol.n, vol.box, float(bound),
         float(act_shift), ptr(out), M, stream())


# ---- device-count forms (the native train step: capacity-sized buffers, the
# live row count in a device int32, launch shapes of the capacity only)

SHADINGS = {"albedo": 0, "textureless": 1, "lambertian": 2, "normal": 3}  # dfhip_shading


def backward_dev_scratch_bytes(cap, dim0):
    """Bytes of field_backward_dev's scratch: 616 rows x 2 bytes per sample of
    the capacity, plus 64 partial images of the gradients per 65536 rows."""
    return int(_d.load().dfhip_voxel_field_backward_dev_scratch(int(cap), int(dim0)))


def _count(m_dev, align):
    checked(m_dev, "m_dev", "int")
    if m_dev.numel() < 1:
        raise RuntimeError("m_dev must hold the live row count (int32)")
    if int(align) < 1:
        raise RuntimeError("align must be at least 1")


def field_forward_dev(xyz, vol, bound, act_shift, params, sigma, albedo, m_dev, align=1):
    """field_forward on the rows [0, m_dev[0]) of capacity-sized buffers: xyz
    [cap, 3], sigma [cap], albedo [cap, 3] f16 or None (density only); rows
    at or past the live count are neither read nor written."""
    cap = _positions(xyz)
    _count(m_dev, align)
    _f32(sigma, "sigma")
    if tuple(sigma.shape) != (cap,):
        raise RuntimeError("sigma [cap] f32 expected")
    pp = None
    if albedo is not None:
        checked(albedo, "albedo")
        if tuple(albedo.shape) != (cap, 3) or albedo.dtype != torch.float16:
            raise RuntimeError("albedo [cap, 3] f16 expected")
        pp = _pointers(params, vol.dim0, "param")
    call("dfhip_voxel_field_forward_dev", ptr(xyz), ptr(vol.density), ptr(vol.k0), *vol.n, vol.C,
         vol.pos_freqs, ptr(vol.view), vol.view_dim, vol.box, float(bound), float(act_shift), pp,
         ptr(sigma), ptr(albedo), cap, ptr(m_dev), int(align), stream())


def field_backward_dev(xyz, vol, bound, params, grad_albedo, grads, m_dev, align=1,
                       accumulate=False, scratch=None):
    """field_backward over min(cap, align_up(m_dev[0], align)) rows of
    capacity-sized buffers, rows from the live count on taken as zero padding
    (never read): the bits of field_backward on that many rows with zeroed
    tail rows.  scratch: uint8 tensor of backward_dev_scratch_bytes(cap,
    dim0) or None (allocated)."""
    cap = _positions(xyz)
    _count(m_dev, align)
    checked(grad_albedo, "grad_albedo")
    if grad_albedo.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("grad_albedo must be float16 or float32")
    if tuple(grad_albedo.shape) != (cap, 3):
        raise RuntimeError("grad_albedo [cap, 3] expected")
    need = backward_dev_scratch_bytes(cap, vol.dim0)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=xyz.device)
    checked(scratch, "scratch", "u8")
    if scratch.numel() < need:
        raise RuntimeError(f"scratch must hold {need} bytes")
    call("dfhip_voxel_field_backward_dev", ptr(xyz), ptr(vol.k0), *vol.n, vol.C, vol.pos_freqs,
         ptr(vol.view), vol.view_dim, vol.box, float(bound), _pointers(params, vol.dim0, "param"),
         ptr(grad_albedo), _d.dtype_code(grad_albedo, "grad_albedo"), cap, ptr(m_dev), int(align),
         ptr(scratch), _pointers(grads, vol.dim0, "grad"), int(bool(accumulate)), stream())


def normal_dev(xyz, vol, bound, act_shift, out, m_dev, align=1):
    """normal on the rows [0, m_dev[0]) of capacity-sized buffers."""
    cap = _positions(xyz)
    _count(m_dev, align)
    _f32(out, "normal")
    if tuple(out.shape) != (cap, 3):
        raise RuntimeError("normal [cap, 3] f32 expected")
    call("dfhip_voxel_normal_dev", ptr(xyz), ptr(vol.density), *vol.n, vol.box, float(bound),
         float(act_shift), ptr(out), cap, ptr(m_dev), int(align), stream())


def shade_partial_doubles(cap):
    return int(_d.load().dfhip_shading_partial_doubles(int(cap)))


def _half(t, what, shape):
    checked(t, what)
    if t.dtype != torch.float16 or tuple(t.shape) != shape:
        raise RuntimeError(f"{what} {list(shape)} f16 expected")


def shade_train_forward(xyz, dirs, vol, bound, act_shift, albedo, light, ratio, shading, m_dev,
                        align, normal, lam, color, partial, orient):
    """The textureless / lambertian colours of a train step on the rows
    [0, m_dev[0]) of capacity-sized buffers (csrc/voxelstep.hip): writes the
    unit normal [cap, 3] f32, the lambertian factor [cap] f16, the colour
    [cap, 3] f16 and orient [1] f32, the orientation term's mean over
    min(cap, align_up(m_dev[0], align)) rows.  albedo [cap, 3] f16 (lambertian;
    else None), light [3] f32 on the device, partial:
    shade_partial_doubles(cap) float64 of scratch."""
    cap = _positions(xyz)
    _count(m_dev, align)
    code = SHADINGS.get(shading, shading) if isinstance(shading, str) else shading
    if code not in (1, 2):
        raise RuntimeError(f"shading must be textureless or lambertian, got {shading!r}")
    for t, what in ((dirs, "dirs"), (normal, "normal")):
        _f32(t, what)
        if tuple(t.shape) != (cap, 3):
            raise RuntimeError(f"{what} [cap, 3] f32 expected")
    if code == 2:
        _half(albedo, "albedo", (cap, 3))
    _half(lam, "lam", (cap,))
    _half(color, "color", (cap, 3))
    _f32(light, "light")
    _f32(orient, "orient")
    if light.numel() != 3 or orient.numel() < 1:
        raise RuntimeError("light [3] and orient [1] f32 expected")
    checked(partial, "partial")
    if partial.dtype != torch.float64 or partial.numel() < shade_partial_doubles(cap):
        raise RuntimeError(f"partial must hold {shade_partial_doubles(cap)} float64")
    call("dfhip_voxel_shade_train_forward", ptr(xyz), ptr(dirs), ptr(vol.density), *vol.n, vol.box,
         float(bound), float(act_shift), ptr(albedo) if code == 2 else None, ptr(light),
         float(ratio), int(code), cap, ptr(m_dev), int(align), ptr(normal), ptr(lam), ptr(color),
         ptr(partial), ptr(orient), stream())


def shade_train_backward(grad_color, lam, shading, m_dev, align, grad_albedo):
    """grad_albedo [cap, 3] f16 = f16(grad_color * lam) on the live rows of a
    lambertian step; a textureless step has no albedo gradient (no launch)."""
    code = SHADINGS.get(shading, shading) if isinstance(shading, str) else shading
    if code not in (1, 2):
        raise RuntimeError(f"shading must be textureless or lambertian, got {shading!r}")
    _count(m_dev, align)
    cap = lam.shape[0]
    _half(lam, "lam", (cap,))
    _half(grad_color, "grad_color", (cap, 3))
    _half(grad_albedo, "grad_albedo", (cap, 3))
    call("dfhip_voxel_shade_train_backward", ptr(grad_color), ptr(lam), int(code), cap,
         ptr(m_dev), int(align), ptr(grad_albedo), stream())


# ---- fused inference render (march + voxel field + composite, persistent queue)


def render_rays_infer(rays_o, rays_d, nears, fars, noises, bound, dt_gamma, max_steps, C, H,
                      bitfield, T_thresh, vol, act_shift, params, weights_sum, depth, image, work,
                      shading="albedo", light=None, ratio=1.0, order=None, chunk_log2=6, tile_w=0):
    """Inference render of N rays of the DVGO backbone in one launch
    (csrc/voxelrender.hip; dfhip_voxel_render_rays_infer, or its _shaded form
    for shading "textureless" / "lambertian" / "normal").  rays_o / rays_d
    [N, 3] f32, nears / fars [N] f32, noises [N] f32 or None, bitfield u8 (C
    cascades of H^3 cells), vol: the checkpoint's Volume, params: the 6 rgbnet
    tensors (None for the textureless and normal shadings, which read no
    colour).  light: [3] f32 device tensor, ratio: the ambient ratio (shaded
    frames).  Writes weights_sum [N], depth [N], image [N, 3] f32; work: [4]
    int32 scratch whose words 1, 2 hold the evaluated sample count afterwards.
    order / chunk_log2 / tile_w: the queue order of _fieldmlp.render_ray_order
    (None: pixel order)."""
    n = rays_o.shape[0]
    for t, what, shp in ((rays_o, "rays_o", (n, 3)), (rays_d, "rays_d", (n, 3)),
                         (nears, "nears", (n,)), (fars, "fars", (n,)),
                         (weights_sum, "weights_sum", (n,)), (depth, "depth", (n,)),
                         (image, "image", (n, 3))):
        _f32(t, what)
        if tuple(t.shape) != shp:
            raise RuntimeError(f"{what} must have shape {shp}, got {tuple(t.shape)}")
    if noises is not None:
        _f32(noises, "noises")
        if tuple(noises.shape) != (n,):
            raise RuntimeError("noises must be [N]")
    checked(bitfield, "bitfield", "u8")
    if bitfield.numel() * 8 < C * H ** 3:
        raise RuntimeError("bitfield is smaller than C * H^3 / 8 bytes")
    checked(work, "work", "int")
    if work.numel() < 4:
        raise RuntimeError("work must hold 4 int32")
    if order is not None:
        checked(order, "order", "int")
        if tuple(order.shape) != (-(-n // (1 << chunk_log2)),):
            raise RuntimeError("order must be [ceil(N / 2^chunk_log2)] int32")
    code = SHADINGS.get(shading, shading) if isinstance(shading, str) else shading
    if isinstance(code, str):
        raise RuntimeError(f"unknown shading {shading!r}")
    colour = code in (0, 2)
    pp = _pointers(params, vol.dim0, "param") if colour else None
    args = (n, ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(noises), float(bound),
            float(dt_gamma), int(max_steps), int(C), int(H), ptr(bitfield), float(T_thresh),
            ptr(vol.density), ptr(vol.k0), *vol.n, vol.C, vol.pos_freqs, ptr(vol.view),
            vol.view_dim, vol.box, float(act_shift), pp, ptr(weights_sum), ptr(depth), ptr(image),
            ptr(work), ptr(order), int(chunk_log2), int(tile_w))
    if code == 0:
        call("dfhip_voxel_render_rays_infer", *args, stream())
        return
    if light is not None:
        _f32(light, "light")
        if light.numel() != 3:
            raise RuntimeError("light must hold 3 float32 values")
    call("dfhip_voxel_render_rays_infer_shaded", *args, int(code), ptr(light), float(ratio),
         stream())
