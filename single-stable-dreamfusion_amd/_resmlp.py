"""Native fused vanilla field (csrc/resmlp.hip): frequency encoding (degree
6) -> residual MLP 39 -> 128 x4 -> 4 -> trunc_exp density with the Gaussian
blob and sigmoid albedo (reference nerf/network.py:13-115 under fp16
autocast), forward and backward, on MFMA.  No reference pybind counterpart:
the reference runs this as torch ops."""
import ctypes

import torch

import _dfhip as _d
from _dfhip import call, checked, ptr, stream

IN, HIDDEN, OUT, BLOCKS = 39, 128, 4, 4
# rows of one MFMA tile (a wave's samples per pass) and rows a workgroup of
# the forward kernel takes per pass (8 waves)
ROW_TILE, WORKGROUP_ROWS = 16, 128

# sigma_net.state_dict() order (include/dfhip.h)
SHAPES = ([(HIDDEN, IN), (HIDDEN,), (HIDDEN,), (HIDDEN,), (HIDDEN, IN)]
          + [(HIDDEN, HIDDEN), (HIDDEN,), (HIDDEN,), (HIDDEN,)] * (BLOCKS - 1)
          + [(OUT, HIDDEN), (OUT,)])


def params_count():
    return int(_d.load().dfhip_resmlp_params())


def backward_scratch_bytes(M):
    return int(_d.load().dfhip_resmlp_field_backward_scratch(int(M)))


def _f32(t, what):
    checked(t, what)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 tensor")


def _pointers(ts, what):
    if len(ts) != len(SHAPES):
        raise RuntimeError(f"expected the {len(SHAPES)} sigma_net tensors in state_dict order")
    for i, (t, shp) in enumerate(zip(ts, SHAPES)):
        _f32(t, f"{what}{i}")
        if tuple(t.shape) != shp:
            raise RuntimeError(f"{what}{i} must have shape {shp}, got {tuple(t.shape)}")
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def field_forward(xyz, params, sigma, albedo):
    """xyz [M, 3] f32 -> sigma [M] f32, albedo [M, 3] f16."""
    M = xyz.shape[0]
    _f32(xyz, "xyz")
    _f32(sigma, "sigma")
    checked(albedo, "albedo")
    if tuple(xyz.shape) != (M, 3) or tuple(sigma.shape) != (M,) or \
            tuple(albedo.shape) != (M, 3) or albedo.dtype != torch.float16:
        raise RuntimeError("xyz [M, 3] f32, sigma [M] f32 and albedo [M, 3] f16 expected")
    call("dfhip_resmlp_field_forward", ptr(xyz), _pointers(params, "param"), ptr(sigma),
         ptr(albedo), M, stream())


def render_rays_infer(rays_o, rays_d, nears, fars, noises, bound, dt_gamma, max_steps, C, H,
                      bitfield, T_thresh, params, weights_sum, depth, image, work, order=None,
                      chunk_log2=6, tile_w=0):
    """Albedo inference render of N rays of the vanilla backbone in one launch
    (csrc/resmlprender.hip, dfhip_resmlp_render_rays_infer).  rays_o / rays_d
    [N, 3] f32, nears / fars [N] f32, noises [N] f32 or None, bitfield u8 (C
    cascades of H^3 cells), params: the 19 sigma_net tensors.  Writes
    weights_sum [N], depth [N], image [N, 3] f32; work: [4] int32 scratch whose
    words 1, 2 hold the evaluated sample count afterwards.  order / chunk_log2
    / tile_w: the queue order of _fieldmlp.render_ray_order (None: pixel
    order)."""
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
    call("dfhip_resmlp_render_rays_infer", n, ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars),
         ptr(noises), float(bound), float(dt_gamma), int(max_steps), int(C), int(H), ptr(bitfield),
         float(T_thresh), _pointers(params, "param"), ptr(weights_sum), ptr(depth), ptr(image),
         ptr(work), ptr(order), int(chunk_log2), int(tile_w), stream())


def field_backward(xyz, params, grad_sigma, grad_albedo, dx=None, grads=None, accumulate=False,
                   scratch=None):
    """grads: the 19 f32 gradients shaped as params (overwritten, or added
    into with accumulate) or None; dx: [M, 3] f32 input gradient or None.
    scratch: uint8 tensor of backward_scratch_bytes(M) or None (allocated)."""
    M = xyz.shape[0]
    _f32(xyz, "xyz")
    _f32(grad_sigma, "grad_sigma")
    checked(grad_albedo, "grad_albedo")
    if grad_albedo.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("grad_albedo must be float16 or float32")
    if tuple(xyz.shape) != (M, 3) or tuple(grad_sigma.shape) != (M,) or \
            tuple(grad_albedo.shape) != (M, 3):
        raise RuntimeError("xyz [M, 3], grad_sigma [M] and grad_albedo [M, 3] expected")
    if dx is not None:
        _f32(dx, "dx")
        if tuple(dx.shape) != (M, 3):
            raise RuntimeError("dx must be [M, 3]")
    need = backward_scratch_bytes(M)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=xyz.device)
    checked(scratch, "scratch", "u8")
    if scratch.numel() < need:
        raise RuntimeError(f"scratch must hold {need} bytes")
    call("dfhip_resmlp_field_backward", ptr(xyz), _pointers(params, "param"), ptr(grad_sigma),
         ptr(grad_albedo), _d.dtype_code(grad_albedo, "grad_albedo"), M, ptr(dx), ptr(scratch),
         None if grads is None else _pointers(grads, "grad"), int(bool(accumulate)), stream())


# ---------------------------------------------------------------- device counts
def backward_dev_scratch_bytes(cap):
    """Bytes of field_backward_dev's scratch: 3392 bytes of tile state and 1232
    neuron-major f16 rows per sample of the capacity, plus 64 partial images
    of the gradients and 256 LayerNorm partials per 65536 rows."""
    return int(_d.load().dfhip_resmlp_field_backward_dev_scratch(int(cap)))


def _count(m_dev, align):
    checked(m_dev, "m_dev", "int")
    if m_dev.numel() < 1:
        raise RuntimeError("m_dev must hold the live row count (int32)")
    if int(align) < 1:
        raise RuntimeError("align must be at least 1")


def field_forward_dev(xyz, params, sigma, albedo, m_dev, align=1):
    """field_forward on the rows [0, m_dev[0]) of capacity-sized buffers: xyz
    [cap, 3], sigma [cap], albedo [cap, 3] f16; rows at or past the live count
    are neither read nor written."""
    cap = xyz.shape[0]
    _f32(xyz, "xyz")
    _f32(sigma, "sigma")
    checked(albedo, "albedo")
    _count(m_dev, align)
    if tuple(xyz.shape) != (cap, 3) or tuple(sigma.shape) != (cap,) or \
            tuple(albedo.shape) != (cap, 3) or albedo.dtype != torch.float16:
        raise RuntimeError("xyz [cap, 3] f32, sigma [cap] f32 and albedo [cap, 3] f16 expected")
    call("dfhip_resmlp_field_forward_dev", ptr(xyz), _pointers(params, "param"), ptr(sigma),
         ptr(albedo), cap, ptr(m_dev), int(align), stream())


def field_backward_dev(xyz, params, grad_sigma, grad_albedo, grads, m_dev, align=1,
                       accumulate=False, scratch=None):
    """field_backward's parameter gradients over min(cap, align_up(m_dev[0],
    align)) rows of capacity-sized buffers, rows from the live count on taken
    as zero padding (never read): the bits of field_backward on that many rows
    with zeroed tail rows.  scratch: uint8 tensor of
    backward_dev_scratch_bytes(cap) or None (allocated)."""
    cap = xyz.shape[0]
    _f32(xyz, "xyz")
    _f32(grad_sigma, "grad_sigma")
    checked(grad_albedo, "grad_albedo")
    _count(m_dev, align)
    if grad_albedo.dtype not in (torch.float16, torch.float32):
        raise RuntimeError("grad_albedo must be float16 or float32")
    if tuple(xyz.shape) != (cap, 3) or tuple(grad_sigma.shape) != (cap,) or \
            tuple(grad_albedo.shape) != (cap, 3):
        raise RuntimeError("xyz [cap, 3], grad_sigma [cap] and grad_albedo [cap, 3] expected")
    need = backward_dev_scratch_bytes(cap)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=xyz.device)
    checked(scratch, "scratch", "u8")
    if scratch.numel() < need:
        raise RuntimeError(f"scratch must hold {need} bytes")
    call("dfhip_resmlp_field_backward_dev", ptr(xyz), _pointers(params, "param"),
         ptr(grad_sigma), ptr(grad_albedo), _d.dtype_code(grad_albedo, "grad_albedo"), cap,
         ptr(m_dev), int(align), ptr(scratch), _pointers(grads, "grad"), int(bool(accumulate)),
         stream())
