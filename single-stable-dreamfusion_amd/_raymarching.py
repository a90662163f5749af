"""`_raymarching` backend module: the reference pybind11 surface
(raymarching/src/bindings.cpp:5-18) over the gfx950 C-ABI (include/dfhip.h).

Same argument order and in-place output convention as the reference: the
caller allocates every output, the function returns None.  Unlike the
reference (no checks, raymarching.cu:13-16 unused), device / contiguity /
dtype are validated and raise RuntimeError.
"""
import torch

import _dfhip as _d
from _dfhip import call, ptr, stream, checked


def _f(t, what):
    checked(t, what)
    return _d.dtype_code(t, what)


def packbits(grid, N, density_thresh, bitfield):
    dt = _f(grid, "grid")
    checked(bitfield, "bitfield", "u8")
    call("dfhip_packbits", dt, ptr(grid), N, density_thresh, ptr(bitfield), stream())


def near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars):
    dt = _f(rays_o, "rays_o")
    for t, w in ((rays_d, "rays_d"), (aabb, "aabb"), (nears, "nears"), (fars, "fars")):
        checked(t, w)
    call("dfhip_near_far_from_aabb", dt, ptr(rays_o), ptr(rays_d), ptr(aabb), N, min_near,
         ptr(nears), ptr(fars), stream())


def sph_from_ray(rays_o, rays_d, radius, N, coords):
    dt = _f(rays_o, "rays_o")
    checked(rays_d, "rays_d")
    checked(coords, "coords")
    call("dfhip_sph_from_ray", dt, ptr(rays_o), ptr(rays_d), radius, N, ptr(coords), stream())


def morton3D(coords, N, indices):
    checked(coords, "coords", "int")
    checked(indices, "indices", "int")
    call("dfhip_morton3D", ptr(coords), N, ptr(indices), stream())


def morton3D_invert(indices, N, coords):
    checked(indices, "indices", "int")
    checked(coords, "coords", "int")
    call("dfhip_morton3D_invert", ptr(indices), N, ptr(coords), stream())


def march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears, fars,
                     xyzs, dirs, deltas, rays, counter, noises):
    dt = _f(rays_o, "rays_o")
    checked(grid, "grid", "u8")
    checked(rays, "rays", "int")
    checked(counter, "counter", "int")
    call("dfhip_march_rays_train", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound, dt_gamma,
         max_steps, N, C, H, M, ptr(nears), ptr(fars), ptr(xyzs), ptr(dirs), ptr(deltas),
         ptr(rays), ptr(counter), ptr(noises), stream())


# ---- native split form (deterministic count / emit; see dfhip.h)

def march_rays_train_scratch_ints(N):
    return int(_d.load().dfhip_march_rays_train_scratch_ints(N))


def _march_opts(mode, guard_ulps, stats):
    """The trailing (mode, guard_ulps, stats) of the _opts march entries, or
    None when all three are the defaults (the plain entry is called then)."""
    if mode == 0 and guard_ulps == 0 and stats is None:
        return None
    if mode not in (0, 1) or not 0 <= guard_ulps < 2 ** 32:
        raise RuntimeError("mode must be 0 or 1 and guard_ulps a uint32")
    if stats is not None:
        checked(stats, "stats", "int")
        if stats.numel() < 2:
            raise RuntimeError("stats must hold two ints (restarted, chain-free)")
    return int(mode), int(guard_ulps), ptr(stats)


def march_rays_train_count(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, nears, fars,
                           rays, counter, noises, block_sums, mode=0, guard_ulps=0, stats=None):
    """mode / guard_ulps / stats: see dfhip_march_rays_train_count_opts (tests
    and tools; results do not depend on them)."""
    dt = _f(rays_o, "rays_o")
    checked(grid, "grid", "u8")
    checked(block_sums, "block_sums", "int")
    opts = _march_opts(mode, guard_ulps, stats)
    if opts is not None:
        call("dfhip_march_rays_train_count_opts", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound,
             dt_gamma, max_steps, N, C, H, ptr(nears), ptr(fars), ptr(rays), ptr(counter),
             ptr(noises), ptr(block_sums), None, *opts, stream())
        return
    call("dfhip_march_rays_train_count", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound, dt_gamma,
         max_steps, N, C, H, ptr(nears), ptr(fars), ptr(rays), ptr(counter), ptr(noises),
         ptr(block_sums), stream())


def march_rays_train_emit(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears,
                          fars, xyzs, dirs, deltas, rays, noises, block_sums, zero_tail, mode=0,
                          guard_ulps=0, stats=None):
    dt = _f(rays_o, "rays_o")
    opts = _march_opts(mode, guard_ulps, stats)
    if opts is not None:
        call("dfhip_march_rays_train_emit_opts", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound,
             dt_gamma, max_steps, N, C, H, M, ptr(nears), ptr(fars), ptr(xyzs), ptr(dirs),
             ptr(deltas), ptr(rays), ptr(noises), ptr(block_sums), int(zero_tail), *opts, stream())
        return
    call("dfhip_march_rays_train_emit", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound, dt_gamma,
         max_steps, N, C, H, M, ptr(nears), ptr(fars), ptr(xyzs), ptr(dirs), ptr(deltas),
         ptr(rays), ptr(noises), ptr(block_sums), int(zero_tail), stream())


def march_rays_train_stage_floats(N, max_steps):
    return int(_d.load().dfhip_march_rays_train_stage_floats(int(N), int(max_steps)))


def march_rays_train_count_staged(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, nears,
                                  fars, rays, counter, noises, block_sums, stage, mode=0,
                                  guard_ulps=0, stats=None):
    """march_rays_train_count that also keeps every sample in `stage` (f32,
    march_rays_train_stage_floats(N, max_steps) floats)."""
    dt = _f(rays_o, "rays_o")
    checked(grid, "grid", "u8")
    checked(block_sums, "block_sums", "int")
    checked(stage, "stage")
    if stage.dtype != torch.float32 or stage.numel() < march_rays_train_stage_floats(N, max_steps):
        raise RuntimeError("stage must be float32 with march_rays_train_stage_floats(N, max_steps) "
                           "elements")
    opts = _march_opts(mode, guard_ulps, stats)
    if opts is not None:
        call("dfhip_march_rays_train_count_opts", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound,
             dt_gamma, max_steps, N, C, H, ptr(nears), ptr(fars), ptr(rays), ptr(counter),
             ptr(noises), ptr(block_sums), ptr(stage), *opts, stream())
        return
    call("dfhip_march_rays_train_count_staged", dt, ptr(rays_o), ptr(rays_d), ptr(grid), bound,
         dt_gamma, max_steps, N, C, H, ptr(nears), ptr(fars), ptr(rays), ptr(counter),
         ptr(noises), ptr(block_sums), ptr(stage), stream())


def march_rays_train_count_staged_quads(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H,
                                        nears, fars, rays, counter, noises, block_sums, stage,
                                        embeddings, offsets, S, Hb, gridtype, align_corners,
                                        table, quads, mode=0, guard_ulps=0, stats=None):
    """march_rays_train_count_staged with _fieldmlp.grid_quads's work (the
    table copy and corner quads of `embeddings`) done by extra workgroups of
    the same launch.  f32 rays; same outputs as the two calls."""
    dt = _f(rays_o, "rays_o")
    checked(grid, "grid", "u8")
    checked(block_sums, "block_sums", "int")
    checked(stage, "stage")
    if stage.dtype != torch.float32 or stage.numel() < march_rays_train_stage_floats(N, max_steps):
        raise RuntimeError("stage must be float32 with march_rays_train_stage_floats(N, max_steps) "
                           "elements")
    checked(embeddings, "embeddings")
    checked(table, "table")
    checked(quads, "quads", "int")
    checked(offsets, "offsets", "int")
    rows = embeddings.shape[0]
    if embeddings.dtype != torch.float32 or tuple(embeddings.shape) != (rows, 2) or \
            table.dtype not in (torch.float16, torch.bfloat16) or tuple(table.shape) != (rows, 2):
        raise RuntimeError("embeddings [rows, 2] f32 and table [rows, 2] f16 / bf16 expected")
    if tuple(quads.shape) != (rows, 4):
        raise RuntimeError("quads must be a [rows, 4] int32 tensor")
    elem = _d.BF16 if table.dtype == torch.bfloat16 else _d.F16
    opts = _march_opts(mode, guard_ulps, stats)
    name = "dfhip_march_rays_train_count_staged_quads" + ("" if opts is None else "_opts")
    call(name, dt, ptr(rays_o), ptr(rays_d), ptr(grid),
         bound, dt_gamma, max_steps, N, C, H, ptr(nears), ptr(fars), ptr(rays), ptr(counter),
         ptr(noises), ptr(block_sums), ptr(stage), elem, ptr(embeddings), ptr(offsets),
         offsets.shape[0] - 1, float(S), int(Hb), int(gridtype), int(bool(align_corners)), rows,
         ptr(table), ptr(quads), *(opts or ()), stream())


def march_rays_train_emit_staged(rays_d, max_steps, N, M, xyzs, dirs, deltas, rays, block_sums,
                                 zero_tail, stage):
    """march_rays_train_emit from the count pass's stage (no second march)."""
    dt = _f(rays_d, "rays_d")
    checked(stage, "stage")
    call("dfhip_march_rays_train_emit_staged", dt, ptr(rays_d), max_steps, N, M, ptr(xyzs),
         ptr(dirs), ptr(deltas), ptr(rays), ptr(block_sums), int(zero_tail), ptr(stage), stream())


def composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth,
                                 image):
    dt = _f(sigmas, "sigmas")
    for t, w in ((rgbs, "rgbs"), (deltas, "deltas"), (weights_sum, "weights_sum"),
                 (depth, "depth"), (image, "image")):
        checked(t, w)
    checked(rays, "rays", "int")
    call("dfhip_composite_rays_train_forward", dt, ptr(sigmas), ptr(rgbs), ptr(deltas), ptr(rays),
         M, N, T_thresh, ptr(weights_sum), ptr(depth), ptr(image), stream())


def _composite_bwd(name, grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum,
                   image, M, N, T_thresh, grad_sigmas, grad_rgbs):
    dt = _f(grad_image, "grad_image")
    for t, w in ((grad_weights_sum, "grad_weights_sum"), (sigmas, "sigmas"), (rgbs, "rgbs"),
                 (deltas, "deltas"), (weights_sum, "weights_sum"), (image, "image"),
                 (grad_sigmas, "grad_sigmas"), (grad_rgbs, "grad_rgbs")):
        checked(t, w)
    call(name, dt, ptr(grad_weights_sum), ptr(grad_image), ptr(sigmas), ptr(rgbs), ptr(deltas),
         ptr(rays), ptr(weights_sum), ptr(image), M, N, T_thresh, ptr(grad_sigmas),
         ptr(grad_rgbs), stream())


def composite_rays_train_backward(*args):
    _composite_bwd("dfhip_composite_rays_train_backward", *args)


def composite_rays_train_backward_dense(*args):
    _composite_bwd("dfhip_composite_rays_train_backward_dense", *args)


# ---- native mixed-precision train compositing (f32 sigmas, f16/f32 colours)

def _f32_only(t, what):
    checked(t, what)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 tensor")


def composite_rays_train_forward_mixed(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum,
                                       depth, image):
    for t, w in ((sigmas, "sigmas"), (deltas, "deltas"), (weights_sum, "weights_sum"),
                 (depth, "depth"), (image, "image")):
        _f32_only(t, w)
    rd = _f(rgbs, "rgbs")
    checked(rays, "rays", "int")
    call("dfhip_composite_rays_train_forward_mixed", rd, ptr(sigmas), ptr(rgbs), ptr(deltas),
         ptr(rays), M, N, T_thresh, ptr(weights_sum), ptr(depth), ptr(image), stream())


def composite_rays_train_backward_mixed(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays,
                                        weights_sum, image, M, N, T_thresh, grad_sigmas,
                                        grad_rgbs, zero_tail=True):
    for t, w in ((grad_weights_sum, "grad_weights_sum"), (grad_image, "grad_image"),
                 (sigmas, "sigmas"), (deltas, "deltas"), (weights_sum, "weights_sum"),
                 (image, "image"), (grad_sigmas, "grad_sigmas")):
        _f32_only(t, w)
    rd = _f(rgbs, "rgbs")
    checked(grad_rgbs, "grad_rgbs")
    if grad_rgbs.dtype != rgbs.dtype:
        raise RuntimeError("grad_rgbs must have the dtype of rgbs")
    checked(rays, "rays", "int")
    call("dfhip_composite_rays_train_backward_mixed", rd, ptr(grad_weights_sum), ptr(grad_image),
         ptr(sigmas), ptr(rgbs), ptr(deltas), ptr(rays), ptr(weights_sum), ptr(image), M, N,
         T_thresh, ptr(grad_sigmas), ptr(grad_rgbs), int(bool(zero_tail)), stream())


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C,
               H, grid, near, far, xyzs, dirs, deltas, noises):
    dt = _f(rays_o, "rays_o")
    checked(rays_alive, "rays_alive", "int")
    checked(grid, "grid", "u8")
    call("dfhip_march_rays", dt, n_alive, n_step, ptr(rays_alive), ptr(rays_t), ptr(rays_o),
         ptr(rays_d), bound, dt_gamma, max_steps, C, H, ptr(grid), ptr(near), ptr(far), ptr(xyzs),
         ptr(dirs), ptr(deltas), ptr(noises), stream())


def composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights,
                   depth, image):
    dt = _f(image, "image")
    checked(rays_alive, "rays_alive", "int")
    for t, w in ((rays_t, "rays_t"), (sigmas, "sigmas"), (rgbs, "rgbs"), (deltas, "deltas"),
                 (weights, "weights"), (depth, "depth")):
        checked(t, w)
    call("dfhip_composite_rays", dt, n_alive, n_step, T_thresh, ptr(rays_alive), ptr(rays_t),
         ptr(sigmas), ptr(rgbs), ptr(deltas), ptr(weights), ptr(depth), ptr(image), stream())


# ---- hierarchical sampling of NeRFRenderer.run (csrc/hiersample.hip, native)

def _f32_opt(t, what):
    if t is not None:
        _f32_only(t, what)


def _i32_opt(t, what):
    if t is not None:
        checked(t, what, "int")


def uniform_samples(rays_o, rays_d, aabb, nears, fars, lin, noise, N, T, z, xyzs):
    for t, w in ((rays_o, "rays_o"), (rays_d, "rays_d"), (aabb, "aabb"), (nears, "nears"),
                 (fars, "fars"), (lin, "lin"), (z, "z"), (xyzs, "xyzs")):
        _f32_only(t, w)
    _f32_opt(noise, "noise")
    call("dfhip_uniform_samples", ptr(rays_o), ptr(rays_d), ptr(aabb), ptr(nears), ptr(fars),
         ptr(lin), ptr(noise), N, T, ptr(z), ptr(xyzs), stream())


def importance_samples(rays_o, rays_d, aabb, nears, fars, z, sigma, u, N, T, t, new_z, new_xyzs):
    for a, w in ((rays_o, "rays_o"), (rays_d, "rays_d"), (aabb, "aabb"), (nears, "nears"),
                 (fars, "fars"), (z, "z"), (sigma, "sigma"), (new_z, "new_z"),
                 (new_xyzs, "new_xyzs")):
        _f32_only(a, w)
    _f32_opt(u, "u")
    call("dfhip_importance_samples", ptr(rays_o), ptr(rays_d), ptr(aabb), ptr(nears), ptr(fars),
         ptr(z), ptr(sigma), ptr(u), N, T, t, ptr(new_z), ptr(new_xyzs), stream())


def merge_samples(z, new_z, xyzs, new_xyzs, N, T, t, z_all, order, xyzs_all):
    for a, w in ((z, "z"), (new_z, "new_z"), (xyzs, "xyzs"), (new_xyzs, "new_xyzs"),
                 (z_all, "z_all"), (xyzs_all, "xyzs_all")):
        _f32_only(a, w)
    checked(order, "order", "int")
    call("dfhip_merge_samples", ptr(z), ptr(new_z), ptr(xyzs), ptr(new_xyzs), N, T, t, ptr(z_all),
         ptr(order), ptr(xyzs_all), stream())


def _rgbs_code(rgbs, what):
    checked(rgbs, what)
    if rgbs.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"{what} must be a float32 or float16 tensor")
    return _d.dtype_code(rgbs, what)


def composite_uniform_forward(sigma_coarse, sigma_new, order, z_all, nears, fars, sample_dist, rgbs,
                              N, T, t, weights_sum, depth, image, weights):
    for a, w in ((sigma_coarse, "sigma_coarse"), (z_all, "z_all"), (nears, "nears"),
                 (fars, "fars"), (sample_dist, "sample_dist"), (weights_sum, "weights_sum"),
                 (depth, "depth"), (image, "image"), (weights, "weights")):
        _f32_only(a, w)
    _f32_opt(sigma_new, "sigma_new")
    _i32_opt(order, "order")
    rd = _rgbs_code(rgbs, "rgbs")
    call("dfhip_composite_uniform_forward", rd, ptr(sigma_coarse), ptr(sigma_new), ptr(order),
         ptr(z_all), ptr(nears), ptr(fars), ptr(sample_dist), ptr(rgbs), N, T, t,
         ptr(weights_sum), ptr(depth), ptr(image), ptr(weights), stream())


def composite_uniform_backward(grad_weights_sum, grad_depth, grad_image, sigma_coarse, sigma_new,
                               order, z_all, nears, fars, sample_dist, rgbs, N, T, t,
                               grad_sigma_coarse, grad_sigma_new, grad_rgbs):
    for a, w in ((sigma_coarse, "sigma_coarse"), (z_all, "z_all"), (nears, "nears"),
                 (fars, "fars"), (sample_dist, "sample_dist"),
                 (grad_sigma_coarse, "grad_sigma_coarse")):
        _f32_only(a, w)
    for a, w in ((grad_weights_sum, "grad_weights_sum"), (grad_depth, "grad_depth"),
                 (grad_image, "grad_image"), (sigma_new, "sigma_new"),
                 (grad_sigma_new, "grad_sigma_new")):
        _f32_opt(a, w)
    _i32_opt(order, "order")
    rd = _rgbs_code(rgbs, "rgbs")
    if grad_rgbs is not None:
        checked(grad_rgbs, "grad_rgbs")
        if grad_rgbs.dtype != rgbs.dtype:
            raise RuntimeError("grad_rgbs must have the dtype of rgbs")
    call("dfhip_composite_uniform_backward", rd, ptr(grad_weights_sum), ptr(grad_depth),
         ptr(grad_image), ptr(sigma_coarse), ptr(sigma_new), ptr(order), ptr(z_all), ptr(nears),
         ptr(fars), ptr(sample_dist), ptr(rgbs), N, T, t, ptr(grad_sigma_coarse),
         ptr(grad_sigma_new), ptr(grad_rgbs), stream())
