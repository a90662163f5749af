"""The SDS train step of the DVGO backbone (nerf/network_dvgo.py) as a fixed
sequence of launches, captured once per (shading, resolution) in a HIP graph
by nerf/graph.py: the counterpart of nerf/native_step.py for a frozen density.

The eager autograd step of this backbone pays a host synchronisation in the
march (`step_counter[0].item()`), about fifty launches and autograd's
bookkeeping for very little arithmetic.  With the density and feature volumes
frozen the step is short: no gradient reaches sigma, so the entropy and
orientation terms reach no parameter (Trainer.backward_only), and the whole
backward is grad_colour = w_i g_ray -> the shading factor -> rgbnet, plus
(1 - weights_sum) g -> bg_net.

  prologue (eager, one launch; csrc/step.hip): camera rays from the host
      pose, near / far, march noise, the synthetic SDS gradient at pred_rgb,
      step counter = 0, the learning rates; shaded steps: the light direction
  graph:
    1. march count / emit, the sample count stays on the device
    2. dfhip_voxel_field_forward_dev (textureless: the density branch only,
       rgbnet is not evaluated); shaded: dfhip_voxel_shade_train_forward
       (closed-form normal, lambertian factor, colour, orientation term)
    3. bg = model.background(rays_d) through torch under fp16 autocast (a
       LayerNorm ResBlock MLP the native 39 -> 64 -> 3 head does not describe);
       its autograd is recorded in the graph
    4. dfhip_composite_rays_train_forward_mixed (f16 colours)
    5. dfhip_ray_head_forward with bg_color = bg.float()
    6. dfhip_entropy_forward: the loss value (+ lambda_orient * orient)
    7. dfhip_ray_head_backward with grad_bg
    8. dfhip_composite_rays_train_backward_mixed
    9. bg's backward, copied into the persistent gradient buffers (one launch)
   10. lambertian: dfhip_voxel_shade_train_backward (grad_albedo = f16(g lam))
   11. dfhip_voxel_field_backward_dev into the persistent rgbnet gradients
   12. GradScaler + Adam with device learning rates (nerf/optim.py)

The SDS gradient is not scaled and the loss scale enters nowhere else: no
scaled term reaches a parameter.  A textureless step gives rgbnet no gradient:
its parameters, Adam moments and step counts stay untouched, as torch's Adam
leaves a parameter without a gradient (their .grad is None while the
optimizer's closure is built, and after every such step).

Per-sample buffers hold N * max_steps rows, as NativeAlbedoStep's do; the
field backward's neuron-major scratch is capacity-sized too (616 rows x 2
bytes per sample, include/dfhip.h).  Given the same rays, noise and SDS
gradient, the live count, weights_sum and every parameter gradient equal the
autograd step's bit for bit (tests/test_gpu_voxel_native_step.py); pred_rgb
differs by at most the head's one contracted multiply-add.  One step in 128
is not the autograd step's to the bit: on a live count m that is a multiple of
128 the march's slice holds m + 128 rows (the reference's rule always adds),
the native step's row count is m, so the orientation mean divides by m and
the last backward chunk splits its equal terms differently.
"""
import ctypes

import numpy as np
import torch

import _dfhip
import _raymarching
import _voxelfield
from _dfhip import call, ptr, stream

from . import voxel_field as _vf

SHADINGS = {"albedo": 0, "textureless": 1, "lambertian": 2}
ALIGN = 128  # march_rays_train's slice: the rows the autograd step's means and sums run over


def serves(model):
    """True for the DVGO backbone, whose steps are graphed as NativeVoxelStep
    or not at all."""
    from .network_dvgo import NeRFNetwork
    return isinstance(model, NeRFNetwork)


def eligible(trainer, shading):
    """True when NativeVoxelStep reproduces trainer.train_step for `shading`:
    the native voxel field applies to the model (width-128 depth-3 rgbnet,
    dim0 <= 96, fused_field), fp16 and cuda_ray, the InjectedSDS guidance, one
    fused backward, no opacity or smoothness term (both reach the frozen
    density only through terms this step does not form), a background
    network, one process, f32 parameters on the GPU.  Anything else (bf16,
    data parallel, a deeper rgbnet, fused_field False) keeps the eager step."""
    from .sd import InjectedSDS
    m, opt = trainer.model, trainer.opt
    if shading not in SHADINGS or not serves(m):
        return False
    if not isinstance(trainer.guidance, InjectedSDS) or not trainer.fused_backward:
        return False
    if not (trainer.fp16 and m.cuda_ray) or getattr(trainer, "bf16", False):
        return False
    if opt.lambda_opacity != 0 or opt.lambda_smooth != 0:
        return False
    if trainer.world_size != 1:
        return False
    if not (m.bg_radius > 0) or getattr(m, "bg_net", None) is None:
        return False
    device = _trained_device(m)
    return device is not None and _vf.model_eligible(m, device)


def _trained_device(model):
    """The device of the trained parameters when all are f32 on one GPU, else None."""
    trained = [p for p in model.parameters() if p.requires_grad]
    if not trained or not all(p.is_cuda and p.dtype == torch.float32 and
                              p.device == trained[0].device for p in trained):
        return None
    return trained[0].device


class NativeVoxelStep:
    """Buffers and launches of one DVGO train step at resolution H x W for
    shading "albedo", "textureless" or "lambertian" (with the ambient ratio)."""

    def __init__(self, trainer, H, W, shading="albedo", ratio=1.0):
        self.trainer = trainer
        m, opt = trainer.model, trainer.opt
        dev = trainer.device
        self.H, self.W = int(H), int(W)
        N = self.N = self.H * self.W
        self.max_steps = int(opt.max_steps)
        cap = self.cap = N * self.max_steps
        self.shading, self.ratio = shading, float(ratio)
        self.shade_code = SHADINGS[shading]
        self.colour = self.shade_code != 1  # rgbnet is evaluated and trained
        self.lam_orient = float(opt.lambda_orient) if self.shade_code else 0.0
        self.lam = float(opt.lambda_entropy)
        self.dt_gamma = float(opt.dt_gamma)
        f32 = dict(device=dev, dtype=torch.float32)
        f16 = dict(device=dev, dtype=torch.float16)
        i32 = dict(device=dev, dtype=torch.int32)
        # prologue outputs (graph inputs)
        self.rays_o = torch.empty(N, 3, **f32)
        self.rays_d = torch.empty(N, 3, **f32)
        self.nears = torch.empty(N, **f32)
        self.fars = torch.empty(N, **f32)
        self.noises = torch.empty(N, **f32)
        self.g_image = torch.empty(3, N, **f32)  # d loss / d pred_rgb (channel-major)
        self.counter = torch.zeros(2, **i32)
        self.m_dev = self.counter[:1]
        self.aabb = np.ascontiguousarray(m.aabb_train.detach().float().cpu().numpy())
        g = trainer.guidance
        self.alphas = g.alphas.detach().float().contiguous()
        self.t_range = (int(g.min_step), int(g.max_step))
        # march
        self.rays = torch.empty(N, 3, **i32)
        self.block_sums = torch.empty(_raymarching.march_rays_train_scratch_ints(N), **i32)
        self.stage = torch.empty(_raymarching.march_rays_train_stage_floats(N, self.max_steps),
                                 **f32)
        self.xyzs = torch.empty(cap, 3, **f32)
        self.dirs = torch.empty(cap, 3, **f32) if self.shade_code else None
        self.deltas = torch.empty(cap, 2, **f32)
        # field
        self.rgbnet = _vf.rgbnet_params(m.main_net.rgbnet)
        self.sigma = torch.empty(cap, **f32)
        self.albedo = torch.empty(cap, 3, **f16) if self.colour else None
        self.rgb = self.albedo  # what the compositing reads
        if self.shade_code:
            self.light = torch.empty(3, **f32)
            self.normal = torch.empty(cap, 3, **f32)
            self.lambert = torch.empty(cap, **f16)
            self.color = torch.empty(cap, 3, **f16)
            self.orient = torch.zeros(1, **f32)
            self.orient_partial = torch.empty(_voxelfield.shade_partial_doubles(cap), device=dev,
                                              dtype=torch.float64)
            self.rgb = self.color
        # compositing + head
        self.ws = torch.empty(N, **f32)
        self.depth = torch.empty(N, **f32)
        self.image = torch.empty(N, 3, **f32)
        self.out_image = torch.empty(3, N, **f32)
        self.out_depth = torch.empty(N, **f32)
        self.mask = torch.empty(N, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros((), **f32)
        # backward
        self.grad_image = torch.empty(N, 3, **f32)
        self.grad_ws = torch.empty(N, **f32)
        self.grad_bg = torch.empty(N, 3, **f32)
        self.grad_sigma = torch.empty(cap, **f32)  # written by the compositing, read by nobody
        self.grad_color = torch.empty(cap, 3, **f16)
        self.grad_albedo = (torch.empty(cap, 3, **f16) if self.shade_code == 2
                            else self.grad_color)
        self.scratch_bytes = (_voxelfield.backward_dev_scratch_bytes(cap, m.main_net.dim0)
                              if self.colour else 0)
        self.scratch = torch.empty(max(self.scratch_bytes, 16), dtype=torch.uint8, device=dev)
        sc = trainer.scaler
        if sc.is_enabled() and sc._scale is None:
            sc._lazy_init_scale_growth_tracker(dev)  # what scaler.scale() does on first use
        # gradients live in persistent buffers, written in place every step
        from .utils import flat_grad_bucket_
        self.grad_bucket = flat_grad_bucket_(m.parameters())
        self.bg_params = list(m.bg_net.parameters())
        self.bg_grads = [p.grad for p in self.bg_params]
        self.rgb_grads = [p.grad for p in self.rgbnet]
        self.params = [p for p in m.parameters() if p.requires_grad]
        # a textureless step leaves rgbnet without a gradient
        skip = set() if self.colour else {id(p) for p in self.rgbnet}
        self.grads = [(p, None if id(p) in skip else p.grad) for p in self.params]
        self.reattach()
        self.n_params = sum(p.numel() for p, g in self.grads if g is not None)
        # optimizer inside the graph (attach_optimizer): the learning rates
        # live on the device, written by the prologue launch every step
        self.lr_dev = torch.zeros(8, **f32)
        self.row_dev = torch.zeros(1, **i32)
        self.adam = None
        self._lr_source = None
        self.found_inf = None
        self.stores_live_count = False
        self.live_rows = None
        self.dp_world = None  # (GraphedTrainStep reads it: no exchange in this step)

    # ------------------------------------------------------------ optimizer
    def attach_optimizer(self, native_adam, data_parallel=False):
        """Run GradScaler + Adam (nerf/optim.py NativeAdamAmp) as the step's
        last launches, with device learning rates.  The closure is built while
        the parameters hold this step's gradients: a textureless step's leaves
        rgbnet out.  No gradient writer reports a non-finite value itself: the
        optimizer's own check reads them all (covered_mask 0).
        trainer.store_live_count: the finalize launch stores the sample count
        into model.step_counter."""
        if data_parallel:
            raise RuntimeError("NativeVoxelStep: one process only")
        t = self.trainer
        self._lr_source = native_adam.group_lrs
        tail = None
        if getattr(t, "store_live_count", True):
            self.live_rows = t.model.step_counter
            tail = dict(live=self.counter, live_rows=self.live_rows, live_row=self.row_dev)
            self.stores_live_count = True
        self.reattach()
        self.adam = native_adam.device_lr_launch(self.lr_dev, tail=tail)
        self.found_inf = native_adam.found_inf

    def optimizer_tail(self):
        with _dfhip.timed("adam", 28 * self.n_params):
            self.adam()

    def clear_found_inf(self):
        if self.found_inf is not None:
            self.found_inf.zero_()

    def embedding_backward(self):
        """No embedding here (GraphedTrainStep's capture calls it)."""

    def reattach(self):
        for p, g in self.grads:
            p.grad = g

    def served(self):
        """Count one train step served (GraphedTrainStep: every replay and
        every eager twin of one)."""
        self.trainer.model.native_step_calls += 1

    # ------------------------------------------------------------ per step
    def prologue(self, pose, intrinsics, seed, step, row=0):
        """Rays, near / far, noise, the SDS gradient, counter reset and the
        learning rates from the host pose of this step (one eager launch);
        shaded: the light direction (renderer.py:462-464), same (seed, step)."""
        host = np.ascontiguousarray(np.asarray(pose, dtype=np.float32).reshape(-1, 4, 4)[0, :3, :4])
        fx, fy, cx, cy = (float(v) for v in intrinsics)
        lo, hi = self.t_range
        lrs = self._lr_source() if self._lr_source is not None else []
        lr_host = (ctypes.c_float * max(1, len(lrs)))(*lrs)
        N = self.N
        with _dfhip.timed("step_prologue", N * (24 + 8 + 4 + 12)):
            call("dfhip_train_step_prologue_row", host.ctypes.data, fx, fy, cx, cy, self.H,
                 self.W, self.aabb.ctypes.data, 0.2, int(seed) & 0xFFFFFFFFFFFFFFFF,
                 int(step) & 0xFFFFFFFFFFFFFFFF, 1, ptr(self.alphas), lo, hi, ptr(self.rays_o),
                 ptr(self.rays_d), ptr(self.nears), ptr(self.fars), ptr(self.noises),
                 None, ptr(self.g_image), ptr(self.counter), lr_host, len(lrs),
                 ptr(self.lr_dev), int(row), ptr(self.row_dev), stream())
        if self.shade_code:
            call("dfhip_shading_light", ptr(self.rays_o), int(seed) & 0xFFFFFFFFFFFFFFFF,
                 int(step) & 0xFFFFFFFFFFFFFFFF, ptr(self.light), stream())

    def body(self):
        """Forward and backward down to the parameter gradients (the
        graph-captured part).  Returns the loss tensor."""
        m = self.trainer.model
        net = m.main_net
        N, cap, md, T = self.N, self.cap, self.m_dev, _dfhip.timed
        vol, _ = _vf.volume(m)
        bound, shift = float(m.bound), float(net.act_shift)
        ws = [p.detach() for p in self.rgbnet]
        # 1. march (raymarching.py:161-235, device count)
        with T("march_rays_train_count", 48 * N + m.density_bitfield.numel(), md, 20):
            _raymarching.march_rays_train_count_staged(
                self.rays_o, self.rays_d, m.density_bitfield, m.bound, self.dt_gamma,
                self.max_steps, N, m.cascade, m.grid_size, self.nears, self.fars, self.rays,
                self.counter, self.noises, self.block_sums, self.stage)
        with T("march_rays_train_emit", 24 * N, md, 52 if self.dirs is not None else 40):
            _raymarching.march_rays_train_emit_staged(
                self.rays_d, self.max_steps, N, cap, self.xyzs, self.dirs, self.deltas,
                self.rays, self.block_sums, 0, self.stage)
        # 2. field (network_dvgo.py common_forward) and shading (forward)
        with T("voxel_field_forward", 0, md, 12 + 4 + (6 if self.colour else 0)):
            _voxelfield.field_forward_dev(self.xyzs, vol, bound, shift, ws if self.colour else None,
                                          self.sigma, self.albedo, md, ALIGN)
        if self.shade_code:
            with T("voxel_shade_forward", 0, md, 24 + (6 if self.colour else 0) + 12 + 2 + 6):
                _voxelfield.shade_train_forward(
                    self.xyzs, self.dirs, vol, bound, shift, self.albedo, self.light, self.ratio,
                    self.shade_code, md, ALIGN, self.normal, self.lambert, self.color,
                    self.orient_partial, self.orient)
        # 3. the background network through torch (its autograd is recorded)
        with torch.enable_grad(), torch.autocast("cuda", dtype=torch.float16):
            bg = m.background(self.rays_d)
            bg32 = bg.float()
        bg_color = bg32.detach().contiguous()
        # 4.-6. compositing, ray head, entropy term
        with T("composite_rays_train_forward", 32 * N, md, 4 + 6 + 8):
            _raymarching.composite_rays_train_forward_mixed(
                self.sigma, self.rgb, self.deltas, self.rays, cap, N, 1e-4, self.ws, self.depth,
                self.image)
        with T("ray_head_forward", 72 * N):
            call("dfhip_ray_head_forward", N, ptr(self.ws), ptr(self.depth), ptr(self.image),
                 ptr(self.rays_d), ptr(self.nears), ptr(self.fars), None, None, None, None,
                 ptr(bg_color), ptr(self.out_image), ptr(self.out_depth), ptr(self.mask),
                 stream())
        if self.lam > 0:
            call("dfhip_entropy_forward", N, ptr(self.ws), self.lam, ptr(self.loss), stream())
        self._add_orient_loss()
        # 7.-8. ray head and compositing backward (the SDS gradient, unscaled)
        with T("ray_head_backward", 60 * N):
            call("dfhip_ray_head_backward", N, ptr(self.g_image), ptr(self.ws), ptr(self.rays_d),
                 None, None, None, None, ptr(bg_color), ptr(self.grad_image), ptr(self.grad_ws),
                 ptr(self.grad_bg), None, None, None, None, None, stream())
        with T("composite_rays_train_backward", 44 * N, md, 4 + 6 + 8 + 4 + 6):
            _raymarching.composite_rays_train_backward_mixed(
                self.grad_ws, self.grad_image, self.sigma, self.rgb, self.deltas, self.rays,
                self.ws, self.image, cap, N, 1e-4, self.grad_sigma, self.grad_color, False)
        # 9. (1 - weights_sum) g -> bg_net
        got = torch.autograd.grad([bg32], self.bg_params, [self.grad_bg])
        torch._foreach_copy_(self.bg_grads, list(got))
        # 10.-11. grad_colour -> the shading factor -> rgbnet
        if self.shade_code == 2:
            with T("voxel_shade_backward", 0, md, 6 + 2 + 6):
                _voxelfield.shade_train_backward(self.grad_color, self.lambert, self.shade_code,
                                                 md, ALIGN, self.grad_albedo)
        if self.colour:
            with T("voxel_field_backward", 4 * self.n_params, md, 12 + 6 + 2 * 2 * 616):
                _voxelfield.field_backward_dev(self.xyzs, vol, bound, ws, self.grad_albedo,
                                               self.rgb_grads, md, ALIGN, scratch=self.scratch)
        return self.loss

    def _add_orient_loss(self):
        """loss (+)= lambda_orient * orient (utils.py:398-400); without the
        entropy launch the loss is written fresh, so no step adds onto the last."""
        if self.lam_orient > 0:
            if self.lam > 0:
                self.loss.add_(self.orient[0], alpha=self.lam_orient)
            else:
                torch.mul(self.orient[0], self.lam_orient, out=self.loss)
        elif self.lam <= 0:
            self.loss.zero_()
