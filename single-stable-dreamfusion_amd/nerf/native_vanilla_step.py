"""The albedo SDS train step of the vanilla backbone (nerf/network.py) as a
fixed sequence of launches, captured once per resolution in a HIP graph by
nerf/graph.py: the counterpart of nerf/native_step.py (grid backbone) and
nerf/native_voxel_step.py (DVGO backbone) for the frequency-encoded ResMLP
field of csrc/resmlp.hip.

The eager autograd step of this backbone pays a host synchronisation in the
march (`step_counter[0].item()`), about fifty launches and autograd's
bookkeeping around the two fused field launches; the autograd-form capture of
Trainer(graph_step=True) is worse: its device-count march sends the field down
the torch path on all N * max_steps capacity rows.  Here:

  prologue (eager, one launch; csrc/step.hip): camera rays from the host
      pose, near / far, march noise, the synthetic SDS gradient at pred_rgb,
      step counter = 0, the learning rates, the step_counter row
  graph:
    1. march count / emit, the sample count stays on the device
    2. dfhip_resmlp_field_forward_dev: sigma f32, albedo f16
    3. bg = model.background(rays_d) through torch under fp16 autocast (a
       LayerNorm ResBlock MLP the native 39 -> 64 -> 3 head does not describe);
       its autograd is recorded in the graph
    4. dfhip_composite_rays_train_forward_mixed (f16 colours)
    5. dfhip_ray_head_forward with bg_color = bg.float()
    6. the loss value: dfhip_entropy_forward (lambda_entropy > 0), then
       dfhip_opacity_forward (lambda_opacity > 0; adding onto the entropy
       value when that was written); zeroed when neither applies
    7. the gradient of the weights sum (below)
    8. dfhip_composite_rays_train_backward_mixed: grad_sigma f32, grad_color f16
    9. bg's backward from grad_bg in the autograd step's channel-major layout,
       copied into the persistent gradient buffers (one launch)
   10. dfhip_resmlp_field_backward_dev into sigma_net's persistent gradients
   11. GradScaler + Adam with device learning rates (nerf/optim.py), where
       the native Adam takes the optimizer (Trainer.native_adam()).  It walks
       at most 24 tensors and this model has 26 (19 of sigma_net, 7 of
       bg_net), so today the graph ends at the gradients and the trainer's
       own optimizer step follows each replay, as after any graph without
       one (GraphedTrainStep.optimizer_in_graph)

Unlike the DVGO step's frozen density, sigma is trained: grad_sigma of the
compositing backward feeds the field backward, and the entropy and opacity
terms reach parameters, with the GradScaler scale as their upstream gradient.
The SDS gradient stays unscaled: the reference quirk Trainer.backward_only
keeps (nerf/native_step.py).

Step 7 follows autograd's summation order.  weights_sum has two consumers,
the ray head and the reshaped pred_ws the regularisers read; autograd sums
the regularisers' gradients at pred_ws first (entropy, the later node, then
opacity), then adds the head's.  One regulariser: dfhip_ray_head_backward_
entropy, or dfhip_ray_head_backward then dfhip_opacity_backward_accumulate
(two terms, either order gives the same bits).  Both: dfhip_ray_head_backward,
dfhip_entropy_backward into a second buffer, dfhip_opacity_backward_accumulate
onto that, and one add of the two buffers: head + (entropy + opacity).

Shaded steps need the parameter gradient of the MLP's input gradient (a
second-order backward) and stay on the eager autograd step.

Per-sample buffers hold N * max_steps rows; the field backward's scratch is
capacity-sized too (5856 bytes per sample, include/dfhip.h).  Given the same
rays, noise and SDS gradient, the live count, weights_sum and every parameter
gradient equal the autograd step's bit for bit
(tests/test_gpu_vanilla_native_step.py); pred_rgb differs by at most the
head's one contracted multiply-add.  One step in 128 is not the autograd
step's to the bit, as nerf/native_voxel_step.py explains: on a live count m
that is a multiple of 128 the march's slice holds m + 128 rows, the native
step's row count is m, and the last backward chunk splits its terms
differently.
"""
import ctypes

import numpy as np
import torch

import _dfhip
import _raymarching
import _resmlp
from _dfhip import call, ptr, stream

from . import vanilla_field as _vf

ALIGN = 128  # march_rays_train's slice: the rows the autograd step's field backward runs over


def serves(model):
    """True for the vanilla backbone (nerf/network.py)."""
    from .network import NeRFNetwork
    return isinstance(model, NeRFNetwork)


def model_eligible(m, device):
    """vanilla_field.eligible's conditions on the model alone (the autocast
    state is the step's own): fused_field, FreqEncoder(3, 6), the reference's
    19 sigma_net tensors as f32 on `device`."""
    from freqencoder import FreqEncoder
    if not getattr(m, "fused_field", False):
        return False
    enc = getattr(m, "encoder", None)
    if not isinstance(enc, FreqEncoder) or enc.input_dim != 3 or enc.degree != 6:
        return False
    ps = _vf.sigma_net_params(m.sigma_net)
    if [tuple(p.shape) for p in ps] != list(_resmlp.SHAPES):
        return False
    names = [n for n, _ in m.sigma_net.named_parameters()]
    if names[:5] != ["net.0.dense.weight", "net.0.dense.bias", "net.0.norm.weight",
                     "net.0.norm.bias", "net.0.skip.weight"]:
        return False
    return all(p.dtype == torch.float32 and p.device == device for p in ps)


def eligible(trainer, shading):
    """True when NativeVanillaStep reproduces trainer.train_step for `shading`:
    the albedo shading, the native vanilla field applies to the model
    (fused_field, the reference's shape), fp16 and cuda_ray, the InjectedSDS
    guidance, one fused backward, a background network, one process, f32
    parameters on one GPU.  lambda_opacity and lambda_entropy may each be zero
    or positive; lambda_orient and lambda_smooth play no part in an albedo
    step.  Anything else (shaded steps, bf16, data parallel, another width,
    fused_field False) keeps today's path."""
    from .sd import InjectedSDS
    m, opt = trainer.model, trainer.opt
    if shading != "albedo" or not serves(m):
        return False
    if not isinstance(trainer.guidance, InjectedSDS) or not trainer.fused_backward:
        return False
    if not (trainer.fp16 and m.cuda_ray) or getattr(trainer, "bf16", False):
        return False
    if opt.lambda_opacity < 0 or opt.lambda_entropy < 0:
        return False
    if trainer.world_size != 1:
        return False
    if not (m.bg_radius > 0) or getattr(m, "bg_net", None) is None:
        return False
    device = _trained_device(m)
    return device is not None and model_eligible(m, device)


def _trained_device(model):
    """The device of the trained parameters when all are f32 on one GPU, else None."""
    trained = [p for p in model.parameters() if p.requires_grad]
    if not trained or not all(p.is_cuda and p.dtype == torch.float32 and
                              p.device == trained[0].device for p in trained):
        return None
    return trained[0].device


class NativeVanillaStep:
    """Buffers and launches of one vanilla-backbone albedo train step at
    resolution H x W."""

    def __init__(self, trainer, H, W, shading="albedo", ratio=1.0):
        if shading != "albedo":
            raise RuntimeError("NativeVanillaStep: the albedo step only")
        self.trainer = trainer
        m, opt = trainer.model, trainer.opt
        dev = trainer.device
        self.H, self.W = int(H), int(W)
        N = self.N = self.H * self.W
        self.max_steps = int(opt.max_steps)
        cap = self.cap = N * self.max_steps
        self.shading, self.ratio = shading, float(ratio)
        self.lam = float(opt.lambda_entropy)
        self.lam_opacity = float(opt.lambda_opacity)
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
        self.deltas = torch.empty(cap, 2, **f32)
        # field
        self.sigma_net = _vf.sigma_net_params(m.sigma_net)
        self.sigma = torch.empty(cap, **f32)
        self.albedo = torch.empty(cap, 3, **f16)
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
        # the regularisers' own sum when both apply (autograd's order, see above)
        self.grad_ws_reg = torch.empty(N, **f32) if self.lam > 0 and self.lam_opacity > 0 else None
        self.grad_bg = torch.empty(N, 3, **f32)
        # the same values channel-major, the layout autograd hands bg_net (body, step 9)
        self.grad_bg_cm = torch.empty(3, N, **f32)
        self.grad_sigma = torch.empty(cap, **f32)
        self.grad_color = torch.empty(cap, 3, **f16)
        self.scratch_bytes = _resmlp.backward_dev_scratch_bytes(cap)
        self.scratch = torch.empty(max(self.scratch_bytes, 16), dtype=torch.uint8, device=dev)
        sc = trainer.scaler
        if sc.is_enabled() and sc._scale is None:
            sc._lazy_init_scale_growth_tracker(dev)  # what scaler.scale() does on first use
        self._ones = torch.ones(1, **f32)  # upstream gradient of the loss without a scaler
        # gradients live in persistent buffers, written in place every step
        from .utils import flat_grad_bucket_
        self.grad_bucket = flat_grad_bucket_(m.parameters())
        self.bg_params = list(m.bg_net.parameters())
        self.bg_grads = [p.grad for p in self.bg_params]
        self.sigma_grads = [p.grad for p in self.sigma_net]
        self.params = [p for p in m.parameters() if p.requires_grad]
        self.grads = [(p, p.grad) for p in self.params]
        self.reattach()
        self.n_params = sum(p.numel() for p in self.params)
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
        last launches, with device learning rates.  No gradient writer reports
        a non-finite value itself: the optimizer's own check reads them all
        (covered_mask 0).  trainer.store_live_count: the finalize launch stores
        the sample count into model.step_counter."""
        if data_parallel:
            raise RuntimeError("NativeVanillaStep: one process only")
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
        """Rays, near / far, noise, the SDS gradient, counter reset, the
        learning rates and the step_counter row from the host pose of this
        step (one eager launch)."""
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

    def body(self):
        """Forward and backward down to the parameter gradients (the
        graph-captured part).  Returns the loss tensor."""
        m = self.trainer.model
        N, cap, md, T = self.N, self.cap, self.m_dev, _dfhip.timed
        sc = self.trainer.scaler
        scale = sc._scale if sc.is_enabled() else self._ones
        ws = [p.detach() for p in self.sigma_net]
        # 1. march (raymarching.py:161-235, device count)
        with T("march_rays_train_count", 48 * N + m.density_bitfield.numel(), md, 20):
            _raymarching.march_rays_train_count_staged(
                self.rays_o, self.rays_d, m.density_bitfield, m.bound, self.dt_gamma,
                self.max_steps, N, m.cascade, m.grid_size, self.nears, self.fars, self.rays,
                self.counter, self.noises, self.block_sums, self.stage)
        with T("march_rays_train_emit", 24 * N, md, 40):
            _raymarching.march_rays_train_emit_staged(
                self.rays_d, self.max_steps, N, cap, self.xyzs, None, self.deltas,
                self.rays, self.block_sums, 0, self.stage)
        # 2. field (network.py common_forward)
        with T("resmlp_field_forward", 4 * 61188, md, 12 + 4 + 6):
            _resmlp.field_forward_dev(self.xyzs, ws, self.sigma, self.albedo, md, ALIGN)
        # 3. the background network through torch (its autograd is recorded)
        with torch.enable_grad(), torch.autocast("cuda", dtype=torch.float16):
            bg = m.background(self.rays_d)
            bg32 = bg.float()
        bg_color = bg32.detach().contiguous()
        # 4.-6. compositing, ray head, the regularisers' loss value
        with T("composite_rays_train_forward", 32 * N, md, 4 + 6 + 8):
            _raymarching.composite_rays_train_forward_mixed(
                self.sigma, self.albedo, self.deltas, self.rays, cap, N, 1e-4, self.ws,
                self.depth, self.image)
        with T("ray_head_forward", 72 * N):
            call("dfhip_ray_head_forward", N, ptr(self.ws), ptr(self.depth), ptr(self.image),
                 ptr(self.rays_d), ptr(self.nears), ptr(self.fars), None, None, None, None,
                 ptr(bg_color), ptr(self.out_image), ptr(self.out_depth), ptr(self.mask),
                 stream())
        if self.lam > 0:
            with T("entropy_forward", 4 * N):
                call("dfhip_entropy_forward", N, ptr(self.ws), self.lam, ptr(self.loss), stream())
        if self.lam_opacity > 0:
            with T("opacity_forward", 4 * N):
                call("dfhip_opacity_forward", N, ptr(self.ws), self.lam_opacity, ptr(self.loss),
                     int(self.lam > 0), stream())
        if self.lam <= 0 and self.lam_opacity <= 0:
            self.loss.zero_()  # no step adds onto the last
        # 7. d / d weights_sum: the SDS gradient (unscaled) through the head,
        # the regularisers with the scale, summed in autograd's order
        head = (N, ptr(self.g_image), ptr(self.ws), ptr(self.rays_d), None, None, None, None,
                ptr(bg_color), ptr(self.grad_image), ptr(self.grad_ws), ptr(self.grad_bg), None,
                None, None, None, None)
        with T("ray_head_backward", 60 * N):
            if self.lam > 0 and self.grad_ws_reg is None:
                call("dfhip_ray_head_backward_entropy", *head, ptr(scale), self.lam, stream())
            else:
                call("dfhip_ray_head_backward", *head, stream())
        if self.grad_ws_reg is not None:
            with T("regulariser_backward", 20 * N):
                call("dfhip_entropy_backward", N, ptr(self.ws), ptr(scale), self.lam,
                     ptr(self.grad_ws_reg), stream())
                call("dfhip_opacity_backward_accumulate", N, ptr(self.ws), ptr(scale),
                     self.lam_opacity, ptr(self.grad_ws_reg), stream())
                self.grad_ws.add_(self.grad_ws_reg)
        elif self.lam_opacity > 0:
            with T("opacity_backward", 12 * N):
                call("dfhip_opacity_backward_accumulate", N, ptr(self.ws), ptr(scale),
                     self.lam_opacity, ptr(self.grad_ws), stream())
        # 8. compositing backward
        with T("composite_rays_train_backward", 44 * N, md, 4 + 6 + 8 + 4 + 6):
            _raymarching.composite_rays_train_backward_mixed(
                self.grad_ws, self.grad_image, self.sigma, self.albedo, self.deltas, self.rays,
                self.ws, self.image, cap, N, 1e-4, self.grad_sigma, self.grad_color, False)
        # 9. (1 - weights_sum) g -> bg_net.  In the autograd step this gradient
        # descends from the channel-major pred_rgb, so bg_net's backward sees it
        # with strides (1, N) and its last Linear's weight-gradient GEMM runs
        # untransposed; a row-major gradient takes another GEMM kernel, whose
        # f32 sums round a few f16 results the other way.  Same layout here.
        self.grad_bg_cm.copy_(self.grad_bg.t())
        got = torch.autograd.grad([bg32], self.bg_params, [self.grad_bg_cm.t()])
        torch._foreach_copy_(self.bg_grads, list(got))
        # 10. grad_sigma, grad_colour -> sigma_net
        with T("resmlp_field_backward", 8 * 61188, md, 12 + 4 + 6 + 2 * 5856):
            _resmlp.field_backward_dev(self.xyzs, ws, self.grad_sigma, self.grad_color,
                                       self.sigma_grads, md, ALIGN, scratch=self.scratch)
        return self.loss
