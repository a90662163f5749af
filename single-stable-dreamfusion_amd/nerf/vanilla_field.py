"""Fused vanilla field: frequency encoding + residual MLP + density / albedo
heads as ONE autograd node on the native kernels (csrc/resmlp.hip), the
native path of nerf/network.py's common_forward (reference
nerf/network.py:104-115) and of its autograd normal (:135-146).

Served: fp16 autocast on CUDA, the reference's shape (FreqEncoder(3, 6),
39 -> 128 x4 -> 4) with f32 parameters.  Anything else (f32, bf16, other
widths) runs the module's torch path.  The node returns no gradient for the
positions: they are leaves in both render paths.  input_gradient is the
first-order input gradient without a graph; the autograd normal of a
grad-enabled call does carry one (through the Gaussian blob and trunc_exp's
backward), so the module uses input_gradient for no-grad calls only.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import _resmlp


def sigma_net_params(sigma_net):
    """The 19 tensors of sigma_net in state_dict order (the packed order of
    include/dfhip.h)."""
    return list(sigma_net.parameters())


def eligible(net, x):
    from freqencoder import FreqEncoder
    if not getattr(net, "fused_field", False):
        return False
    if not (x.is_cuda and torch.is_autocast_enabled("cuda")):
        return False
    if torch.get_autocast_dtype("cuda") != torch.float16:
        return False
    enc = net.encoder
    if not isinstance(enc, FreqEncoder) or enc.input_dim != 3 or enc.degree != 6:
        return False
    ps = sigma_net_params(net.sigma_net)
    if [tuple(p.shape) for p in ps] != list(_resmlp.SHAPES):
        return False
    names = [n for n, _ in net.sigma_net.named_parameters()]
    if names[:5] != ["net.0.dense.weight", "net.0.dense.bias", "net.0.norm.weight",
                     "net.0.norm.bias", "net.0.skip.weight"]:
        return False
    return all(p.dtype == torch.float32 and p.device == x.device for p in ps)


class _VanillaField(Function):
    @staticmethod
    def forward(ctx, x, *params):
        """x [M, 3] -> sigma [M] f32, albedo [M, 3] f16."""
        x = x.detach().contiguous().float()
        M = x.shape[0]
        ws = [p.detach().contiguous() for p in params]
        sigma = torch.empty(M, device=x.device, dtype=torch.float32)
        albedo = torch.empty(M, 3, device=x.device, dtype=torch.float16)
        _resmlp.field_forward(x, ws, sigma, albedo)
        ctx.save_for_backward(x, *ws)
        return sigma, albedo

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sigma, grad_albedo):
        x, *ws = ctx.saved_tensors
        M, dev = x.shape[0], x.device
        if grad_sigma is None:
            grad_sigma = torch.zeros(M, device=dev)
        if grad_albedo is None:
            grad_albedo = torch.zeros(M, 3, device=dev, dtype=torch.float16)
        grad_sigma = grad_sigma.float().contiguous()
        if grad_albedo.dtype not in (torch.float16, torch.float32):
            grad_albedo = grad_albedo.float()
        grads = [torch.empty_like(w) for w in ws]
        _resmlp.field_backward(x, ws, grad_sigma, grad_albedo.contiguous(), grads=grads)
        return (None, *grads)


def vanilla_field(net, x):
    """sigma [M] f32, albedo [M, 3] f16 of positions x [M, 3] on the native node."""
    net.native_calls += 1
    return _VanillaField.apply(x.reshape(-1, 3), *sigma_net_params(net.sigma_net))


class InferField:
    """What NeRFRenderer._infer_fused needs to render this backbone's albedo
    frames in one persistent launch (csrc/resmlprender.hip): sigma_net's 19
    f32 parameters themselves, taken when the frame is launched and read by
    the kernel, so an optimizer step between two frames (torch's or the native
    Adam, both of which write the parameters in place) is seen by the next
    frame with no cast and no cache to invalidate."""
    kind = "vanilla"
    field_bytes = 4 * 61188  # the parameters, read once per workgroup

    def __init__(self, net):
        self.net = net

    def launched(self, shading):
        """Count one fused frame: in native_render_calls, and as ONE native
        evaluation of the field for the whole frame, where the host loop
        counts one per iteration."""
        self.net.native_render_calls += 1
        self.net.native_calls += 1

    def operands(self):
        """The 19 sigma_net tensors in state_dict order."""
        return [p.detach() for p in sigma_net_params(self.net.sigma_net)]


def input_gradient(net, x):
    """d sigma.sum() / d x [M, 3] f32 (no graph): the weight-free backward
    with grad_sigma = 1, grad_albedo = 0."""
    net.native_normal_calls += 1
    x = x.detach().reshape(-1, 3).contiguous().float()
    M = x.shape[0]
    ws = [p.detach().contiguous() for p in sigma_net_params(net.sigma_net)]
    dx = torch.empty(M, 3, device=x.device, dtype=torch.float32)
    if M:
        _resmlp.field_backward(x, ws, torch.ones(M, device=x.device),
                               torch.zeros(M, 3, device=x.device, dtype=torch.float16), dx=dx)
    return dx
