"""Fused voxel field: coordinate map + trilinear density / feature samples +
encodings + colour MLP + activations as ONE autograd node on the native
kernels (csrc/voxelfield.hip), the native path of nerf/network_dvgo.py's
common_forward (reference nerf/network.py:251-268 with weight = None) and of
its normal (:135-146).

Served: fp16 autocast on CUDA, f32 parameters and volumes, rgbnet a BasicMLP
of width 128 and depth 3 with dim0 <= 96, position frequencies 2^i, and an
act_shift below 0.99 (above it the reference colours no row when weight is
None).  Anything else runs the module's torch path.

The node returns no gradient for the positions, the density volume or the
feature volume: positions are leaves in both render paths and the volumes are
frozen (requires_grad = False from construction), so sigma has no gradient at
all and is marked non-differentiable, as it is on the torch path.  For the
same reason the normal -d sigma / d x depends on no trainable tensor: the
closed-form native normal (input_gradient) is exact for grad-enabled calls
too, which the vanilla backbone's is not.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import _voxelfield

NAMES = ["net.0.weight", "net.0.bias", "net.2.0.weight", "net.2.0.bias", "net.3.weight",
         "net.3.bias"]


def rgbnet_params(rgbnet):
    """The 6 tensors of rgbnet in state_dict order (the packed order of
    include/dfhip.h)."""
    return list(rgbnet.parameters())


def volume(net):
    """The native operands of net.main_net's frozen volumes: density
    [Nx, Ny, Nz], one channel-last f32 copy of k0 [Nx, Ny, Nz, C], the box as
    host floats, the view encoding.  Built once; rebuilt only when a tensor
    was moved or written (a checkpoint load), which their versions show."""
    m = net.main_net
    srcs = [m.density, m.k0, m.xyz_min, m.xyz_max, getattr(m, "posfreq", None),
            getattr(m, "viewfreq", None)]
    key = tuple((t.data_ptr(), t._version, t.device) if t is not None else None for t in srcs)
    cached = net.__dict__.get("_voxel_volume")
    if cached is not None and cached[0] == key:
        return cached[1]
    with torch.no_grad():
        density = m.density.detach()[0, 0].contiguous()
        k0 = m.k0.detach()[0].permute(1, 2, 3, 0).contiguous()
        box = m.xyz_min.detach().tolist() + m.xyz_max.detach().tolist()
        pos = getattr(m, "posfreq", None)
        pos_freqs = 0 if pos is None else int(pos.numel())
        pow2 = pos is None or pos.detach().tolist() == [float(2 ** i) for i in range(pos_freqs)]
        view = None
        if getattr(m, "viewfreq", None) is not None:
            with torch.autocast(m.k0.device.type, enabled=False):
                view = net.view_encoding(1, m.k0.device)[0].float().contiguous()
    vol = _voxelfield.Volume(density, k0, box, pos_freqs, view) if density.is_cuda else None
    net.__dict__["_voxel_volume"] = (key, (vol, pow2))
    return vol, pow2


def eligible(net, x):
    if not (x.is_cuda and torch.is_autocast_enabled("cuda")):
        return False
    if torch.get_autocast_dtype("cuda") != torch.float16:
        return False
    return model_eligible(net, x.device)


def model_eligible(net, device):
    """The model's share of eligible(): what the native kernels need of the
    network itself, whatever the autocast state of the caller (the native
    train step, nerf/native_voxel_step.py, runs them under no autocast)."""
    if not getattr(net, "fused_field", False):
        return False
    m = net.main_net
    if not 1.0 > 1e-2 + m.act_shift:
        return False
    if [n for n, _ in m.rgbnet.named_parameters()] != NAMES:
        return False
    if m.dim0 > _voxelfield.MAX_IN or m.k0.shape[1] < 1:
        return False
    ps = rgbnet_params(m.rgbnet)
    if [tuple(p.shape) for p in ps] != _voxelfield.shapes(m.dim0):
        return False
    if not all(p.dtype == torch.float32 and p.device == device
               for p in ps + [m.density, m.k0, m.xyz_min, m.xyz_max]):
        return False
    vol, pow2 = volume(net)
    return vol is not None and pow2 and vol.pos_freqs <= 15 and vol.dim0 == m.dim0


class _VoxelField(Function):
    @staticmethod
    def forward(ctx, x, density, k0, vol, bound, act_shift, *params):
        """x [M, 3] -> sigma [M] f32, albedo [M, 3] f16."""
        x = x.detach().contiguous().float()
        M = x.shape[0]
        ws = [p.detach().contiguous() for p in params]
        sigma = torch.empty(M, device=x.device, dtype=torch.float32)
        albedo = torch.empty(M, 3, device=x.device, dtype=torch.float16)
        _voxelfield.field_forward(x, vol, bound, act_shift, ws, sigma, albedo)
        ctx.save_for_backward(x, *ws)
        ctx.vol, ctx.bound = vol, bound
        ctx.mark_non_differentiable(sigma)
        return sigma, albedo

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sigma, grad_albedo):
        x, *ws = ctx.saved_tensors
        if grad_albedo is None:
            grad_albedo = torch.zeros(x.shape[0], 3, device=x.device, dtype=torch.float16)
        if grad_albedo.dtype not in (torch.float16, torch.float32):
            grad_albedo = grad_albedo.float()
        grads = [torch.empty_like(w) for w in ws]
        _voxelfield.field_backward(x, ctx.vol, ctx.bound, ws, grad_albedo.contiguous(), grads)
        return (None, None, None, None, None, None, *grads)


def voxel_field(net, x):
    """sigma [M] f32, albedo [M, 3] f16 of positions x [M, 3] on the native node."""
    net.native_calls += 1
    m = net.main_net
    vol, _ = volume(net)
    return _VoxelField.apply(x.reshape(-1, 3), m.density, m.k0, vol, float(net.bound),
                             float(m.act_shift), *rgbnet_params(m.rgbnet))


def input_gradient(net, x):
    """-d sigma.sum() / d x [M, 3] f32 (no graph, not normalised): the
    negated input gradient in closed form, which is the reference's normal
    before safe_normalize."""
    net.native_normal_calls += 1
    x = x.detach().reshape(-1, 3).contiguous().float()
    vol, _ = volume(net)
    out = torch.empty(x.shape[0], 3, device=x.device, dtype=torch.float32)
    _voxelfield.normal(x, vol, float(net.bound), float(net.main_net.act_shift), out)
    return out


class InferField:
    """What NeRFRenderer._infer_fused needs to render this backbone in one
    persistent launch (csrc/voxelrender.hip): the frozen volumes' cached
    operands and rgbnet's f32 parameters themselves, taken when the frame is
    launched, so an optimizer step between two frames (torch's, the native
    Adam or a replayed graph, all of which write the parameters in place) is
    seen by the next frame with no cache to invalidate."""
    kind = "voxel"

    def __init__(self, net):
        self.net = net

    def launched(self, shading):
        """Count one fused frame: in native_render_calls, and as ONE native
        evaluation of the field (shaded: and of the normal) for the whole
        frame, where the host loop counts one per iteration."""
        net = self.net
        net.native_render_calls += 1
        net.native_calls += 1
        if shading != "albedo":
            net.native_normal_calls += 1

    def operands(self):
        """(Volume, act_shift, the 6 rgbnet tensors in state_dict order)."""
        m = self.net.main_net
        vol, _ = volume(self.net)
        return vol, float(m.act_shift), [p.detach() for p in rgbnet_params(m.rgbnet)]
