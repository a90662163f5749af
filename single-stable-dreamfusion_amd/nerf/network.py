"""Vanilla-backbone NeRF field (behavioural mirror of reference nerf/network.py:13-221).

Frequency-encoded position (degree 6, 39 features) -> residual MLP of width
128 (four ResBlocks Linear -> LayerNorm -> + skip -> SiLU, then
Linear(128, 4)), the Gaussian density blob at the origin, normals as the
field's input gradient, and a frequency-encoded background MLP 39 -> 64 -> 3.
Module names, parameter shapes and creation order (hence seeded
initialisation and state_dict keys) match the reference.

Under fp16 autocast on the GPU, with the reference's shape, common_forward
runs on the fused native kernels (nerf/vanilla_field.py, csrc/resmlp.hip),
and so does the normal of no-grad calls (eval frames); `fused_field = False`,
f32, bf16 or any other width run the torch path below (encoder -> MLP ->
heads, normal by autograd.grad), and so do shaded training steps, whose
autograd normal carries a graph (through the Gaussian blob and trunc_exp).
`native_calls` / `native_normal_calls` / `torch_calls` count which path ran.
Albedo eval frames (`--test`, eval_step, test_step, the GUI) render in one
persistent launch under the same conditions (csrc/resmlprender.hip):
native_infer_field returns the descriptor NeRFRenderer._infer_fused dispatches
on, and `native_render_calls` counts the frames (each also counts once in
`native_calls`, where the host loop makes one call per iteration);
`native_infer = False` returns to the host loop.  Not covered: the three
shaded views (their normal is the MLP's input gradient; they keep the host
loop on the native field and normal) and the background MLP (a LayerNorm
ResBlock net the native ray head does not evaluate: native_background_layers
returns None).
Under Trainer(graph_step=True) the albedo train step replays as a graph of
native launches (nerf/native_vanilla_step.py: the device-count forms of the
field, the opacity regulariser, GradScaler + Adam in the graph), and
`native_step_calls` counts the steps so served; shaded train steps need the
parameter gradient of the MLP's input gradient and stay on the eager autograd
step.
The reference's NeRFNetwork_Kailu wrapper of this file is nerf/network_dvgo.py.
"""
import torch
import torch.nn as nn

import raymarching
from activation import trunc_exp
from encoding import get_encoder

from . import vanilla_field as _vf
from .renderer import NeRFRenderer
from .utils import safe_normalize


class ResBlock(nn.Module):
    """Linear -> LayerNorm -> + identity (projected when the width changes) -> SiLU."""

    def __init__(self, dim_in, dim_out, bias=True):
        super().__init__()
        self.dim_in, self.dim_out = dim_in, dim_out
        self.dense = nn.Linear(dim_in, dim_out, bias=bias)
        self.norm = nn.LayerNorm(dim_out)
        self.activation = nn.SiLU()
        self.skip = nn.Linear(dim_in, dim_out, bias=False) if dim_in != dim_out else None

    def forward(self, x):
        out = self.norm(self.dense(x))
        out += x if self.skip is None else self.skip(x)
        return self.activation(out)


class MLP(nn.Module):
    """num_layers - 1 ResBlocks, then a Linear to dim_out."""

    def __init__(self, dim_in, dim_out, dim_hidden, num_layers, bias=True):
        super().__init__()
        self.dim_in, self.dim_out = dim_in, dim_out
        self.dim_hidden, self.num_layers = dim_hidden, num_layers
        net = [ResBlock(dim_in if i == 0 else dim_hidden, dim_hidden, bias=bias)
               for i in range(num_layers - 1)]
        net.append(nn.Linear(dim_hidden, dim_out, bias=bias))
        self.net = nn.ModuleList(net)

    def forward(self, x):
        for layer in self.net:
            x = layer(x)
        return x


class NeRFNetwork(NeRFRenderer):
    def __init__(self, opt, num_layers=5, hidden_dim=128, num_layers_bg=2, hidden_dim_bg=64):
        super().__init__(opt)
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.encoder, self.in_dim = get_encoder("frequency", input_dim=3)
        self.sigma_net = MLP(self.in_dim, 4, hidden_dim, num_layers, bias=True)
        # encoder + MLP + heads as one native node (nerf/vanilla_field.py)
        # where it applies; False: FreqEncoder -> MLP -> trunc_exp / sigmoid
        self.fused_field = True
        # which path served common_forward / the normal's input gradient
        self.native_calls = self.native_normal_calls = self.torch_calls = 0
        # eval frames rendered by the fused persistent launch (csrc/resmlprender.hip)
        self.native_render_calls = 0
        # train steps served by the native step (nerf/native_vanilla_step.py)
        self.native_step_calls = 0
        if self.bg_radius > 0:
            self.num_layers_bg = num_layers_bg
            self.hidden_dim_bg = hidden_dim_bg
            self.encoder_bg, self.in_dim_bg = get_encoder("frequency", input_dim=3)
            self.bg_net = MLP(self.in_dim_bg, 3, hidden_dim_bg, num_layers_bg, bias=True)
        else:
            self.bg_net = None

    def gaussian(self, x):
        """Density blob at the scene centre: 5 * exp(-|x|^2 / (2 * 0.2^2))."""
        return 5 * torch.exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2))

    def _native(self, x):
        # capacity-sized samples of the device-count march keep the torch path
        return raymarching.live_rows(x) is None and _vf.eligible(self, x)

    def common_forward(self, x, native=True):
        """x [N, 3] in [-bound, bound] -> sigma [N] (f32), albedo [N, 3].
        native=False: the torch path even where the native node applies."""
        if native and self._native(x):
            return _vf.vanilla_field(self, x)
        self.torch_calls += 1
        h = self.sigma_net(self.encoder(x, bound=self.bound))
        sigma = trunc_exp(h[..., 0] + self.gaussian(x))
        albedo = torch.sigmoid(h[..., 1:])
        return sigma, albedo

    def _native_normal(self, x):
        # The autograd normal carries a graph when grad is on (through the
        # Gaussian blob and trunc_exp's backward, which are torch ops on x and
        # sigma), so only no-grad calls (eval frames, the occupancy refresh)
        # take the native input gradient; shaded training steps run the
        # torch path.
        return not torch.is_grad_enabled() and self._native(x)

    def _field_and_gradient(self, x):
        """sigma, albedo and -d sigma.sum() / dx (reference network.py:165-173)."""
        if self._native_normal(x):
            sigma, albedo = self.common_forward(x)
            return sigma, albedo, -_vf.input_gradient(self, x)
        with torch.enable_grad():
            x.requires_grad_(True)
            sigma, albedo = self.common_forward(x, native=False)
            grad = torch.autograd.grad(torch.sum(sigma), x, create_graph=True)[0]
        return sigma, albedo, -grad

    @staticmethod
    def _unit(n):
        n = safe_normalize(n)
        n[torch.isnan(n)] = 0
        return n

    def normal(self, x):
        return self._unit(self._field_and_gradient(x)[2])

    def forward(self, x, d, l=None, ratio=1, shading="albedo"):
        """x, d: [N, 3]; l: [3] light direction; ratio: ambient share.
        Returns sigma [N], color [N, 3], normal [N, 3] or None."""
        if shading == "albedo":
            sigma, color = self.common_forward(x)
            return sigma, color, None
        sigma, albedo, normal = self._field_and_gradient(x)
        normal = self._unit(normal)
        lambertian = ratio + (1 - ratio) * (normal @ l).clamp(min=0)
        if shading == "textureless":
            color = lambertian.unsqueeze(-1).repeat(1, 3)
        elif shading == "normal":
            color = (normal + 1) / 2
        else:  # lambertian
            color = albedo * lambertian.unsqueeze(-1)
        return sigma, color, normal

    def native_infer_field(self, shading, x):
        """The vanilla-field descriptor when the fused inference renderer
        serves this frame: the albedo shading under the conditions of the
        native field (fp16 autocast on the GPU, the reference's shape, f32
        parameters, fused_field); else None, and the host loop runs.  The
        shaded views need the MLP's input gradient, which the kernel does not
        hold the weights for."""
        if shading != "albedo" or not self.native_infer:
            return None
        if not _vf.eligible(self, x):
            return None
        return _vf.InferField(self)

    def density(self, x):
        sigma, albedo = self.common_forward(x)
        return {"sigma": sigma, "albedo": albedo}

    def background(self, d):
        return torch.sigmoid(self.bg_net(self.encoder_bg(d)))

    def get_params(self, lr):
        groups = [{"params": self.sigma_net.parameters(), "lr": lr}]
        if self.bg_radius > 0:
            groups.append({"params": self.bg_net.parameters(), "lr": lr})
        return groups
