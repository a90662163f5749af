"""DVGO voxel-grid backbone (behavioural mirror of reference
nerf/network.py:224-312, NeRFNetwork_Kailu, and of what it uses from the
reference's frameworks/ package: DVGO_Coarse's buffers and act_shift,
grid_sample_3d, DVGO_Fine.query_rgb, position_encoding, BasicMLP).

A pretrained dense-voxel NeRF is edited by SDS: the density volume
[1, 1, Nx, Ny, Nz] and the feature volume k0 [1, C, Nx, Ny, Nz] are frozen;
only the colour MLP rgbnet (and the background MLP) train.  A position is
mapped into the volume's box (y / z swap, scale 1.25), sampled trilinearly
(corner indices clamped, weights not), and
    sigma  = 10 * softplus(raw + act_shift), raw = 0 outside the box,
    albedo = sigmoid(rgbnet(cat(k0 sample, PE(normalised xyz), PE((1,1,1)/sqrt 3))))
             inside the box, 0.5 outside.
`main_net`'s state_dict keys are the reference's, so a checkpoint saved by
either side loads in the other.  The reference computes the flat corner index
in float32 (exact only below 2^24 voxels); this module indexes with integers.

Under fp16 autocast on the GPU, with a width-128 depth-3 rgbnet and
dim0 <= 96, common_forward runs on the fused native kernels
(nerf/voxel_field.py, csrc/voxelfield.hip); `fused_field = False`, f32, bf16,
another MLP shape, a `weight` argument or capacity-sized samples of the
device-count march run the torch path below.  The normal (-d sigma / d x) is
served natively for no-grad AND grad-enabled calls: the density volume is
frozen and the positions are leaves, so the normal carries no graph to any
trainable tensor and the closed form loses nothing (the vanilla backbone's
normal does carry one, nerf/network.py).  `native_calls` /
`native_normal_calls` / `torch_calls` count which path ran.

Eval frames (run_cuda without grad: --test, eval_step, test_step, test_gui)
of the four shadings run as one persistent launch (csrc/voxelrender.hip)
under the same conditions: native_infer_field returns the descriptor
NeRFRenderer._infer_fused dispatches on, and `native_render_calls` counts the
frames so rendered (each also counts once in `native_calls` and, shaded, in
`native_normal_calls`: the native field served it, in one evaluation where
the host loop makes one per iteration); `native_infer = False` returns to the
host loop.

Graph-replayed training (Trainer graph_step) runs this backbone's steps as
NativeVoxelStep (nerf/native_voxel_step.py: the device-count forms of the
field kernels, the training shading entry of csrc/voxelstep.hip, bg_net
through torch inside the graph) where its eligible() holds, and eagerly where
it does not; `native_step_calls` counts the steps so served.  The native
background head does not describe bg_net (native_background_layers returns
None).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import raymarching
from encoding import get_encoder

from . import voxel_field as _vf
from .network import MLP
from .renderer import NeRFRenderer
from .utils import safe_normalize


class BasicMLP(nn.Module):
    """Linear -> ReLU, depth - 2 times (Linear -> ReLU), Linear; keys net.0,
    net.2.0, ..., net.<depth> (reference decoders/mlps.py:59-73)."""

    def __init__(self, in_dim, out_dim=3, width=128, depth=3):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(in_dim, width), nn.ReLU(inplace=True),
            *[nn.Sequential(nn.Linear(width, width), nn.ReLU(inplace=True))
              for _ in range(depth - 2)],
            nn.Linear(width, out_dim))
        nn.init.constant_(self.net[-1].bias, 0)

    def forward(self, x):
        return self.net(x)


def position_encoding(x, freqs):
    """[x, sin(x_d f_i), cos(x_d f_i)], d major (reference modules/utils.py:129-131)."""
    emb = (x.unsqueeze(-1) * freqs).flatten(-2)
    return torch.cat([x, emb.sin(), emb.cos()], -1)


class VoxelNet(nn.Module):
    """The tensors of a fine DVGO model: frozen volumes, box, encodings' frequencies,
    colour MLP (reference dvgo_coarse.py:14-32, dvgo_fine.py:13-28)."""

    def __init__(self, world_size, C, posbase_pe, viewbase_pe, width, depth, xyz_min, xyz_max,
                 alpha_init):
        super().__init__()
        ws = [int(v) for v in world_size]
        self.density = nn.Parameter(torch.zeros(1, 1, *ws), requires_grad=False)
        self.k0 = nn.Parameter(torch.zeros(1, C, *ws), requires_grad=False)
        lo = torch.as_tensor(xyz_min, dtype=torch.float32).reshape(3)
        hi = torch.as_tensor(xyz_max, dtype=torch.float32).reshape(3)
        self.register_buffer("xyz_min", lo.clone())
        self.register_buffer("xyz_max", hi.clone())
        size = torch.tensor(ws)
        self.register_buffer("voxel_size_each", (hi - lo) / (size - 1).clamp(min=1))
        self.register_buffer("voxel_size_ratio", torch.tensor(1.0))
        self.register_buffer("voxel_size", ((hi - lo).prod() / size.prod()).pow(1 / 3))
        self.register_buffer("world_size", size.long())
        dim0 = C
        if posbase_pe:
            self.register_buffer("posfreq", torch.FloatTensor([2 ** i for i in range(posbase_pe)]))
            dim0 += 3 + 6 * posbase_pe
        if viewbase_pe:
            self.register_buffer("viewfreq",
                                 torch.FloatTensor([2 ** i for i in range(viewbase_pe)]))
            dim0 += 3 + 6 * viewbase_pe
        self.dim0 = dim0
        self.rgbnet = BasicMLP(dim0, 3, width, depth)
        self.alpha_init = float(alpha_init)
        self.act_shift = math.log(1 / (1 - self.alpha_init) - 1)


# ---------------------------------------------------------------- checkpoint
def _lookup(tree, path):
    """tree.a.b for plain dicts or namespaces at any level, else None."""
    for name in path:
        if tree is None:
            return None
        tree = tree.get(name) if isinstance(tree, dict) else getattr(tree, name, None)
    return tree


def _find_alpha_init(hyper):
    """alpha_init at fine_model_and_render.alpha_init, searched at the top
    level and under any one or two enclosing keys (Lightning nests the config
    under the constructor's argument names, e.g. hparams.cfg)."""
    path = ("fine_model_and_render", "alpha_init")
    roots, seen = [hyper], []
    for _ in range(3):
        nxt = []
        for r in roots:
            v = _lookup(r, path)
            if v is not None:
                return float(v)
            seen.append(r)
            kids = r.values() if isinstance(r, dict) else getattr(r, "__dict__", {}).values()
            nxt += [k for k in kids if isinstance(k, dict) or hasattr(k, "__dict__")]
        roots = nxt
    return None


def load_dvgo(path, alpha_init=None):
    """Read a DVGO checkpoint: a Lightning-style {"state_dict", "hyper_parameters"}
    dict or a bare state_dict.  Returns (VoxelNet with the checkpoint's tensors,
    the checkpoint's state_dict).  Shapes, C, the encodings' sizes, width and
    depth come from the tensors; alpha_init from the hyper-parameters, else
    from the argument (--dvgo_alpha_init).  Needs neither pytorch_lightning nor
    omegaconf unless the file itself pickles their classes."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    hyper = None
    if isinstance(ckpt, dict) and isinstance(ckpt.get("state_dict"), dict):
        hyper, sd = ckpt.get("hyper_parameters"), ckpt["state_dict"]
    else:
        sd = ckpt
    if not isinstance(sd, dict) or not all(k in sd for k in ("density", "k0", "xyz_min",
                                                                "xyz_max")):
        raise ValueError(f"{path}: not a DVGO checkpoint (density, k0, xyz_min and xyz_max "
                         "expected in its state_dict)")
    found = _find_alpha_init(hyper) if hyper is not None else None
    if found is None:
        found = alpha_init
    if found is None:
        raise ValueError(f"{path}: alpha_init is not in the checkpoint's hyper_parameters "
                         "(fine_model_and_render.alpha_init); pass --dvgo_alpha_init")
    if not 0.0 < float(found) < 1.0:
        raise ValueError(f"alpha_init must lie in (0, 1), got {found}")
    density, k0 = sd["density"], sd["k0"]
    if density.dim() != 5 or k0.dim() != 5 or density.shape[2:] != k0.shape[2:]:
        raise ValueError(f"{path}: density [1, 1, Nx, Ny, Nz] and k0 [1, C, Nx, Ny, Nz] expected")
    layers = sorted({k[len("rgbnet.net."):-len(".weight")] for k in sd
                     if k.startswith("rgbnet.net.") and k.endswith(".weight")},
                    key=lambda s: [int(p) for p in s.split(".")])
    if len(layers) < 2 or "rgbnet.net.0.weight" not in sd:
        raise ValueError(f"{path}: no rgbnet of the BasicMLP layout (rgbnet.net.0, .2.0, ...)")
    width = sd["rgbnet.net.0.weight"].shape[0]
    posbase = sd["posfreq"].numel() if "posfreq" in sd else 0
    viewbase = sd["viewfreq"].numel() if "viewfreq" in sd else 0
    net = VoxelNet(density.shape[2:], k0.shape[1], posbase, viewbase, width, len(layers),
                   sd["xyz_min"], sd["xyz_max"], float(found))
    own = net.state_dict()
    missing = [k for k in own if k not in sd and not k.startswith("voxel_size")
               and k != "world_size"]
    if missing:
        raise ValueError(f"{path}: missing {missing}")
    # keys of the reference's training state (mask cache, metrics) are not ours
    net.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    return net, sd


class NeRFNetwork(NeRFRenderer):
    def __init__(self, opt, num_layers_bg=2, hidden_dim_bg=64):
        super().__init__(opt)
        path = getattr(opt, "dvgo_ckpt", None)
        if not path:
            raise ValueError("the dvgo backbone needs a pretrained checkpoint: pass --dvgo_ckpt")
        self.main_net, _ = load_dvgo(path, getattr(opt, "dvgo_alpha_init", None))
        # map + samples + encodings + MLP + activations as one native node
        # (nerf/voxel_field.py) where it applies; False: the torch ops below
        self.fused_field = True
        # which path served common_forward / the normal
        self.native_calls = self.native_normal_calls = self.torch_calls = 0
        # eval frames rendered by the fused persistent launch (csrc/voxelrender.hip)
        self.native_render_calls = 0
        # train steps served by the native voxel step (nerf/native_voxel_step.py)
        self.native_step_calls = 0
        if self.bg_radius > 0:
            self.num_layers_bg = num_layers_bg
            self.hidden_dim_bg = hidden_dim_bg
            self.encoder_bg, self.in_dim_bg = get_encoder("frequency", input_dim=3)
            self.bg_net = MLP(self.in_dim_bg, 3, hidden_dim_bg, num_layers_bg, bias=True)
        else:
            self.bg_net = None

    # ------------------------------------------------------------ torch path
    def to_our_coor(self, x):
        """[-bound, bound]^3 -> the volume's box: y / z swapped, scaled by 1.25
        about the centre (the box covers 0.8 of the bound)."""
        m = self.main_net
        s = ((x + self.bound) / (2 * self.bound))[..., [0, 2, 1]]
        s = (s - 0.5) * 1.25 + 0.5
        return s * (m.xyz_max - m.xyz_min) + m.xyz_min

    def trilinear(self, pts, grid):
        """pts [n, 3] in the box, grid [1, C, Nx, Ny, Nz] -> [n, C]: the cell of
        floor, weights (floor + 1 - g) and (g - floor) not clamped, corner
        indices clamped; differentiable in pts (reference osr_fine.py:559-673
        through network.py:318-324)."""
        m = self.main_net
        C, (Nx, Ny, Nz) = grid.shape[1], grid.shape[2:]
        last = torch.tensor([Nx - 1, Ny - 1, Nz - 1], device=pts.device)
        u = (pts - m.xyz_min) / (m.xyz_max - m.xyz_min)
        g = ((u * 2 - 1) + 1) / 2 * last.to(pts.dtype)
        with torch.no_grad():
            f = torch.floor(g)
            i0 = torch.minimum(f.long().clamp(min=0), last)
            i1 = torch.minimum((f.long() + 1).clamp(min=0), last)
        hi, lo = (f + 1) - g, g - f
        vol = grid[0].reshape(C, -1)
        out = None
        for k in range(8):  # grid z fastest, then y, then x: the reference's order
            z1, y1, x1 = k & 1, k & 2, k & 4
            w = (lo if z1 else hi)[:, 2] * (lo if y1 else hi)[:, 1] * (lo if x1 else hi)[:, 0]
            idx = ((i1 if x1 else i0)[:, 0] * Ny + (i1 if y1 else i0)[:, 1]) * Nz \
                + (i1 if z1 else i0)[:, 2]
            term = vol[:, idx] * w
            out = term if out is None else out + term
        return out.T

    def view_encoding(self, n, device):
        """The encoding of the fixed view direction (1, 1, 1) / sqrt(3), n rows."""
        d = torch.ones(n, 3, device=device) / (3 ** 0.5)
        return position_encoding(d, self.main_net.viewfreq)

    def query_rgb(self, pts):
        """Albedo of points inside the box (reference dvgo_fine.py:45-54)."""
        m = self.main_net
        feats = [self.trilinear(pts, m.k0)]
        if hasattr(m, "posfreq"):
            feats.append(position_encoding((pts - m.xyz_min) / (m.xyz_max - m.xyz_min), m.posfreq))
        if hasattr(m, "viewfreq"):
            feats.append(self.view_encoding(pts.shape[0], pts.device).to(pts.dtype))
        return torch.sigmoid(m.rgbnet(torch.cat(feats, -1)))

    def _sigma(self, x):
        m = self.main_net
        pts = self.to_our_coor(x)
        inside = ((pts <= m.xyz_max) & (m.xyz_min <= pts)).all(dim=-1)
        raw = torch.zeros_like(x[..., 0])
        raw[inside] = self.trilinear(pts[inside], m.density)[..., 0]
        return F.softplus(raw + m.act_shift) * 10, pts, inside

    # ------------------------------------------------------------ field
    def _native(self, x):
        # capacity-sized samples of the device-count march keep the torch path
        return raymarching.live_rows(x) is None and _vf.eligible(self, x)

    def common_forward(self, x, weight=None, native=True):
        """x [N, 3] in [-bound, bound] -> sigma [N] (f32), albedo [N, 3].
        weight [N] (optional): rows at or below 1e-2 + act_shift keep the
        default albedo 0.5 (reference network.py:252-266).
        native=False: the torch path even where the native node applies."""
        if native and weight is None and self._native(x):
            return _vf.voxel_field(self, x)
        self.torch_calls += 1
        sigma, pts, inside = self._sigma(x)
        if weight is None:
            weight = torch.ones_like(x[..., 0])
        albedo = torch.ones_like(x).float() * 0.5
        valid = (weight > (1e-2 + self.main_net.act_shift)) & inside
        albedo[valid] = self.query_rgb(pts[valid]).float()
        return sigma, albedo

    @staticmethod
    def _unit(n):
        n = safe_normalize(n)
        n[torch.isnan(n)] = 0
        return n

    def normal(self, x):
        """safe_normalize(-d sigma / d x), NaN -> 0 (reference network.py:135-146)."""
        if self._native(x):
            return self._unit(_vf.input_gradient(self, x))
        self.torch_calls += 1
        with torch.enable_grad():
            x.requires_grad_(True)
            sigma, _, _ = self._sigma(x)
            grad = torch.autograd.grad(torch.sum(sigma), x, create_graph=True)[0]
        return self._unit(-grad)

    def forward(self, x, d, l=None, ratio=1, shading="albedo", weight=None):
        """x, d: [N, 3]; l: [3] light direction; ratio: ambient share.
        Returns sigma [N], color [N, 3], normal [N, 3] or None."""
        sigma, albedo = self.common_forward(x, weight)
        if shading == "albedo":
            return sigma, albedo, None
        normal = self.normal(x)
        lambertian = ratio + (1 - ratio) * (normal @ l).clamp(min=0)
        if shading == "textureless":
            color = lambertian.unsqueeze(-1).repeat(1, 3)
        elif shading == "normal":
            color = (normal + 1) / 2
        else:  # lambertian
            color = albedo * lambertian.unsqueeze(-1)
        return sigma, color, normal

    def native_infer_field(self, shading, x):
        """The voxel-field descriptor when the fused inference renderer serves
        this frame: one of the four shadings, and the conditions of the
        native field (fp16 autocast on the GPU, width 128, depth 3,
        dim0 <= 96, fused_field); else None, and the host loop runs."""
        if shading not in ("albedo", "textureless", "lambertian", "normal"):
            return None
        if not self._native(x):
            return None
        return _vf.InferField(self)

    def density(self, x):
        sigma, albedo = self.common_forward(x)
        return {"sigma": sigma, "albedo": albedo}

    def background(self, d):
        return torch.sigmoid(self.bg_net(self.encoder_bg(d)))

    def get_params(self, lr):
        """rgbnet and the background MLP; the volumes stay frozen."""
        self.main_net.density.requires_grad = False
        self.main_net.k0.requires_grad = False
        groups = [{"params": self.main_net.rgbnet.parameters(), "lr": lr}]
        if self.bg_radius > 0:
            groups.append({"params": self.bg_net.parameters(), "lr": lr})
        return groups
