"""GPU tests of the DVGO backbone's native train step
(nerf/native_voxel_step.py, the device-count voxel entries, csrc/voxelstep.hip):

* one native step gives the live count, weights_sum and every parameter
  gradient of the autograd step fed the same rays, noise, light and SDS
  gradient, bit for bit (albedo: at 16 x 16 with the trained bitfield and at
  32 x 32 with every cell occupied, more than one 65536-row backward chunk);
  pred_rgb within 2^-22: the head forms image + (1 - ws) * bg with one
  contracted multiply-add where torch multiplies and adds, two half-ulp
  roundings (2^-23) on values below 2, doubled;
* a lambertian step: counts, sigma, weights_sum and the per-sample colour
  gradient bit for bit, pred_rgb within 2^-9 (the bound of
  tests/test_gpu_voxel_render.py), the rgbnet gradients no farther from a
  float64 truth than twice the autograd step's are, the loss no farther from
  a float64 evaluation on the step's own buffers than twice the autograd
  step's is;
* a textureless step leaves rgbnet, its Adam moments and step counts alone;
* graph-replayed training runs natively, and the replay equals the same
  launches run eagerly with the host-lr optimizer, bit for bit;
* a model the native step does not serve trains eagerly under graph_step.
"""
import copy

import numpy as np
import pytest
import torch

import voxel_cases as vc

pytestmark = pytest.mark.gpu

B_RGB = 2.0 ** -22
B_TL = 2.0 ** -9


@pytest.fixture(scope="module")
def ckpts(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dvgo_native")
    out = {}
    for name, kw in (("small", dict(world=vc.WORLD_SMALL)),
                     ("deep", dict(world=vc.WORLD_SMALL, depth=4))):
        sd, _ = vc.make_state(seed=len(out), **kw)
        out[name] = (vc.save_checkpoint(tmp / f"{name}.dvgo", sd), sd)
    return out


def make_trainer(gpu, ckpts, seed, res=16, graph=False, ckpt="small", args=()):
    import main
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", "-O", *args, "--backbone", "dvgo", "--dvgo_ckpt",
                          ckpts[ckpt][0], "--h", str(res), "--w", str(res), "--guidance",
                          "synthetic", "--seed", str(seed)])
    seed_everything(seed)
    model = main.network_class(opt)(opt)
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    decay = lambda it: 0.1 ** min(it / 50, 1)  # noqa: E731  every step's lr differs in f32
    sched = lambda o: torch.optim.lr_scheduler.LambdaLR(o, decay)  # noqa: E731
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=None, optimizer=optimizer, ema_decay=None, fp16=True,
                      lr_scheduler=sched, scheduler_update_every_step=True,
                      use_checkpoint="scratch", mute=True, graph_step=graph)
    data = NeRFDataset(opt, device=gpu, type="train", H=res, W=res, size=100)
    trainer.model.train()
    return trainer, data


def settle(trainer, seed=4):
    torch.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16):
        trainer.model.update_extra_state()
    assert int(trainer.model.density_bitfield.count_nonzero()) > 0


def norm_err(g, r):
    g, r = g.detach().double().cpu(), r.detach().double().cpu()
    if float(r.norm()) == 0.0:
        return float(g.norm())
    return float((g - r).norm() / r.norm())


def native_once(trainer, batch, res, shading, ratio):
    """One native step's launches (no optimizer); the gradients cloned."""
    from nerf.native_voxel_step import NativeVoxelStep, eligible
    assert eligible(trainer, shading)
    nat = NativeVoxelStep(trainer, res, res, shading, ratio)
    nat.prologue(batch["pose"], batch["intrinsics"], 11, 1234)
    nat.body()
    torch.cuda.synchronize()
    m = trainer.model
    grads = {"rgb": [None if p.grad is None else p.grad.detach().clone()
                     for p in m.main_net.rgbnet.parameters()],
             "bg": [p.grad.detach().clone() for p in m.bg_net.parameters()]}
    return nat, grads


def autograd_once(trainer, nat, batch, res, shading, ratio):
    """The autograd step on the native step's rays, noise, light and SDS
    gradient, with the host-count march.  Returns (pred_rgb, pred_ws, loss,
    the field's outputs and the per-sample colour with its gradient)."""
    model = trainer.model
    trainer.optimizer.zero_grad(set_to_none=True)
    g_img = nat.g_image.view(1, 3, res, res).clone()
    trainer.guidance.sds_grad = lambda text_z, pred_rgb, *a, **k: (pred_rgb, g_img)
    model.march_noises = nat.noises.clone()
    if nat.shade_code:
        trainer.opt.light_d = nat.light.clone()
    eager = {"H": res, "W": res, "rays_o": nat.rays_o.view(1, -1, 3).clone(),
             "rays_d": nat.rays_d.view(1, -1, 3).clone(), "dir": batch["dir"]}
    text_z = trainer.text_z[batch["dir"]]
    keep = {}
    forward = model.forward

    def recording(*a, **k):
        sigma, color, normal = forward(*a, **k)
        if color.requires_grad:  # a textureless colour carries no graph
            color.retain_grad()
        keep.update(sigma=sigma, color=color)
        return sigma, color, normal
    model.forward = recording
    torch_calls = model.torch_calls
    try:
        assert model.device_count_march is False
        with torch.autocast("cuda", dtype=torch.float16):
            pred_rgb, pred_ws, loss = trainer.train_step(eager, shading, ratio, text_z)
        trainer.backward_only(loss)
    finally:
        del model.forward
        del model.march_noises
        del trainer.guidance.sds_grad
        if nat.shade_code:
            del trainer.opt.light_d
    torch.cuda.synchronize()
    assert model.torch_calls == torch_calls
    return pred_rgb, pred_ws, loss, keep


def compare_forward(nat, model, pred_rgb, pred_ws, keep, bound):
    live = int(nat.counter[0])
    assert live > 0 and int(model.last_counter[0]) == live
    # (on a multiple of 128 the march's slice adds a whole block of zero rows,
    # the reference's rule, which the native step's row count does not)
    assert live % 128 != 0
    Me = -(-live // 128) * 128
    assert keep["sigma"].shape[0] == Me
    assert torch.equal(keep["sigma"][:live], nat.sigma[:live])
    assert torch.equal(pred_ws.reshape(-1), nat.ws)
    err = float((pred_rgb.detach().float().reshape(3, -1) - nat.out_image).abs().max())
    print(f"parity: {nat.shading} {nat.H}x{nat.W} live={live} pred_rgb max err {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound
    return live, Me


# ---------------------------------------------------------------- albedo
@pytest.mark.parametrize("res, dense", [(16, False), (32, True)])
def test_albedo_step_matches_autograd_step(gpu, ckpts, res, dense):
    trainer, data = make_trainer(gpu, ckpts, 3, res=res)
    model = trainer.model
    settle(trainer)
    if dense:
        model.density_bitfield.fill_(255)
    batch = data.collate([0])
    nat, got = native_once(trainer, batch, res, "albedo", 1.0)
    assert nat.loss.isfinite()
    pred_rgb, pred_ws, loss, keep = autograd_once(trainer, nat, batch, res, "albedo", 1.0)
    live, _ = compare_forward(nat, model, pred_rgb, pred_ws, keep, B_RGB)
    if dense:
        assert live > 65536  # more than one chunk of the field backward
    assert torch.equal(loss.detach().float().reshape(()), nat.loss)
    assert torch.equal(keep["color"][:live], nat.albedo[:live])
    assert torch.equal(keep["color"].grad[:live], nat.grad_color[:live])
    m = model.main_net
    assert m.density.grad is None and m.k0.grad is None
    for p, g in zip(m.rgbnet.parameters(), got["rgb"]):
        assert torch.equal(p.grad, g), (tuple(p.shape), float((p.grad - g).abs().max()))
        assert float(g.abs().sum()) > 0
    for p, g in zip(model.bg_net.parameters(), got["bg"]):
        assert torch.equal(p.grad, g), (tuple(p.shape), float((p.grad - g).abs().max()))
        assert float(g.abs().sum()) > 0


# ---------------------------------------------------------------- lambertian
def test_lambertian_step(gpu, ckpts):
    """The rgbnet gradients against a float64 truth (2x rule, the stick is
    the autograd step): vc.truth on the step's live rows, the upstream the
    step's colour gradient times a float64 lambert factor."""
    res, ratio = 16, 0.1
    trainer, data = make_trainer(gpu, ckpts, 3, res=res)
    model = trainer.model
    settle(trainer)
    batch = data.collate([0])
    nat, got = native_once(trainer, batch, res, "lambertian", ratio)
    pred_rgb, pred_ws, loss, keep = autograd_once(trainer, nat, batch, res, "lambertian", ratio)
    live, Me = compare_forward(nat, model, pred_rgb, pred_ws, keep, B_TL)
    assert torch.equal(keep["color"].grad[:live], nat.grad_color[:live])
    assert float(nat.grad_color[:live].float().abs().sum()) > 0
    for p, g in zip(model.bg_net.parameters(), got["bg"]):
        assert torch.equal(p.grad, g), (tuple(p.shape), float((p.grad - g).abs().max()))
    # float64 truth of the rgbnet gradients
    x = nat.xyzs[:live].cpu()
    rs, ra, ps, aux = vc.truth(ckpts["small"][1], x)
    rn = vc.unit(vc.normal_of(rs, aux))
    lam = ratio + (1 - ratio) * (rn @ nat.light.double().cpu()).clamp(min=0)
    up = nat.grad_color[:live].double().cpu() * lam[:, None]
    rg = torch.autograd.grad(ra, ps, up)
    names = [n for n, _ in model.main_net.rgbnet.named_parameters()]
    for n, p, gy, r in zip(names, model.main_net.rgbnet.parameters(), got["rgb"], rg):
        ey, et = norm_err(gy, r), norm_err(p.grad, r)
        print(f"parity: lambertian step {n}: native {ey:.3e} autograd {et:.3e}")
        assert torch.isfinite(gy).all() and ey <= 2 * et, (n, ey, et)
    # the loss: entropy + lambda_orient * orient, float64 on the step's buffers
    a = nat.ws.double().clamp(1e-5, 1 - 1e-5)
    ent = (-a * torch.log2(a) - (1 - a) * torch.log2(1 - a)).mean()
    n64, d64, s64 = (t[:live].double() for t in (nat.normal, nat.dirs, nat.sigma))
    orient = ((1 - torch.exp(-s64)) * (n64 * d64).sum(-1).clamp(min=0) ** 2).sum() / Me
    r = float(trainer.opt.lambda_entropy * ent + trainer.opt.lambda_orient * orient)
    y, t = float(nat.loss), float(loss.detach())
    print(f"parity: lambertian step loss: native {abs(y - r):.3e} autograd {abs(t - r):.3e} "
          f"of {r:.6e}")
    assert abs(y - r) <= 2 * abs(t - r)


# ---------------------------------------------------------------- textureless
def test_textureless_step_leaves_rgbnet_alone(gpu, ckpts):
    from nerf.native_voxel_step import NativeVoxelStep
    res, ratio = 16, 0.1
    trainer, data = make_trainer(gpu, ckpts, 5, res=res)
    model = trainer.model
    for i in range(2):  # eager albedo steps: every parameter has its Adam state
        trainer.train_iteration(data.collate([i]))
    rgb = list(model.main_net.rgbnet.parameters())
    bg = list(model.bg_net.parameters())
    state = trainer.optimizer.state
    snap = copy.deepcopy([(p.detach(), state[p]["exp_avg"], state[p]["exp_avg_sq"],
                           state[p]["step"]) for p in rgb])
    bg_before = [p.detach().clone() for p in bg]
    batch = data.collate([2])
    nat = NativeVoxelStep(trainer, res, res, "textureless", ratio)
    nat.attach_optimizer(trainer.native_adam())
    assert nat.albedo is None and all(p.grad is None for p in rgb)
    nat.prologue(batch["pose"], batch["intrinsics"], 11, 1234)
    nat.body()
    torch.cuda.synchronize()
    got = [p.grad.detach().clone() for p in bg]
    pred_rgb, pred_ws, loss, keep = autograd_once(trainer, nat, batch, res, "textureless", ratio)
    compare_forward(nat, model, pred_rgb, pred_ws, keep, B_TL)
    assert all(p.grad is None for p in rgb)  # the autograd step gives rgbnet none either
    for p, g in zip(bg, got):
        assert torch.equal(p.grad, g), (tuple(p.shape), float((p.grad - g).abs().max()))
        assert float(g.abs().sum()) > 0
    # the optimizer tail of the native step
    nat.reattach()
    nat.prologue(batch["pose"], batch["intrinsics"], 11, 1234)
    nat.body()
    nat.optimizer_tail()
    torch.cuda.synchronize()
    for p, (w, m1, m2, step) in zip(rgb, snap):
        assert torch.equal(p.detach(), w)
        assert torch.equal(state[p]["exp_avg"], m1) and torch.equal(state[p]["exp_avg_sq"], m2)
        assert torch.equal(state[p]["step"].cpu(), step.cpu())
    assert all(not torch.equal(p.detach(), b) for p, b in zip(bg, bg_before))


# ---------------------------------------------------------------- graph replay
def test_graph_replayed_training(gpu, ckpts):
    from nerf.native_voxel_step import NativeVoxelStep
    trainer, data = make_trainer(gpu, ckpts, 9, graph=True, args=("--albedo_iters", "5"))
    model = trainer.model
    before = copy.deepcopy(model.state_dict())
    losses = [float(trainer.train_iteration(data.collate([i % 4]))) for i in range(40)]
    assert 1 <= len(trainer._graphs) <= 3
    for g in trainer._graphs.values():
        assert isinstance(g.native, NativeVoxelStep) and g.optimizer_in_graph
    assert all(np.isfinite(losses))
    assert model.torch_calls == 0 and model.native_step_calls == 40
    after = model.state_dict()
    for k in before:
        if k.startswith(("main_net.rgbnet.", "bg_net.")):
            assert torch.isfinite(after[k]).all() and not torch.equal(after[k], before[k]), k
    assert torch.equal(after["main_net.density"], before["main_net.density"])
    assert torch.equal(after["main_net.k0"], before["main_net.k0"])
    assert int(model.step_counter[:, 0].min()) > 0


def test_replay_equals_the_same_launches_run_eagerly(gpu, ckpts):
    """Over 10 steps of decaying learning rates through albedo and shaded
    steps: parameters, Adam state and the loss scale of the replayed graphs
    equal a twin whose steps run the same launches eagerly and the optimizer
    as the host-lr NativeAdamAmp.step()."""
    def run(hook):
        tr, dt = make_trainer(gpu, ckpts, 5, graph=True, args=("--albedo_iters", "3"))
        tr.step_hook = hook
        for i in range(10):
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        return tr

    def host_optimizer(g):
        g.optimizer_in_graph = False  # optimizer_step() then runs the host-lr Adam
        g.native.body()
        for p, gr in g.grads:
            p.grad = gr
    a = run(None)
    b = run(host_optimizer)
    assert len(a._graphs) == len(b._graphs) >= 1
    assert all(g.native is not None and g.optimizer_in_graph for g in a._graphs.values())
    lrs = [g["lr"] for g in a.optimizer.param_groups]
    assert lrs == [g["lr"] for g in b.optimizer.param_groups]
    assert lrs[0] < a.optimizer.param_groups[0]["initial_lr"]  # the schedule moved
    for pa, pb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb)
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    assert sa.keys() == sb.keys()
    for i in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][name], sb[i][name]), (i, name)
    assert float(a.scaler.get_scale()) == float(b.scaler.get_scale())
    assert torch.equal(a.model.step_counter, b.model.step_counter)


def test_ineligible_model_trains_eagerly(gpu, ckpts):
    from nerf.native_voxel_step import eligible
    trainer, data = make_trainer(gpu, ckpts, 3, graph=True, ckpt="deep")
    assert not eligible(trainer, "albedo")
    losses = [float(trainer.train_iteration(data.collate([i]))) for i in range(3)]
    assert all(np.isfinite(losses)) and trainer._graphs == {}
    assert trainer.model.native_step_calls == 0
