"""GPU tests of the vanilla backbone's native albedo train step
(nerf/native_vanilla_step.py, the device-count ResMLP entries, the opacity
regulariser's entries):

* one native step gives the live count, weights_sum and every parameter
  gradient of sigma_net and bg_net of the autograd step fed the same rays,
  noise and SDS gradient, bit for bit, and after the optimizer every
  parameter, Adam moment and the loss scale (at 16 x 16, max_steps 64, with a
  bitfield settled by occupancy refreshes, under each regulariser and both;
  at 32 x 32 and max_steps 512 with every cell occupied, more than one
  65536-row backward chunk); pred_rgb within 2^-22: the head forms image + (1 - ws) * bg with
  one contracted multiply-add where torch multiplies and adds, two half-ulp
  roundings (2^-23) on values below 2, doubled; the loss value within
  N * 2^-24 relative: torch's mean is an f32 reduction over N rays, the native
  value one rounding of a f64 sum;
* a live count that is a multiple of 128 is excluded (asserted): there the
  march's slice adds a full block of 128 zero rows, which the native step's
  row count does not (nerf/native_voxel_step.py);
* GradScaler + Adam join the graph where the native Adam takes the model's
  tensors (at most 24; this backbone has 26, so the trainer's own optimizer
  step follows each replay, as after any graph without one);
* a replay equals the same launches run eagerly; six graph-replayed
  iterations across an occupancy refresh equal six eager iterations from the
  same state and draws; native_step_calls counts the replays and torch_calls
  does not grow;
* every ineligible case keeps its present path and still trains.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B_RGB = 2.0 ** -22
MAX_STEPS = 64
CONFIGS = [(1e-3, 0.0), (0.0, 1e-4), (1e-3, 1e-4)]  # (lambda_opacity, lambda_entropy)


def make_trainer(gpu, seed, res=16, graph=False, lambdas=(1e-3, 0.0), args=(), model_kw=None,
                 bf16=False, max_steps=MAX_STEPS):
    import main
    from nerf.network import NeRFNetwork
    from nerf.provider import NeRFDataset
    from nerf.sd import InjectedSDS
    from nerf.utils import Trainer, make_adam, seed_everything
    opt = main.parse_opt(["--text", "x", "-O", *args, "--backbone", "vanilla", "--h", str(res),
                          "--w", str(res), "--max_steps", str(max_steps), "--guidance",
                          "synthetic", "--seed", str(seed)])
    assert (opt.lambda_opacity, opt.lambda_entropy) == (1e-3, 0)  # the backbone's defaults
    opt.lambda_opacity, opt.lambda_entropy = lambdas
    seed_everything(seed)
    model = NeRFNetwork(opt, **(model_kw or {}))
    optimizer = lambda m: make_adam(m.get_params(opt.lr), betas=(0.9, 0.99), eps=1e-15)  # noqa
    decay = lambda it: 0.1 ** min(it / 50, 1)  # noqa: E731  every step's lr differs in f32
    sched = lambda o: torch.optim.lr_scheduler.LambdaLR(o, decay)  # noqa: E731
    trainer = Trainer("df", opt, model, InjectedSDS(gpu, text_dim=768), device=gpu,
                      workspace=None, optimizer=optimizer, ema_decay=None, fp16=not bf16,
                      bf16=bf16, lr_scheduler=sched, scheduler_update_every_step=True,
                      use_checkpoint="scratch", mute=True, graph_step=graph)
    data = NeRFDataset(opt, device=gpu, type="train", H=res, W=res, size=100)
    trainer.model.train()
    return trainer, data


def settle(trainer, rounds=3, seed=4):
    """A few occupancy refreshes: the bitfield the field itself gives."""
    torch.manual_seed(seed)
    for _ in range(rounds):
        with torch.autocast("cuda", dtype=torch.float16):
            trainer.model.update_extra_state()
    assert int(trainer.model.density_bitfield.count_nonzero()) > 0


def autograd_step(trainer, nat, batch, res):
    """trainer.train_step + backward_only on the native step's rays, noise and
    SDS gradient, with the host-count march."""
    model = trainer.model
    trainer.optimizer.zero_grad(set_to_none=True)
    g_img = nat.g_image.view(1, 3, res, res).clone()
    trainer.guidance.sds_grad = lambda text_z, pred_rgb, *a, **k: (pred_rgb, g_img)
    model.march_noises = nat.noises.clone()
    eager = {"H": res, "W": res, "rays_o": nat.rays_o.view(1, -1, 3).clone(),
             "rays_d": nat.rays_d.view(1, -1, 3).clone(), "dir": batch["dir"]}
    text_z = trainer.text_z[batch["dir"]]
    torch_calls = model.torch_calls
    try:
        assert model.device_count_march is False
        with torch.autocast("cuda", dtype=torch.float16):
            pred_rgb, pred_ws, loss = trainer.train_step(eager, "albedo", 1.0, text_z)
        trainer.backward_only(loss)
    finally:
        del model.march_noises
        del trainer.guidance.sds_grad
    torch.cuda.synchronize()
    assert model.torch_calls == torch_calls  # the eager step ran the native field too
    return pred_rgb, pred_ws, loss


def optimizer_state(trainer):
    st = trainer.optimizer.state
    out = []
    for p in trainer.model.parameters():
        out += [p.detach().clone(), st[p]["exp_avg"].clone(), st[p]["exp_avg_sq"].clone(),
                st[p]["step"].detach().clone().cpu()]
    return out, float(trainer.scaler.get_scale())


@pytest.mark.parametrize("res, dense, lambdas", [(16, False, CONFIGS[0]), (16, False, CONFIGS[1]),
                                                 (16, False, CONFIGS[2]), (32, True, CONFIGS[0])])
def test_native_step_matches_autograd_step(gpu, res, dense, lambdas):
    from nerf.native_vanilla_step import NativeVanillaStep, eligible

    def prepared():
        # dense: the backbone's max_steps 512, so that the rays hold more than a chunk
        trainer, data = make_trainer(gpu, 3, res=res, lambdas=lambdas,
                                     max_steps=512 if dense else MAX_STEPS)
        settle(trainer)
        if dense:
            trainer.model.density_bitfield.fill_(255)
        # one eager step first: every parameter has its Adam state
        torch.manual_seed(11)
        trainer.train_iteration(data.collate([1]))
        return trainer, data
    # ---- the native step, optimizer included
    ta, data = prepared()
    assert eligible(ta, "albedo")
    nat = NativeVanillaStep(ta, res, res, "albedo", 1.0)
    adam = ta.native_adam()  # False: more tensors than the native Adam takes
    if adam:
        nat.attach_optimizer(adam)
    batch = data.collate([0])
    nat.prologue(batch["pose"], batch["intrinsics"], 11, 1234)
    before = ta.model.torch_calls
    nat.body()
    torch.cuda.synchronize()
    assert ta.model.torch_calls == before
    got = [p.grad.detach().clone() for p in ta.model.parameters()]
    if adam:
        nat.optimizer_tail()
    else:
        ta.optimizer_step()  # what follows a replay whose graph holds no optimizer
    torch.cuda.synchronize()
    live = int(nat.counter[0])
    # ---- the autograd step of a twin on the same inputs, then its optimizer
    tb, _ = prepared()
    for pa, pb in zip(ta.model.state_dict().values(), tb.model.state_dict().values()):
        assert pa.shape == pb.shape
    pred_rgb, pred_ws, loss = autograd_step(tb, nat, batch, res)
    assert live > 0 and int(tb.model.last_counter[0]) == live
    assert live % 128 != 0  # (the excluded case, see the module docstring)
    if dense:
        assert live > 65536  # more than one chunk of the field backward
    assert torch.equal(pred_ws.reshape(-1), nat.ws)
    err = float((pred_rgb.detach().float().reshape(3, -1) - nat.out_image).abs().max())
    N = res * res
    y, t = float(nat.loss), float(loss.detach())
    print(f"parity: vanilla step {res}x{res} lambdas={lambdas} live={live} pred_rgb max err "
          f"{err:.3e} (bound {B_RGB:.3e}) loss native {y:.9e} autograd {t:.9e} "
          f"(bound {N * 2.0 ** -24 * abs(t):.3e})")
    assert err <= B_RGB
    assert np.isfinite(y) and abs(y - t) <= N * 2.0 ** -24 * abs(t)
    names = [n for n, _ in tb.model.named_parameters()]
    assert any(n.startswith("sigma_net.") for n in names) and any(n.startswith("bg_net.")
                                                                  for n in names)
    for n, p, g in zip(names, tb.model.parameters(), got):
        assert torch.equal(p.grad, g), (n, float((p.grad - g).abs().max()))
        assert float(g.abs().sum()) > 0, n
    tb.optimizer_step()
    torch.cuda.synchronize()
    (sa, scale_a), (sb, scale_b) = optimizer_state(ta), optimizer_state(tb)
    for i, (a, b) in enumerate(zip(sa, sb)):
        assert torch.equal(a, b), (names[i // 4], i % 4)
    assert scale_a == scale_b


def same_training_state(a, b):
    for (n, pa), pb in zip(a.model.named_parameters(), b.model.parameters()):
        assert torch.equal(pa, pb), n
    sa, sb = a.optimizer.state_dict()["state"], b.optimizer.state_dict()["state"]
    assert sa.keys() == sb.keys()
    for i in sa:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[i][name], sb[i][name]), (i, name)
    assert float(a.scaler.get_scale()) == float(b.scaler.get_scale())
    assert torch.equal(a.model.density_bitfield, b.model.density_bitfield)


def test_replay_equals_the_same_launches_run_eagerly(gpu):
    from nerf.native_vanilla_step import NativeVanillaStep

    def run(hook):
        tr, dt = make_trainer(gpu, 5, graph=True, args=("--update_extra_interval", "4"))
        tr.step_hook = hook
        for i in range(6):
            torch.manual_seed(100 + i)
            tr.train_iteration(dt.collate([i % 4]))
        torch.cuda.synchronize()
        return tr

    def host_optimizer(g):
        g.optimizer_in_graph = False  # optimizer_step() then runs the host-lr Adam
        g.native.body()
        g.native.served()
        for p, gr in g.grads:
            p.grad = gr
    a = run(None)
    b = run(host_optimizer)
    assert len(a._graphs) == len(b._graphs) == 1
    for g in a._graphs.values():
        assert isinstance(g.native, NativeVanillaStep)
        assert g.optimizer_in_graph == bool(a.native_adam())
    assert a.model.native_step_calls == b.model.native_step_calls == 6
    same_training_state(a, b)
    assert torch.equal(a.model.step_counter, b.model.step_counter)


def test_replayed_training_equals_eager_training(gpu):
    """Six graph-replayed iterations across an occupancy refresh (steps 0 and
    4) against six eager iterations that take each step's rays, noise and SDS
    gradient from the same prologue launch."""
    from nerf.native_vanilla_step import NativeVanillaStep
    res, steps = 16, 6
    args = ("--update_extra_interval", "4")
    a, data = make_trainer(gpu, 7, graph=True, args=args)
    before = [p.detach().clone() for p in a.model.parameters()]
    calls = a.model.torch_calls
    losses = []
    for i in range(steps):
        torch.manual_seed(200 + i)
        losses.append(float(a.train_iteration(data.collate([i % 4]))))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert a.model.native_step_calls == steps and a.model.torch_calls == calls
    assert all(isinstance(g.native, NativeVanillaStep) for g in a._graphs.values())
    assert all(not torch.equal(p, q) for p, q in zip(a.model.parameters(), before))
    # ---- the eager twin
    b, data_b = make_trainer(gpu, 7, graph=False, args=args)
    draws = NativeVanillaStep(b, res, res, "albedo", 1.0)  # its prologue only
    for p in b.model.parameters():
        p.grad = None
    for i in range(steps):
        torch.manual_seed(200 + i)
        batch = data_b.collate([i % 4])
        if b.global_step % b.opt.update_extra_interval == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                b.model.update_extra_state()
        b.local_step += 1
        b.global_step += 1
        draws.prologue(batch["pose"], batch["intrinsics"],
                       int(b.opt.seed) * 1000003 + int(b.local_rank), b.global_step)
        _, _, loss = autograd_step(b, draws, batch, res)
        live = int(b.model.last_counter[0])
        assert live > 0 and live % 128 != 0, (i, live)  # (the excluded case)
        b.optimizer_step()
    torch.cuda.synchronize()
    assert b.model.native_step_calls == 0
    same_training_state(a, b)
    # the six live counts (whatever rows of step_counter the two paths file them in)
    assert torch.equal(a.model.step_counter[:, 0].sort().values,
                       b.model.step_counter[:, 0].sort().values)


# ---------------------------------------------------------------- ineligible cases
def train_three(trainer, data, moves=True):
    """Three iterations on the present path; moves: the parameters change (the
    autograd-form capture runs the field on every capacity row, and its
    GradScaler may skip these first steps: there only the path is checked)."""
    before = [p.detach().clone() for p in trainer.model.parameters()]
    losses = [float(trainer.train_iteration(data.collate([i]))) for i in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses))
    assert trainer.model.native_step_calls == 0
    if moves:
        assert any(not torch.equal(p, q) for p, q in zip(trainer.model.parameters(), before))


def test_shaded_step_runs_eagerly(gpu):
    from nerf.native_vanilla_step import eligible
    trainer, data = make_trainer(gpu, 3, graph=True)
    trainer.pick_shading = lambda: ("lambertian", 0.1)
    assert eligible(trainer, "albedo") and not eligible(trainer, "lambertian")
    train_three(trainer, data)
    assert trainer._graphs == {}


@pytest.mark.parametrize("case", ["bf16", "fused_field", "hidden64", "bg_radius", "native_step"])
def test_ineligible_albedo_configuration_keeps_its_path(gpu, case):
    from nerf.native_vanilla_step import eligible
    kw = {}
    if case == "bf16":
        kw = dict(bf16=True, args=("--bf16",))
    elif case == "hidden64":
        kw = dict(model_kw=dict(hidden_dim=64))
    elif case == "bg_radius":
        kw = dict(args=("--bg_radius", "0"))
    trainer, data = make_trainer(gpu, 3, graph=True, **kw)
    if case == "fused_field":
        trainer.model.fused_field = False
    if case == "native_step":
        trainer.native_step = False
        assert eligible(trainer, "albedo")
    else:
        assert not eligible(trainer, "albedo")
    train_three(trainer, data, moves=case == "bf16")
    for g in trainer._graphs.values():
        assert getattr(g, "native", None) is None  # never the native step
    if case == "bf16":
        assert trainer._graphs == {}  # bf16 steps run eagerly
    else:
        assert len(trainer._graphs) == 1  # the present capture (autograd form / module buckets)
