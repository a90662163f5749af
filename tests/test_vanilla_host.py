"""Host-side checks of the vanilla backbone (nerf/network.py, main.py
--backbone vanilla, the dfhip_resmlp_* queries): no GPU needed."""
import pytest
import torch

H, IN = 128, 39

# sigma_net.* / bg_net.* of the reference's vanilla network (network.py:13-94)
SIGMA_KEYS = (
    [("sigma_net.net.0.dense.weight", (H, IN)), ("sigma_net.net.0.dense.bias", (H,)),
     ("sigma_net.net.0.norm.weight", (H,)), ("sigma_net.net.0.norm.bias", (H,)),
     ("sigma_net.net.0.skip.weight", (H, IN))]
    + [(f"sigma_net.net.{l}.{n}", s) for l in (1, 2, 3)
       for n, s in (("dense.weight", (H, H)), ("dense.bias", (H,)), ("norm.weight", (H,)),
                    ("norm.bias", (H,)))]
    + [("sigma_net.net.4.weight", (4, H)), ("sigma_net.net.4.bias", (4,))])
BG_KEYS = [("bg_net.net.0.dense.weight", (64, IN)), ("bg_net.net.0.dense.bias", (64,)),
           ("bg_net.net.0.norm.weight", (64,)), ("bg_net.net.0.norm.bias", (64,)),
           ("bg_net.net.0.skip.weight", (64, IN)), ("bg_net.net.1.weight", (3, 64)),
           ("bg_net.net.1.bias", (3,))]


def test_cli_selects_the_vanilla_backbone():
    import main
    from nerf.network import NeRFNetwork as Vanilla
    from nerf.network_grid import NeRFNetwork as Grid
    opt = main.parse_opt(["--text", "x", "--backbone", "vanilla"])
    assert opt.lambda_entropy == 0 and opt.lambda_opacity == 1e-3
    assert main.network_class(opt) is Vanilla
    default = main.parse_opt(["--text", "x"])
    assert main.network_class(default) is Grid
    assert default.lambda_opacity == 0 and default.lambda_entropy != 0
    with pytest.raises(NotImplementedError):
        main.network_class(main.parse_opt(["--text", "x", "--backbone", "foo"]))


def test_module_shapes_and_parameter_groups():
    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "--backbone", "vanilla"])
    net = NeRFNetwork(opt)
    sd = net.state_dict()
    got = [(k, tuple(v.shape)) for k, v in sd.items()
           if k.startswith(("sigma_net.", "bg_net."))]
    assert got == SIGMA_KEYS + BG_KEYS  # names, shapes and creation order
    count = lambda m: sum(p.numel() for p in m.parameters())  # noqa: E731
    assert count(net.sigma_net) == 61188 and count(net.bg_net) == 5379
    assert [count(b) for b in net.sigma_net.net] == [10368, 16768, 16768, 16768, 516]
    assert [count(b) for b in net.bg_net.net] == [5184, 195]
    assert not list(net.encoder.parameters())
    groups = net.get_params(1e-3)
    assert [g["lr"] for g in groups] == [1e-3, 1e-3]
    assert [sum(p.numel() for p in g["params"]) for g in groups] == [61188, 5379]
    assert net.fused_field is True
    assert net.native_background_layers() is None
    assert net.native_infer_field("albedo", torch.zeros(1, 3)) is None
    # the sigma MLP alone runs on the CPU (the encoder is a GPU kernel)
    assert net.sigma_net(torch.zeros(5, IN).uniform_(-1, 1)).shape == (5, 4)
    assert net.native_calls == net.native_normal_calls == net.torch_calls == 0
    nobg = NeRFNetwork(main.parse_opt(["--text", "x", "--backbone", "vanilla", "--bg_radius",
                                       "0"]))
    assert nobg.bg_net is None
    assert not any(k.startswith("bg_net.") for k in nobg.state_dict())
    assert len(nobg.get_params(1e-3)) == 1


def test_seeded_initialisation_follows_creation_order():
    """Same seed, same creation order as the reference's ResBlock / MLP:
    dense, norm, skip per block, sigma_net before bg_net."""
    import torch.nn as nn

    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "--backbone", "vanilla"])
    torch.manual_seed(3)
    net = NeRFNetwork(opt)
    torch.manual_seed(3)
    dense, skip = nn.Linear(IN, H), None
    nn.LayerNorm(H)
    skip = nn.Linear(IN, H, bias=False)
    assert torch.equal(net.sigma_net.net[0].dense.weight, dense.weight)
    assert torch.equal(net.sigma_net.net[0].skip.weight, skip.weight)


def test_resmlp_queries_without_a_gpu():
    import _dfhip
    import _resmlp
    lib = _dfhip.load()
    assert lib.dfhip_resmlp_params() == 61188 == _resmlp.params_count()
    assert sum(torch.Size(s).numel() for s in _resmlp.SHAPES) == 61188
    for m in (0, 1, 1000, 1 << 20):
        assert _resmlp.backward_scratch_bytes(m) > 0
    assert _resmlp.backward_scratch_bytes(1 << 20) == _resmlp.backward_scratch_bytes(1 << 24)
    # argument checks run before any device work
    assert lib.dfhip_resmlp_field_forward(None, None, None, None, 4, None) == 1
    assert b"null parameter list" in lib.dfhip_last_error()
    assert _resmlp.ROW_TILE == 16 and _resmlp.WORKGROUP_ROWS % _resmlp.ROW_TILE == 0
