"""Host-side checks of the DVGO voxel backbone (nerf/network_dvgo.py, main.py
--backbone dvgo, the dfhip_voxel_* argument checks): no GPU needed.

The torch path is the stick of tests/test_gpu_voxel.py; here it runs on the
CPU in float32 against the float64 restatement of tests/voxel_cases.py and
must lie inside the float32 windows derived there (sigma, the unnormalised
normal and, float32 on this path, albedo, per row)."""
import numpy as np
import pytest
import torch

import voxel_cases as vc


def build(tmp_path, world=vc.WORLD_SMALL, args=(), hyper="dicts", **kw):
    import main
    sd, dim0 = vc.make_state(world, **kw)
    path = vc.save_checkpoint(tmp_path / "synthetic.dvgo", sd, hyper)
    opt = main.parse_opt(["--text", "x", "--backbone", "dvgo", "--dvgo_ckpt", path, *args])
    return main.network_class(opt)(opt), sd, dim0


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dvgo"))


def test_checkpoint_loads_with_the_reference_keys(small, tmp_path):
    net, sd, dim0 = small
    from nerf.network_dvgo import NeRFNetwork
    assert isinstance(net, NeRFNetwork)
    own = net.main_net.state_dict()
    assert list(own) == vc.expected_keys()
    assert dim0 == 72 == net.main_net.dim0
    for k in own:
        assert own[k].shape == sd[k].shape, k
        assert torch.equal(own[k].float(), sd[k].float()), k
    assert net.main_net.act_shift == pytest.approx(vc.act_shift())
    assert tuple(net.main_net.density.shape) == (1, 1, 5, 7, 6)
    assert tuple(net.main_net.k0.shape) == (1, 12, 5, 7, 6)
    assert [k for k in net.state_dict() if k.startswith("bg_net.")]
    assert net.fused_field is True
    assert net.native_calls == net.native_normal_calls == net.torch_calls == 0
    assert net.native_background_layers() is None
    assert net.native_infer_field("albedo", torch.zeros(1, 3)) is None
    # a state_dict saved by this side loads back: the keys are the reference's both ways
    from nerf.network_dvgo import load_dvgo
    torch.save(own, tmp_path / "own.dvgo")
    again, _ = load_dvgo(tmp_path / "own.dvgo", alpha_init=vc.ALPHA_INIT)
    assert list(again.state_dict()) == list(own)
    assert all(torch.equal(v, own[k]) for k, v in again.state_dict().items())


def test_loading_variants(tmp_path):
    import main
    net, _, _ = build(tmp_path, hyper=None, args=("--dvgo_alpha_init", "0.01"))
    assert net.main_net.act_shift == pytest.approx(vc.act_shift())
    with pytest.raises(ValueError, match="dvgo_alpha_init"):
        build(tmp_path, hyper=None)
    with pytest.raises(ValueError, match="--dvgo_ckpt"):
        main.network_class(main.parse_opt(["--text", "x", "--backbone", "dvgo"]))
    # namespaces instead of dicts, one level deeper
    import types
    sd, _ = vc.make_state()
    cfg = types.SimpleNamespace(fine_model_and_render=types.SimpleNamespace(alpha_init=0.05))
    path = tmp_path / "ns.dvgo"
    torch.save({"state_dict": sd, "hyper_parameters": {"hparams": {"cfg": cfg}}}, path)
    opt = main.parse_opt(["--text", "x", "--backbone", "dvgo", "--dvgo_ckpt", str(path)])
    assert main.network_class(opt)(opt).main_net.act_shift == pytest.approx(vc.act_shift(0.05))
    # the lambdas keep the grid defaults
    assert opt.lambda_opacity == 0 and opt.lambda_entropy != 0
    # other shapes load too: no encodings, a deeper MLP
    other, _, dim0 = build(tmp_path, C=4, posbase=0, viewbase=4, depth=4)
    assert dim0 == 4 + 27 == other.main_net.dim0
    assert list(other.main_net.state_dict()) == vc.expected_keys(0, 4, 4)
    with pytest.raises(ValueError, match="not a DVGO checkpoint"):
        torch.save({"state_dict": {"foo": torch.zeros(1)}}, tmp_path / "bad.dvgo")
        opt = main.parse_opt(["--text", "x", "--backbone", "dvgo", "--dvgo_ckpt",
                              str(tmp_path / "bad.dvgo")])
        main.network_class(opt)(opt)


def test_only_the_mlps_train(small):
    net, _, _ = small
    m = net.main_net
    assert m.density.requires_grad is False and m.k0.requires_grad is False
    groups = net.get_params(1e-3)
    assert [g["lr"] for g in groups] == [1e-3, 1e-3]
    got = [sorted(id(p) for p in g["params"]) for g in net.get_params(1e-3)]
    assert got == [sorted(id(p) for p in m.rgbnet.parameters()),
                   sorted(id(p) for p in net.bg_net.parameters())]
    net.zero_grad(set_to_none=True)
    x = vc.positions(200, vc.WORLD_SMALL)
    sigma, albedo = net.common_forward(x)
    assert sigma.requires_grad is False  # frozen density, leaf positions
    (albedo.sum() + net.normal(x.clone()).sum()).backward()
    assert m.density.grad is None and m.k0.grad is None
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in m.rgbnet.parameters())


def test_no_background(tmp_path):
    net, _, _ = build(tmp_path, args=("--bg_radius", "0"))
    assert net.bg_net is None and len(net.get_params(1e-3)) == 1
    assert not any(k.startswith("bg_net.") for k in net.state_dict())


@pytest.mark.parametrize("world", [vc.WORLD_SMALL, vc.WORLD_LARGE])
def test_torch_path_lies_inside_the_f32_window(tmp_path, world):
    net, sd, _ = build(tmp_path, world=world)
    x = vc.positions(600, world)
    with torch.no_grad():
        ts, ta = net.common_forward(x)
    xs = x.clone().requires_grad_(True)
    tn = -torch.autograd.grad(net._sigma(xs)[0].sum(), xs)[0]
    rs, ra, _, aux = vc.truth(sd, x)
    rn = vc.normal_of(rs, aux)
    w_sigma, w_n = vc.windows(rs, aux)
    assert ts.dtype == torch.float32 and ta.dtype == torch.float32
    inside = aux["inside"]
    assert 0.3 < float(inside.float().mean()) < 0.8
    es = (ts.double() - rs.detach()).abs()
    en = (tn.double() - rn).abs()
    print(f"parity: host sigma world={world}: max err/window {float((es / w_sigma).max()):.3f}")
    print(f"parity: host normal world={world}: max err/window "
          f"{float((en / w_n.clamp(min=1e-300))[inside].max()):.3f}")
    assert (es <= w_sigma).all()
    assert (en <= w_n).all()
    assert torch.equal(tn[~inside], torch.zeros_like(tn[~inside]))
    ea = (ta.double() - ra.detach()).abs()
    print(f"parity: host albedo world={world}: max err {float(ea.max()):.3e}, max window "
          f"{float(aux['w_albedo'].max()):.3e}")
    assert (ea <= aux["w_albedo"]).all()
    assert torch.equal(ta[~inside], torch.full_like(ta[~inside], 0.5))


def test_edge_rows(small):
    net, sd, _ = small
    rows, labels = vc.edge_rows(vc.WORLD_SMALL)
    x = torch.from_numpy(rows)
    dec = vc.restate32(rows, vc.WORLD_SMALL)
    with torch.no_grad():
        sigma, albedo = net.common_forward(x)
        pts = net.to_our_coor(x)
    xs = x.clone().requires_grad_(True)
    normal_raw = -torch.autograd.grad(net._sigma(xs)[0].sum(), xs)[0]
    unit = net.normal(x.clone())
    assert np.array_equal(pts.numpy(), dec["p"])  # the map, bit for bit
    hi, lo = np.array(vc.BOX_MAX, np.float32), np.array(vc.BOX_MIN, np.float32)
    outside_sigma = np.float32(10 * np.log1p(np.exp(vc.act_shift())))
    rs, ra, _, aux = vc.truth(sd, x)
    rn = vc.normal_of(rs, aux)
    w_sigma, w_n = vc.windows(rs, aux)
    for i, label in enumerate(labels):
        inside = bool(dec["inside"][i])
        a = int(label[-1]) if label[-1].isdigit() and not label.startswith("corner") else None
        if label.startswith("on_max"):
            assert dec["p"][i, a] == hi[a] and inside, label
            assert dec["g"][i, a] == vc.WORLD_SMALL[a] - 1  # the last voxel: a clamped corner
        elif label.startswith("on_min"):
            assert dec["p"][i, a] == lo[a] and dec["g"][i, a] == 0 and inside, label
        elif label.startswith("past_max"):
            assert dec["p"][i, a] > hi[a] and not inside, label
        elif label.startswith("before_min"):
            assert dec["p"][i, a] < lo[a] and not inside, label
        elif label.startswith("corner"):
            c = int(label[-1])
            want = np.where([c >> k & 1 for k in range(3)], hi, lo)
            assert np.array_equal(dec["p"][i], want) and inside, label
        elif label == "integer":
            assert np.array_equal(dec["cell"][i], [vc.VOXEL] * 3) and inside
            assert (dec["g"][i] - vc.VOXEL <= 2 * np.spacing(np.float32(vc.VOXEL))).all()
            assert dec["g"][i, 0] == vc.VOXEL  # exactly reachable on this axis
        elif label.startswith("integer"):
            assert dec["cell"][i, a] == vc.VOXEL and inside, label
            assert dec["g"][i, a] - vc.VOXEL <= 2 * np.spacing(np.float32(vc.VOXEL))
        elif label.startswith("below"):
            assert dec["cell"][i, a] == vc.VOXEL - 1 and inside, label
            assert vc.VOXEL - dec["g"][i, a] <= 2 * np.spacing(np.float32(vc.VOXEL))
        else:
            assert label == "zero" and inside
            assert np.array_equal(dec["p"][i], (hi + lo) / 2)
        if inside:
            assert abs(float(sigma[i]) - float(rs[i].detach())) <= float(w_sigma[i]), label
            assert ((normal_raw[i].double() - rn[i]).abs() <= w_n[i]).all(), label
            assert ((albedo[i].double() - ra[i]).abs() <= aux["w_albedo"][i]).all(), label
        else:
            assert float(sigma[i]) == pytest.approx(float(outside_sigma), rel=1e-6), label
            assert torch.equal(albedo[i], torch.full((3,), 0.5)), label
            assert torch.equal(normal_raw[i], torch.zeros(3)), label
            assert torch.equal(unit[i], torch.zeros(3)), label
    assert torch.isfinite(unit).all()
    # the value on the integer coordinates is the voxel's own (to the slope x 1 ulp)
    k = labels.index("integer")
    v = vc.VOXEL
    want = 10 * np.log1p(np.exp(float(sd["density"][0, 0, v, v, v]) + vc.act_shift()))
    assert float(sigma[k]) == pytest.approx(want, rel=1e-4)


@pytest.mark.parametrize("axis, world_axis", [(0, 0), (1, 2), (2, 1)])
def test_single_axis_volume_gives_a_normal_along_one_world_axis(tmp_path, axis, world_axis):
    """Density rising along one grid axis only: the normal points down that
    axis in world coordinates (grid y is world z), and nowhere else.  On the
    non-cubic world (5, 7, 6) a swapped, flipped or mis-strided axis fails."""
    shape = [1, 1, 1, 1, 1]
    shape[2 + axis] = vc.WORLD_SMALL[axis]
    ramp = torch.arange(vc.WORLD_SMALL[axis], dtype=torch.float32).reshape(shape)
    density = ramp.expand(1, 1, *vc.WORLD_SMALL).contiguous() * 0.7 - 1.0
    net, sd, _ = build(tmp_path, density=density)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(64, 3, generator=g) * 2 - 1) * 0.75  # all inside
    n = net.normal(x.clone())
    want = torch.zeros(64, 3)
    want[:, world_axis] = -1.0
    assert torch.allclose(n, want, atol=1e-5)
    # sigma follows the ramp: larger further along the axis
    hi, lo = x.clone(), x.clone()
    hi[:, world_axis], lo[:, world_axis] = 0.5, -0.5
    with torch.no_grad():
        assert (net.common_forward(hi)[0] > net.common_forward(lo)[0]).all()


def test_weight_argument_keeps_the_reference_meaning(small):
    net, _, _ = small
    x = vc.positions(100, vc.WORLD_SMALL)
    shift = net.main_net.act_shift
    weight = torch.full((100,), 1e-2 + shift - 1.0)  # at or below the threshold: default albedo
    weight[::2] = 1e-2 + shift + 1.0
    with torch.no_grad():
        sigma, albedo = net.common_forward(x, weight)
        full_sigma, full = net.common_forward(x)
    assert torch.equal(sigma, full_sigma)
    assert torch.equal(albedo[1::2], torch.full_like(albedo[1::2], 0.5))
    assert torch.equal(albedo[::2], full[::2])


def test_voxel_queries_without_a_gpu():
    import _dfhip
    import _voxelfield
    lib = _dfhip.load()
    assert _voxelfield.ROW_TILE == 16 and _voxelfield.WORKGROUP_ROWS % _voxelfield.ROW_TILE == 0
    for m in (0, 1, 1000, 1 << 20):
        assert _voxelfield.backward_scratch_bytes(m, 72) > 0
    assert _voxelfield.backward_scratch_bytes(1 << 20, 72) == \
        _voxelfield.backward_scratch_bytes(1 << 24, 72)
    assert _voxelfield.backward_scratch_bytes(1000, 96) > _voxelfield.backward_scratch_bytes(1000, 31)
    # argument checks run before any device work
    import ctypes
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    rc = lib.dfhip_voxel_field_forward(None, None, None, 5, 7, 6, 12, 5, None, 27, box, 1.0, -4.6,
                                       None, None, 1, 4, None)
    assert rc == 1 and b"null parameter list" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_field_forward(None, None, None, 5, 7, 6, 60, 5, None, 27, box, 1.0, -4.6,
                                       None, None, 1, 4, None)
    assert rc == 1 and b"feature row" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_normal(None, None, 0, 7, 6, box, 1.0, -4.6, None, 4, None)
    assert rc == 1 and b"voxels" in lib.dfhip_last_error()
    bad = (ctypes.c_float * 6)(1, 1, 1, -1, -1, -1)
    rc = lib.dfhip_voxel_normal(None, None, 5, 7, 6, bad, 1.0, -4.6, None, 4, None)
    assert rc == 1 and b"box_max" in lib.dfhip_last_error()
    assert lib.dfhip_voxel_normal(None, None, 5, 7, 6, box, 1.0, -4.6, None, 0, None) == 0
