"""Host-side checks of the DVGO backbone's native train step
(nerf/native_voxel_step.py, the dfhip_voxel_*_dev entries): no GPU needed.

eligible() is a chain of refusals; the option cases run it on stub objects
around a real (CPU) dvgo model, with the model's own share of the decision
(voxel_field.model_eligible, which needs the GPU) stubbed to True, so every
excluded option is seen to flip an otherwise eligible trainer."""
import re
import types
from pathlib import Path

import pytest
import torch

import voxel_cases as vc

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["dfhip_voxel_field_forward_dev", "dfhip_voxel_normal_dev",
           "dfhip_voxel_field_backward_dev", "dfhip_voxel_field_backward_dev_scratch"]


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    import main
    sd, _ = vc.make_state()
    path = vc.save_checkpoint(tmp_path_factory.mktemp("dvgo") / "synthetic.dvgo", sd)
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
    return main.network_class(opt)(opt), opt


def stub_trainer(net, **changes):
    """A trainer-shaped object on which eligible() says yes once the model's
    device checks are stubbed out."""
    from nerf.sd import InjectedSDS
    model, opt = net
    guidance = InjectedSDS.__new__(InjectedSDS)  # the type is all eligible() reads
    t = types.SimpleNamespace(model=model, opt=types.SimpleNamespace(**vars(opt)),
                              guidance=guidance, fused_backward=True, fp16=True, bf16=False,
                              world_size=1, device=torch.device("cpu"))
    for k, v in changes.items():
        target = t.opt if k.startswith("lambda_") else t
        setattr(target, k, v)
    return t


def test_module_imports_and_a_cpu_trainer_is_not_served(net):
    from nerf import native_voxel_step as nv
    assert nv.serves(net[0]) and not nv.serves(torch.nn.Linear(2, 2))
    for shading in ("albedo", "textureless", "lambertian"):
        assert nv.eligible(stub_trainer(net), shading) is False  # parameters on the CPU
    assert nv.ALIGN == 128 and set(nv.SHADINGS) == {"albedo", "textureless", "lambertian"}


def test_each_excluded_option_declines(net, monkeypatch):
    from nerf import native_voxel_step as nv
    from nerf import voxel_field as vf
    # the two checks that need the GPU, stubbed to yes
    monkeypatch.setattr(vf, "model_eligible", lambda m, device: True)
    monkeypatch.setattr(nv, "_trained_device", lambda m: torch.device("cpu"))
    assert nv.eligible(stub_trainer(net), "albedo") is True
    assert nv.eligible(stub_trainer(net), "textureless") is True
    assert nv.eligible(stub_trainer(net), "lambertian") is True
    assert nv.eligible(stub_trainer(net), "normal") is False
    for change in (dict(fp16=False), dict(fp16=False, bf16=True), dict(fused_backward=False),
                   dict(world_size=2), dict(lambda_opacity=1e-3), dict(lambda_smooth=1e-2),
                   dict(guidance=object())):
        assert nv.eligible(stub_trainer(net, **change), "albedo") is False, change
    model = net[0]
    for attr, value in (("cuda_ray", False), ("bg_radius", 0.0)):
        saved = getattr(model, attr)
        setattr(model, attr, value)
        try:
            assert nv.eligible(stub_trainer(net), "albedo") is False, attr
        finally:
            setattr(model, attr, saved)
    assert nv.eligible(stub_trainer(net), "albedo") is True
    # each of the stubbed checks declines on its own
    monkeypatch.setattr(vf, "model_eligible", lambda m, device: False)
    assert nv.eligible(stub_trainer(net), "albedo") is False
    monkeypatch.setattr(vf, "model_eligible", lambda m, device: True)
    monkeypatch.setattr(nv, "_trained_device", lambda m: None)
    assert nv.eligible(stub_trainer(net), "albedo") is False
    monkeypatch.setattr(nv, "_trained_device", lambda m: torch.device("cpu"))
    # a grid model is not this step's
    other = stub_trainer(net)
    other.model = torch.nn.Linear(2, 2)
    assert nv.eligible(other, "albedo") is False


def test_model_eligible_is_the_model_share_of_the_field_dispatch(net):
    from nerf import voxel_field as vf
    from nerf import native_voxel_step as nv
    model = net[0]
    assert nv._trained_device(model) is None  # trained parameters on the CPU
    assert vf.model_eligible(model, torch.device("cpu")) is False  # no native operands on the CPU
    model.fused_field = False
    try:
        assert vf.model_eligible(model, torch.device("cpu")) is False
    finally:
        model.fused_field = True
    assert model.native_step_calls == 0


def test_header_declares_and_python_binds_the_new_entries():
    import _dfhip
    import _voxelfield
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfhip.h").read_text(), flags=re.S)
    lib = _dfhip.load()
    for name in ENTRIES + ["dfhip_voxel_shade_train_forward", "dfhip_voxel_shade_train_backward"]:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name) and name in _dfhip.exported_symbols(), name
    for name in ENTRIES:
        if not name.endswith("_scratch"):
            assert name in _dfhip._SIGS
    for fn in ("field_forward_dev", "normal_dev", "field_backward_dev",
               "backward_dev_scratch_bytes", "shade_train_forward", "shade_train_backward"):
        assert callable(getattr(_voxelfield, fn))


def test_dev_queries_and_argument_checks_without_a_gpu():
    import ctypes
    import _dfhip
    import _voxelfield
    lib = _dfhip.load()
    # 616 rows x 2 bytes per padded sample + 64 partial images per 65536 rows
    per_chunk = 64 * 4 * (128 * 72 + 17027)
    assert _voxelfield.backward_dev_scratch_bytes(64 * 64 * 512, 72) == 2798673920
    assert _voxelfield.backward_dev_scratch_bytes(128 * 128 * 512, 72) == 11194695680
    assert _voxelfield.backward_dev_scratch_bytes(33, 72) == 616 * 2 * 64 + per_chunk
    assert _voxelfield.backward_dev_scratch_bytes(65537, 72) == 616 * 2 * 65568 + 2 * per_chunk
    assert _voxelfield.backward_dev_scratch_bytes(0, 72) > 0
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    one = ctypes.c_int32(0)
    m_dev = ctypes.addressof(one)  # never dereferenced: the checks come first
    rc = lib.dfhip_voxel_field_forward_dev(None, None, None, 5, 7, 6, 12, 5, None, 27, box, 1.0,
                                           -4.6, None, None, None, 4, None, 128, None)
    assert rc == 1 and b"m_dev is null" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_normal_dev(None, None, 5, 7, 6, box, 1.0, -4.6, None, 4, m_dev, 0, None)
    assert rc == 1 and b"align must be at least 1" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_normal_dev(None, None, 5, 7, 6, box, 1.0, -4.6, None, 1 << 31, m_dev, 1,
                                    None)
    assert rc == 1 and b"capacity" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_normal_dev(None, None, 5, 7, 6, box, 1.0, -4.6, None, 4, m_dev, 1, None)
    assert rc == 1 and b"null pointer" in lib.dfhip_last_error()
    assert lib.dfhip_voxel_normal_dev(None, None, 5, 7, 6, box, 1.0, -4.6, None, 0, m_dev, 1,
                                      None) == 0
    rc = lib.dfhip_voxel_field_backward_dev(None, None, 5, 7, 6, 12, 5, None, 27, box, 1.0, None,
                                            None, 1, 4, m_dev, 128, None, None, 0, None)
    assert rc == 1 and b"null parameter list" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_shade_train_forward(None, None, None, 5, 7, 6, box, 1.0, -4.6, None, None,
                                             0.1, 0, 4, m_dev, 128, None, None, None, None, None,
                                             None)
    assert rc == 1 and b"shading must be" in lib.dfhip_last_error()
    rc = lib.dfhip_voxel_shade_train_backward(None, None, 3, 4, m_dev, 128, None, None)
    assert rc == 1 and b"shading must be" in lib.dfhip_last_error()
    # a textureless step has no albedo gradient: no launch, no pointer needed
    assert lib.dfhip_voxel_shade_train_backward(None, None, 1, 4, m_dev, 128, None, None) == 0
