"""Host-side checks of the vanilla backbone's native train step
(nerf/native_vanilla_step.py, the dfhip_resmlp_*_dev and dfhip_opacity_*
entries): no GPU needed.

eligible() is a chain of refusals; the option cases run it on stub objects
around a real (CPU) vanilla model, with the one check that needs the GPU (the
device of the trained parameters) stubbed, so every excluded option is seen
to flip an otherwise eligible trainer."""
import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["dfhip_resmlp_field_forward_dev", "dfhip_resmlp_field_backward_dev",
           "dfhip_resmlp_field_backward_dev_scratch", "dfhip_opacity_forward",
           "dfhip_opacity_backward_accumulate"]


def make_net(*args):
    import main
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla", *args])
    torch.manual_seed(0)
    return main.network_class(opt)(opt), opt


@pytest.fixture(scope="module")
def net():
    return make_net()


def stub_trainer(net, **changes):
    """A trainer-shaped object on which eligible() says yes once the device
    check is stubbed out."""
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


def test_the_backbone_defaults_and_a_cpu_trainer_is_not_served(net):
    from nerf import native_vanilla_step as nv
    model, opt = net
    assert opt.lambda_opacity == 1e-3 and opt.lambda_entropy == 0 and opt.max_steps == 512
    assert nv.serves(model) and not nv.serves(torch.nn.Linear(2, 2))
    assert nv.eligible(stub_trainer(net), "albedo") is False  # parameters on the CPU
    assert nv._trained_device(model) is None
    assert nv.ALIGN == 128
    assert model.native_step_calls == 0


def test_eligible_truth_table(net, monkeypatch):
    from nerf import native_vanilla_step as nv
    monkeypatch.setattr(nv, "_trained_device", lambda m: torch.device("cpu"))
    assert nv.eligible(stub_trainer(net), "albedo") is True
    for shading in ("textureless", "lambertian", "normal"):
        assert nv.eligible(stub_trainer(net), shading) is False
    # each regulariser may be zero or positive; orient / smooth play no part
    for change in (dict(lambda_opacity=0.0, lambda_entropy=1e-4),
                   dict(lambda_opacity=1e-3, lambda_entropy=1e-4),
                   dict(lambda_opacity=0.0, lambda_entropy=0.0),
                   dict(lambda_orient=1e-2), dict(lambda_smooth=1e-2)):
        assert nv.eligible(stub_trainer(net, **change), "albedo") is True, change
    for change in (dict(fp16=False), dict(fp16=False, bf16=True), dict(bf16=True),
                   dict(fused_backward=False), dict(world_size=2), dict(guidance=object())):
        assert nv.eligible(stub_trainer(net, **change), "albedo") is False, change
    model = net[0]
    for attr, value in (("cuda_ray", False), ("bg_radius", 0.0), ("bg_net", None),
                        ("fused_field", False)):
        saved = getattr(model, attr)
        setattr(model, attr, value)
        try:
            assert nv.eligible(stub_trainer(net), "albedo") is False, attr
        finally:
            setattr(model, attr, saved)
    assert nv.eligible(stub_trainer(net), "albedo") is True
    # the stubbed check declines on its own
    monkeypatch.setattr(nv, "_trained_device", lambda m: None)
    assert nv.eligible(stub_trainer(net), "albedo") is False
    monkeypatch.setattr(nv, "_trained_device", lambda m: torch.device("cpu"))
    # another width is not the native field's; another model is not this step's
    import main
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla"])
    narrow = NeRFNetwork(opt, hidden_dim=64)
    assert nv.eligible(stub_trainer((narrow, opt)), "albedo") is False
    other = stub_trainer(net)
    other.model = torch.nn.Linear(2, 2)
    assert nv.eligible(other, "albedo") is False


def test_header_declares_and_python_binds_the_new_entries():
    import _dfhip
    import _resmlp
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dfhip.h").read_text(), flags=re.S)
    lib = _dfhip.load()
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name) and name in _dfhip.exported_symbols(), name
        if not name.endswith("_scratch"):
            assert name in _dfhip._SIGS
    for fn in ("field_forward_dev", "field_backward_dev", "backward_dev_scratch_bytes"):
        assert callable(getattr(_resmlp, fn))


def test_scratch_formula_at_the_worked_sizes():
    import _resmlp
    per_sample = 53 * 64 * 16 // 16 + (64 + 512 + 656) * 2  # 3392 tile state + 2464 f16 rows
    per_chunk = 64 * 61188 * 4 + 256 * 4 * 2 * 128 * 4
    assert per_sample == 3392 + 2464

    def formula(cap):
        return -(-cap // 32) * 32 * per_sample + -(-cap // 65536) * per_chunk
    assert _resmlp.backward_dev_scratch_bytes(131072) == formula(131072) == 800983040
    assert _resmlp.backward_dev_scratch_bytes(64 * 64 * 512) == formula(2097152) == 12815728640
    for cap in (1, 33, 65536, 65537, 65536 + 256, 16384):
        assert _resmlp.backward_dev_scratch_bytes(cap) == formula(cap), cap
    assert _resmlp.backward_dev_scratch_bytes(0) > 0


def test_argument_errors_without_a_gpu():
    import _dfhip
    lib = _dfhip.load()
    one = ctypes.c_int32(0)
    m_dev = ctypes.addressof(one)  # never dereferenced: the checks come first
    buf = (ctypes.c_char * 64)()
    p = -(-ctypes.addressof(buf) // 16) * 16  # a 16-byte aligned stand-in, never dereferenced
    full = (ctypes.c_void_p * 19)(*([p] * 19))
    hole = (ctypes.c_void_p * 19)(*([p] * 7 + [None] + [p] * 11))
    fwd, bwd = lib.dfhip_resmlp_field_forward_dev, lib.dfhip_resmlp_field_backward_dev
    # forward
    assert fwd(None, None, None, None, 4, m_dev, 128, None) == 1
    assert b"null parameter list" in lib.dfhip_last_error()
    assert fwd(None, hole, None, None, 4, m_dev, 128, None) == 1
    assert b"parameter 7 is null" in lib.dfhip_last_error()
    assert fwd(None, full, None, None, 4, None, 128, None) == 1
    assert b"m_dev is null" in lib.dfhip_last_error()
    assert fwd(None, full, None, None, 4, m_dev, 0, None) == 1
    assert b"align must be at least 1" in lib.dfhip_last_error()
    assert fwd(None, full, None, None, 1 << 31, m_dev, 1, None) == 1
    assert b"capacity" in lib.dfhip_last_error()
    assert fwd(None, full, None, None, 4, m_dev, 1, None) == 1
    assert b"null pointer" in lib.dfhip_last_error()
    assert fwd(None, full, None, None, 0, m_dev, 1, None) == 0  # nothing to do, no launch
    # backward: xyz, params, grad_sigma, grad_albedo, dtype, cap, m_dev, align, scratch, grads, acc
    f32, f16, bf16 = 0, 1, 3  # enum dfhip_dtype
    assert bwd(None, None, None, None, f16, 4, m_dev, 128, p, full, 0, None) == 1
    assert b"null parameter list" in lib.dfhip_last_error()
    assert bwd(None, hole, None, None, f16, 4, m_dev, 128, p, full, 0, None) == 1
    assert b"parameter 7 is null" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, m_dev, 128, p, None, 0, None) == 1
    assert b"null gradient list" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f32, 4, m_dev, 128, p, hole, 0, None) == 1
    assert b"gradient 7 is null" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, bf16, 4, m_dev, 128, p, full, 0, None) == 2
    assert b"dtype must be f16 or f32" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, None, 128, p, full, 0, None) == 1
    assert b"m_dev is null" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, m_dev, 0, p, full, 0, None) == 1
    assert b"align must be at least 1" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 1 << 31, m_dev, 1, p, full, 0, None) == 1
    assert b"capacity" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, m_dev, 1, None, full, 0, None) == 1
    assert b"scratch must be a 16-byte aligned" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, m_dev, 1, p + 8, full, 0, None) == 1
    assert b"scratch must be a 16-byte aligned" in lib.dfhip_last_error()
    assert bwd(None, full, None, None, f16, 4, m_dev, 1, p, full, 0, None) == 1
    assert b"null pointer" in lib.dfhip_last_error()
    # the opacity entries: empty is a no-op, null pointers are refused
    assert lib.dfhip_opacity_forward(0, None, 1e-3, None, 0, None) == 0
    assert lib.dfhip_opacity_backward_accumulate(0, None, None, 1e-3, None, None) == 0
    assert lib.dfhip_opacity_forward(4, None, 1e-3, None, 0, None) == 1
    assert b"opacity_forward: null pointer" in lib.dfhip_last_error()
    assert lib.dfhip_opacity_backward_accumulate(4, p, None, 1e-3, p, None) == 1
    assert b"opacity_backward_accumulate: null pointer" in lib.dfhip_last_error()
