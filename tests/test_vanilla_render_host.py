"""Host-side checks of the vanilla backbone's fused inference renderer
(dfhip_resmlp_render_rays_infer, nerf/vanilla_field.py InferField): the header,
the binding and the dispatch hook, without a GPU."""
import ctypes

import pytest
import torch

NAME = "dfhip_resmlp_render_rays_infer"


def test_entry_is_declared_and_bound():
    """The entry is in include/dfhip.h and exported; its prototype is the
    voxel entry's ray, march, output, work and order arguments with `params`
    in place of the voxel field arguments, and _dfhip._SIGS follows the
    header."""
    import _dfhip
    from test_abi import declared_prototypes
    protos = declared_prototypes()
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_uint32: "u32",
            ctypes.c_float: "f32"}
    assert NAME in protos and NAME in _dfhip.exported_symbols()
    assert [kind[a] for a in _dfhip._SIGS[NAME]] == protos[NAME]
    voxel = protos["dfhip_voxel_render_rays_infer"]
    # N .. T_thresh | density .. act_shift (11 voxel field arguments) | params ..
    assert protos[NAME] == voxel[:13] + voxel[13 + 11:]
    assert protos[NAME][13:] == ["ptr"] * 6 + ["u32", "u32", "ptr"]
    import _resmlp
    assert callable(_resmlp.render_rays_infer)


def test_entry_rejects_bad_arguments_without_a_gpu():
    """The argument checks run before any device work."""
    import _dfhip
    lib = _dfhip.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    full = (ctypes.c_void_p * 19)(*[16] * 19)
    hole = (ctypes.c_void_p * 19)(*[16] * 7, None, *[16] * 11)

    def rc(params=full, cascades=1, H=128, max_steps=128, tile_w=0, chunk_log2=6, order=None,
           work=one, N=64):
        return lib.dfhip_resmlp_render_rays_infer(
            N, *[one] * 5, 1.0, 0.0, max_steps, cascades, H, one, 1e-4, params, *[one] * 3, work,
            order, chunk_log2, tile_w, None)

    assert rc(params=None) == 1 and b"null parameter list" in lib.dfhip_last_error()
    assert rc(params=hole) == 1 and b"parameter 7 is null" in lib.dfhip_last_error()
    assert rc(cascades=0) == 1 and b"invalid C=0" in lib.dfhip_last_error()
    assert rc(cascades=17) == 1 and b"invalid C=17" in lib.dfhip_last_error()
    assert rc(H=1) == 1 and rc(max_steps=0) == 1
    assert rc(order=one, chunk_log2=17) == 1 and b"chunk_log2" in lib.dfhip_last_error()
    assert rc(order=one, tile_w=12) == 1 and b"tile chunks" in lib.dfhip_last_error()
    assert rc(order=one, tile_w=16, N=64) == 1 and b"tile chunks" in lib.dfhip_last_error()
    assert rc(order=one, tile_w=8, chunk_log2=5) == 1 and b"tile chunks" in lib.dfhip_last_error()
    assert rc(work=None) == 1 and b"work is null" in lib.dfhip_last_error()
    assert b"resmlp_render_rays_infer" in lib.dfhip_last_error()


def test_binding_rejects_cpu_operands():
    import _resmlp
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _resmlp.render_rays_infer(z, z, z[:, 0], z[:, 0], None, 1.0, 0.0, 8, 1, 128, z, 1e-4,
                                  None, z[:, 0], z[:, 0], z, z)


def test_hook_declines_on_the_cpu_and_the_field_is_unchanged():
    """On CPU tensors native_infer_field returns None for every shading and
    autocast setting, with `native_infer` set or not, so an eval frame keeps
    the host loop; the CPU field (the sigma MLP: the encoder is a GPU kernel)
    answers the same either way and no fused frame is counted."""
    import main
    from nerf import vanilla_field
    from nerf.network import NeRFNetwork
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "vanilla"])
    torch.manual_seed(0)
    net = NeRFNetwork(opt)
    net.eval()
    assert net.native_render_calls == 0 and net.native_infer is True
    assert vanilla_field.InferField.kind == "vanilla"
    assert vanilla_field.InferField.field_bytes == 4 * 61188
    x = torch.rand(64, 3) * 2 - 1
    feats = torch.rand(64, 39) * 2 - 1
    outs = []
    for flag in (True, False):
        net.native_infer = flag
        for shading in ("albedo", "textureless", "lambertian", "normal", "phong"):
            assert net.native_infer_field(shading, x) is None
            with torch.autocast("cpu", dtype=torch.bfloat16):
                assert net.native_infer_field(shading, x) is None
            with torch.autocast("cpu", enabled=False):
                assert net.native_infer_field(shading, x) is None
        with torch.no_grad():
            outs.append(net.sigma_net(feats))
    net.native_infer = True
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    assert net.native_render_calls == 0 and net.native_calls == 0
