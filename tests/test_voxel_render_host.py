"""Host-side checks of the DVGO backbone's fused inference renderer
(dfhip_voxel_render_rays_infer[_shaded], nerf/voxel_field.py InferField): the
header, the binding and the dispatch hook, without a GPU."""
import ctypes

import pytest
import torch

import voxel_cases as vc

NAMES = ("dfhip_voxel_render_rays_infer", "dfhip_voxel_render_rays_infer_shaded")


def test_entries_are_declared_and_bound():
    """Both entries are in include/dfhip.h; their ray, march, order and output
    arguments are dfhip_render_rays_infer_ordered's, their field arguments
    dfhip_voxel_field_forward's (bound given once, no xyz / outputs / M), and
    _dfhip._SIGS follows the header."""
    import _dfhip
    from test_abi import declared_prototypes
    protos = declared_prototypes()
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_uint32: "u32",
            ctypes.c_float: "f32"}
    for name in NAMES:
        assert name in protos and name in _dfhip.exported_symbols()
        assert [kind[a] for a in _dfhip._SIGS[name]] == protos[name], name
    ordered = protos["dfhip_render_rays_infer_ordered"]
    field = protos["dfhip_voxel_field_forward"]
    # N .. T_thresh, then density .. box (xyz dropped), act_shift (bound dropped),
    # params, then weights_sum .. work, order, chunk_log2, tile_w, stream
    want = ordered[:13] + field[1:11] + field[12:14] + ["ptr"] * 4 + ["ptr", "u32", "u32", "ptr"]
    assert protos[NAMES[0]] == want
    assert protos[NAMES[1]] == want[:-1] + ["i32", "ptr", "f32", "ptr"]


def test_entries_reject_bad_arguments_without_a_gpu():
    """The argument checks run before any device work."""
    import _dfhip
    lib = _dfhip.load()
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    box = (ctypes.c_float * 6)(*vc.BOX_MIN, *vc.BOX_MAX)
    params = (ctypes.c_void_p * 6)(*[16] * 6)

    def rc(shaded, shading=2, light=one, Nx=5, C=12, cascades=1, tile_w=0, chunk_log2=6,
           order=None, box=box):
        args = [64, *[one] * 5, 1.0, 0.0, 128, cascades, 128, one, 1e-4, one, one, Nx, 7, 6, C, 5,
                one, 27, box, -4.6, params, *[one] * 4, order, chunk_log2, tile_w]
        if shaded:
            return lib.dfhip_voxel_render_rays_infer_shaded(*args, shading, light, 0.1, None)
        return lib.dfhip_voxel_render_rays_infer(*args, None)

    assert rc(True, light=None) == 1 and b"light is NULL" in lib.dfhip_last_error()
    assert rc(True, shading=7) == 1 and b"shading must be" in lib.dfhip_last_error()
    assert rc(True, shading=0) == 1
    assert b"dfhip_voxel_render_rays_infer's" in lib.dfhip_last_error()
    for shaded in (False, True):
        assert rc(shaded, Nx=0) == 1 and b"voxels" in lib.dfhip_last_error()
        assert rc(shaded, C=60) == 1 and b"feature row" in lib.dfhip_last_error()
        assert rc(shaded, cascades=0) == 1 and b"invalid C=0" in lib.dfhip_last_error()
        assert rc(shaded, box=None) == 1 and b"box is null" in lib.dfhip_last_error()
        assert rc(shaded, order=one, tile_w=12) == 1 and b"tile chunks" in lib.dfhip_last_error()
        assert rc(shaded, order=one, chunk_log2=17) == 1 and b"chunk_log2" in lib.dfhip_last_error()
    # the textureless and normal views read no colour: their feature row is not checked
    assert rc(True, shading=1, C=60, Nx=0) == 1 and b"voxels" in lib.dfhip_last_error()


def test_binding_rejects_cpu_operands():
    import _voxelfield
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _voxelfield.render_rays_infer(z, z, z[:, 0], z[:, 0], None, 1.0, 0.0, 8, 1, 128, z, 1e-4,
                                      None, -4.6, None, z[:, 0], z[:, 0], z, z)
    assert _voxelfield.SHADINGS == {"albedo": 0, "textureless": 1, "lambertian": 2, "normal": 3}


def test_hook_declines_on_the_cpu_and_the_field_is_unchanged(tmp_path):
    """On CPU tensors native_infer_field returns None for every shading and
    autocast setting, so an eval frame keeps the host loop; the field the loop
    calls answers as before, with `native_infer` set or not, and counts no
    fused frame.  (A whole CPU frame cannot run: the ray ops have no CPU form.)"""
    import main
    sd, _ = vc.make_state()
    path = vc.save_checkpoint(tmp_path / "small.dvgo", sd)
    opt = main.parse_opt(["--text", "x", "-O", "--backbone", "dvgo", "--dvgo_ckpt", path])
    net = main.network_class(opt)(opt)
    net.eval()
    assert net.native_render_calls == 0 and net.native_infer is True
    x = vc.positions(64, vc.WORLD_SMALL)
    for shading in ("albedo", "textureless", "lambertian", "normal", "phong"):
        assert net.native_infer_field(shading, x) is None
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert net.native_infer_field(shading, x) is None
    d = torch.nn.functional.normalize(vc.positions(64, vc.WORLD_SMALL, seed=1, edges=False), dim=-1)
    light = torch.nn.functional.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
    outs = []
    for flag in (True, False):
        net.native_infer = flag
        outs.append(net(x.clone(), d, light, ratio=0.1, shading="lambertian"))
    net.native_infer = True
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    rs, ra, _, aux = vc.truth(sd, x)
    assert float((outs[0][0].double() - rs.detach()).abs().max()) < 1e-4
    assert net.native_render_calls == 0 and net.native_calls == 0 and net.torch_calls > 0
