"""Host pieces of the shaded inference render (no GPU): the GUI's light
angles, the eval batch's shading keys and the new entry point's binding."""
import ctypes

import numpy as np
import pytest


def test_light_from_angles():
    """(theta, phi) in degrees -> (sin t sin p, cos t, sin t cos p) as float32
    (reference utils.py:628-633).  cos(pi / 2) is 6e-17 in f64, far below the
    f32 spacing at 1, so the axis cases are exact to 1e-7."""
    from nerf.utils import light_from_angles
    for phi in (0.0, 37.0, 90.0, 250.0):
        v = light_from_angles((0.0, phi))
        assert v.dtype == np.float32 and v.shape == (3,)
        np.testing.assert_allclose(v, [0.0, 1.0, 0.0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(light_from_angles((90.0, 0.0)), [0.0, 0.0, 1.0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(light_from_angles((90.0, 90.0)), [1.0, 0.0, 0.0], rtol=0,
                               atol=1e-7)
    # a general direction against the formula in f64, and unit length
    t, p = np.deg2rad(60.0), np.deg2rad(30.0)
    want = np.array([np.sin(t) * np.sin(p), np.cos(t), np.sin(t) * np.cos(p)])
    got = light_from_angles(np.array([60.0, 30.0]))
    np.testing.assert_allclose(got, want, rtol=0, atol=2.0 ** -24)
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-6


def test_eval_batch_shading_keys():
    """The keys test_step / eval_step read, with the albedo view as default."""
    from nerf.utils import Trainer
    assert Trainer._view_shading({}) == ("albedo", 1.0, None)
    light = object()
    data = {"shading": "normal", "ambient_ratio": 0.3, "light_d": light}
    assert Trainer._view_shading(data) == ("normal", 0.3, light)
    for name in ("eval_step", "test_step", "test_gui"):
        assert callable(getattr(Trainer, name))


def test_shaded_entry_is_bound_and_declared():
    """dfhip_render_rays_infer_shaded: the header's prototype is the ordered
    entry's with (int shading, const float *light, float ratio, float eps)
    before prof, and _dfhip._SIGS follows it."""
    import _dfhip
    from test_abi import declared_prototypes
    protos = declared_prototypes()
    shaded = protos["dfhip_render_rays_infer_shaded"]
    ordered = protos["dfhip_render_rays_infer_ordered"]
    assert shaded == ordered[:-2] + ["i32", "ptr", "f32", "f32"] + ordered[-2:]
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_uint32: "u32",
            ctypes.c_float: "f32"}
    assert [kind[a] for a in _dfhip._SIGS["dfhip_render_rays_infer_shaded"]] == shaded


def test_shaded_entry_rejects_bad_arguments_without_a_gpu():
    """The shading checks run before any device work."""
    import _dfhip
    lib = _dfhip.load()
    fn = lib.dfhip_render_rays_infer_shaded
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first

    def rc(shading, light, bound=1.0, eps=1e-2):
        return fn(64, *[one] * 5, bound, 0.0, 128, 1, 128, one, 1e-4, one, one, 16, 0.5, 16, 0,
                  0, *[one] * 11, None, 6, 0, shading, light, 0.1, eps, None, None)
    assert rc(2, None) == 1 and b"light is NULL" in lib.dfhip_last_error()
    assert rc(7, one) == 1 and b"shading must be" in lib.dfhip_last_error()
    assert rc(-1, one) == 1 and b"shading must be" in lib.dfhip_last_error()
    assert rc(0, one) == 1
    assert b"dfhip_render_rays_infer_ordered" in lib.dfhip_last_error()
    assert rc(3, one, bound=0.0) == 1 and b"bound must be > 0" in lib.dfhip_last_error()
    assert rc(1, one, eps=0.0) == 1 and b"eps must be > 0" in lib.dfhip_last_error()


def test_binding_rejects_cpu_operands():
    import torch
    import _fieldmlp
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _fieldmlp.render_rays_infer_shaded(z, z, z[:, 0], z[:, 0], None, 1.0, 0.0, 8, 1, 128, z,
                                           1e-4, z, z, 0.5, 16, 0, False, [z] * 6, z[:, 0],
                                           z[:, 0], z, z, "lambertian", z[0], 0.1)
