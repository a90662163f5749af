"""The entry points of csrc/hiersample.hip (the native glue of
NeRFRenderer.run) check their arguments before any device work, so their
errors are testable without a GPU; the public functions raise on CPU tensors."""
import pytest
import torch

import _dfhip

NULLS = {
    "dfhip_uniform_samples": lambda N, T, t: ([None] * 7, [N, T], [None] * 3),
    "dfhip_importance_samples": lambda N, T, t: ([None] * 8, [N, T, t], [None] * 3),
    "dfhip_merge_samples": lambda N, T, t: ([None] * 4, [N, T, t], [None] * 4),
    "dfhip_composite_uniform_forward": lambda N, T, t: ([0] + [None] * 8, [N, T, t], [None] * 5),
    "dfhip_composite_uniform_backward": lambda N, T, t: ([0] + [None] * 11, [N, T, t],
                                                         [None] * 4),
}


def _call(name, N, T, t):
    lib = _dfhip.load()
    head, sizes, tail = NULLS[name](N, T, t)
    rc = getattr(lib, name)(*head, *sizes, *tail)
    return rc, lib.dfhip_last_error().decode()


@pytest.mark.parametrize("name", sorted(NULLS))
def test_sizes_are_checked(name):
    for T, t in ((2, 0), (0, 0), (257, 0)):
        rc, msg = _call(name, 4, T, t)
        assert rc == 1 and "3 <= T <= 256" in msg and f"T = {T}" in msg, (T, t, rc, msg)
    if name == "dfhip_uniform_samples":
        return
    for T, t in ((256, 257), (255, 258), (2, 16)):
        rc, msg = _call(name, 4, T, t)
        assert rc == 1 and "T + t <= 512" in msg and f"t = {t}" in msg, (T, t, rc, msg)


@pytest.mark.parametrize("name", sorted(NULLS))
def test_null_pointers_are_errors_and_empty_batches_are_not(name):
    rc, msg = _call(name, 4, 64, 64)
    assert rc == 1 and "must not be NULL" in msg, (rc, msg)
    assert _call(name, 0, 64, 64)[0] == 0
    assert _call(name, 0, 3, 0)[0] == 0


def test_rgbs_dtype_is_checked():
    lib = _dfhip.load()
    for name, n_ptr, n_out in (("dfhip_composite_uniform_forward", 8, 5),
                               ("dfhip_composite_uniform_backward", 11, 4)):
        for bad in (_dfhip.F64, _dfhip.BF16):
            rc = getattr(lib, name)(bad, *[None] * n_ptr, 4, 16, 16, *[None] * n_out)
            assert rc == 2 and b"f32 or f16" in lib.dfhip_last_error()


def test_public_functions_raise_on_cpu_tensors():
    import raymarching
    N, T, t = 5, 16, 8
    o, d = torch.zeros(N, 3), torch.ones(N, 3)
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    nears, fars = torch.zeros(N), torch.ones(N)
    z, xyzs = torch.zeros(N, T), torch.zeros(N, T, 3)
    new_z, new_xyzs = torch.zeros(N, t), torch.zeros(N, t, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        raymarching.uniform_samples(o, d, aabb, nears, fars, torch.linspace(0, 1, T))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        raymarching.importance_samples(o, d, aabb, nears, fars, z, torch.zeros(N, T), t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        raymarching.merge_samples(z, new_z, xyzs, new_xyzs)
    order = torch.zeros(N, T + t, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        raymarching.composite_uniform(torch.zeros(N, T), torch.zeros(N, t), order,
                                      torch.zeros(N, T + t), nears, fars, fars / T,
                                      torch.zeros(N, T + t, 3))


def test_renderer_keeps_torch_off_the_supported_sizes():
    """CPU tensors, non-f32 rays and sizes outside 3 <= T <= 256, t <= 256,
    T + t <= 512 keep the torch path."""
    from nerf.renderer import NeRFRenderer
    ok = NeRFRenderer._run_native_eligible
    cpu = torch.zeros(4, 3)
    assert not ok(cpu, cpu, torch.zeros(4), 64, 64)
    from types import SimpleNamespace
    f32 = SimpleNamespace(is_cuda=True, dtype=torch.float32)
    for T, t, want in ((64, 64, True), (3, 0, True), (256, 256, True), (2, 0, False),
                       (257, 0, False), (256, 257, False), (64, -1, False)):
        assert ok(f32, f32, f32, T, t) is want, (T, t)
    f16 = SimpleNamespace(is_cuda=True, dtype=torch.float16)
    assert not ok(f16, f32, f32, 64, 64) and not ok(f32, f16, f32, 64, 64)
