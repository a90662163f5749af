"""The fused grid field (csrc/fieldmlp.hip through nerf/field.py's autograd
node) on a trained-like head: y = h0 + gaussian(x) spans about [-60, 60], so a
quarter of the rows lie below the trunc_exp clamp, a seventh above it, and a
third of the albedo entries round to exactly 0 or 1 (tests/field_head_cases.py;
tests/test_field_head_cases_host.py holds the case to that on the CPU).

Checked with oracle_checks.check_field, the windows of test_gpu_field.py
unchanged: sigma (as log sigma), albedo, the six MLP gradients and the
embedding gradient against oracle/field.py's restatement, whose backward takes
g * exp(clamp(y, -15, 15)) rounded to the autocast type and g (1 - a) a on the
rounded albedo.  Upstream gradients: gs_i = 1e-2 n_i exp(-clip(y_i, -15, 15)),
so every row weighs alike in the parameter gradients; one run each with gs
kept on the low class only (y < -16) and on the high class only (y > 16) names
the side of a failure.
"""
import copy

import numpy as np
import pytest
import torch

import field_head_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def field(gpu):
    c = fc.grid_case()
    return copy.deepcopy(c["enc"]).to(gpu), copy.deepcopy(c["layers"]).to(gpu)


def _run(gpu, field, M, dtype, side=None):
    from nerf.field import eligible, grid_field
    from oracle_checks import check_field
    enc, layers = field
    c = fc.grid_case()
    bf16 = dtype == torch.bfloat16
    x = c["xs"][M].to(gpu)
    gs_np, ga_np = fc.grid_upstream(M, bf16)
    if side is not None:
        gs_np = fc.only(gs_np, fc.grid_restatement(M, bf16)["y"], side)
        assert np.count_nonzero(gs_np) >= 2
    gs, ga = torch.from_numpy(gs_np).to(gpu), torch.from_numpy(ga_np).to(gpu)
    with torch.autocast("cuda", dtype=dtype):
        assert eligible(enc, layers, x)
        s, a = grid_field(x, 1.0, enc, layers)
    assert s.dtype == torch.float32 and a.dtype == dtype
    assert torch.isfinite(s).all() and bool((s > 0).all())
    params = [enc.embeddings] + list(layers.parameters())
    g = torch.autograd.grad((s * gs).sum() + (a.float() * ga).sum(), params)
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in g)
    ga16 = ga.to(dtype).float().cpu().numpy() if bf16 else ga_np.astype(np.float16)
    label = f"trained head M={M} {'bf16' if bf16 else 'f16'} gs={side or 'all'}"
    stats = check_field(x.cpu().numpy(), c["emb"], c["offsets"], c["S"], c["H"], c["ws"],
                        s.detach().cpu().numpy(), a.detach().float().cpu().numpy(), gs_np, ga16,
                        [t.cpu().numpy() for t in g[1:]], g[0].cpu().numpy(), label=label,
                        bf16=bf16)
    a_np = a.detach().float().cpu().numpy()
    stats.update(ones=float((a_np == 1).mean()), zeros=float((a_np == 0).mean()),
                 **fc.class_shares(np.log(s.detach().cpu().numpy().astype(np.float64))))
    print(f"heads: {label}: {stats}")
    return stats


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M", list(fc.GRID_SIZES))
def test_trained_head_matches_oracle(gpu, field, M, dtype):
    stats = _run(gpu, field, M, dtype)
    # the GPU's own outputs hold the classes too
    assert stats["low"] >= 0.15 and stats["high"] >= 0.08 and stats["ones"] >= 0.05
    if dtype == torch.float16:
        assert stats["zeros"] >= 0.02


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("side", ["low", "high"])
def test_trained_head_one_class_matches_oracle(gpu, field, side, dtype):
    _run(gpu, field, 4099, dtype, side)
