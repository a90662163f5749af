"""CPU checks of tests/field_head_cases.py: the trained-like heads hold what
they are named for, on the rows every GPU test uses, from the restatements
alone (oracle/field.py for the grid field, the float64 truth for the vanilla
field).  These are conditions on the inputs, not tolerances.

* at least 15 % of rows have y < -16, at least 8 % have y > 16, at least 30 %
  have |y| < 14, every |y| <= 80, sigma is finite and positive;
* at least 5 % of albedo entries are exactly 1 (f16 and bf16), at least 2 %
  exactly 0 in f16;
* the class-scaled gs is finite and the density row's gradient gs exp(clamp y)
  stays far inside f16 range;
* the overflow case has at least 10 % of rows with y > ln 65520 + 0.1 and at
  least 30 % with y < 7;
* the float64 trunc_exp equals activation.trunc_exp in value and gradient at
  y = +-14.5, +-15, +-15.5, +-40, and the truth built on it equals the plain
  exp form where |y| < 15.
"""
import numpy as np
import pytest
import torch

import field_head_cases as fc


def _check_classes(y, sigma):
    s = fc.class_shares(y)
    assert s["low"] >= 0.15, s
    assert s["high"] >= 0.08, s
    assert s["mid"] >= 0.30, s
    assert s["max_abs"] <= fc.Y_MAX, s
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    return s


def _check_gs(gs, y):
    assert np.isfinite(gs).all()
    d0 = np.abs(gs.astype(np.float64)) * np.exp(np.clip(np.asarray(y, np.float64), -15, 15))
    assert d0.max() < 1.0  # 1e-2 |n|: no f16 overflow, every row alike
    for side in ("low", "high"):
        assert np.count_nonzero(fc.only(gs, y, side)) >= 2


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("M", list(fc.GRID_SIZES))
def test_grid_case_holds_its_classes(M, bf16):
    fo = fc.grid_restatement(M, bf16)
    s = _check_classes(fo["y"], fo["sigma"])
    a = fo["albedo"].astype(np.float64)
    ones, zeros = float((a == 1).mean()), float((a == 0).mean())
    print(f"grid M={M} {'bf16' if bf16 else 'f16'}: {s} albedo == 1 {ones:.3f} == 0 {zeros:.3f}")
    assert ones >= 0.05
    if not bf16:
        assert zeros >= 0.02
    gs, ga = fc.grid_upstream(M, bf16)
    _check_gs(gs, fo["y"])
    assert gs.dtype == np.float32 and ga.shape == (M, 3)
    c = fc.grid_case()
    assert all(np.abs(w).max() < 65504 for w in c["ws"])


@pytest.mark.parametrize("M", list(fc.VAN_SIZES))
def test_vanilla_case_holds_its_classes(M):
    o, y = fc.vanilla_truth_y(M)
    s = _check_classes(y.numpy(), torch.exp(y).float().numpy())
    a = torch.sigmoid(o[:, 1:])
    ones16, zeros16 = float((a.half() == 1).float().mean()), float((a.half() == 0).float().mean())
    print(f"vanilla M={M}: {s} f16 albedo == 1 {ones16:.3f} == 0 {zeros16:.3f}")
    assert ones16 >= 0.05 and zeros16 >= 0.02
    assert float((a.bfloat16() == 1).float().mean()) >= 0.05
    gs, ga = fc.vanilla_upstream(M)
    _check_gs(gs.numpy(), y.numpy())
    assert all(float(p.abs().max()) < 65504 for p in fc.vanilla_case()["trained"])


def test_vanilla_shapes_and_base_parameters():
    import _resmlp
    assert fc.SHAPES == [tuple(s) for s in _resmlp.SHAPES]
    assert (fc.IN, fc.HIDDEN) == (_resmlp.IN, _resmlp.HIDDEN)
    c = fc.vanilla_case()
    assert [tuple(p.shape) for p in c["base"]] == fc.SHAPES
    # only the output layer differs from the base net
    for i, (a, b, o) in enumerate(zip(c["base"], c["trained"], c["overflow"])):
        assert torch.equal(a, b) == (i < 17), i
        assert torch.equal(a, o) == (i != 18), i
    d = c["overflow"][18] - c["base"][18]
    assert d.tolist() == [fc.VAN_BIAS_UP, 0.0, 0.0, 0.0]
    # the base net is in the range the existing tests cover
    with torch.no_grad():
        _, y = fc.truth_outputs([p.double() for p in c["base"]], c["xs"][1000].double())
    assert float(y.max()) < 7 and float(y.min()) > -7


def test_overflow_case_holds_its_classes():
    c = fc.vanilla_case()
    x = c["x_overflow"]
    assert x.shape == (fc.VAN_OVERFLOW_M, 3) and float(x.abs().max()) <= 1
    with torch.no_grad():
        _, y = fc.truth_outputs([p.double() for p in c["overflow"]], x.double())
    hi = float((y > fc.LN_F16_MAX + 0.1).double().mean())
    lo = float((y < 7).double().mean())
    print(f"overflow case: y > ln 65520 + 0.1 on {hi:.3f}, y < 7 on {lo:.3f}, in between "
          f"{1 - hi - lo:.3f}")
    assert hi >= 0.10 and lo >= 0.30 and 1 - hi - lo >= 0.10
    assert float(y.max()) < 15  # the clamp plays no part in this case
    assert torch.isinf(torch.exp(y[y > fc.LN_F16_MAX + 0.1]).half()).all()


def test_trunc_exp64_equals_activation_trunc_exp():
    from activation import trunc_exp
    pts = [14.5, -14.5, 15.0, -15.0, 15.5, -15.5, 40.0, -40.0]
    g = torch.tensor([0.3, -1.7, 2.0, 1.0, -0.5, 4.0, 1e-3, 7.0], dtype=torch.float64)
    out = []
    for f in (fc.trunc_exp64, trunc_exp):
        y = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
        v = f(y)
        assert v.dtype == torch.float64
        (d,) = torch.autograd.grad(v, y, g)
        out.append((v.detach(), d))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    want = g * torch.exp(torch.tensor(pts, dtype=torch.float64).clamp(-15, 15))
    assert torch.equal(out[0][1], want)
    assert torch.equal(out[0][0], torch.exp(torch.tensor(pts, dtype=torch.float64)))
    # past the clamp the gradient is NOT the derivative
    assert float(out[0][1][6]) == 1e-3 * float(torch.exp(torch.tensor(15.0, dtype=torch.float64)))


def test_truth_equals_the_exp_form_inside_the_clamp():
    """On the base net (|y| < 7) the truth with trunc_exp64 and the plain exp
    form give the same sigma and the same 19 gradients, bit for bit."""
    c = fc.vanilla_case()
    x = c["xs"][257].double()
    gs, ga = torch.randn(257, dtype=torch.float64), torch.randn(257, 3, dtype=torch.float64)
    s1, a1, p1, y = fc.truth_field(c["base"], x)
    assert float(y.detach().abs().max()) < 15
    torch.autograd.backward([s1, a1], [gs, ga])
    p2 = [p.detach().double().requires_grad_(True) for p in c["base"]]
    o, y2 = fc.truth_outputs(p2, x)
    s2, a2 = torch.exp(y2), torch.sigmoid(o[:, 1:])
    torch.autograd.backward([s2, a2], [gs, ga])
    assert torch.equal(s1, s2) and torch.equal(a1, a2)
    for u, v in zip(p1, p2):
        assert torch.equal(u.grad, v.grad)
