"""CPU checks of tests/composite_cases.py: the cases and the bounds of
tests/test_gpu_composite_edges.py stand on their own.

* every break decision the float64 truth takes has |log(T / T_thresh)| >= log 2
  (on the f32, f16-rounded and bf16-colour inputs alike), so an f32 evaluation
  cannot decide differently, and the rays break where the case says they do;
* the truth's closed-form backward equals torch.autograd in f64 on the
  truncated forward;
* the f32 C oracle alone (oracle.composite_rays_train_forward / _backward,
  oracle.composite_rays) meets one third of every bound, on every case, layout
  and element type;
* the NaN ray's NaN pattern is the same in the oracle and the truth and is
  confined to that ray's outputs and rows.
"""
import numpy as np
import pytest
import torch

import composite_cases as cc

# (N, layout, order) of every case the GPU tests run
TRAIN_CASES = ([(n, "B", "ordered") for n in cc.RAY_COUNTS]
               + [(n, "T", "scattered") for n in cc.RAY_COUNTS]
               + [(70, "A", "ordered"), (70, "T", "ordered"), (17, "A", "ordered")])
# (elem, rgb_elem) of every entry
TRAIN_ELEMS = [("f32", "f32"), ("f16", "f16"), ("f64", "f64"), ("f32", "f16"), ("f32", "bf16")]
OUTPUTS = ("ws", "depth", "image", "grad_sigma", "grad_rgb")


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("case", TRAIN_CASES, ids=_ids)
def test_break_margins_and_oracle_within_a_third(case):
    c = cc.train_case(*case)
    worst = np.inf
    for T_thresh in cc.T_THRESH:
        for elem, ce in TRAIN_ELEMS:
            ref = cc.train_reference(c, T_thresh, elem, ce)
            worst = min(worst, ref["margin"])
            assert ref["margin"] >= cc.LOG2, (T_thresh, elem, ce, ref["margin"])
            for name in OUTPUTS:
                store = ce if name == "grad_rgb" else elem
                cc.check_bounds(name, ref["oracle"][name], ref["truth"][name],
                                ref["oracle"][name], store, share=1.0 / 3.0,
                                tag=f"[{_ids(case)} T {T_thresh:g} {elem}/{ce}]")
    print(f"\nsmallest break margin |log(T / T_thresh)| of {_ids(case)}: {worst:.3f}")


def test_rays_break_where_the_case_says():
    c = cc.train_case(70, "T", "ordered")
    for elem in ("f32", "f16"):
        want = {1e-4: {13: 1, 14: 5, 15: 16, 16: 17, 17: 96, 18: 101, 20: 3, 21: 6, 32: 8, 33: 21,
                       34: 41, 35: 50},
                1e-2: {13: 1, 14: 4, 15: 16, 16: 17, 17: 96, 18: 101, 20: 3, 21: 6, 32: 8, 33: 21,
                       34: 41, 35: 50}}
        for T_thresh, rays in want.items():
            taken = cc.train_reference(c, T_thresh, elem)["taken"]
            for ray, k in rays.items():
                assert taken[ray] == k, (elem, T_thresh, ray, taken[ray], k)
            plain = [r for r in range(70) if r not in rays]
            assert np.array_equal(taken[plain], c.rays[plain, 2])
        ref = cc.train_reference(c, 0.0, elem)
        assert np.array_equal(ref["taken"], c.rays[:, 2])   # nothing breaks at T_thresh 0
        # behind an opaque sample T is exactly 0: no weight, no colour gradient
        for ray, (num, at) in cc._OPAQUE.items():
            o = int(c.rays[ray, 1])
            assert not ref["truth"]["grad_rgb"][o + at + 1:o + num].any()
            assert ref["truth"]["grad_rgb"][o + at].any()
    # layouts: the final ray past the capacity (A), ending at M (B)
    a, b = cc.train_case(70, "A", "ordered"), cc.train_case(70, "B", "ordered")
    assert a.rays[-1, 1] + a.rays[-1, 2] > a.M > a.rays[-1, 1]
    assert b.rays[-1, 1] + b.rays[-1, 2] == b.M
    assert cc.train_reference(a, 1e-4)["taken"][-1] == 0
    s = cc.train_case(70, "T", "scattered")
    row = s.row_of(s.victim)
    assert 0 < row < 69 and s.rays[row, 1] + s.rays[row, 2] > s.M
    assert sorted(s.rays[:, 0]) == list(range(70)) and not np.array_equal(s.rays[:, 0], np.arange(70))


@pytest.mark.parametrize("T_thresh", cc.T_THRESH)
@pytest.mark.parametrize("case", [(70, "T", "scattered"), (70, "A", "ordered")], ids=_ids)
def test_truth_backward_equals_f64_autograd(case, T_thresh):
    c = cc.train_case(*case)
    sg, cl, dl, gw, gi = c.inputs("f32")
    tb = cc.train_truth_backward(gw, gi, sg, cl, dl, c.rays, c.M, T_thresh)
    tf = cc.train_truth_forward(sg, cl, dl, c.rays, c.M, T_thresh)
    checked = 0
    for n in range(c.N):
        index, o, _ = (int(v) for v in c.rays[n])
        k = int(tb["taken"][n])
        if k == 0 or c.ray_id[n] == cc.NAN_RAY:
            continue
        s = torch.tensor(sg[o:o + k], requires_grad=True)
        col = torch.tensor(cl[o:o + k], requires_grad=True)
        x = s * torch.tensor(dl[o:o + k, 0])
        before = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(x, 0)[:-1]])
        w = (1.0 - torch.exp(-x)) * torch.exp(-before)
        ws, image = w.sum(), (w[:, None] * col).sum(0)
        (ws * float(gw[index]) + (image * torch.tensor(gi[index])).sum()).backward()
        np.testing.assert_allclose(ws.item(), tf["ws"][index], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(image.detach().numpy(), tf["image"][index], rtol=1e-12,
                                   atol=1e-15)
        np.testing.assert_allclose(tb["grad_sigma"][o:o + k], s.grad.numpy(), rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(tb["grad_rgb"][o:o + k], col.grad.numpy(), rtol=1e-9, atol=1e-13)
        checked += 1
    assert checked >= 55
    # rows of no taken sample carry no gradient
    assert not tb["grad_sigma"][~tb["owned"]].any() and not tb["grad_rgb"][~tb["owned"]].any()


@pytest.mark.parametrize("T_thresh", cc.T_THRESH)
@pytest.mark.parametrize("case", [(70, "T", "scattered"), (70, "A", "ordered")], ids=_ids)
def test_nan_ray_is_confined_and_matches_the_oracle(case, T_thresh):
    c = cc.train_case(*case)
    row = c.row_of(cc.NAN_RAY)
    index, o, num = (int(v) for v in c.rays[row])
    for elem, ce in TRAIN_ELEMS:
        ref = cc.train_reference(c, T_thresh, elem, ce)
        t, orc = ref["truth"], ref["oracle"]
        for name in OUTPUTS:
            assert np.array_equal(np.isnan(t[name]), np.isnan(orc[name])), (name, elem)
        for name in ("ws", "depth", "image"):
            nan = np.isnan(t[name]).reshape(c.N, -1)
            assert nan[index].all() and not np.delete(nan, index, 0).any(), name
        assert np.isnan(t["grad_sigma"][o:o + num]).all()
        assert np.isfinite(t["grad_rgb"][o:o + cc.NAN_AT]).all()
        assert np.isnan(t["grad_rgb"][o + cc.NAN_AT:o + num]).all()
        for name in ("grad_sigma", "grad_rgb"):
            nan = np.isnan(t[name]).reshape(c.rows, -1).any(1)
            assert not nan[:o].any() and not nan[o + num:].any(), name


@pytest.mark.parametrize("n_step", cc.INFER_STEPS)
@pytest.mark.parametrize("n_alive", cc.INFER_ALIVE)
def test_inference_cases(n_alive, n_step):
    c = cc.infer_case(n_alive, n_step)
    assert len(set(c.rays_alive[:n_alive].tolist())) == n_alive and c.n_rays > n_alive
    for T_thresh in cc.INFER_THRESH:
        for elem in ("f32", "f16", "f64"):
            ref = cc.infer_reference(c, T_thresh, elem)
            assert ref["margin"] >= cc.LOG2, (T_thresh, elem, ref["margin"])
            t, orc = ref["truth"], ref["oracle"]
            assert np.array_equal(t["rays_alive"], orc["rays_alive"])
            for name in ("ws", "depth", "image", "rays_t"):
                cc.check_bounds(name, orc[name], t[name], orc[name], elem, share=1.0 / 3.0,
                                tag=f"[infer {n_alive} x {n_step} T {T_thresh:g} {elem}]")
            # the kinds do what they claim
            retired = t["rays_alive"][:n_alive] < 0
            for n in range(n_alive):
                kind, took = cc.KINDS[c.kind[n]], int(t["taken"][n])
                if kind == "plain" or kind == "opaque last step":
                    assert took == n_step and not retired[n]
                elif kind == "ends at step 0":
                    assert took == 0 and retired[n]
                elif kind == "ends mid-way" and n_step >= 2:
                    assert took == n_step // 2 and retired[n]
                elif kind == "T_thresh at the first step" and T_thresh == 1e-2:
                    assert took == 1 and retired[n]
                elif kind == "T_thresh at the last step" and n_step >= 2:
                    assert took == n_step and retired[n]
            rt0 = cc.round_to(c.rays_t, elem)
            dead = c.rays_alive[:n_alive][retired]
            assert np.array_equal(t["rays_t"][dead], rt0[dead])


def test_inference_kinds_all_occur():
    seen = set()
    for n_alive in cc.INFER_ALIVE:
        for n_step in cc.INFER_STEPS:
            c = cc.infer_case(n_alive, n_step)
            t = cc.infer_reference(c, 1e-2)["truth"]
            seen |= {(cc.KINDS[k], bool(a < 0)) for k, a in zip(c.kind, t["rays_alive"])}
    assert {k for k, _ in seen} == set(cc.KINDS)
    assert {r for _, r in seen} == {False, True}
