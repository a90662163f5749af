"""Shared oracle comparisons for the GPU field tests (imported by test
modules; not collected itself).  See tests/test_gpu_field_oracle.py for the
tolerance model: every GPU value must lie inside the oracle's propagated
f16-rounding window (oracle/field.py), which is closed — i.e. bit-exact — for
most values."""
import numpy as np

import oracle
import oracle.field as of

# forward GEMMs: MFMA chains, few f32 roundings (oracle.field._gamma)
MFMA_ULPS = 8


def embedding_window(d_enc, d_enc_win, x01, offsets, S, H):
    """|grad_embeddings| window: the corner weights are non-negative, so the
    backward of the feature-gradient window bounds the propagated error; the
    f64-accumulated, once-rounded product path adds one f32 rounding plus the
    f16 products' own rounding (2^-22 of the |term| sum)."""
    M = d_enc.shape[0]
    win = oracle.grid_encode_backward(np.asarray(d_enc_win, np.float32).reshape(M, 16, 2), x01,
                                      offsets, 2, S, H)
    mag = oracle.grid_encode_backward(np.abs(d_enc.astype(np.float32)).reshape(M, 16, 2), x01,
                                      offsets, 2, S, H)
    return np.abs(win) + 2.0 ** -22 * mag


def check_field(xyz, emb, offsets, S, H, weights, sigma, albedo, grad_sigma=None,
                grad_albedo16=None, grads=None, grad_emb=None, label="", bf16=False):
    """Compare one GPU field evaluation (and optionally its backward) with the
    oracle.  Arrays are numpy; weights = the six f32 MLP tensors; grads = the
    six GPU gradients; grad_emb = the GPU embedding gradient.  bf16: the bf16
    autocast restatement (oracle.field.precision("bf16"); albedo and
    grad_albedo16 then hold bf16 values as f32).  Returns a dict of
    statistics (printed by the callers)."""
    with of.precision("bf16" if bf16 else "f16"):
        return _check_field(xyz, emb, offsets, S, H, weights, sigma, albedo, grad_sigma,
                            grad_albedo16, grads, grad_emb, label, bf16)


def _check_field(xyz, emb, offsets, S, H, weights, sigma, albedo, grad_sigma, grad_albedo16,
                 grads, grad_emb, label, bf16):
    M = xyz.shape[0]
    stats = {"M": M}
    x16 = (of.encode_bf16 if bf16 else of.encode)(xyz, 1.0, emb, offsets, S, H)
    fo = of.field_forward(xyz, weights, x16)
    fb = of.forward_bounds(fo, weights, acc_ulps=MFMA_ULPS)
    dlog = np.abs(np.log(sigma.astype(np.float64)) - np.log(fo["sigma"].astype(np.float64)))
    assert np.all(dlog <= fb["dlog_sigma"]), \
        f"{label} sigma outside its window by {(dlog - fb['dlog_sigma']).max():.3e}"
    da = np.abs(albedo.astype(np.float64) - fo["albedo"].astype(np.float64))
    assert np.all(da <= fb["dalbedo"]), \
        f"{label} albedo outside its window by {(da - fb['dalbedo']).max():.3e}"
    stats["h0_differs"] = float(np.mean(
        dlog > 8 * 2.0 ** -24 * np.maximum(np.abs(fo["y"].astype(np.float64)), 1.0)))
    stats["albedo_differs"] = float(np.mean((da > 0).any(1))) if M else 0.0
    if grads is None:
        return stats
    bo = of.field_backward(fo, weights, grad_sigma, grad_albedo16)
    bb = of.backward_bounds(fo, bo, weights, fb, acc_ulps=None)
    d_win = bb["d_enc"]
    if not bf16:  # f16 subnormal allowance, see test_gpu_field_oracle.py
        sub = np.abs(bo["d_enc"].astype(np.float64)) < 2.0 ** -14
        d_win = d_win + np.where(sub, 2.0 ** -24, 0.0)
    for i, (a, b, w) in enumerate(zip(grads, bo["grads"], bb["grads"])):
        a = np.asarray(a, np.float64).reshape(b.shape)
        err = np.abs(a - b)
        assert np.all(err <= w), f"{label} MLP param {i} outside its window by {(err - w).max():.3e}"
    if grad_emb is not None:
        x01 = ((np.asarray(xyz, np.float32) + np.float32(1)) / np.float32(2)).astype(np.float32)
        want = oracle.grid_encode_backward(bo["d_enc"].astype(np.float32).reshape(M, 16, 2), x01,
                                           offsets, 2, S, H)
        win = embedding_window(bo["d_enc"], d_win, x01, offsets, S, H)
        err = np.abs(np.asarray(grad_emb, np.float64) - want)
        assert np.all(err <= win + 1e-30), \
            f"{label} embedding grads outside their window by {(err - win).max():.3e}"
        stats["emb_rel_norm"] = float(np.linalg.norm(err) / max(np.linalg.norm(want), 1e-30))
    return stats


def ray_head_inputs(N, seed):
    """Random inputs of the ray head (CPU tensors): unit directions, ws in
    [0, 1), depth, image, nears, fars (a few fars below nears) and the upstream
    image gradient [3, N]."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = torch.randn(N, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    ws = torch.rand(N, generator=g)
    depth = torch.rand(N, generator=g) * 2
    image = torch.rand(N, 3, generator=g)
    nears = torch.rand(N, generator=g) * 0.5 + 0.2
    fars = nears + (torch.rand(N, generator=g) * 2 - 0.1)
    gimg = torch.randn(3, N, generator=g) * 1e-2
    return {"d": d, "ws": ws, "depth": depth, "image": image, "nears": nears, "fars": fars,
            "gimg": gimg}


def check_ray_head(gpu, N, l1, l2, inputs):
    """nerf.head.ray_head with the background network (l1, l2) on `inputs`
    (ray_head_inputs' dict, N rays) against oracle.field.bg_forward / ray_tail /
    bg_backward inside bg_bounds' windows.  Returns the GPU outputs and the
    oracle's (numpy) for further checks."""
    import torch
    from nerf import head as _head
    d, depth, nears, fars = (inputs[k].to(gpu) for k in ("d", "depth", "nears", "fars"))
    ws, image, gimg = (inputs[k].to(gpu) for k in ("ws", "image", "gimg"))
    assert ws.numel() == N
    ws.requires_grad_(True)
    image.requires_grad_(True)
    out_img, out_depth, mask = _head.ray_head(ws, depth, image, d, nears, fars, None, (l1, l2))
    wts = [t.detach().cpu().numpy() for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
    bo = of.bg_forward(d.cpu().numpy(), wts)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ei, ed, em = of.ray_tail(ws.detach().cpu().numpy(), depth.cpu().numpy(),
                                 image.detach().cpu().numpy(), nears.cpu().numpy(),
                                 fars.cpu().numpy(), bo["bg"].astype(np.float32))
    gi = out_img.detach().t().cpu().numpy()
    # colour: (1 - ws) times the background's f16 window, plus the f32 mix
    bb = of.bg_bounds(bo, wts, acc_ulps=None)  # VALU fmaf chains: order-free bound
    one_m = (1.0 - ws.detach().cpu().numpy().astype(np.float64))[:, None]
    win = one_m * bb["dbg"] + 2 * 2.0 ** -24 * np.abs(ei)
    diff = np.abs(gi.astype(np.float64) - ei)
    assert np.all(diff <= win), f"colour outside its window: {(diff - win).max():.3e}"
    print(f"\nN={N}: background colour differs on {(diff > 0).any(1).mean():.2e} of rays")
    np.testing.assert_array_equal(out_depth.detach().cpu().numpy(), ed)
    np.testing.assert_array_equal(mask.cpu().numpy(), em)
    grads = torch.autograd.grad(out_img, [ws, image, l1.weight, l1.bias, l2.weight, l2.bias],
                                gimg)
    gimg_np = gimg.t().cpu().numpy().astype(np.float32)
    np.testing.assert_array_equal(grads[1].cpu().numpy(), gimg_np)
    # grad_ws = -sum_c g_c bg_c: the background's f16 window carried through
    # the sum plus the f32 products and sums (4 u of sum|g bg|), the window
    # test_gpu_step_structures.py uses for this term.  (A relative tolerance
    # on the sum itself, as this check had, fails where the three terms cancel
    # on a ray whose background legitimately took the neighbouring f16 value.)
    g64 = gimg_np.astype(np.float64)
    want_ws = -(g64 * bo["bg"].astype(np.float64)).sum(1)
    win_ws = ((np.abs(g64) * bb["dbg"]).sum(1)
              + 4 * 2.0 ** -24 * (np.abs(g64) * bo["bg"].astype(np.float64)).sum(1))
    err_ws = np.abs(grads[0].cpu().numpy().astype(np.float64) - want_ws)
    assert np.all(err_ws <= win_ws), f"grad_ws outside its window: {(err_ws - win_ws).max():.3e}"
    gbg = gimg_np * (np.float32(1) - ws.detach().cpu().numpy())[:, None]
    bw = of.bg_bounds(bo, wts, gbg)
    for i, (a, b, w) in enumerate(zip(grads[2:], of.bg_backward(bo, wts, gbg), bw["grads"])):
        a = a.cpu().numpy().astype(np.float64).reshape(b.shape)
        err = np.abs(a - b)
        assert np.all(err <= w), f"bg param {i}: worst excess {(err - w).max():.3e}"
    return {"image": gi, "depth": out_depth.detach().cpu().numpy(), "mask": mask.cpu().numpy(),
            "want_image": ei, "want_depth": ed, "want_mask": em,
            "grads": [g.cpu().numpy() for g in grads]}
