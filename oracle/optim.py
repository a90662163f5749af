"""float64 restatement of one `scaler.step(optimizer); scaler.update()` of the
train loop (reference nerf/utils.py:708-713 with torch.optim.Adam and
torch.amp.GradScaler), the oracle of csrc/optim.hip.

Per step, over every tensor that has a gradient:

* found_inf = any gradient element is inf or nan
  (torch._amp_foreach_non_finite_check_and_unscale_);
* unless found_inf, per element with t = step + 1 (ATen fused_adam_utils.cuh,
  ADAM mode, no amsgrad, no maximize):
      g = grad / scale;  g += wd * p
      m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g
      step_size = lr / (1 - b1^t);  denom = sqrt(v) / sqrt(1 - b2^t) + eps
      p -= step_size * m / denom
  and the tensor's step count becomes t;
* torch._amp_update_scale_: on found_inf the scale is multiplied by the
  backoff factor and the growth tracker reset; otherwise the tracker counts
  one more clean step and, when it reaches growth_interval, the scale is
  multiplied by the growth factor — unless that is not a finite float32, the
  scale being a float32 tensor — and the tracker reset.

Everything is float64; the hyper-parameters are arguments, so a caller that
models a float32 C ABI passes the float32-rounded values.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def found_inf(grads):
    """True when any element of any gradient (None: no gradient) is not finite."""
    return any(g is not None and not np.isfinite(np.asarray(g, F64)).all() for g in grads)


def adam_element(p, g, m, v, step, scale, lr, b1, b2, eps, wd):
    """The Adam update of one tensor from state (p, m, v) at step count `step`
    (so t = step + 1).  Returns (p, m, v) after it, float64."""
    p, m, v = (np.asarray(a, F64) for a in (p, m, v))
    lr, b1, b2, eps, wd, scale = (F64(a) for a in (lr, b1, b2, eps, wd, scale))
    t = F64(step) + 1.0
    g = np.asarray(g, F64) / scale
    g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    with np.errstate(divide="ignore", invalid="ignore"):  # m = v = eps = 0: nan, as torch
        p = p - step_size * m / denom
    return p, m, v


def update_scale(scale, tracker, inf, growth_interval, growth_factor=2.0, backoff_factor=0.5):
    """torch._amp_update_scale_ -> (scale, tracker)."""
    if inf:
        return float(F32(F32(scale) * F32(backoff_factor))), 0
    tracker = int(tracker) + 1
    if tracker == int(growth_interval):
        with np.errstate(over="ignore"):
            grown = F32(F32(scale) * F32(growth_factor))
        return (float(grown) if np.isfinite(grown) else float(scale)), 0
    return float(scale), tracker


def amp_adam_step(params, grads, exp_avg, exp_avg_sq, steps, hyper, scale, tracker,
                  growth_interval, growth_factor=2.0, backoff_factor=0.5):
    """One scaler.step + scaler.update.

    params / grads / exp_avg / exp_avg_sq: one array per tensor (a None
    gradient: the tensor is skipped, as torch skips it); steps: one count per
    tensor; hyper: one (lr, b1, b2, eps, weight_decay) per tensor.  Nothing is
    modified; returns (params, exp_avg, exp_avg_sq, steps, scale, tracker,
    found_inf) with float64 arrays."""
    inf = found_inf(grads)
    P = [np.array(a, F64) for a in params]
    M = [np.array(a, F64) for a in exp_avg]
    V = [np.array(a, F64) for a in exp_avg_sq]
    S = [float(s) for s in steps]
    if not inf:
        for k, g in enumerate(grads):
            if g is None:
                continue
            P[k], M[k], V[k] = adam_element(P[k], g, M[k], V[k], S[k], scale, *hyper[k])
            S[k] += 1.0
    scale, tracker = update_scale(scale, tracker, inf, growth_interval, growth_factor,
                                  backoff_factor)
    return P, M, V, S, scale, tracker, inf
