"""Float64 restatement of what fd_grad_sumsq_f32 + fd_grad_clip_finish publish in the clip block (include/fcosdet.h fd_grad_clip): the sum of squares of the
gradients as they are (still scaled), the unscaled global 2-norm, torch.nn.utils.clip_grad_norm_'s coefficient, the effective scale the update kernels divide
by, and the found flag.  Works on tensors of any device and dtype; everything is computed in float64 on the host."""
import math
from typing import NamedTuple

import numpy as np


class Clip(NamedTuple):
    sumsq: float
    total_norm: float       # sqrt(sumsq) / scale
    clip_coef: float        # min(1, max_norm / (total_norm + 1e-6)); 1 when found
    eff_scale: float        # scale / clip_coef in float64 (the kernel publishes its fp32 rounding)
    found: bool             # sumsq not finite, or found_inf given and set


def sumsq(grads) -> float:
    """Sum over every element of every gradient (None entries left out) of g * g, in float64: one math.fsum over the per-tensor sums, each a pairwise numpy sum."""
    parts = []
    for g in grads:
        if g is None or g.numel() == 0:
            continue
        a = g.detach().double().cpu().numpy().reshape(-1)
        with np.errstate(over="ignore", invalid="ignore"):
            parts.append(float(np.sum(a * a)))
    if any(not math.isfinite(v) for v in parts):
        return float("nan") if any(math.isnan(v) for v in parts) else float("inf")
    return math.fsum(parts)


def clip(grads, max_norm, grad_scale=None, found_inf=False) -> Clip:
    s = sumsq(grads)
    scale = 1.0 if grad_scale is None else float(grad_scale)
    total = math.sqrt(s) / scale if not math.isnan(s) else float("nan")
    found = (not math.isfinite(s)) or bool(found_inf)
    coef = 1.0 if found else min(1.0, float(max_norm) / (total + 1e-6))
    return Clip(s, total, coef, scale / coef, found)
