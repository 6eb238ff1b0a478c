"""float64 reference of the MBConv depthwise conv (k in {3, 5}, stride in {1, 2}, asymmetric static "SAME" padding) and the closed forms of its data and
weight gradients, written as explicit tap loops -- what fd_dwconv2d_bwd_data_nhwc / fd_dwconv2d_bwd_weight_nhwc compute.  Shared by
tests/test_mbconv_train_cpu.py (closed forms vs float64 autograd) and tests/test_mbconv_train_gpu.py (kernels vs closed forms)."""
from __future__ import annotations

import functools
import itertools

import torch
import torch.nn.functional as F

# (k, stride, (pad_before, pad_after)): the rows efficientnet_pytorch's static padding produces in B0 / B3, and the symmetric (1,1) / (2,2) stride-2 rows
GEOMS = ((3, 1, (1, 1)), (5, 1, (2, 2)), (3, 2, (0, 1)), (3, 2, (1, 1)), (5, 2, (1, 2)), (5, 2, (2, 2)))
MAPS = ((9, 14), (8, 7), (2, 3))


def out_size(n: int, k: int, s: int, pad) -> int:
    return (n + pad[0] + pad[1] - k) // s + 1


def maps_of(geom):
    """The (H, W) maps a GEOMS row is tested on: three for every row, plus (1, 1) for the stride-1 rows."""
    return MAPS + (((1, 1),) if geom[1] == 1 else ())


CASES = tuple((g, hw) for g in GEOMS for hw in maps_of(g))
assert all(out_size(h, k, s, p) >= 1 and out_size(w, k, s, p) >= 1 for (k, s, p), (h, w) in CASES)


def dw_forward(x: torch.Tensor, w: torch.Tensor, s: int, pad) -> torch.Tensor:
    """x [N, C, H, W], w [C, 1, k, k] (float64) -> F.conv2d over the asymmetrically padded input."""
    return F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), w, None, s, 0, 1, x.shape[1])


def dw_dgrad(dy: torch.Tensor, w: torch.Tensor, s: int, pad, H: int, W: int) -> torch.Tensor:
    """dx[n,c,h,w] = sum_{r,q} dy[n,c,ho,wo] * w[c,0,r,q] over the taps with h + pad - r = s * ho, 0 <= ho < Ho (same along w)."""
    N, C, Ho, Wo = dy.shape
    k = w.shape[-1]
    dx = torch.zeros(N, C, H, W, dtype=dy.dtype)
    for h, x_, r, q in itertools.product(range(H), range(W), range(k), range(k)):
        a, b = h + pad[0] - r, x_ + pad[0] - q
        if a % s or b % s or not (0 <= a // s < Ho) or not (0 <= b // s < Wo):
            continue
        dx[:, :, h, x_] += dy[:, :, a // s, b // s] * w[:, 0, r, q]
    return dx


def dw_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int, s: int, pad) -> torch.Tensor:
    """dw[c,0,r,q] = sum_{n,ho,wo} dy[n,c,ho,wo] * x[n,c,ho*s - pad + r, wo*s - pad + q] over the taps inside the input."""
    N, C, H, W = x.shape
    _, _, Ho, Wo = dy.shape
    dw = torch.zeros(C, 1, k, k, dtype=x.dtype)
    for ho, wo, r, q in itertools.product(range(Ho), range(Wo), range(k), range(k)):
        hi, wi = ho * s - pad[0] + r, wo * s - pad[0] + q
        if 0 <= hi < H and 0 <= wi < W:
            dw[:, 0, r, q] += (dy[:, :, ho, wo] * x[:, :, hi, wi]).sum(0)
    return dw


@functools.lru_cache(maxsize=None)
def case(geom, hw, C: int, N: int = 2):
    """Inputs and float64 references of one table entry, computed once and shared (callers must not modify them):
    dict(x, w, dy, scale, y, dx, dw) -- dx / dw WITHOUT the scale."""
    k, s, pad = geom
    H, W = hw
    g = torch.Generator().manual_seed(1000 * k + 100 * s + 10 * pad[0] + H + 31 * W + C)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(C, 1, k, k, generator=g, dtype=torch.float64) * 0.3
    y = dw_forward(x, w, s, pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return dict(x=x, w=w, dy=dy, scale=scale, y=y, dx=dw_dgrad(dy, w, s, pad, H, W), dw=dw_wgrad(x, dy, k, s, pad))
