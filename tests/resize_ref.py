"""numpy restatement of the device resize (csrc/fd_resize.hip): bilinear, half-pixel geometry, no antialiasing,
11-bit integer blending.  Every fp32 operation is a separate numpy float32 operation (one rounding each, no FMA), so the
result equals the kernels bit for bit.  Test infrastructure only."""
import numpy as np

F = np.float32


def axis_taps(S: int, D: int):
    """(i0, i1, c0, c1) for destination indices 0 .. D-1 of one axis: source length S, destination length D."""
    d = np.arange(D, dtype=np.int64).astype(F)
    scale = F(S) / F(D)
    x = (d + F(0.5)) * scale - F(0.5)
    fl = np.floor(x)
    f = x - fl
    lo = fl < F(0)
    fl = np.where(lo, F(0), fl)
    f = np.where(lo, F(0), f)
    hi = fl >= F(S - 1)
    fl = np.where(hi, F(S - 1), fl)
    f = np.where(hi, F(0), f)
    assert fl.dtype == F and f.dtype == F and x.dtype == F
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, S - 1)
    c1 = np.floor(f * F(2048.0) + F(0.5)).astype(np.int64)
    c0 = 2048 - c1
    return i0, i1, c0, c1


def resize_u8(img: np.ndarray, nh: int, nw: int) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [nh, nw, 3]."""
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w = img.shape[:2]
    y0, y1, cy0, cy1 = axis_taps(h, nh)
    x0, x1, cx0, cx1 = axis_taps(w, nw)
    p = img.astype(np.int64)
    cy0, cy1 = cy0[:, None, None], cy1[:, None, None]
    cx0, cx1 = cx0[None, :, None], cx1[None, :, None]
    acc = (p[y0][:, x0] * (cx0 * cy0) + p[y0][:, x1] * (cx1 * cy0) + p[y1][:, x0] * (cx0 * cy1) + p[y1][:, x1] * (cx1 * cy1)
           + (1 << 21))
    assert int(acc.max()) < 2 ** 31
    return (acc >> 22).astype(np.uint8)


def normalise(levels: np.ndarray, mean, std) -> np.ndarray:
    """ToTensor + Normalize in the kernels' fp32 order: (u8 / 255 - mean) / std -> [..., 4], channel 3 = 0."""
    out = np.zeros(levels.shape[:-1] + (4,), F)
    for c in range(3):
        out[..., c] = (levels[..., c].astype(F) / F(255.0) - F(mean[c])) / F(std[c])
    return out
