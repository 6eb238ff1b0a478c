"""numpy restatement of the device augmentations (csrc/fd_augment.hip): PIL's nearest-neighbour rotate as
16.16 fixed-point integer arithmetic, the colour chain (PIL's ImageEnhance Brightness / Contrast / Color and the HSV hue
shift) with every fp32 operation a separate numpy float32 operation, the integer L sums, and the whole fused pixel path
(colour chain -> rotate -> crop -> flip folded into the taps of tests/resize_ref.py).  Test infrastructure only."""
import math

import numpy as np

import resize_ref

F = np.float32
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 1, 2, 3, 4
MAX_ROT_SIDE = 16384


# ---------------------------------------------------------------------------------------------------------------- rotation
def fix16(v: float) -> int:
    """16.16 fixed point of a double, rounded half away from zero."""
    return int(v * 65536.0 + (-0.5 if v < 0 else 0.5))


def rotation_fixed(d: float, h: int, w: int):
    """The six integers of img.rotate(d) (NEAREST, no expand, centre (w/2, h/2)) for an h x w image:
    (A0, A1, X0, A3, A4, Y0) with source pixel of (x, y) = ((X0 + A0*x + A1*y) >> 16, (Y0 + A3*x + A4*y) >> 16)."""
    angle = -math.radians(d % 360.0)
    a0, a1 = round(math.cos(angle), 15), round(math.sin(angle), 15)
    a3, a4 = round(-math.sin(angle), 15), round(math.cos(angle), 15)
    cx, cy = w / 2.0, h / 2.0
    a2 = a0 * -cx + a1 * -cy + 0.0
    a5 = a3 * -cx + a4 * -cy + 0.0
    a2 += cx
    a5 += cy
    return (fix16(a0), fix16(a1), fix16(a2 + a0 * 0.5 + a1 * 0.5), fix16(a3), fix16(a4), fix16(a5 + a3 * 0.5 + a4 * 0.5))


def rotation_extent(fx, h: int, w: int) -> int:
    """Largest |fixed-point coordinate| over the image: the four corners bound the affine form."""
    A0, A1, X0, A3, A4, Y0 = fx
    m = 0
    for x in (0, w - 1):
        for y in (0, h - 1):
            m = max(m, abs(X0 + A0 * x + A1 * y), abs(Y0 + A3 * x + A4 * y))
    return m


def rotate_map(fx, h: int, w: int):
    """(sy, sx, inside) int64 / bool [h, w]: the source pixel of every destination pixel."""
    A0, A1, X0, A3, A4, Y0 = fx
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    sx = (X0 + A0 * x + A1 * y) >> 16
    sy = (Y0 + A3 * x + A4 * y) >> 16
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    return sy, sx, inside


def rotate_u8(img: np.ndarray, d: float) -> np.ndarray:
    assert img.dtype == np.uint8 and img.ndim == 3
    if d == 0:
        return img.copy()
    h, w = img.shape[:2]
    sy, sx, inside = rotate_map(rotation_fixed(d, h, w), h, w)
    out = img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    out[~inside] = 0
    return out


# ------------------------------------------------------------------------------------------------------------------ colour
def luma(p: np.ndarray) -> np.ndarray:
    """PIL's RGB -> L on integer levels [..., 3] -> int64 [...]."""
    p = p.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def _blend(deg: np.ndarray, pix: np.ndarray, f: float) -> np.ndarray:
    """clip(trunc(deg + f * (pix - deg))): fp32, one rounding per operation; integer inputs."""
    f = F(f)
    v = deg.astype(F) + f * (pix.astype(np.int64) - deg.astype(np.int64)).astype(F)
    assert v.dtype == F
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def rgb_to_hsv(p: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [..., 3] (h, s, v), PIL's arithmetic: the ratios in fp32, the sums with constants in fp64."""
    r, g, b = (p[..., c].astype(np.int64) for c in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(F)
    mx = np.where(grey, 1, maxc).astype(F)
    s = cr / mx
    rc = (maxc - r).astype(F) / cr
    gc = (maxc - g).astype(F) / cr
    bc = (maxc - b).astype(F) / cr
    D = np.float64
    h = np.where(r == maxc, (bc - gc).astype(D), np.where(g == maxc, (D(2.0) + rc.astype(D)) - bc.astype(D), (D(4.0) + gc.astype(D)) - rc.astype(D))).astype(F)
    h = np.fmod(h.astype(D) / D(6.0) + D(1.0), D(1.0)).astype(F)
    uh = np.clip((h.astype(D) * D(255.0)).astype(np.int64), 0, 255)
    us = np.clip((s.astype(D) * D(255.0)).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1)
    return out.astype(np.uint8)


def hsv_to_rgb(q: np.ndarray) -> np.ndarray:
    """uint8 (h, s, v) [..., 3] -> uint8 RGB, PIL's arithmetic in fp32."""
    h, s, v = (q[..., c].astype(F) for c in range(3))
    x = h * F(6.0) / F(255.0)
    fi = np.floor(x)
    f = x - fi
    fs = s / F(255.0)
    one = F(1.0)
    rnd = lambda a: np.clip(np.floor(a + F(0.5)), 0, 255).astype(np.int64)      # noqa: E731
    p = rnd(v * (one - fs))
    qq = rnd(v * (one - fs * f))
    t = rnd(v * (one - fs * (one - f)))
    i = fi.astype(np.int64) % 6
    vi = q[..., 2].astype(np.int64)
    r = np.choose(i, [vi, qq, p, p, t, vi])
    g = np.choose(i, [t, vi, vi, qq, p, p])
    b = np.choose(i, [p, p, t, vi, vi, qq])
    grey = q[..., 1] == 0
    out = np.stack([np.where(grey, vi, r), np.where(grey, vi, g), np.where(grey, vi, b)], -1)
    return out.astype(np.uint8)


def hue_shift_of(hue: float) -> int:
    """The uint8 added to H (with wrap) for a hue factor in [-0.5, 0.5]: truncation toward zero, modulo 256."""
    return int(hue * 255) & 255


def apply_op(p: np.ndarray, op: int, arg, mean_l=None) -> np.ndarray:
    """One operation on uint8 [..., 3].  arg: the factor (brightness / contrast / saturation) or the uint8 hue shift;
    mean_l: the contrast mean, int(mean(L) + 0.5) of the WHOLE image at this point of the chain."""
    if op == OP_BRIGHTNESS:
        return _blend(np.zeros_like(p), p, arg)
    if op == OP_CONTRAST:
        return _blend(np.full_like(p, mean_l), p, arg)
    if op == OP_SATURATION:
        return _blend(np.repeat(luma(p)[..., None], 3, -1), p, arg)
    if op == OP_HUE:
        q = rgb_to_hsv(p)
        q[..., 0] = (q[..., 0].astype(np.int64) + int(arg)) & 255
        return hsv_to_rgb(q)
    raise ValueError(op)


def l_sum_and_mean(img: np.ndarray, chain):
    """(sum of L, int(sum / (h*w) + 0.5)) of the image after the operations that precede contrast in `chain`; (0, 0)
    when the chain has no contrast."""
    p = img
    for op, arg in chain:
        if op == OP_CONTRAST:
            s = int(luma(p).sum())
            return s, int(s / (img.shape[0] * img.shape[1]) + 0.5)
        p = apply_op(p, op, arg)
    return 0, 0


def color_jitter_u8(img: np.ndarray, chain, mean_l=None) -> np.ndarray:
    """The chain [(op, arg), ...] in order on a uint8 [h, w, 3] image.  mean_l given: used as the contrast mean (what
    the device does with the value in its record); None: computed from the image, as PIL does."""
    p = img
    for op, arg in chain:
        m = (l_sum_and_mean(img, chain)[1] if mean_l is None else mean_l) if op == OP_CONTRAST else None
        p = apply_op(p, op, arg, m)
    return p


# ----------------------------------------------------------------------------------------------------------- fused pixel path
def augmented_source(img: np.ndarray, *, flip=False, chain=(), d=0.0, crop=None) -> np.ndarray:
    """flip -> colour chain -> rotate -> crop, the reference's order, as single steps: uint8 [ch, cw, 3]."""
    p = img[:, ::-1] if flip else img
    p = color_jitter_u8(np.ascontiguousarray(p), list(chain))
    p = rotate_u8(p, d)
    if crop is not None:
        x, y, cw, ch = crop
        p = p[y:y + ch, x:x + cw]
    return np.ascontiguousarray(p)


def fused_levels(img: np.ndarray, nh: int, nw: int, H: int, W: int, **kw) -> np.ndarray:
    """uint8 [H, W, 3]: the augmented image resized to nh x nw on a zero canvas."""
    out = np.zeros((H, W, 3), np.uint8)
    out[:nh, :nw] = resize_ref.resize_u8(augmented_source(img, **kw), nh, nw)
    return out


def fused_planar(img: np.ndarray, nh: int, nw: int, H: int, W: int, mean, std, **kw) -> np.ndarray:
    """fp32 [3, H, W]: fused_levels through ToTensor + Normalize."""
    return np.ascontiguousarray(resize_ref.normalise(fused_levels(img, nh, nw, H, W, **kw), mean, std)[..., :3].transpose(2, 0, 1))
