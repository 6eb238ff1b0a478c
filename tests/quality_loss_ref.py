"""The IoU-aware classification losses of DESIGN 4.3q restated in numpy: quality(), qfl() and vfl(), each with its closed-form
gradient.  These are the project's own definitions (the reference has neither loss); csrc/fd_quality_loss.hip implements them.

Every function takes dtype = np.float64 (the yardstick) or np.float32: the "fp32 restatement", the device's operations in the
device's order on fp32 numpy scalars-in-arrays, with sums taken in float64 as the kernels take them.  quality() in fp32 is what
fd_ltrb_quality must return bit for bit (IEEE operations only, no contraction on either side); the loss terms hold expf / log1pf,
which numpy and the device round differently by a few ulp, so they are compared within a bound (tests/test_quality_loss_gpu.py).

    s = sigmoid(x), bce(x, y) = max(x, 0) - x*y + log1p(exp(-|x|))
    q        0 where label <= 0; else iou of the two LTRB boxes as fd_loss.hip's ltrb_terms() forms it, then (iou > 0) ? min(iou, 1) : 0
    y        q[b, l] where label[b, l] == c + 1, else 0 (a label above C matches no class)
    QFL      (y - s)^2 * bce(x, y);      d/dx = -2 (y - s) s (1 - s) bce(x, y) + (y - s)^2 (s - y)
    VFL      y > 0: y * bce(x, y),       d/dx = y (s - y)
             else:  a * s^2 * bce(x, 0), d/dx = a (2 s * s (1 - s) * bce(x, 0) + s^2 * s),   a = 0.75
"""
import numpy as np

VFL_ALPHA = 0.75
KINDS = ("qfl", "vfl")


def quality(reg_pred, reg_target, labels, dtype=np.float32):
    """reg_pred / reg_target [..., 4] (l, t, r, b), labels [...] -> q [...] of `dtype`."""
    p, t = np.asarray(reg_pred).astype(dtype), np.asarray(reg_target).astype(dtype)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        wi = np.maximum(np.minimum(p[..., 2], t[..., 2]) + np.minimum(p[..., 0], t[..., 0]), zero)
        hi = np.maximum(np.minimum(p[..., 3], t[..., 3]) + np.minimum(p[..., 1], t[..., 1]), zero)
        ov = wi * hi
        a1 = (p[..., 2] + p[..., 0]) * (p[..., 3] + p[..., 1])
        a2 = (t[..., 2] + t[..., 0]) * (t[..., 3] + t[..., 1])
        U = (a1 + a2) - ov
        iou = ov / U
        q = np.where(iou > zero, np.minimum(iou, dtype(1)), zero)        # NaN > 0 is False
    return np.where(np.asarray(labels) > 0, q, zero).astype(dtype)


def soft_target(labels, q, C, dtype=np.float64):
    """labels [B, L] int, q [B, L] -> y [B, L, C]."""
    labels = np.asarray(labels)
    hit = labels[..., None] == (np.arange(C) + 1)
    return np.where(hit, np.asarray(q).astype(dtype)[..., None], dtype(0)).astype(dtype)


def _parts(x, dtype):
    """e = exp(-|x|), log1p(e), s and 1 - s, both formed from e (neither cancels at a saturated logit): the kernel's order."""
    x = np.asarray(x).astype(dtype)
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(x))
        sp = np.log1p(e)
        inv = dtype(1) / (dtype(1) + e)
        s = np.where(x >= 0, inv, e * inv)
        oms = np.where(x >= 0, e * inv, inv)
    return x, sp.astype(dtype), s.astype(dtype), oms.astype(dtype)


def qfl(x, y, dtype=np.float64):
    """Elementwise Quality Focal Loss and d/dx, arrays of `dtype`."""
    x, sp, s, oms = _parts(x, dtype)
    y = np.asarray(y).astype(dtype)
    with np.errstate(under="ignore"):
        b = (np.maximum(x, dtype(0)) - x * y) + sp
        d = y - s
        loss = (d * d) * b
        grad = ((dtype(-2) * d) * (s * oms)) * b + (d * d) * (s - y)
    return loss.astype(dtype), grad.astype(dtype)


def vfl(x, y, alpha=VFL_ALPHA, dtype=np.float64):
    """Elementwise Varifocal Loss and d/dx, arrays of `dtype`."""
    x, sp, s, oms = _parts(x, dtype)
    y = np.asarray(y).astype(dtype)
    a = dtype(alpha)
    with np.errstate(under="ignore"):
        b = (np.maximum(x, dtype(0)) - x * y) + sp
        b0 = np.maximum(x, dtype(0)) + sp
        loss = np.where(y > 0, y * b, (a * (s * s)) * b0)
        grad = np.where(y > 0, y * (s - y), a * (((dtype(2) * s) * (s * oms)) * b0 + (s * s) * s))
    return loss.astype(dtype), grad.astype(dtype)


def loss_and_grad(kind, logits, labels, q, gscale=None, dtype=np.float64):
    """logits [B, L, C], labels [B, L], q [B, L], gscale [B] or None (ones) -> (loss [B], qsum [B], grad [B, L, C] = d loss_b /
    d logits * gscale[b]), all of `dtype`.  The sums are taken in float64 over the elementwise `dtype` values and then rounded to
    `dtype`, as the kernels sum in doubles and store fp32."""
    assert kind in KINDS
    logits = np.asarray(logits)
    B, L, C = logits.shape
    y = soft_target(labels, q, C, dtype)
    el, g = (qfl if kind == "qfl" else vfl)(logits, y, dtype=dtype)
    gs = np.ones(B, dtype) if gscale is None else np.asarray(gscale).astype(dtype)
    with np.errstate(under="ignore"):
        g = (g * gs[:, None, None]).astype(dtype)
    return el.astype(np.float64).sum(axis=(1, 2)).astype(dtype), np.asarray(q).astype(np.float64).sum(axis=1).astype(dtype), g


def max_err(got, want):
    """The largest absolute error of `got` against float64 `want` over the largest magnitude of `want`."""
    want = np.asarray(want, np.float64)
    top = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got).astype(np.float64) - want).max())
    return err / top if top else (0.0 if not err else float("inf"))


def rel_err(got, want):
    """The largest elementwise relative error of `got` against float64 `want`, magnitudes floored at fp32 epsilon times the
    largest magnitude of `want` (so an element that should be 0 is measured against the tensor's scale)."""
    want = np.asarray(want, np.float64)
    got = np.asarray(got).astype(np.float64)
    floor = float(np.finfo(np.float32).eps) * float(np.abs(want).max())
    if floor == 0.0:
        return 0.0 if not np.abs(got).max() else float("inf")
    return float((np.abs(got - want) / np.maximum(np.abs(want), floor)).max())
