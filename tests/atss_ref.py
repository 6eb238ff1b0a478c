"""ATSS target assignment restated in numpy, brute force -- the checker of fd_atss_gen_targets.

Definition (this project's own).  Levels, strides and the location order (levels concatenated, row-major inside a level) are
those of fd_fcos_gen_targets.  Every fp32 operation below is one np.float32 operation (rounded once, no fused multiply-add);
step 3 runs in Python floats (fp64).  A ground-truth row is VALID when label >= 0, its four coordinates are finite and
x2 > x1, y2 > y1; other rows are padding.  For every valid row m of image b:

1. candidates   centre of location (px, py) of a level with stride s: c = ((float)(px*s) + (float)(s//2), same for y);
                box centre g = ((x1 + x2) / 2, (y1 + y2) / 2); d2 = (cx-gx)*(cx-gx) + (cy-gy)*(cy-gy);
                per level the k_l = min(topk, H_l*W_l) locations with the smallest (d2, pix), lexicographically (equal d2:
                lower row-major index); candidate order = levels ascending, then that rank
2. iou          anchor = c -/+ r, r = (anchor_scale * (float)s) / 2; IoU of anchor and box without the "+1", operation
                order of fd_pairwise_iou(plus_one = 0): inter / ((area_anchor + area_box) - inter)
3. threshold    over the n candidates in candidate order: mean = (sum iou) / n summed sequentially,
                std = sqrt(sum (iou - mean)^2 / (n - 1)) (0 when n == 1), thr = mean + std
4. positive     (double)iou >= thr  and  min(cx-x1, cy-y1, x2-cx, y2-cy) > inside_eps (fp32)
5. contest      a location positive for several rows goes to the largest fp32 iou, equal iou to the lowest row
6. outputs      cls [B, L] int64 label (0 negative), reg [B, L, 4] = (cx-x1, cy-y1, x2-cx, y2-cy) (-1 negative),
                cnt [B, L] = sqrt(min(l,r)*min(t,b) / (max(l,r)*max(t,b) + 1e-10)) (-1 negative)
"""
import math

import numpy as np

F = np.float32


def centres(level_hw, strides):
    """-> (cx [L], cy [L], level [L], pix [L]) in the location order of the kernels."""
    cx, cy, lv, px_ = [], [], [], []
    for l, ((h, w), s) in enumerate(zip(level_hw, strides)):
        pix = np.arange(h * w)
        py, px = pix // w, pix % w
        cx.append((px * s).astype(F) + F(s // 2))
        cy.append((py * s).astype(F) + F(s // 2))
        lv.append(np.full(h * w, l))
        px_.append(pix)
    return np.concatenate(cx), np.concatenate(cy), np.concatenate(lv), np.concatenate(px_)


def row_valid(box, label):
    return bool(label >= 0 and np.all(np.isfinite(box)) and box[2] > box[0] and box[3] > box[1])


def anchor_iou(cx, cy, s, anchor_scale, box):
    """fp32 IoU of the anchors centred on (cx, cy) [n] of stride s [n] with one box, fd_pairwise_iou(plus_one = 0) order."""
    with np.errstate(all="ignore"):
        r = (F(anchor_scale) * s.astype(F)) / F(2)
        ax1, ay1, ax2, ay2 = cx - r, cy - r, cx + r, cy + r
        ltx, lty = np.maximum(ax1, box[0]), np.maximum(ay1, box[1])
        rbx, rby = np.minimum(ax2, box[2]), np.minimum(ay2, box[3])
        w, h = np.maximum(rbx - ltx, F(0)), np.maximum(rby - lty, F(0))
        inter = w * h
        a1 = (ax2 - ax1) * (ay2 - ay1)
        a2 = (box[2] - box[0]) * (box[3] - box[1])
        return (inter / ((a1 + a2) - inter)).astype(F)


def threshold(ious):
    """Step 3 in Python floats, sequential sums in the given order -> thr."""
    n = len(ious)
    total = 0.0
    for v in ious:
        total += float(v)
    mean = total / n
    ss = 0.0
    for v in ious:
        d = float(v) - mean
        ss += d * d
    std = math.sqrt(ss / (n - 1)) if n > 1 else 0.0
    return mean + std


def candidates(box, level_hw, strides, topk):
    """Step 1 for one box -> global location indices in candidate order."""
    cx, cy, lv, pix = centres(level_hw, strides)
    with np.errstate(all="ignore"):
        gx, gy = (box[0] + box[2]) / F(2), (box[1] + box[3]) / F(2)
        dx, dy = cx - gx, cy - gy
        d2 = dx * dx + dy * dy
    out, start = [], 0
    for l, (h, w) in enumerate(level_hw):
        k = min(topk, h * w)
        order = sorted(range(h * w), key=lambda p: (float(d2[start + p]), p))
        out += [start + p for p in order[:k]]
        start += h * w
    return np.array(out, dtype=np.int64)


def atss_gen_targets(gt_boxes, labels, level_hw, strides, topk=9, anchor_scale=8.0, inside_eps=0.01):
    """gt_boxes [B, M, 4], labels [B, M] -> dict(cls [B, L] int64, cnt [B, L] f32, reg [B, L, 4] f32, thr [B, M] f64 (NaN for
    padding), npos [B, M] int32 (positives of step 4), claims [B, L] int32 (rows positive at the location), cand: {(b, m): loc})."""
    gt = np.asarray(gt_boxes, dtype=F).reshape(len(labels), -1, 4)
    labels = np.asarray(labels, dtype=np.int64)
    B, M = labels.shape
    cx, cy, lv, _ = centres(level_hw, strides)
    st = np.asarray(strides)[lv]
    L = len(cx)
    cls = np.zeros((B, L), np.int64)
    cnt = np.full((B, L), -1, F)
    reg = np.full((B, L, 4), -1, F)
    thr = np.full((B, M), np.nan, np.float64)
    npos = np.zeros((B, M), np.int32)
    claims = np.zeros((B, L), np.int32)
    best_iou = np.full((B, L), -1, F)
    owner = np.full((B, L), -1, np.int64)
    cand = {}
    for b in range(B):
        for m in range(M):
            box = gt[b, m]
            if not row_valid(box, labels[b, m]):
                continue
            c = candidates(box, level_hw, strides, topk)
            cand[(b, m)] = c
            iou = anchor_iou(cx[c], cy[c], st[c], anchor_scale, box)
            t = threshold(iou)
            thr[b, m] = t
            with np.errstate(all="ignore"):
                inside = np.minimum(np.minimum(cx[c] - box[0], cy[c] - box[1]), np.minimum(box[2] - cx[c], box[3] - cy[c]))
            for j, loc in enumerate(c):
                if float(iou[j]) >= t and inside[j] > F(inside_eps):
                    npos[b, m] += 1
                    claims[b, loc] += 1
                    if owner[b, loc] < 0 or iou[j] > best_iou[b, loc]:      # rows ascend: an equal iou keeps the lower row
                        owner[b, loc], best_iou[b, loc] = m, iou[j]
        for loc in np.nonzero(owner[b] >= 0)[0]:
            box = gt[b, owner[b, loc]]
            off = np.array([cx[loc] - box[0], cy[loc] - box[1], box[2] - cx[loc], box[3] - cy[loc]], dtype=F)
            lr_min, lr_max = min(off[0], off[2]), max(off[0], off[2])
            tb_min, tb_max = min(off[1], off[3]), max(off[1], off[3])
            cls[b, loc] = labels[b, owner[b, loc]]
            reg[b, loc] = off
            with np.errstate(all="ignore"):
                cnt[b, loc] = np.sqrt((lr_min * tb_min) / (lr_max * tb_max + F(1e-10)))
    return dict(cls=cls, cnt=cnt, reg=reg, thr=thr, npos=npos, claims=claims, cand=cand, owner=owner)
