"""numpy restatement of the anchor codec (fd_anchor.hip): DataEncoder's anchors, encode and decode in fp32,
one IEEE rounding per operation, plus what the reference does not have -- the repaired cases (one candidate, an image
without boxes) and the max_candidates cap.  tests/golden/g15_anchor_codec.npz holds the REAL reference's outputs; this file
is checked against it (test_anchor_cpu.py) and then stands in for the reference where the reference raises.

Also the deterministic inputs of the decode cases: [A, C] logits are regenerated on both sides from tests/golden/lcg.py
instead of being stored (774 x 80 floats would be most of the fixture's size budget)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import lcg  # noqa: E402

F = np.float32
AREAS = [32 * 32., 64 * 64., 128 * 128., 256 * 256., 512 * 512.]
RATIOS = [1 / 2., 1 / 1., 2 / 1.]
SCALES = [1., pow(2, 1 / 3.), pow(2, 2 / 3.)]


def anchor_wh() -> np.ndarray:
    rows = []
    for area in AREAS:
        for ratio in RATIOS:
            h = math.sqrt(area / ratio)
            w = ratio * h
            rows.extend([w * s, h * s] for s in SCALES)
    return np.array(rows, np.float64).astype(F).reshape(5, 9, 2)


def _size(input_size) -> np.ndarray:
    return np.array([input_size, input_size] if isinstance(input_size, (int, float)) else list(input_size), F)


def fm_sizes(input_size):
    size = _size(input_size)
    return [tuple(int(v) for v in np.ceil(size / F(2.0 ** (i + 3)))) for i in range(5)]


def num_anchors(input_size) -> int:
    return 9 * sum(w * h for w, h in fm_sizes(input_size))


def anchor_boxes(input_size) -> np.ndarray:
    """[A, 4] fp32 (cx, cy, w, h); rows ordered level, y, x, anchor."""
    size, wh, out = _size(input_size), anchor_wh(), []
    for i, (fw, fh) in enumerate(fm_sizes(input_size)):
        grid = size / np.array([fw, fh], F)
        xs = (np.arange(fw, dtype=F) + F(0.5)) * grid[0]
        ys = (np.arange(fh, dtype=F) + F(0.5)) * grid[1]
        box = np.empty((fh, fw, 9, 4), F)
        box[..., 0] = xs[None, :, None]
        box[..., 1] = ys[:, None, None]
        box[..., 2:] = wh[i][None, None]
        out.append(box.reshape(-1, 4))
    return np.concatenate(out, 0)


def _corners(xywh: np.ndarray) -> np.ndarray:
    return np.concatenate([xywh[:, :2] - xywh[:, 2:] / F(2), xywh[:, :2] + xywh[:, 2:] / F(2)], 1)


def iou_plus1(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[N, 4] x [M, 4] xyxy -> [N, M], the '+1' convention, fp32 in the reference's order of operations."""
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.maximum((rb - lt) + F(1), F(0))
    inter = wh[..., 0] * wh[..., 1]
    a1 = ((a[:, 2] - a[:, 0]) + F(1)) * ((a[:, 3] - a[:, 1]) + F(1))
    a2 = ((b[:, 2] - b[:, 0]) + F(1)) * ((b[:, 3] - b[:, 1]) + F(1))
    return inter / ((a1[:, None] + a2[None]) - inter)


def encode(boxes, labels, input_size):
    """boxes [M, 4] xyxy, labels [M] (rows with label < 0 are padding) -> (loc [A, 4] fp32, cls [A] int64, max_iou [A])."""
    boxes, labels = np.asarray(boxes, F).reshape(-1, 4), np.asarray(labels, np.int64).reshape(-1)
    keep = labels >= 0
    boxes, labels = boxes[keep], labels[keep]
    anchors = anchor_boxes(input_size)
    A = anchors.shape[0]
    if boxes.shape[0] == 0:
        return np.zeros((A, 4), F), np.zeros(A, np.int64), np.zeros(A, F)
    a, b = boxes[:, :2], boxes[:, 2:]
    xywh = np.concatenate([(a + b) / F(2), (b - a) + F(1)], 1)
    ious = iou_plus1(_corners(anchors), _corners(xywh))
    ids = ious.argmax(1)                                   # first maximum
    mx = ious[np.arange(A), ids]
    g = xywh[ids]
    loc = np.concatenate([(g[:, :2] - anchors[:, :2]) / anchors[:, 2:], np.log(g[:, 2:] / anchors[:, 2:])], 1).astype(F)
    cls = 1 + labels[ids]
    cls[mx < F(0.5)] = 0
    cls[(mx > F(0.4)) & (mx < F(0.5))] = -1
    return loc, cls, mx


def sigmoid(x: np.ndarray) -> np.ndarray:
    return (F(1) / (F(1) + np.exp(-x.astype(F)))).astype(F)


def nms_plus1(boxes: np.ndarray, scores: np.ndarray, thr: float = 0.5):
    """Greedy NMS, '+1' areas, keep while ovr <= thr; scores descending, ties by lower index.  -> kept indices."""
    order = list(np.lexsort((np.arange(len(scores)), -scores.astype(np.float64))))
    keep = []
    while order:
        i = order.pop(0)
        keep.append(i)
        if not order:
            break
        ovr = iou_plus1(boxes[i:i + 1], boxes[order])[0]
        order = [j for j, o in zip(order, ovr) if o <= F(thr)]
    return np.array(keep, np.int64)


def decode_boxes(loc: np.ndarray, input_size) -> np.ndarray:
    anchors = anchor_boxes(input_size)
    xy = loc[:, :2] * anchors[:, 2:] + anchors[:, :2]
    wh = np.exp(loc[:, 2:]).astype(F) * anchors[:, 2:]
    return np.concatenate([xy - wh / F(2), xy + wh / F(2)], 1)


def decode(loc, cls, input_size, cls_thresh=0.5, nms_thresh=0.5, max_candidates=1000):
    """loc [A, 4], cls [A, C] logits -> (boxes [n, 4], labels [n] int64, scores [n], n_candidates): score-descending rows
    kept by the NMS.  More than max_candidates candidates: the best max_candidates by score (ties: lower row) go on."""
    loc, cls = np.asarray(loc, F), np.asarray(cls, F)
    boxes = decode_boxes(loc, input_size)
    sg = sigmoid(cls)
    labels = sg.argmax(1)                                  # first maximum over the sigmoid VALUES
    score = sg[np.arange(sg.shape[0]), labels]
    ids = np.nonzero(score > F(cls_thresh))[0]
    n_cand = len(ids)
    if n_cand > max_candidates:
        top = np.lexsort((ids, -score[ids].astype(np.float64)))[:max_candidates]
        ids = np.sort(ids[top])
    keep = nms_plus1(boxes[ids], score[ids], nms_thresh) if len(ids) else np.zeros(0, np.int64)
    return boxes[ids][keep], labels[ids][keep].astype(np.int64), score[ids][keep], n_cand


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in units in the last place between fp32 arrays (finite values; -0 == +0)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------------- the decode cases
# name -> (C, number of candidate rows, seed).  Every case is at input size (64, 64): A = 774.
DECODE_SIZE = (64, 64)
# The seeds were picked so that no two candidate boxes have an IoU within 3e-4 of the NMS threshold (the fixture's maker asserts 1e-4).
DECODE_CASES = {"c20": (20, 60, 207), "c80": (80, 275, 273), "c3": (3, 40, 203), "zero": (20, 0, 204), "saturated": (20, 30, 211),
                "single": (20, 1, 206)}
SATURATED_ROW, SATURATED_LOGITS = 417, [(5, 30.0), (2, 20.0), (9, 25.0), (17, 88.0)]     # every one gives 1.0f: label 2


def decode_case(name: str):
    """(loc [A, 4], cls [A, C]) fp32 of a decode case, the same on every platform.  Background logits sit around -log 99, well
    below 0 and pairwise distinct within a row; `n` rows get one positive class logit each, all distinct multiples of 0.012 (sigmoid values >= 1e-4 apart), with
    the runner-up of the row >= 0.04 below; loc is uniform in (-0.3, 0.3), so boxes of neighbouring anchors overlap and the NMS
    has work to do.  "saturated" adds one row whose logits are >= 20 in several classes: they all give 1.0f, the lowest of those classes wins
    (one row only: two rows at 1.0f would tie in the sort, whose order the reference leaves open)."""
    C, n, seed = DECODE_CASES[name]
    A = num_anchors(DECODE_SIZE)
    # background: per row a permutation of C grid levels in (-5.35, -3.85), each moved by less than half a step: distinct by >= 0.009
    order = np.argsort(lcg.u01(A * C, seed).reshape(A, C), 1, kind="stable").astype(F)
    cls = ((order + F(0.5) * lcg.u01(A * C, seed + 500).reshape(A, C)) * F(1.5 / C) - F(4.6 + 0.75)).astype(F)
    loc = (lcg.u01(A * 4, seed + 1000) * F(0.6) - F(0.3)).astype(F).reshape(A, 4)
    perm = np.argsort(lcg.u01(A, seed + 2000), kind="stable")
    rows = np.sort(perm[:n])
    rank = np.argsort(lcg.u01(max(n, 1), seed + 3000), kind="stable")[:n]
    col = (lcg.u01(max(n, 1), seed + 4000) * F(C)).astype(np.int64).clip(0, C - 1)[:n]
    for r, k, c in zip(rows, rank, col):
        cls[r, c] = F(0.06) + F(0.012) * F(k)
        cls[r, (c + 1) % C] = cls[r, c] - F(0.04) - F(0.5) * lcg.u01(1, seed + 5000 + int(r))[0]
    if name == "saturated":
        for c, v in SATURATED_LOGITS:
            cls[SATURATED_ROW, c] = F(v)
    return loc, cls
