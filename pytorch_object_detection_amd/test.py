"""VOC mAP evaluation on the device: the drop-in for the reference's test.py (sort_by_score, eval_ap_2d, evaluate).

The arithmetic is the reference's (test.py:15-162, 225-238), quirks included: per image, detections in descending score order;
per detection, the argmax GT box of its label (fp32 IoU without "+1", first maximum, NaN wins) is a true positive only if
unassigned -- a taken box makes it a false positive, with no fall-back to the next best; per label, detections of all images
sorted by score, fp64 running recall / precision, the precision envelope and the change-point sum in numpy's pairwise order.
The per-label AP is bit-identical to the reference's.  The one intended difference: detections with exactly equal scores keep
their (image, rank) order (a stable sort), where the reference's np.argsort quicksort may permute them.  The kernels are in
csrc/fd_eval.hip (fd_eval_ap, include/fcosdet.h).
"""
from __future__ import annotations

import time
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import FdError
from .model.modules.head import ClipBoxes, FCOSHead

VOC_CLASSES = ("__background__ ", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair",
               "cow", "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa",
               "train", "tvmonitor",)
MAX_DETECTIONS = 1024       # per image (fd_eval_ap's K limit)
MAX_GT = 512                # per image (fd_eval_ap's G limit)


def _mean_ap(ap_row: np.ndarray, num_cls: int) -> float:
    """evaluate's mAP (test.py:234-237): a Python float sum over the labels in order, divided by num_cls - 1 (NaN propagates)."""
    m = 0.
    for v in ap_row:
        m += float(v)
    return m / (num_cls - 1)


class VOCEvaluator:
    """Accumulates detections and GT boxes on the device, then computes VOC AP in one library call.

    add() takes what FCOSHead.detect_padded + ClipBoxes produce and what the VOC collate yields, and only enqueues device copies
    (no host synchronisation); batches may differ in K (detections per image) and G (GT rows per image).  compute() runs
    fd_eval_ap once and copies one packed result to the host."""

    def __init__(self, num_cls: int = 21, iou_thresholds: Sequence[float] = (0.5,), device=None):
        if not 2 <= num_cls <= 128 or not 1 <= len(iou_thresholds) <= 16:
            raise FdError(f"VOCEvaluator: needs 2 <= num_cls <= 128 and 1 .. 16 thresholds (got {num_cls}, {len(iou_thresholds)})")
        self.num_cls = int(num_cls)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.device = torch.device(device) if device is not None else None
        self._n = 0
        self._bufs = None       # scores [cap, K] f32, classes [cap, K] int64 (0 = not taking part), boxes [cap, K, 4], gt boxes [cap, G, 4], gt classes [cap, G] (-1 = padding)

    def reset(self) -> None:
        """Forget every image added; the device buffers are kept for reuse (add() overwrites the rows it appends in full)."""
        self._n = 0

    @property
    def num_images(self) -> int:
        return self._n

    def _alloc(self, cap: int, K: int, G: int, dev):
        return (torch.zeros(cap, K, dtype=torch.float32, device=dev), torch.zeros(cap, K, dtype=torch.int64, device=dev),
                torch.zeros(cap, K, 4, dtype=torch.float32, device=dev), torch.zeros(cap, G, 4, dtype=torch.float32, device=dev),
                torch.full((cap, G), -1, dtype=torch.int64, device=dev))

    def _reserve(self, n: int, K: int, G: int, dev) -> None:
        if self._bufs is None:
            self._bufs = self._alloc(max(n, 64), K, G, dev)
            return
        s, c, b, gb, gc = self._bufs
        cap, K0, G0 = s.shape[0], s.shape[1], gc.shape[1]
        if n <= cap and K <= K0 and G <= G0:
            return
        new = self._alloc(max(n, 2 * cap) if n > cap else cap, max(K, K0), max(G, G0), dev)
        m = self._n
        new[0][:m, :K0] = s[:m]
        new[1][:m, :K0] = c[:m]
        new[2][:m, :K0] = b[:m]
        new[3][:m, :G0] = gb[:m]
        new[4][:m, :G0] = gc[:m]
        self._bufs = new

    def add(self, scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, counts: Optional[torch.Tensor],
            gt_boxes: torch.Tensor, gt_classes: torch.Tensor) -> None:
        """scores [B,K], classes [B,K] (1-based), boxes [B,K,4], counts [B] (rows >= counts[b] ignored; None = all rows), gt_boxes
        [B,G,4], gt_classes [B,G] (-1 = padding).  Device tensors only."""
        ops._need_gpu(scores, classes, boxes, counts, gt_boxes, gt_classes)
        B, K = scores.shape
        G = gt_classes.shape[1]
        if tuple(classes.shape) != (B, K) or tuple(boxes.shape) != (B, K, 4) or tuple(gt_boxes.shape) != (B, G, 4) or gt_classes.shape[0] != B:
            raise FdError("VOCEvaluator.add: shapes do not agree")
        if K > MAX_DETECTIONS or G > MAX_GT:
            raise FdError(f"VOCEvaluator.add: at most {MAX_DETECTIONS} detections and {MAX_GT} GT rows per image (got K={K}, G={G})")
        dev = scores.device
        if self.device is None:
            self.device = dev
        n = self._n
        self._reserve(n + B, K, G, dev)
        s, c, b, gb, gc = self._bufs
        cls = classes.to(torch.int64)
        if counts is not None:
            cls = torch.where(torch.arange(K, device=dev)[None, :] < counts.to(dev)[:, None].to(torch.int64), cls, torch.zeros_like(cls))
        # the rows are written across the buffers' full width: columns past K / G are marked as not taking part, whatever
        # an earlier (wider) batch left there before a reset()
        s[n:n + B, :K] = scores
        c[n:n + B, :K] = cls
        c[n:n + B, K:] = 0
        b[n:n + B, :K] = boxes
        gb[n:n + B, :G] = gt_boxes
        gc[n:n + B, :G] = gt_classes
        gc[n:n + B, G:] = -1
        self._n = n + B

    def compute(self) -> Dict[str, np.ndarray]:
        """-> {"ap": [T, num_cls-1] f64 (labels 1 ..), "mAP": [T], "n_gt", "n_pred": [num_cls-1], "n_tp": [T, num_cls-1],
        "iou_thresholds": [T]}."""
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n = max(self._n, 1)
        if self._n == 0:        # nothing added since construction or reset(): one image without detections or GT (every label: AP 0)
            self._reserve(1, 1, 1, dev)
            self._bufs[1][0] = 0
            self._bufs[4][0] = -1
        s, c, b, gb, gc = self._bufs
        T, Cn = len(self.iou_thresholds), self.num_cls
        out = torch.empty(ops.eval_ap_bytes(T, Cn), dtype=torch.uint8, device=dev)
        ops.eval_ap(s[:n], c[:n], b[:n], None, gb[:n], gc[:n], None, Cn, self.iou_thresholds, out=out)
        ap, n_gt, n_pred, n_tp = (t.numpy() for t in ops.eval_ap_views(out.cpu(), T, Cn))
        return {"ap": ap[:, 1:].copy(), "mAP": np.array([_mean_ap(ap[t, 1:], Cn) for t in range(T)]), "n_gt": n_gt[1:].copy(),
                "n_pred": n_pred[1:].copy(), "n_tp": n_tp[:, 1:].copy(), "iou_thresholds": np.array(self.iou_thresholds, dtype=np.float32)}


def sort_by_score(pred_boxes, pred_labels, pred_scores):
    """Host helper with the reference's signature (test.py:15-20): each image's predictions reordered by descending score
    (np.argsort of the negated scores, as there).  The device path sorts by itself; this stays so that imports resolve."""
    order = [np.argsort(-np.asarray(s)) for s in pred_scores]
    return ([np.asarray(x)[o] for x, o in zip(pred_boxes, order)], [np.asarray(x)[o] for x, o in zip(pred_labels, order)],
            [np.asarray(x)[o] for x, o in zip(pred_scores, order)])


def eval_ap_2d(gt_boxes, gt_labels, pred_boxes, pred_labels, pred_scores, iou_thread, num_cls):
    """The reference's eval_ap_2d (test.py:85-162) on the GPU: lists of per-image numpy arrays in, {label: np.float64 AP} out.
    Each image's predictions are matched in the order given (as the reference does; sort_by_score is the caller's step).  Boxes
    and scores are taken as fp32 -- what evaluate feeds -- and the threshold compares in fp32, as numpy >= 2 does."""
    N = len(gt_boxes)
    if not (len(gt_labels) == len(pred_boxes) == len(pred_labels) == len(pred_scores) == N):
        raise FdError("eval_ap_2d: the five lists must have one entry per image")
    Nn = max(N, 1)
    K = max([len(x) for x in pred_scores] + [1])
    G = max([len(x) for x in gt_labels] + [1])
    if K > MAX_DETECTIONS or G > MAX_GT:
        raise FdError(f"eval_ap_2d: at most {MAX_DETECTIONS} predictions and {MAX_GT} GT boxes per image (got {K}, {G})")
    s = np.zeros((Nn, K), np.float32)
    c = np.zeros((Nn, K), np.int64)
    b = np.zeros((Nn, K, 4), np.float32)
    gb = np.zeros((Nn, G, 4), np.float32)
    gc = np.full((Nn, G), -1, np.int64)
    for i in range(N):
        k, g = len(pred_scores[i]), len(gt_labels[i])
        if k:
            s[i, :k] = np.asarray(pred_scores[i], np.float32).reshape(k)
            c[i, :k] = np.asarray(pred_labels[i]).reshape(k).astype(np.int64)
            b[i, :k] = np.asarray(pred_boxes[i], np.float32).reshape(k, 4)
        if g:
            gc[i, :g] = np.asarray(gt_labels[i]).reshape(g).astype(np.int64)
            gb[i, :g] = np.asarray(gt_boxes[i], np.float32).reshape(g, 4)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = [torch.from_numpy(a).to(dev) for a in (s, c, b, gb, gc)]
    ap = ops.eval_ap(up[0], up[1], up[2], None, up[3], up[4], None, int(num_cls), (float(iou_thread),), flags=ops.EVAL_INPUT_ORDER)[0]
    ap = ap.cpu().numpy()
    return {label: np.float64(ap[0, label]) for label in range(1, int(num_cls))}


def evaluate(model: torch.nn.Module, val_data_loader, amp_enable: bool, ddp_enable: bool, devices, strides=None):
    """The reference's evaluate (test.py:165-238): FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64]) -- four strides, reproducing the
    reference's dropped P7; `strides=` overrides -- then ClipBoxes, autocast flag, per-class / mAP / fps prints.
    Detections stay on the device (VOCEvaluator).  Every image of a batch is evaluated (the reference takes index 0 only; the
    two agree at its batch size of 1).  Each rank evaluates what it saw: there is no cross-rank gather.
    -> {"ap": {label: AP at IoU 0.5}, "mAP": float, "fps": float, "result": VOCEvaluator.compute()}."""
    model.eval()
    local_rank = torch.distributed.get_rank() if ddp_enable else 0
    head = FCOSHead(0.05, 0.6, 1000, list(strides) if strides is not None else [8, 16, 32, 64])
    clip = ClipBoxes()
    num_cls = len(VOC_CLASSES)
    ev = VOCEvaluator(num_cls, (0.5,), device=devices)
    inference_time = 0.0
    nb = 0
    for imgs, targets, classes in val_data_loader:
        imgs, targets, classes = imgs.to(devices), targets.to(devices), classes.to(devices)
        with torch.autocast("cuda", enabled=amp_enable):
            torch.cuda.synchronize()
            start_time = time.time()
            with torch.no_grad():
                out = model(imgs)
                score, cls, boxes, counts = head.detect_padded(out)
                box = clip(imgs, boxes)
                ev.add(score.float(), cls, box.float(), counts, targets.float(), classes)
            torch.cuda.synchronize()
            inference_time += time.time() - start_time
        nb += 1
    fps = 1.0 / (inference_time / nb) if nb and inference_time > 0 else float("nan")
    res = ev.compute()
    all_ap = {label: np.float64(res["ap"][0, label - 1]) for label in range(1, num_cls)}
    m_ap = float(res["mAP"][0])
    if local_rank == 0:
        print('all Classes AP\n')
        for key, value in all_ap.items():
            print(f'{VOC_CLASSES[int(key)]}: {value}')
        print(f'mAP: {m_ap:.3f}\n fps: {fps}')
    return {"ap": all_ap, "mAP": m_ap, "fps": fps, "result": res}
