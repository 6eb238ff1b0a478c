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
import zlib
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import dist as _dist
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
    fd_eval_ap once and copies one packed result to the host.

    Under sharded evaluation every rank fills its own evaluator and gather() returns the union on every rank.
    Image ids (add(image_ids=...)) let the union drop the images a padding sampler handed to two ranks and put the rest in id
    order, which fixes the order among equal scores; without ids the union is every row in (rank, arrival) order."""

    def __init__(self, num_cls: int = 21, iou_thresholds: Sequence[float] = (0.5,), device=None):
        if not 2 <= num_cls <= 128 or not 1 <= len(iou_thresholds) <= 16:
            raise FdError(f"VOCEvaluator: needs 2 <= num_cls <= 128 and 1 .. 16 thresholds (got {num_cls}, {len(iou_thresholds)})")
        self.num_cls = int(num_cls)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.device = torch.device(device) if device is not None else None
        self._n = 0
        self._bufs = None       # scores [cap, K] f32, classes [cap, K] int64 (0 = not taking part), boxes [cap, K, 4], gt boxes [cap, G, 4], gt classes [cap, G] (-1 = padding)
        self._ids = None        # image id of each added row; None: add() was given no ids (or nothing was added yet)

    def reset(self) -> None:
        """Forget every image added; the device buffers are kept for reuse (add() overwrites the rows it appends in full)."""
        self._n = 0
        self._ids = None

    def _take_ids(self, image_ids, B: int) -> None:
        """One evaluator takes ids on every add() or on none; an id is added once."""
        if image_ids is None:
            if self._ids is not None:
                raise FdError("VOCEvaluator.add: earlier batches came with image_ids, this one without")
            return
        ids = [int(i) for i in image_ids]
        if self._ids is None and self._n:
            raise FdError("VOCEvaluator.add: earlier batches came without image_ids, this one with")
        if len(ids) != B:
            raise FdError(f"VOCEvaluator.add: {len(ids)} image_ids for {B} images")
        seen = set(self._ids or ())
        for i in ids:
            if i in seen:
                raise FdError(f"VOCEvaluator.add: image id {i} added twice")
            seen.add(i)
        self._ids = (self._ids or []) + ids

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
            gt_boxes: torch.Tensor, gt_classes: torch.Tensor, *, image_ids: Optional[Sequence[int]] = None) -> None:
        """scores [B,K], classes [B,K] (1-based), boxes [B,K,4], counts [B] (rows >= counts[b] ignored; None = all rows), gt_boxes
        [B,G,4], gt_classes [B,G] (-1 = padding).  Device tensors only.  image_ids: B host ints, on every add() or on none."""
        ops._need_gpu(scores, classes, boxes, counts, gt_boxes, gt_classes)
        B, K = scores.shape
        G = gt_classes.shape[1]
        if tuple(classes.shape) != (B, K) or tuple(boxes.shape) != (B, K, 4) or tuple(gt_boxes.shape) != (B, G, 4) or gt_classes.shape[0] != B:
            raise FdError("VOCEvaluator.add: shapes do not agree")
        if K > MAX_DETECTIONS or G > MAX_GT:
            raise FdError(f"VOCEvaluator.add: at most {MAX_DETECTIONS} detections and {MAX_GT} GT rows per image (got K={K}, G={G})")
        self._take_ids(image_ids, B)
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

    def _assign_ids(self, image_ids) -> None:
        """Name the rows added so far (all of them without ids) after the fact: evaluate() learns its sampler's ids this way."""
        ids = [int(i) for i in image_ids]
        if self._ids is not None or len(ids) != self._n:
            raise FdError(f"VOCEvaluator: {len(ids)} image ids for {self._n} rows, or the rows carry ids already")
        if len(set(ids)) != len(ids):
            raise FdError("VOCEvaluator: an image id added twice")
        self._ids = ids

    def gather(self, group=None, force: bool = False) -> "VOCEvaluator":
        """The union of every rank's evaluator, as a new evaluator on this rank's device; every rank must call it, and every
        rank gets the same rows.  With image ids: each distinct id once (of an id two ranks hold, the lowest rank's row), ids
        ascending.  Without: every row, rank 0's first, in arrival order.  Two collectives (dist.gather_rows); num_cls, the
        thresholds and the with / without ids choice travel in the first and a disagreement raises FdError on every rank.
        No process group, or world size 1 without `force`: returns self."""
        if _dist._no_group(group, force):
            return self
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n = self._n
        bufs = self._bufs if self._bufs is not None else self._alloc(0, 0, 0, dev)
        ids = torch.tensor(self._ids if (n and self._ids is not None) else [0] * n, dtype=torch.int64).to(dev)
        header = (self.num_cls, len(self.iou_thresholds), zlib.crc32(np.asarray(self.iou_thresholds, np.float64).tobytes()),
                  -1 if n == 0 else int(self._ids is not None))
        got, _, headers = _dist._gather_rows(list(bufs) + [ids], n, group, (0, 0, 0, 0, -1, 0), header)
        out = VOCEvaluator(self.num_cls, self.iou_thresholds, device=dev)
        all_ids = got.pop()
        if int(headers[:, 3].max()) == 1:
            order = _dist.merge_order(all_ids.cpu())
            out._ids = all_ids.cpu()[order].tolist()
            got = [t.index_select(0, order.to(dev)) for t in got]
        if got[0].shape[0]:
            out._bufs, out._n = tuple(got), got[0].shape[0]
        return out

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


def evaluate(model: torch.nn.Module, val_data_loader, amp_enable: bool, ddp_enable: bool, devices, strides=None, gather: bool = False):
    """The reference's evaluate (test.py:165-238): FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64]) -- four strides, reproducing the
    reference's dropped P7; `strides=` overrides -- then ClipBoxes, autocast flag, per-class / mAP / fps prints.
    Detections stay on the device (VOCEvaluator).  Every image of a batch is evaluated (the reference takes index 0 only; the
    two agree at its batch size of 1).

    gather=False: the result covers what this rank's loader yielded, and a call on one rank alone is fine; `ddp_enable` only
    says that the printing rank is the process group's rank 0.  gather=True: EVERY rank must call; after the loop the ranks'
    evaluators are merged (VOCEvaluator.gather: two collectives) and every rank computes the same, global, result, which rank 0
    prints.  The images are named by list(val_data_loader.sampler) when the loader has a sampler that long -- what a
    DistributedSampler gives, padding included, so an image two ranks were handed counts once and the merged order is the data
    set's; otherwise the rows merge unnamed, in (rank, arrival) order.  Without a process group gather=True changes nothing.
    -> {"ap": {label: AP at IoU 0.5}, "mAP": float, "fps": float (this rank's), "result": VOCEvaluator.compute(), "images":
    distinct images evaluated, "world": ranks the result covers}."""
    model.eval()
    grouped = gather and torch.distributed.is_available() and torch.distributed.is_initialized()
    local_rank = torch.distributed.get_rank() if (ddp_enable or grouped) else 0
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
    world = 1
    if gather and not _dist._no_group(None, False):     # more than one rank: name the rows, merge
        sampler = getattr(val_data_loader, "sampler", None)
        if sampler is not None and hasattr(sampler, "__len__") and hasattr(sampler, "__iter__") and len(sampler) == ev.num_images:
            ev._assign_ids(list(sampler))
        ev = ev.gather()
        world = torch.distributed.get_world_size()
    res = ev.compute()
    all_ap = {label: np.float64(res["ap"][0, label - 1]) for label in range(1, num_cls)}
    m_ap = float(res["mAP"][0])
    if local_rank == 0:
        print('all Classes AP\n')
        for key, value in all_ap.items():
            print(f'{VOC_CLASSES[int(key)]}: {value}')
        print(f'mAP: {m_ap:.3f}\n fps: {fps}')
    return {"ap": all_ap, "mAP": m_ap, "fps": fps, "result": res, "images": ev.num_images, "world": world}
