"""COCO bbox evaluation on the device: the drop-in for the reference's Test_coco.py (evaluate_coco) without pycocotools.

The arithmetic is COCOeval's for iouType 'bbox' with default Params (include/fcosdet.h fd_eval_coco): per (image, category) the
top 100 detections by score, fp64 bbIou (crowd: over the detection's area), greedy matching per area range and IoU threshold to
the last best GT row (non-ignored rows first), then per (category, area, maxDets) the stable score sort across images in id
order, cumulative TP / FP, the precision envelope sampled at 101 recall thresholds.  `precision` and `recall` are bit-identical
to that restatement (tests/coco_eval_ref.py); the 12 summary numbers are COCOeval.summarize's, computed here in numpy from them.
The kernels are in csrc/fd_eval.hip.
"""
from __future__ import annotations

import json
import zlib
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import dist as _dist
from . import ops
from ._lib import FdError
from .model.modules.head import ClipBoxes, FCOSHead

MAX_DETECTIONS = 1024       # per image (fd_eval_coco's K limit)
MAX_GT = 512                # per image (fd_eval_coco's G limit)
MAX_CATEGORIES = 128
AREA_LBL = ("all", "small", "medium", "large")


class CocoGT:
    """Per-image GT arrays of an instances file: row order within an image is the file's annotation order."""

    def __init__(self, image_ids, category_ids, boxes, area, crowd, labels):
        self.image_ids = image_ids          # [Ni] int64, the file's image order
        self.category_ids = category_ids    # [C] int64 ascending; label l (1 .. C) is category_ids[l - 1]
        self.boxes = boxes                  # [Ni, G, 4] f64 xywh
        self.area = area                    # [Ni, G] f64 (the annotation's "area")
        self.crowd = crowd                  # [Ni, G] uint8
        self.labels = labels                # [Ni, G] int64, -1 = padding
        self.index = {int(i): n for n, i in enumerate(image_ids)}

    @property
    def num_cats(self) -> int:
        return len(self.category_ids)

    def label_of(self, category_id: int) -> int:
        """Contiguous label (1 .. C) of a COCO category id; 0 when the GT file has no such category."""
        k = int(np.searchsorted(self.category_ids, category_id))
        return k + 1 if k < len(self.category_ids) and self.category_ids[k] == category_id else 0


def load_coco_gt(src) -> CocoGT:
    """`src`: an instances JSON path, its dict, or an object with a `.dataset` dict (a pycocotools COCO).  Plain json, no pycocotools.
    Annotations of categories the file does not list take no part (COCOeval's useCats)."""
    if isinstance(src, CocoGT):
        return src
    if hasattr(src, "dataset"):
        src = src.dataset
    if not isinstance(src, dict):
        with open(src) as f:
            src = json.load(f)
    image_ids = np.array([int(im["id"]) for im in src.get("images", [])], dtype=np.int64)
    cat_ids = np.array(sorted({int(c["id"]) for c in src.get("categories", [])}), dtype=np.int64)
    if len(cat_ids) == 0 or len(cat_ids) > MAX_CATEGORIES:
        raise FdError(f"load_coco_gt: needs 1 .. {MAX_CATEGORIES} categories (got {len(cat_ids)})")
    if len(set(image_ids.tolist())) != len(image_ids):
        raise FdError("load_coco_gt: duplicate image ids")
    index = {int(i): n for n, i in enumerate(image_ids)}
    cat_label = {int(c): k + 1 for k, c in enumerate(cat_ids)}
    rows = [[] for _ in image_ids]
    for ann in src.get("annotations", []):
        n = index.get(int(ann["image_id"]))
        lab = cat_label.get(int(ann["category_id"]), 0)
        if n is None or lab == 0:
            continue
        rows[n].append((lab, [float(v) for v in ann["bbox"]], float(ann["area"]), 1 if ann.get("iscrowd", 0) else 0))
    G = max([len(r) for r in rows] + [1])
    if G > MAX_GT:
        raise FdError(f"load_coco_gt: at most {MAX_GT} annotations per image (got {G})")
    Ni = max(len(image_ids), 1)
    boxes, area = np.zeros((Ni, G, 4)), np.zeros((Ni, G))
    crowd, labels = np.zeros((Ni, G), np.uint8), np.full((Ni, G), -1, np.int64)
    for n, r in enumerate(rows):
        for j, (lab, bb, ar, cr) in enumerate(r):
            labels[n, j], boxes[n, j], area[n, j], crowd[n, j] = lab, bb, ar, cr
    return CocoGT(image_ids, cat_ids, boxes, area, crowd, labels)


def coco_stats(precision: np.ndarray, recall: np.ndarray, iou_thrs=ops.COCO_IOU_THRS, max_dets=ops.COCO_MAX_DETS) -> np.ndarray:
    """COCOeval.summarize's 12 numbers (summarizeDets), with its slicing: mean of the cells > -1, or -1."""
    iou_thrs = np.asarray(iou_thrs, np.float64)

    def one(ap, iou_thr=None, area="all", md=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, m in enumerate(max_dets) if m == md]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    m = max_dets
    return np.array([one(1, md=m[2]), one(1, .5, md=m[2]), one(1, .75, md=m[2]), one(1, area="small", md=m[2]),
                     one(1, area="medium", md=m[2]), one(1, area="large", md=m[2]), one(0, md=m[0]), one(0, md=m[1]), one(0, md=m[2]),
                     one(0, area="small", md=m[2]), one(0, area="medium", md=m[2]), one(0, area="large", md=m[2])], dtype=np.float64)


def format_stats(stats, iou_thrs=ops.COCO_IOU_THRS, max_dets=ops.COCO_MAX_DETS) -> str:
    """The 12 lines COCOeval.summarize prints."""
    i_str = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    rows = [(1, None, "all", 2), (1, .5, "all", 2), (1, .75, "all", 2), (1, None, "small", 2), (1, None, "medium", 2), (1, None, "large", 2),
            (0, None, "all", 0), (0, None, "all", 1), (0, None, "all", 2), (0, None, "small", 2), (0, None, "medium", 2), (0, None, "large", 2)]
    out = []
    for v, (ap, thr, area, mi) in zip(stats, rows):
        iou = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1]) if thr is None else "{:0.2f}".format(thr)
        out.append(i_str.format("Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, max_dets[mi], v))
    return "\n".join(out)


class COCOEvaluator:
    """Accumulates detections on the device and computes COCOeval's precision / recall in one library call.

    add() takes FCOSHead.detect_padded + ClipBoxes + ops.boxes_rescale_xywh_ output (labels already mapped to this evaluator's
    contiguous labels, see CocoGT.label_of) and only enqueues device copies; batches may differ in K.  compute() orders the images
    it was given by id, runs fd_eval_coco once and copies the result to the host."""

    def __init__(self, gt, device=None):
        self.gt = load_coco_gt(gt)
        self.device = torch.device(device) if device is not None else None
        self._n = 0
        self._ids = []          # image id of each added row
        self._seen = set()
        self._bufs = None       # scores [cap, K] f32, labels [cap, K] int64 (0 = not taking part), boxes [cap, K, 4] f32 xywh
        self._gt_dev = None
        self.result = None

    def reset(self) -> None:
        """Forget every image added; the device buffers are kept (add() overwrites the rows it appends in full)."""
        self._n = 0
        self._ids = []
        self._seen = set()
        self.result = None

    @property
    def num_images(self) -> int:
        return self._n

    def _alloc(self, cap: int, K: int, dev):
        return (torch.zeros(cap, K, dtype=torch.float32, device=dev), torch.zeros(cap, K, dtype=torch.int64, device=dev),
                torch.zeros(cap, K, 4, dtype=torch.float32, device=dev))

    def _reserve(self, n: int, K: int, dev) -> None:
        if self._bufs is None:
            self._bufs = self._alloc(max(n, 64), K, dev)
            return
        s, c, b = self._bufs
        cap, K0 = s.shape
        if n <= cap and K <= K0:
            return
        new = self._alloc(max(n, 2 * cap) if n > cap else cap, max(K, K0), dev)
        m = self._n
        new[0][:m, :K0] = s[:m]
        new[1][:m, :K0] = c[:m]
        new[2][:m, :K0] = b[:m]
        self._bufs = new

    def add(self, image_ids: Sequence[int], scores: torch.Tensor, labels: torch.Tensor, boxes_xywh: torch.Tensor,
            counts: Optional[torch.Tensor]) -> None:
        """image_ids: B host ints (COCO image ids); scores [B,K] f32, labels [B,K] (1 .. num_cats), boxes_xywh [B,K,4] f32, counts [B]
        (rows >= counts[b] take no part; None = all rows).  Device tensors; no host synchronisation."""
        ops._need_gpu(scores, labels, boxes_xywh, counts)
        B, K = scores.shape
        ids = [int(i) for i in image_ids]
        if len(ids) != B or tuple(labels.shape) != (B, K) or tuple(boxes_xywh.shape) != (B, K, 4):
            raise FdError("COCOEvaluator.add: shapes do not agree")
        if K > MAX_DETECTIONS:
            raise FdError(f"COCOEvaluator.add: at most {MAX_DETECTIONS} detections per image (got K={K})")
        for i in ids:
            if i not in self.gt.index:
                raise FdError(f"COCOEvaluator.add: image id {i} is not in the GT")
            if i in self._seen:
                raise FdError(f"COCOEvaluator.add: image id {i} added twice")
        if len(set(ids)) != len(ids):
            raise FdError("COCOEvaluator.add: duplicate image ids in one batch")
        dev = scores.device
        if self.device is None:
            self.device = dev
        n = self._n
        self._reserve(n + B, K, dev)
        s, c, b = self._bufs
        lab = labels.to(torch.int64)
        if counts is not None:
            lab = torch.where(torch.arange(K, device=dev)[None, :] < counts.to(dev)[:, None].to(torch.int64), lab, torch.zeros_like(lab))
        s[n:n + B, :K] = scores
        c[n:n + B, :K] = lab
        c[n:n + B, K:] = 0       # columns an earlier, wider batch wrote before a reset()
        b[n:n + B, :K] = boxes_xywh
        self._ids.extend(ids)
        self._seen.update(ids)
        self._n = n + B

    def gather(self, group=None, force: bool = False) -> "COCOEvaluator":
        """The union of every rank's evaluator, as a new evaluator on this rank's device; every rank must call it, and every
        rank gets the same rows: each distinct image id once (of an id two ranks hold, the lowest rank's row), ids ascending.
        Only detections and ids travel -- every rank holds the GT already (two collectives, dist.gather_rows); ranks whose GT
        differ in their categories or images raise FdError, all of them.  No process group, or world size 1 without
        `force`: returns self."""
        if _dist._no_group(group, force):
            return self
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n = self._n
        bufs = self._bufs if self._bufs is not None else self._alloc(0, 0, dev)
        ids = torch.tensor(self._ids, dtype=torch.int64).to(dev)
        header = (self.gt.num_cats, len(self.gt.image_ids),
                  zlib.crc32(np.ascontiguousarray(self.gt.category_ids, np.int64).tobytes() + np.ascontiguousarray(self.gt.image_ids, np.int64).tobytes()))
        got, _, _ = _dist._gather_rows(list(bufs) + [ids], n, group, None, header)
        out = COCOEvaluator(self.gt, device=dev)
        out._gt_dev = self._gt_dev
        all_ids = got.pop().cpu()
        order = _dist.merge_order(all_ids)
        if order.numel():
            out._ids = all_ids[order].tolist()
            out._seen = set(out._ids)
            out._bufs = tuple(t.index_select(0, order.to(dev)) for t in got)
            out._n = order.numel()
        return out

    def _gt_on(self, dev):
        if self._gt_dev is None or self._gt_dev[0].device != dev:
            g = self.gt
            self._gt_dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g.boxes, g.area, g.crowd, g.labels))
        return self._gt_dev

    def compute(self) -> Dict[str, np.ndarray]:
        """-> {"precision" [10,101,C,4,3], "recall" [10,C,4,3] f64, "stats" [12], "category_ids" [C], "image_ids" (sorted), "n_gt" [C,4]}."""
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if self._n == 0:        # nothing added: one image position without detections or GT
            self._reserve(1, 1, dev)
            self._bufs[1][0] = 0
            n, gidx, order = 1, None, None
        else:
            n = self._n
            gidx = torch.tensor([self.gt.index[i] for i in self._ids], dtype=torch.int64, device=dev)
            order = torch.from_numpy(np.argsort(np.array(self._ids, np.int64), kind="stable").astype(np.int32)).to(dev)
        gb, ga, gc, gl = self._gt_on(dev)
        if gidx is None:
            gb, ga, gc = gb[:1], ga[:1], gc[:1]
            gl = torch.full_like(gl[:1], -1)
        else:
            gb, ga, gc, gl = (t.index_select(0, gidx) for t in (gb, ga, gc, gl))
        s, c, b = self._bufs
        prec, rec, n_gt = ops.eval_coco(s[:n], c[:n], b[:n], None, gb.contiguous(), ga.contiguous(), gc.contiguous(), gl.contiguous(),
                                        self.gt.num_cats, order)
        precision, recall, n_gt = prec.cpu().numpy(), rec.cpu().numpy(), n_gt.cpu().numpy()
        self.result = {"precision": precision, "recall": recall, "stats": coco_stats(precision, recall),
                       "category_ids": self.gt.category_ids.copy(), "image_ids": np.sort(np.array(self._ids, np.int64)), "n_gt": n_gt}
        return self.result

    def summarize(self) -> np.ndarray:
        """Prints COCOeval.summarize's 12 lines (computing first if needed); -> stats."""
        if self.result is None:
            self.compute()
        print(format_stats(self.result["stats"]))
        return self.result["stats"]


def evaluate_coco(generator, model, threshold=0.05, gather=False):
    """The reference's evaluate_coco (Test_coco.py:120-190): per image FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64]) -> ClipBoxes ->
    boxes / scale -> xywh, detections from the first with score < threshold on dropped, labels mapped through
    generator.id2category; then COCOeval against generator.coco (crowd annotations included) over the processed images, and the
    summary printed.  The generator is duck-typed: len, [index] -> (img, boxes, classes, scale), .ids, .id2category, .coco.
    Detections stay on the device (COCOEvaluator).  Difference: no coco_bbox_results.json is written.
    gather=False: this process runs every image of the generator, computes and prints.  gather=True: EVERY rank must call; rank
    r of W runs the generator's indices r, r + W, r + 2W, ..., the evaluators are merged (COCOEvaluator.gather: two collectives),
    every rank computes the same stats and rank 0 prints them; whether there is a detection at all is read off the merged rows
    (a detection whose category the GT does not list takes no part there, as in the evaluation itself).  Without a process
    group gather=True runs every image here.  -> stats (12 numbers), or None when there is no detection at all."""
    grouped = gather and torch.distributed.is_available() and torch.distributed.is_initialized()
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if grouped else (0, 1)
    head = FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64])
    clip = ClipBoxes()
    ev = COCOEvaluator(generator.coco)
    dev = torch.device("cuda", torch.cuda.current_device())
    ids = sorted(generator.id2category)
    lut = torch.zeros(max(ids) + 1 if ids else 1, dtype=torch.int64)
    for lab in ids:
        lut[lab] = ev.gt.label_of(int(generator.id2category[lab]))
    lut = lut.to(dev)
    any_det = torch.zeros((), dtype=torch.int64, device=dev)
    with torch.no_grad():
        for index in range(rank, len(generator), world):
            img, _, _, scale = generator[index]
            x = (img if torch.is_tensor(img) else torch.from_numpy(np.asarray(img))).unsqueeze(dim=0).to(dev)
            out = model(x)
            scores, labels, boxes, counts = head.detect_padded(out)
            boxes = clip(x, boxes.contiguous())
            ops.boxes_rescale_xywh_(boxes, float(scale))
            K = scores.shape[1]
            pos = torch.arange(K, device=dev)
            # "scores are sorted, so we can break": rows from the first score below the threshold on take no part
            first_low = torch.where(scores < threshold, pos[None, :], torch.full_like(pos[None, :], K)).min(dim=1).values
            n = torch.minimum(counts.to(torch.int64), first_low)
            lab = lut[labels.clamp(0, lut.shape[0] - 1)] * (labels < lut.shape[0]).to(torch.int64)
            any_det += n.sum()
            ev.add([generator.ids[index]], scores.float().contiguous(), lab, boxes.float().contiguous(), n.to(torch.int32))
    if gather:
        ev = ev.gather()
        if ev.num_images == 0 or not bool((ev._bufs[1][:ev.num_images] != 0).any()):
            return None
    elif int(any_det) == 0:
        return None
    stats = ev.compute()["stats"]
    if rank == 0:
        print(format_stats(stats))
    return stats
