"""Config loader, location grid and DataEncoder with the reference's names (utill/utills.py:58-73, 100-255, 258-272)."""
from __future__ import annotations

import math
import os
from typing import List

import torch
from yaml import safe_load

from .._lib import FdError

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coords_origin_fcos(feature: torch.Tensor, strides: int) -> torch.Tensor:
    """[H*W, 2] fp32 (x*s + s//2, y*s + s//2), x fastest, for an NHWC-shaped `feature` ([N, H, W, C]).
    The HIP decode kernel derives the same grid in-kernel; this helper exists for callers of the reference API."""
    h, w = feature.shape[1:3]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=feature.device) * strides,
                            torch.arange(w, dtype=torch.float32, device=feature.device) * strides, indexing='ij')
    return torch.stack([xs.reshape(-1), ys.reshape(-1)], -1) + strides // 2


def resize_rule(h: int, w: int, resize_size=(800, 1333)):
    """(scale, nh, nw) of the reference's preprocess_img_boxes (dataset/voc.py:117-125, Test_coco.py:83-91) for a raw
    h x w image: the short side is scaled to min_side, the long side capped at max_side, the sizes truncated.  Python
    doubles in the reference's order of operations -- the truncation depends on it (289 x 333 -> 799 x 921, not 800)."""
    min_side, max_side = resize_size
    smallest_side = min(w, h)
    largest_side = max(w, h)
    scale = min_side / smallest_side
    if largest_side * scale > max_side:
        scale = max_side / largest_side
    return scale, int(scale * h), int(scale * w)


def pad32(n: int) -> int:
    """Padded side of dataset/voc.py:128-131: n + 32 - n % 32 (a full extra 32 when n is already a multiple of 32)."""
    return n + 32 - n % 32


def load_config(cfg: str = os.path.join(_PKG, 'config', 'main.yaml')) -> dict:
    """main.yaml names the dataset + model; the dataset yaml holds one block per model.  Result keys as in the
    reference: dataset_setting, <MODEL> blocks, model{dataset,name,amp,ddp,persistent,prefetch}, savename.
    Dataset yaml paths are resolved relative to main.yaml's directory's parent when not found as given."""
    with open(cfg) as f:
        main = safe_load(f)
    dataset = main['dataset']
    path = main[dataset]
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(cfg))), path)
    with open(path) as f:
        config = safe_load(f)
    config['model'] = {'dataset': dataset, 'name': main['model'], 'amp': main['amp'], 'ddp': main['ddp_enabled'],
                       'persistent': main['persistent_workers'], 'prefetch': main['prefetch_factor']}
    config['savename'] = main['savename']
    return config


class DataEncoder:
    """The reference's DataEncoder (utill/utills.py:100-255) on the GPU: anchors, encode (ground truth -> per-anchor regression and
    class targets), decode (per-anchor predictions -> boxes and labels after NMS), _box_iou and _box_nms, each one HIP launch chain
    (fd_anchor_boxes / fd_anchor_encode / fd_anchor_decode, fd_pairwise_iou, fd_box_nms_plus1).  Tensors are CUDA fp32
    (boxes, predictions) and int64 (labels); anything else raises FdError -- there is no CPU path.  encode_batch / decode_batch take
    a whole padded batch in one call.  The RetinaNet model that would use this class is not built: its reference cannot be
    constructed.

    Two upstream defects are repaired: decode with exactly one candidate returns that box (the reference raises IndexError on a
    0-d index), and encode of an image without boxes returns cls = 0, loc = 0 (the reference raises)."""

    def __init__(self):
        self.anchor_areas = [32 * 32., 64 * 64., 128 * 128., 256 * 256., 512 * 512.]      # p3 .. p7
        self.aspect_ratios = [1 / 2., 1 / 1., 2 / 1.]                                      # w / h
        self.scale_ratios = [1., pow(2, 1 / 3.), pow(2, 2 / 3.)]
        self.anchor_wh = self._get_anchor_wh()
        self._params = {}

    def _get_anchor_wh(self) -> torch.Tensor:
        """[5, 9, 2] fp32 (w, h) on the host: per area and aspect ratio h = sqrt(area / ratio), w = ratio * h, each times the three
        scales -- in doubles, rounded once to fp32."""
        rows = []
        for area in self.anchor_areas:
            for ratio in self.aspect_ratios:
                h = math.sqrt(area / ratio)
                w = ratio * h
                rows.extend([w * scale, h * scale] for scale in self.scale_ratios)
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32).view(len(self.anchor_areas), -1, 2)

    def _anchor_params(self, input_size):
        """The fd_anchor_params of `input_size` (an int, (w, h) or a 2-element tensor), cached per size."""
        from .. import ops
        if isinstance(input_size, torch.Tensor):
            input_size = tuple(float(v) for v in input_size.tolist())
        key = (input_size, input_size) if isinstance(input_size, (int, float)) else tuple(input_size)
        p = self._params.get(key)
        if p is None:
            p = self._params[key] = ops.anchor_params(key, self.anchor_wh)
        return p

    def _get_anchor_boxes(self, input_size, device=None) -> torch.Tensor:
        """[A, 4] fp32 (cx, cy, w, h) on the GPU, rows ordered level, y, x, anchor; A = 9 * sum fm_w * fm_h with
        fm = ceil(input_size / 2^(level + 3)), centres (index + 0.5) * (input_size / fm)."""
        from .. import ops
        return ops.anchor_boxes(self._anchor_params(input_size), torch.device("cuda") if device is None else device)

    def _meshgrid(self, x: int, y: int, row_major: bool = True) -> torch.Tensor:
        """[x * y, 2] int64 cell indices, x fastest: (x, y) pairs when row_major, else (y, x)."""
        yy, xx = torch.meshgrid(torch.arange(y), torch.arange(x), indexing='ij')
        cols = [xx.reshape(-1), yy.reshape(-1)]
        return torch.stack(cols if row_major else cols[::-1], 1)

    def _change_box_order(self, boxes, order: str) -> torch.Tensor:
        """'xyxy2xywh': (x1, y1, x2, y2) -> (centre, b - a + 1); 'xywh2xyxy': (cx, cy, w, h) -> (c - wh / 2, c + wh / 2).  fp32, on the
        device of `boxes`."""
        assert order in ['xyxy2xywh', 'xywh2xyxy']
        boxes = torch.as_tensor(boxes, dtype=torch.float32)
        a, b = boxes[:, :2], boxes[:, 2:]
        if order == 'xyxy2xywh':
            return torch.cat([(a + b) / 2, b - a + 1], 1)
        return torch.cat([a - b / 2, a + b / 2], 1)

    def encode_batch(self, gt_boxes: torch.Tensor, labels: torch.Tensor, input_size):
        """gt_boxes [B, M, 4] xyxy fp32, labels [B, M] int64 (a row with label < 0 is padding, M <= 256) -> (loc [B, A, 4] fp32,
        cls [B, A] int64), one launch.  Per anchor: the image's box of largest IoU ('+1' convention on boxes grown by half a
        pixel, first box on ties); loc = ((gt_xy - a_xy) / a_wh, log(gt_wh / a_wh)); cls = 1 + label, 0 where that IoU < 0.5,
        -1 (ignored) where it is in (0.4, 0.5).  An image without a valid box: cls = 0, loc = 0."""
        from .. import ops
        return ops.anchor_encode(self._anchor_params(input_size), gt_boxes, labels)

    def encode(self, boxes: torch.Tensor, labels: torch.Tensor, input_size):
        """boxes [M, 4] xyxy, labels [M] -> (loc_targets [A, 4], cls_targets [A]); encode_batch on one image.  M = 0 returns
        cls = 0, loc = 0 (the reference raises)."""
        if not isinstance(boxes, torch.Tensor) or not isinstance(labels, torch.Tensor) or boxes.dim() != 2 or labels.dim() != 1:
            raise FdError("DataEncoder.encode: boxes [M, 4] and labels [M] must be tensors")
        loc, cls = self.encode_batch(boxes[None], labels[None], input_size)
        return loc[0], cls[0]

    def decode_batch(self, loc_preds: torch.Tensor, cls_preds: torch.Tensor, input_size, cls_thresh: float = 0.5, nms_thresh: float = 0.5,
                     max_candidates: int = 1000):
        """loc_preds [B, A, 4], cls_preds [B, A, C] logits (C <= 128) -> (boxes [B, K, 4] xyxy, labels [B, K] int64 0-based with -1
        in the padding, scores [B, K], counts [B] int32, n_candidates [B] int32), K = min(max_candidates, A), rows score-descending,
        no host synchronisation.  Per anchor: box = (loc_xy * a_wh + a_xy) -/+ exp(loc_wh) * a_wh / 2; score, label = first maximum
        over the fp32 sigmoid values; candidates are score > cls_thresh; greedy '+1' NMS keeps while IoU <= nms_thresh.  Where more
        than max_candidates (<= 1024) anchors pass the threshold the best max_candidates by score go on, and n_candidates -- the
        number that passed -- shows it; within the cap the result is the reference's."""
        from .. import ops
        return ops.anchor_decode(self._anchor_params(input_size), loc_preds, cls_preds, cls_thresh, nms_thresh, max_candidates)

    def decode(self, loc_preds: torch.Tensor, cls_preds: torch.Tensor, input_size):
        """loc_preds [A, 4], cls_preds [A, C] -> (boxes [n, 4], labels [n]) after NMS, thresholds 0.5 / 0.5 as in the reference;
        decode_batch on one image with the default cap of 1000 candidates.  A single candidate is returned (the reference raises
        IndexError there); none gives empty tensors."""
        if not isinstance(loc_preds, torch.Tensor) or not isinstance(cls_preds, torch.Tensor) or loc_preds.dim() != 2 or cls_preds.dim() != 2:
            raise FdError("DataEncoder.decode: loc_preds [A, 4] and cls_preds [A, C] must be tensors")
        boxes, labels, _, counts, _ = self.decode_batch(loc_preds[None], cls_preds[None], input_size)
        n = int(counts[0])
        return boxes[0, :n], labels[0, :n]

    def _box_iou(self, box1: torch.Tensor, box2: torch.Tensor, order: str = 'xyxy') -> torch.Tensor:
        """[N,4] x [M,4] -> [N,M] IoU with the '+1' pixel convention."""
        from .. import ops
        if order == 'xywh':          # utills.py:196-199 _change_box_order('xywh2xyxy'): (cx, cy, w, h) -> (c - wh/2, c + wh/2)
            box1 = torch.cat([box1[:, :2] - box1[:, 2:] / 2, box1[:, :2] + box1[:, 2:] / 2], 1)
            box2 = torch.cat([box2[:, :2] - box2[:, 2:] / 2, box2[:, :2] + box2[:, 2:] / 2], 1)
        elif order != 'xyxy':
            raise ValueError(f"unknown box order '{order}'")
        return ops.pairwise_iou(box1.contiguous().float(), box2.contiguous().float(), True)

    def _box_nms(self, bboxes: torch.Tensor, scores: torch.Tensor, threshold: float = 0.5, mode: str = 'union') -> torch.Tensor:
        """Greedy class-agnostic NMS, '+1' areas, keep while ovr <= threshold; returns kept indices (int64, score-descending)."""
        from .. import ops
        if mode not in ('union', 'min'):
            raise TypeError('Unknown nms mode: %s.' % mode)
        keep, counts = ops.box_nms_plus1(bboxes.contiguous().float()[None], scores.contiguous().float()[None], threshold, mode)
        return keep[0, :int(counts[0])].to(torch.int64)
