"""The reference's training augmentations with the pixel work on the device.

Per image the reference does, on the host (dataset/voc.py:97-103, data/augment.py): flip (p 0.5), Transforms = colorJitter
(p 0.3), random_rotation (p 0.5, |d| <= 10), random_crop_resize (p 0.5, up to 10 attempts), then preprocess_img_boxes and
collate_fn.  Here the host only draws the random decisions and moves the (tiny) boxes -- `sample_params`, the reference's
box arithmetic in its number types and order -- and the device does every pixel step of the whole batch in one fused
launch (ops.augment_resize_collate_u8): `collate_train_raw` is raw uint8 images + boxes in, collate_fn's triple out.

Mosaic (this project's definition): `collate_train_mosaic` tiles four such augmented images around a random centre
per output -- `sample_mosaic` draws and moves the boxes, ops.mosaic_collate_u8 is the one device launch for the pixels.
"""
from __future__ import annotations

import math
import random as _random
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from .._lib import FdError
from ..utill.utills import pad32, resize_rule

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # dataset/voc.py:57-58
JITTER_P, ROTATE_P, CROP_P = 0.3, 0.5, 0.5                         # data/augment.py:13-18
ROTATE_DEGREE = 10
JITTER_RANGE, HUE_RANGE = 0.1, 0.1                                 # colorJitter's brightness = contrast = saturation = hue = 0.1
CROP_SCALE_MIN, CROP_ASPECT, CROP_REMAIN_MIN, CROP_ATTEMPTS = 0.2, (3. / 4, 4. / 3), 0.7, 10


@dataclass
class AugmentParams:
    """What was drawn for one image.  chain: ((ops.AUG_OP_*, factor or uint8 hue shift), ...) in application order, empty when
    the jitter was not drawn; d: rotation in degrees, 0.0 when not drawn; crop: (x, y, cw, ch) in the (rotated) image or None;
    out_hw: the image size after the crop."""
    flip: bool
    chain: Tuple[Tuple[int, float], ...]
    d: float
    crop: Optional[Tuple[int, int, int, int]]
    out_hw: Tuple[int, int]

    def record_kwargs(self) -> dict:
        return dict(flip=self.flip, chain=self.chain, d=self.d, crop=self.crop)


def _flip_boxes(w: int, boxes: np.ndarray) -> np.ndarray:
    # dataset/voc.py:14-19: numpy fp32, int - fp32
    if boxes.shape[0] != 0:
        xmin = w - boxes[:, 2]
        xmax = w - boxes[:, 0]
        boxes[:, 2] = xmax
        boxes[:, 0] = xmin
    return boxes


def _rotate_boxes(d: float, h: int, w: int, boxes: np.ndarray) -> np.ndarray:
    # data/augment.py:26-59: every box -> hull of its four rotated corners, clamped; torch fp32 tensors with Python-double
    # cos / sin / centre scalars, one fp32 rounding per operation, in the reference's order of operations
    rx0, ry0 = w / 2.0, h / 2.0
    a = -d / 180.0 * math.pi
    b = torch.from_numpy(boxes)
    xmin, ymin, xmax, ymax = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    zx = torch.stack([xmin, xmin, xmax, xmax], 1)         # corners (x0, y0) (x1, y1) (x2, y2) (x3, y3) of the reference
    zy = torch.stack([ymin, ymax, ymin, ymax], 1)
    tx = (zx - rx0) * math.cos(a) - (zy - ry0) * math.sin(a) + rx0
    ty = (zx - rx0) * math.sin(a) + (zy - ry0) * math.cos(a) + ry0
    out = torch.stack([tx.min(1)[0].clamp(min=0, max=w - 1), ty.min(1)[0].clamp(min=0, max=h - 1),
                       tx.max(1)[0].clamp(min=0, max=w - 1), ty.max(1)[0].clamp(min=0, max=h - 1)], 1)
    return out.numpy()


def _crop_ok(x: int, y: int, w: int, h: int, boxes: torch.Tensor) -> bool:
    # data/augment.py:85-98: every box the crop touches (intersection > 0.0001) must keep more than 0.7 of its area
    crop = torch.tensor([[x, y, x + w, y + h]], dtype=torch.float32)
    tl = torch.max(crop[:, None, :2], boxes[:, :2])
    br = torch.min(crop[:, None, 2:], boxes[:, 2:])
    hw = (br - tl).clamp(min=0)
    inter = hw[:, :, 0] * hw[:, :, 1]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    mask = inter > 0.0001
    remain = inter[mask].view(-1) / area[mask.view(-1)]
    return remain.shape[0] == 0 or bool(torch.min(remain > CROP_REMAIN_MIN))


def sample_params(h: int, w: int, boxes, rng=None, flip_p: float = 0.5, augment: bool = True):
    """Draw one image's augmentation and move its boxes: (AugmentParams, boxes_out fp32 [n, 4]).

    `rng` (a random.Random; None: the `random` module's global stream, the one the reference consumes) is consumed in the
    reference's order of draws: flip; jitter decision; rotation decision and uniform(-10, 10); crop decision and, per attempt,
    uniform, uniform, random, then randint, randint when the size fits.  With the same seed the geometric decisions, `d` and
    the crop rectangle are the reference's, and the boxes are its boxes bit for bit (flip in numpy fp32, rotation and crop in
    torch fp32).  flip_p <= 0 draws nothing for the flip; augment=False draws nothing for Transforms.

    THE JITTER SAMPLING IS THIS PROJECT'S DEFINITION: the reference delegates it to torchvision's ColorJitter, which is absent
    and draws from torch's generator.  When the jitter decision falls, the chain is drawn from the same rng AFTER the geometric
    draws of the image (so the geometric stream stays the reference's): a permutation rng.sample(range(4), 4) of (brightness,
    contrast, saturation, hue), then the factors uniform(0.9, 1.1) x 3 and the hue uniform(-0.1, 0.1), in that fixed order."""
    rng = _random if rng is None else rng
    h, w = int(h), int(w)
    boxes = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    flip = False
    if flip_p > 0 and rng.random() < flip_p:
        flip = True
        boxes = _flip_boxes(w, boxes)
    jitter, d, crop = False, 0.0, None
    if augment:
        jitter = rng.random() < JITTER_P
        if rng.random() < ROTATE_P:
            d = rng.uniform(-ROTATE_DEGREE, ROTATE_DEGREE)
            boxes = _rotate_boxes(d, h, w, boxes)
        if rng.random() < CROP_P:
            tb = torch.from_numpy(boxes)
            for _ in range(CROP_ATTEMPTS):
                area = w * h
                target_area = rng.uniform(CROP_SCALE_MIN, 1.0) * area
                ratio = rng.uniform(CROP_ASPECT[0], CROP_ASPECT[1])
                cw = int(round(math.sqrt(target_area * ratio)))
                ch = int(round(math.sqrt(target_area / ratio)))
                if rng.random() < 0.5:
                    cw, ch = ch, cw
                if cw <= w and ch <= h:
                    x = rng.randint(0, w - cw)
                    y = rng.randint(0, h - ch)
                    if _crop_ok(x, y, cw, ch, tb):
                        crop = (x, y, cw, ch)
                        break
            if crop is not None:
                x, y, cw, ch = crop
                tb = tb - torch.Tensor([x, y, x, y])
                tb[:, 1::2].clamp_(min=0, max=ch - 1)
                tb[:, 0::2].clamp_(min=0, max=cw - 1)
                boxes = tb.numpy()
    chain = ()
    if jitter:
        order = rng.sample(range(4), 4)
        fb, fc, fs = (rng.uniform(1 - JITTER_RANGE, 1 + JITTER_RANGE) for _ in range(3))
        hue = rng.uniform(-HUE_RANGE, HUE_RANGE)
        entries = [(ops.AUG_OP_BRIGHTNESS, fb), (ops.AUG_OP_CONTRAST, fc), (ops.AUG_OP_SATURATION, fs), (ops.AUG_OP_HUE, ops.hue_shift(hue))]
        chain = tuple(entries[k] for k in order)
    out_hw = (h, w) if crop is None else (crop[3], crop[2])
    return AugmentParams(flip, chain, float(d), crop, out_hw), np.ascontiguousarray(boxes, dtype=np.float32)


def collate_train_raw(images: Sequence[torch.Tensor], boxes_list, classes_list, resize_size=(800, 1333), rng=None, augment: bool = True,
                      flip_p: float = 0.5, mean=MEAN, std=STD, return_params: bool = False):
    """A training batch from RAW images: decoded uint8 [h_n, w_n, 3] CUDA images, their boxes (fp32 [k_n, 4], x1 y1 x2 y2, host)
    and classes (int [k_n], host) -> (batch_imgs [B, 3, H, W] fp32 CUDA, batch_boxes [B, M, 4] fp32 CUDA, batch_classes [B, M]
    int64 CUDA), the triple of the reference's collate_fn (dataset/voc.py:141-173).

    Per image: sample_params (flip, Transforms), the size rule of preprocess_img_boxes on the CROPPED size
    (utill.utills.resize_rule), boxes * scale in numpy fp32 (voc.py:137-138); then pad32 and the batch maximum for the canvas,
    the fused device launch for all pixels, boxes / classes padded with -1.  Two small uploads (records + pointers; boxes +
    classes), no synchronisation.  rng=None, augment=False, flip_p=0 is the plain training collate.  return_params=True appends
    the list of AugmentParams."""
    images = list(images)
    B = len(images)
    if B < 1 or len(boxes_list) != B or len(classes_list) != B:
        raise FdError("collate_train_raw: images, boxes_list and classes_list must be non-empty and of one length")
    for t in images:
        ops._check_raw_image(t, "collate_train_raw")
    params, kwargs, out_boxes, out_classes = [], [], [], []
    for t, bx, cl in zip(images, boxes_list, classes_list):
        p, b = sample_params(int(t.shape[0]), int(t.shape[1]), bx.cpu().numpy() if isinstance(bx, torch.Tensor) else bx, rng, flip_p, augment)
        c = np.asarray(cl.cpu().numpy() if isinstance(cl, torch.Tensor) else cl, dtype=np.int64).reshape(-1)
        if c.shape[0] != b.shape[0]:
            raise FdError(f"collate_train_raw: {b.shape[0]} boxes but {c.shape[0]} classes")
        scale, nh, nw = resize_rule(p.out_hw[0], p.out_hw[1], resize_size)
        if nh < 1 or nw < 1:
            raise FdError(f"collate_train_raw: a {p.out_hw[0]} x {p.out_hw[1]} image resizes to nothing under {tuple(resize_size)}")
        b[:, [0, 2]] = b[:, [0, 2]] * scale
        b[:, [1, 3]] = b[:, [1, 3]] * scale
        params.append(p)
        kwargs.append(dict(p.record_kwargs(), nh=nh, nw=nw))
        out_boxes.append(b)
        out_classes.append(c)
    H = max(pad32(k["nh"]) for k in kwargs)
    W = max(pad32(k["nw"]) for k in kwargs)
    batch_imgs, _ = ops.augment_resize_collate_u8(images, kwargs, H, W, mean, std)
    M = max(b.shape[0] for b in out_boxes)
    # one upload: B*M*4 fp32 box words, then B*M int64 classes as int32 pairs (the box part is a multiple of 16 bytes)
    pack = np.empty(B * M * 6, np.int32)
    pb = pack[:B * M * 4].view(np.float32).reshape(B, M, 4)
    pc = pack[B * M * 4:].view(np.int64).reshape(B, M)
    pb[...] = -1
    pc[...] = -1
    for i, (b, c) in enumerate(zip(out_boxes, out_classes)):
        pb[i, :b.shape[0]] = b
        pc[i, :c.shape[0]] = c
    if M == 0:              # no ground truth in the whole batch: nothing to upload
        batch_boxes = torch.empty(B, 0, 4, dtype=torch.float32, device=images[0].device)
        batch_classes = torch.empty(B, 0, dtype=torch.int64, device=images[0].device)
    else:
        dev_pack = torch.from_numpy(pack).to(images[0].device, non_blocking=True)
        batch_boxes = dev_pack[:B * M * 4].view(torch.float32).view(B, M, 4)
        batch_classes = dev_pack[B * M * 4:].view(torch.int64).view(B, M)
    if return_params:
        return batch_imgs, batch_boxes, batch_classes, params
    return batch_imgs, batch_boxes, batch_classes


# ---------------------------------------------------------------------------------------------- mosaic
@dataclass
class MosaicParams:
    """What was drawn for one mosaic output.  centre: (xc, yc); sources: index into the batch's images per tile (0 top-left,
    1 top-right, 2 bottom-left, 3 bottom-right); tiles: the four AugmentParams; gains: the four g; scales / sizes: the factor the
    boxes were multiplied by and the tile's (nh, nw); placements: the four (px, py)."""
    centre: Tuple[int, int]
    sources: Tuple[int, int, int, int]
    tiles: Tuple[AugmentParams, ...]
    gains: Tuple[float, ...]
    scales: Tuple[float, ...]
    sizes: Tuple[Tuple[int, int], ...]
    placements: Tuple[Tuple[int, int], ...]


def mosaic_tile_boxes(b, scale: float, px: int, py: int, nh: int, nw: int, t: int, xc: int, yc: int, H: int, W: int, min_side: float = 2.0,
                      min_visible: float = 0.2):
    """Steps 1 - 5 of sample_mosaic's box rule for tile t (an nh x nw image at canvas (py, px), any placement) of a mosaic with
    centre (xc, yc) on an H x W canvas: (kept clipped boxes fp32 [k, 4], their indices in b).  numpy fp32, one rounding per
    operation."""
    F = np.float32
    b = np.array(b, dtype=np.float32).reshape(-1, 4)
    none = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    qx0, qx1 = (xc, W) if t & 1 else (0, xc)
    qy0, qy1 = (yc, H) if t & 2 else (0, yc)
    vx0, vx1, vy0, vy1 = max(qx0, px), min(qx1, px + nw), max(qy0, py), min(qy1, py + nh)
    if vx1 <= vx0 or vy1 <= vy0 or b.shape[0] == 0:
        return none
    b = b * F(scale)
    b[:, [0, 2]] = b[:, [0, 2]] + F(px)
    b[:, [1, 3]] = b[:, [1, 3]] + F(py)
    ow, oh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    c = b.copy()
    c[:, [0, 2]] = np.clip(b[:, [0, 2]], F(vx0), F(vx1 - 1))
    c[:, [1, 3]] = np.clip(b[:, [1, 3]], F(vy0), F(vy1 - 1))
    cw, ch = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    keep = (ow > 0) & (oh > 0) & (cw >= F(min_side)) & (ch >= F(min_side)) & (cw * ch >= F(min_visible) * (ow * oh))
    idx = np.nonzero(keep)[0]
    return np.ascontiguousarray(c[idx]), idx


def sample_mosaic(sizes, boxes_list, n: int, out_hw, rng=None, flip_p: float = 0.5, augment: bool = True, scale_range=(0.5, 1.0),
                  centre_range=(0.25, 0.75), min_side: float = 2.0, min_visible: float = 0.2, group=None):
    """Draw mosaic output n of a batch whose images have `sizes` [(h, w)] and boxes `boxes_list`, on an out_hw = (H, W) canvas:
    (MosaicParams, boxes fp32 [k, 4], origin int64 [k, 2] = (source image, box index in that image) of every kept box).

    THIS IS THIS PROJECT'S DEFINITION (the reference has no mosaic).  Draws from `rng` (a random.Random; None: the `random`
    module's global stream) in this fixed order:
      1. group=None: three rng.randrange(B) partners, then q = rng.randrange(4); image n takes quadrant q, the partners fill the
         other quadrants in ascending order.  group = four source indices in tile order: nothing is drawn here.
      2. xc = rng.randint(int(W * lo), int(W * hi)), then yc = rng.randint(int(H * lo), int(H * hi)), (lo, hi) = centre_range.
      3. for t = 0 .. 3: sample_params(h, w, boxes, rng, flip_p, augment) of tile t's source (the reference's per-image transforms
         and box arithmetic, unchanged), then g = rng.uniform(*scale_range).
    Tile size: L = max(1, int(round(g * max(H, W)))); (scale, nh, nw) = resize_rule(out_h, out_w, (L, L)) on the cropped size --
    the long side goes to L -- with nh, nw clamped to >= 1.  Placement: the tile's corner touches the centre: (px, py) =
    (xc - nw, yc - nh), (xc, yc - nh), (xc - nw, yc), (xc, yc) for t = 0, 1, 2, 3.

    Boxes, all in numpy fp32 with one rounding per operation:
      1. b * np.float32(scale), as collate_train_raw does;  2. + px on x, + py on y;
      3. the visible rectangle [vx0, vx1) x [vy0, vy1) is the tile's quadrant ([0, xc) or [xc, W) by [0, yc) or [yc, H)) intersected
         with [px, px + nw) x [py, py + nh); empty: the tile contributes no boxes;
      4. clip x to [vx0, vx1 - 1] and y to [vy0, vy1 - 1];
      5. keep a box when its width and height after step 2 are > 0, its clipped width and clipped height are >= min_side, and
         clipped width * clipped height >= np.float32(min_visible) * (width * height after step 2);
      6. output order: tile 0 .. 3, source order within a tile."""
    rng = _random if rng is None else rng
    B = len(sizes)
    H, W = int(out_hw[0]), int(out_hw[1])
    if group is None:
        partners = [rng.randrange(B) for _ in range(3)]
        q = rng.randrange(4)
        it = iter(partners)
        sources = tuple(n if t == q else next(it) for t in range(4))
    else:
        sources = tuple(int(v) for v in group)
        if len(sources) != 4 or not all(0 <= s < B for s in sources):
            raise FdError(f"sample_mosaic: a group is four indices into the {B} images (got {group!r})")
    lo, hi = centre_range
    xc = rng.randint(int(W * lo), int(W * hi))
    yc = rng.randint(int(H * lo), int(H * hi))
    tiles, gains, scales, tsizes, places, out_b, out_o = [], [], [], [], [], [], []
    for t, s in enumerate(sources):
        h, w = (int(v) for v in sizes[s])
        p, b = sample_params(h, w, boxes_list[s], rng, flip_p, augment)
        g = rng.uniform(*scale_range)
        L = max(1, int(round(g * max(H, W))))
        scale, nh, nw = resize_rule(p.out_hw[0], p.out_hw[1], (L, L))
        nh, nw = max(nh, 1), max(nw, 1)
        px, py = (xc if t & 1 else xc - nw), (yc if t & 2 else yc - nh)
        kept, idx = mosaic_tile_boxes(b, scale, px, py, nh, nw, t, xc, yc, H, W, min_side, min_visible)
        tiles.append(p), gains.append(g), scales.append(scale), tsizes.append((nh, nw)), places.append((px, py))
        out_b.append(kept)
        out_o.append(np.stack([np.full(idx.shape[0], s, np.int64), idx], 1))
    params = MosaicParams((xc, yc), sources, tuple(tiles), tuple(gains), tuple(scales), tuple(tsizes), tuple(places))
    return params, np.concatenate(out_b, 0), np.concatenate(out_o, 0)


def collate_train_mosaic(images: Sequence[torch.Tensor], boxes_list, classes_list, out_size=(640, 640), rng=None, augment: bool = True,
                         flip_p: float = 0.5, scale_range=(0.5, 1.0), centre_range=(0.25, 0.75), min_side: float = 2.0, min_visible: float = 0.2,
                         fill=(0, 0, 0), groups=None, mean=MEAN, std=STD, return_params: bool = False):
    """A mosaic training batch from RAW images: decoded uint8 [h_n, w_n, 3] CUDA images, their boxes (fp32 [k_n, 4], x1 y1 x2 y2,
    host) and classes -> collate_fn's triple (batch_imgs [B, 3, H, W] fp32 CUDA, batch_boxes [B, M, 4] fp32 CUDA, batch_classes
    [B, M] int64 CUDA) with B = len(images) outputs on one (H, W) = out_size canvas, both sides multiples of 32.

    Output n holds image n and three partners tiled around a random centre, every tile through the reference's per-image
    transforms (sample_params) and a random gain; sample_mosaic states the draws, the tile sizes, the placement and the box rule
    (this project's definition) and is called for n = 0 .. B - 1 in turn.  groups (int [B][4], tile order) fixes the sources
    instead of drawing partners.  Classes follow their boxes, padding is -1, and a batch without any box returns the [B, 0, 4] /
    [B, 0] empties of collate_train_raw.  The host draws and moves boxes; every pixel is one device launch
    (ops.mosaic_collate_u8: two small uploads, no synchronisation).  return_params=True appends the list of MosaicParams."""
    images = list(images)
    B = len(images)
    if B < 1 or len(boxes_list) != B or len(classes_list) != B:
        raise FdError("collate_train_mosaic: images, boxes_list and classes_list must be non-empty and of one length")
    for t in images:
        ops._check_raw_image(t, "collate_train_mosaic")
    H, W = (int(v) for v in out_size)
    if H < 32 or W < 32 or H % 32 or W % 32:
        raise FdError(f"collate_train_mosaic: out_size sides must be positive multiples of 32 (got {tuple(out_size)})")
    if groups is not None and len(groups) != B:
        raise FdError("collate_train_mosaic: groups holds four source indices per output")
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    host_boxes, host_classes = [], []
    for bx, cl in zip(boxes_list, classes_list):
        b = np.array(bx.cpu().numpy() if isinstance(bx, torch.Tensor) else bx, dtype=np.float32).reshape(-1, 4)
        c = np.asarray(cl.cpu().numpy() if isinstance(cl, torch.Tensor) else cl, dtype=np.int64).reshape(-1)
        if c.shape[0] != b.shape[0]:
            raise FdError(f"collate_train_mosaic: {b.shape[0]} boxes but {c.shape[0]} classes")
        host_boxes.append(b), host_classes.append(c)
    params, tiles, centres, out_boxes, out_classes = [], [], [], [], []
    for n in range(B):
        p, b, origin = sample_mosaic(sizes, host_boxes, n, (H, W), rng, flip_p, augment, scale_range, centre_range, min_side, min_visible,
                                     None if groups is None else groups[n])
        params.append(p)
        centres.append(p.centre)
        tiles.append([dict(p.tiles[t].record_kwargs(), src=p.sources[t], px=p.placements[t][0], py=p.placements[t][1], nh=p.sizes[t][0],
                           nw=p.sizes[t][1]) for t in range(4)])
        out_boxes.append(b)
        out_classes.append(np.array([host_classes[s][i] for s, i in origin], np.int64))
    batch_imgs, _ = ops.mosaic_collate_u8(images, tiles, centres, H, W, mean, std, fill=fill)
    M = max(b.shape[0] for b in out_boxes)
    dev = images[0].device
    if M == 0:              # no ground truth in the whole batch: nothing to upload
        batch_boxes = torch.empty(B, 0, 4, dtype=torch.float32, device=dev)
        batch_classes = torch.empty(B, 0, dtype=torch.int64, device=dev)
    else:
        # one upload: B*M*4 fp32 box words, then B*M int64 classes as int32 pairs (the box part is a multiple of 16 bytes)
        pack = np.empty(B * M * 6, np.int32)
        pb = pack[:B * M * 4].view(np.float32).reshape(B, M, 4)
        pc = pack[B * M * 4:].view(np.int64).reshape(B, M)
        pb[...] = -1
        pc[...] = -1
        for i, (b, c) in enumerate(zip(out_boxes, out_classes)):
            pb[i, :b.shape[0]] = b
            pc[i, :c.shape[0]] = c
        dev_pack = torch.from_numpy(pack).to(dev, non_blocking=True)
        batch_boxes = dev_pack[:B * M * 4].view(torch.float32).view(B, M, 4)
        batch_classes = dev_pack[B * M * 4:].view(torch.int64).view(B, M)
    if return_params:
        return batch_imgs, batch_boxes, batch_classes, params
    return batch_imgs, batch_boxes, batch_classes
