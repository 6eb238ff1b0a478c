"""Mosaic restated in numpy -- the checker of fd_mosaic_collate_u8 and data.augment.collate_train_mosaic.  Nothing
here comes from the package: pixels are tests/augment_ref.py's fused_levels per tile pasted into the tile's quadrant, the boxes
are the rule of the issue written out again."""
import numpy as np

import augment_ref as A
import resize_ref

F = np.float32


def quadrant(t, xc, yc, H, W):
    """(x0, x1, y0, y1) of tile t's quadrant, half open."""
    x0, x1 = (xc, W) if t & 1 else (0, xc)
    y0, y1 = (yc, H) if t & 2 else (0, yc)
    return x0, x1, y0, y1


def visible(t, xc, yc, H, W, px, py, nh, nw):
    """The quadrant intersected with the tile's rectangle, or None when that is empty."""
    x0, x1, y0, y1 = quadrant(t, xc, yc, H, W)
    vx0, vx1, vy0, vy1 = max(x0, px), min(x1, px + nw), max(y0, py), min(y1, py + nh)
    if vx1 <= vx0 or vy1 <= vy0:
        return None
    return vx0, vx1, vy0, vy1


def mosaic_levels(sources, tiles, centre, H, W, fill=(0, 0, 0)):
    """uint8 [H, W, 3] of one output.  tiles: four dict(src=, px=, py=, nh=, nw=, flip=, chain=, d=, crop=)."""
    xc, yc = centre
    out = np.empty((H, W, 3), np.uint8)
    out[...] = np.array(fill, np.uint8)
    for t, tile in enumerate(tiles):
        kw = {k: v for k, v in tile.items() if k not in ("src", "px", "py", "nh", "nw")}
        nh, nw, px, py = tile["nh"], tile["nw"], tile["px"], tile["py"]
        v = visible(t, xc, yc, H, W, px, py, nh, nw)
        if v is None:
            continue
        vx0, vx1, vy0, vy1 = v
        img = A.fused_levels(sources[tile["src"]], nh, nw, nh, nw, **kw)
        out[vy0:vy1, vx0:vx1] = img[vy0 - py:vy1 - py, vx0 - px:vx1 - px]
    return out


def mosaic_planar(sources, tiles, centre, H, W, mean, std, fill=(0, 0, 0)):
    """fp32 [3, H, W]: mosaic_levels through the Normalize expression ((float)level / 255 - mean) / std in fp32."""
    lv = mosaic_levels(sources, tiles, centre, H, W, fill)
    return np.ascontiguousarray(resize_ref.normalise(lv, mean, std)[..., :3].transpose(2, 0, 1))


KEPT_WHOLE, CLIPPED_KEPT, DROPPED_SIZE, DROPPED_VISIBLE, DROPPED_DEGENERATE = "whole", "clipped", "size", "visible", "degenerate"


def tile_boxes(boxes, scale, px, py, nh, nw, t, xc, yc, H, W, min_side=2.0, min_visible=0.2):
    """The box rule for one tile: (kept boxes fp32 [k, 4], indices of the kept rows, the kind of every input row)."""
    b = np.array(boxes, np.float32).reshape(-1, 4)
    v = visible(t, xc, yc, H, W, px, py, nh, nw)
    if v is None or b.shape[0] == 0:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int64), ["novisible"] * b.shape[0]
    vx0, vx1, vy0, vy1 = v
    kept, idx, kinds = [], [], []
    for i, row in enumerate(b):
        x1, y1, x2, y2 = (row * F(scale)).astype(np.float32)                 # 1. scale
        x1, x2, y1, y2 = F(x1 + F(px)), F(x2 + F(px)), F(y1 + F(py)), F(y2 + F(py))        # 2. translate
        ow, oh = F(x2 - x1), F(y2 - y1)
        cx1, cx2 = (min(max(x, F(vx0)), F(vx1 - 1)) for x in (x1, x2))      # 4. clip
        cy1, cy2 = (min(max(y, F(vy0)), F(vy1 - 1)) for y in (y1, y2))
        cw, ch = F(cx2 - cx1), F(cy2 - cy1)
        if not (ow > 0 and oh > 0):                                          # 5. keep
            kinds.append(DROPPED_DEGENERATE)
        elif not (cw >= F(min_side) and ch >= F(min_side)):
            kinds.append(DROPPED_SIZE)
        elif not (F(cw * ch) >= F(F(min_visible) * F(ow * oh))):
            kinds.append(DROPPED_VISIBLE)
        else:
            kinds.append(KEPT_WHOLE if (cx1, cy1, cx2, cy2) == (x1, y1, x2, y2) else CLIPPED_KEPT)
            kept.append([cx1, cy1, cx2, cy2])
            idx.append(i)
    return np.array(kept, np.float32).reshape(-1, 4), np.array(idx, np.int64), kinds


def output_boxes(tile_inputs, centre, H, W, min_side=2.0, min_visible=0.2):
    """One output: tile_inputs[t] = (boxes after the tile's own augmentation, classes, scale, px, py, nh, nw) -> (boxes [k, 4],
    classes [k], kinds of every input row), tiles 0 .. 3 in order, source order within a tile."""
    xc, yc = centre
    bs, cs, kinds = [], [], []
    for t, (boxes, classes, scale, px, py, nh, nw) in enumerate(tile_inputs):
        kb, idx, kd = tile_boxes(boxes, scale, px, py, nh, nw, t, xc, yc, H, W, min_side, min_visible)
        bs.append(kb)
        cs.append(np.asarray(classes, np.int64).reshape(-1)[idx])
        kinds += kd
    return np.concatenate(bs, 0), np.concatenate(cs, 0), kinds


def pad_batch(box_list, class_list):
    """collate_fn's padding with -1; the [B, 0, 4] / [B, 0] empties when the whole batch has no box."""
    B, M = len(box_list), max(b.shape[0] for b in box_list)
    pb, pc = np.full((B, M, 4), -1, np.float32), np.full((B, M), -1, np.int64)
    for i, (b, c) in enumerate(zip(box_list, class_list)):
        pb[i, :b.shape[0]] = b
        pc[i, :c.shape[0]] = c
    return pb, pc
