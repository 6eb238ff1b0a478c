"""The inputs shared by tests/test_mosaic_cpu.py and tests/test_mosaic_gpu.py: the hand-built kernel cases, the
random batches for collate_train_mosaic, and `replay`, which restates the documented order of draws, the tile size and the
placement (the only package function it calls is sample_params, which mosaic leaves unchanged)."""
import numpy as np

from pytorch_object_detection_amd.data.augment import sample_params

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OP_B, OP_C, OP_S, OP_HUE = 1, 2, 3, 4
SOURCE_SIZES = [(1, 1), (7, 5), (37, 53), (50, 41), (64, 64)]
CANVASES = [(32, 32), (64, 96), (96, 64)]
CHAINS = [[], [(OP_S, 1.07), (OP_B, 0.93), (OP_HUE, 20), (OP_C, 1.09)], [(OP_C, 1.08), (OP_B, 0.95)], [(OP_HUE, 240), (OP_S, 1.1)], [(OP_B, 1.1), (OP_C, 0.92), (OP_HUE, 12)]]


def sources(seed=31):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SOURCE_SIZES]


def _crop_for(h, w, k):
    if h >= 30:
        return [(3, 5, w - 11, h - 9), (w - 1, 0, 1, h), (0, h - 1, w, 1), None][k % 4]
    if (h, w) == (7, 5):
        return [(1, 1, 3, 4), None][k % 2]
    return None


def kernel_case(k, N=5):
    """Canvas k: (H, W, centres [N], tiles [N][4]).  Centres take 0, 1, side - 1, side and an interior value on both axes in
    different pairings per canvas; tile placements cycle through: corner at the centre and larger than the quadrant / short of the
    centre so that fill shows between the tiles / negative offsets with a tile larger than the canvas; every source appears in
    several tiles and outputs with different chains; flip, rotation, crop and all four chain operations occur."""
    H, W = CANVASES[k]
    xs, ys = [0, 1, W - 1, W, W // 2 + 3], [0, 1, H - 1, H, H // 2 - 5]
    centres = [(xs[n % 5], ys[(n + k) % 5]) for n in range(N)]
    tiles = []
    for n in range(N):
        xc, yc = centres[n]
        quad = []
        for t in range(4):
            j = n * 4 + t
            src = (n + 2 * t + k) % 5
            h, w = SOURCE_SIZES[src]
            mode = (n + t + k) % 3
            if mode == 0:
                nh, nw = H // 2 + 9 + t, W // 2 + 5 + n
                px, py = (xc if t & 1 else xc - nw), (yc if t & 2 else yc - nh)
            elif mode == 1:
                nh, nw = 9 + 2 * t, 7 + 3 * n
                px, py = (xc + 2 if t & 1 else xc - nw - 3), (yc + 1 if t & 2 else yc - nh - 2)
            else:
                nh, nw = H + 10, W + 7
                px, py = -5 - t, -9 + n
            quad.append(dict(src=src, px=px, py=py, nh=nh, nw=nw, flip=bool(j & 1), chain=CHAINS[(j + k) % 5], d=[0.0, 7.3, -10.0, 0.0, 2.5][(j + n) % 5],
                             crop=_crop_for(h, w, j)))
        tiles.append(quad)
    return H, W, centres, tiles


# ---------------------------------------------------------------------------------------------- collate_train_mosaic
BATCH_SIZES = [(37, 53), (50, 41), (64, 64), (7, 5), (53, 37)]


def batch(seed=17):
    """Five raw images with boxes and classes: boxes of every scale from a few pixels to most of the image, one degenerate row,
    and one image without any box."""
    rng = np.random.default_rng(seed)
    raws, boxes, classes = [], [], []
    for i, (h, w) in enumerate(BATCH_SIZES):
        raws.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        n = [6, 5, 7, 0, 4][i]
        xy = rng.uniform(0, 0.7, (n, 2)) * [w, h]
        wh = rng.uniform(0.03, 0.9, (n, 2)) * [w, h]
        b = np.concatenate([xy, np.minimum(xy + wh, [w - 1, h - 1])], 1).astype(np.float32)
        if n:
            b[-1, 2] = b[-1, 0]                                   # a degenerate row
        boxes.append(b)
        classes.append(rng.integers(1, 21, n).astype(np.int64))
    return raws, boxes, classes


# (seed, keywords) of the collate_train_mosaic runs on batch(): test_mosaic_cpu.py shows that each holds every kind of box
COLLATE_CASES = [(5, {}), (8, dict(fill=(114, 114, 114), min_visible=0.4)), (11, dict(groups=[[0, 1, 2, 3], [4, 4, 4, 4], [2, 0, 2, 1], [3, 3, 0, 0], [1, 2, 3, 4]]))]


def resize_rule(h, w, size):
    """preprocess_img_boxes' size rule, restated: short side to min_side, long side capped at max_side, truncated."""
    min_side, max_side = size
    scale = min_side / min(w, h)
    if max(w, h) * scale > max_side:
        scale = max_side / max(w, h)
    return scale, int(scale * h), int(scale * w)


def replay(sizes, boxes_list, n, H, W, rng, flip_p=0.5, augment=True, scale_range=(0.5, 1.0), centre_range=(0.25, 0.75), group=None):
    """The documented draws of mosaic output n, in order: dict(centre, sources, tiles (AugmentParams), gains, scales, sizes,
    placements, aug_boxes (every tile's boxes after its own augmentation, before the mosaic box rule))."""
    B = len(sizes)
    if group is None:
        partners = [rng.randrange(B), rng.randrange(B), rng.randrange(B)]
        q = rng.randrange(4)
        srcs = list(partners)
        srcs.insert(q, n)
    else:
        srcs = list(group)
    lo, hi = centre_range
    xc = rng.randint(int(W * lo), int(W * hi))
    yc = rng.randint(int(H * lo), int(H * hi))
    out = dict(centre=(xc, yc), sources=tuple(srcs), tiles=[], gains=[], scales=[], sizes=[], placements=[], aug_boxes=[])
    for t, s in enumerate(srcs):
        h, w = sizes[s]
        p, b = sample_params(h, w, np.array(boxes_list[s], np.float32), rng, flip_p, augment)
        g = rng.uniform(*scale_range)
        L = max(1, int(round(g * max(H, W))))
        scale, nh, nw = resize_rule(p.out_hw[0], p.out_hw[1], (L, L))
        nh, nw = max(nh, 1), max(nw, 1)
        px = xc if t in (1, 3) else xc - nw
        py = yc if t in (2, 3) else yc - nh
        out["tiles"].append(p), out["gains"].append(g), out["scales"].append(scale), out["sizes"].append((nh, nw)), out["placements"].append((px, py))
        out["aug_boxes"].append(b)
    return out


def tile_dicts(r):
    """replay's result (or a MosaicParams) as the tile dictionaries of mosaic_ref.mosaic_levels / ops.mosaic_collate_u8."""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    return [dict(src=g("sources")[t], px=g("placements")[t][0], py=g("placements")[t][1], nh=g("sizes")[t][0], nw=g("sizes")[t][1], flip=g("tiles")[t].flip,
                 chain=list(g("tiles")[t].chain), d=g("tiles")[t].d, crop=g("tiles")[t].crop) for t in range(4)]
