"""Inputs of the ATSS tests, shared by test_atss_cpu.py (which proves on the numpy restatement what each case exercises) and
test_atss_gpu.py (which runs them on the device).  A case is a dict: gt [B, M, 4] f32, labels [B, M] int64, level_hw, strides,
topk, anchor_scale, inside_eps."""
import numpy as np

F = np.float32
EPS = 0.01
STRIDES5 = [8, 16, 32, 64, 128]
GRID5_PICKS16 = [12, 7, 11, 13, 17, 6, 8, 16, 18, 2, 10, 14, 22, 1, 3, 5]


def pyramid(h, w, strides=STRIDES5):
    return [(-(-h // s), -(-w // s)) for s in strides]


def _case(gt, labels, level_hw, strides, topk=9, anchor_scale=8.0, inside_eps=EPS):
    gt = np.asarray(gt, dtype=F)
    labels = np.asarray(labels, dtype=np.int64)
    return dict(gt=gt.reshape(labels.shape + (4,)), labels=labels, level_hw=[tuple(hw) for hw in level_hw], strides=list(strides), topk=topk,
                anchor_scale=anchor_scale, inside_eps=inside_eps)


def grid5(topk):
    """One 5 x 5 level of stride 8 (centres 4, 12, 20, 28, 36) and a box centred exactly on the grid point (20, 20) = pix 12.
    Squared distances: 0 once; 64 four times (pix 7, 11, 13, 17); 128 four times (6, 8, 16, 18); 256 four times (2, 10, 14, 22);
    320 eight times (1, 3, 5, 9, 15, 19, 21, 23).  With the lower index first, topk = 9 picks GRID5_PICKS16[:9] and topk = 16 all
    of GRID5_PICKS16: the eight-way tie gives its first three."""
    return _case([[[6., 6., 34., 34.]]], [[4]], [(5, 5)], [8], topk=topk)


def equal_ious():
    """One 3 x 3 level of stride 8: every anchor (side 64, centres 4 / 12 / 20) lies inside the box, so the nine IoUs are one
    fp32 value v = 4096 / 90000; 9 v is exact in fp64, mean = v, std = 0, thr = v: all nine are positive by `>=`, none by `>`."""
    return _case([[[-100., -100., 200., 200.]]], [[2]], [(3, 3)], [8])


def single_location():
    """n == 1: a 1 x 1 level of stride 128, centre (64, 64); std = 0, thr = the one IoU, which is positive."""
    return _case([[[10., 10., 100., 120.]]], [[7]], [(1, 1)], [128])


def short_levels():
    """Levels of 6 and 2 locations under topk = 9: k_l = 6 and 2, n = 8.  Anchors of side 16 and 32, so the IoUs differ."""
    return _case([[[3., 2., 20., 15.]]], [[1]], [(2, 3), (1, 2)], [8, 16], anchor_scale=2.0)


def inside_boundary():
    """A 1 x 1 level of stride 1 has its centre at (0, 0), so cx - x1 = -x1 exactly.  Image 0: x1 = -eps, the offset equals
    inside_eps and is rejected; image 1: x1 = -(the next fp32 above eps), accepted.  n == 1, so the IoU test always passes."""
    e = F(EPS)
    e1 = np.nextafter(e, F(1))
    return _case([[[-e, -5., 5., 5.]], [[-e1, -5., 5., 5.]]], [[3], [3]], [(1, 1)], [1])


def twin_rows():
    """Rows 0 and 1 are the same box under different labels: every positive location is claimed twice with equal IoU -> row 0."""
    return _case([[[8., 8., 56., 48.], [8., 8., 56., 48.]]], [[5, 9]], pyramid(64, 64), STRIDES5)


def skipped_rows():
    """One valid row (row 3) among padding, degenerate (x2 == x1, y2 < y1) and non-finite rows."""
    n, i = np.nan, np.inf
    gt = [[[-1., -1., -1., -1.], [10., 10., 10., 40.], [10., 30., 40., 20.], [12., 9., 50., 44.], [n, 0., 20., 20.], [0., 0., i, 20.],
           [-i, 0., 20., 20.], [5., 5., 30., 30.]]]
    return _case(gt, [[-1, 2, 2, 6, 1, 1, 1, -1]], pyramid(64, 64), STRIDES5)


def skipped_rows_valid_only():
    c = skipped_rows()
    return _case(c["gt"][:, 3:4], c["labels"][:, 3:4], c["level_hw"], c["strides"])


def no_rows():
    return _case(np.zeros((2, 0, 4)), np.zeros((2, 0)), pyramid(64, 96), STRIDES5)


KNOWN = {"grid5_k9": lambda: grid5(9), "grid5_k16": lambda: grid5(16), "equal_ious": equal_ious, "single_location": single_location,
         "short_levels": short_levels, "inside_boundary": inside_boundary, "twin_rows": twin_rows, "skipped_rows": skipped_rows,
         "no_rows": no_rows}


def random_case(h, w, topk, anchor_scale, seed=0):
    """B = 3, M = 7, 20 classes on the five-level pyramid of an h x w image.  Per image: rows 0 / 1 a planted pair of overlapping
    boxes (the second shifted by two pixels) so that locations are contested, row 2 centred on the image border, row 3 centred outside
    the image, row 4 random, row 5 degenerate (x2 < x1), row 6 padding; image 2 has rows 3.. as padding.  Centres sit at
    non-dyadic offsets."""
    rng = np.random.RandomState(1000 * h + 10 * topk + int(anchor_scale) + seed)
    B, M = 3, 7
    gt = np.full((B, M, 4), -1.0)
    labels = np.full((B, M), -1, np.int64)

    def box(cx, cy, bw, bh):
        return [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]
    for b in range(B):
        cx, cy = w * (0.3 + 0.4 * rng.rand()) + 0.37, h * (0.3 + 0.4 * rng.rand()) + 0.23
        bw, bh = w * (0.3 + 0.3 * rng.rand()), h * (0.3 + 0.3 * rng.rand())
        gt[b, 0] = box(cx, cy, bw, bh)
        gt[b, 1] = box(cx + 2.0, cy + 2.0, bw, bh)
        gt[b, 2] = box(0.0, h * rng.rand(), w * 0.375, h * 0.5) if b % 2 == 0 else box(w * rng.rand(), float(h), w * 0.5, h * 0.375)
        labels[b, :3] = rng.randint(1, 21, 3)
        if b < 2:
            gt[b, 3] = box(w + 10.3, -7.1, w * 0.3, h * 0.3)
            gt[b, 4] = box(w * rng.rand(), h * rng.rand(), w * (0.1 + 0.5 * rng.rand()), h * (0.1 + 0.5 * rng.rand()))
            gt[b, 5] = [30.0, 10.0, 20.0, 40.0]
            labels[b, 3:6] = rng.randint(1, 21, 3)
    return _case(gt, labels, pyramid(h, w), STRIDES5, topk=topk, anchor_scale=anchor_scale)


RANDOM = {f"rand{h}x{w}_k{k}_a{a}": (h, w, k, float(a)) for (h, w) in ((64, 96), (256, 320)) for k in (1, 9, 16) for a in (4, 8)}


EXTRA = {"rand128x128_k9_a8": (128, 128, 9, 8.0)}        # the loss test's image: the smallest the FPN's five levels fit


def get(name):
    return KNOWN[name]() if name in KNOWN else random_case(*{**RANDOM, **EXTRA}[name])


ALL = list(KNOWN) + list(RANDOM)
