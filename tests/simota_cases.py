"""Inputs of the SimOTA tests, shared by test_simota_cpu.py (which proves on the numpy restatement what each case exercises and
that every decision of the random cases keeps a margin) and test_simota_gpu.py (which runs them on the device).  A case is a dict:
cls [B, L, C], cnt [B, L], reg [B, L, 4] f32 predictions, gt [B, M, 4] f32, labels [B, M] int64, level_hw, strides, top_q,
centre_radius, iou_weight, inside_eps, quality (0 centre-ness, 1 IoU).  The pyramids are those of atss_cases.py."""
import numpy as np

from atss_cases import STRIDES5, pyramid
from atss_ref import centres

F = np.float32
EPS = 0.01


def _case(cls, cnt, reg, gt, labels, level_hw, strides, top_q=10, centre_radius=2.5, iou_weight=3.0, inside_eps=EPS, quality=0):
    labels = np.asarray(labels, dtype=np.int64)
    cls = np.asarray(cls, dtype=F)
    B, L, C = cls.shape
    return dict(cls=cls, cnt=np.asarray(cnt, dtype=F).reshape(B, L), reg=np.asarray(reg, dtype=F).reshape(B, L, 4),
                gt=np.asarray(gt, dtype=F).reshape(labels.shape + (4,)), labels=labels, level_hw=[tuple(hw) for hw in level_hw],
                strides=list(strides), top_q=top_q, centre_radius=centre_radius, iou_weight=iou_weight, inside_eps=inside_eps, quality=quality)


def exact_reg(gt_row, level_hw, strides):
    """reg_pred [L, 4] that reproduces one box at every location: (cx-x1, cy-y1, x2-cx, y2-cy)."""
    cx, cy, _, _ = centres(level_hw, strides)
    x1, y1, x2, y2 = [F(v) for v in gt_row]
    return np.stack([cx - x1, cy - y1, x2 - cx, y2 - cy], 1).astype(F)


def _flat(B, L, C, cls=0.0, cnt=0.0):
    return np.full((B, L, C), cls, F), np.full((B, L), cnt, F), np.zeros((B, L, 4), F)


# ---------------------------------------------------------------------------------------------------- hand-derived cases
def equal_cost_pair():
    """A 1 x 2 level of stride 8 (centres (4, 4) and (12, 4)) under the box (0, 0, 16, 8): both locations predict the box exactly
    (iou = 1) from equal logits, so their costs are one fp32 value; top_q = 1 gives sum = 1, k = 1: location 0."""
    hw, st = [(1, 2)], [8]
    cls, cnt, reg = _flat(1, 2, 3)
    reg[0] = exact_reg([0, 0, 16, 8], hw, st)
    return _case(cls, cnt, reg, [[[0., 0., 16., 8.]]], [[2]], hw, st, top_q=1)


def preferred_beats_cheaper():
    """A 1 x 8 level of stride 8 (centres x = 4 .. 60, y = 4) under the box (0, 0, 64, 8), centre (32, 4); centre_radius = 1: only
    locations 3 and 4 (|cx - 32| = 4 < 8) are preferred.  Location 0 predicts the box exactly (iou 1, the lowest cost of all),
    location 3 predicts its left half (iou 0.5), the others predict empty boxes (iou 0).  top_q = 1: k = 1, and the one positive
    is location 3, the cheaper of the preferred, not location 0."""
    hw, st = [(1, 8)], [8]
    cls, cnt, reg = _flat(1, 8, 2)
    reg[0, 0] = exact_reg([0, 0, 64, 8], hw, st)[0]
    reg[0, 3] = exact_reg([0, 0, 32, 8], hw, st)[3]
    return _case(cls, cnt, reg, [[[0., 0., 64., 8.]]], [[1]], hw, st, top_q=1, centre_radius=1.0)


def two_exact(top_q=10):
    """The level and box of preferred_beats_cheaper with the default radius (20: locations 2 .. 5 preferred): locations 2 and 5
    predict the box exactly, all others predict empty boxes: the IoUs are 1, 1, 0 ..., the sum is 2, k = 2: locations 2 and 5."""
    hw, st = [(1, 8)], [8]
    cls, cnt, reg = _flat(1, 8, 2)
    e = exact_reg([0, 0, 64, 8], hw, st)
    reg[0, 2], reg[0, 5] = e[2], e[5]
    return _case(cls, cnt, reg, [[[0., 0., 64., 8.]]], [[1]], hw, st, top_q=top_q)


def all_zero_iou():
    """The same level and box with empty predicted boxes everywhere: every iou is 0, the sum 0, k = max(0, 1) = 1; equal costs, so
    the positive is the lowest preferred location, 2."""
    hw, st = [(1, 8)], [8]
    cls, cnt, reg = _flat(1, 8, 2)
    return _case(cls, cnt, reg, [[[0., 0., 64., 8.]]], [[1]], hw, st)


def few_candidates():
    """n < top_q: the box (0, 0, 24, 8) holds three locations (centres 4, 12, 20) of the 1 x 8 level; 0 and 1 predict it exactly,
    2 predicts an empty box: n = 3, sum = 2, k = 2.  Image 1: the box (0, 0, 8, 8) holds one location, which predicts an empty box:
    n = 1, sum = 0, k = min(max(0, 1), 1) = 1."""
    hw, st = [(1, 8)], [8]
    cls, cnt, reg = _flat(2, 8, 2)
    e = exact_reg([0, 0, 24, 8], hw, st)
    reg[0, 0], reg[0, 1] = e[0], e[1]
    return _case(cls, cnt, reg, [[[0., 0., 24., 8.]], [[0., 0., 8., 8.]]], [[1], [2]], hw, st)


def no_candidates():
    """A valid box between the centres (4, 4) and (12, 4): n = 0, k = 0, everything negative."""
    hw, st = [(1, 8)], [8]
    cls, cnt, reg = _flat(1, 8, 2)
    return _case(cls, cnt, reg, [[[5., 1., 11., 7.]]], [[1]], hw, st)


def inside_boundary():
    """A 1 x 1 level of stride 1 has its centre at (0, 0), so cx - x1 = -x1 exactly.  Image 0: x1 = -eps, the offset equals
    inside_eps and is rejected; image 1: x1 = -(the next fp32 above eps), accepted."""
    e = F(EPS)
    e1 = np.nextafter(e, F(1))
    cls, cnt, reg = _flat(2, 1, 4)
    return _case(cls, cnt, reg, [[[-e, -5., 5., 5.]], [[-e1, -5., 5., 5.]]], [[3], [3]], [(1, 1)], [1])


def twin_rows():
    """Rows 0 and 1 are the same box under different labels, the logits are one constant and every location predicts the box:
    every positive location is claimed twice at equal (preference, cost) -> row 0."""
    hw = pyramid(64, 64)
    L = sum(h * w for h, w in hw)
    cls, cnt, reg = _flat(1, L, 9)
    reg[0] = exact_reg([8, 8, 56, 48], hw, STRIDES5)
    return _case(cls, cnt, reg, [[[8., 8., 56., 48.], [8., 8., 56., 48.]]], [[5, 9]], hw, STRIDES5)


def skipped_rows():
    """One valid row (row 3) among label 0, label C + 1, negative label, degenerate (x2 == x1, y2 < y1) and non-finite rows."""
    n, i = np.nan, np.inf
    hw = pyramid(64, 64)
    L = sum(h * w for h, w in hw)
    rng = np.random.RandomState(7)
    cls, cnt = rng.randn(1, L, 6).astype(F), rng.randn(1, L).astype(F)
    reg = exact_reg([12, 9, 50, 44], hw, STRIDES5)[None] * np.exp(0.2 * rng.randn(1, L, 4)).astype(F)
    gt = [[[5., 5., 30., 30.], [10., 10., 10., 40.], [10., 30., 40., 20.], [12., 9., 50., 44.], [n, 0., 20., 20.], [0., 0., i, 20.],
           [-i, 0., 20., 20.], [5., 5., 30., 30.], [5., 5., 30., 30.]]]
    return _case(cls, cnt, reg, gt, [[0, 2, 2, 6, 1, 1, 1, 7, -1]], hw, STRIDES5)


def skipped_rows_valid_only():
    c = skipped_rows()
    return _case(c["cls"], c["cnt"], c["reg"], c["gt"][:, 3:4], c["labels"][:, 3:4], c["level_hw"], c["strides"])


def no_rows():
    hw = pyramid(64, 96)
    L = sum(h * w for h, w in hw)
    rng = np.random.RandomState(11)
    return _case(rng.randn(2, L, 3), rng.randn(2, L), rng.rand(2, L, 4) * 20, np.zeros((2, 0, 4)), np.zeros((2, 0)), hw, STRIDES5)


def non_finite_predictions(quality=0):
    """rand64x96_q10_v0 with NaN, +inf and -inf planted in the logits and the distances of locations inside the boxes."""
    c = dict(random_case("rand64x96_q10_v0"))
    cls, cnt, reg = c["cls"].copy(), c["cnt"].copy(), c["reg"].copy()
    L = cls.shape[1]
    bad = [np.nan, np.inf, -np.inf]
    for j, p in enumerate(range(3, L, 5)):
        which, v = j % 6, bad[(j // 6) % 3]                 # which == 5: left alone
        if which == 0:
            cls[:, p, j % cls.shape[2]] = v
        elif which == 1:
            cls[:, p, :] = v
        elif which == 2:
            cnt[:, p] = v
        elif which == 3:
            reg[:, p, j % 4] = v
        elif which == 4:
            reg[:, p, :] = v
    c.update(cls=cls, cnt=cnt, reg=reg, quality=quality)
    return c


def one_row(C=1):
    """M = 1, C = 1 on the small pyramid: a single box, noisy predictions."""
    hw = pyramid(64, 96)
    L = sum(h * w for h, w in hw)
    rng = np.random.RandomState(5)
    reg = exact_reg([10.3, 6.1, 80.7, 55.2], hw, STRIDES5)[None] * np.exp(0.15 * rng.randn(1, L, 4)).astype(F)
    return _case(rng.randn(1, L, C) - 1.0, rng.randn(1, L), reg, [[[10.3, 6.1, 80.7, 55.2]]], [[1]], hw, STRIDES5)


KNOWN = {"equal_cost_pair": equal_cost_pair, "preferred_beats_cheaper": preferred_beats_cheaper, "two_exact": two_exact,
         "two_exact_q16": lambda: two_exact(16), "all_zero_iou": all_zero_iou, "few_candidates": few_candidates, "no_candidates": no_candidates,
         "inside_boundary": inside_boundary, "twin_rows": twin_rows, "skipped_rows": skipped_rows, "no_rows": no_rows,
         "non_finite_q0": lambda: non_finite_predictions(0), "non_finite_q1": lambda: non_finite_predictions(1), "one_row_c1": one_row}


# ---------------------------------------------------------------------------------------------------- random cases
def _random(h, w, top_q, C, centre_radius, quality, seed):
    """B = 3, M = 7 on the five-level pyramid of an h x w image.  Per image: rows 0 / 1 a planted pair of overlapping boxes (the second
    shifted by two pixels and of another shape) so that locations are contested, row 2 centred on the image border, row 3 a wide flat box (few preferred
    locations, so that positives beyond them are taken), row 4 random, row 5 degenerate (x2 < x1), row 6 padding; image 2 has rows 4..
    as padding.  Every location predicts, with log-normal noise, the box of one of the rows that hold it (a random one), so the IoUs
    with that row are high and with the others mixed; locations outside every box predict random distances.  Logits: cls ~ N(-2, 1.5),
    cnt ~ N(0, 1): scores well inside (0, 1), as a head under training emits them."""
    rng = np.random.RandomState(seed)
    B, M = 3, 7
    hw = pyramid(h, w)
    cx, cy, lv, _ = centres(hw, STRIDES5)
    L = len(cx)
    gt = np.full((B, M, 4), -1.0)
    labels = np.full((B, M), -1, np.int64)

    def box(bx, by, bw, bh):
        return [bx - bw / 2, by - bh / 2, bx + bw / 2, by + bh / 2]
    for b in range(B):
        bx, by = w * (0.3 + 0.4 * rng.rand()) + 0.37, h * (0.3 + 0.4 * rng.rand()) + 0.23
        bw, bh = w * (0.3 + 0.3 * rng.rand()), h * (0.3 + 0.3 * rng.rand())
        gt[b, 0] = box(bx, by, bw, bh)
        gt[b, 1] = box(bx + 2.0, by + 2.0, bw * 1.07, bh * 0.95)
        gt[b, 2] = box(0.0, h * rng.rand(), w * 0.375, h * 0.5) if b % 2 == 0 else box(w * rng.rand(), float(h), w * 0.5, h * 0.375)
        gt[b, 3] = box(w * 0.5 + 1.3, 4.0 + (h - 8.0) * rng.rand(), w * 0.9, 6.6)
        labels[b, :4] = rng.randint(1, C + 1, 4)
        if b < 2:
            gt[b, 4] = box(w * rng.rand(), h * rng.rand(), w * (0.1 + 0.5 * rng.rand()), h * (0.1 + 0.5 * rng.rand()))
            gt[b, 5] = [30.0, 10.0, 20.0, 40.0]
            labels[b, 4:6] = rng.randint(1, C + 1, 2)
    gt = gt.astype(F)
    cls = (rng.randn(B, L, C) * 1.5 - 2.0).astype(F)
    cnt = rng.randn(B, L).astype(F)
    reg = (np.asarray(STRIDES5)[lv][None, :, None] * (0.5 + 3.5 * rng.rand(B, L, 4))).astype(F)
    for b in range(B):
        for p in range(L):
            holds = [m for m in range(M) if labels[b, m] >= 1 and gt[b, m, 2] > gt[b, m, 0] and gt[b, m, 3] > gt[b, m, 1]
                     and min(cx[p] - gt[b, m, 0], cy[p] - gt[b, m, 1], gt[b, m, 2] - cx[p], gt[b, m, 3] - cy[p]) > 0]
            if holds:
                m = holds[rng.randint(len(holds))]
                g = gt[b, m]
                sigma = 0.04 if m == 3 else 0.25
                reg[b, p] = np.array([cx[p] - g[0], cy[p] - g[1], g[2] - cx[p], g[3] - cy[p]]) * np.exp(sigma * rng.randn(4))
    return _case(cls, cnt, reg, gt, labels, hw, STRIDES5, top_q=top_q, centre_radius=centre_radius, quality=quality)


# name -> (h, w, top_q, C, centre_radius, quality, seed).  The seeds were chosen on the CPU so that every decision of the float64
# restatement keeps the margins test_simota_cpu.py demands; it proves that for every case, every time it runs.
RANDOM = {
    "rand64x96_q1_v0": (64, 96, 1, 3, 0.3, 0, 1),
    "rand64x96_q1_v1": (64, 96, 1, 80, 0.2, 1, 0),
    "rand64x96_q10_v0": (64, 96, 10, 80, 2.5, 0, 1),
    "rand64x96_q10_v1": (64, 96, 10, 1, 0.75, 1, 0),
    "rand64x96_q16_v0": (64, 96, 16, 3, 2.5, 1, 0),
    "rand64x96_q16_v1": (64, 96, 16, 80, 0.75, 0, 0),
    "rand256x320_q1_v0": (256, 320, 1, 1, 0.3, 1, 0),
    "rand256x320_q1_v1": (256, 320, 1, 3, 0.2, 0, 0),
    "rand256x320_q10_v0": (256, 320, 10, 80, 2.5, 0, 0),
    "rand256x320_q10_v1": (256, 320, 10, 3, 0.75, 1, 0),
    "rand256x320_q16_v0": (256, 320, 16, 1, 2.5, 0, 1),
    "rand256x320_q16_v1": (256, 320, 16, 80, 0.75, 1, 0),
}
EXTRA = {"rand128x128_q10": (128, 128, 10, 20, 2.5, 0, 1)}        # the loss test's image: the smallest the FPN's five levels fit
_CACHE = {}


def random_case(name):
    if name not in _CACHE:
        c = _random(*{**RANDOM, **EXTRA}[name])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]


def get(name):
    return KNOWN[name]() if name in KNOWN else random_case(name)


def args(c):
    """The keyword arguments a case passes to simota_ref.simota_gen_targets after the five tensors and the level table."""
    return dict(top_q=c["top_q"], centre_radius=c["centre_radius"], iou_weight=c["iou_weight"], inside_eps=c["inside_eps"], quality=c["quality"])


ALL = list(KNOWN) + list(RANDOM)
