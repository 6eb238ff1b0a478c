"""Designed inputs for the loss and target kernels of csrc/fd_loss.hip: every comparison those kernels are made of is
hit by construction instead of by chance.  Plain builders returning CPU tensors, shared by test_loss_edges_cpu.py
(which proves each edge is hit and that the fp32 oracle meets the GPU test's tolerances against float64) and
test_loss_edges_gpu.py.  All values are finite and exact in fp32, so a float64 evaluation of the oracle decides every
tie and comparison the way the fp32 kernels do."""
import torch
import torch.nn.functional as F

from oracle import torch_ref as R

B = 3
LS = (1, 255, 256, 257, 513)
IMG_W = (0.5, 1.75, 3.0)          # unequal weights of the per-image losses: (out * w).sum().backward() gives a distinct gscale[b]

# tolerances of tests/test_loss_gpu.py for the same kernels
LOSS_RTOL = 1e-5
GRAD_TOL = dict(rtol=2e-5, atol=1e-8)
FOCAL_LOSS_RTOL = 2e-6
FOCAL_GRAD_TOL = dict(rtol=3e-5, atol=1e-9)

# ---------------------------------------------------------------------------------------------------- LTRB IoU / GIoU
# (name, pred (l, t, r, b), target (l, t, r, b)); every row has a non-zero union and enclosing area.  No perfect prediction
# at the 1e-3 scale: there torch's fp32 autograd adds d(ov)/U and -ov dU/U^2 with one rounding each and leaves 1e-7 / side
# where float64 (and the closed form) give 0 -- the fp32 oracle itself misses atol 1e-8 on that row.
LTRB_ROWS = (
    ("perfect", (4, 2, 4, 8), (4, 2, 4, 8)),                             # four-way tie, the limit training converges to: loss 0, gradient 0
    ("partial_tie", (4, 4, 4, 4), (4, 2, 4, 8)),                         # ties on l and r only
    ("zero_width", (8, 2, -8, 2), (8, 6, 3, 1)),                         # min(r) + min(l) == 0 with a tie on l: clamp(min=0) passes the gradient at equality
    ("iou_1.2e-6", (1, 1, 1, 1), (900, 900, 900, 900)),                  # above the 1e-6 clamp by 23 %: gradient flows
    ("iou_4e-6", (1, 1, 1, 1), (500, 500, 500, 500)),                    # above the clamp by 4x
    ("iou_clamped", (1, 1, 1, 1), (2000, 2000, 2000, 2000)),             # 2.5e-7: clamped, gradient 0 in 'iou' mode
    ("negative_sum", (10, 3, -5, 4), (2, 5, 3, 2)),                      # min(r) + min(l) == -3: width clamped to 0, nothing passes
    ("tiny", (1e-3, 2e-3, 1.5e-3, 1e-3), (2e-3, 1e-3, 1e-3, 1.5e-3)),
    ("g_clamped", (1e-6, 2e-6, 1.5e-6, 1e-6), (2e-6, 1e-6, 1e-6, 1.5e-6)),   # enclosing area 1.2e-11 < 1e-10: g.clamp(1e-10) cuts dG
    ("large", (1000.25, 2000.5, 1500.75, 3999.5), (1000.5, 2000.25, 1500.5, 4000.0)),
    ("large_perfect", (1000.25, 2000.5, 1500.75, 3999.5), (1000.25, 2000.5, 1500.75, 3999.5)),
)
# rows whose values and gradients also fit fp16 (the wrapper's half-precision input)
LTRB_ROWS_MODERATE = tuple(r for r in LTRB_ROWS if r[0] in ("perfect", "partial_tie", "zero_width", "iou_4e-6", "negative_sum"))


def _row(rows, name):
    return next(r for r in rows if r[0] == name)


def ltrb_case(L, rows=LTRB_ROWS):
    """-> pred [3, L, 4], target [3, L, 4], mask [3, L].  Image 0 has no positive, image 1 is fully positive with the
    designed rows on both sides of index 256 and again at the tail, image 2 has its only positive at L - 1.
    Masked-out rows are all-zero boxes (0 / 0 if a kernel ever looked at them)."""
    gen = torch.Generator().manual_seed(100 + L)
    pred, tgt = torch.zeros(B, L, 4), torch.zeros(B, L, 4)
    mask = torch.zeros(B, L, dtype=torch.bool)
    n = len(rows)
    P = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    T = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    tie = _row(rows, "partial_tie")
    if L >= n:
        pred[1] = torch.exp(torch.randn(L, 4, generator=gen)) * 8
        tgt[1] = torch.exp(torch.randn(L, 4, generator=gen)) * 8
        for start in sorted({min(256 - n // 2, L - n), L - n}):
            pred[1, start:start + n], tgt[1, start:start + n] = P, T
        mask[1] = True
    else:
        zw = _row(rows, "zero_width")
        pred[1, 0], tgt[1, 0] = torch.tensor(zw[1], dtype=torch.float32), torch.tensor(zw[2], dtype=torch.float32)
        mask[1, 0] = True
    pred[2, L - 1], tgt[2, L - 1] = torch.tensor(tie[1], dtype=torch.float32), torch.tensor(tie[2], dtype=torch.float32)
    mask[2, L - 1] = True
    return pred, tgt, mask


def _weighted_backward(out, leaf):
    (out * torch.tensor(IMG_W, dtype=out.dtype)).sum().backward()
    return out.detach().numpy(), leaf.grad.numpy()


def ltrb_ref(pred, tgt, mask, mode, dtype=torch.float64):
    """oracle iou_loss / giou_loss per image over the positives / max(num_pos, 1) -> (loss [3], d sum(loss * IMG_W) / d pred)."""
    p, t = pred.detach().to(dtype, copy=True).requires_grad_(True), tgt.to(dtype)
    fn = R.giou_loss if mode == "giou" else R.iou_loss
    out = torch.stack([fn(p[b][mask[b]], t[b][mask[b]]) / mask[b].sum().clamp(min=1) for b in range(p.shape[0])])
    return _weighted_backward(out, p)


# ---------------------------------------------------------------------------------------------------- centerness BCE
BCE_LOGITS = (-100.0, -88.7, -30.0, -1e-3, 0.0, 1e-3, 17.0, 30.0, 88.7, 100.0)
BCE_TARGETS = (0.0, 0.3, 0.5, 1.0)
BCE_COMBOS = tuple((x, t) for x in BCE_LOGITS for t in BCE_TARGETS)
# sigmoid(x) - t cancels here: fp32 sigmoid's half-ulp (3e-8 .. 6e-8, torch's own fp32 included) is the whole error of the
# gradient, so these combos only appear where gscale <= 0.2 keeps it under the absolute tolerance 1e-8
BCE_CANCELLING = ((17.0, 1.0), (1e-3, 0.5), (-1e-3, 0.5))


def bce_case(L):
    """-> logits [3, L], target [3, L], mask [3, L] with the mask patterns of ltrb_case.  The fully positive image cycles
    through BCE_COMBOS (gscale = w / L there); masked-out slots hold extreme finite logits."""
    x = torch.full((B, L), 100.0)
    x[:, ::2] = -100.0
    t = torch.full((B, L), 0.3)
    mask = torch.zeros(B, L, dtype=torch.bool)
    if L >= len(BCE_COMBOS):
        combos = torch.tensor([BCE_COMBOS[(i * 7) % len(BCE_COMBOS)] for i in range(L)], dtype=torch.float32)   # 7 coprime to 40
        x[1], t[1] = combos[:, 0], combos[:, 1]
        mask[1] = True
    else:
        x[1, 0], t[1, 0] = 88.7, 0.3
        mask[1, 0] = True
    x[2, L - 1], t[2, L - 1] = -30.0, 0.5
    mask[2, L - 1] = True
    return x, t, mask


def bce_ref(x, t, mask, dtype=torch.float64):
    """F.binary_cross_entropy_with_logits summed over the positives / max(num_pos, 1) -> (loss [3], weighted gradient)."""
    xx, tt = x.detach().to(dtype, copy=True).requires_grad_(True), t.to(dtype)
    out = torch.stack([F.binary_cross_entropy_with_logits(xx[b][mask[b]], tt[b][mask[b]], reduction="sum") / mask[b].sum().clamp(min=1)
                       for b in range(xx.shape[0])])
    return _weighted_backward(out, xx)


def bce_grid():
    """One image per target value, one location per logit -> logits [4, 10], target [4, 10], gscale [4] (all <= 0.2)."""
    x = torch.tensor(BCE_LOGITS, dtype=torch.float32)[None].repeat(len(BCE_TARGETS), 1)
    t = torch.tensor(BCE_TARGETS, dtype=torch.float32)[:, None].repeat(1, len(BCE_LOGITS))
    return x, t, torch.tensor([0.2, 0.125, 0.05, 0.1])


def bce_grid_ref(dtype=torch.float64):
    """-> (per-image sums [4], d sum(loss * gscale) / d logits) of bce_grid()."""
    x, t, gs = bce_grid()
    xx = x.to(dtype).requires_grad_(True)
    out = F.binary_cross_entropy_with_logits(xx, t.to(dtype), reduction="none").sum(1)
    (out * gs.to(dtype)).sum().backward()
    return out.detach().numpy(), xx.grad.numpy()


# ---------------------------------------------------------------------------------------------------- focal
FOCAL_SHAPES = ((1, 1), (7, 20), (205, 80), (820, 20), (13200, 80), (341, 81))
FOCAL_GSCALE = (0.5, 1.25, 2.0)
FOCAL_CLIP_LOGIT = -12.206072645530174          # ln(5e-6): where sigmoid crosses the lower clip (to 5e-6); every logit in a case keeps 0.15 away from it
# designed logits of a positive class (t = 1): both sides of the lower clip, and far into the saturated side
FOCAL_POS_LOGITS = (-30.0, -20.0, -13.0, -12.4, -12.0, 16.0, 40.0)
# designed logits of a background class.  1 - sigmoid(x) carries fp32 sigmoid's absolute error (6e-8), i.e. a relative error
# 6e-8 * e^x that log() turns into an absolute one: 0.04 per element at x = 16.  15.942385 = 23 ln 2 is the one point
# up there where 1 + e^-x and its reciprocal are exact in fp32; plain 16.0 is only used where the summed loss is >= 1e5.
FOCAL_BG_LOGITS = (-30.0, -20.0, -13.0, -12.4, -12.0, 15.942385)
FOCAL_BG_MAX = 16.0


def focal_special_labels(C):
    return (0, C, -1, C + 1)                     # in range; then padded GT's -1 and one past the last class, both background


def focal_case(L, C):
    """-> logits [3, L, C], labels [3, L].  Random rows (randn * 3 - 2, 5 % positives), the four special labels, and the
    designed logits spread over distinct (image, row) slots; background logits are capped at 16."""
    gen = torch.Generator().manual_seed(1000 * L + C)
    logits = torch.randn(B, L, C, generator=gen) * 3 - 2
    labels = (torch.rand(B, L, generator=gen) < 0.05).long() * torch.randint(1, C + 1, (B, L), generator=gen)
    if L * C == 1:
        logits[:, 0, 0] = torch.tensor([-12.4, 15.942385, 1.5])      # a lone background logit below 0 would leave a loss of 1e-16 made of 1 - sigmoid's rounding
        labels[:, 0] = torch.tensor([1, 0, -1])
        return logits, labels
    logits = torch.where((logits - FOCAL_CLIP_LOGIT).abs() < 0.15, torch.full_like(logits, FOCAL_CLIP_LOGIT - 0.2), logits)
    bg = FOCAL_BG_LOGITS + ((FOCAL_BG_MAX,) if L * C >= 1000000 else ())
    jobs = [("label", v) for v in focal_special_labels(C)] + [("pos", v) for v in FOCAL_POS_LOGITS] + [("bg", v) for v in bg]
    assert B * L >= len(jobs)
    for k, (kind, v) in enumerate(jobs):
        slot = (k * B * L) // len(jobs)
        row, b = divmod(slot, B)
        if kind == "label":
            labels[b, row] = v
        elif kind == "pos":
            labels[b, row] = 1 + k % C
            logits[b, row, k % C] = v
        else:
            labels[b, row] = 0
            logits[b, row, k % C] = v
    return torch.where(focal_onehot(labels, C).bool(), logits, logits.clamp(max=FOCAL_BG_MAX)), labels


def focal_onehot(labels, C, dtype=torch.float32):
    """The reference's one-hot comparison (loss.py:17): labels outside 1..C match no class."""
    return (torch.arange(1, C + 1)[None, None, :] == labels[..., None]).to(dtype)


def focal_ref(logits, labels, alpha, dtype=torch.float64):
    """oracle focal_loss per image -> (loss [3], d sum(loss * FOCAL_GSCALE) / d logits)."""
    x = logits.detach().to(dtype, copy=True).requires_grad_(True)
    onehot = focal_onehot(labels, logits.shape[-1], dtype)
    out = torch.stack([R.focal_loss(x[b], onehot[b], alpha=alpha) for b in range(x.shape[0])])
    (out * torch.tensor(FOCAL_GSCALE, dtype=dtype)).sum().backward()
    return out.detach().numpy(), x.grad.numpy()


# ---------------------------------------------------------------------------------------------------- target assignment
TGT_HW = ((16, 16), (8, 8), (4, 4))              # a 128 x 128 image: L = 336, the second block of 256 threads is partial
TGT_STRIDES = (8, 16, 32)
TGT_RANGES = ((-1, 32), (32, 64), (64, 9999999))
_PAD = (-1.0, -1.0, -1.0, -1.0)


def _boxes(images):
    M = max(len(im) for im in images)
    gt = torch.full((len(images), M, 4), -1.0)
    labels = torch.full((len(images), M), -1, dtype=torch.int64)
    for b, im in enumerate(images):
        for m, (box, lab) in enumerate(im):
            gt[b, m] = torch.tensor(box, dtype=torch.float32)
            labels[b, m] = lab
    return gt, labels


def targets_case():
    """-> gt [3, M, 4], labels [3, M].  Locations are x = stride / 2 + k * stride; each box below names the location and
    level whose comparison it sits on (all other conditions hold there).  -1 rows pad the middle and the tail."""
    img0 = [
        ((4, 20, 52, 52), 1),        # level 0 (36,36): omax == 32 == hi -> positive; level 1 (40,40): omax 36 -> positive
        ((84, 4, 100, 28), 2),       # level 0 (84,12): omin == 0
        (_PAD, -1),
        ((68, 60, 108, 100), 3),     # level 0 (76,76): cmax == 12 == 8 * 1.5
        ((8, 56, 56, 88), 4),        # level 1 (40,72): omax == 32 == lo -> negative (level 0 (36,68): omax 28, positive)
        (_PAD, -1),
        ((8, 92, 104, 156), 5),      # level 1 (72,120): omax == 64 == hi -> positive
        ((16, 40, 120, 120), 17),    # level 2 (80,80): omax == 64 == lo -> negative
    ]
    img1 = [
        ((40, 8, 80, 56), 6),        # level 1 (40,24): omin == 0
        ((16, 56, 80, 120), 7),      # level 1 (24,88): cmax == 24 == 16 * 1.5
        ((0, 0, 128, 128), 8),       # level 2 (16,48): cmax == 48 == 32 * 1.5
        (_PAD, -1),
        ((0, 0, 128, 128), 9),       # identical to box 2 with another label: the first wins wherever they are the minimum (level 2)
        ((44, 44, 76, 76), 10),      # larger box listed before ...
        ((44, 44, 68, 68), 11),      # ... the smaller one: the smaller wins at level 0 (52,52), (60,60), ...
        ((44, 44, 68, 68), 12),      # its twin with another label: equal-area tie at level 0
        ((80, 16, 100, 36), 13),     # level 1 (88,24): the area minimum, but omax == 12 is not in (32, 64] ...
        ((48, 4, 112, 60), 14),      # ... so this positive one wins there
        ((48, 4, 112, 60), 15),      # and its twin: equal-area tie at level 1
    ]
    img2 = [
        ((48, 8, 120, 120), 16),     # level 2 (48,48): omin == 0
    ]
    return _boxes([img0, img1, img2])


def targets_case_empty():
    """Same boxes with image 1 emptied: an image without any GT between two that have some."""
    gt, labels = targets_case()
    gt[1], labels[1] = -1.0, -1
    return gt, labels


def targets_case_m1():
    """M = 1: one box, a padding row, one box."""
    return _boxes([[((4, 20, 52, 52), 1)], [(_PAD, -1)], [((48, 8, 120, 120), 16)]])


ODD_HW, ODD_STRIDE, ODD_RANGE = ((9, 9),), (7,), ((-1, 64),)


def targets_case_odd_stride():
    """Stride 7 on one level: locations are 7 k + 3 (stride // 2, not 3.5), radius 10.5; half-integer boxes."""
    return _boxes([
        [((24, 10, 44, 40), 1)],                                   # (24,24): omin == 0 only if x == 7 * 3 + 3
        [((20, 14, 49, 34), 2)],                                   # centre x 34.5: (24,24) has cmax == 10.5 == 7 * 1.5
        [((10.5, 10.5, 30.5, 30.5), 3), ((10.5, 10.5, 30.5, 30.5), 4)],
    ])
