"""Designed inputs for the post-processing kernels of csrc/fd_postproc.hip (decode, top-k, batched NMS): the decisions
those kernels are made of -- which sigmoid is the first maximal one, which key is the K-th, which box suppresses which --
are hit by construction instead of by chance.  Plain numpy builders, shared by test_postproc_edges_cpu.py (which checks
that the tables are what they claim and runs the oracle over them) and test_postproc_edges_gpu.py (the kernels).

Out of scope: NaN scores or boxes into NMS (the kernel's contract is score-descending rows, and FCOSHead.post_process
rejects NaN scores before it gets there); in top-k, -0.0 against +0.0 and negative NaN (the decode kernel produces
neither: its scores are sqrt of a product of two sigmoids)."""
import numpy as np

B = 3

# ---------------------------------------------------------------------------------------------------- decode
PYR = ((24, 20), (3, 5), (2, 3), (1, 1))        # 502 locations: 31 full 16-location waves + a tail of 6; the last two waves straddle level boundaries
STRIDES = (8, 16, 32, 64)
DEC_L = sum(h * w for h, w in PYR)
DEC_CS_COALESCED = (4, 8, 12, 20, 80, 256)     # C % 4 == 0 and C <= 256: decode_coalesced_kernel on an aligned view; 4, 8, 12 leave quarters of the row empty
DEC_CS_PLAIN = (260, 21)                       # decode_kernel only (C > 256: its float4 form on an aligned view; 21: scalar)
NEAR_L = (-100.0, -95.0, -88.72, -88.5, -87.5, -60.0, -20.0, -5.0, 0.0, 3.0, 8.0, 12.0, 15.0, 16.5, 17.0, 30.0, 79.5, 80.0, 81.0, 100.0)
NEAR_D = (0, 1, 2, 4, 16, 256)
NEAR_PLACES = ("same_lower", "same_higher", "other_lower", "other_higher")     # runner-up: same / another quarter of the row, below / above L's index
KINDS = ("random", "near", "saturated", "underflow", "denormal", "tie_all", "neg_inf", "pos_inf", "nan_all", "nan_some")
GAP = 1e-3                                     # a random row is decidable when its runner-up logit is at least this far below the maximum
CNT_SPECIAL = (100.0, -100.0, 0.0)


def part_of(c, C):
    """The quarter (lane `part` of decode_coalesced_kernel) that scans class c of a row of C classes: quads
    [part * Q / 4, (part + 1) * Q / 4) of Q = C / 4.  For C % 4 != 0 (plain kernel only) just the quarter of the row."""
    if C % 4:
        return min(3, 4 * c // C)
    Q, q = C // 4, c // 4
    return next(p for p in range(4) if p * Q // 4 <= q < (p + 1) * Q // 4)


def ulps_below(x, d):
    v = np.float32(x)
    for _ in range(d):
        v = np.nextafter(v, np.float32(-np.inf))
    return v


def near_pair(C, place, k):
    """-> (index of L, index of the runner-up) for the k-th near-tie row."""
    parts = {}
    for c in range(C):
        parts.setdefault(part_of(c, C), []).append(c)
    keys = sorted(parts)
    kind, side = place.split("_")
    if kind == "other" and len(keys) > 1:
        j = k % (len(keys) - 1)
        lo_part, hi_part = parts[keys[j]], parts[keys[j + 1 + (k // 7) % (len(keys) - 1 - j)]]
        a, b = lo_part[k % len(lo_part)], hi_part[(3 * k) % len(hi_part)]
        return (b, a) if side == "lower" else (a, b)
    same = parts[keys[k % len(keys)]]            # (C = 4 has one non-empty quarter: 'other' falls back to it)
    pos = 1 + k % (len(same) - 2)
    return same[pos], same[pos - 1 if side == "lower" else pos + 1]


def _designed_rows(C, rng):
    """-> list of (kind, row [C] float32, decidable, expected class or 0 where only the oracle says)."""
    rows = []
    k = 0
    for L in NEAR_L:
        for d in NEAR_D:
            for place in NEAR_PLACES:
                iL, iR = near_pair(C, place, k)
                row = np.full(C, np.float32(L) - np.float32(30.0), np.float32)
                row[iL], row[iR] = np.float32(L), ulps_below(L, d)
                rows.append(("near", row, d == 0, 0))
                k += 1
    # saturation: several classes whose sigmoid is exactly 1.0f, in every quarter, the largest logit not first
    sat = sorted({min(C - 1, 1 + j * max(1, C // 4)) for j in range(4)})
    for others in ("random", 12.0):
        row = rng.uniform(-5, 5, C).astype(np.float32) if others == "random" else np.full(C, others, np.float32)
        row[sat] = np.float32([17.5, 25.0, 60.0, 18.0])[:len(sat)]
        rows.append(("saturated", row, True, sat[0] + 1))
    # underflow: every sigmoid is exactly 0, the largest logit not at index 0
    row = np.full(C, -95.0, np.float32); row[min(5, C - 1)] = -90.0
    rows.append(("underflow", row, True, 1))
    row = np.full(C, -120.0, np.float32); row[C - 1] = -89.0
    rows.append(("underflow", row, True, 1))
    row = rng.uniform(-140, -89.5, C).astype(np.float32); row[C // 2] = -89.0
    rows.append(("underflow", row, True, 1))
    # every sigmoid denormal (or zero where the device flushes): device against device only
    for lo, hi in ((-88.7, -87.4), (-88.7, -88.0)):
        row = rng.uniform(lo, hi, C).astype(np.float32); row[0] = lo
        rows.append(("denormal", row, False, 0))
    for v in (0.0, -4.6, 20.0):
        rows.append(("tie_all", np.full(C, v, np.float32), True, 1))
    rows.append(("neg_inf", np.full(C, -np.inf, np.float32), True, 1))
    row = rng.uniform(-5, 5, C).astype(np.float32); row[C - 2] = np.inf
    rows.append(("pos_inf", row, True, C - 1))
    rows.append(("nan_all", np.full(C, np.nan, np.float32), False, 0))
    row = (rng.standard_normal(C) * 2 - 3).astype(np.float32); row[0] = np.nan
    rows.append(("nan_some", row, False, 0))
    row = (rng.standard_normal(C) * 2 - 3).astype(np.float32); row[[c for c in range(C) if part_of(c, C) == part_of(C - 1, C)]] = np.nan
    row[0] = 1.0
    rows.append(("nan_some", row, False, 0))
    row = np.full(C, np.nan, np.float32); row[C - 1] = -2.0
    rows.append(("nan_some", row, False, 0))
    return rows


_DEC = {}


def decode_case(C):
    """-> dict: cls [3, 502, C], cnt [3, 502, 1], reg [3, 502, 4] (levels concatenated per image, the oracle's layout),
    kind [3, 502] (index into KINDS), decidable [3, 502], expect [3, 502] (class, 0 = ask the oracle), nan [3, 502].
    The designed rows are spread evenly over the 1506 (location, image) slots, so every wave holds some, the tail wave and
    the waves across level boundaries included; the rest is randn * 2 - 3."""
    if C in _DEC:
        return _DEC[C]
    rng = np.random.default_rng(4000 + C)
    cls = (rng.standard_normal((B, DEC_L, C)) * 2 - 3).astype(np.float32)
    cnt = rng.standard_normal((B, DEC_L, 1)).astype(np.float32)
    reg = (np.exp(rng.standard_normal((B, DEC_L, 4))) * 16).astype(np.float32)
    kind = np.zeros((B, DEC_L), np.int8)
    expect = np.zeros((B, DEC_L), np.int32)
    top2 = np.sort(cls.astype(np.float64), axis=2)[:, :, -2:]
    decidable = (top2[:, :, 1] - top2[:, :, 0]) >= GAP          # derived from the logits alone
    rows = _designed_rows(C, rng)
    assert len(rows) <= B * DEC_L
    for k, (kd, row, dec, exp) in enumerate(rows):
        loc, b = divmod((k * B * DEC_L) // len(rows), B)
        cls[b, loc], kind[b, loc], decidable[b, loc], expect[b, loc] = row, KINDS.index(kd), dec, exp
        if k % 5 < 3:
            cnt[b, loc, 0] = CNT_SPECIAL[k % 5]
    out = dict(cls=cls, cnt=cnt, reg=reg, kind=kind, decidable=decidable, expect=expect, nan=np.isnan(cls).any(2))
    for a in out.values():
        a.setflags(write=False)
    _DEC[C] = out
    return out


def sigmoid32(x):
    """fp32 1 / (1 + exp(-x)), the form of the oracle and of fd_sigmoid."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))).astype(np.float32)


def ulp_distance(a, b):
    """Number of float32 values between two non-negative floats."""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


# ---------------------------------------------------------------------------------------------------- top-k
TOPK_MAXE_L = 24 * 1024                          # the last L of topk_kernel<true> (keys in registers); above it topk_kernel<false> re-reads the scores
TOPK_SIZES = tuple((L, K) for L in (24575, 24576, 24577, 30000) for K in (1, 1000, 1024)) + ((30000, 3000),) \
    + tuple((L, min(L, 1000)) for L in (1023, 1024, 1025, 2047, 2049))
TOPK_LOWBITS = tuple((L, K) for L in (1000, 5000, 30000) for K in (1, 999, 1000))
TOPK_OTHER = (("negative", 5000, 1000), ("negative", 30000, 1024), ("mixed", 5000, 1000), ("mixed", 30000, 1000),
              ("equal", 2049, 1000), ("equal", 30000, 1000), ("equal", 30000, 1), ("ties", 1024, 1024),
              ("same_round", 30000, 1000), ("same_round", 24576, 1000))
TOPK_NAN = ((5000, 1000), (30000, 1000), (30000, 3000), (1024, 1024))
TOPK_KINDS = ("ties", "lowbits", "negative", "mixed", "equal", "nan", "same_round")
QNAN = np.uint32(0x7FC00000)                     # the positive quiet NaN
LOWBITS_BASE = np.float32(0.25)


def order_key(s):
    """fd_order_key: float32 -> uint32 whose unsigned order is the float order (a positive NaN above +inf)."""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk_by_key(scores, K):
    """Indices of the K largest keys per row, descending, ties by lower index -> [B, K] int32."""
    return np.stack([np.argsort(~order_key(row), kind="stable")[:K] for row in scores]).astype(np.int32)


def _tie_recipe(rng, L):
    scores = rng.uniform(0, 1, (B, L)).astype(np.float32)
    scores[:, rng.integers(0, L, L // 3)] = np.float32(0.25)     # heavy ties, also straddling the K-th value
    scores[1] = np.round(scores[1] * 8) / 8                      # very few distinct values
    return scores


def topk_case(kind, L, K):
    """-> scores [3, L] f32, classes [3, L] i32, boxes [3, L, 4] f32."""
    rng = np.random.default_rng(100000 * TOPK_KINDS.index(kind) + 3 * L + K)
    if kind == "ties":
        scores = _tie_recipe(rng, L)
    elif kind == "lowbits":              # keys differ only below bit 15: the first radix digit (and the second for L <= 1024) is shared by every element
        base = LOWBITS_BASE.view(np.uint32)
        scores = np.stack([(base + rng.permutation(L).astype(np.uint32)).view(np.float32) for _ in range(B)])
    elif kind == "negative":
        scores = -_tie_recipe(rng, L)
        scores[1] = np.minimum(scores[1], np.float32(-0.125))       # (no -0.0)
    elif kind == "mixed":
        scores = _tie_recipe(rng, L) * 2 - 1
        scores[:, rng.integers(0, L, L // 5)] = np.float32(-0.25)
        scores[1] = np.round(scores[1] * 8) / 8 + np.float32(0.0)   # -0.0 + 0.0 = +0.0
        neg = np.arange(L) % 37 != 0                                # image 2: fewer positive scores than K, the K-th key is a negative one
        scores[2, neg] = -np.abs(scores[2, neg])
        scores = scores + np.float32(0.0)
    elif kind == "equal":
        scores = np.empty((B, L), np.float32)
        scores[0], scores[1], scores[2] = 0.25, -1.5, 0.0
    elif kind == "same_round":
        # the compaction walks the scores 1024 at a time: here the K-th value's 30 ties (all needed) and one larger score sit
        # together in the LAST round, every other larger score in an earlier one -- the round's ties fill the last 30 slots of the
        # candidate list while a strictly larger key is appended in the same round
        e0 = (L - 1) // 1024 * 1024
        assert L - e0 >= 300 and K >= 64
        scores = np.full((B, L), 0.1, np.float32)
        for b in range(B):
            scores[b, rng.choice(e0, K - 31, replace=False)] = (0.6 + 0.2 * rng.permutation(K - 31) / K).astype(np.float32)
        scores[0, e0:e0 + 30], scores[0, L - 1] = 0.5, 0.9             # ties in the round's first wave, the larger score in its last
        scores[1, L - 30:], scores[1, e0] = 0.5, 0.9                   # the other way round
        scores[2, e0:e0 + 270:9], scores[2, e0 + 100] = 0.5, 0.9       # ties spread over the round's waves
    elif kind == "nan":
        scores = _tie_recipe(rng, L)
        for b, n in ((0, 3), (2, min(L // 2, K + 5))):              # fewer NaNs than K; more NaNs than K (the K-th key is the NaN's)
            scores[b].view(np.uint32)[rng.choice(L, n, replace=False)] = QNAN
        scores[0].view(np.uint32)[L - 1] = QNAN
    else:
        raise KeyError(kind)
    classes = rng.integers(1, 81, (B, L)).astype(np.int32)
    boxes = rng.uniform(0, 640, (B, L, 4)).astype(np.float32)
    return np.ascontiguousarray(scores, np.float32), classes, boxes


# ---------------------------------------------------------------------------------------------------- NMS
SCORE_THR = 0.05
CHAIN_NS = (31, 32, 33, 63, 64, 65, 127, 129, 1023, 1024)        # rows 31/32, 63/64 and 1023/1024: the two halves of the in-block scan, the carry into later words
CHAIN_NS_LARGE = (1025, 1100)
CHAIN_FORMS = ("next", "next2", "behind30")
CHAIN_PREFIX = 30


def _desc_scores(n, hi=0.95, lo=0.10):
    s = np.linspace(hi, lo, n).astype(np.float32)
    assert n < 2 or (s[1:] < s[:-1]).all()
    return s


def chain_case(form, n):
    """n unit-height boxes of one class, 10 wide.  'next': shifted by 3, box i overlaps only box i + 1 above 0.5 (IoU 7/13;
    4/16 with i + 2).  'next2': shifted by 2 with threshold 0.4, box i overlaps i + 1 and i + 2 (8/12, 6/14; 4/16 with i + 3).
    'behind30': the 'next' chain in rows 30 .. 30 + n - 1 behind 30 unrelated boxes with higher scores.
    -> dict(boxes, scores, classes, iou_thr, chain = slice of the chain's rows)."""
    shift, thr = (2, 0.4) if form == "next2" else (3, 0.5)
    x = np.arange(n, dtype=np.float32) * shift
    boxes = np.stack([x, np.zeros(n, np.float32), x + 10, np.ones(n, np.float32)], 1)
    chain = slice(0, n)
    if form == "behind30":
        y = 1000 + 50 * np.arange(CHAIN_PREFIX, dtype=np.float32)
        pre = np.stack([np.zeros(CHAIN_PREFIX, np.float32), y, np.full(CHAIN_PREFIX, 40, np.float32), y + 20], 1)
        boxes = np.concatenate([pre, boxes])
        chain = slice(CHAIN_PREFIX, CHAIN_PREFIX + n)
    m = len(boxes)
    return dict(boxes=boxes, scores=_desc_scores(m), classes=np.ones(m, np.int64), iou_thr=thr, chain=chain)


def iou_plain(a, b):
    """float64 IoU of two xyxy boxes (the table's own check, not the kernel's arithmetic)."""
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0])); h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _set(boxes, classes, iou_thr=0.5, scores=None, **flags):
    boxes = np.asarray(boxes, np.float32)
    return dict(boxes=boxes, scores=_desc_scores(len(boxes)) if scores is None else np.asarray(scores, np.float32),
                classes=np.asarray(classes, np.int64), iou_thr=iou_thr, **flags)


def degenerate_cases():
    """name -> dict(boxes, scores, classes, iou_thr[, must_keep = rows that have to survive, all_kept])."""
    pair = [[200, 200, 230, 230], [201, 201, 231, 231]]              # an ordinary overlapping pair (IoU 0.88): its second box goes
    d = {}
    d["zero_area_dups"] = _set([[5, 5, 5, 5]] * 4 + [[7, 7, 7, 7]] * 2 + pair, [1] * 8, must_keep=list(range(6)))       # 0 / 0 = NaN suppresses nothing
    d["zero_width"] = _set([[5, 0, 5, 10]] * 3 + [[0, 0, 10, 10]] + pair + [[5, 0, 5, 10]], [1] * 7, must_keep=[0, 1, 2, 3, 6])
    d["inverted"] = _set([[10, 0, 0, 10], [10, 0, 0, 10], [0, 0, 10, 10], [10, 10, 0, 0], [10, 10, 0, 0], [15, 0, 0, 10]] + pair, [1] * 8,
                         must_keep=[0, 1, 2, 3, 4, 5])
    d["dups_distinct_scores"] = _set([[10, 10, 50, 60]] * 4 + [[300, 300, 340, 360]] * 3, [2] * 7)
    d["dups_equal_scores"] = _set([[10, 10, 50, 60]] * 4 + [[300, 300, 340, 360]] * 3, [2] * 7, scores=[0.5] * 7)
    d["max_is_minus_one"] = _set([[-11, -11, -1, -1], [-11, -11, -1, -1], [-30, -30, -20, -20], [-12, -12, -2, -2], [-30, -30, -20, -20]],
                                 [1, 2, 3, 4, 1])                     # max + 1 == 0: every class offset is 0, classes collide
    d["all_below_minus_one"] = _set([[-50, -50, -5, -5], [-50, -50, -5, -5], [-50, -50, -5, -5], [-49, -49, -6, -6], [-40, -40, -10, -10],
                                     [-50, -50, -5, -5], [-20, -20, -8, -8]], [1, 1, 2, 3, 7, 2, 1])      # max + 1 == -4: negative offsets
    big = np.float32(1e6)
    bb = [[big + a, big + a, big + a + w, big + a + w] for a, w in ((0, 10), (3, 10), (0, 10), (40, 10), (41, 10), (0, 10), (3, 10), (100, 3))]
    d["coords_1e6_classes_80"] = _set(bb, [80, 80, 0, 79, 79, 0, 0, 80])    # 80 * (1e6 + 1) ~ 8e7, ulp 8: the boxes collapse after the offset
    d["classes_0_and_1"] = _set([[10, 10, 50, 60], [11, 11, 51, 61], [10, 10, 50, 60], [11, 11, 51, 61], [12, 12, 52, 62]], [0, 1, 1, 0, 0])
    return d


def threshold_cases():
    thr = np.float32(SCORE_THR)
    far = [[100 * i, 0, 100 * i + 50, 50] for i in range(5)]
    d = {}
    d["score_at_threshold"] = _set(far, [1] * 5, scores=[0.9, 0.5, thr, thr, np.nextafter(thr, np.float32(0))], n_kept=4)    # >= keeps, the next float below drops
    over = [[0, 0, 10, 10], [9, 9, 20, 20], [10, 10, 30, 30], [0, 0, 10, 10], [40, 40, 50, 50], [50, 40, 60, 50]]
    d["iou_thr_0"] = _set(over, [1] * 6, iou_thr=0.0)                # any overlap suppresses, touching boxes (intersection 0) do not
    d["iou_thr_1"] = _set(over, [1] * 6, iou_thr=1.0, all_kept=True)      # an exact duplicate has IoU 1.0, not > 1.0
    return d


PREFIXES = (0, 1, 64, 65)
PREFIX_K = 200


def prefix_case(p):
    """K = 200 'next2' chain rows (integer boxes) of which the first p pass the score threshold."""
    c = chain_case("next2", PREFIX_K)
    c["scores"] = np.concatenate([_desc_scores(p), np.full(PREFIX_K - p, 0.01, np.float32)]).astype(np.float32)
    return c


def plus1_chain(n=PREFIX_K):
    """Integer boxes for DataEncoder._box_nms ("+1" areas): 10 x 4 pixels shifted by 3, 7/15 with the next box above 0.45."""
    x = np.arange(n, dtype=np.float32) * 3
    boxes = np.stack([x, np.zeros(n, np.float32), x + 9, np.full(n, 3, np.float32)], 1)
    return boxes, _desc_scores(n)


def pad_case(c, K):
    """Rows of a case padded to K with scores below the threshold and boxes that would suppress everything if they were read."""
    n = len(c["scores"])
    assert n <= K
    scores = np.concatenate([c["scores"], np.full(K - n, 0.01, np.float32)]).astype(np.float32)
    classes = np.concatenate([c["classes"], np.ones(K - n, np.int64)])
    boxes = np.concatenate([c["boxes"], np.tile(np.float32([[-1e7, -1e7, 1e7, 1e7]]), (K - n, 1))]).astype(np.float32)
    return scores, classes, boxes
