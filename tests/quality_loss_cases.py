"""Inputs of the quality-loss tests (numpy only; tests/test_quality_loss_cpu.py proves what each case holds).

A case is a dict of read-only arrays: logits [B, L, C] f32, labels [B, L] int64 (0 = background), reg_pred / reg_target [B, L, 4]
f32 LTRB distances (target -1 on negatives, as the assigners write it), gscale [B] f32.

random cases    C in {1, 3, 6, 20, 80, 81} (rows read in 16-, 8- and 4-byte pieces), L in {1, 255, 257, 341, 502} (one wave tile is
                64 locations, one reduction chunk CHUNK_LOCATIONS = 256: 257, 341 and 502 sum several partials), B in {1, 3}.
                Logits uniform in [-30, 30].  With B = 3, image 1 has no positive and in image 2 every location is positive.
                From L >= 32 on, image 0 holds the planted locations of PLANTED and rows pinned at 0, +-90, +-200.
long            L = 16 500: more wave tiles than 4 x 64 chunks, so a chunk holds several tiles per wave
saturated       one image per pinned value and sign of the target, nothing else in it: per-image sums isolate each value
"""
import numpy as np

F = np.float32
CHUNK_LOCATIONS = 256
PINS = (0.0, 90.0, -90.0, 200.0, -200.0)
# planted locations of image 0 (L >= 32): index -> what it is
PLANTED = {"identical": 0, "disjoint": 1, "degenerate": 2, "label_above_C": 3, "negative_area": 4}
PIN_POS0, PIN_NEG0 = 5, 10           # rows 5..9: pinned and positive; rows 10..14: pinned and negative

RANDOM = {          # name: (seed, B, L, C)
    "b1_l1_c1": (1, 1, 1, 1),
    "b3_l255_c3": (2, 3, 255, 3),
    "b1_l257_c20": (3, 1, 257, 20),
    "b3_l341_c80": (4, 3, 341, 80),
    "b1_l502_c81": (5, 1, 502, 81),
    "b3_l502_c6": (6, 3, 502, 6),
    "b3_l341_c1": (7, 3, 341, 1),
    "b1_l255_c80": (8, 1, 255, 80),
}
EXTRA = ("long", "saturated")
ALL = tuple(RANDOM) + EXTRA
_CACHE = {}


def _random(seed, B, L, C):
    g = np.random.default_rng(1000 + seed)
    logits = g.uniform(-30, 30, (B, L, C)).astype(F)
    labels = np.where(g.random((B, L)) < 0.3, g.integers(1, C + 1, (B, L)), 0).astype(np.int64)
    labels[0, 0] = 1 + (seed % C)
    if B == 3:
        labels[1] = 0
        labels[2] = g.integers(1, C + 1, L)
    tgt = g.uniform(4, 60, (B, L, 4)).astype(F)
    pred = (tgt * np.exp(0.3 * g.standard_normal((B, L, 4)))).astype(F)
    if L >= 32:
        P = PLANTED
        labels[0, :15] = g.integers(1, C + 1, 15)
        pred[0, P["identical"]] = tgt[0, P["identical"]]
        pred[0, P["disjoint"]], tgt[0, P["disjoint"]] = (-10, 5, 20, 5), (20, 5, -10, 5)          # side by side: no overlap, both areas 100
        pred[0, P["degenerate"]] = tgt[0, P["degenerate"]] = 0                                      # 0 / 0
        labels[0, P["label_above_C"]] = C + 3
        pred[0, P["negative_area"]], tgt[0, P["negative_area"]] = (-10, 5, 4, 5), (3, 3, 3, 3)      # a1 = -60: U = -24, iou = -0
        for k, v in enumerate(PINS):
            logits[0, PIN_POS0 + k] = v
            logits[0, PIN_NEG0 + k] = v
            labels[0, PIN_NEG0 + k] = 0
    tgt[labels <= 0] = -1
    gscale = g.uniform(0.25, 1.5, B).astype(F)
    return dict(logits=logits, labels=labels, reg_pred=pred, reg_target=tgt, gscale=gscale)


def _long():
    c = _random(99, 1, 16500, 4)
    return c


def _saturated():
    """Image 2k: every logit PINS[k], no positive; image 2k + 1: every logit PINS[k], every location positive, q in (0, 1)."""
    g = np.random.default_rng(77)
    B, L, C = 2 * len(PINS), 4, 3
    logits = np.repeat(np.array(PINS, F), 2)[:, None, None] * np.ones((B, L, C), F)
    labels = np.zeros((B, L), np.int64)
    labels[1::2] = g.integers(1, C + 1, (len(PINS), L))
    tgt = g.uniform(4, 60, (B, L, 4)).astype(F)
    pred = (tgt * np.exp(0.3 * g.standard_normal((B, L, 4)))).astype(F)
    tgt[labels <= 0] = -1
    return dict(logits=logits.astype(F), labels=labels, reg_pred=pred, reg_target=tgt, gscale=np.ones(B, F))


def get(name):
    if name not in _CACHE:
        c = _random(*RANDOM[name]) if name in RANDOM else {"long": _long, "saturated": _saturated}[name]()
        for v in c.values():
            v.setflags(write=False)
        _CACHE[name] = c
    return _CACHE[name]
