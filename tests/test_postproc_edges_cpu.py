"""The designed inputs of tests/postproc_edge_cases.py are what they claim to be, and the oracle (oracle/postproc_ref.c)
decides them the way test_postproc_edges_gpu.py expects.  Runs without a GPU."""
import numpy as np
import pytest

import postproc_edge_cases as E
from oracle import torch_ref as R


def _coords():
    return np.concatenate([R.coords_fcos(h, w, s) for (h, w), s in zip(E.PYR, E.STRIDES)], 0)


# ---------------------------------------------------------------------------------------------------- decode
def test_decode_pyramid_shape():
    assert E.DEC_L == 502 and E.DEC_L % 16 == 6
    level = np.repeat(np.arange(len(E.PYR)), [h * w for h, w in E.PYR])
    levels_of_wave = [len(set(level[w:w + 16].tolist())) for w in range(0, E.DEC_L, 16)]
    assert levels_of_wave == [1] * 30 + [2, 2]      # the waves of locations 480..495 and 496..501 read rows of two levels


@pytest.mark.parametrize("C", [4, 8, 12, 20, 80, 256])
def test_near_tie_placements_cover_the_quarters(C):
    """The runner-up sits below and above L's index, in L's quarter of the row and (where C has more than one non-empty
    quarter) in another one."""
    seen = set()
    for k in range(len(E.NEAR_L) * len(E.NEAR_D) * 4):
        place = E.NEAR_PLACES[k % 4]
        iL, iR = E.near_pair(C, place, k)
        assert iL != iR and 0 <= iL < C and 0 <= iR < C
        same = E.part_of(iL, C) == E.part_of(iR, C)
        assert (iR < iL) == place.endswith("lower")
        assert same == (place.startswith("same") or C == 4)
        seen.add((E.part_of(iL, C), E.part_of(iR, C)))
    nonempty = {E.part_of(c, C) for c in range(C)}
    assert {p for p, _ in seen} == nonempty and {p for _, p in seen} == nonempty


@pytest.mark.parametrize("C", E.DEC_CS_COALESCED + E.DEC_CS_PLAIN)
def test_decode_table_and_oracle(C):
    """Every kind of row is present in every image-independent sense the GPU test relies on; on the rows the table calls
    decidable the oracle's winning sigmoid is bit-equal to the best other one (a tie: the first index wins in any
    implementation) or at least 16 ulp above it (far more than two expf can differ); the classes the table states are the
    oracle's."""
    d = E.decode_case(C)
    kind, dec = d["kind"], d["decidable"]
    for name in E.KINDS:
        assert (kind == E.KINDS.index(name)).any(), name
    assert (kind == E.KINDS.index("near")).sum() == len(E.NEAR_L) * len(E.NEAR_D) * 4
    assert (kind[:, 480:] != 0).any() and (kind[:, 496:] != 0).any()          # designed rows in the level-straddling wave and in the tail
    assert not dec[d["nan"]].any()
    assert dec[kind == 0].mean() > 0.95                                        # the random rows are almost all decidable
    for v in E.CNT_SPECIAL:
        assert (d["cnt"] == v).any()
    es, ec, eb = R.decode(d["cls"], d["cnt"], d["reg"], _coords())
    sig = E.sigmoid32(d["cls"])
    win = np.take_along_axis(sig, (ec - 1)[..., None].astype(np.int64), 2)[..., 0]
    rest = sig.copy()
    np.put_along_axis(rest, (ec - 1)[..., None].astype(np.int64), np.float32(-1), 2)
    other = rest.max(2)
    gap = E.ulp_distance(win, np.maximum(other, 0))
    bad = dec & ~((win == other) | ((win > other) & (gap >= 16)))
    assert not bad.any(), [(int(b), int(l), E.KINDS[kind[b, l]], float(win[b, l]), float(other[b, l])) for b, l in np.argwhere(bad)[:5]]
    stated = d["expect"] > 0
    assert stated.sum() >= 9
    np.testing.assert_array_equal(ec[stated], d["expect"][stated])
    # what the kinds claim, in the oracle's own arithmetic
    assert (sig[kind == E.KINDS.index("underflow")] == 0).all()
    sat = kind == E.KINDS.index("saturated")
    assert ((sig[sat] == 1).sum(1) >= 3).all() and (d["cls"][sat].argmax(1) + 1 != ec[sat]).all()     # the largest logit is not the first saturated one
    assert (d["cls"][kind == E.KINDS.index("underflow")].argmax(1) != 0).all()
    den = sig[kind == E.KINDS.index("denormal")]
    assert (den < np.finfo(np.float32).tiny).all()
    assert np.isfinite(es[~d["nan"]]).all() and np.isfinite(eb).all()


def test_issue_example_row():
    """A row of -95 with one -90 at index 5: the first index wins (all sigmoids are 0), not the argmax of the logits."""
    cls = np.full((1, 1, 8), -95.0, np.float32); cls[0, 0, 5] = -90.0
    _, ec, _ = R.decode(cls, np.zeros((1, 1, 1), np.float32), np.ones((1, 1, 4), np.float32), np.zeros((1, 2), np.float32))
    assert int(ec[0, 0]) == 1 and int(cls.argmax()) == 5


# ---------------------------------------------------------------------------------------------------- top-k
def _all_topk_cases():
    return [("ties", L, K) for L, K in E.TOPK_SIZES] + [("lowbits", L, K) for L, K in E.TOPK_LOWBITS] + list(E.TOPK_OTHER) \
        + [("nan", L, K) for L, K in E.TOPK_NAN]


def test_topk_sizes_reach_every_kernel():
    ls = {L for L, K in E.TOPK_SIZES if K <= 1024}
    assert E.TOPK_MAXE_L in ls and E.TOPK_MAXE_L + 1 in ls and E.TOPK_MAXE_L - 1 in ls and max(ls) == 30000
    assert any(K > 1024 and L > E.TOPK_MAXE_L for L, K in E.TOPK_SIZES)
    assert all(1 <= K <= L for _, L, K in _all_topk_cases())


@pytest.mark.parametrize("kind,L,K", [c for c in _all_topk_cases() if c[0] != "nan"])
def test_topk_numpy_key_order_is_the_oracles(kind, L, K):
    """order_key / topk_by_key (the expectation of the NaN cases) agree with the oracle's stable sort wherever it is defined,
    and no case holds a -0.0 or, outside the NaN cases, a NaN."""
    scores, classes, boxes = E.topk_case(kind, L, K)
    assert scores.shape == (E.B, L) and not np.isnan(scores).any()
    assert not (np.signbit(scores) & (scores == 0)).any()
    np.testing.assert_array_equal(E.topk_by_key(scores, K), R.topk(scores, K))
    if kind == "lowbits":
        key = E.order_key(scores)
        assert (np.sort(key, 1) == np.sort(key, 1)[0]).all() and len(np.unique(key[0])) == L      # distinct keys, the same set in every image
        assert len(np.unique(key >> 21)) == 1 and (len(np.unique((key >> 10) & 2047)) == 1) == (L <= 1024)
        assert len(np.unique(key & 1023)) == min(L, 1024)
    if kind in ("negative", "mixed"):
        assert (scores < 0).any() and ((scores > 0).any() == (kind == "mixed"))
        kth = np.take_along_axis(scores, R.topk(scores, K)[:, -1:].astype(np.int64), 1)
        assert (kth < 0).any()                                                                  # the K-th key itself comes from fd_order_key's negative branch
    if kind == "same_round":
        e0 = (L - 1) // 1024 * 1024
        assert ((scores >= 0.5).sum(1) == K).all() and ((scores == 0.5).sum(1) == 30).all()      # exactly K candidates, the 30 ties all needed
        for b in range(E.B):
            last = np.flatnonzero(scores[b, e0:] >= 0.5)
            assert len(last) == 31 and (scores[b, e0:][last] > 0.5).sum() == 1                   # the ties and one larger score share the last round
        assert {int(np.argmax(scores[b, e0:])) // 64 for b in range(E.B)} == {0, 1, (L - 1 - e0) // 64}
    if kind == "ties":
        kth = np.take_along_axis(scores, R.topk(scores, K)[:, -1:].astype(np.int64), 1)
        assert ((scores == kth).sum(1) > 1).any() or K == 1 or K == L


@pytest.mark.parametrize("L,K", E.TOPK_NAN)
def test_topk_nan_cases(L, K):
    scores, _, _ = E.topk_case("nan", L, K)
    nan = np.isnan(scores)
    assert (scores.view(np.uint32)[nan] == E.QNAN).all()
    assert 0 < nan[0].sum() < K and nan[1].sum() == 0 and (nan[2].sum() > K or nan[2].sum() == L // 2)
    idx = E.topk_by_key(scores, K)
    for b in range(E.B):
        n = min(int(nan[b].sum()), K)
        np.testing.assert_array_equal(idx[b, :n], np.flatnonzero(nan[b])[:n])      # NaNs first, lower index first
        rest = np.take(scores[b], idx[b, n:])
        assert (rest[:-1] >= rest[1:]).all()
    np.testing.assert_array_equal(idx, R.topk(np.where(nan, np.float32(2.0), scores), K))     # a NaN sorts like a value above every score


# ---------------------------------------------------------------------------------------------------- NMS
def _oracle_keep(c, K=None):
    s, cl, b = (c["scores"], c["classes"], c["boxes"]) if K is None else E.pad_case(c, K)
    return R.post_process(s[None], cl[None], b[None], E.SCORE_THR, c["iou_thr"])[0]


@pytest.mark.parametrize("n", E.CHAIN_NS + E.CHAIN_NS_LARGE)
@pytest.mark.parametrize("form", E.CHAIN_FORMS)
def test_chain_tables(form, n):
    """The overlaps are the stated ones; the oracle keeps every other box of a chain (between 40 % and 60 %).  A chain whose
    boxes each overlap the next TWO cannot keep more than one box in three: the bound there is 30 % .. 37 %."""
    c = E.chain_case(form, n)
    ch = c["boxes"][c["chain"]]
    reach = 2 if form == "next2" else 1
    for i in (0, 1, n // 2, n - 4):
        for j in range(1, 4):
            assert (E.iou_plain(ch[i], ch[i + j]) > c["iou_thr"]) == (j <= reach), (i, j)
    assert abs(E.iou_plain(ch[0], ch[1]) - (8 / 12 if form == "next2" else 7 / 13)) < 1e-12
    assert (c["scores"][1:] < c["scores"][:-1]).all() and c["scores"].min() >= 0.1 > E.SCORE_THR
    keep = _oracle_keep(c)
    lo = c["chain"].start
    kept_chain = keep[keep >= lo] - lo
    np.testing.assert_array_equal(keep[:lo], np.arange(lo))                        # the unrelated boxes in front all stay
    np.testing.assert_array_equal(kept_chain, np.arange(0, n, reach + 1))
    share = len(kept_chain) / n
    assert (0.30 <= share <= 0.37) if form == "next2" else (0.40 <= share <= 0.60)
    np.testing.assert_array_equal(_oracle_keep(c, max(1100, len(c["scores"]))), keep)     # padding below the score threshold changes nothing


@pytest.mark.parametrize("name", sorted(E.degenerate_cases()) + sorted(E.threshold_cases()))
def test_degenerate_and_threshold_tables(name):
    c = {**E.degenerate_cases(), **E.threshold_cases()}[name]
    n = len(c["scores"])
    assert (c["scores"][1:] <= c["scores"][:-1]).all()
    keep = _oracle_keep(c)
    np.testing.assert_array_equal(keep, R.batched_nms(c["boxes"], c["scores"], c["classes"], c["iou_thr"])[:len(keep)])
    assert len(keep) >= 1
    if c.get("all_kept"):
        assert len(keep) == n
    elif "n_kept" in c:
        assert len(keep) == c["n_kept"] < n
    else:
        assert len(keep) < n                                                          # something is suppressed
    assert set(c.get("must_keep", ())) <= set(keep.tolist())
    np.testing.assert_array_equal(_oracle_keep(c, 1100), keep)


def test_degenerate_geometry_is_what_it_claims():
    d = E.degenerate_cases()
    b = d["zero_area_dups"]["boxes"]
    assert ((b[:6, 2] - b[:6, 0]) * (b[:6, 3] - b[:6, 1]) == 0).all()
    b = d["inverted"]["boxes"]
    assert (b[[0, 1, 3, 4, 5], 2] < b[[0, 1, 3, 4, 5], 0]).all()
    assert d["max_is_minus_one"]["boxes"].max() == -1
    assert d["all_below_minus_one"]["boxes"].max() < -1
    c = d["coords_1e6_classes_80"]
    off = np.float32(80) * (c["boxes"].max() + np.float32(1))
    moved = c["boxes"][0] + off
    assert moved[2] - moved[0] != c["boxes"][0][2] - c["boxes"][0][0]                 # the offset eats the box's mantissa: its width changes
    assert set(d["classes_0_and_1"]["classes"].tolist()) == {0, 1}
    # classes collide only where the offset is 0: the same rows with max > -1 keep the cross-class duplicate
    m = d["max_is_minus_one"]
    assert 1 not in _oracle_keep(m)
    shifted = dict(m, boxes=m["boxes"] + np.float32(20))
    assert 1 in _oracle_keep(shifted)
    t = E.threshold_cases()["score_at_threshold"]["scores"]
    assert t[2] == np.float32(E.SCORE_THR) and t[4] < np.float32(E.SCORE_THR) and np.nextafter(t[4], np.float32(1)) == t[2]


@pytest.mark.parametrize("p", E.PREFIXES)
def test_prefix_tables(p):
    c = E.prefix_case(p)
    assert len(c["scores"]) == E.PREFIX_K and (c["scores"] >= E.SCORE_THR).sum() == p
    keep = _oracle_keep(c)
    np.testing.assert_array_equal(keep, np.arange(0, p, 3))
    boxes, scores = E.plus1_chain()
    assert (boxes == np.round(boxes)).all()
    for mode in ("union", "min"):
        k = R.box_nms_plus1(boxes[:p], scores[:p], 0.45, mode) if p else np.zeros(0, np.int32)
        assert (p == 0 and len(k) == 0) or 0 < len(k) <= p
        if p > 1:
            assert len(k) < p
