"""The post-processing kernels of csrc/fd_postproc.hip at their decision boundaries: the designed inputs of
tests/postproc_edge_cases.py (test_postproc_edges_cpu.py checks the tables) through decode, top-k and batched NMS.
decode_coalesced_kernel is held against decode_kernel on the same logits bit for bit (both evaluate the same fd_sigmoid:
no rounding excuse), and both against the oracle wherever host and device expf cannot disagree about the winner; top-k and
NMS are held bit for bit against the oracle's C restatement."""
import numpy as np
import pytest
import torch

import postproc_edge_cases as E
from oracle import torch_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import Segs
from pytorch_object_detection_amd.ops import Rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype else t).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------- decode
_COORDS = []


def _coords():
    if not _COORDS:
        _COORDS.append(np.concatenate([R.coords_fcos(h, w, s) for (h, w), s in zip(E.PYR, E.STRIDES)], 0))
    return _COORDS[0]


def _rows_view(flat, cs, co):
    """[3, 502, C] (the oracle's layout) -> the kernels' rows buffer (level-major, then image, then pixel) as a channel view
    at offset `co` of a [rows, cs] buffer that is NaN everywhere else."""
    C = flat.shape[2]
    buf = torch.full((E.B * E.DEC_L, cs), float("nan"), dtype=torch.float32)
    m = l0 = 0
    for h, w in E.PYR:
        hw = h * w
        buf[m:m + E.B * hw, co:co + C] = torch.from_numpy(flat[:, l0:l0 + hw].reshape(E.B * hw, C).copy())
        m, l0 = m + E.B * hw, l0 + hw
    return Rows(buf.to(DEV), co, C)


def _decode(d, aligned):
    C = d["cls"].shape[2]
    cls = _rows_view(d["cls"], (C + 7) // 4 * 4, 0) if aligned else _rows_view(d["cls"], C + 5, 1)
    cnt, reg = _rows_view(d["cnt"], 3, 1), _rows_view(d["reg"], 7, 2)
    s, c, b = ops.fcos_decode(cls, cnt, reg, Segs.make(E.B, list(E.PYR)), list(E.STRIDES))
    return s.cpu().numpy(), c.cpu().numpy(), b.cpu().numpy()


def _rows_msg(d, mask, got, other):
    """(kind, largest logit of the row) -> how many such rows differ, then the first of each: (image, location, got, other)."""
    seen = {}
    for b, l in np.argwhere(mask):
        with np.errstate(invalid="ignore"):
            key = (E.KINDS[d["kind"][b, l]], float(np.nanmax(d["cls"][b, l])) if not np.isnan(d["cls"][b, l]).all() else None)
        n, first = seen.get(key, (0, (int(b), int(l), int(got[b, l]), int(other[b, l]))))
        seen[key] = (n + 1, first)
    return sorted(seen.items(), key=str)


def _against_oracle(d, s, c, b):
    es, ec, eb = R.decode(d["cls"], d["cnt"], d["reg"], _coords())
    np.testing.assert_array_equal(b, eb)
    ok = ~d["nan"]
    np.testing.assert_allclose(s[ok], es[ok], rtol=2e-6, atol=1e-7)
    wrong = d["decidable"] & (c != ec)
    print("decidable rows", int(d["decidable"].sum()), "class differs from the oracle on", int(wrong.sum()),
          "| undecidable rows that differ", int((~d["decidable"] & ok & (c != ec)).sum()))
    assert not wrong.any(), _rows_msg(d, wrong, c, ec)
    stated = d["expect"] > 0
    np.testing.assert_array_equal(c[stated], d["expect"][stated])


@pytest.mark.parametrize("C", E.DEC_CS_COALESCED)
def test_decode_coalesced_equals_plain_kernel_and_oracle(C):
    """The same logits through decode_coalesced_kernel (aligned view) and decode_kernel (view at channel 1 of C + 5): scores,
    classes and boxes identical on every row, the NaN rows included (their scores are the same NaN); then both against the
    oracle -- boxes exact, scores within the tolerance of test_postproc_gpu.py, classes exact on every decidable row."""
    d = E.decode_case(C)
    s1, c1, b1 = _decode(d, aligned=True)
    s2, c2, b2 = _decode(d, aligned=False)
    diff = c1 != c2
    print("C", C, "classes differ between the two kernels on", int(diff.sum()), "rows")
    assert not diff.any(), _rows_msg(d, diff, c1, c2)
    sd = _bits(s1) != _bits(s2)
    assert not sd.any(), _rows_msg(d, sd, c1, c2)
    ok = ~d["nan"]
    assert torch.equal(torch.from_numpy(s1[ok]), torch.from_numpy(s2[ok])) and np.isnan(s1[d["kind"] == E.KINDS.index("nan_all")]).all()
    np.testing.assert_array_equal(b1, b2)
    assert (c1[d["kind"] == E.KINDS.index("nan_all")] == 1).all()                 # a row of NaNs: class 1 (torch.max over NaNs aside, the plain kernel's answer)
    _against_oracle(d, s1, c1, b1)
    _against_oracle(d, s2, c2, b2)


@pytest.mark.parametrize("C", E.DEC_CS_PLAIN)
def test_decode_plain_kernel_only(C):
    """C = 260 (> 256 classes: decode_kernel's float4 form on the aligned view, its scalar form on the other) and C = 21."""
    d = E.decode_case(C)
    s1, c1, b1 = _decode(d, aligned=True)
    s2, c2, b2 = _decode(d, aligned=False)
    np.testing.assert_array_equal(c1, c2)
    np.testing.assert_array_equal(_bits(s1), _bits(s2))
    np.testing.assert_array_equal(b1, b2)
    _against_oracle(d, s1, c1, b1)


# ---------------------------------------------------------------------------------------------------- top-k
def _check_topk(scores, classes, boxes, K, idx):
    ts, tc, tb, ti = ops.fcos_topk(_t(scores), _t(classes), _t(boxes), K, want_idx=True)
    np.testing.assert_array_equal(ti.cpu().numpy(), idx)
    for b in range(E.B):
        np.testing.assert_array_equal(_bits(ts[b]), _bits(scores[b][idx[b]]))
        np.testing.assert_array_equal(tc[b].cpu().numpy(), classes[b][idx[b]])
        np.testing.assert_array_equal(_bits(tb[b]), _bits(boxes[b][idx[b]]))


@pytest.mark.parametrize("L,K", E.TOPK_SIZES)
def test_topk_sizes_around_the_register_kernels_limit(L, K):
    """L = 24 576 is the last length of topk_kernel<true>; 24 577 and 30 000 run topk_kernel<false> (K <= 1024) and the
    K > 1024 kernel at a long L; 1023 .. 2049: one and two elements per thread with a partial last round."""
    scores, classes, boxes = E.topk_case("ties", L, K)
    _check_topk(scores, classes, boxes, K, R.topk(scores, K))


@pytest.mark.parametrize("L,K", E.TOPK_LOWBITS)
def test_topk_keys_that_differ_only_in_the_low_bits(L, K):
    """Distinct keys 0.25 + i ulp: every element shares the first radix digit (and the second for L <= 1024), so the last
    pass and the carry of `need` through the passes decide everything."""
    scores, classes, boxes = E.topk_case("lowbits", L, K)
    _check_topk(scores, classes, boxes, K, R.topk(scores, K))


@pytest.mark.parametrize("kind,L,K", E.TOPK_OTHER)
def test_topk_negative_mixed_equal_and_k_equals_l(kind, L, K):
    scores, classes, boxes = E.topk_case(kind, L, K)
    idx = R.topk(scores, K)
    if kind == "equal":
        np.testing.assert_array_equal(idx, np.tile(np.arange(K, dtype=np.int32), (E.B, 1)))
    _check_topk(scores, classes, boxes, K, idx)


@pytest.mark.parametrize("L,K", E.TOPK_NAN)
def test_topk_positive_nan_first(L, K):
    """A positive quiet NaN sorts above every score, as in torch.topk, several of them by lower index.  The expectation is
    built in numpy from the order key (the oracle's qsort comparator is no total order with NaN).  Out of scope: -0.0
    against +0.0 and negative NaN -- the decode kernel produces neither."""
    scores, classes, boxes = E.topk_case("nan", L, K)
    _check_topk(scores, classes, boxes, K, E.topk_by_key(scores, K))


# ---------------------------------------------------------------------------------------------------- NMS
def _check_batched_nms(scores, classes, boxes, iou_thr, score_thr=E.SCORE_THR):
    """[N, K] rows through ops.batched_nms against the oracle: kept indices and counts equal, kept rows bit-equal to the input
    rows, padding -1 / 0."""
    os_, oc, ob, keep, counts = ops.batched_nms(_t(scores), _t(classes), _t(boxes), score_thr, iou_thr)
    exp = R.post_process(scores, classes, boxes, score_thr, iou_thr)
    os_, oc, ob, keep, counts = (x.cpu().numpy() for x in (os_, oc, ob, keep, counts))
    for b in range(scores.shape[0]):
        n = int(counts[b])
        assert n == len(exp[b]), (b, n, len(exp[b]))
        np.testing.assert_array_equal(keep[b, :n], exp[b], err_msg=f"image {b}")
        assert (keep[b, n:] == -1).all() and (_bits(os_[b, n:]) == 0).all() and (oc[b, n:] == 0).all() and (_bits(ob[b, n:]) == 0).all()
        np.testing.assert_array_equal(_bits(os_[b, :n]), _bits(scores[b][exp[b]]))
        np.testing.assert_array_equal(oc[b, :n], classes[b][exp[b]])
        np.testing.assert_array_equal(_bits(ob[b, :n]), _bits(boxes[b][exp[b]]))
    return exp


def _both_paths(c):
    """One case at K = its own length (K <= 1024: the LDS path) and padded to K >= 1100 (the global-workspace path)."""
    n = len(c["scores"])
    exp = None
    if n <= 1024:
        exp = _check_batched_nms(c["scores"][None], c["classes"][None], c["boxes"][None], c["iou_thr"])[0]
    s, cl, b = E.pad_case(c, max(1100, n))
    big = _check_batched_nms(s[None], cl[None], b[None], c["iou_thr"])[0]
    if exp is not None:
        np.testing.assert_array_equal(big, exp)
    return big


def _check_plus1(boxes, scores, thr, n_valid=None):
    """[N, K] boxes through ops.box_nms_plus1 in both modes against the oracle on each image's valid prefix."""
    N, K = scores.shape
    nv = None if n_valid is None else _t(np.asarray(n_valid, np.int32))
    for mode in ("union", "min"):
        keep, counts = ops.box_nms_plus1(_t(boxes), _t(scores), thr, mode, nv)
        keep, counts = keep.cpu().numpy(), counts.cpu().numpy()
        for b in range(N):
            p = K if n_valid is None else int(n_valid[b])
            exp = R.box_nms_plus1(boxes[b, :p], scores[b, :p], thr, mode) if p else np.zeros(0, np.int32)
            assert int(counts[b]) == len(exp), (mode, b)
            np.testing.assert_array_equal(keep[b, :len(exp)], exp, err_msg=f"{mode} image {b}")
            assert (keep[b, len(exp):] == -1).all()


@pytest.mark.parametrize("n", E.CHAIN_NS + E.CHAIN_NS_LARGE)
@pytest.mark.parametrize("form", E.CHAIN_FORMS)
def test_nms_domino_chains(form, n):
    """A suppression chain laid across rows 31/32, 63/64 and 1023/1024: every decision depends on the one before it, through
    both halves of the in-block scan and through the carry into the later words."""
    c = E.chain_case(form, n)
    keep = _both_paths(c)
    assert 0.3 * n < len(keep) - c["chain"].start < 0.6 * n
    if len(c["scores"]) <= 1024:
        _check_plus1(c["boxes"][None], c["scores"][None], 0.45)


@pytest.mark.parametrize("name", sorted(E.degenerate_cases()))
def test_nms_degenerate_geometry(name):
    c = E.degenerate_cases()[name]
    keep = _both_paths(c)
    assert set(c.get("must_keep", ())) <= set(keep.tolist())
    _check_plus1(c["boxes"][None], c["scores"][None], 0.5)


@pytest.mark.parametrize("name", sorted(E.threshold_cases()))
def test_nms_thresholds(name):
    c = E.threshold_cases()[name]
    keep = _both_paths(c)
    if "n_kept" in c:
        assert len(keep) == c["n_kept"]
    if c.get("all_kept"):
        assert len(keep) == len(c["scores"])
    for thr in (0.0, 1.0):
        _check_plus1(c["boxes"][None], c["scores"][None], thr)


def test_nms_valid_prefixes():
    """0, 1, 64 and 65 rows of K = 200 above the score threshold, in one launch; box_nms_plus1 with the same n_valid."""
    cases = [E.prefix_case(p) for p in E.PREFIXES]
    exp = _check_batched_nms(np.stack([c["scores"] for c in cases]), np.stack([c["classes"] for c in cases]),
                             np.stack([c["boxes"] for c in cases]), cases[0]["iou_thr"])
    assert [len(e) for e in exp] == [0, 1, 22, 22]
    for c in cases:
        _both_paths(c)
    boxes, scores = E.plus1_chain()
    n = len(E.PREFIXES)
    _check_plus1(np.tile(boxes, (n, 1, 1)), np.tile(scores, (n, 1)), 0.45, list(E.PREFIXES))


@pytest.mark.parametrize("K", [1024, 1100])
def test_nms_several_images_with_different_cases(K):
    """Batch 5 in one launch: a chain, an image with nothing above the threshold, two degenerate sets, a chain behind other boxes."""
    d = E.degenerate_cases()
    empty = dict(E.chain_case("next", 100))
    empty["scores"] = np.full(100, 0.01, np.float32)
    cases = [E.chain_case("next", 1023), empty, d["coords_1e6_classes_80"], d["max_is_minus_one"], E.chain_case("behind30", 129)]
    rows = [E.pad_case(c, K) for c in cases]
    exp = _check_batched_nms(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), 0.5)
    assert len(exp[1]) == 0 and len(exp[0]) == 512
