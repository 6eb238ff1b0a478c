"""COCO bbox evaluation: hand-derived known answers pin the numpy restatement (tests/coco_eval_ref.py), plus the host side of
pytorch_object_detection_amd.Test_coco (GT loader, summary format) -- no GPU needed."""
import numpy as np
import pytest

import coco_eval_ref as R
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.Test_coco import coco_stats, format_stats, load_coco_gt

ONE = 1.0 / (1.0 + np.spacing(1))       # one TP out of one detection: 1 / (0 + 1 + 2^-52) = 0.9999999999999998


def dataset(anns, imgs=(1,), cats=(1,)):
    """anns: (image_id, category_id, bbox xywh, iscrowd[, area]); area defaults to w * h."""
    out = []
    for n, a in enumerate(anns):
        img, cat, bb, crowd = a[:4]
        out.append({"id": n + 1, "image_id": img, "category_id": cat, "bbox": [float(v) for v in bb], "iscrowd": crowd,
                    "area": float(a[4]) if len(a) > 4 else float(bb[2] * bb[3])})
    return {"images": [{"id": i} for i in imgs], "categories": [{"id": c} for c in cats], "annotations": out}


def det(img, cat, bb, score):
    return {"image_id": img, "category_id": cat, "bbox": [float(v) for v in bb], "score": float(score)}


def run(ds, res, imgs=None):
    p, r = R.evaluate(ds, res, imgs if imgs is not None else [im["id"] for im in ds["images"]])
    return p, r, R.summarize(p, r)


def test_constants_are_cocoeval_params():
    assert R.IOU_THRS.dtype == np.float64 and len(R.IOU_THRS) == 10 and len(R.REC_THRS) == 101
    assert R.IOU_THRS[0] == .5 and R.IOU_THRS[-1] == .95 and R.REC_THRS[0] == 0 and R.REC_THRS[-1] == 1


def test_perfect_single_match():
    # one 100x100 GT (area 10 000: large), one detection on it: at every threshold a TP out of one detection, so every recall bin
    # holds 1 / (1 + 2^-52); recall 1.0; small / medium have no GT: -1 and left out of the means
    ds = dataset([(1, 1, [10, 20, 100, 100], 0)])
    p, r, s = run(ds, [det(1, 1, [10, 20, 100, 100], .9)])
    for a in (0, 3):
        assert np.all(p[:, :, 0, a, :] == ONE) and ONE == 0.9999999999999998
        assert np.all(r[:, 0, a, :] == 1.0)
    assert np.all(p[:, :, 0, 1:3, :] == -1) and np.all(r[:, 0, 1:3, :] == -1)
    assert s[0] == ONE and s[5] == ONE and s[3] == -1 and s[4] == -1
    assert s[11] == 1.0 and s[9] == -1 and s[10] == -1


@pytest.mark.parametrize("crowd", [1, 0])
def test_crowd_detection_is_ignored(crowd):
    # GT1 = [0,0,100,100], GT2 = [200,200,50,50].  det1 (.9) = [10,10,20,20] lies inside GT1: over a crowd GT IoU = inter / da
    # = 400 / 400 = 1, so it matches the crowd row and is ignored; without the flag IoU = 400 / 10 000 = 0.04: a false positive.
    # det2 (.8) is a perfect TP on GT2.  Crowd: npig = 1, the TP is first -> 1 / (0 + 1 + eps).  Not crowd: npig = 2, the TP
    # comes after one FP -> 1 / (1 + 1 + eps) = 1/2 (2 + 2^-52 rounds to 2), at recall 1/2, 0 above
    ds = dataset([(1, 1, [0, 0, 100, 100], crowd), (1, 1, [200, 200, 50, 50], 0)])
    p, r, _ = run(ds, [det(1, 1, [10, 10, 20, 20], .9), det(1, 1, [200, 200, 50, 50], .8)])
    if crowd:
        assert np.all(p[0, :, 0, 0, 2] == ONE) and r[0, 0, 0, 2] == 1.0
    else:
        assert np.all(p[0, :51, 0, 0, 2] == 0.5) and np.all(p[0, 51:, 0, 0, 2] == 0) and r[0, 0, 0, 2] == 0.5


def test_area_boundary_counts_in_small_and_medium():
    # annotation area exactly 32^2 = 1024: inside [0, 1024] and [1024, 9216] (both ends inclusive), outside large
    ds = dataset([(1, 1, [0, 0, 32, 32], 0, 1024.0)])
    p, r, _ = run(ds, [det(1, 1, [0, 0, 32, 32], .9)])
    assert np.all(r[:, 0, 1, 2] == 1.0) and np.all(r[:, 0, 2, 2] == 1.0) and np.all(r[:, 0, 3, 2] == -1)


def test_last_max_tie_rule():
    # A = [0,0,10,10], B = [2,0,10,10]; det1 = [1,0,10,10] (.9): inter 9 x 10 with either, union 110 -> 9/11 = 0.818 with both.
    # pycocotools keeps the LAST GT with the best IoU: det1 takes B, det2 (= A, .8) takes A -> 2 TPs for t in .7, .75, .8.
    # A first-max rule would give det1 A, and det2 (IoU 80/120 = .667 with B) would be an FP there.  At .85 and above det1 misses.
    ds = dataset([(1, 1, [0, 0, 10, 10], 0), (1, 1, [2, 0, 10, 10], 0)])
    _, r, _ = run(ds, [det(1, 1, [1, 0, 10, 10], .9), det(1, 1, [0, 0, 10, 10], .8)])
    assert np.all(r[:7, 0, 0, 2] == 1.0) and np.all(r[7:, 0, 0, 2] == 0.5)


def test_non_ignored_gt_preferred():
    # det = [0,0,10,10]; crowd C = [1,0,10,10]: IoU = 90 / da 100 = 0.9; non-crowd N = [0,0,10,6]: IoU = 60 / 100 = 0.6.
    # Up to t = .6 the non-ignored N wins although C is better: a TP.  From .65 to .9 only C qualifies: ignored (recall 0, no FP).
    # At .95 nothing: a false positive.
    ds = dataset([(1, 1, [1, 0, 10, 10], 1), (1, 1, [0, 0, 10, 6], 0)])
    p, r, _ = run(ds, [det(1, 1, [0, 0, 10, 10], .9)])
    assert np.all(r[:3, 0, 0, 2] == 1.0) and np.all(r[3:, 0, 0, 2] == 0.0)
    assert np.all(p[:3, :, 0, 0, 2] == ONE) and np.all(p[3:, :, 0, 0, 2] == 0.0)


def test_cut_is_per_image_and_category():
    # category 1: 100 far-away FPs score above a perfect 101st detection, which is cut; category 2 in the same image: its one
    # perfect detection is kept (the cut counts per (image, category), not per image)
    ds = dataset([(1, 1, [0, 0, 50, 50], 0), (1, 2, [100, 100, 50, 50], 0)], cats=(1, 2))
    res = [det(1, 1, [500 + i, 500, 5, 5], .9 - i * 1e-3) for i in range(100)] + [det(1, 1, [0, 0, 50, 50], .1), det(1, 2, [100, 100, 50, 50], .05)]
    _, r, _ = run(ds, res)
    assert np.all(r[:, 0, 0, 2] == 0.0) and np.all(r[:, 1, 0, 2] == 1.0)


@pytest.mark.parametrize("fp_img,tp_img,ap", [(1, 2, 0.5), (2, 1, ONE)])
def test_cross_image_tie_order(fp_img, tp_img, ap):
    # equal scores: images in ascending id order.  FP first: the TP's precision is 1 / (1 + 1 + eps) = 1/2 in every bin; TP first:
    # 1 / (0 + 1 + eps), the FP after it only lowers later positions (the mean of 101 such cells rounds to 1 - 2^-53)
    ds = dataset([(tp_img, 1, [0, 0, 40, 40], 0)], imgs=(1, 2))
    p, _, s = run(ds, [det(fp_img, 1, [100, 100, 40, 40], .5), det(tp_img, 1, [0, 0, 40, 40], .5)])
    assert s[1] == pytest.approx(ap, abs=1e-15) and np.all(p[0, :, 0, 0, 2] == ap)


def test_empty_categories():
    # category 2 has no GT: -1 everywhere and left out of the means; no GT at all: every stat is -1
    ds = dataset([(1, 1, [0, 0, 100, 100], 0)], cats=(1, 2))
    p, r, s = run(ds, [det(1, 1, [0, 0, 100, 100], .9), det(1, 2, [0, 0, 100, 100], .8)])
    assert np.all(p[:, :, 1] == -1) and np.all(r[:, 1] == -1) and s[0] == ONE
    p, r, s = run(dataset([], cats=(1, 2)), [det(1, 1, [0, 0, 100, 100], .9)])
    assert np.all(p == -1) and np.all(r == -1) and np.all(s == -1)


def test_stats_follow_from_arrays():
    rng = np.random.default_rng(0)
    p = np.where(rng.random((10, 101, 3, 4, 3)) < .2, -1.0, rng.random((10, 101, 3, 4, 3)))
    r = np.where(rng.random((10, 3, 4, 3)) < .2, -1.0, rng.random((10, 3, 4, 3)))
    assert coco_stats(p, r).tobytes() == R.summarize(p, r).tobytes()


def test_summary_format():
    s = np.array([.377, .562, .405, .21, .406, .506, .311, .5, .544, .331, .595, -1])
    lines = format_stats(s).split("\n")
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.377"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.562"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.210"
    assert lines[4] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = 0.406"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.311"
    assert lines[7] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 0.500"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
    assert len(lines) == 12


def test_load_coco_gt():
    ds = {"images": [{"id": 5}, {"id": 2}, {"id": 7}], "categories": [{"id": 90}, {"id": 3}, {"id": 17}],
          "annotations": [{"image_id": 2, "category_id": 17, "bbox": [1, 2, 3, 4], "area": 11.5, "iscrowd": 0},
                          {"image_id": 5, "category_id": 90, "bbox": [5, 6, 7, 8], "area": 50.0, "iscrowd": 1},
                          {"image_id": 2, "category_id": 3, "bbox": [9, 9, 9, 9], "area": 81.0},
                          {"image_id": 2, "category_id": 4, "bbox": [0, 0, 1, 1], "area": 1.0, "iscrowd": 0}]}
    g = load_coco_gt(ds)
    assert g.category_ids.tolist() == [3, 17, 90] and g.image_ids.tolist() == [5, 2, 7] and g.num_cats == 3
    assert g.labels.shape == (3, 2) and g.boxes.dtype == np.float64 and g.area.dtype == np.float64 and g.crowd.dtype == np.uint8
    assert g.labels[0].tolist() == [3, -1] and g.crowd[0, 0] == 1 and g.boxes[0, 0].tolist() == [5, 6, 7, 8]
    assert g.labels[1].tolist() == [2, 1] and g.area[1].tolist() == [11.5, 81.0] and g.crowd[1].tolist() == [0, 0]   # file order; category 4 is not listed
    assert g.labels[2].tolist() == [-1, -1]                                                                           # no annotations
    assert g.label_of(17) == 2 and g.label_of(4) == 0

    class FakeCOCO:
        dataset = ds
    assert load_coco_gt(FakeCOCO()).category_ids.tolist() == [3, 17, 90]
    with pytest.raises(FdError):
        load_coco_gt({"images": [{"id": 1}, {"id": 1}], "categories": [{"id": 1}], "annotations": []})


def random_case(rng, n_img, n_det, n_cat, max_gt=8):
    """A dataset and a results list in Test_coco's form: crowd rows, areas over every range, duplicated scores, near-GT boxes."""
    anns, res = [], []
    for i in range(1, n_img + 1):
        gts = []
        for _ in range(int(rng.integers(1, max_gt + 1))):
            wh = rng.choice([rng.uniform(4, 30), rng.uniform(30, 90), rng.uniform(90, 300)], 2)
            bb = [float(rng.uniform(0, 400)), float(rng.uniform(0, 400)), float(wh[0]), float(wh[1])]
            c = int(rng.integers(1, n_cat + 1))
            anns.append((i, c, bb, int(rng.random() < .1), bb[2] * bb[3] * float(rng.uniform(.5, 1.0))))
            gts.append((c, bb))
        for _ in range(n_det):
            if gts and rng.random() < .6:
                c, bb = gts[int(rng.integers(len(gts)))]
                bb = [float(np.float32(v + rng.normal(0, .1 * bb[2 + k % 2]))) for k, v in enumerate(bb)]
            else:
                c = int(rng.integers(1, n_cat + 1))
                bb = [float(np.float32(v)) for v in (rng.uniform(0, 400), rng.uniform(0, 400), rng.uniform(2, 200), rng.uniform(2, 200))]
            res.append(det(i, c, bb, float(np.float32(np.round(rng.random(), 2)))))
    return dataset(anns, imgs=range(1, n_img + 1), cats=range(1, n_cat + 1)), res


def test_against_pycocotools():
    pytest.importorskip("pycocotools")
    import contextlib
    import io

    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    ds, res = random_case(np.random.default_rng(5), 12, 40, 4)
    gt = COCO()
    gt.dataset = ds
    gt.createIndex()
    with contextlib.redirect_stdout(io.StringIO()):
        ev = COCOeval(gt, gt.loadRes(res), "bbox")
        ev.params.imgIds = list(range(1, 13))
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    p, r = R.evaluate(ds, res, range(1, 13))
    assert np.array_equal(p, ev.eval["precision"]) and np.array_equal(r, ev.eval["recall"])
    assert np.array_equal(R.summarize(p, r), ev.stats)
