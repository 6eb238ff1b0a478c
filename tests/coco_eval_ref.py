"""COCO bbox evaluation in numpy, restated from the published COCOeval algorithm (pycocotools cocoeval.py evaluate / evaluateImg /
accumulate / summarize, maskApi.c bbIou) for iouType 'bbox', useCats=1 and default Params -- the checker of the device path
(pytorch_object_detection_amd.Test_coco / fd_eval_coco).  pycocotools itself is not needed; where it is installed,
test_eval_coco_cpu.py cross-checks this file against it.

Inputs are what reach pycocotools: `dataset`, an instances dict (images, annotations, categories); `results`, Test_coco's list of
{"image_id", "category_id", "score", "bbox" (xywh)}; `img_ids`, the evaluated images (COCOeval.params.imgIds).
"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


def _fmin(a, b):
    return b if a != a else (a if b != b else (a if a < b else b))


def _fmax(a, b):
    return b if a != a else (a if b != b else (a if a > b else b))


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one detection / GT pair of xywh boxes, in its operation order (fp64)."""
    d = [float(v) for v in d]
    g = [float(v) for v in g]
    da, ga = d[2] * d[3], g[2] * g[3]
    w = _fmin(d[2] + d[0], g[2] + g[0]) - _fmax(d[0], g[0])
    if w <= 0:
        return 0.0
    h = _fmin(d[3] + d[1], g[3] + g[1]) - _fmax(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def _evaluate_img(gt, dt, a_rng, max_det):
    """COCOeval.evaluateImg for one (image, category, area range)."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    ign = [1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(ign, kind="mergesort")
    gt = [gt[i] for i in gtind]
    gt_ig = np.array([ign[i] for i in gtind])
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = [[bb_iou(d["bbox"], g["bbox"], iscrowd[j]) for j, g in enumerate(gt)] for d in dt]
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    dt_ig = np.zeros((T, D))
    for tind, t in enumerate(IOU_THRS):
        for dind, d in enumerate(dt):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind, gind] > 0 and not iscrowd[gind]:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind][gind] < iou:
                    continue
                iou = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dtm[tind, dind] = gt[m]["id"]
            gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def evaluate(dataset, results, img_ids):
    """-> (precision [T, R, K, A, M], recall [T, K, A, M]) as COCOeval.accumulate leaves them; K = every category of the dataset in
    ascending id."""
    cat_ids = sorted({c["id"] for c in dataset["categories"]})
    img_ids = sorted(set(int(i) for i in img_ids))
    cats, imgs = set(cat_ids), set(img_ids)
    gts, dts = {}, {}
    for n, g in enumerate(dataset["annotations"]):
        if g["image_id"] in imgs and g["category_id"] in cats:
            g = dict(g, iscrowd=int(g.get("iscrowd", 0)), id=g.get("id", n + 1))
            gts.setdefault((g["image_id"], g["category_id"]), []).append(g)
    for n, d in enumerate(results):        # COCO.loadRes: ids from 1, area = w * h, iscrowd 0
        if d["image_id"] in imgs and d["category_id"] in cats:
            bb = d["bbox"]
            d = dict(d, area=bb[2] * bb[3], id=n + 1, iscrowd=0)
            dts.setdefault((d["image_id"], d["category_id"]), []).append(d)
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, c in enumerate(cat_ids):
        for a, rng in enumerate(AREA_RNG):
            E = [_evaluate_img(gts.get((i, c), []), dts.get((i, c), []), rng, MAX_DETS[-1]) for i in img_ids]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def summarize(precision, recall):
    """COCOeval.summarize's 12 numbers (summarizeDets) from the two arrays."""
    def one(ap, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(1), one(1, .5), one(1, .75), one(1, area="small"), one(1, area="medium"), one(1, area="large"),
                     one(0, max_dets=1), one(0, max_dets=10), one(0), one(0, area="small"), one(0, area="medium"), one(0, area="large")],
                    dtype=np.float64)
