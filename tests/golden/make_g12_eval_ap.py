"""tests/golden/make_g12_eval_ap.py — the VOC AP fixture g12_eval_ap.npz from the REAL reference evaluation.

Run ONLY in the build container (needs the reference tree, read-only; FD_REFERENCE overrides its path):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g12_eval_ap.py

Imports the reference's test.py with make_golden.py's stub finder (absent third-party modules are stubbed; only the reference's
own numpy code runs) and calls its live sort_by_score + eval_ap_2d at IoU thresholds 0.5, 0.55 (not representable in fp32) and
0.75.  Stores data only: padded detections / GT rows, their counts, the thresholds, the per-label APs and numpy's version.
The zip entries carry a fixed timestamp, so a second run reproduces the file byte for byte.
"""
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stub finder and puts the reference on sys.path)

import numpy as np  # noqa: E402

import test as ref_test  # noqa: E402  (the reference's test.py)

NUM_CLS = 12
THRESHOLDS = (0.5, 0.55, 0.75)


def random_images(rng, n):
    """Labels 1..5 with distinct scores; jittered copies of GT boxes (TPs and near misses) and random boxes; ignored rows
    (labels 0, -1, >= NUM_CLS) sprinkled in."""
    imgs = []
    for _ in range(n):
        g = int(rng.integers(1, 6))
        xy = rng.uniform(0, 400, (g, 2)).astype(np.float32)
        wh = rng.uniform(10, 120, (g, 2)).astype(np.float32)
        gb = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        gl = rng.integers(1, 6, g).astype(np.int64)
        if rng.random() < 0.3:
            gb = np.concatenate([gb, np.array([[-1, -1, -1, -1]], np.float32)])
            gl = np.concatenate([gl, np.array([int(rng.choice([0, -1, NUM_CLS]))])])
        k = int(rng.integers(0, 40))
        src = rng.integers(0, g, k)
        jit = rng.normal(0, 1, (k, 4)).astype(np.float32) * (wh[src].repeat(2, 1) * np.float32(rng.uniform(0.02, 0.4)))
        pb = (gb[src] + jit).astype(np.float32)
        rnd = rng.random(k) < 0.3
        rxy = rng.uniform(0, 400, (k, 2)).astype(np.float32)
        pb[rnd] = np.concatenate([rxy, rxy + rng.uniform(10, 120, (k, 2)).astype(np.float32)], 1)[rnd]
        pl = gl[src].copy()
        flip = rng.random(k) < 0.15
        pl[flip] = rng.integers(1, 6, int(flip.sum()))
        odd = rng.random(k) < 0.05
        pl[odd] = rng.choice([0, -1, NUM_CLS, NUM_CLS + 3], int(odd.sum()))
        imgs.append([gb, gl, pb, pl])
    return imgs


def crafted_images():
    f = lambda *r: np.array(r, np.float32).reshape(-1, 4)  # noqa: E731
    i = lambda *r: np.array(r, np.int64)  # noqa: E731
    imgs = []
    # label 6: the best GT box is already taken; a second GT box is above the threshold -- still a false positive (no fall-back)
    imgs.append([f(0, 0, 10, 10, 0, 0, 10, 9), i(6, 6), f(0, 0, 10, 10, 0, 0, 10, 9.9), i(6, 6)])
    # label 7: zero-area GT against a zero-area prediction: IoU NaN, the first NaN wins the argmax, never a TP
    imgs.append([f(0, 0, 10, 10, 5, 5, 5, 5), i(7, 7), f(5, 5, 5, 5, 0, 0, 10, 10, 5, 5, 5, 5), i(7, 7, 7)])
    imgs.append([f(5, 5, 5, 5, 0, 0, 10, 10), i(7, 7), f(5, 5, 5, 5, 0, 1, 10, 10), i(7, 7)])
    # label 8: predictions, no GT anywhere (AP NaN); label 9: GT, no predictions (AP 0.0)
    imgs.append([f(20, 20, 40, 40), i(9), f(0, 0, 5, 5, 1, 1, 6, 6), i(8, 8)])
    # label 10: IoU exactly 0.5 and exactly 0.75 in fp32
    imgs.append([f(0, 0, 2, 1, 10, 0, 14, 1), i(10, 10), f(0, 0, 1, 1, 10, 0, 13, 1), i(10, 10)])
    # rows the evaluation ignores: labels 0, -1 and >= NUM_CLS, in GT and predictions
    imgs.append([f(0, 0, 10, 10, 0, 0, 10, 10, 0, 0, 10, 10), i(0, -1, NUM_CLS), f(0, 0, 10, 10, 0, 0, 10, 10, 0, 0, 10, 10),
                 i(0, -1, NUM_CLS)])
    # empty images
    imgs.append([f(), i(), f(), i()])
    imgs.append([f(30, 30, 50, 50), i(3), f(), i()])
    imgs.append([f(), i(), f(30, 30, 50, 50), i(4)])
    return imgs


def big_label_images(rng, label=11, n_img=8, per_img=40):
    """One label with n_img * per_img = 320 GT boxes and ~250 TPs among false positives: its AP sums over 128 terms."""
    imgs = []
    for _ in range(n_img):
        xy = (rng.integers(0, 40, (per_img, 2)) * 25).astype(np.float32)
        gb = np.concatenate([xy, xy + np.float32(20)], 1)
        hit = rng.random(per_img) < 0.8
        pb = gb[hit] + rng.uniform(-2, 2, (int(hit.sum()), 4)).astype(np.float32)
        fp = rng.uniform(0, 1000, (per_img // 3, 2)).astype(np.float32)
        pb = np.concatenate([pb, np.concatenate([fp, fp + np.float32(7)], 1)]).astype(np.float32)
        imgs.append([gb, np.full(per_img, label, np.int64), pb, np.full(len(pb), label, np.int64)])
    return imgs


def main():
    rng = np.random.default_rng(12)
    imgs = random_images(rng, 60) + crafted_images() + big_label_images(rng)
    rng.shuffle(imgs)
    total = sum(len(im[2]) for im in imgs)
    # scores: distinct over the whole set (no ties anywhere), in (0.05, 1)
    pool = rng.permutation(np.linspace(0.05, 0.999, 4 * total + 17, dtype=np.float32))[:total]
    assert len(np.unique(pool)) == total, "score ties"
    off = 0
    for im in imgs:
        k = len(im[2])
        im.append(pool[off:off + k].copy())
        off += k
    N = len(imgs)
    K = max(len(im[2]) for im in imgs)
    G = max(len(im[0]) for im in imgs)
    det_scores = np.zeros((N, K), np.float32)
    det_classes = np.zeros((N, K), np.int64)
    det_boxes = np.zeros((N, K, 4), np.float32)
    det_counts = np.zeros(N, np.int32)
    gt_boxes = np.zeros((N, G, 4), np.float32)
    gt_classes = np.full((N, G), -1, np.int64)
    gt_counts = np.zeros(N, np.int32)
    for n, (gb, gl, pb, pl, ps) in enumerate(imgs):
        det_counts[n], gt_counts[n] = len(ps), len(gl)
        det_scores[n, :len(ps)], det_classes[n, :len(ps)], det_boxes[n, :len(ps)] = ps, pl, pb
        gt_boxes[n, :len(gl)], gt_classes[n, :len(gl)] = gb, gl

    pred_boxes, pred_labels, pred_scores = ref_test.sort_by_score([im[2] for im in imgs], [im[3] for im in imgs], [im[4] for im in imgs])
    ap = np.zeros((len(THRESHOLDS), NUM_CLS - 1), np.float64)
    for t, thr in enumerate(THRESHOLDS):
        with np.errstate(invalid="ignore", divide="ignore"):
            res = ref_test.eval_ap_2d([im[0] for im in imgs], [im[1] for im in imgs], pred_boxes, pred_labels, pred_scores, thr, NUM_CLS)
        ap[t] = [res[lab] for lab in range(1, NUM_CLS)]
    assert np.isnan(ap[:, 7]).all() and (ap[:, 8] == 0).all(), ap    # label 8 NaN, label 9 0.0
    arrays = dict(det_scores=det_scores, det_classes=det_classes, det_boxes=det_boxes, det_counts=det_counts, gt_boxes=gt_boxes,
                  gt_classes=gt_classes, gt_counts=gt_counts, thresholds=np.array(THRESHOLDS, np.float64), num_cls=np.int64(NUM_CLS),
                  ap=ap, numpy_version=np.array(np.__version__))
    path = os.path.join(HERE, "g12_eval_ap.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"g12_eval_ap.npz  {os.path.getsize(path) / 1024:.1f} KB  N={N} K={K} G={G} detections={total}")
    print("AP:\n", ap)


if __name__ == "__main__":
    main()
