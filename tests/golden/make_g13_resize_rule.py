"""tests/golden/make_g13_resize_rule.py — the resize-rule fixture g13_resize_rule.npz from the REAL reference.

Run ONLY in the build container (needs the reference tree, read-only; FD_REFERENCE overrides its path):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g13_resize_rule.py

Imports the reference's dataset/voc.py and Test_coco.py with make_golden.py's stub finder (torchvision, cv2, pycocotools
are absent and stubbed; the stub's CocoDetection is made an empty class so that COCOGenerator can derive from it) and
calls their two live `preprocess_img_boxes` (voc.py:110-139, Test_coco.py:76-105) on zero images of many shapes.  `cv2.resize` -- third-party, absent -- is replaced by a recorder that notes the requested (nw, nh) and
returns zeros of that size, so everything stored is the reference's own arithmetic: the size rule, the pad-to-32 and the
fp32 box scaling.  Both modules import with the stubs and both functions agree on every row (asserted); `scale` itself is
returned only by Test_coco.py's version.  Stores data only; the zip entries carry a fixed timestamp, so a second run
reproduces the file byte for byte.

Rows: shapes[i] = (h, w, min_side, max_side) -> resized[i] = (nh, nw), padded[i] = (padded h, padded w), scale[i] (float64),
boxes_in[i] / boxes_out[i] = fp32 [4, 4] ground-truth boxes before / after the reference scaled them.
"""
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stub finder and puts the reference on sys.path)

import numpy as np  # noqa: E402

import torchvision.datasets  # noqa: E402  (a stub; Test_coco.py derives COCOGenerator from its CocoDetection, so that name must be a class)

torchvision.datasets.CocoDetection = type("CocoDetection", (), {})

import Test_coco as ref_coco  # noqa: E402  (the reference's Test_coco.py)
from dataset import voc as ref_voc  # noqa: E402  (the reference's dataset/voc.py)

NBOX = 4
_calls = []


def _recording_resize(image, dsize, *a, **k):
    nw, nh = dsize
    _calls.append((int(nh), int(nw)))
    return np.zeros((nh, nw, 3), np.uint8)


ref_voc.cv2.resize = _recording_resize
ref_coco.cv2.resize = _recording_resize


def shapes():
    named = [(289, 333), (375, 500), (480, 640), (500, 375), (640, 480), (333, 289), (427, 640), (640, 427), (1200, 1600), (1600, 1200),
             (37, 53), (2000, 900), (900, 2000), (512, 512), (800, 1333), (1333, 800), (800, 800), (32, 32), (1, 9), (9, 1), (5, 7),
             (100, 1000), (1000, 100), (768, 1024), (1080, 1920), (1920, 1080), (224, 224), (300, 451), (451, 300), (641, 359)]
    rng = np.random.default_rng(13)
    rnd = [(int(h), int(w)) for h, w in rng.integers(30, 2100, (90, 2))]
    out = []
    for h, w in named + rnd:
        for size in ([512, 512], [800, 1333]):
            out.append((h, w, size[0], size[1]))
    return out


def main():
    rng = np.random.default_rng(113)
    rows = shapes()
    n = len(rows)
    shp = np.array(rows, np.int64)
    resized = np.zeros((n, 2), np.int64)
    padded = np.zeros((n, 2), np.int64)
    scale = np.zeros(n, np.float64)
    boxes_in = np.zeros((n, NBOX, 4), np.float32)
    boxes_out = np.zeros((n, NBOX, 4), np.float32)
    for i, (h, w, mn, mx) in enumerate(rows):
        img = np.zeros((h, w, 3), np.uint8)
        xy = rng.uniform(0, 1, (NBOX, 2)) * [w, h] * 0.7
        wh = rng.uniform(0.05, 0.3, (NBOX, 2)) * [w, h]
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        boxes_in[i] = b
        del _calls[:]
        pad_c, box_c, sc = ref_coco.COCOGenerator.preprocess_img_boxes(None, img, b.copy(), [mn, mx])
        pad_v, box_v = ref_voc.VOCDataset.preprocess_img_boxes(None, img, b.copy(), [mn, mx])
        assert len(_calls) == 2 and _calls[0] == _calls[1], _calls
        assert pad_c.shape == pad_v.shape and np.array_equal(box_c, box_v) and box_c.dtype == np.float32
        assert isinstance(sc, float)
        resized[i] = _calls[0]
        padded[i] = pad_c.shape[:2]
        scale[i] = sc
        boxes_out[i] = box_c
    k = rows.index((289, 333, 800, 1333))
    assert tuple(resized[k]) == (799, 921), resized[k]
    arrays = dict(shapes=shp, resized=resized, padded=padded, scale=scale, boxes_in=boxes_in, boxes_out=boxes_out,
                  source=np.array("reference preprocess_img_boxes (dataset/voc.py and Test_coco.py), cv2.resize stubbed by a recorder"),
                  numpy_version=np.array(np.__version__))
    path = os.path.join(HERE, "g13_resize_rule.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"g13_resize_rule.npz  {os.path.getsize(path) / 1024:.1f} KB  rows={n}")


if __name__ == "__main__":
    main()
