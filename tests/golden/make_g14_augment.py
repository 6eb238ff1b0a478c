"""tests/golden/make_g14_augment.py — the augmentation fixture g14_augment.npz from the REAL reference and from PIL itself.

Run ONLY in the build container (needs the reference tree, read-only; FD_REFERENCE overrides its path; needs PIL):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g14_augment.py

Imports the reference's dataset/voc.py (flip) and data/augment.py (Transforms) with make_golden.py's stub finder
(torchvision and cv2 are absent and stubbed).  `colorJitter` -- torchvision's ColorJitter, absent -- is replaced: in part (a)
by a recorder that returns the image unchanged, in part (b) by a function that applies a stored chain with PIL's own
ImageEnhance / HSV conversions.  Image.rotate and Image.crop are wrapped to note the angle and the rectangle the reference
hands them.  Stores data only; the zip entries carry a fixed timestamp, so a second run reproduces the file byte for byte.

(a) decisions and boxes: rows over seeds x image sizes x box sets.  With random.seed(seed): the flip line of
    VOCDataset.__getitem__ (voc.py:98-99, restated here: `if random.random() < 0.5: flip`), then Transforms()(img, boxes).
    a_hw, a_seed, a_nbox, a_boxes_in [R, K, 4], a_flip, a_jitter, a_rot, a_d (float64), a_crop, a_rect (x, y, w, h),
    a_out_hw, a_boxes_out [R, K, 4].
(b) pixels PIL returns: img0..img2 = base images; rot_img / rot_d / rot_out_k: Image.rotate(d); enh_img / enh_op / enh_arg /
    enh_out_k: ImageEnhance.Brightness / Contrast / Color .enhance(f) (op 1 / 2 / 3) and the hue operation (op 4: convert to
    HSV, H += uint8 shift with wrap, convert back; arg = the shift); whole_seed / whole_chain_ops / whole_chain_args /
    whole_out_k / whole_boxes_in / whole_boxes_out: flip + the reference's whole Transforms call on img1 with the chain applied
    by PIL when the jitter decision falls.
"""
import io
import os
import random
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (installs the stub finder and puts the reference on sys.path)

import numpy as np  # noqa: E402
from PIL import Image, ImageEnhance  # noqa: E402

import torchvision.datasets  # noqa: E402  (a stub; the reference's data package derives classes from these names, so they must be classes)

torchvision.datasets.VOCDetection = type("VOCDetection", (), {})
torchvision.datasets.CocoDetection = type("CocoDetection", (), {})

from data import augment as ref_aug  # noqa: E402  (the reference's data/augment.py)
from dataset import voc as ref_voc  # noqa: E402  (the reference's dataset/voc.py)

K = 5
_seen = {}
_orig_rotate, _orig_crop = Image.Image.rotate, Image.Image.crop


def _rotate(self, angle, *a, **k):
    _seen["d"] = float(angle)
    return _orig_rotate(self, angle, *a, **k)


def _crop(self, box=None):
    _seen["rect"] = tuple(int(v) for v in box)
    return _orig_crop(self, box)


Image.Image.rotate = _rotate
Image.Image.crop = _crop
_chain = []


def pil_hue(img, shift):
    h, s, v = img.convert("HSV").split()
    nh = ((np.array(h, dtype=np.int64) + int(shift)) & 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")


def pil_op(img, op, arg):
    if op == 4:
        return pil_hue(img, arg)
    cls = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}[op]
    return cls(img).enhance(arg)


def _jitter(img, boxes, *a, **k):
    _seen["jitter"] = True
    for op, arg in _chain:
        img = pil_op(img, op, arg)
    return img, boxes


ref_aug.colorJitter = _jitter


def run_reference(seed, img, boxes):
    _seen.clear()
    random.seed(seed)
    flipped = False
    if random.random() < 0.5:                      # dataset/voc.py:98-99
        img, boxes = ref_voc.flip(img, boxes)
        flipped = True
    img, boxes = ref_aug.Transforms()(img, boxes)
    return img, boxes, flipped, dict(_seen)


def box_sets(rng, h, w):
    def rnd(n):
        xy = rng.uniform(0, 0.7, (n, 2)) * [w, h]
        wh = rng.uniform(0.05, 0.3, (n, 2)) * [w, h]
        return np.concatenate([xy, xy + wh], 1).astype(np.float32)
    border = np.array([[0, 0, w - 1, h - 1], [0, h * 0.25, w * 0.5, h - 1], [w * 0.5, 0, w - 1, h * 0.5]], np.float32)
    return [np.zeros((0, 4), np.float32), rnd(1), rnd(K), border]


def part_a():
    sizes = [(375, 500), (500, 375), (480, 640), (37, 53), (333, 289), (64, 96)]
    rng = np.random.default_rng(14)
    rows = []
    for _ in range(40):
        for h, w in sizes:
            for b in box_sets(rng, h, w):
                img = Image.new("RGB", (w, h))
                s = len(rows) * 7 + 1          # a seed of its own for every row
                out_img, out_b, flipped, seen = run_reference(s, img, b.copy())
                rows.append((h, w, s, b, flipped, seen, out_img.size, np.asarray(out_b, np.float32)))
    R = len(rows)
    a = dict(a_hw=np.zeros((R, 2), np.int64), a_seed=np.zeros(R, np.int64), a_nbox=np.zeros(R, np.int64), a_boxes_in=np.zeros((R, K, 4), np.float32),
             a_flip=np.zeros(R, bool), a_jitter=np.zeros(R, bool), a_rot=np.zeros(R, bool), a_d=np.zeros(R, np.float64), a_crop=np.zeros(R, bool),
             a_rect=np.zeros((R, 4), np.int64), a_out_hw=np.zeros((R, 2), np.int64), a_boxes_out=np.zeros((R, K, 4), np.float32))
    for i, (h, w, seed, b, flipped, seen, size, ob) in enumerate(rows):
        n = b.shape[0]
        assert ob.shape == (n, 4) and ob.dtype == np.float32
        a["a_hw"][i], a["a_seed"][i], a["a_nbox"][i] = (h, w), seed, n
        a["a_boxes_in"][i, :n], a["a_boxes_out"][i, :n] = b, ob
        a["a_flip"][i], a["a_jitter"][i] = flipped, seen.get("jitter", False)
        a["a_rot"][i], a["a_d"][i] = "d" in seen, seen.get("d", 0.0)
        a["a_crop"][i] = "rect" in seen
        if "rect" in seen:
            x0, y0, x1, y1 = seen["rect"]
            a["a_rect"][i] = (x0, y0, x1 - x0, y1 - y0)
        a["a_out_hw"][i] = (size[1], size[0])
    for k in ("a_flip", "a_jitter", "a_rot", "a_crop"):
        assert 0.15 < a[k].mean() < 0.85, (k, a[k].mean())
    return a


def part_b():
    rng = np.random.default_rng(41)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(33, 47), (48, 64), (64, 96)]]
    imgs[0] = (imgs[0] // 3 + 150).astype(np.uint8)          # a bright image: brightness / contrast clip at 255
    out = {f"img{i}": im for i, im in enumerate(imgs)}
    rot = [(0, 7.25), (0, -89.5), (1, -3.3), (1, 10.0), (2, 45.0), (2, -0.37)]
    out["rot_img"], out["rot_d"] = np.array([r[0] for r in rot], np.int64), np.array([r[1] for r in rot], np.float64)
    for k, (i, d) in enumerate(rot):
        out[f"rot_out_{k}"] = np.array(Image.fromarray(imgs[i]).rotate(d))
    enh = [(0, 1, 1.0837), (0, 2, 1.0999), (0, 3, 0.9013), (0, 4, 25), (1, 1, 0.9125), (1, 2, 0.9301), (1, 3, 1.0955), (1, 4, 231)]
    out["enh_img"], out["enh_op"] = np.array([e[0] for e in enh], np.int64), np.array([e[1] for e in enh], np.int64)
    out["enh_arg"] = np.array([e[2] for e in enh], np.float64)
    for k, (i, op, arg) in enumerate(enh):
        out[f"enh_out_{k}"] = np.array(pil_op(Image.fromarray(imgs[i]), op, arg))
    # the whole Transforms call: the first seed of every (jitter, rotation, crop) combination
    h, w = imgs[1].shape[:2]
    boxes = np.array([[5, 6, 30, 40], [20, 10, 60, 44]], np.float32)
    crng = np.random.default_rng(77)
    want, picked = {(j, r, c) for j in (0, 1) for r in (0, 1) for c in (0, 1)}, []
    for seed in range(1000):
        if not want:
            break
        _, _, _, seen = run_reference(seed, Image.new("RGB", (w, h)), boxes.copy())
        key = (int("jitter" in seen), int("d" in seen), int("rect" in seen))
        if key in want:
            want.discard(key)
            picked.append(seed)
    assert not want
    S = len(picked)
    out["whole_seed"] = np.array(picked, np.int64)
    out["whole_chain_ops"], out["whole_chain_args"] = np.zeros((S, 4), np.int64), np.zeros((S, 4), np.float64)
    out["whole_boxes_in"], out["whole_boxes_out"] = boxes, np.zeros((S, 2, 4), np.float32)
    for k, seed in enumerate(picked):
        order = crng.permutation(4) + 1
        args = {1: crng.uniform(0.9, 1.1), 2: crng.uniform(0.9, 1.1), 3: crng.uniform(0.9, 1.1), 4: float(int(crng.uniform(-0.1, 0.1) * 255) & 255)}
        del _chain[:]
        _chain.extend((int(op), args[int(op)]) for op in order)
        out["whole_chain_ops"][k], out["whole_chain_args"][k] = order, [args[int(op)] for op in order]
        img, ob, _, _ = run_reference(seed, Image.fromarray(imgs[1]), boxes.copy())
        out[f"whole_out_{k}"] = np.array(img)
        out["whole_boxes_out"][k] = ob
    del _chain[:]
    return out


def main():
    arrays = dict(part_a())
    arrays.update(part_b())
    arrays["source"] = np.array("reference dataset/voc.py flip + data/augment.py Transforms (colorJitter replaced); pixels by PIL " + Image.__version__)
    arrays["numpy_version"] = np.array(np.__version__)
    path = os.path.join(HERE, "g14_augment.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"g14_augment.npz  {os.path.getsize(path) / 1024:.1f} KB  rows(a)={len(arrays['a_seed'])}")


if __name__ == "__main__":
    main()
