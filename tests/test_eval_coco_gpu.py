"""COCO bbox evaluation on the device (fd_eval_coco / pytorch_object_detection_amd.Test_coco) against the numpy restatement
(tests/coco_eval_ref.py): precision and recall equal in every cell (-1 cells included), stats identical."""
import numpy as np
import pytest
import torch

import coco_eval_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.Test_coco import COCOEvaluator, evaluate_coco, load_coco_gt
from test_eval_coco_cpu import dataset, det, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(gt, results, ids, K=None):
    """Test_coco's results of the images `ids` -> padded device tensors (row order = results order within an image) + counts."""
    per = {i: [r for r in results if r["image_id"] == i] for i in ids}
    K = K or max([len(v) for v in per.values()] + [1])
    s, c, b = np.zeros((len(ids), K), np.float32), np.zeros((len(ids), K), np.int64), np.zeros((len(ids), K, 4), np.float32)
    n = np.zeros(len(ids), np.int32)
    for j, i in enumerate(ids):
        rows = per[i]
        n[j] = len(rows)
        for k, r in enumerate(rows):
            s[j, k], c[j, k], b[j, k] = r["score"], gt.label_of(r["category_id"]), r["bbox"]
    return [_d(x) for x in (s, c, b, n)]


def _device(ds, results, ids=None, ev=None):
    ids = ids if ids is not None else [im["id"] for im in ds["images"]]
    ev = ev or COCOEvaluator(ds)
    ev.add(ids, *_batch(ev.gt, results, ids))
    return ev.compute()


def _check(ds, results, ids=None):
    ids = ids if ids is not None else [im["id"] for im in ds["images"]]
    res = _device(ds, results, ids)
    p, r = R.evaluate(ds, results, ids)
    assert res["precision"].shape == p.shape and res["recall"].shape == r.shape
    assert np.array_equal(res["precision"], p), np.argwhere(res["precision"] != p)[:10]
    assert np.array_equal(res["recall"], r), np.argwhere(res["recall"] != r)[:10]
    assert res["stats"].tobytes() == R.summarize(p, r).tobytes()
    return res


# --------------------------------------------------------------------------------------------------------------------------------
# the known-answer cases of test_eval_coco_cpu.py, on the device
def test_perfect_single_match():
    res = _check(dataset([(1, 1, [10, 20, 100, 100], 0)]), [det(1, 1, [10, 20, 100, 100], .9)])
    assert res["precision"][0, 0, 0, 0, 2] == 0.9999999999999998 and res["stats"][3] == -1


@pytest.mark.parametrize("crowd", [1, 0])
def test_crowd(crowd):
    _check(dataset([(1, 1, [0, 0, 100, 100], crowd), (1, 1, [200, 200, 50, 50], 0)]),
           [det(1, 1, [10, 10, 20, 20], .9), det(1, 1, [200, 200, 50, 50], .8)])


def test_area_boundary():
    _check(dataset([(1, 1, [0, 0, 32, 32], 0, 1024.0)]), [det(1, 1, [0, 0, 32, 32], .9)])


def test_last_max_tie_rule():
    res = _check(dataset([(1, 1, [0, 0, 10, 10], 0), (1, 1, [2, 0, 10, 10], 0)]), [det(1, 1, [1, 0, 10, 10], .9), det(1, 1, [0, 0, 10, 10], .8)])
    assert np.all(res["recall"][:7, 0, 0, 2] == 1.0)


def test_non_ignored_preferred():
    _check(dataset([(1, 1, [1, 0, 10, 10], 1), (1, 1, [0, 0, 10, 6], 0)]), [det(1, 1, [0, 0, 10, 10], .9)])


def test_cut_per_image_and_category():
    ds = dataset([(1, 1, [0, 0, 50, 50], 0), (1, 2, [100, 100, 50, 50], 0)], cats=(1, 2))
    res = [det(1, 1, [500 + i, 500, 5, 5], .9 - i * 1e-3) for i in range(100)] + [det(1, 1, [0, 0, 50, 50], .1), det(1, 2, [100, 100, 50, 50], .05)]
    out = _check(ds, res)
    assert np.all(out["recall"][:, 0, 0, 2] == 0.0) and np.all(out["recall"][:, 1, 0, 2] == 1.0)


@pytest.mark.parametrize("fp_img,tp_img", [(1, 2), (2, 1)])
def test_cross_image_tie_order(fp_img, tp_img):
    _check(dataset([(tp_img, 1, [0, 0, 40, 40], 0)], imgs=(1, 2)), [det(fp_img, 1, [100, 100, 40, 40], .5), det(tp_img, 1, [0, 0, 40, 40], .5)])


def test_empty_categories():
    _check(dataset([(1, 1, [0, 0, 100, 100], 0)], cats=(1, 2)), [det(1, 1, [0, 0, 100, 100], .9), det(1, 2, [0, 0, 100, 100], .8)])
    res = _check(dataset([], cats=(1, 2)), [det(1, 1, [0, 0, 100, 100], .9)])
    assert np.all(res["stats"] == -1)


# --------------------------------------------------------------------------------------------------------------------------------
# scale: 500 images x 300 detections x 80 categories, crowd rows, every area range, duplicated scores, > 100 detections of one
# category in some images
def _scale_case():
    rng = np.random.default_rng(21)
    ds, res = random_case(rng, 500, 300, 80, max_gt=20)
    heavy = [r for r in res if r["image_id"] % 25 == 0]
    for r in heavy:     # every detection of these images in one category: the per-(image, category) cut of 100 bites
        r["category_id"] = 7
    return ds, res


def test_scale_bit_identical():
    ds, res = _scale_case()
    per = {}
    for r in res:
        per[(r["image_id"], r["category_id"])] = per.get((r["image_id"], r["category_id"]), 0) + 1
    assert max(per.values()) > 100
    out = _check(ds, res)
    assert np.any(out["precision"] > 0) and np.all(out["n_gt"] >= 0)


def test_ragged_batches_no_sync_and_order():
    ds, res = random_case(np.random.default_rng(3), 40, 30, 6, max_gt=10)
    ids = list(range(1, 41))
    whole = _device(ds, res, ids)
    rng = np.random.default_rng(4)
    shuffled = [int(i) for i in rng.permutation(ids)]
    ev = COCOEvaluator(ds)
    batches, i = [], 0
    while i < len(shuffled):
        n = int(rng.integers(1, 7))
        chunk = shuffled[i:i + n]
        i += n
        batches.append((chunk, _batch(ev.gt, res, chunk, K=30 + int(rng.integers(0, 5)))))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for chunk, bt in batches:
            ev.add(chunk, *bt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = ev.compute()
    for k in ("precision", "recall", "stats", "n_gt"):
        assert out[k].tobytes() == whole[k].tobytes(), k
    # reset(), then a narrower batch of fewer images: equal to a fresh evaluator
    ev.reset()
    assert ev.num_images == 0
    sub = ids[:9]
    again = _device(ds, res, sub, ev=ev)
    fresh = _device(ds, res, sub)
    for k in ("precision", "recall", "stats"):
        assert again[k].tobytes() == fresh[k].tobytes(), k
    p, r = R.evaluate(ds, res, sub)
    assert np.array_equal(again["precision"], p) and np.array_equal(again["recall"], r)


def test_limits_and_ids():
    ds = dataset([(1, 1, [0, 0, 10, 10], 0)], imgs=(1, 2))
    ev = COCOEvaluator(ds)
    s, c, b, n = _batch(ev.gt, [det(1, 1, [0, 0, 10, 10], .9)], [1])
    with pytest.raises(FdError):
        ev.add([99], s, c, b, n)                 # not in the GT
    ev.add([1], s, c, b, n)
    with pytest.raises(FdError):
        ev.add([1], s, c, b, n)                  # added twice
    with pytest.raises(FdError):
        ev.add([2], torch.zeros(1, 1025, device=DEV), torch.zeros(1, 1025, dtype=torch.int64, device=DEV),
               torch.zeros(1, 1025, 4, device=DEV), None)
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=DEV)  # noqa: E731
    with pytest.raises(FdError, match="limits"):
        ops.eval_coco(z(1, 4), z(1, 4, dt=torch.int64), z(1, 4, 4), None, z(1, 513, 4, dt=torch.float64), z(1, 513, dt=torch.float64),
                      z(1, 513, dt=torch.uint8), z(1, 513, dt=torch.int64), 3)
    with pytest.raises(FdError, match="limits"):
        ops.eval_coco(z(1, 4), z(1, 4, dt=torch.int64), z(1, 4, 4), None, z(1, 2, 4, dt=torch.float64), z(1, 2, dt=torch.float64),
                      z(1, 2, dt=torch.uint8), z(1, 2, dt=torch.int64), 129)
    with pytest.raises(FdError):
        load_coco_gt(dataset([(1, 1, [0, 0, 1, 1], 0)] * 513))


# --------------------------------------------------------------------------------------------------------------------------------
# evaluate_coco end to end
class _Recorder(torch.nn.Module):
    """Runs the model and, on the same outputs, the reference's loop (Test_coco.py:140-171): FCOSHead -> ClipBoxes -> numpy,
    boxes /= scale, xywh, break at the first score < threshold, results list."""

    def __init__(self, model, gen):
        super().__init__()
        self.model, self.gen, self.results, self.n = model, gen, [], 0

    def forward(self, imgs):
        from pytorch_object_detection_amd.model.modules.head import ClipBoxes, FCOSHead
        out = self.model(imgs)
        s, c, b, n = FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64]).detect_padded(out)
        b = ClipBoxes()(imgs, b.clone())
        k = int(n[0])
        scores, labels, boxes = s[:, :k].cpu().numpy(), c[:, :k].cpu().numpy(), b[:, :k].cpu().numpy()
        scale = self.gen.scales[self.n]
        boxes /= scale
        boxes[:, :, 2] -= boxes[:, :, 0]
        boxes[:, :, 3] -= boxes[:, :, 1]
        for box, score, label in zip(boxes[0], scores[0], labels[0]):
            if score < 0.05:
                break
            self.results.append({"image_id": self.gen.ids[self.n], "category_id": self.gen.id2category[label], "score": float(score),
                                 "bbox": box.tolist()})
        self.n += 1
        return out


class _Gen:
    def __init__(self, rng, n):
        self.ids = [int(i) for i in rng.choice(np.arange(100, 200), n, replace=False)]
        self.scales = [float(rng.uniform(0.3, 1.5)) for _ in range(n)]
        self.imgs = [torch.from_numpy(rng.standard_normal((3, 128, 128)).astype(np.float32)) for _ in range(n)]
        self.id2category = {k + 1: 3 * k + 2 for k in range(20)}             # 20 contiguous labels -> sparse category ids
        anns = []
        for i, s in zip(self.ids, self.scales):
            for _ in range(int(rng.integers(1, 6))):
                xy = rng.uniform(0, 80, 2) / s
                wh = rng.uniform(8, 60, 2) / s
                anns.append((i, int(rng.choice(list(self.id2category.values()))), [*xy, *wh], int(rng.random() < .15)))
        ds = dataset(anns, imgs=sorted(self.ids) + [999], cats=[3 * k + 2 for k in range(20)] + [77])
        self.coco = type("COCO", (), {"dataset": ds})()

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.imgs[i], None, None, self.scales[i]


def test_evaluate_coco_end_to_end(capsys):
    from test_model_gpu import randomize_norms

    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval()
    randomize_norms(model, 1)
    gen = _Gen(np.random.default_rng(7), 6)
    rec = _Recorder(model.to(DEV), gen)
    stats = evaluate_coco(gen, rec)
    printed = capsys.readouterr().out
    assert rec.n == 6 and len(rec.results) > 0
    assert "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in printed
    p, r = R.evaluate(gen.coco.dataset, rec.results, gen.ids)
    assert stats.tobytes() == R.summarize(p, r).tobytes()
