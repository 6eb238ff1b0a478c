"""VOC AP on the device (fd_eval_ap / pytorch_object_detection_amd.test) against the reference's recorded APs (g12) and the numpy
restatement (tests/eval_ap_ref.py): bit-identical per-label AP, NaN in the same places, identical TP counts."""
import numpy as np
import pytest
import torch

import eval_ap_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd.test import VOCEvaluator, eval_ap_2d, evaluate, sort_by_score

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same_bits(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    m = ~np.isnan(a)
    assert np.array_equal(a[m].view(np.int64), b[m].view(np.int64)), (what, a, b)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pad(imgs):
    """[(gt_boxes, gt_labels, det_boxes, det_labels, det_scores)] -> padded numpy arrays (class 0 / -1 padding) + counts."""
    N = len(imgs)
    K = max([len(im[4]) for im in imgs] + [1])
    G = max([len(im[1]) for im in imgs] + [1])
    s, c, b = np.zeros((N, K), np.float32), np.zeros((N, K), np.int64), np.zeros((N, K, 4), np.float32)
    gb, gc = np.zeros((N, G, 4), np.float32), np.full((N, G), -1, np.int64)
    dn = np.zeros(N, np.int32)
    for i, (g, gl, d, dl, ds) in enumerate(imgs):
        k, m = len(ds), len(gl)
        dn[i] = k
        s[i, :k], c[i, :k], b[i, :k] = ds, dl, np.asarray(d, np.float32).reshape(k, 4)
        gb[i, :m], gc[i, :m] = np.asarray(g, np.float32).reshape(m, 4), gl
    return s, c, b, dn, gb, gc


def _device(imgs, thresholds, num_cls):
    s, c, b, dn, gb, gc = _pad(imgs)
    ev = VOCEvaluator(num_cls, thresholds)
    ev.add(_d(s), _d(c), _d(b), _d(dn), _d(gb), _d(gc))
    return ev.compute()


def _ref(imgs, thresholds, num_cls):
    return R.eval_ap([im[0] for im in imgs], [im[1] for im in imgs], [im[2] for im in imgs], [im[3] for im in imgs],
                     [im[4] for im in imgs], thresholds, num_cls)


def _check(imgs, thresholds, num_cls):
    res = _device(imgs, thresholds, num_cls)
    ap, n_gt, n_pred, n_tp = _ref(imgs, thresholds, num_cls)
    _same_bits(res["ap"], ap)
    assert np.array_equal(res["n_gt"], n_gt) and np.array_equal(res["n_pred"], n_pred) and np.array_equal(res["n_tp"], n_tp)
    return res


def _f(*r):
    return np.array(r, np.float32).reshape(-1, 4)


def _i(*r):
    return np.array(r, np.int64)


def _s(*r):
    return np.array(r, np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# (a) the reference's recorded APs
def test_g12_reference_ap_bit_identical(golden):
    g = golden("g12_eval_ap")
    num_cls, thr = int(g["num_cls"]), [float(t) for t in g["thresholds"]]
    gtb, gtl, pb, pl, ps = R.unpad(g["det_scores"], g["det_classes"], g["det_boxes"], g["det_counts"], g["gt_boxes"], g["gt_classes"],
                                   g["gt_counts"])
    # eval_ap_2d, fed as evaluate feeds it: sort_by_score first
    sb, sl, ss = sort_by_score(pb, pl, ps)
    for t, th in enumerate(thr):
        res = eval_ap_2d(gtb, gtl, sb, sl, ss, th, num_cls)
        assert sorted(res) == list(range(1, num_cls)) and all(isinstance(v, np.float64) for v in res.values())
        _same_bits([res[lab] for lab in range(1, num_cls)], g["ap"][t], f"eval_ap_2d thr {th}")
    # VOCEvaluator: padded batches with counts, all thresholds in one call
    ev = VOCEvaluator(num_cls, thr)
    ev.add(_d(g["det_scores"]), _d(g["det_classes"]), _d(g["det_boxes"]), _d(g["det_counts"]), _d(g["gt_boxes"]), _d(g["gt_classes"]))
    out = ev.compute()
    _same_bits(out["ap"], g["ap"], "VOCEvaluator")
    for t in range(len(thr)):
        assert np.isnan(out["mAP"][t])      # label 8 is NaN: the mAP is NaN, as in the reference
    ref = R.eval_ap(gtb, gtl, pb, pl, ps, thr, num_cls)
    assert np.array_equal(out["n_tp"], ref[3]) and np.array_equal(out["n_gt"], ref[1]) and np.array_equal(out["n_pred"], ref[2])


# --------------------------------------------------------------------------------------------------------------------------------
# (b) one test per quirk of the contract
def test_taken_gt_is_false_positive_without_fallback():
    imgs = [(_f(0, 0, 10, 10, 0, 0, 10, 9), _i(1, 1), _f(0, 0, 10, 10, 0, 0, 10, 9.9), _i(1, 1), _s(0.9, 0.8))]
    res = _check(imgs, [0.5], 3)
    assert res["n_tp"][0, 0] == 1 and res["ap"][0, 0] == 0.5     # a fall-back to the second box would give 2 TPs, AP 1.0


def test_nan_iou_is_never_a_tp_and_wins_the_argmax():
    imgs = [(_f(5, 5, 5, 5, 0, 0, 10, 10), _i(1, 1), _f(5, 5, 5, 5, 0, 0, 10, 10), _i(1, 1), _s(0.9, 0.8)),
            (_f(0, 0, 10, 10, 5, 5, 5, 5), _i(1, 1), _f(5, 5, 5, 5), _i(1), _s(0.7))]
    res = _check(imgs, [0.5], 2)
    assert res["n_tp"][0, 0] == 1 and res["n_gt"][0] == 4


def test_nan_and_zero_labels_and_nan_map():
    imgs = [(_f(0, 0, 10, 10, 20, 20, 30, 30), _i(1, 3), _f(0, 0, 10, 10, 50, 50, 60, 60), _i(1, 2), _s(0.9, 0.8))]
    res = _check(imgs, [0.5], 5)
    assert res["ap"][0, 0] == 1.0                     # label 1: one GT, one TP
    assert np.isnan(res["ap"][0, 1])                  # label 2: predictions, no GT
    assert res["ap"][0, 2] == 0.0                     # label 3: GT, no predictions
    assert res["ap"][0, 3] == 0.0                     # label 4: neither
    assert np.isnan(res["mAP"][0])


def test_ignored_labels_and_padding_rows():
    base = [(_f(0, 0, 10, 10, 20, 20, 40, 40), _i(1, 2), _f(0, 0, 10, 10, 21, 20, 40, 40), _i(1, 2), _s(0.9, 0.6))]
    noisy = [(_f(0, 0, 10, 10, 0, 0, 10, 10, 20, 20, 40, 40, 0, 0, 10, 10, 0, 0, 10, 10), _i(1, 0, 2, -1, 7),
              _f(0, 0, 10, 10, 0, 0, 10, 10, 21, 20, 40, 40, 0, 0, 10, 10, 0, 0, 10, 10), _i(1, -1, 2, 0, 9),
              _s(0.9, 0.95, 0.6, 0.99, 0.97))]
    a = _check(base, [0.5, 0.75], 4)
    b = _check(noisy, [0.5, 0.75], 4)
    for k in ("ap", "n_gt", "n_pred", "n_tp"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # rows >= det_counts do not take part, whatever their label
    s, c, bx, dn, gb, gc = _pad(base)
    s2 = np.concatenate([s, np.full((1, 3), 0.99, np.float32)], 1)
    c2 = np.concatenate([c, np.full((1, 3), 1, np.int64)], 1)
    b2 = np.concatenate([bx, np.tile(_f(0, 0, 10, 10), (1, 3, 1))], 1)
    ev = VOCEvaluator(4, [0.5, 0.75])
    ev.add(_d(s2), _d(c2), _d(b2), _d(dn), _d(gb), _d(gc))
    r = ev.compute()
    for k in ("ap", "n_gt", "n_pred", "n_tp"):
        assert a[k].tobytes() == r[k].tobytes(), k


def test_empty_inputs():
    ev = VOCEvaluator(21)
    r = ev.compute()                                     # nothing added
    assert (r["ap"] == 0).all() and r["mAP"][0] == 0.0 and (r["n_pred"] == 0).all()
    ev.add(torch.zeros(2, 0, device=DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV), torch.zeros(2, 0, 4, device=DEV), None,
           torch.zeros(2, 0, 4, device=DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    r = ev.compute()
    assert (r["ap"] == 0).all() and ev.num_images == 2
    imgs = [(_f(), _i(), _f(), _i(), _s()), (_f(0, 0, 5, 5), _i(2), _f(), _i(), _s()), (_f(), _i(), _f(0, 0, 5, 5), _i(3), _s(0.5))]
    res = _check(imgs, [0.5], 4)
    assert res["ap"][0, 1] == 0.0 and np.isnan(res["ap"][0, 2])
    d = eval_ap_2d([], [], [], [], [], 0.5, 4)
    assert d == {1: 0.0, 2: 0.0, 3: 0.0}


def test_reset_then_narrower_batch_equals_fresh_evaluator():
    wide = [(_f(0, 0, 10, 10, 20, 20, 30, 30, 40, 40, 50, 50), _i(3, 3, 3), _f(0, 0, 10, 10, 20, 20, 30, 30, 40, 40, 50, 50, 1, 1, 9, 9),
             _i(3, 3, 3, 3), _s(0.9, 0.8, 0.7, 0.6))] * 2
    narrow = [(_f(0, 0, 10, 10), _i(7), _f(0, 0, 10, 10), _i(7), _s(0.5))]
    ev = VOCEvaluator(21, [0.5, 0.75])
    s, c, b, dn, gb, gc = _pad(wide)
    ev.add(_d(s), _d(c), _d(b), None, _d(gb), _d(gc))
    ev.compute()
    ev.reset()
    r = ev.compute()                                     # nothing added since reset(): every label 0, nothing counted
    assert (r["ap"] == 0).all() and (r["n_pred"] == 0).all() and (r["n_gt"] == 0).all()
    s, c, b, dn, gb, gc = _pad(narrow)
    ev.add(_d(s), _d(c), _d(b), None, _d(gb), _d(gc))
    got = ev.compute()
    fresh = _device(narrow, [0.5, 0.75], 21)
    for k in ("ap", "n_gt", "n_pred", "n_tp"):
        assert got[k].tobytes() == fresh[k].tobytes(), k
    assert got["n_pred"][2] == 0 and got["n_gt"][2] == 0 and got["n_tp"][0, 6] == 1


def test_nan_coordinates_give_nan_iou():
    # GT 0 has a NaN coordinate: its IoU is NaN (np.minimum / np.maximum propagate it), so it wins the argmax and the detection
    # is a false positive, although GT 1 matches it exactly
    imgs = [(_f(np.nan, 0, 10, 10, 0, 0, 10, 10), _i(1, 1), _f(0, 0, 10, 10), _i(1), _s(0.9)),
            (_f(0, 0, 10, 10), _i(1), _f(0, 0, 10, np.nan, 0, 0, 10, 10), _i(1, 1), _s(0.8, 0.7))]
    res = _check(imgs, [0.5], 2)
    assert res["n_tp"][0, 0] == 1       # only image 1's second detection


def test_equal_scores_keep_image_order():
    # label 1, score 0.5 in both images: a TP in image 0, a false positive in image 1.  Stable order (TP first): AP 1.0;
    # the other order would give 0.5
    imgs = [(_f(0, 0, 10, 10), _i(1), _f(0, 0, 10, 10), _i(1), _s(0.5)),
            (_f(), _i(), _f(0, 0, 10, 10), _i(1), _s(0.5))]
    res = _check(imgs, [0.5], 2)
    assert res["ap"][0, 0] == 1.0
    res = _check(imgs[::-1], [0.5], 2)
    assert res["ap"][0, 0] == 0.5


# --------------------------------------------------------------------------------------------------------------------------------
def _scale_data(seed, n_img, n_det, num_cls, max_gt=10):
    rng = np.random.default_rng(seed)
    total = n_img * n_det
    pool = np.unique(rng.random(3 * total).astype(np.float32) * np.float32(0.95) + np.float32(0.05))
    pool = rng.permutation(pool)[:total]
    assert len(pool) == total
    imgs = []
    for i in range(n_img):
        g = int(rng.integers(1, max_gt + 1))
        xy = rng.uniform(0, 500, (g, 2)).astype(np.float32)
        gb = np.concatenate([xy, xy + rng.uniform(8, 150, (g, 2)).astype(np.float32)], 1)
        gl = rng.integers(1, num_cls, g)
        src = rng.integers(0, g, n_det)
        db = gb[src] + rng.normal(0, 6, (n_det, 4)).astype(np.float32)
        far = rng.random(n_det) < 0.5
        rxy = rng.uniform(0, 500, (n_det, 2)).astype(np.float32)
        db[far] = np.concatenate([rxy, rxy + rng.uniform(8, 150, (n_det, 2)).astype(np.float32)], 1)[far]
        dl = np.where(rng.random(n_det) < 0.7, gl[src], rng.integers(1, num_cls, n_det))
        imgs.append((gb.astype(np.float32), gl.astype(np.int64), db.astype(np.float32), dl.astype(np.int64), pool[i * n_det:(i + 1) * n_det]))
    return imgs


# (c) scale against the restatement
def test_scale_against_restatement():
    imgs = _scale_data(5, 1000, 300, 21)
    res = _check(imgs, [0.5], 21)
    assert res["n_tp"].sum() > 1000


# (d) ten thresholds in one call == ten single-threshold calls
def test_multi_threshold_equals_single_calls():
    imgs = _scale_data(6, 300, 200, 21)
    thr = [0.5 + 0.05 * i for i in range(10)]
    many = _device(imgs, thr, 21)
    for t, th in enumerate(thr):
        one = _device(imgs, [th], 21)
        assert one["ap"][0].tobytes() == many["ap"][t].tobytes() and np.array_equal(one["n_tp"][0], many["n_tp"][t]), th
    assert len(set(many["n_tp"].sum(1).tolist())) > 5


# (e) ragged batches without host syncs, deterministic bytes
def test_ragged_batches_no_sync_deterministic():
    imgs = _scale_data(7, 120, 60, 21, max_gt=12)
    rng = np.random.default_rng(8)
    thr = [0.5, 0.75]
    whole = _device(imgs, thr, 21)
    batches = []
    i = 0
    while i < len(imgs):
        n = int(rng.integers(1, 9))
        chunk = imgs[i:i + n]
        i += n
        s, c, b, dn, gb, gc = _pad(chunk)
        kx, gx = int(rng.integers(0, 5)), int(rng.integers(0, 4))      # extra padding columns: K / G differ per batch
        s = np.pad(s, ((0, 0), (0, kx)), constant_values=0.99)
        c = np.pad(c, ((0, 0), (0, kx)), constant_values=1)          # beyond counts: ignored whatever the label
        b = np.pad(b, ((0, 0), (0, kx), (0, 0)))
        gb = np.pad(gb, ((0, 0), (0, gx), (0, 0)))
        gc = np.pad(gc, ((0, 0), (0, gx)), constant_values=-1)
        batches.append([_d(x) for x in (s, c, b, dn, gb, gc)])
    runs = []
    for _ in range(2):
        ev = VOCEvaluator(21, thr)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for bt in batches:
                ev.add(*bt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        runs.append(ev.compute())
    for k in ("ap", "n_gt", "n_pred", "n_tp"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes() == whole[k].tobytes(), k
    ev.reset()
    assert ev.num_images == 0


# --------------------------------------------------------------------------------------------------------------------------------
# (f) evaluate() end to end
class _Recorder(torch.nn.Module):
    """Runs the model and, on the same forward outputs, the reference's pipeline: FCOSHead -> ClipBoxes -> per-image numpy."""

    def __init__(self, model, strides):
        super().__init__()
        self.model = model
        self.strides = strides
        self.dets = []

    def forward(self, imgs):
        from pytorch_object_detection_amd.model.modules.head import ClipBoxes, FCOSHead
        out = self.model(imgs)
        s, c, b, n = FCOSHead(0.05, 0.6, 1000, self.strides).detect_padded(out)
        b = ClipBoxes()(imgs, b.clone())
        s, c, b, n = s.cpu().numpy(), c.cpu().numpy(), b.cpu().numpy(), n.cpu().numpy()
        for i in range(imgs.shape[0]):
            self.dets.append((b[i, :n[i]], c[i, :n[i]], s[i, :n[i]]))
        return out


def _loader(rng, n_img, bs):
    batches = []
    for i in range(0, n_img, bs):
        B = min(bs, n_img - i)
        G = int(rng.integers(2, 6))
        imgs = torch.from_numpy(rng.standard_normal((B, 3, 128, 128)).astype(np.float32))
        xy = rng.uniform(0, 90, (B, G, 2)).astype(np.float32)
        tb = np.concatenate([xy, xy + rng.uniform(16, 60, (B, G, 2)).astype(np.float32)], 2)
        tc = rng.integers(1, 21, (B, G)).astype(np.int64)
        for b in range(B):
            k = int(rng.integers(1, G + 1))
            tb[b, k:], tc[b, k:] = -1, -1                   # the collate's -1 padding
        batches.append((imgs, torch.from_numpy(tb), torch.from_numpy(tc)))
    return batches


@pytest.mark.parametrize("bs", [1, 3])
def test_evaluate_end_to_end(bs, capsys):
    from test_model_gpu import randomize_norms

    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval()
    randomize_norms(model, 1)
    model = model.to(DEV)
    rec = _Recorder(model, [8, 16, 32, 64])
    loader = _loader(np.random.default_rng(11), 6, bs)
    res = evaluate(rec, loader, False, False, torch.device(DEV))
    printed = capsys.readouterr().out
    assert "mAP:" in printed and "aeroplane:" in printed and "fps:" in printed
    assert len(rec.dets) == 6 and np.isfinite(res["fps"])                 # every image of every batch
    gt_b = [t[b][c[b] >= 0].numpy() for _, t, c in loader for b in range(t.shape[0])]
    gt_c = [c[b][c[b] >= 0].numpy() for _, t, c in loader for b in range(t.shape[0])]
    ap, n_gt, n_pred, n_tp = R.eval_ap(gt_b, gt_c, [d[0] for d in rec.dets], [d[1] for d in rec.dets], [d[2] for d in rec.dets], [0.5], 21)
    assert n_pred.sum() > 0 and n_gt.sum() > 0
    _same_bits([res["ap"][k] for k in range(1, 21)], ap[0])
    ref_map = R.mean_ap(ap[0])
    assert (np.isnan(ref_map) and np.isnan(res["mAP"])) or res["mAP"] == ref_map
    assert np.array_equal(res["result"]["n_tp"], n_tp) and np.array_equal(res["result"]["n_pred"], n_pred)
