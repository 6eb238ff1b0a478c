"""VOC AP evaluation: the numpy restatement against the reference's recorded APs (g12), and the device-only contract of the
drop-in module -- no GPU needed."""
import numpy as np
import pytest
import torch

import eval_ap_ref as R
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd._lib import FdError


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    m = ~np.isnan(a)
    assert np.array_equal(a[m].view(np.int64), b[m].view(np.int64)), (a, b)


def test_pairwise_sum_is_numpy_sum():
    rng = np.random.default_rng(3)
    for n in list(range(0, 40)) + [127, 128, 129, 135, 136, 255, 256, 257, 300, 1000, 1031, 4099]:
        a = rng.random(n) * 10.0 ** rng.integers(-8, 8, n)
        assert R.pairwise_sum(a).view(np.int64) == np.float64(np.sum(a)).view(np.int64), n


def test_restatement_reproduces_reference_g12(golden):
    g = golden("g12_eval_ap")
    num_cls = int(g["num_cls"])
    lists = R.unpad(g["det_scores"], g["det_classes"], g["det_boxes"], g["det_counts"], g["gt_boxes"], g["gt_classes"], g["gt_counts"])
    # evaluate's order: sort_by_score per image, then eval_ap_2d on the lists as given
    ap, n_gt, n_pred, n_tp = R.eval_ap(*lists, g["thresholds"], num_cls)
    _same_bits(ap, g["ap"])
    assert n_gt[10] > 300 and n_tp[0, 10] > 128          # label 11: the pairwise recursion, not only one 128-block
    assert np.isnan(g["ap"][:, 7]).all() and (g["ap"][:, 8] == 0).all()
    assert g["ap"][0, 9] == 1.0 and g["ap"][1, 9] < 1.0   # IoU exactly 0.5 passes 0.5, fails float32(0.55)
    assert int(str(g["numpy_version"]).split(".")[0]) >= 2


def test_evaluator_rejects_cpu_tensors_before_the_library(monkeypatch):
    from pytorch_object_detection_amd.test import VOCEvaluator

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", boom)
    ev = VOCEvaluator(num_cls=21)
    with pytest.raises(FdError):
        ev.add(torch.rand(1, 4), torch.ones(1, 4, dtype=torch.int64), torch.rand(1, 4, 4), None, torch.rand(1, 2, 4),
               torch.ones(1, 2, dtype=torch.int64))
    assert ev.num_images == 0


def test_eval_ap_op_rejects_cpu_tensors():
    from pytorch_object_detection_amd import ops
    with pytest.raises(FdError):
        ops.eval_ap(torch.rand(1, 4), torch.ones(1, 4, dtype=torch.int64), torch.rand(1, 4, 4), None, torch.rand(1, 2, 4),
                    torch.ones(1, 2, dtype=torch.int64), None, 21, (0.5,))


def test_workspace_limits_and_linear_growth():
    lib = _lib.lib()
    a = lib.fd_eval_ap_workspace_bytes(1000, 1000, 50, 21, 1)
    b = lib.fd_eval_ap_workspace_bytes(2000, 1000, 50, 21, 1)
    assert 0 < a < b <= 2 * a + 4096
    assert a < 40 * 1000 * 1000
    assert lib.fd_eval_ap_workspace_bytes(10000, 1024, 512, 128, 16) > 0
    for bad in ((1, 1025, 1, 21, 1), (1, 1, 513, 21, 1), (1, 1, 1, 129, 1), (1, 1, 1, 21, 17), (0, 1, 1, 21, 1), (1, 1, 1, 1, 1)):
        assert lib.fd_eval_ap_workspace_bytes(*bad) == -1, bad
    rc = lib.fd_eval_ap(None, None, None, None, 1, 2048, None, None, None, 1, 21, None, 1, 0, None, None, None, None, None, None)
    assert rc == _lib.E_UNSUPPORTED
    assert b"1024" in lib.fd_last_error()


def test_sort_by_score_matches_reference_semantics():
    from pytorch_object_detection_amd.test import sort_by_score
    b = [np.arange(12, dtype=np.float32).reshape(3, 4)]
    lab = [np.array([1, 2, 3])]
    s = [np.array([0.2, 0.9, 0.5], np.float32)]
    ob, ol, os_ = sort_by_score(b, lab, s)
    assert ol[0].tolist() == [2, 3, 1] and os_[0].tolist() == pytest.approx([0.9, 0.5, 0.2]) and ob[0][0].tolist() == [4, 5, 6, 7]


def test_evaluator_rows_after_reset_hold_only_the_new_batch(monkeypatch):
    """reset() keeps the buffers: a narrower batch added afterwards must not inherit the earlier batch's wider columns
    (buffer contents checked on host tensors, with the device check bypassed; the GPU suite checks compute())."""
    from pytorch_object_detection_amd import ops
    from pytorch_object_detection_amd.test import VOCEvaluator
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    ev = VOCEvaluator(num_cls=21)
    ev.add(torch.rand(2, 8), torch.full((2, 8), 3, dtype=torch.int64), torch.rand(2, 8, 4), None, torch.rand(2, 5, 4),
           torch.full((2, 5), 3, dtype=torch.int64))
    ev.reset()
    ev.add(torch.rand(1, 2), torch.full((1, 2), 7, dtype=torch.int64), torch.rand(1, 2, 4), None, torch.rand(1, 1, 4),
           torch.full((1, 1), 7, dtype=torch.int64))
    _, c, _, _, gc = ev._bufs
    assert c[0].tolist() == [7, 7] + [0] * 6 and gc[0].tolist() == [7, -1, -1, -1, -1]
    assert ev.num_images == 1
