"""The stem weight gradient without a device: the float64 restatement the GPU tests compare against, the ABI of the new entry points, the model switches."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stem_ref import stem_wgrad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_stem7x7_wgrad_workspace_bytes", "fd_stem7x7_bwd_weight_nhwc4")


def _autograd64(x, dy, y=None, scale=None):
    w = torch.zeros(dy.shape[1], 3, 7, 7, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x, w, stride=2, padding=3)
    if scale is not None:
        out = out * scale.view(1, -1, 1, 1)
    g = dy if y is None else dy * (y > 0)
    out.backward(g)
    return w.grad.numpy()


@pytest.mark.parametrize("shape", [(2, 16, 24), (1, 2, 2), (3, 6, 10)])
@pytest.mark.parametrize("mode", ["plain", "mask", "scale", "mask+scale"])
def test_restatement_matches_float64_autograd(shape, mode):
    N, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, 3, H, W, dtype=torch.float64, generator=g)
    dy = torch.randn(N, 64, H // 2, W // 2, dtype=torch.float64, generator=g)
    y = torch.randn(N, 64, H // 2, W // 2, dtype=torch.float64, generator=g) if "mask" in mode else None
    scale = torch.randn(64, dtype=torch.float64, generator=g) if "scale" in mode else None
    ref = _autograd64(x, dy, y, scale)
    got = stem_wgrad_ref(x.numpy(), dy.numpy(), None if y is None else y.numpy(), None if scale is None else scale.numpy())
    assert got.shape == (64, 3, 7, 7) and got.dtype == np.float64
    # rtol 1e-12, relative to the tensor: the two float64 sums run in different orders, so an element that cancels to near zero carries the rounding of its terms
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


def test_restatement_is_exact_on_integer_data():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (2, 3, 8, 12), generator=g).double()
    dy = torch.randint(-3, 4, (2, 64, 4, 6), generator=g).double()
    y = torch.randint(-1, 2, (2, 64, 4, 6), generator=g).double()
    scale = torch.randint(-2, 3, (64,), generator=g).double()
    assert np.array_equal(stem_wgrad_ref(x.numpy(), dy.numpy(), y.numpy(), scale.numpy()), _autograd64(x, dy, y, scale))


def test_new_symbols_in_header_exports_and_ctypes_table():
    from pytorch_object_detection_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/fcosdet.h"
        assert name in _lib.EXPORTS and name in _lib._SIGS, f"{name} is missing from _lib"
        assert hasattr(_lib.lib(), name), f"{name} is not exported by the library"
    res, args = _lib._SIGS["fd_stem7x7_bwd_weight_nhwc4"]
    assert res is ctypes.c_int32 and len(args) == 15
    assert _lib._SIGS["fd_stem7x7_wgrad_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int32] * 3)


def test_workspace_query_is_host_only_and_rejects_bad_sizes():
    from pytorch_object_detection_amd import _lib
    q = _lib.lib().fd_stem7x7_wgrad_workspace_bytes
    for bad in [(1, 31, 32), (1, 32, 31), (0, 32, 32), (-1, 32, 32), (1, 0, 32), (1, 32, 0), (1, -2, 32), (1, 1, 1)]:
        assert q(*bad) == -1, bad
    one = q(1, 2, 2)
    assert one > 0 and one % 16 == 0
    assert q(1, 32, 32) == one                      # one tile, one split
    assert q(16, 512, 512) > q(16, 256, 256) > one


def test_switch_is_off_by_default():
    from pytorch_object_detection_amd.model.od import FCOS, MNFCOS, HalfInvertedStageFCOS
    for m in (FCOS([2048, 1024, 512], 20, 256), HalfInvertedStageFCOS([512, 1024, 2048], 20, 256), MNFCOS([2048, 1024, 512], 20, 256)):
        assert m.backbone.hip_stem_train is False
        assert getattr(m.backbone.trunk, "hip_stem_train") is False
    m = FCOS([2048, 1024, 512], 20, 256)
    assert m.enable_stem_training() is m and m.backbone.hip_stem_train is True and m.backbone.trunk.hip_stem_train is True
    h = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256)
    assert h.enable_stem_training() is h and h.backbone.trunk.hip_stem_train is True
    assert FCOS([2048, 1024, 512], 20, 256).backbone.hip_stem_train is False            # (an instance switch, not a class one)


def test_mnfcos_train_stem_keeps_the_stem_trainable_without_a_warning():
    from pytorch_object_detection_amd.model.od import MNFCOS
    m = MNFCOS([2048, 1024, 512], 20, 256)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert m.enable_training(train_stem=True) is m
    assert m.backbone.conv1.weight.requires_grad and m.hip_train and m.backbone.trunk.hip_stem_train is True
    d = MNFCOS([2048, 1024, 512], 20, 256)
    with pytest.warns(UserWarning, match="freezes the 7x7 stem"):
        d.enable_training()
    assert not d.backbone.conv1.weight.requires_grad and d.backbone.hip_stem_train is False
