"""Host-side checks of MNFCOS training on the HIP path: the dilated depthwise weight-gradient entry points exist and validate their
arguments without a launch, and training is opt-in (`hip_train`, `enable_training()`)."""
import ctypes

import pytest
import torch

from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd._lib import FdError, Segs
from pytorch_object_detection_amd.model.modules.modules import MNBlock
from pytorch_object_detection_amd.model.od import MNFCOS
from pytorch_object_detection_amd.model.od.MNFcos import LieghtWeightFeaturePyramid_old, MNHeadFCOS

NEW = ("fd_dwconv_dilated_bwd_weight_nhwc", "fd_dwconv_dilated_wgrad_workspace_bytes")


def test_library_exports_the_dilated_weight_gradient():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_workspace_query_rejects_bad_arguments():
    lib = _lib.lib()
    segs = Segs.make(2, [(8, 8), (4, 4)])
    for K in (3, 5, 7):
        nb = lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(segs), 128, K)
        assert nb >= K * K * 128 * 4 and nb % 16 == 0
    assert lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(segs), 128, 4) == -1        # bad K
    assert lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(segs), 128, 9) == -1
    assert lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(segs), 130, 3) == -1        # C % 4
    bad = Segs()                                                                               # an empty table
    assert lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(bad), 128, 3) == -1
    assert lib.fd_dwconv_dilated_wgrad_workspace_bytes(None, 128, 3) == -1


def test_weight_gradient_entry_point_validates_on_the_host():
    """Bad arguments return FD_E_* before any launch (this runs without a GPU)."""
    lib = _lib.lib()
    segs = Segs.make(2, [(8, 8), (4, 4)])
    p = ctypes.c_void_p(4096)           # aligned, never dereferenced: every case below is rejected first
    fn = lib.fd_dwconv_dilated_bwd_weight_nhwc
    assert fn(p, 128, 0, p, 128, 0, p, 128, 4, 1, None, 0, ctypes.byref(segs), p, None) < 0     # K = 4
    assert fn(p, 128, 0, p, 128, 0, p, 128, 3, 9, None, 0, ctypes.byref(segs), p, None) < 0     # dil = 9
    assert fn(p, 128, 0, p, 128, 0, p, 128, 3, 0, None, 0, ctypes.byref(segs), p, None) < 0     # dil = 0
    assert fn(p, 130, 0, p, 130, 0, p, 130, 3, 1, None, 0, ctypes.byref(segs), p, None) < 0     # C % 4
    assert fn(p, 128, 0, p, 128, 0, p, 128, 3, 1, None, 0, ctypes.byref(segs), None, None) < 0  # no workspace
    assert fn(p, 128, 0, p, 128, 0, None, 128, 3, 1, None, 0, ctypes.byref(segs), p, None) < 0  # no output
    assert fn(p, 128, 0, p, 128, 0, p, 128, 3, 1, None, 2, ctypes.byref(segs), p, None) < 0     # layout
    assert fn(p, 128, 0, p, 128, 0, p, 128, 3, 1, None, 0, None, p, None) < 0                   # no table
    assert lib.fd_last_error()


def test_training_is_opt_in():
    model = MNFCOS([2048, 1024, 512], 20, 256)
    blocks = [m for m in model.modules() if isinstance(m, MNBlock)]
    assert len(blocks) == 8                         # MNB1_P3 (never called), MNB3..7, head.block1 / block2
    assert MNBlock.hip_train is False and LieghtWeightFeaturePyramid_old.hip_train is False and MNHeadFCOS.hip_train is False
    assert not model.hip_train and not model.FeaturePyramidNetwork.hip_train and not model.head.hip_train
    assert not any(b.hip_train for b in blocks)
    assert model.backbone.conv1.weight.requires_grad
    with pytest.warns(UserWarning, match="freezes the 7x7 stem"):       # an optimizer built earlier would hold a dead parameter
        assert model.enable_training() is model
    assert model.hip_train and model.FeaturePyramidNetwork.hip_train and model.head.hip_train
    assert all(b.hip_train for b in blocks)
    assert not model.backbone.conv1.weight.requires_grad        # the Cin = 3 stem has no HIP backward: frozen by the switch
    assert model.backbone.extract_feature.layer1[0].conv1.weight.requires_grad
    # the containers on their own
    fpn = LieghtWeightFeaturePyramid_old([128, 64, 32], 32)
    assert fpn.enable_training() is fpn and fpn.hip_train and all(m.hip_train for m in fpn.modules() if isinstance(m, MNBlock))
    head = MNHeadFCOS(32, 20)
    assert head.enable_training() is head and head.block1.hip_train and head.block2.hip_train
    assert not MNBlock(32, 32, 3, 1, 2).hip_train               # other instances are untouched


def test_hip_training_forward_is_gpu_only():
    model = MNFCOS([2048, 1024, 512], 20, 256).enable_training().train()
    with pytest.raises(FdError, match="GPU only"):
        model(torch.zeros(1, 3, 128, 128))
    blk = MNBlock(32, 32, 3, 1, 2)
    blk.hip_train = True
    with pytest.raises(FdError, match="GPU only"):
        blk.train()(torch.zeros(1, 32, 8, 8))
