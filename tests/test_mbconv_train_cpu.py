"""MBConv training, the parts that need no GPU: the closed-form depthwise gradients of tests/mbconv_ref.py against float64 autograd over the whole geometry
table, the static "SAME" padding of B0 / B3, the new entry points' host-side checks, and the host behaviour of FCOS.enable_training()."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import mbconv_ref as M
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd.model.backbone.efficientnetv1 import EfficientNetV1, static_same_padding
from pytorch_object_detection_amd.model.od import FCOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_dwconv2d_bwd_data_nhwc", "fd_dwconv2d_bwd_weight_nhwc", "fd_dwconv2d_wgrad_workspace_bytes")


def test_table_is_complete():
    assert len(M.GEOMS) == 6 and len(M.CASES) == 6 * 3 + 2
    assert ((3, 2, (0, 1)), (8, 7)) in M.CASES and ((5, 2, (2, 2)), (9, 14)) in M.CASES


@pytest.mark.parametrize("geom,hw", M.CASES, ids=lambda v: "-".join(str(i) for i in v).replace(" ", ""))
def test_closed_forms_match_float64_autograd(geom, hw):
    k, s, pad = geom
    c = M.case(geom, hw, 4)
    x = c["x"].clone().requires_grad_(True)
    w = c["w"].clone().requires_grad_(True)
    (M.dw_forward(x, w, s, pad) * c["dy"]).sum().backward()
    torch.testing.assert_close(c["dx"], x.grad, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(c["dw"], w.grad, atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("geom,hw", [((3, 2, (0, 1)), (8, 7)), ((5, 2, (2, 2)), (9, 14))])
def test_uncovered_last_row_and_column(geom, hw):
    """(H + pads - k) % stride != 0 along one axis: the last PADDED row / column is read by no window.  With the table's pads (after >= stride - 1) that is
    always padding, never an input pixel; an output cropped by two rows and columns (what the entry points also take) does leave input rows and columns
    unreached, and their data gradient is exactly 0."""
    k, s, pad = geom
    H, W = hw
    assert (H + pad[0] + pad[1] - k) % s or (W + pad[0] + pad[1] - k) % s
    c = M.case(geom, hw, 4)
    dy = c["dy"][:, :, :-2, :-2]
    dx = M.dw_dgrad(dy, c["w"], s, pad, H, W)
    x = c["x"].clone().requires_grad_(True)
    (M.dw_forward(x, c["w"], s, pad)[:, :, :-2, :-2] * dy).sum().backward()
    torch.testing.assert_close(dx, x.grad, atol=1e-12, rtol=1e-12)
    assert not dx[:, :, -1].any() and not dx[:, :, :, -1].any() and dx.any()


def test_static_same_padding_of_b0_and_b3():
    """The (before, after) pads of the geometry table at the nominal sizes efficientnet_pytorch builds B0 (224) and B3 (300) for."""
    assert static_same_padding(112, 3, 1) == (1, 1) and static_same_padding(14, 5, 1) == (2, 2)
    assert static_same_padding(112, 3, 2) == (0, 1)          # B0 block 1: even nominal size
    assert static_same_padding(75, 3, 2) == (1, 1)           # an odd nominal size (the models between B0 and B3)
    assert static_same_padding(56, 5, 2) == (1, 2)           # B0 block 3
    assert static_same_padding(75, 5, 2) == (2, 2)           # B3 block 5
    for number, want in ((0, {(3, 1, (1, 1)), (5, 1, (2, 2)), (3, 2, (0, 1)), (5, 2, (1, 2))}),
                         (3, {(3, 1, (1, 1)), (5, 1, (2, 2)), (3, 2, (0, 1)), (5, 2, (2, 2))})):
        got = {(b.kernel, b.stride, tuple(b.pad)) for b in EfficientNetV1(number).model._blocks}
        assert got <= set(M.GEOMS), got - set(M.GEOMS)
        assert want <= got, want - got


def test_new_symbols_in_header_exports_and_library():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name), name
    assert len(_lib._SIGS["fd_dwconv2d_bwd_data_nhwc"][1]) == 19 and len(_lib._SIGS["fd_dwconv2d_bwd_weight_nhwc"][1]) == 21


def test_entry_points_validate_on_the_host():
    """Bad arguments return an error before any launch (no GPU here: the pointers are never dereferenced)."""
    lib = _lib.lib()
    q = lib.fd_dwconv2d_wgrad_workspace_bytes
    assert q(2, 4, 4, 144, 3) >= 9 * 144 * 4 and q(2, 4, 4, 144, 5) % 16 == 0
    for bad in [(0, 4, 4, 8, 3), (2, 0, 4, 8, 3), (2, 4, 0, 8, 3), (2, 4, 4, 126, 3), (2, 4, 4, 8, 7), (2, 4, 4, 0, 3)]:
        assert q(*bad) == -1, bad
    p = ctypes.c_void_p(4096)

    def dgrad(C=8, K=3, s=2, pt=0, pl=0, H=8, W=7, Ho=4, Wo=3, dy=p, dx=p, w=p, cs=8, co=0):
        return lib.fd_dwconv2d_bwd_data_nhwc(dy, cs, co, w, None, dx, cs, co, 2, H, W, C, K, s, pt, pl, Ho, Wo, None)

    def wgrad(C=8, K=3, s=2, pt=0, pl=0, H=8, W=7, Ho=4, Wo=3, ws=p, layout=0, cs=8):
        return lib.fd_dwconv2d_bwd_weight_nhwc(p, cs, 0, p, cs, 0, p, C, K, s, pt, pl, 2, H, W, Ho, Wo, None, layout, ws, None)

    for fn in (dgrad, wgrad):
        assert fn(K=7) == _lib.E_UNSUPPORTED and fn(s=3) == _lib.E_UNSUPPORTED and fn(K=4) == _lib.E_UNSUPPORTED
        assert fn(C=126) < 0 and fn(C=0) < 0 and fn(cs=6) < 0
        assert fn(Ho=5) == _lib.E_INVAL and fn(Wo=5) == _lib.E_INVAL          # the output reaches past the input
        assert fn(pt=3) == _lib.E_INVAL and fn(Ho=0) == _lib.E_INVAL
        assert b"fd_dwconv2d_bwd" in lib.fd_last_error()
    assert dgrad(dy=None) < 0 and dgrad(dx=ctypes.c_void_p(4100)) < 0 and dgrad(w=None) < 0 and dgrad(co=2) < 0
    assert wgrad(ws=None) == _lib.E_INVAL and wgrad(ws=ctypes.c_void_p(4104)) == _lib.E_INVAL and wgrad(layout=2) == _lib.E_INVAL


def test_enable_training_on_the_host():
    model = FCOS([320, 112, 40], 20, 64, efficientnet=True)
    keys = list(model.state_dict().keys())
    net = model.backbone.model
    assert net._conv_stem.weight.requires_grad and not model.hip_train
    with pytest.warns(UserWarning, match="freezes the EfficientNet stem"):
        assert model.enable_training() is model
    assert model.hip_train
    for m in (net._conv_stem, net._bn0, net._conv_head, net._bn1, net._fc):
        assert all(not p.requires_grad for p in m.parameters())
    assert net._blocks[0]._depthwise_conv.weight.requires_grad and net._blocks[3]._expand_conv.weight.requires_grad
    assert model.FPN.P3.weight.requires_grad
    assert list(model.state_dict().keys()) == keys
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.enable_training()                              # the stem is frozen already: nothing to warn about
    assert model.backbone.drop_connect_rate == 0.0 and net.drop_connect_rate == 0.0


def test_enable_training_is_a_no_op_on_the_resnet_trunk():
    model = FCOS([2048, 1024, 512], 20, 64)
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert model.enable_training() is model
    assert {n: p.requires_grad for n, p in model.named_parameters()} == flags and not model.hip_train
