"""Host-side checks of the deformable convolution: the float64 reference of tests/deform_ref.py against F.conv2d where the two must agree, the new
entry points in the header / export list and their validation without a launch, the DeformableConv2d module's contract, and the shared GPU-test
inputs: they reach every branch of the sampler and their coordinates are exact in fp32."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import deform_ref as D
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd._lib import FdError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_deform_im2col_nhwc", "fd_deform_bwd_nhwc")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("K,stride,pad,H,W", [(1, 1, 0, 5, 6), (3, 1, 1, 7, 10), (3, 2, 1, 7, 10), (3, 1, 0, 5, 6), (5, 1, 2, 6, 5), (5, 2, 2, 9, 8),
                                              (3, 2, 0, 7, 7), (3, 1, 1, 1, 1), (1, 2, 0, 4, 4)])
def test_reference_zero_offsets_is_conv2d(K, stride, pad, H, W):
    x, w, b = _rand(2, 8, H, W), _rand(4, 8, K, K, seed=1), _rand(4, seed=2)
    Ho, Wo = D.out_hw(H, W, K, stride, pad)
    y, cols = D.deform_conv2d(x, torch.zeros(2, 2 * K * K, Ho, Wo, dtype=torch.float64), w, b, stride, pad)
    ref = F.conv2d(x, w, b, stride, pad)
    assert y.shape == ref.shape and cols.shape == (2 * Ho * Wo, K * K * 8)
    assert float((y - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_integer_shift_identity(stride):
    """A constant integer offset (+1, -2) on every tap = F.conv2d(padding=0) of the zero-padded input cropped at the shifted window."""
    K, pad, H, W, dy, dx, big = 3, 1, 7, 10, 1, -2, 4
    x, w = _rand(2, 8, H, W), _rand(4, 8, K, K, seed=1)
    Ho, Wo = D.out_hw(H, W, K, stride, pad)
    off = torch.zeros(2, 2 * K * K, Ho, Wo, dtype=torch.float64)
    off[:, 0::2], off[:, 1::2] = dy, dx
    y, _ = D.deform_conv2d(x, off, w, None, stride, pad)
    xp = F.pad(x, (big, big, big, big))
    top, left = big - pad + dy, big - pad + dx
    crop = xp[:, :, top:top + (Ho - 1) * stride + K, left:left + (Wo - 1) * stride + K]
    ref = F.conv2d(crop, w, None, stride, 0)
    assert ref.shape == y.shape
    assert float((y - ref).abs().max()) < 1e-12


def test_reference_mask_linearity():
    geom = D.GEOMS[0]
    H, W, K, stride, pad = geom
    x, off, logits = (t.double() for t in D.make_inputs(geom, 8))
    mask = 2 * torch.sigmoid(logits)
    cols = D.deform_cols(x, off, mask, K, stride, pad)
    m2 = mask.clone()
    m2[:, 4] *= 2
    cols2 = D.deform_cols(x, off, m2, K, stride, pad)
    expect = cols.clone().view(-1, K * K, 8)
    expect[:, 4] *= 2
    assert torch.equal(cols2, expect.view_as(cols))
    assert torch.equal(D.deform_cols(x, off, None, K, stride, pad) * 1.0, D.deform_cols(x, off, torch.ones_like(mask), K, stride, pad))


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and name in _lib._SIGS and name in declared, name
        assert hasattr(lib, name), name


def test_entry_points_validate_on_the_host():
    """Bad arguments return FD_E_INVAL before any launch (this runs without a GPU); the pointers are never dereferenced."""
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)

    def im2col(x=(p, 32, 0), off=(p, 18, 0), mask=(p, 9, 0), act=0, cols=(p, 288, 0), B=2, H=7, W=10, C=32, K=3, stride=1, pad=1, dil=1):
        return lib.fd_deform_im2col_nhwc(*x, *off, *mask, act, *cols, B, H, W, C, K, stride, pad, dil, None)

    def bwd(dcols=(p, 288, 0), x=(p, 32, 0), off=(p, 18, 0), mask=(p, 9, 0), act=0, doff=(p, 18, 0), dmask=(p, 9, 0), dx=(p, 32, 0), C=32, K=3, stride=1, dil=1):
        return lib.fd_deform_bwd_nhwc(*dcols, *x, *off, *mask, act, *doff, *dmask, *dx, 2, 7, 10, C, K, stride, 1, dil, None)

    for fn in (im2col, bwd):
        assert fn(C=30) == _lib.E_INVAL                      # C % 4
        assert fn(K=8) == _lib.E_INVAL and fn(K=0) == _lib.E_INVAL
        assert fn(stride=5) == _lib.E_INVAL and fn(stride=0) == _lib.E_INVAL
        assert fn(dil=5) == _lib.E_INVAL
        assert fn(x=(p, 32, 2)) == _lib.E_INVAL              # co % 4
        assert fn(x=(p, 34, 0)) == _lib.E_INVAL              # cs % 4
        assert fn(x=(p, 32, 4)) == _lib.E_INVAL              # co + C > cs
        assert fn(x=(None, 32, 0)) == _lib.E_INVAL
        assert fn(off=(p, 18, 1)) == _lib.E_INVAL            # co + 2*K*K > cs
        assert fn(off=(None, 18, 0)) == _lib.E_INVAL
        assert fn(mask=(p, 8, 0)) == _lib.E_INVAL
        assert fn(act=2) == _lib.E_INVAL
    assert im2col(pad=8) == _lib.E_INVAL and im2col(cols=(p, 284, 0)) == _lib.E_INVAL and im2col(H=1, W=1, pad=0) == _lib.E_INVAL      # empty output
    assert bwd(dcols=(p, 288, 4)) == _lib.E_INVAL and bwd(doff=(None, 18, 0)) == _lib.E_INVAL and bwd(dx=(p, 32, 2)) == _lib.E_INVAL
    assert bwd(dmask=(None, 0, 0)) == _lib.E_INVAL and bwd(mask=(None, 0, 0)) == _lib.E_INVAL     # mask and d_mask come together
    assert lib.fd_last_error()


def test_module_contract():
    from pytorch_object_detection_amd.model.modules.modules import DeformableConv2d, deform_conv2d      # noqa: F401
    m = DeformableConv2d(256, 256, 3, padding=1, bias=True)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "offset_conv.weight": (18, 256, 3, 3), "offset_conv.bias": (18,), "modulator_conv.weight": (9, 256, 3, 3), "modulator_conv.bias": (9,),
        "regular_conv.weight": (256, 256, 3, 3), "regular_conv.bias": (256,)}
    for side in (m.offset_conv, m.modulator_conv):
        assert not side.weight.any() and not side.bias.any()
    assert m.regular_conv.weight.any()
    assert m.stride == (1, 1) and m.padding == 1
    assert "regular_conv.bias" not in DeformableConv2d(32, 8, 3, stride=2).state_dict()
    with pytest.raises(FdError):
        m(torch.zeros(1, 256, 4, 4))
    with pytest.raises(FdError):
        deform_conv2d(torch.zeros(1, 32, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(8, 32, 3, 3), padding=1)


@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("geom", D.GEOMS)
def test_shared_inputs_reach_every_branch(geom, seed):
    H, W, K, stride, pad = geom
    _, off, _ = D.make_inputs(geom, 32, seed=seed)
    assert torch.equal(off, D.make_inputs(geom, 256, seed=seed)[1])
    outside, partial, full = D.tap_classes(off, H, W, K, stride, pad)
    print(f"{geom}: outside {outside:.2f} partial {partial:.2f} inside {full:.2f}")
    assert outside >= 0.10 and partial >= 0.10
    if (H, W) == (1, 1):
        assert full == 0.0          # a one-pixel map has no sample with four corners inside
    else:
        assert full >= 0.10


def test_integer_offset_case_reaches_every_branch():
    """The one integer-offset case (D.INTEGER_GEOM) exists for the ly = 0 / lx = 0 side of the derivative; there only the map's last row / column is
    "partial", so the shares are smaller: each class must be met."""
    H, W, K, stride, pad = D.INTEGER_GEOM
    for seed in D.SEEDS:
        _, off, _ = D.make_inputs(D.INTEGER_GEOM, 32, seed=seed, integer=True)
        outside, partial, full = D.tap_classes(off, H, W, K, stride, pad)
        print(f"integer offsets, seed {seed}: outside {outside:.2f} partial {partial:.2f} inside {full:.2f}")
        assert outside >= 0.05 and partial >= 0.05 and full >= 0.05


@pytest.mark.parametrize("geom", D.GEOMS)
def test_shared_coordinates_are_exact_in_fp32(geom):
    """base + offset is exact in fp32 as in float64, so floor() and the fractions cannot differ between the device and the reference."""
    H, W, K, stride, pad = geom
    for integer in (False, True):
        _, off, _ = D.make_inputs(geom, 32, integer=integer)
        y32, x32 = D.coords(off, H, W, K, stride, pad)
        y64, x64 = D.coords(off.double(), H, W, K, stride, pad)
        assert y32.dtype == torch.float32 and torch.equal(y32.double(), y64) and torch.equal(x32.double(), x64)
        frac = y64 - torch.floor(y64)
        assert bool((frac == 0).all()) if integer else bool(((frac * 8) % 2 == 1).all())
