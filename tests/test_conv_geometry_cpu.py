"""What can be checked of the dense-conv geometry handling without a GPU: the coverage predicates against torch's own output shape, the parity
classes of the strided data gradient against a float64 transposed conv, and the float64 reference (tests/conv_ref.py) against torch.nn.grad."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_ref as R
from pytorch_object_detection_amd import ops, train_ops as T
from pytorch_object_detection_amd._lib import Segs

H, W, B = 9, 9, 1


def _modules():
    """(id, module): dense (32 -> 32) and depthwise (32 channels) nn.Conv2d over int, tuple and string paddings."""
    out = []
    for groups in (1, 32):
        kind = "dense" if groups == 1 else "dw"
        for k, s, d in itertools.product((1, 2, 3, 4, 5), (1, 2), (1, 2)):
            pads = [0, 1, k // 2, d * (k - 1) // 2, d * (k - 1), d * (k - 1) + 1, (1, 1), (0, 1), (2, 1), (1, 0), (1, 2), "valid"] + (["same"] if s == 1 else [])   # ('same' is stride 1 only)
            # (p, q) with p the padding a predicate may look for and q next to it: a predicate that reads padding[0] alone admits these
            pads += [(k // 2, k // 2 + 1), (k // 2 + 1, k // 2), (d * (k - 1) // 2, d * (k - 1) // 2 + 1)]
            for p in dict.fromkeys(pads):
                name = f"{kind}-k{k}s{s}d{d}p{p}".replace(" ", "")
                out.append((name, nn.Conv2d(32, 32, k, s, p, d, groups, bias=False)))
    return out


MODULES = _modules()


@pytest.mark.parametrize("name,m", MODULES, ids=[n for n, _ in MODULES])
def test_a_covered_module_gets_the_geometry_torch_computes(name, m):
    """Either the predicates decline the module, or the (k, stride, pad, dil) the node hands to the kernel reproduces m(x).shape: the kernel geometry from
    train_ops._pad_of, the output size from ops.conv_out_segs (dense) or the input size (the depthwise node writes a map of its input's size)."""
    x = torch.zeros(B, 32, H, W)
    want = tuple(m(x).shape[2:])
    dense, dw = T._dense_ok(m, x), T._dw_ok(m, x)
    assert T.covered(m, None, x) == (dense or dw)
    if dense:
        pad = T._pad_of(m)
        assert isinstance(pad, int) and pad >= 0
        so = ops.conv_out_segs(Segs.make(B, [(H, W)]), m.kernel_size[0], m.stride[0], pad, m.dilation[0])
        assert so.level_hw()[0] == want, f"{name}: the node would return {so.level_hw()[0]}, the module returns {want}"
    if dw:
        assert (H, W) == want and m.kernel_size == (3, 3) and T._pad_of(m) == 1
    if m.groups == 32 and T._dw_dilated_ok(m, x):        # the dilated depthwise node (MNBlock) writes a map of its input's size too
        assert (H, W) == want


def test_string_padding_rule():
    x = torch.zeros(B, 32, H, W)
    for k, d in itertools.product((1, 2, 3, 4, 5), (1, 2)):
        same, valid = nn.Conv2d(32, 32, k, 1, "same", d), nn.Conv2d(32, 32, k, 1, "valid", d)
        assert T._pad_of(valid) == 0 and T._dense_ok(valid, x)
        if (d * (k - 1)) % 2:        # torch pads asymmetrically: not a kernel geometry
            assert T._pad_of(same) is None and not T._dense_ok(same, x) and not T.covered(same, None, x)
        else:
            assert T._pad_of(same) == d * (k - 1) // 2 and T._dense_ok(same, x)
    assert not T._dw_ok(nn.Conv2d(32, 32, 3, 1, "valid", 1, 32, bias=False), x)
    assert T._dw_ok(nn.Conv2d(32, 32, 3, 1, "same", 1, 32, bias=False), x)
    for p in ((1, 0), (1, 2)):       # the depthwise node writes a map of its input's size: only padding (1, 1) does that
        m = nn.Conv2d(32, 32, 3, 1, p, 1, 32, bias=False)
        assert not T._dw_ok(m, x) and not T.covered(m, None, x)


# --------------------------------------------------------------------------- the parity classes of the strided data gradient
KSP = sorted({(g.kh, g.stride, g.pad) for g in R.GEOMS if g.square})


@pytest.mark.parametrize("k,stride,pad", KSP)
def test_strided_dgrad_classes_reproduce_the_transposed_conv(k, stride, pad):
    """dX assembled from ops.strided_dgrad_classes alone -- input row h = stride * i + a takes the taps r = r0 + stride * t, t < T, from dY row i + c - t --
    equals the float64 transposed conv (dilation 1, which is what the classes describe)."""
    gen = torch.Generator().manual_seed(k * 100 + stride * 10 + pad)
    Hh, Ww, Ci, Co = 11, 8, 2, 3
    Ho, Wo = R.out_hw(Hh, Ww, k, k, stride, pad, 1)
    w = torch.randn(Co, Ci, k, k, generator=gen, dtype=torch.float64)
    gy = torch.randn(1, Co, Ho, Wo, generator=gen, dtype=torch.float64)
    ref = R.dgrad(gy, w, (Hh, Ww), stride, pad, 1)
    cls = ops.strided_dgrad_classes(k, stride, pad)
    assert len(cls) == stride
    dx = torch.zeros(1, Ci, Hh, Ww, dtype=torch.float64)
    for h in range(Hh):
        a, i = h % stride, h // stride
        r0, Ta, ca = cls[a]
        assert r0 == (a + pad) % stride and Ta == len(range(r0, k, stride))
        for x_ in range(Ww):
            b, j = x_ % stride, x_ // stride
            q0, Tb, cb = cls[b]
            for t in range(Ta):
                for u in range(Tb):
                    yi, yj = i + ca - t, j + cb - u
                    if 0 <= yi < Ho and 0 <= yj < Wo:
                        dx[0, :, h, x_] += gy[0, :, yi, yj] @ w[:, :, r0 + stride * t, q0 + stride * u]
    np.testing.assert_allclose(dx.numpy(), ref.numpy(), atol=1e-12)
    if stride == 3 and k == 3 and pad == 1 and Hh == 11:       # (geometry 7's kind: rows read by no window stay exactly zero)
        assert float(R.dgrad(gy, w, (12, Ww), stride, pad, 1)[0, :, 11].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- the reference checks itself
def test_row_and_pyramid_helpers_round_trip():
    gen = torch.Generator().manual_seed(0)
    hw = [(5, 7), (3, 4), (1, 2)]
    maps = [torch.randn(2, 6, h, w, generator=gen) for h, w in hw]
    for t in maps:
        r = R.to_rows(t)
        assert r.shape == (2 * t.shape[2] * t.shape[3], 6)
        assert torch.equal(r[-1], t[1, :, -1, -1]) and torch.equal(r[t.shape[3] - 1], t[0, :, 0, -1])       # row = (n * H + h) * W + w
        assert torch.equal(R.from_rows(r, 2, t.shape[2], t.shape[3]), t)
    rows = R.pyr_to_rows(maps)
    assert rows.shape[0] == sum(2 * h * w for h, w in hw)
    assert torch.equal(rows[2 * 5 * 7 + 3 * 4 + 5], maps[1][1, :, 1, 1])        # level-major, then image, then pixel
    for a, b in zip(R.pyr_from_rows(rows, 2, hw), maps):
        assert torch.equal(a, b)
    assert float((R.h16(torch.tensor([1.0 + 2.0 ** -12])) - 1.0).abs()) == 0.0 and R.h16(torch.zeros(1)).dtype == torch.float64


CASES = R.cases()


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_reference_closed_forms_equal_torch_nn_grad(c):
    g = c.g
    xs, w, scale, shift, ress, gys = R.make_inputs(c)
    assert all(h >= 1 and w_ >= 1 for h, w_ in c.out_levels()), "empty output level"
    for x, res, gy in zip(xs, ress, gys):
        x, gy, wd = x.double(), gy.double(), w.double()
        st, pd, dl = (g.stride, g.stride), (g.pad, g.pad), (g.dil, g.dil)
        gr = R.grads(x, w, gy, g.stride, g.pad, g.dil)
        assert gr.y.shape[2:] == R.out_hw(x.shape[2], x.shape[3], g.kh, g.kw, g.stride, g.pad, g.dil)
        np.testing.assert_allclose(R.dgrad(gy, w, x.shape[2:], g.stride, g.pad, g.dil).numpy(), torch.nn.grad.conv2d_input(x.shape, wd, gy, st, pd, dl).numpy(), atol=1e-12)
        np.testing.assert_allclose(R.wgrad(x, gy, (g.kh, g.kw), g.stride, g.pad, g.dil).numpy(), torch.nn.grad.conv2d_weight(x, w.shape, gy, st, pd, dl).numpy(), atol=1e-11)
        np.testing.assert_allclose(gr.dx.numpy(), R.dgrad(gy, w, x.shape[2:], g.stride, g.pad, g.dil).numpy(), atol=1e-12)
        np.testing.assert_allclose(gr.dw.numpy(), R.wgrad(x, gy, (g.kh, g.kw), g.stride, g.pad, g.dil).numpy(), atol=1e-11)
        # the full layer: the ReLU mask and the folded scale reach every gradient
        full = R.grads(x, w, gy, g.stride, g.pad, g.dil, scale, shift, res, "relu")
        gm = gy * (full.y > 0)
        np.testing.assert_allclose(full.dres.numpy(), gm.numpy(), atol=0)
        np.testing.assert_allclose(full.dshift.numpy(), gm.sum((0, 2, 3)).numpy(), atol=1e-11)
        np.testing.assert_allclose(full.dx.numpy(), R.dgrad(gm, wd * scale.double().view(-1, 1, 1, 1), x.shape[2:], g.stride, g.pad, g.dil).numpy(), atol=1e-11)
        np.testing.assert_allclose(full.dw.numpy(), (R.wgrad(x, gm, (g.kh, g.kw), g.stride, g.pad, g.dil) * scale.double().view(-1, 1, 1, 1)).numpy(), atol=1e-11)
    if g.gid == "7":     # input row 11 is read by no window
        assert float(gr.dx[:, :, 11].abs().max()) == 0.0
    if g.gid == "12":    # windows entirely inside the padding: the output there is the shift
        y = R.forward(xs[0], w, g.stride, g.pad, g.dil, None, shift)
        assert torch.equal(y[:, :, 0, 0], shift.double().expand(R.BATCH, -1))
