"""The loss and target kernels of csrc/fd_loss.hip at their decision boundaries: the designed inputs of
tests/loss_edge_cases.py (test_loss_edges_cpu.py proves which edges they hit) against oracle/torch_ref.py and
F.binary_cross_entropy_with_logits evaluated in float64 with autograd on the same fp32 values.  Every reference value is
asserted finite before it is compared."""
import numpy as np
import pytest
import torch

import loss_edge_cases as E
from oracle import torch_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd.model.loss import compute_cls_loss, compute_cnt_loss, ltrb_reg_loss
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _ref(key, fn, *args):
    """One float64 reference per case, shared by the tests that need it, asserted finite once."""
    if key not in _REF:
        out = fn(*args)
        for a in out:
            assert np.isfinite(a).all(), key
        _REF[key] = out
    return _REF[key]


def _w(dtype=torch.float32):
    return torch.tensor(E.IMG_W, dtype=dtype, device=DEV)


def _cmp(got, ref, what, **tol):
    got = got.detach().cpu().numpy()
    print(what, "max |err|", float(np.abs(got - ref).max()), "max |ref|", float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, err_msg=what, **tol)


# ---------------------------------------------------------------------------------------------------- LTRB IoU / GIoU
@pytest.mark.parametrize("mode", ["iou", "giou"])
@pytest.mark.parametrize("L", E.LS)
def test_ltrb_edges_vs_float64(L, mode):
    pred, tgt, mask = E.ltrb_case(L)
    loss, grad = _ref(("ltrb", L, mode), E.ltrb_ref, pred, tgt, mask, mode)
    p = pred.to(DEV).requires_grad_(True)
    out = ltrb_reg_loss(p, tgt.to(DEV), mask.to(DEV), mode)
    (out * _w()).sum().backward()
    _cmp(out, loss, f"ltrb {mode} L={L} loss", rtol=E.LOSS_RTOL)
    _cmp(p.grad, grad, f"ltrb {mode} L={L} grad", **E.GRAD_TOL)
    g = p.grad.cpu()
    assert float(out[0].detach()) == 0 and (g[0] == 0).all()                    # no positive: num_pos clamps to 1, loss 0, gradient exactly 0
    assert (g[~mask] == 0).all()                                         # all-zero boxes behind the mask never reach the arithmetic
    perfect = (pred == tgt).all(-1) & mask
    assert (g[perfect] == 0).all()                                       # pred == target: every term of the closed form cancels exactly


@pytest.mark.parametrize("mode", ["iou", "giou"])
def test_ltrb_raw_kernels_num_pos_and_gscale(mode):
    """ops.ltrb_loss_fwd / _bwd without the autograd node: un-normalised sums, exact num_pos, gscale[b] per image."""
    L = 513
    pred, tgt, mask = E.ltrb_case(L)
    loss, grad = _ref(("ltrb", L, mode), E.ltrb_ref, pred, tgt, mask, mode)
    npos = mask.sum(1)
    m = {"iou": 0, "giou": 1}[mode]
    s, n = ops.ltrb_loss_fwd(pred.to(DEV), tgt.to(DEV), mask.to(torch.uint8).to(DEV), m)
    assert n.cpu().tolist() == npos.tolist() == [0, L, 1]
    _cmp(s, loss * npos.clamp(min=1).numpy(), f"ltrb {mode} raw sums", rtol=E.LOSS_RTOL)
    gs = torch.tensor([7.0, 0.002, 1.5])                                 # at most the scale the CPU tolerance check ran at
    got = ops.ltrb_loss_bwd(pred.to(DEV), tgt.to(DEV), mask.to(torch.uint8).to(DEV), gs.to(DEV), m)
    scale = (gs.double() / (torch.tensor(E.IMG_W).double() / npos.clamp(min=1))).numpy()
    _cmp(got, grad * scale[:, None, None], f"ltrb {mode} raw grad", **E.GRAD_TOL)


@pytest.mark.parametrize("mode", ["iou", "giou"])
def test_ltrb_wrapper_strided_and_fp16_pred(mode):
    L = 257
    pred, tgt, mask = E.ltrb_case(L, E.LTRB_ROWS_MODERATE)
    pred = pred.half().float()                                           # fp16-exact values, so all three calls see the same numbers
    loss, grad = _ref(("ltrb16", mode), E.ltrb_ref, pred, tgt, mask, mode)
    td, md = tgt.to(DEV), mask.to(DEV)
    base = pred.to(DEV).requires_grad_(True)
    out0 = ltrb_reg_loss(base, td, md, mode)
    (out0 * _w()).sum().backward()
    _cmp(out0, loss, f"ltrb {mode} fp16-exact loss", rtol=E.LOSS_RTOL)
    _cmp(base.grad, grad, f"ltrb {mode} fp16-exact grad", **E.GRAD_TOL)

    buf = torch.zeros(E.B, 4, L + 3, device=DEV)                         # [B, L, 4] as a transposed window of a larger buffer
    buf[:, :, 2:L + 2] = pred.to(DEV).transpose(1, 2)
    buf.requires_grad_(True)
    view = buf[:, :, 2:L + 2].transpose(1, 2)
    assert not view.is_contiguous()
    out1 = ltrb_reg_loss(view, td, md, mode)
    (out1 * _w()).sum().backward()
    assert torch.equal(out1.detach(), out0.detach())
    assert buf.grad.shape == buf.shape and torch.equal(buf.grad[:, :, 2:L + 2].transpose(1, 2), base.grad)
    assert (buf.grad[:, :, :2] == 0).all() and (buf.grad[:, :, L + 2:] == 0).all()

    half = pred.half().to(DEV).requires_grad_(True)
    out2 = ltrb_reg_loss(half, td, md, mode)
    (out2 * _w()).sum().backward()
    assert out2.dtype == torch.float32 and torch.equal(out2.detach(), out0.detach())
    assert half.grad.dtype == torch.float16 and half.grad.shape == half.shape
    assert torch.isfinite(half.grad).all() and torch.equal(half.grad, base.grad.half())


# ---------------------------------------------------------------------------------------------------- centerness BCE
def _cnt_preds(x):
    """[B, L] logits -> the list of [B, 1, h, w] maps compute_cnt_loss flattens back to [B, L, 1]."""
    return [x.reshape(x.shape[0], 1, 1, x.shape[1])]


@pytest.mark.parametrize("L", E.LS)
def test_bce_edges_vs_float64(L):
    x, t, mask = E.bce_case(L)
    loss, grad = _ref(("bce", L), E.bce_ref, x, t, mask)
    npos = mask.sum(1)
    xd, td, md = x.to(DEV), t.to(DEV), mask.to(DEV)
    # the kernels themselves
    s, n = ops.bce_loss_fwd(xd, td, md.to(torch.uint8))
    assert n.cpu().tolist() == npos.tolist()
    _cmp(s, loss * npos.clamp(min=1).numpy(), f"bce L={L} raw sums", rtol=E.LOSS_RTOL)
    gs = (_w() / npos.clamp(min=1).to(DEV)).contiguous()
    _cmp(ops.bce_loss_bwd(xd, td, md.to(torch.uint8), gs), grad, f"bce L={L} raw grad", **E.GRAD_TOL)
    # through the autograd node
    leaf = xd.clone().requires_grad_(True)
    out = compute_cnt_loss(_cnt_preds(leaf), td[..., None], md)
    (out * _w()).sum().backward()
    _cmp(out, loss, f"bce L={L} loss", rtol=E.LOSS_RTOL)
    _cmp(leaf.grad, grad, f"bce L={L} grad", **E.GRAD_TOL)
    assert float(out[0].detach()) == 0 and (leaf.grad[0] == 0).all() and (leaf.grad.cpu()[~mask] == 0).all()


def test_bce_grid_per_target_rows():
    """Every (logit, target) pair with a gscale of its own per target value; mask all on."""
    x, t, gs = E.bce_grid()
    loss, grad = _ref("bce_grid", E.bce_grid_ref)
    mask = torch.ones_like(x, dtype=torch.uint8).to(DEV)
    s, n = ops.bce_loss_fwd(x.to(DEV), t.to(DEV), mask)
    assert n.cpu().tolist() == [10] * 4
    _cmp(s, loss, "bce grid sums", rtol=E.LOSS_RTOL)
    _cmp(ops.bce_loss_bwd(x.to(DEV), t.to(DEV), mask, gs.to(DEV)), grad, "bce grid grad", **E.GRAD_TOL)


def test_bce_wrapper_strided_and_fp16_pred():
    L = 257
    x, t, mask = E.bce_case(L)
    x = x.half().float()
    loss, grad = _ref("bce16", E.bce_ref, x, t, mask)
    td, md = t.to(DEV)[..., None], mask.to(DEV)
    base = x.to(DEV).requires_grad_(True)
    out0 = compute_cnt_loss(_cnt_preds(base), td, md)
    (out0 * _w()).sum().backward()
    _cmp(out0, loss, "bce fp16-exact loss", rtol=E.LOSS_RTOL)
    _cmp(base.grad, grad, "bce fp16-exact grad", **E.GRAD_TOL)

    buf = torch.zeros(E.B, 3, 1, L, device=DEV)                          # the centerness map as channel 1 of a 3-channel buffer
    buf[:, 1, 0] = x.to(DEV)
    buf.requires_grad_(True)
    view = buf[:, 1:2]
    assert not view.is_contiguous()
    out1 = compute_cnt_loss([view], td, md)
    (out1 * _w()).sum().backward()
    assert torch.equal(out1.detach(), out0.detach())
    assert buf.grad.shape == buf.shape and torch.equal(buf.grad[:, 1, 0], base.grad)
    assert (buf.grad[:, 0] == 0).all() and (buf.grad[:, 2] == 0).all()

    half = x.half().to(DEV).requires_grad_(True)
    out2 = compute_cnt_loss(_cnt_preds(half), td, md)
    (out2 * _w()).sum().backward()
    assert out2.dtype == torch.float32 and torch.equal(out2.detach(), out0.detach())
    assert half.grad.dtype == torch.float16 and half.grad.shape == half.shape and torch.equal(half.grad, base.grad.half())


# ---------------------------------------------------------------------------------------------------- focal
@pytest.mark.parametrize("alpha", [0.25, 0.5])
@pytest.mark.parametrize("L,C", E.FOCAL_SHAPES)
def test_focal_edges_vs_float64(L, C, alpha):
    logits, labels = E.focal_case(L, C)
    loss, grad = _ref(("focal", L, C, alpha), E.focal_ref, logits, labels, alpha)
    xd, ld = logits.to(DEV), labels.to(DEV)
    _cmp(ops.focal_loss_fwd(xd, ld, alpha), loss, f"focal ({L},{C}) a={alpha} loss", rtol=E.FOCAL_LOSS_RTOL)
    got = ops.focal_loss_bwd(xd, ld, torch.tensor(E.FOCAL_GSCALE, device=DEV), alpha)
    _cmp(got, grad, f"focal ({L},{C}) a={alpha} grad", **E.FOCAL_GRAD_TOL)
    clipped = E.focal_onehot(labels, C).bool() & (logits < E.FOCAL_CLIP_LOGIT)
    assert clipped.any() and (grad[clipped.numpy()] == 0).all() and (got.cpu()[clipped] == 0).all()


def test_focal_through_compute_cls_loss():
    """(341, 81) as four levels through flatten_levels and the autograd node: loss / num_pos, gradient scaled per image."""
    L, C = 341, 81
    hw = [(16, 16), (8, 8), (4, 4), (1, 5)]
    logits, labels = E.focal_case(L, C)
    loss, grad = _ref(("focal", L, C, 0.25), E.focal_ref, logits, labels, 0.25)
    mask = (labels >= 1) & (labels <= C)
    mask[0] = False                                                      # num_pos clamps to 1 here
    npos = mask.sum(1).clamp(min=1)
    maps, start = [], 0
    for h, w in hw:
        maps.append(logits[:, start:start + h * w].reshape(E.B, h, w, C).permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True))
        start += h * w
    out = compute_cls_loss(maps, labels[..., None].to(DEV), mask.to(DEV))
    (out * torch.tensor(E.FOCAL_GSCALE, device=DEV) * npos.to(DEV)).sum().backward()
    _cmp(out, loss / npos.numpy(), "compute_cls_loss", rtol=E.FOCAL_LOSS_RTOL)
    got = torch.cat([m.grad.permute(0, 2, 3, 1).reshape(E.B, -1, C) for m in maps], 1)
    _cmp(got, grad, "compute_cls_loss grad", **E.FOCAL_GRAD_TOL)


# ---------------------------------------------------------------------------------------------------- target assignment
def _targets_vs_oracle(gt, labels, hw, strides, ranges, key, module=False):
    exp = _ref(key, lambda: tuple(t.numpy() for t in R.gen_targets(hw, strides, ranges, gt.double(), labels)))
    if module:
        outs = [[torch.zeros(gt.shape[0], 1, h, w, device=DEV) for h, w in hw]]
        got = FCOSGenTargets(list(strides), [list(r) for r in ranges])([outs, gt.to(DEV), labels.to(DEV)])
    else:
        got = ops.fcos_gen_targets(gt.to(DEV), labels.to(DEV), list(hw), list(strides), [list(r) for r in ranges])
    np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0])
    np.testing.assert_array_equal(got[2].cpu().numpy(), exp[2])
    np.testing.assert_allclose(got[1].cpu().numpy(), exp[1], rtol=1e-6)
    return exp


@pytest.mark.parametrize("module", [False, True])
def test_gen_targets_boundaries(module):
    gt, labels = E.targets_case()
    cls = _targets_vs_oracle(gt, labels, E.TGT_HW, E.TGT_STRIDES, E.TGT_RANGES, "targets", module)[0][..., 0]
    assert cls.shape == (3, 336)
    assert cls[0, 4 * 16 + 4] == 1 and cls[0, 256 + 4 * 8 + 2] == 0       # omax == hi is positive, omax == lo is not
    assert cls[1, 256 + 64 + 1 * 4 + 1] == 8 and cls[1, 6 * 16 + 6] == 11 and cls[1, 256 + 1 * 8 + 5] == 14


def test_gen_targets_image_without_gt():
    gt, labels = E.targets_case_empty()
    cls, cnt, reg = _targets_vs_oracle(gt, labels, E.TGT_HW, E.TGT_STRIDES, E.TGT_RANGES, "targets_empty")
    assert (cls[1] == 0).all() and (cnt[1] == -1).all() and (reg[1] == -1).all() and (cls[0] > 0).any() and (cls[2] > 0).any()


def test_gen_targets_single_box():
    gt, labels = E.targets_case_m1()
    assert gt.shape == (3, 1, 4)
    cls = _targets_vs_oracle(gt, labels, E.TGT_HW, E.TGT_STRIDES, E.TGT_RANGES, "targets_m1")[0]
    assert (cls[0] == 1).any() and (cls[1] == 0).all() and (cls[2] == 16).any()


def test_gen_targets_odd_stride():
    gt, labels = E.targets_case_odd_stride()
    cls = _targets_vs_oracle(gt, labels, E.ODD_HW, E.ODD_STRIDE, E.ODD_RANGE, "targets_odd")[0][..., 0]
    assert cls[0, 3 * 9 + 3] == 0 and cls[1, 3 * 9 + 3] == 0 and cls[0, 3 * 9 + 4] == 1 and cls[2, 2 * 9 + 2] == 3
