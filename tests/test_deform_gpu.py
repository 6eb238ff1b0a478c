"""Modulated deformable convolution on the GPU against the float64 reference of tests/deform_ref.py: the two kernels (fd_deform_im2col_nhwc,
fd_deform_bwd_nhwc) on contiguous maps and channel views, the functional deform_conv2d with all five gradients, the DeformableConv2d module, autocast,
graph capture and the rejections.  Inputs are the seeded ones of deform_ref.make_inputs: coordinates exact in fp32 (test_deform_cpu.py), so floor()
cannot differ between the device and the reference.  Bars: the project's (tests/test_layer_views_gpu.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import deform_ref as D
import layer_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.modules.modules import DeformableConv2d, deform_conv2d

pytestmark = pytest.mark.gpu
DEV = R.DEV
ATOL, RTOL = 1e-4, 1e-5                 # outputs
GRAD, PGRAD = 2e-5, 5e-5                # gradients / parameter gradients relative to the largest reference magnitude
NAN = float("nan")
MODES = ["none", "mask", "logits"]      # mask=None / an activated mask (mask_act 0) / modulator logits (mask_act 1)
CASES = [(g, False) for g in D.GEOMS] + [(D.INTEGER_GEOM, True)]
CASE_IDS = ["x".join(map(str, g)) + ("-int" if i else "") for g, i in CASES]


def close(a, b, tol, what=""):
    s = float(b.abs().max()) + 1e-12
    print(f"{what}: max |err| / max |ref| = {float((a.double().cpu() - b).abs().max()) / s:.3e} (bar {tol:.0e})")
    np.testing.assert_allclose(a.double().cpu().numpy() / s, b.numpy() / s, atol=tol, err_msg=what)


def out_close(a, b, what=""):
    print(f"{what}: max |err| = {float((a.double().cpu() - b).abs().max()):.3e}, max |ref| = {float(b.abs().max()):.3e}")
    np.testing.assert_allclose(a.double().cpu().numpy(), b.numpy(), atol=ATOL, rtol=RTOL, err_msg=what)


@functools.lru_cache(maxsize=None)
def kernel_ref(geom, C, integer, mode):
    """Inputs as rows, the reference columns, a random dcols and the reference's autograd gradients of sum(cols * dcols).  Computed once, never modified."""
    H, W, K, stride, pad = geom
    x, off, logits = D.make_inputs(geom, C, integer=integer)
    m_in = None if mode == "none" else (logits if mode == "logits" else 2 * torch.sigmoid(logits))      # what the kernel is handed
    xd, od = x.double().requires_grad_(), off.double().requires_grad_()
    md = m_in.double().requires_grad_() if m_in is not None else None
    act = None if md is None else (2 * torch.sigmoid(md) if mode == "logits" else md)
    cols = D.deform_cols(xd, od, act, K, stride, pad)
    dcols = torch.randn(cols.shape, generator=torch.Generator().manual_seed(7 + C + K))
    grads = torch.autograd.grad(cols, [xd, od] + ([md] if md is not None else []), dcols.double())
    return dict(x=D.rows(x), off=D.rows(off), mask=D.rows(m_in) if m_in is not None else None, cols=cols.detach(), dcols=dcols,
                d_x=D.rows(grads[0]), d_off=D.rows(grads[1]), d_mask=D.rows(grads[2]) if md is not None else None)


def _views(ts, geoms):
    """name -> (Rows, buffer) with every tensor on its own channel view (NaN in the neighbour channels); None stays None."""
    out = {}
    for (n, t), (co, tail) in zip(ts.items(), geoms):
        out[n] = R.make_view(t, co, tail) if t is not None else (None, None)
    return out


# ------------------------------------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("geom", D.GEOMS, ids=CASE_IDS[:len(D.GEOMS)])
def test_im2col_against_reference_and_on_views(geom, C, mode):
    H, W, K, stride, pad = geom
    r = kernel_ref(geom, C, False, mode)
    B, M, act = D.BATCH, r["cols"].shape[0], mode == "logits"
    x, off = ops.Rows(r["x"].to(DEV)), ops.Rows(r["off"].to(DEV))
    mask = ops.Rows(r["mask"].to(DEV)) if r["mask"] is not None else None
    cols = ops.Rows(torch.full((M, K * K * C), NAN, device=DEV))
    ops.deform_im2col(x, off, mask, cols, B, H, W, K, stride, pad, 1, act)
    out_close(cols.buf, r["cols"], "cols")
    # every operand on a channel view: x and cols 4-aligned, offset / mask on odd channel offsets (they are read one float at a time)
    v = _views(dict(x=r["x"], off=r["off"], mask=r["mask"], cols=torch.full((M, K * K * C), NAN)), [(8, 4), (5, 3), (2, 1), (4, 8)])
    before = {n: b.clone() for n, (_, b) in v.items() if b is not None}
    ops.deform_im2col(v["x"][0], v["off"][0], v["mask"][0], v["cols"][0], B, H, W, K, stride, pad, 1, act)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(v["cols"][0].tensor()), R.bits(cols.buf)), "the view result differs from the contiguous one"
    assert R.outside_untouched(v["cols"][1], 4, K * K * C, before["cols"]), "write outside the cols view"
    for n in ("x", "off", "mask"):
        if n in before:
            assert R.unchanged(v[n][1], before[n]), f"input {n} changed"
    assert torch.equal(x.buf.cpu(), r["x"]) and torch.equal(off.buf.cpu(), r["off"])


# ------------------------------------------------------------------------------------------------ 2. the backward kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("geom,integer", CASES, ids=CASE_IDS)
def test_bwd_against_reference_autograd(geom, integer, C, mode):
    H, W, K, stride, pad = geom
    r = kernel_ref(geom, C, integer, mode)
    B, M, act, KK = D.BATCH, r["cols"].shape[0], mode == "logits", K * K
    has_mask = r["mask"] is not None

    def run(views, with_dx=True):
        ins = dict(dcols=r["dcols"], x=r["x"], off=r["off"], mask=r["mask"])
        outs = dict(d_off=torch.full((M, 2 * KK), NAN), d_mask=torch.full((M, KK), NAN) if has_mask else None, d_x=torch.zeros(B * H * W, C))
        geoms = [(4, 8), (8, 4), (5, 3), (2, 1), (3, 2), (1, 6), (12, 4)] if views else [(0, 0)] * 7
        v = _views({**ins, **outs}, geoms)
        before = {n: b.clone() for n, (_, b) in v.items() if b is not None}
        ops.deform_bwd(v["dcols"][0], v["x"][0], v["off"][0], v["mask"][0], v["d_off"][0], v["d_mask"][0], v["d_x"][0] if with_dx else None,
                       B, H, W, K, stride, pad, 1, act)
        torch.cuda.synchronize()
        for n in ins:
            if n in before:
                assert R.unchanged(v[n][1], before[n]), f"input {n} changed"
        for n, width in (("d_off", 2 * KK), ("d_mask", KK), ("d_x", C)):
            if n in before:
                assert R.outside_untouched(v[n][1], v[n][0].co, width, before[n]), f"write outside the view of {n}"
        if not with_dx:
            assert R.unchanged(v["d_x"][1], before["d_x"]), "d_x written although no pointer was given"
        return {n: v[n][0].tensor().clone() for n in outs if v[n][0] is not None}

    first, second, no_dx = run(False), run(True), run(False, with_dx=False)
    for got in (first, second):
        close(got["d_off"], r["d_off"], GRAD, "d_offset")
        if has_mask:
            close(got["d_mask"], r["d_mask"], GRAD, "d_mask")
        close(got["d_x"], r["d_x"], GRAD, "d_x")
    for n in ("d_off", "d_mask"):
        if n in first:
            assert torch.equal(R.bits(first[n]), R.bits(second[n])), f"{n} differs between two runs (contiguous / views)"
            assert torch.equal(R.bits(first[n]), R.bits(no_dx[n])), f"{n} changes when d_x is skipped"


# ------------------------------------------------------------------------------------------------ 3. the functional
@functools.lru_cache(maxsize=None)
def conv_ref(geom, C, Cout, full, integer=False):
    """The float64 reference of deform_conv2d and its five gradients for a random output gradient (full: with mask and bias)."""
    H, W, K, stride, pad = geom
    x, off, logits = D.make_inputs(geom, C, seed=1, integer=integer)
    g = torch.Generator().manual_seed(11 + Cout + K)
    w = torch.randn(Cout, C, K, K, generator=g) / (K * K * C) ** 0.5
    b = torch.randn(Cout, generator=g) if full else None
    mask = 2 * torch.sigmoid(logits) if full else None
    leaves = [t.double().requires_grad_() if t is not None else None for t in (x, off, mask, w, b)]
    y, _ = D.deform_conv2d(leaves[0], leaves[1], leaves[3], leaves[4], stride, pad, 1, leaves[2])
    gy = torch.randn(y.shape, generator=g)
    grads = iter(torch.autograd.grad(y, [t for t in leaves if t is not None], gy.double()))
    return dict(ins=(x, off, mask, w, b), y=y.detach(), gy=gy, grads=[next(grads) if t is not None else None for t in leaves])


def _check_functional(r, geom):
    H, W, K, stride, pad = geom
    leaves = [t.to(DEV).requires_grad_() if t is not None else None for t in r["ins"]]
    y = deform_conv2d(leaves[0], leaves[1], leaves[3], leaves[4], stride, pad, 1, leaves[2])
    assert y.shape == r["y"].shape and y.dtype == torch.float32
    out_close(y.detach(), r["y"], "output")
    grads = iter(torch.autograd.grad(y, [t for t in leaves if t is not None], r["gy"].to(DEV)))
    for name, leaf, ref, tol in zip(("input", "offset", "mask", "weight", "bias"), leaves, r["grads"], (GRAD, GRAD, GRAD, PGRAD, PGRAD)):
        if leaf is not None:
            got = next(grads)
            assert got.shape == ref.shape
            close(got, ref, tol, f"d_{name}")


@pytest.mark.parametrize("full", [True, False], ids=["mask+bias", "plain"])
@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("geom", D.GEOMS, ids=CASE_IDS[:len(D.GEOMS)])
def test_deform_conv2d_forward_and_five_gradients(geom, Cout, full):
    _check_functional(conv_ref(geom, 32, Cout, full), geom)


@pytest.mark.parametrize("integer", [False, True], ids=["eighths", "integer"])
def test_deform_conv2d_wide_input_and_integer_offsets(integer):
    _check_functional(conv_ref(D.INTEGER_GEOM, 256, 64, True, integer), D.INTEGER_GEOM)


@pytest.mark.parametrize("geom", D.GEOMS, ids=CASE_IDS[:len(D.GEOMS)])
def test_deform_conv2d_zero_offsets_is_conv2d(geom):
    H, W, K, stride, pad = geom
    x, _, _ = D.make_inputs(geom, 32, seed=2)
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(8, 32, K, K, generator=g) / (K * K * 32) ** 0.5, torch.randn(8, generator=g)
    Ho, Wo = D.out_hw(H, W, K, stride, pad)
    y = deform_conv2d(x.to(DEV), torch.zeros(D.BATCH, 2 * K * K, Ho, Wo, device=DEV), w.to(DEV), b.to(DEV), stride, pad)
    out_close(y, F.conv2d(x.double(), w.double(), b.double(), stride, pad), "zero offsets")


# ------------------------------------------------------------------------------------------------ 4. the module
def _module_ref(m, x):
    """The module's definition in float64 on the CPU: offsets and modulator from the side convs, then the reference."""
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    s, p = m.stride[0], m.padding
    xd = x.double().cpu()
    off = F.conv2d(xd, sd["offset_conv.weight"], sd["offset_conv.bias"], s, p)
    mask = 2 * torch.sigmoid(F.conv2d(xd, sd["modulator_conv.weight"], sd["modulator_conv.bias"], s, p))
    return D.deform_conv2d(xd, off, sd["regular_conv.weight"], sd.get("regular_conv.bias"), s, p, 1, mask)


@pytest.mark.parametrize("stride,bias", [(1, True), (2, False)])
def test_module_fresh_is_plain_conv_and_follows_reference_once_offsets_are_learned(stride, bias):
    torch.manual_seed(5)
    m = DeformableConv2d(32, 64, 3, stride=stride, padding=1, bias=bias).to(DEV)
    x = torch.randn(2, 32, 7, 10)
    y = m(x.to(DEV))
    rc = m.regular_conv
    ref = F.conv2d(x.double(), rc.weight.detach().double().cpu(), rc.bias.detach().double().cpu() if bias else None, stride, 1)
    assert y.shape == ref.shape
    out_close(y.detach(), ref, "fresh module")
    with torch.no_grad():
        for side in (m.offset_conv, m.modulator_conv):
            side.weight.normal_(std=0.05)
            side.bias.normal_(std=0.05)
    y = m(x.to(DEV))
    ref, _ = _module_ref(m, x)
    out_close(y.detach(), ref, "module with random side convs")
    assert float((ref - F.conv2d(x.double(), rc.weight.detach().double().cpu(), rc.bias.detach().double().cpu() if bias else None, stride, 1)).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------ 5. autocast
def test_module_under_autocast():
    """Under torch.autocast(float16) the sampler stays fp32 and the GEMM takes f16 operands with fp32 accumulation: the output is the reference with the
    columns and regular_conv.weight rounded to f16.  The side convs have zero weights and dyadic / random biases, so that offsets (odd eighths) and
    modulator logits are the same numbers in f16-operand arithmetic as in the reference."""
    torch.manual_seed(6)
    m = DeformableConv2d(32, 64, 3, padding=1, bias=True).to(DEV)
    with torch.no_grad():
        m.offset_conv.bias.copy_((2 * torch.randint(-12, 12, (18,)) + 1).float() / 8)
        m.modulator_conv.bias.normal_()
    x = torch.randn(2, 32, 7, 10)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(x.to(DEV))
    assert y.dtype == torch.float32
    _, cols = _module_ref(m, x)
    w16 = m.regular_conv.weight.detach().cpu().half().double().permute(0, 2, 3, 1).reshape(64, -1)
    ref = cols.float().half().double() @ w16.t() + m.regular_conv.bias.detach().double().cpu()
    got = y.detach().permute(0, 2, 3, 1).reshape(-1, 64)
    print(f"autocast: max |err| = {float((got.double().cpu() - ref).abs().max()):.3e}")
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.numpy(), atol=2e-3, rtol=2e-3)
    y.sum().backward()                          # the backward runs under autocast's arithmetic too and does not raise
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------------------ 6. graph capture
def test_forward_backward_captured_in_one_graph():
    """Forward + backward of deform_conv2d on static tensors in one torch.cuda.graph, replayed twice: no host synchronisation, no stream switch."""
    from pytorch_object_detection_amd.train_graph import GraphedStep
    geom = D.GEOMS[0]
    H, W, K, stride, pad = geom
    r = conv_ref(geom, 32, 64, True)
    names = ("input", "offset", "mask", "weight", "bias")
    gy = r["gy"].to(DEV)
    got = [torch.zeros_like(t, device=DEV) for t in r["ins"]]

    def step(*ins):
        leaves = [t.detach().requires_grad_() for t in ins]
        y = deform_conv2d(leaves[0], leaves[1], leaves[3], leaves[4], stride, pad, 1, leaves[2])
        for dst, g in zip(got, torch.autograd.grad(y, leaves, gy)):
            dst.copy_(g)
        return y.detach()

    graphed = GraphedStep(step, [t.to(DEV) for t in r["ins"]])
    for replay in range(2):
        for t in got:
            t.zero_()
        y = graphed(*[t.to(DEV) for t in r["ins"]])
        torch.cuda.synchronize()
        out_close(y, r["y"], f"replay {replay}: output")
        for name, g, ref, tol in zip(names, got, r["grads"], (GRAD, GRAD, GRAD, PGRAD, PGRAD)):
            close(g, ref, tol, f"replay {replay}: d_{name}")


# ------------------------------------------------------------------------------------------------ 7. rejections
class BadRows:
    """An ops.Rows look-alike that may describe an illegal view (ops.Rows itself refuses to)."""

    def __init__(self, buf, co, cs, C):
        self.buf, self.co, self.cs, self.C, self.rows, self.ptr, self.f16 = buf, co, cs, C, buf.shape[0], buf.data_ptr(), False


def test_rejections_raise_before_any_launch():
    geom = D.GEOMS[0]
    H, W, K, stride, pad = geom
    B, Ho, Wo = D.BATCH, *D.out_hw(H, W, K, stride, pad)
    M = B * Ho * Wo

    def bufs(C):
        return (torch.zeros(B * H * W, C, device=DEV), torch.zeros(M, 18, device=DEV), torch.zeros(M, 9, device=DEV), torch.full((M, 9 * C), NAN, device=DEV))

    def untouched(t):
        torch.cuda.synchronize()
        return bool(torch.isnan(t).all())

    # the kernel: C % 4, a wrong offset / mask width, illegal views
    x, off, mask, cols = bufs(30)
    with pytest.raises(FdError):
        ops.deform_im2col(ops.Rows(x), ops.Rows(off), ops.Rows(mask), ops.Rows(cols), B, H, W, K, stride, pad)
    assert untouched(cols)
    x, off, mask, cols = bufs(32)
    for bad in (dict(off=ops.Rows(torch.zeros(M, 16, device=DEV))), dict(mask=ops.Rows(torch.zeros(M, 8, device=DEV))),
                dict(x=BadRows(torch.zeros(B * H * W, 40, device=DEV), 2, 40, 32)), dict(x=BadRows(torch.zeros(B * H * W, 38, device=DEV), 4, 38, 32)),
                dict(x=BadRows(x, 4, 32, 32)), dict(cols=BadRows(cols, 2, 288, 288)), dict(off=BadRows(off, 1, 18, 18)),
                dict(mask=BadRows(mask, 0, 8, 9)), dict(K=8), dict(stride=0), dict(pad=8)):
        a = dict(x=ops.Rows(x), off=ops.Rows(off), mask=ops.Rows(mask), cols=ops.Rows(cols), K=K, stride=stride, pad=pad)
        a.update(bad)
        with pytest.raises(FdError):
            ops.deform_im2col(a["x"], a["off"], a["mask"], a["cols"], B, H, W, a["K"], a["stride"], a["pad"])
        assert untouched(cols), bad
        d_off, d_mask, d_x = torch.full((M, 18), NAN, device=DEV), torch.full((M, 9), NAN, device=DEV), torch.full((B * H * W, 32), NAN, device=DEV)
        with pytest.raises(FdError):
            ops.deform_bwd(a["cols"], a["x"], a["off"], a["mask"], ops.Rows(d_off), ops.Rows(d_mask), ops.Rows(d_x), B, H, W, a["K"], a["stride"], a["pad"])
        assert untouched(d_off) and untouched(d_mask) and untouched(d_x), bad
    with pytest.raises(FdError):        # d_mask without mask
        ops.deform_bwd(ops.Rows(cols), ops.Rows(x), ops.Rows(off), None, ops.Rows(d_off), ops.Rows(d_mask), None, B, H, W, K, stride, pad)
    assert untouched(d_off) and untouched(d_mask)

    # the functional: wrong offset / mask channel counts, a CPU tensor
    xi, w = torch.zeros(B, 32, H, W, device=DEV), torch.zeros(8, 32, 3, 3, device=DEV)
    with pytest.raises(FdError):
        deform_conv2d(xi, torch.zeros(B, 16, Ho, Wo, device=DEV), w, None, stride, pad)
    with pytest.raises(FdError):
        deform_conv2d(xi, torch.zeros(B, 18, Ho, Wo, device=DEV), w, None, stride, pad, 1, torch.zeros(B, 8, Ho, Wo, device=DEV))
    with pytest.raises(FdError):
        deform_conv2d(xi, torch.zeros(B, 18, Ho, Wo), w, None, stride, pad)
    with pytest.raises(FdError):
        deform_conv2d(torch.zeros(B, 48, H, W, device=DEV), torch.zeros(B, 18, Ho, Wo, device=DEV), torch.zeros(8, 48, 3, 3, device=DEV), None, stride, pad)

    # the module: in_channels % 32, a non-square kernel, groups != 1
    with pytest.raises(FdError, match="in_channels % 32"):
        DeformableConv2d(48, 8, 3).to(DEV)(torch.zeros(1, 48, 4, 4, device=DEV))
    with pytest.raises(FdError, match="square"):
        DeformableConv2d(32, 8, (3, 5), padding=1).to(DEV)(torch.zeros(1, 32, 6, 6, device=DEV))
    m = DeformableConv2d(32, 8, 3).to(DEV)
    m.regular_conv = nn.Conv2d(32, 8, 3, padding=1, groups=2).to(DEV)
    with pytest.raises(FdError, match="groups"):
        m(torch.zeros(1, 32, 4, 4, device=DEV))
