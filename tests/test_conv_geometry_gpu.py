"""The dense conv path over every geometry its entry points admit (tests/conv_ref.py GEOMS), against the float64 reference of the same op:
forward on every precision and tile, weight gradient, data gradient (stride 1 and the strided parity classes), the autograd nodes and the public layers.

Bars (the project's own): fp32 / f16x3 outputs atol 1e-4 + rtol 1e-5; gradients 2e-5 and parameter gradients 5e-5 of the largest reference magnitude;
FD_PREC_F16 against the reference on f16-rounded operands: forward-kernel outputs atol = rtol = 2e-5 (test_amp_gpu.test_conv_f16_on_k_tiles_of_64_channels),
weight gradient 2e-5 * max|ref| + 1e-5.  Every comparison prints `[geom] <kernel family> ... rel <max|err| / max|ref|>`."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_ref as R
from pytorch_object_detection_amd import _lib, ops, train_ops as T
from pytorch_object_detection_amd._lib import ACT_NONE, ACT_RELU, FdError, Segs
from pytorch_object_detection_amd.model.modules.modules import DepthWiseConv2d, PointWiseConv, _layer_conv
from pytorch_object_detection_amd.ops import Rows, WFormat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = R.BATCH
ATOL, RTOL = 1e-4, 1e-5
GRAD, PGRAD = 2e-5, 5e-5
F16_TOL = 2e-5
PREC = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3, "f16": _lib.PREC_F16}
ACT = {"none": ACT_NONE, "relu": ACT_RELU}
F16_DIRECT_TILES = _lib.F16_TILES      # the tiles the single-plane f16 instantiation of the direct kernel is built for (kept beside TILES, following fd_conv.hip)
FAMILY = {_lib.PATCH_TILE: "patch", _lib.WAVE_TILE: "wave", _lib.WINO_TILE: "winograd-f2", _lib.WINO4_TILE: "winograd-f4", _lib.NARROW_TILE: "narrow",
          _lib.F16K64_TILE: "f16k64"}


def _report(family: str, what: str, got: torch.Tensor, ref: torch.Tensor) -> float:
    err, s = float((got - ref).abs().max()), float(ref.abs().max()) + 1e-12
    print(f"[geom] {family} {what}: max|err| {err:.3e} rel {err / s:.3e}")
    return err / s


def out_close(got, ref, family, what, atol=ATOL, rtol=RTOL):
    """got (device) against ref (float64, CPU): |got - ref| <= atol + rtol * |ref| elementwise."""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(ref.shape)}"
    assert not torch.isnan(g).any(), f"{what}: NaN left in the output"
    _report(family, what, g, ref)
    np.testing.assert_allclose(g.numpy(), ref.numpy(), atol=atol, rtol=rtol, err_msg=what)


def rel_close(got, ref, tol, family, what, extra=0.0):
    """max |got - ref| <= tol * max |ref| + extra."""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(ref.shape)}"
    assert not torch.isnan(g).any(), f"{what}: NaN left in the result"
    _report(family, what, g, ref)
    s = float(ref.abs().max())
    assert float((g - ref).abs().max()) <= tol * s + extra, f"{what}: max |err| {float((g - ref).abs().max()):.3e} > {tol:.0e} * {s:.3e} + {extra:.0e}"


def _nan(rows, C):
    return torch.full((rows, C), float("nan"), dtype=torch.float32, device=DEV)


def _variant(i: int, Cout: int):
    """(scale?, residual?, act) of the i-th case: scale + shift + residual + ReLU / shift only / scale + shift + ReLU.  Cout <= 8 runs without a residual (the narrow kernel takes none)."""
    v = i % 3
    return v != 1, v == 0 and Cout > 8, ("relu" if v != 1 else "none")


# ======================================================================================== a. forward, kernel level
FWD = R.cases()


@pytest.mark.parametrize("c", FWD, ids=[c.id for c in FWD])
def test_forward_on_every_precision_and_tile(c):
    g, Cin, Cout = c.g, c.Cin, c.Cout
    xs, w, scale, shift, ress, _ = R.make_inputs(c)
    use_scale, use_res, act = _variant(FWD.index(c), Cout)
    segs = Segs.make(B, c.levels)
    rows_out = sum(B * h * w_ for h, w_ in c.out_levels())
    ref = {name: R.pyr_to_rows([R.forward(fx(xl), fx(w), g.stride, g.pad, g.dil, scale if use_scale else None, shift, rl if use_res else None, act)
                                for xl, rl in zip(xs, ress)])
           for name, fx in (("f64", lambda t: t.double()), ("f16", R.h16))}
    x, wd = R.pyr_to_rows(xs).to(DEV), w.to(DEV)
    res = R.pyr_to_rows(ress).to(DEV) if use_res else None
    sc, sh = (scale.to(DEV) if use_scale else None), shift.to(DEV)
    direct = {"f32": ops.pack_conv_weight(wd), "f16x3": ops.pack_conv_weight_f16x3(wd),
              "f16": WFormat.DIRECT_F16.pack(wd) if Cin % 32 == 0 else ops.pack_conv_weight_f16x3(wd)}
    own = {}      # the kernels with a weight format of their own, packed where the packer takes the filter (else the launch must decline before it reads any weight)
    if (g.kh, g.kw) == (3, 3) and Cin % 8 == 0:
        own[_lib.WINO_TILE], own[_lib.WINO4_TILE] = WFormat.WINO.pack(wd), WFormat.WINO4.pack(wd)
    if (g.kh, g.kw) == (3, 3) and Cout <= 8 and Cin % 16 == 0:
        own[_lib.NARROW_TILE] = ops.pack_conv_weight_narrow(wd)
    if Cin % 64 == 0:
        own[_lib.F16K64_TILE] = WFormat.F16K64.pack(wd)
    w_frag = ops.pack_conv_weight_wave(wd) if (g.kh, g.kw) == (1, 1) and Cin % 32 == 0 else None
    k = g.kh if g.square else 0       # (a rectangular filter satisfies none of the square-kernel predicates)

    def runs(prec: str, tile: int) -> bool:
        """The documented predicate of a forced tile."""
        if tile == 0:
            return True               # the direct kernel claims the whole space
        if tile == _lib.PATCH_TILE:
            return prec in ("f32", "f16x3") and k == 3 and g.stride == 1 and g.pad == g.dil
        if tile == _lib.WAVE_TILE:
            return prec == "f32" and ops.wave_ok(Cin, Cout, k, g.stride, g.pad)
        if tile in (_lib.WINO_TILE, _lib.WINO4_TILE):
            return prec == "f32" and (ops.wino_ok if tile == _lib.WINO_TILE else ops.wino4_ok)(Cin, Cout, k, g.stride, g.pad, g.dil)
        if tile == _lib.NARROW_TILE:
            return prec == "f32" and ops.narrow_ok(Cin, Cout, k, g.stride, g.pad, g.dil) and not use_res
        if tile == _lib.F16K64_TILE:
            return prec == "f16" and ops.f16k64_ok(Cin, Cout)
        return prec != "f16" or tile in F16_DIRECT_TILES

    tiles = [0] + sorted(_lib.TILES) + [_lib.WINO_TILE, _lib.WINO4_TILE, _lib.NARROW_TILE, _lib.F16K64_TILE]
    ran = declined = 0
    for prec in ("f32", "f16x3", "f16"):
        for tile in tiles:
            y = _nan(rows_out, Cout)
            call = ops.conv_call(Rows(x), segs, own.get(tile, direct[prec]), Rows(y), Cin=Cin, Cout=Cout, k=g.kh, kw=g.kw, stride=g.stride, pad=g.pad, dil=g.dil,
                                 scale=sc, shift=sh, res=Rows(res) if use_res else None, act=ACT[act], tile=tile, precision=PREC[prec],
                                 w_frag=w_frag if tile == _lib.WAVE_TILE else None)
            if not runs(prec, tile):
                with pytest.raises(FdError):
                    call()
                torch.cuda.synchronize()
                assert bool(torch.isnan(y).all()), f"{prec} tile {tile}: declined, but wrote to the output"
                declined += 1
                continue
            call()                    # (a decline here is an FdError: the predicate says this tile covers the layer)
            fam = FAMILY.get(tile, "direct") + "-" + prec
            if prec == "f16":
                out_close(y, ref["f16"], fam, f"{c.id} tile {tile}", atol=F16_TOL, rtol=F16_TOL)
            else:
                out_close(y, ref["f64"], fam, f"{c.id} tile {tile}")
            ran += 1
    print(f"[geom] {c.id}: {ran} launches compared, {declined} declined by their predicate")
    assert ran >= 3 + 12 + 12 + len(F16_DIRECT_TILES)


# ========================================================================================== b. weight gradient
WG = R.cases(square_only=True)


@pytest.mark.parametrize("c", WG, ids=[c.id for c in WG])
def test_weight_gradient(c):
    g, Cin, Cout = c.g, c.Cin, c.Cout
    xs, _, scale, _, _, gys = R.make_inputs(c)
    segs = Segs.make(B, c.levels)
    x, dy, sc = R.pyr_to_rows(xs).to(DEV), R.pyr_to_rows(gys).to(DEV), scale.to(DEV)
    for prec, fx in (("f32", lambda t: t.double()), ("f16", R.h16)):
        ref = sum(R.wgrad(fx(xl), fx(gl), (g.kh, g.kw), g.stride, g.pad, g.dil) for xl, gl in zip(xs, gys)) * scale.double().view(-1, 1, 1, 1)
        for nsplit in (0, 3):
            kw = dict(Cin=Cin, Cout=Cout, k=g.kh, stride=g.stride, pad=g.pad, dil=g.dil, nsplit=nsplit, scale=sc, oihw=True, precision=PREC[prec])
            dw = ops.conv_wgrad(Rows(x), Rows(dy), segs, **kw)
            again = ops.conv_wgrad(Rows(x), Rows(dy), segs, **kw)
            assert torch.equal(dw, again), f"{prec} nsplit {nsplit}: two runs differ"
            if prec == "f32":
                rel_close(dw, ref, PGRAD, "wgrad-f32", f"{c.id} nsplit {nsplit}")
            else:
                rel_close(dw, ref, 2e-5, "wgrad-f16", f"{c.id} nsplit {nsplit}", extra=1e-5)


# ============================================================================================ c. data gradient
DG1 = [c for c in R.cases(square_only=True) if c.g.stride == 1 and c.Cout % 32 == 0 and c.g.dil * (c.g.kh - 1) - c.g.pad >= 0]


@pytest.mark.parametrize("c", DG1, ids=[c.id for c in DG1])
def test_data_gradient_stride_1(c):
    """The forward kernel on dY with the flipped / transposed / scaled weights and pad' = dil * (k - 1) - pad; under AMP on F16K64 weights where the widths allow."""
    g, Cin, Cout = c.g, c.Cin, c.Cout
    xs, w, scale, _, _, gys = R.make_inputs(c)
    so = Segs.make(B, c.out_levels())
    rows_in = sum(B * h * w_ for h, w_ in c.levels)
    dy, wd, sc = R.pyr_to_rows(gys).to(DEV), w.to(DEV), scale.to(DEV)
    padp = g.dil * (g.kh - 1) - g.pad
    weff = w * scale.view(-1, 1, 1, 1)                   # (fp32, as the packer multiplies)
    for prec in ("f32", "f16"):
        fmt = WFormat.DIRECT if prec == "f32" else ops.amp_format(Cout, Cin)
        fx = (lambda t: t.double()) if prec == "f32" else R.h16
        ref = R.pyr_to_rows([R.dgrad(fx(gl), fx(weff), xl.shape[2:], 1, g.pad, g.dil) for xl, gl in zip(xs, gys)])
        gx = _nan(rows_in, Cin)
        ops.conv_call(Rows(dy), so, fmt.pack(wd, sc, dgrad=True), Rows(gx), Cin=Cout, Cout=Cin, k=g.kh, stride=1, pad=padp, dil=g.dil, precision=fmt.prec, tile=fmt.tile)()
        if prec == "f32":
            rel_close(gx, ref, GRAD, "dgrad-s1-f32", c.id)
        else:
            out_close(gx, ref, "dgrad-s1-" + fmt.name.lower(), c.id, atol=F16_TOL, rtol=F16_TOL)


DGS = [c for c in R.cases(square_only=True) if c.g.stride > 1 and c.g.dil == 1]       # (ops.conv_dgrad_strided describes dilation 1)


@pytest.mark.parametrize("c", DGS, ids=[c.id for c in DGS])
def test_data_gradient_strided(c):
    g, Cin, Cout = c.g, c.Cin, c.Cout
    (x,), w, scale, _, _, (gy,) = R.make_inputs(c)
    H, W = g.H, g.W
    dy, wd, sc = R.to_rows(gy).to(DEV), w.to(DEV), scale.to(DEV)
    weff = w * scale.view(-1, 1, 1, 1)
    empty = any(t == 0 for _, t, _ in ops.strided_dgrad_classes(g.kh, g.stride, g.pad))      # a class without a tap is never written: dX starts as zeros then
    for prec in ("f32", "f16"):
        fx = (lambda t: t.double()) if prec == "f32" else R.h16
        dx = torch.zeros(B * H * W, Cin, device=DEV) if empty else _nan(B * H * W, Cin)
        ok = ops.conv_dgrad_strided(Rows(dy), wd, sc, Rows(dx), B, H, W, g.kh, g.stride, g.pad, precision=PREC[prec])
        torch.cuda.synchronize()
        print(f"[geom] {c.id} {prec}: conv_dgrad_strided {'ran' if ok else 'declined'}")
        if not ok:
            assert bool((dx == 0).all() if empty else torch.isnan(dx).all()), "declined, but wrote to dX"
            continue
        ref4 = R.dgrad(fx(gy), fx(weff), (H, W), g.stride, g.pad, 1)
        if prec == "f32":
            rel_close(dx, R.to_rows(ref4), GRAD, "dgrad-strided-f32", c.id)
        else:
            out_close(dx, R.to_rows(ref4), "dgrad-strided-f16", c.id, atol=F16_TOL, rtol=F16_TOL)
        dead = [h for h in range(H) if float(ref4[:, :, h].abs().max()) == 0.0]              # rows no window reads (geometry 7: row 11)
        dead_w = [j for j in range(W) if float(ref4[:, :, :, j].abs().max()) == 0.0]
        for h in dead:
            assert float(dx.view(B, H, W, Cin)[:, h].abs().max()) == 0.0, f"input row {h} is read by no window: dX must be exactly 0 there"
        for j in dead_w:
            assert float(dx.view(B, H, W, Cin)[:, :, j].abs().max()) == 0.0, f"input column {j} is read by no window: dX must be exactly 0 there"
        assert g.gid != "10c" or (dead == [8] and dead_w == [10])
    if g.gid in ("10a", "10c") and Cout % 32 == 0:
        assert ok, "a k = stride, pad 0 conv has one tap per class and needs no padding: covered"


# ====================================================================================== d. nodes and public layers
def _stock_rungs(Cout: int, k: int, stride: int, pad: int, dil: int) -> int:
    """Stock-op rungs train_ops._dense_dgrad documents for this layer's data gradient (0: it runs on the HIP conv kernel)."""
    if stride == 1 and Cout % 32 == 0 and 0 <= pad <= dil * (k - 1):
        return 0
    if stride > 1 and dil == 1 and Cout % 32 == 0 and all(t == 0 or t - 1 - cc == 0 for _, t, cc in ops.strided_dgrad_classes(k, stride, pad)):
        return 0
    return 1


def _frozen_bn(C: int, gen: torch.Generator) -> nn.BatchNorm2d:
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=gen) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=gen) * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    bn.eval()
    for p in bn.parameters():
        p.requires_grad_(False)
    return bn


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _check_layer(run, conv: nn.Conv2d, bn, x: torch.Tensor, gy: torch.Tensor, res, act: str, amp: bool, what: str, family: str, pad=None, depthwise: bool = False):
    """One forward + backward of `run(conv, bn, x, res)` on the GPU (FD_STRICT off, fallbacks counted) against the float64 layer
    act(bn(conv(x)) + res): forward, dX, dW, d bias, d res.  amp: under torch.autocast(float16), against the reference on f16-rounded operands (what a rung
    that runs on stock fp32 ops computes is compared with the full-precision reference).  The ReLU mask of the gradients is the one of the GPU's own output
    (the output is compared first): an output within rounding of zero must not decide a gradient element.  Returns the number of stock fallbacks taken."""
    k, s, d = conv.kernel_size[0], conv.stride[0], conv.dilation[0]
    pad = conv.padding[0] if pad is None else pad
    Cout = conv.out_channels
    w, b = conv.weight.detach().cpu(), (conv.bias.detach().cpu() if conv.bias is not None else None)
    if bn is not None:
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        shift = bn.bias.double() - bn.running_mean.double() * scale
    else:
        scale, shift = torch.ones(Cout, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64)
    shift_all = shift + (b.double() * scale if b is not None else 0.0)
    groups = conv.groups
    hip_dx = depthwise or _stock_rungs(Cout, k, s, pad, d) == 0
    f16 = amp and not depthwise                      # (the depthwise node computes in fp32 under autocast)
    fx = R.h16 if f16 else (lambda t: t.double())

    def conv64(xx, ww):
        return torch.nn.functional.conv2d(xx, ww, None, s, pad, d, groups)

    y_ref = conv64(fx(x), fx(w)) * scale.view(1, -1, 1, 1) + shift_all.view(1, -1, 1, 1) + (res.double() if res is not None else 0.0)
    y_ref = torch.relu(y_ref) if act == "relu" else y_ref

    cd, bd = copy.deepcopy(conv).to(DEV), (copy.deepcopy(bn).to(DEV) if bn is not None else None)
    xd = _cl(x).requires_grad_(True)
    rd = _cl(res).requires_grad_(True) if res is not None else None
    strict, n0 = T.STRICT, T.STATS["stock_fallbacks"]
    T.STRICT = False
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            y = run(cd, bd, xd, rd)
        assert y.dtype == torch.float32
        (y * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        T.STRICT = strict
    taken = T.STATS["stock_fallbacks"] - n0
    tol = dict(atol=F16_TOL, rtol=F16_TOL) if f16 else {}
    out_close(y, y_ref, family, what + " y", **tol)

    gm = gy.double() * ((y.detach().cpu() > 0) if act == "relu" else 1.0)
    weff = w.float() * scale.float().view(-1, 1, 1, 1)
    if depthwise:
        xr = x.double().clone().requires_grad_(True)
        wr = w.double().clone().requires_grad_(True)
        (conv64(xr, wr) * gm * scale.view(1, -1, 1, 1)).sum().backward()
        dx_ref, dw_ref = xr.grad, wr.grad
    else:
        fdx = R.h16 if (f16 and hip_dx) else (lambda t: t.double())
        dx_ref = R.dgrad(fdx(gm), fdx(weff), x.shape[2:], s, pad, d)
        dw_ref = R.wgrad(fx(x), fx(gm), (k, k), s, pad, d) * scale.view(-1, 1, 1, 1)
    if f16 and hip_dx:
        out_close(xd.grad, dx_ref, family, what + " dX", atol=F16_TOL, rtol=F16_TOL)
    else:
        rel_close(xd.grad, dx_ref, GRAD, family, what + " dX")
    if f16:
        rel_close(cd.weight.grad, dw_ref, 2e-5, family, what + " dW", extra=1e-5)
    else:
        rel_close(cd.weight.grad, dw_ref, PGRAD, family, what + " dW")
    if b is not None:
        rel_close(cd.bias.grad, gm.sum((0, 2, 3)) * scale, PGRAD, family, what + " d bias")
    if res is not None:
        rel_close(rd.grad, gm, GRAD, family, what + " d res")
    return taken


def _raises_strict_in_backward(run, conv, bn, x, res):
    """FD_STRICT on (the suite's default): the forward of a covered layer runs, its stock data-gradient rung raises FdError naming FD_STRICT."""
    assert T.STRICT
    cd, bd = copy.deepcopy(conv).to(DEV), (copy.deepcopy(bn).to(DEV) if bn is not None else None)
    y = run(cd, bd, _cl(x).requires_grad_(True), _cl(res) if res is not None else None)
    with pytest.raises(FdError, match="FD_STRICT"):
        y.sum().backward()
    torch.cuda.synchronize()


NODE = [c for c in R.cases(square_only=True, cin32=True) if not c.pyramid]


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("c", NODE, ids=[c.id for c in NODE])
def test_conv_bn_act_node(c, amp):
    g = c.g
    (x,), w, _, _, (res,), (gy,) = R.make_inputs(c)
    _, use_res, act = _variant(NODE.index(c), 64)
    gen = torch.Generator().manual_seed(R.seed_of(c) + 1)
    conv = nn.Conv2d(c.Cin, c.Cout, g.kh, g.stride, g.pad, g.dil, bias=True)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(torch.randn(c.Cout, generator=gen))
    bn = _frozen_bn(c.Cout, gen)
    assert T.covered(conv, bn, x)

    def run(cv, b_, xx, rr):
        return T.conv_bn_act(cv, b_, xx, ACT[act], residual=rr)
    want = _stock_rungs(c.Cout, g.kh, g.stride, g.pad, g.dil)
    taken = _check_layer(run, conv, bn, x, gy, res if use_res else None, act, amp, c.id, "node-" + ("amp" if amp else "f32"))
    assert taken == want, f"{c.id}: {taken} stock fallbacks, _dense_dgrad documents {want}"
    if want and not amp:
        _raises_strict_in_backward(run, conv, bn, x, res if use_res else None)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("k,st", [(1, 1), (1, 2), (3, 1), (3, 2), (5, 1), (5, 2)])
def test_pointwise_conv_layer(k, st, amp):
    gen = torch.Generator().manual_seed(10 * k + st)
    m = PointWiseConv(32, 64, k, st, bs=True)
    x, Ho, Wo = torch.randn(B, 32, 9, 10, generator=gen), *R.out_hw(9, 10, k, k, st, k // 2, 1)
    gy = torch.randn(B, 64, Ho, Wo, generator=gen)
    want = _stock_rungs(64, k, st, k // 2, 1)
    taken = _check_layer(lambda cv, _b, xx, _r: cv(xx), m, None, x, gy, None, "none", amp, f"PointWiseConv k{k} s{st}", "layer-" + ("amp" if amp else "f32"))
    assert taken == want
    if want and not amp:
        _raises_strict_in_backward(lambda cv, _b, xx, _r: cv(xx), m, None, x, None)


@pytest.mark.parametrize("k,st", [(3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (7, 2)])
def test_depthwise_conv_layer(k, st):
    gen = torch.Generator().manual_seed(100 + 10 * k + st)
    m = DepthWiseConv2d(32, k, st)
    x, Ho, Wo = torch.randn(B, 32, 9, 10, generator=gen), *R.out_hw(9, 10, k, k, st, k // 2, 1)
    gy = torch.randn(B, 32, Ho, Wo, generator=gen)
    if (k, st) == (3, 1):      # the node with a backward
        assert _check_layer(lambda cv, _b, xx, _r: cv(xx), m, None, x, gy, None, "none", False, "DepthWiseConv2d k3 s1", "layer-dw", depthwise=True) == 0
        return
    md = copy.deepcopy(m).to(DEV)
    with torch.no_grad():
        y = md(_cl(x))
    ref = torch.nn.functional.conv2d(x.double(), m.weight.detach().double(), None, st, k // 2, 1, 32)
    out_close(y, ref, "layer-dw", f"DepthWiseConv2d k{k} s{st} y")
    with pytest.raises(FdError, match="forward only"):      # no silent stock backward
        md(_cl(x).requires_grad_(True))


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast"])
@pytest.mark.parametrize("k,padding", [(3, "valid"), (3, "same"), (4, "valid"), (4, "same")])
def test_conv2d_with_string_padding(k, padding, amp):
    gen = torch.Generator().manual_seed(7 * k + len(padding))
    m = nn.Conv2d(32, 64, k, 1, padding)
    x = torch.randn(B, 32, 9, 9, generator=gen)
    with torch.no_grad():
        shape = m(x).shape
    gy = torch.randn(shape, generator=gen)
    if T.covered(m, None, x):
        pad = T._pad_of(m)
        assert pad == (0 if padding == "valid" else (k - 1) // 2)
        run = lambda cv, _b, xx, _r: T.conv2d(cv, xx)      # noqa: E731
        assert _check_layer(run, m, None, x, gy, None, "none", amp, f"Conv2d k{k} '{padding}'", "layer-" + ("amp" if amp else "f32"), pad=pad) == 0
        assert tuple(_layer_conv(copy.deepcopy(m).to(DEV), _cl(x)).shape) == tuple(shape)
        return
    assert (k, padding) == (4, "same")        # torch pads (1, 2): asymmetric, declined
    md, xd = copy.deepcopy(m).to(DEV), _cl(x)
    with pytest.raises(FdError, match="FD_STRICT"):
        T.conv2d(md, xd)
    with pytest.raises(FdError, match="not covered"):
        _layer_conv(md, xd)
    if amp:
        return
    strict, n0 = T.STRICT, T.STATS["stock_fallbacks"]
    T.STRICT = False
    try:
        y = T.conv2d(md, xd.requires_grad_(True))           # the counted stock fallback: the module's own shape and numbers
        (y * gy.to(DEV)).sum().backward()
    finally:
        T.STRICT = strict
    assert T.STATS["stock_fallbacks"] == n0 + 1
    x64 = x.double().requires_grad_(True)
    y64 = copy.deepcopy(m).double()(x64)
    (y64 * gy.double()).sum().backward()
    out_close(y, y64.detach(), "stock", f"Conv2d k{k} '{padding}' y")
    rel_close(xd.grad, x64.grad, GRAD, "stock", f"Conv2d k{k} '{padding}' dX")
