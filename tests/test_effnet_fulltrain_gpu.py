"""The whole EfficientNet trunk trains on the HIP path: batch-statistics BatchNorm at any width, drop-connect and the stem's weight gradient.

1. fd_batchnorm_train_fwd / _bwd against the float64 closed form (torch autograd in float64), 2. fd_stem_conv_bwd_weight_nhwc4 against float64 autograd of
F.conv2d, 3. fd_sample_scale_add_nhwc against the fp32 torch expression (exact), 4. one MBConv block per geometry with batch statistics and drop-connect,
5. the whole FCOS-B0 / B3 step with all three switches of FCOS.enable_training (and each alone on B0) against tests/effnet_train_ref.py, 6. scope and
regression, 7. the B0 step with all switches under AMP and as one HIP graph.

Kernel tolerances (1, 2): nothing fixed.  e32 = max |torch's own fp32 CPU op - ref64| on the same inputs; the kernel must stay within
4 * e32 + 1e-6 * max |ref64| (tests/test_stem_wgrad_gpu.py's bound)."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import effnet_train_ref as TR
from effnet_init import init_effnet
from oracle import effnet_ref as E
from oracle import torch_ref as R
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd._lib import FdError, Segs
from pytorch_object_detection_amd.model.backbone.efficientnetv1 import EfficientNetV1, _MBConv
from pytorch_object_detection_amd.model.loss import FCOSLoss
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
from pytorch_object_detection_amd.model.od import FCOS
from test_mbconv_train_gpu import BLOCKS, CONFIGS, RANGES, STRIDES, TOL, _batch, _pad_rows, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
EPS, MOM = 1e-3, 0.01
ACTS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU}
RELU_MARGIN = 1e-3          # ReLU cases: every float64 pre-activation is farther than this from 0 (checked when the case is built), far above the bound on y


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bound(ref, f32):
    ref, f32 = np.asarray(ref, dtype=np.float64), np.asarray(f32, dtype=np.float64)
    e32 = float(np.abs(f32 - ref).max())
    return 4 * e32 + 1e-6 * float(np.abs(ref).max()), e32


# ================================================================================================ 1. the BatchNorm kernels
def _act(t, act):
    return F.relu(t) if act == "relu" else (F.silu(t) if act == "silu" else t)


def _bn_torch(x, gamma, beta, dy, rm, rv, act, dtype):
    """torch's CPU op in `dtype`: (y, dx, dgamma, dbeta, running_mean', running_var')."""
    x, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = _act(F.batch_norm(x, rm, rv, gamma, beta, True, MOM, EPS), act)
    y.backward(dy.to(dtype))
    return [t.detach().double().numpy() for t in (y, x.grad, gamma.grad, beta.grad, rm, rv)]


@functools.lru_cache(maxsize=4)
def _bn_case(C, rows, act):
    gen = torch.Generator().manual_seed(1000 * C + 10 * rows + len(act))
    x = torch.randn(rows, C, generator=gen) * (torch.rand(C, generator=gen) + 0.5) + torch.randn(C, generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    dy = torch.randn(rows, C, generator=gen)
    rm, rv = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5

    def stats64(x):
        xd = x.double()
        mean, var = xd.mean(0), xd.var(0, unbiased=False)
        return mean, var, (xd - mean) / torch.sqrt(var + EPS) * gamma.double() + beta.double()

    if act == "relu":       # move pre-activations away from the kink (the statistics move with x: a few passes), then check in float64
        for it in range(12):
            _, var, z = stats64(x)
            close = z.abs() < 4 * RELU_MARGIN
            if not bool(close.any()):
                break
            if it < 6:
                step = (16 * RELU_MARGIN * torch.sqrt(var + EPS) / gamma.double()).float().expand_as(x)
                x = torch.where(close, x + torch.where(z >= 0, step, -step), x)
            else:           # (two rows: xhat is +-1 whatever x is; move the channel's beta instead)
                ch = close.any(0)
                sign = torch.where((z * close).sum(0) >= 0, 1.0, -1.0).float()
                beta = torch.where(ch, beta + 16 * RELU_MARGIN * sign, beta)
        assert float(stats64(x)[2].abs().min()) > RELU_MARGIN, "could not build a ReLU case clear of the kink"
    mean, var, _ = stats64(x)
    c = dict(x=x, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv, mean=mean.numpy(), rstd=(1.0 / torch.sqrt(var + EPS)).numpy())
    c["ref"] = _bn_torch(x, gamma, beta, dy, rm, rv, act, torch.float64)
    c["f32"] = _bn_torch(x, gamma, beta, dy, rm, rv, act, torch.float32)
    c["mean32"] = x.mean(0).double().numpy()
    c["rstd32"] = torch.rsqrt(x.var(0, unbiased=False) + EPS).double().numpy()
    return c


def _view(t, pad, co, fill=float("nan")):
    """[rows, C] CPU tensor -> (device buffer [rows, C + pad] holding it at channels [co, co + C), `fill` elsewhere)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, co:co + t.shape[1]] = t.to(DEV)
    return buf


def _outside_is_nan(buf, co, C):
    return bool(torch.isnan(buf[:, :co]).all()) and bool(torch.isnan(buf[:, co + C:]).all())


def _bn_run(c, act_id, with_running=True):
    """Forward + backward through the C ABI on channel views inside NaN-filled buffers, every output behind canaries.  Returns the outputs on the CPU."""
    lib = _lib.lib()
    rows, C = c["x"].shape
    nb = lib.fd_batchnorm_train_workspace_bytes(rows, C)
    assert nb > 0 and nb % 8 == 0
    xb, gb = _view(c["x"], 12, 8), _view(c["dy"], 8, 4)
    yb = torch.full((rows, C + 8), float("nan"), device=DEV)
    dxb = torch.full((rows, C + 16), float("nan"), device=DEV)
    gm, bt = c["gamma"].to(DEV), c["beta"].to(DEV)
    run = torch.full((2, C + 64), SENTINEL, device=DEV)
    run[0, 32:32 + C], run[1, 32:32 + C] = c["rm"].to(DEV), c["rv"].to(DEV)
    par = torch.full((2, C + 64), SENTINEL, device=DEV)                       # dgamma / dbeta at [32, 32 + C)
    ws = [torch.full((nb // 8 + 32,), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(2)]
    keep = [t.clone() for t in (xb, gb, gm, bt)]
    rc = lib.fd_batchnorm_train_fwd_nhwc(xb.data_ptr(), C + 12, 8, gm.data_ptr(), bt.data_ptr(), yb.data_ptr(), C + 8, 4, rows, C, EPS, act_id, MOM,
                                         run[0, 32:].data_ptr() if with_running else None, run[1, 32:].data_ptr() if with_running else None,
                                         ws[0].data_ptr(), nb, _stream())
    assert rc == 0, lib.fd_last_error()
    rc = lib.fd_batchnorm_train_bwd_nhwc(xb.data_ptr(), C + 12, 8, gb.data_ptr(), C + 8, 4, gm.data_ptr(), bt.data_ptr(), dxb.data_ptr(), C + 16, 12,
                                         par[0, 32:].data_ptr(), par[1, 32:].data_ptr(), rows, C, EPS, act_id, ws[0].data_ptr(), ws[1].data_ptr(), nb, _stream())
    assert rc == 0, lib.fd_last_error()
    torch.cuda.synchronize()
    assert _outside_is_nan(yb, 4, C) and _outside_is_nan(dxb, 12, C), "y / dx: written outside the channel view"
    for t in (run, par):
        if t is par or with_running:
            assert bool((t[:, :32] == SENTINEL).all()) and bool((t[:, 32 + C:] == SENTINEL).all()), "words around the per-channel outputs were written"
    if not with_running:
        assert bool((run[:, :32] == SENTINEL).all()) and torch.equal(run[0, 32:32 + C].cpu(), c["rm"])
    assert all(bool((w[nb // 8:] == SENTINEL).all()) for w in ws), "words past the declared workspace size were written"
    assert all(torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) for a, b in zip((xb, gb, gm, bt), keep)), "an input was modified"
    return dict(y=yb[:, 4:4 + C].cpu(), dx=dxb[:, 12:12 + C].cpu(), dgamma=par[0, 32:32 + C].cpu(), dbeta=par[1, 32:32 + C].cpu(),
                rm=run[0, 32:32 + C].cpu(), rv=run[1, 32:32 + C].cpu(), mean=ws[0][:C].cpu(), rstd=ws[0][C:2 * C].cpu())


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("rows", [2, 37, 4099])
@pytest.mark.parametrize("C", [24, 40, 144, 816, 1392, 2048, 2304, 4096])
def test_batchnorm_train_kernels_match_float64(C, rows, act):
    c = _bn_case(C, rows, act)
    got = _bn_run(c, ACTS[act])
    refs = dict(zip(("y", "dx", "dgamma", "dbeta", "rm", "rv"), zip(c["ref"], c["f32"])))
    refs["mean"], refs["rstd"] = (c["mean"], c["mean32"]), (c["rstd"], c["rstd32"])
    for k, (ref, f32) in refs.items():
        g = got[k].double().numpy()
        assert np.isfinite(g).all(), k
        bound, e32 = _bound(ref, f32)
        err = float(np.abs(g - ref).max())
        print(f"batchnorm C={C} rows={rows} {act} {k}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  max|ref| {np.abs(ref).max():.3e}")
        if act == "relu" and k == "y":
            assert bound < RELU_MARGIN
        assert err <= bound, (k, err, e32, bound)
    again = _bn_run(c, ACTS[act])
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    if (C, rows) == (144, 37):              # without running statistics: the same outputs, the running tensors untouched
        free = _bn_run(c, ACTS[act], with_running=False)
        assert all(torch.equal(free[k], got[k]) for k in ("y", "dx", "dgamma", "dbeta", "mean", "rstd"))


def test_batchnorm_train_rejections_leave_outputs_untouched():
    lib = _lib.lib()
    rows, C = 64, 24
    nb = lib.fd_batchnorm_train_workspace_bytes(rows, C)
    x = torch.randn(rows, 4104, device=DEV)
    out = torch.full((rows, 4104), SENTINEL, device=DEV)
    vec = torch.full((2, 4104), SENTINEL, device=DEV)
    gm = torch.ones(4104, device=DEV)
    ws = torch.full((lib.fd_batchnorm_train_workspace_bytes(rows, 4096) // 8,), SENTINEL, dtype=torch.float64, device=DEV)

    def fwd(rows=rows, C=C, wsp=ws.data_ptr(), nbytes=nb):
        return lib.fd_batchnorm_train_fwd_nhwc(x.data_ptr(), 4104, 0, gm.data_ptr(), gm.data_ptr(), out.data_ptr(), 4104, 0, rows, C, EPS, 0, MOM,
                                               vec[0].data_ptr(), vec[1].data_ptr(), wsp, nbytes, _stream())

    def bwd(rows=rows, C=C, wsp=ws.data_ptr(), nbytes=nb):
        return lib.fd_batchnorm_train_bwd_nhwc(x.data_ptr(), 4104, 0, x.data_ptr(), 4104, 0, gm.data_ptr(), gm.data_ptr(), out.data_ptr(), 4104, 0,
                                               vec[0].data_ptr(), vec[1].data_ptr(), rows, C, EPS, 0, ws.data_ptr(), wsp, nbytes, _stream())

    for fn in (fwd, bwd):
        assert fn(C=6) in (_lib.E_INVAL, _lib.E_UNSUPPORTED) and fn(C=4100) in (_lib.E_INVAL, _lib.E_UNSUPPORTED)
        assert fn(rows=1) in (_lib.E_INVAL, _lib.E_UNSUPPORTED)
        assert fn(wsp=None) == _lib.E_INVAL and fn(nbytes=nb - 8) == _lib.E_INVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((vec == SENTINEL).all()) and bool((ws == SENTINEL).all())
    with pytest.raises(FdError):
        ops.batchnorm_train_workspace(1, 24, DEV)
    with pytest.raises(FdError):
        ops.batchnorm_train_fwd(ops.Rows(x, 0, 6), gm[:6], gm[:6], ops.Rows(out, 0, 6), EPS)
    assert fwd() == 0 and bwd() == 0                                         # and the good calls run
    torch.cuda.synchronize()
    assert not bool((out[:, :C] == SENTINEL).any()) and bool((out[:, C:] == SENTINEL).all())


# ================================================================================================ 2. the stem weight gradient
STEM_SHAPES = [(1, 6, 6, 32), (2, 33, 47, 40), (3, 64, 64, 48), (1, 130, 258, 64)]
STEM_PAD = (0, 1)


@functools.lru_cache(maxsize=None)
def _stem_case(shape):
    N, H, W, Cout = shape
    gen = torch.Generator().manual_seed(H * 7 + W + Cout)
    x = torch.randn(N, 3, H, W, generator=gen)
    Ho, Wo = (H + sum(STEM_PAD) - 3) // 2 + 1, (W + sum(STEM_PAD) - 3) // 2 + 1
    dy = torch.randn(N, Cout, Ho, Wo, generator=gen)
    scale = torch.rand(Cout, generator=gen) + 0.5
    out = dict(x=x, dy=dy, scale=scale, Ho=Ho, Wo=Wo)
    for mode in ("plain", "scale"):
        for dtype, key in ((torch.float64, "ref_"), (torch.float32, "f32_")):
            w = torch.zeros(Cout, 3, 3, 3, dtype=dtype, requires_grad=True)
            o = F.conv2d(F.pad(x.to(dtype), (STEM_PAD[0], STEM_PAD[1], STEM_PAD[0], STEM_PAD[1])), w, stride=2)
            if mode == "scale":
                o = o * scale.to(dtype).view(1, -1, 1, 1)
            o.backward(dy.to(dtype))
            out[key + mode] = w.grad.double().numpy()
    return out


def _stem_raw(x4, dy, dy_cs, dy_co, scale, dw_ptr, ws_ptr, nb, N, H, W, Cout, Ho, Wo, K=3, stride=2):
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())     # noqa: E731
    return _lib.lib().fd_stem_conv_bwd_weight_nhwc4(p(x4), p(dy), dy_cs, dy_co, p(scale), dw_ptr, ws_ptr, nb, N, H, W, Cout, K, stride, STEM_PAD[0], STEM_PAD[0],
                                                    Ho, Wo, _stream())


def _stem_run(shape, c, x4, dy, scale, cs, co):
    N, H, W, Cout = shape
    nb = _lib.lib().fd_stem_conv_wgrad_workspace_bytes(N, H, W, Cout, c["Ho"], c["Wo"])
    assert nb > 0 and nb % 16 == 0
    n = Cout * 27
    big = torch.full((64 + n + 64,), SENTINEL, device=DEV)
    wsb = torch.full((nb // 4 + 256,), SENTINEL, device=DEV)
    rc = _stem_raw(x4, dy, cs, co, scale, big[64:].data_ptr(), wsb.data_ptr(), nb, N, H, W, Cout, c["Ho"], c["Wo"])
    assert rc == 0, _lib.lib().fd_last_error()
    torch.cuda.synchronize()
    big_c = big.cpu()
    assert (big_c[:64] == SENTINEL).all() and (big_c[64 + n:] == SENTINEL).all(), "words around dw were written"
    assert (wsb[nb // 4:] == SENTINEL).all(), "words past the declared workspace size were written"
    return big_c[64:64 + n].view(Cout, 3, 3, 3).clone()


def _x4(x):
    N, _, H, W = x.shape
    x4 = torch.empty(N * H * W, 4, device=DEV)
    ops.nchw3_to_nhwc4(x.to(DEV).contiguous(), x4)
    return x4


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_wgrad_matches_float64_autograd(shape):
    N, H, W, Cout = shape
    c = _stem_case(shape)
    x4 = _x4(c["x"])
    r = c["dy"].permute(0, 2, 3, 1).reshape(-1, Cout)
    dy, dyv = r.to(DEV).contiguous(), _view(r, 8, 4)
    for mode in ("plain", "scale"):
        scale = c["scale"].to(DEV) if mode == "scale" else None
        got = _stem_run(shape, c, x4, dy, scale, Cout, 0)
        ref = c["ref_" + mode]
        bound, e32 = _bound(ref, c["f32_" + mode])
        err = float(np.abs(got.double().numpy() - ref).max())
        print(f"stem3 wgrad {shape} {mode}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  max|ref| {np.abs(ref).max():.3e}")
        assert np.isfinite(got.numpy()).all() and err <= bound, (mode, err, e32, bound)
        assert torch.equal(got, _stem_run(shape, c, x4, dy, scale, Cout, 0)), f"{mode}: two runs differ"
        assert torch.equal(got, _stem_run(shape, c, x4, dyv, scale, Cout + 8, 4)), f"{mode}: the NaN-padded view run differs"
        if mode == "scale":
            w = ops.stem_conv3_wgrad(x4, ops.Rows(dyv, 4, Cout), N, H, W, 3, 2, STEM_PAD[0], STEM_PAD[0], c["Ho"], c["Wo"], scale)
            assert torch.equal(w.cpu(), got)


def test_stem_wgrad_rejections():
    shape = STEM_SHAPES[0]
    N, H, W, Cout = shape
    c = _stem_case(shape)
    x4 = _x4(c["x"])
    dy = torch.randn(N * c["Ho"] * c["Wo"], 72, device=DEV)
    dw = torch.full((72 * 27,), SENTINEL, device=DEV)
    ws = torch.full((64 * 32,), SENTINEL, device=DEV)
    call = lambda **kw: _stem_raw(x4, dy, 72, 0, None, dw.data_ptr(), ws.data_ptr(), ws.numel() * 4, N, H, W, kw.pop("Cout", Cout), c["Ho"], c["Wo"], **kw)  # noqa: E731
    assert call(K=5) == _lib.E_UNSUPPORTED and call(stride=1) == _lib.E_UNSUPPORTED and call(Cout=68) == _lib.E_UNSUPPORTED
    assert _stem_raw(x4, dy, 72, 0, None, dw.data_ptr(), None, 0, N, H, W, Cout, c["Ho"], c["Wo"]) == _lib.E_INVAL
    assert _stem_raw(x4, dy, 72, 0, None, dw.data_ptr(), ws.data_ptr(), 64, N, H, W, Cout, c["Ho"], c["Wo"]) == _lib.E_INVAL
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((ws == SENTINEL).all())
    with pytest.raises(FdError):
        ops.stem_conv3_wgrad(x4, ops.Rows(dy, 0, 68), N, H, W, 3, 2, 0, 0, c["Ho"], c["Wo"])


# ================================================================================================ 3. the per-sample scale-add
@pytest.mark.parametrize("N,HW,C", [(3, 35, 24), (2, 77, 136), (5, 1, 4)])
def test_sample_scale_add_is_the_fp32_expression(N, HW, C):
    gen = torch.Generator().manual_seed(N + HW + C)
    a, r = torch.randn(N * HW, C, generator=gen), torch.randn(N * HW, C, generator=gen)
    s = torch.rand(N, generator=gen) * 2
    s[0] = 0.0
    sr = s.repeat_interleave(HW).view(-1, 1)
    want, want_nor = a * sr + r, a * sr
    ab, rb = _view(a, 12, 8), _view(r, 8, 4)
    yb = torch.full((N * HW, C + 4), float("nan"), device=DEV)
    sd = s.to(DEV)
    ops.sample_scale_add(ops.Rows(ab, 8, C), sd, ops.Rows(rb, 4, C), ops.Rows(yb, 0, C), N, HW)
    assert torch.equal(yb[:, :C].cpu(), want) and bool(torch.isnan(yb[:, C:]).all())
    assert bool((yb[:HW, :C].cpu() == r[:HW]).all())                         # s = 0: the skip input itself
    yb.fill_(float("nan"))
    ops.sample_scale_add(ops.Rows(ab, 8, C), sd, None, ops.Rows(yb, 0, C), N, HW)
    assert torch.equal(yb[:, :C].cpu(), want_nor)
    ops.sample_scale_add(ops.Rows(ab, 8, C), sd, ops.Rows(rb, 4, C), ops.Rows(ab, 8, C), N, HW)      # y aliases a
    assert torch.equal(ab[:, 8:8 + C].cpu(), want) and _outside_is_nan(ab, 8, C)
    assert torch.equal(rb[:, 4:4 + C].cpu(), r) and torch.equal(sd.cpu(), s)


# ================================================================================================ 4. one MBConv block, batch statistics + drop-connect
def _ref_bar(ref32, ref64):
    """The file's bar (TOL) or 4 x the restatement's own fp32-vs-float64 deviation, whichever is larger (absolute, per tensor)."""
    return max(0.0, 4 * float((ref32.double() - ref64).abs().max()))


@pytest.mark.parametrize("name", list(BLOCKS))
def test_mbconv_block_on_batch_statistics_with_drop_connect(name):
    k, s, e, cin, cout, nominal = BLOCKS[name]
    torch.manual_seed(k * 10 + s + cin)
    blk = _MBConv(k, s, e, cin, cout, 0.25, nominal).train()
    init_effnet(blk, 5 + k + s + cin)
    gen = torch.Generator().manual_seed(3)
    N, H, W = 2, 11, 7
    x = torch.randn(N, cin, H, W, generator=gen)
    p_drop, u = 0.2, torch.tensor([0.05, 0.9])                               # sample 0 drops, sample 1 keeps (scaled by 1 / 0.8)
    sc = TR.drop_scale(p_drop, u, torch.float32) if blk.skip else None
    assert sc is None or sc.tolist() == [0.0, 1.25]

    def reference(dtype):
        sd = {"blk." + n: v.clone().to(dtype).requires_grad_(v.is_floating_point() and "running" not in n and "num_batches" not in n)
              if v.is_floating_point() else v.clone() for n, v in blk.state_dict().items()}
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        run = TR.Running()
        out = TR.mbconv(sd, "blk", xr, k, s, e, cin, cout, nominal, batch=True, running=run, scale=None if sc is None else sc.to(dtype))
        return sd, xr, run, out

    sd, xr, run, ref = reference(torch.float32)
    gy = torch.randn(ref.shape, generator=gen)
    (ref * gy).sum().backward()
    sd64, xr64, _, ref64 = reference(torch.float64)
    (ref64 * gy.double()).sum().backward()

    def close(got, r32, r64, what):
        bar = _ref_bar(r32.detach(), r64.detach())
        err = float((got - r32.detach()).abs().max())
        print(f"MBConv(batch stats) {name}: {what} max |err| = {err:.3e} (max |ref| {float(r32.detach().abs().max()):.3e}, 4 x fp32-vs-fp64 {bar:.3e})")
        tol = TOL["atol"] + TOL["rtol"] * r32.detach().abs()
        assert bool(((got - r32.detach()).abs() <= torch.clamp(tol, min=bar)).all()), what

    blk.to(DEV)
    cin_p, cout_p = T.round32(cin), T.round32(cout)
    xd = _pad_rows(x, cin_p).to(DEV).requires_grad_(True)
    n0 = T.STATS["stock_fallbacks"]
    got, so = T.mbconv_rows(blk, xd, Segs.make(N, [(H, W)]), batch_stats=True, drop_scale=sc.to(DEV) if sc is not None else None)
    assert tuple(got.shape) == (N * ref.shape[2] * ref.shape[3], cout_p)
    close(got[:, :cout].detach().cpu(), _rows(ref), _rows(ref64), "output")
    assert bool((got[:, cout:] == 0.0).all())
    (got * _pad_rows(gy, cout_p).to(DEV)).sum().backward()
    assert T.STATS["stock_fallbacks"] == n0
    close(xd.grad[:, :cin].cpu(), _rows(xr.grad), _rows(xr64.grad), "input gradient")
    assert bool((xd.grad[:, cin:] == 0.0).all())
    checked = 0
    for n, p in blk.named_parameters():
        g_ref = sd["blk." + n].grad
        assert p.requires_grad and p.grad is not None and g_ref is not None and p.grad.shape == p.shape, n
        close(p.grad.cpu(), g_ref, sd64["blk." + n].grad, n)
        checked += 1
    assert checked == (6 if e == 1 else 7) + (4 if e == 1 else 6)             # ... + the BatchNorm weights and biases
    for bn_name, (rm, rv, cnt) in run.stats.items():
        m = dict(blk.named_modules())[bn_name[len("blk."):]]
        assert cnt == 1 and int(m.num_batches_tracked) == 1
        np.testing.assert_allclose(m.running_mean.cpu().numpy(), rm.numpy(), **TOL)
        np.testing.assert_allclose(m.running_var.cpu().numpy(), rv.numpy(), **TOL)
    assert len(run.stats) == (2 if e == 1 else 3)


# ================================================================================================ 5. the whole step
ALL = dict(train_stem=True, batch_stats=True, drop_connect_rate=0.2)
SWITCHES = {"all": ALL, "stem": dict(train_stem=True), "batch_stats": dict(batch_stats=True), "drop_connect": dict(drop_connect_rate=0.2)}


def _fcos(cfg, freeze_bn):
    """tests/test_mbconv_train_gpu.py::_fcos_effnet with the freeze_bn argument (the parameters do not depend on it)."""
    widths, number, hw, seed = CONFIGS[cfg]
    torch.manual_seed(seed)
    model = FCOS(widths, 20, 64, freeze_bn=freeze_bn, efficientnet=True, backbone_number=number).eval()
    init_effnet(model.backbone, seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    for m in model.head.modules():
        if isinstance(m, torch.nn.GroupNorm):
            m.weight.data.copy_(torch.rand(m.num_channels, generator=gen) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_channels, generator=gen) * 0.1)
        if isinstance(m, torch.nn.Conv2d):
            with torch.no_grad():
                m.weight.mul_(8.0)
    return model


# The fixed uniform numbers: a seeded draw, then every third skip block is made to drop one of the two samples (the package's rates are <= 0.2, a plain draw
# drops next to nothing; B0: 3 dropped samples).  What the bars rest on is the RESTATEMENT's own conditioning, measured on the CPU: at these sizes the head
# has 1x1-pixel levels whose tower ReLUs sit near their thresholds, and with drop-connect on, the fp32 restatement's FPN + head gradients are 1e-3 ... 3e-1 of
# the gradient's maximum away from its own float64 run depending on the draw (B3, plain draws at seeds 80 ... 91: 1.4e-2, 3.1e-3, 4.1e-2, 2.5e-3, 7.8e-4,
# 8.4e-2, 3.8e-3, 2.8e-1, 2.5e-2, 2.3e-3, 3.8e-3, 3.0e-1).  One fp32 run can agree with float64 by luck -- seed 84 (7.8e-4) is 1.7e-2 away once the fp32 run's
# images are scaled by 1 + 1e-6, and the HIP step showed that same 1.7e-2 against it -- so the draws below were probed three ways (images as they are, scaled
# by 1 + 1e-6 and by 1 - 1e-6; FPN + head): B0 (77, 0) 8.9e-3 / 4.0e-3 / 4.6e-3.  B3 with forced drops, (77, 0), is NOT usable: 2.5e-2 / 2.5e-3 / 2.5e-2 on one
# machine, 2.4e-3 for the same fp32 run on another, and the HIP step 2.5e-2 away; B3 therefore takes the plain draw at seed 96, the best-conditioned of the
# seeds 92 ... 111 probed (1.0e-3 / 1.3e-3 / 1.2e-3), in which one block (23) drops one sample.  B0 (77, 1) is NOT usable either: 8.5e-2 / 2.7e-1 / 4.2e-1.
DROP_SEEDS = {"b0": (77, 0), "b3": (96, None)}       # (seed of the uniform numbers, which third of the skip blocks is made to drop; None: the plain draw)


def _drop_u(cfg):
    """Fixed uniform numbers [len(blocks), 2], none within 0.02 of a block's threshold p (where floor((1 - p) + u) flips)."""
    number = CONFIGS[cfg][1]
    rates = TR.block_rates(E.VALID_MODELS[number], 0.2)
    seed, phase = DROP_SEEDS[cfg]
    u = torch.rand(len(rates), 2, generator=torch.Generator().manual_seed(seed))
    for i, p in enumerate(rates):
        for j in range(2):
            if abs(float(u[i, j]) - p) < 0.02:
                u[i, j] = p + 0.05
    # the rates are small (<= 0.2): so that blocks do drop, every third skip block drops ONE of the two samples, alternately the first and the second
    for n, i in enumerate([i for i, p in enumerate(rates) if p > 0][phase::3] if phase is not None else []):
        u[i, n % 2], u[i, 1 - n % 2] = rates[i] / 2, (1 + rates[i]) / 2
    return u, rates


@functools.lru_cache(maxsize=None)
def _ref_step(cfg, key, dtype):
    """One restatement step on the CPU in `dtype`: (targets, losses, gradients by name, Running)."""
    sw = SWITCHES[key]
    widths, number, hw, seed = CONFIGS[cfg]
    model = _fcos(cfg, not sw.get("batch_stats", False))
    x, gt, labels = _batch(hw)
    frozen = ("_conv_head", "_fc", "backbone.model._bn1") + (() if sw.get("train_stem") else ("_conv_stem", "backbone.model._bn0"))
    bn_trains = sw.get("batch_stats", False)

    def needs_grad(k, v):
        if not v.is_floating_point() or "running" in k or any(f in k for f in frozen):
            return False
        is_bn = k.startswith("backbone.") and ("_bn0." in k or "_bn1." in k or "_bn2." in k)
        return bn_trains or not is_bn

    sd = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    sd = {k: v.requires_grad_(needs_grad(k, v)) for k, v in sd.items()}
    run = TR.Running()
    drop_u = _drop_u(cfg)[0] if sw.get("drop_connect_rate") else None
    outs = TR.fcos_effnet_forward(sd, x.to(dtype), number, train_stem=bool(sw.get("train_stem")), batch_stats=bn_trains,
                                  drop_rate=sw.get("drop_connect_rate", 0.0), drop_u=drop_u, running=run)
    tg = R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], STRIDES, RANGES, gt, labels)
    ref = R.fcos_loss(outs, tg, "giou")
    ref[3].backward()
    return tg, [float(v.detach()) for v in ref], {k: v.grad.double() for k, v in sd.items() if v.grad is not None}, run


def _group(name):
    if name.startswith("backbone.model._conv_stem") or name.startswith("backbone.model._bn0"):
        return "stem"
    return "trunk" if name.startswith("backbone.") else "fpn+head"


def _expected_zero_class(cfg, key):
    """The parameters whose true gradient is 0 on batch statistics: the _bn2.bias of every block whose output stream reaches nothing but 1x1 expand convs
    followed by a batch-statistics BatchNorm (the stages whose last block is not one of the three endpoints; every later block of the stage and the next
    stage's first block must have an expand conv) and whose branch is scaled alike for every sample (no drop-connect, or uniform numbers that keep or drop the
    whole batch).  B0: 10 parameters without drop-connect."""
    sw = SWITCHES[key]
    if not sw.get("batch_stats"):
        return set()
    number = CONFIGS[cfg][1]
    _, blocks, _, _ = E.block_table(E.VALID_MODELS[number])
    ends = [i for i in range(len(blocks)) if i + 1 == len(blocks) or blocks[i + 1][1] > 1][-3:]
    u, rates = _drop_u(cfg)
    out, stage = set(), []
    for i, b in enumerate(blocks):
        stage.append(i)
        if i + 1 == len(blocks) or not (blocks[i + 1][1] == 1 and blocks[i + 1][3] == blocks[i + 1][4]):      # the next block opens a new stream
            if i not in ends:
                for j in stage:
                    mixed = sw.get("drop_connect_rate") and rates[j] > 0 and len({float(v) for v in TR.drop_scale(rates[j], u[j], torch.float32)}) > 1
                    pointwise = all(blocks[c][2] != 1 for c in range(j + 1, i + 2))      # (a zero-padded depthwise conv does not pass a constant on as one)
                    if not mixed and pointwise:
                        out.add(f"backbone.model._blocks.{j}._bn2.bias")
            stage = []
    return out


def _run_step(cfg, key):
    sw = SWITCHES[key]
    hw = CONFIGS[cfg][2]
    tg, ref_losses, g32, run = _ref_step(cfg, key, torch.float32)
    _, _, g64, _ = _ref_step(cfg, key, torch.float64)
    x, gt, labels = _batch(hw)
    model = _fcos(cfg, not sw.get("batch_stats", False))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.enable_training(**sw)
    model.to(DEV).train()
    model.zero_grad()
    T.STATS["stock_fallbacks"], T.STATS["cl_copies"] = 0, 0
    drop_u = _drop_u(cfg)[0].to(DEV) if sw.get("drop_connect_rate") else None
    out = model(x.to(DEV), drop_u=drop_u)
    target = FCOSGenTargets(STRIDES, RANGES)([out, gt.to(DEV), labels.to(DEV)])
    for a, b in zip(target, tg):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-6)
    losses = FCOSLoss("giou")([out, target])
    got_losses = [float(v.detach()) for v in losses]
    print(cfg, key, "losses", got_losses, "restatement", ref_losses)
    losses[-1].backward()
    torch.cuda.synchronize()
    assert T.STATS["stock_fallbacks"] == 0 and T.STATS["cl_copies"] == 0, T.STATS
    np.testing.assert_allclose(got_losses, ref_losses, rtol=2e-4)
    params = dict(model.named_parameters())
    assert (params["backbone.model._conv_stem.weight"].grad is not None) == bool(sw.get("train_stem"))
    # the restatement's own conditioning per group (fp32 vs float64, relative to the parameter's maximum), and the structurally-zero class
    top = max(float(g.abs().max()) for g in g64.values())
    # (a float64 gradient that is EXACTLY 0 -- the ScaleExp of a level without a positive location -- is not of this class: the ordinary rule below asks the same 0)
    zero = {n for n, g in g64.items() if 0.0 < float(g.abs().max()) < 1e-9 * top}
    assert zero == _expected_zero_class(cfg, key), zero ^ _expected_zero_class(cfg, key)
    fig = {}
    for n, g in g64.items():
        if n not in zero and float(g.abs().max()) > 0.0:
            fig[_group(n)] = max(fig.get(_group(n), 0.0), float((g32[n] - g).abs().max()) / float(g.abs().max()))
    zero_bar = 4 * max([float(g32[n].abs().max()) for n in zero], default=0.0)
    print(cfg, key, "restatement fp32-vs-float64 per group:", fig, "| structurally zero:", len(zero), "parameters, bar", zero_bar)
    worst, checked, bad = {}, 0, []
    for name, p in params.items():
        if not p.requires_grad:
            assert p.grad is None and name not in g32, name
            continue
        g_ref = g32.get(name)
        assert p.grad is not None and g_ref is not None and p.grad.shape == p.shape, name
        if name in zero:
            if not float(p.grad.abs().max()) <= zero_bar:
                bad.append((name, float(p.grad.abs().max()), zero_bar))
            checked += 1
            continue
        grp = _group(name)
        scale = float(g_ref.abs().max()) + 1e-12
        err = float((p.grad.cpu().double() - g_ref).abs().max()) / scale
        if err > worst.get(grp, ("", 0.0))[1]:
            worst[grp] = (name, err)
        if not err <= max(2e-3 if grp == "fpn+head" else 2e-2, 4 * fig[grp]):
            bad.append((name, err, scale))
        checked += 1
    print(cfg, key, "gradients checked:", checked, "worst max |err| / max |ref|:", worst)
    assert checked > 100 and not bad, bad
    if sw.get("batch_stats"):
        mods = dict(model.named_modules())
        assert len(run.stats) > 40
        for bn_name, (rm, rv, cnt) in run.stats.items():
            m = mods[bn_name]
            assert cnt == 1 and int(m.num_batches_tracked) == 1, bn_name
            np.testing.assert_allclose(m.running_mean.cpu().numpy(), rm.numpy(), atol=1e-4, rtol=1e-4, err_msg=bn_name)
            np.testing.assert_allclose(m.running_var.cpu().numpy(), rv.numpy(), atol=1e-4, rtol=1e-4, err_msg=bn_name)
    return zero


# Conditioning of the restatement (fp32 vs float64 run of tests/effnet_train_ref.py on the CPU, max |delta| / max |ref64| per parameter, worst per group) with
# the drop_u of _drop_u(); every run prints it ("restatement fp32-vs-float64 per group") and the bars are max(2e-2 trunk and stem / 2e-3 FPN + head, 4 x it):
#                          trunk     stem      FPN + head   loss (relative)   structurally zero (fp32 restatement's largest)
#   B0, all switches       3.7e-5    3.7e-5    8.9e-3       (printed)         10 minus the skip blocks that drop one sample
#   B3, all switches       1.5e-4    7.7e-5    1.0e-3       1.9e-6            14 parameters (3.4e-7)
#   B0, stem only          5.8e-6    2.5e-6    1.7e-4       2.8e-8            none
#   B0, batch statistics   1.1e-4    -         1.4e-1       1.9e-7            10 parameters (2.2e-7)
#   B0, drop-connect only  (printed by the run)
# (FPN + head at 1.4e-1 with batch statistics alone: with the stem folded on its running statistics a ReLU of the 1x1-pixel head towers sits close to its
# threshold at this seed and the fp32 restatement itself is that far from its float64 run; the bar follows it.)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_full_train_step_matches_the_restatement(cfg):
    """Targets, losses and the gradient of EVERY trainable parameter -- the stem and every trunk BatchNorm included -- with train_stem, batch_stats and
    drop-connect on; running statistics; no stock fallback, no layout copy."""
    _run_step(cfg, "all")


@pytest.mark.parametrize("key", ["stem", "batch_stats", "drop_connect"])
def test_each_switch_alone_b0(key):
    zero = _run_step("b0", key)
    assert len(zero) == (10 if key == "batch_stats" else 0)


# ================================================================================================ 6. scope and regression
def _one_step(model, x, gt, labels):
    model.zero_grad(set_to_none=True)
    out = model(x)
    loss = FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_default_paths_are_bit_identical():
    """The ResNet-trunk step and today's enable_training() EfficientNet step against a second model built the same way that never touches the switches."""
    x, gt, labels = (t.to(DEV) for t in _batch((64, 64)))

    def resnet(touch):
        torch.manual_seed(3)
        m = FCOS([2048, 1024, 512], 20, 64).enable_stem_training()
        if touch:
            m.enable_training(train_stem=True, batch_stats=True, drop_connect_rate=0.2)           # the ResNet trunk: does nothing
        return m.to(DEV).train()

    def effnet(touch):
        m = _fcos("b0", True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.enable_training(train_stem=False, batch_stats=False, drop_connect_rate=0.0) if touch else m.enable_training()
        return m.to(DEV).train()

    for build, n_min in ((resnet, 50), (effnet, 100)):
        (l0, g0), (l1, g1) = _one_step(build(False), x, gt, labels), _one_step(build(True), x, gt, labels)
        assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > n_min
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n


def test_scope_errors_that_remain(monkeypatch):
    x = torch.randn(1, 3, 64, 64, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loose = FCOS([320, 112, 40], 20, 64, freeze_bn=False, efficientnet=True).enable_training(train_stem=True).to(DEV).train()
        model = FCOS([320, 112, 40], 20, 64, efficientnet=True).enable_training(train_stem=True).to(DEV).train()
    with pytest.raises(FdError, match="freeze_bn"):
        loose(x)                                              # freeze_bn=False without batch_stats
    model.backbone.drop_connect_rate = 0.2                    # by hand, without the switch
    with pytest.raises(FdError, match="drop_connect_rate"):
        model(x)
    model.backbone.drop_connect_rate = 0.0
    assert model(x)[0][0].grad_fn is not None
    with pytest.raises(FdError, match="freeze_bn=False"):
        FCOS([320, 112, 40], 20, 64, efficientnet=True).enable_training(batch_stats=True)
    with pytest.raises(FdError, match="inference-only"):
        EfficientNetV1(0).to(DEV).train()(x)
    bn = torch.nn.SyncBatchNorm(144).to(DEV).train()
    monkeypatch.setattr(T, "_is_sync", lambda m: isinstance(m, torch.nn.SyncBatchNorm))          # as in a process group of more than one rank
    with pytest.raises(FdError, match="no synchronised form"):
        T.batchnorm_train_wide_rows(bn, torch.zeros(8, 160, device=DEV))


# ================================================================================================ 7. AMP and graph, all switches on
def _b0_all():
    model = _fcos("b0", False).enable_training(**ALL)
    return model.to(DEV).train()


def test_b0_full_step_under_autocast_tracks_the_fp32_step():
    model = _b0_all()
    x, gt, labels = (t.to(DEV) for t in _batch(CONFIGS["b0"][2]))
    u = _drop_u("b0")[0].to(DEV)
    gen, crit = FCOSGenTargets(STRIDES, RANGES), FCOSLoss("giou")

    def step(amp):
        model.zero_grad(set_to_none=True)
        scaler = torch.amp.GradScaler("cuda", enabled=amp)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = model(x, drop_u=u)
            loss = crit([out, gen([out, gt, labels])])[-1]
        scaler.scale(loss).backward()
        return float(loss.detach()), {n: p.grad for n, p in model.named_parameters() if p.requires_grad}

    T.STATS["stock_fallbacks"] = 0
    l32, _ = step(False)
    l16, g16 = step(True)
    print("B0 full step loss fp32", l32, "amp", l16)
    assert T.STATS["stock_fallbacks"] == 0
    assert np.isfinite(l16) and abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert "backbone.model._conv_stem.weight" in g16 and "backbone.model._blocks.3._bn1.weight" in g16
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in g16.values())


def test_b0_full_step_as_one_hip_graph():
    """Forward (torch.rand drop-connect masks included), loss, backward and fused SGD captured once: it captures, replays twice with finite losses, and the
    parameters move."""
    from pytorch_object_detection_amd.train_graph import GraphedStep
    model = _b0_all()
    x, gt, labels = (t.to(DEV) for t in _batch(CONFIGS["b0"][2]))
    gen_t, crit = FCOSGenTargets(STRIDES, RANGES), FCOSLoss("giou")
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4, fused=True)

    def step(x_, gt_, labels_):
        opt.zero_grad(set_to_none=True)
        out = model(x_)
        losses = crit([out, gen_t([out, gt_, labels_])])
        losses[-1].backward()
        opt.step()
        return losses[-1].detach()

    graphed = GraphedStep(step, [x, gt, labels], warmup=3)
    names = ("backbone.model._conv_stem.weight", "backbone.model._blocks.5._bn2.weight", "head.cls_logits.weight")
    params = dict(model.named_parameters())
    before = {n: params[n].detach().clone() for n in names}
    tracked = int(model.backbone.model._blocks[5]._bn2.num_batches_tracked)
    losses = [float(graphed(x, gt, labels).clone()) for _ in range(2)]
    print("graph replays", losses)
    assert all(np.isfinite(v) for v in losses)
    assert all(not torch.equal(before[n], params[n].detach()) for n in names)
    assert int(model.backbone.model._blocks[5]._bn2.num_batches_tracked) == tracked + 2
