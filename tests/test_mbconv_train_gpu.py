"""FCOS on the EfficientNet trunk trains on the HIP path (opt-in: enable_training()): the two depthwise backward kernels against the float64 closed forms
of tests/mbconv_ref.py on channel views, the adjoint identities at B3's real shapes, the rejections, one MBConv block and the whole step (B0 and B3) against
the oracle's CPU autograd, the scope errors, and the B0 step under AMP and as one HIP graph."""
import copy
import functools

import numpy as np
import pytest
import torch

import mbconv_ref as M
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-4, rtol=1e-4)                    # the project's output bar
STRIDES = [8, 16, 32, 64, 128]
RANGES = [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]]
_ID = lambda v: "-".join(str(i) for i in v).replace(" ", "") if isinstance(v, tuple) else str(v)  # noqa: E731


def _rows(t):
    """NCHW -> [N*H*W, C] rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _in_view(t, cs, co, fill=0.0):
    """NCHW float64 tensor -> fp32 [rows, cs] device buffer holding it at channels [co, co + C) (everything else `fill`) and its Rows view."""
    C = t.shape[1]
    buf = torch.full((t.shape[0] * t.shape[2] * t.shape[3], cs), fill, dtype=torch.float32)
    buf[:, co:co + C] = _rows(t).float()
    buf = buf.to(DEV)
    return buf, ops.Rows(buf, co, C)


# ------------------------------------------------------------------------------------------------ 1. the kernels vs the closed forms
@pytest.mark.parametrize("C", [8, 144])
@pytest.mark.parametrize("geom,hw", M.CASES, ids=_ID)
def test_depthwise_backward_kernels_on_channel_views(geom, hw, C):
    """dx and dw of every table entry at N = 2 against the float64 closed forms; every tensor is a channel view (cs > C, co > 0) whose surroundings
    are canaries; dx starts as NaN and must come back finite everywhere inside the view (no stale pixel); scale, both layouts, bitwise repeatability."""
    k, s, pad = geom
    H, W = hw
    N = 2
    c = M.case(geom, hw, C, N)
    Ho, Wo = c["dy"].shape[2:]
    cs, co = C + 12, 8
    xbuf, x = _in_view(c["x"], cs, co, 7.0)
    gbuf, dy = _in_view(c["dy"], cs + 4, 4, 7.0)
    wkc = ops.pack_dwk_weight(c["w"].float().to(DEV))
    scale = c["scale"].float().to(DEV)
    geo = (N, H, W, k, s, pad[0], pad[0], Ho, Wo)

    def dgrad(sc):
        buf = torch.full((N * H * W, cs), float("nan"), device=DEV)
        ops.dwconv2d_dgrad(dy, wkc, ops.Rows(buf, co, C), *geo, scale=sc)
        return buf

    buf = dgrad(None)
    got = buf[:, co:co + C].cpu()
    assert bool(torch.isfinite(got).all()), "a dx pixel inside the view was left unwritten"
    assert bool(torch.isnan(buf[:, :co]).all()) and bool(torch.isnan(buf[:, co + C:]).all()), "dx: written outside the view"
    ref = _rows(c["dx"])
    print(f"dgrad k={k} s={s} pad={pad} {H}x{W} C={C}: max |err| = {float((got.double() - ref).abs().max()):.3e}")
    np.testing.assert_allclose(got.numpy(), ref.float().numpy(), **TOL)
    assert torch.equal(dgrad(None)[:, co:co + C], buf[:, co:co + C])             # bit-identical
    got_s = dgrad(scale)[:, co:co + C].cpu()
    np.testing.assert_allclose(got_s.numpy(), (ref * c["scale"][None, :]).float().numpy(), **TOL)

    dw = ops.dwconv2d_wgrad(x, dy, *geo)                                         # [k*k][C]
    ref_w = c["dw"].reshape(C, k * k).t()
    m = float(ref_w.abs().max())
    print(f"wgrad k={k} s={s} pad={pad} {H}x{W} C={C}: max |err| / max |ref| = {float((dw.cpu().double() - ref_w).abs().max()) / m:.3e}")
    np.testing.assert_allclose(dw.cpu().numpy() / m, (ref_w / m).float().numpy(), atol=2e-5, rtol=0)
    d1 = ops.dwconv2d_wgrad(x, dy, *geo, scale=scale, torch_layout=True)
    assert tuple(d1.shape) == (C, 1, k, k)
    np.testing.assert_allclose(d1.reshape(C, k * k).cpu().numpy(), (dw * scale[None, :]).t().cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert torch.equal(ops.dwconv2d_wgrad(x, dy, *geo), dw)                     # bit-identical
    # the inputs and their surroundings are untouched
    assert bool((xbuf[:, :co] == 7.0).all()) and bool((xbuf[:, co + C:] == 7.0).all()) and bool((gbuf[:, :4] == 7.0).all())
    assert torch.equal(xbuf[:, co:co + C].cpu(), _rows(c["x"]).float())


def test_cropped_output_leaves_no_stale_input_pixel():
    """An output two rows / columns short of the full one leaves the last input rows and columns unreached: they come back exactly 0."""
    geom, hw, C, N = (5, 2, (2, 2)), (9, 14), 8, 2
    c = M.case(geom, hw, C, N)
    dy64 = c["dy"][:, :, :-2, :-2].contiguous()
    Ho, Wo = dy64.shape[2:]
    _, dy = _in_view(dy64, C, 0)
    buf = torch.full((N * 9 * 14, C), float("nan"), device=DEV)
    ops.dwconv2d_dgrad(dy, ops.pack_dwk_weight(c["w"].float().to(DEV)), ops.Rows(buf), N, 9, 14, 5, 2, 2, 2, Ho, Wo)
    ref = M.dw_dgrad(dy64, c["w"], 2, (2, 2), 9, 14)
    got = buf.cpu().view(N, 9, 14, C).permute(0, 3, 1, 2)
    np.testing.assert_allclose(got.numpy(), ref.float().numpy(), **TOL)
    assert bool((got[:, :, -1] == 0).all()) and bool((got[:, :, :, -1] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. adjoint identities, full size
@pytest.mark.parametrize("k,s,pad,C,HW", [(3, 2, (0, 1), 144, 256), (5, 2, (2, 2), 816, 32)], ids=["b3-block1-k3s2-144x256", "b3-k5s2-816x32"])
def test_depthwise_backward_adjoint_identity_full_size(k, s, pad, C, HW):
    """<dw(x, w), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)> in fp64 at batch 16 and B3's real shapes (the bar of the dilated test)."""
    gen = torch.Generator(device=DEV).manual_seed(7 + k + C)
    N, H, W = 16, HW, HW
    Ho = M.out_size(H, k, s, pad)
    x = torch.randn(N * H * W, C, device=DEV, generator=gen)
    w = torch.randn(C, 1, k, k, device=DEV, generator=gen) / k
    dy = torch.randn(N * Ho * Ho, C, device=DEV, generator=gen)
    wkc = ops.pack_dwk_weight(w)
    y, dx = ops.new_rows(N * Ho * Ho, C, DEV), ops.new_rows(N * H * W, C, DEV)
    geo = (N, H, W, k, s, pad[0], pad[0], Ho, Ho)
    ops.dwconv2d(ops.Rows(x), wkc, y, *geo)
    ops.dwconv2d_dgrad(ops.Rows(dy), wkc, dx, *geo)
    dw = ops.dwconv2d_wgrad(ops.Rows(x), ops.Rows(dy), *geo, torch_layout=True)
    s_y = float((y.buf.double() * dy.double()).sum())
    scale = float(y.buf.double().norm() * dy.double().norm())
    e_w = abs(s_y - float((dw.double() * w.double()).sum())) / scale
    e_x = abs(s_y - float((dx.buf.double() * x.double()).sum())) / scale
    print(f"adjoint k={k} s={s} pad={pad} C={C} {H}x{W}: weight {e_w:.3e}  data {e_x:.3e}")
    assert e_w < 2e-6
    assert e_x < 2e-6


# ------------------------------------------------------------------------------------------------ 3. rejections
def test_depthwise_backward_rejects_bad_arguments():
    """K = 7, stride 3, C = 126, a null workspace and an output that reaches past the input each return an error with no launch (outputs untouched)."""
    lib = _lib.lib()
    N, H, W, C, K, s, Ho, Wo = 2, 8, 7, 128, 3, 2, 4, 3
    x = torch.randn(N * H * W, C, device=DEV)
    dy = torch.randn(N * Ho * Wo, C, device=DEV)
    w = torch.randn(49, C, device=DEV)
    dx = torch.full((N * H * W, C), 7.0, device=DEV)
    dw = torch.full((49, C), 7.0, device=DEV)
    ws = torch.empty(lib.fd_dwconv2d_wgrad_workspace_bytes(N, Ho, Wo, C, 5) // 4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def dgrad(C=C, K=K, s=s, Ho=Ho, Wo=Wo):
        return lib.fd_dwconv2d_bwd_data_nhwc(dy.data_ptr(), 128, 0, w.data_ptr(), None, dx.data_ptr(), 128, 0, N, H, W, C, K, s, 0, 0, Ho, Wo, st)

    def wgrad(C=C, K=K, s=s, Ho=Ho, Wo=Wo, wsp=ws.data_ptr()):
        return lib.fd_dwconv2d_bwd_weight_nhwc(x.data_ptr(), 128, 0, dy.data_ptr(), 128, 0, dw.data_ptr(), C, K, s, 0, 0, N, H, W, Ho, Wo, None, 0, wsp, st)

    for fn in (dgrad, wgrad):
        assert fn(K=7) == _lib.E_UNSUPPORTED
        assert fn(s=3) == _lib.E_UNSUPPORTED
        assert fn(C=126) < 0
        assert fn(Ho=5) < 0 and fn(Wo=5) < 0                  # (Ho - 1) * stride - pad >= H: the output reaches past the input
    assert wgrad(wsp=None) < 0
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((dw == 7.0).all())
    with pytest.raises(FdError):
        ops.dwconv2d_wgrad(ops.Rows(x), ops.Rows(dy), N, H, W, 7, s, 0, 0, Ho, Wo)
    with pytest.raises(FdError):
        ops.dwconv2d_dgrad(ops.Rows(dy), w[:9].contiguous(), ops.Rows(dx), N, H, W, K, 3, 0, 0, Ho, Wo)
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())
    assert dgrad() == 0 and wgrad() == 0                      # and the good calls run
    torch.cuda.synchronize()
    assert not bool((dx == 7.0).any()) and not bool((dw[:9] == 7.0).any()) and bool((dw[9:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 4. one block vs the oracle's autograd
BLOCKS = {  # (kernel, stride, expand, cin, cout, nominal input size)
    "expand1-k3s1": (3, 1, 1, 32, 16, 112),
    "k3s2-pad01-24to40": (3, 2, 6, 24, 40, 112),
    "k5s1-skip-112": (5, 1, 6, 112, 112, 14),
    "k5s2-pad12": (5, 2, 6, 24, 40, 56),
}


def _pad_rows(t, width):
    r = _rows(t)
    return torch.nn.functional.pad(r, (0, width - r.shape[1])).contiguous()


@pytest.mark.parametrize("name", list(BLOCKS))
def test_mbconv_block_trains_like_the_oracle(name):
    """mbconv_rows on maps padded to 32: output, input gradient and every parameter gradient (at its real shape) vs CPU autograd of
    oracle.effnet_ref.mbconv; the pad channels of the output and of the input gradient are exactly 0."""
    k, s, e, cin, cout, nominal = BLOCKS[name]
    torch.manual_seed(k * 10 + s + cin)
    blk = _MBConv(k, s, e, cin, cout, 0.25, nominal).eval()
    init_effnet(blk, 5 + k + s + cin)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            for p in m.parameters():
                p.requires_grad = False
    assert tuple(blk.pad) == {"expand1-k3s1": (1, 1), "k3s2-pad01-24to40": (0, 1), "k5s1-skip-112": (2, 2), "k5s2-pad12": (1, 2)}[name]
    assert blk.skip == (name == "k5s1-skip-112")
    sd = {"blk." + n: v.clone().requires_grad_(v.is_floating_point() and "running" not in n) for n, v in blk.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    N, H, W = 2, 11, 7
    x = torch.randn(N, cin, H, W, generator=gen)
    xr = x.clone().requires_grad_(True)
    ref = E.mbconv(sd, "blk", xr, k, s, e, cin, cout, nominal)
    gy = torch.randn(ref.shape, generator=gen)
    (ref * gy).sum().backward()

    blk.to(DEV)
    cin_p, cout_p = T.round32(cin), T.round32(cout)
    xd = _pad_rows(x, cin_p).to(DEV).requires_grad_(True)
    n0 = T.STATS["stock_fallbacks"]
    got, so = T.mbconv_rows(blk, xd, Segs.make(N, [(H, W)]))
    assert (so.H[0], so.W[0]) == tuple(ref.shape[2:]) and tuple(got.shape) == (N * ref.shape[2] * ref.shape[3], cout_p)
    np.testing.assert_allclose(got[:, :cout].detach().cpu().numpy(), _rows(ref.detach()).numpy(), **TOL)
    assert bool((got[:, cout:] == 0.0).all())
    # the incoming gradient of a padded map has zero pad channels (what the next block's nodes produce)
    (got * _pad_rows(gy, cout_p).to(DEV)).sum().backward()
    assert T.STATS["stock_fallbacks"] == n0
    np.testing.assert_allclose(xd.grad[:, :cin].cpu().numpy(), _rows(xr.grad).numpy(), **TOL)
    assert bool((xd.grad[:, cin:] == 0.0).all())
    checked = 0
    for n, p in blk.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        g_ref = sd["blk." + n].grad
        assert p.grad is not None and g_ref is not None and p.grad.shape == p.shape, n
        print(f"MBConv {name}: {n} max |err| = {float((p.grad.cpu() - g_ref).abs().max()):.3e} (max |ref| {float(g_ref.abs().max()):.3e})")
        np.testing.assert_allclose(p.grad.cpu().numpy(), g_ref.numpy(), err_msg=n, **TOL)
        checked += 1
    assert checked == (6 if e == 1 else 7)      # [expand], depthwise, SE reduce / expand weights and biases, project


# ------------------------------------------------------------------------------------------------ 5. the whole step
# (in_channel, backbone_number, input H x W, initialisation seed).  The seeds are chosen on the REFERENCE's own conditioning: at these the fp32 CPU oracle's
# gradients deviate from the same oracle run in float64 by 5.9e-6 (B0) / 5.4e-6 (B3) of the gradient's maximum in the trunk and 1.7e-4 / 2.9e-4 in FPN + head
# (the stride-2 P6 / P7 convs over 2x1 and 1x1 maps), i.e. under a quarter of the bars below.  Seed 20 on B0 is NOT such an input: a ReLU of the 1x1-pixel head
# towers sits on its threshold and the fp32 oracle itself is 4.0e-2 / 2.1e-2 away from its float64 run.
CONFIGS = {"b0": ([320, 112, 40], 0, (96, 64), 21), "b3": ([384, 136, 48], 3, (64, 96), 23)}


def _fcos_effnet(widths, ncls, feature, number, seed):
    """The model of tests/test_plan_pool_gpu.py::_fcos_effnet (init_effnet trunk, randomised head GroupNorm, head convs x 8), on the CPU."""
    torch.manual_seed(seed)
    model = FCOS(widths, ncls, feature, efficientnet=True, backbone_number=number).eval()
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


def _batch(hw):
    H, W = hw
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H))
    gt = torch.tensor([[[4., 6., 40., 50.], [20., 10., W - 3., H - 5.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., W - 1., H - 1.], [30., 20., 60., 60.]]])
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]])
    return x, gt, labels


@functools.lru_cache(maxsize=None)
def _oracle_step(cfg):
    """(initial state dict, oracle targets, oracle losses, oracle gradients by parameter name) of one config, computed once on the CPU."""
    widths, number, hw, seed = CONFIGS[cfg]
    model = _fcos_effnet(widths, 20, 64, number, seed)
    x, gt, labels = _batch(hw)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd0.items()}
    outs = E.fcos_effnet_forward(sd, x, number)
    tg = R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], STRIDES, RANGES, gt, labels)
    ref = R.fcos_loss(outs, tg, "giou")
    ref[3].backward()
    return sd0, tg, [float(v.detach()) for v in ref], {k: v.grad for k, v in sd.items() if v.grad is not None}


def _model(cfg):
    widths, number, hw, seed = CONFIGS[cfg]
    return _fcos_effnet(widths, 20, 64, number, seed)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_fcos_efficientnet_train_step_matches_oracle_autograd(cfg):
    """Targets, the three losses and their total, and the gradient of EVERY trainable parameter against the oracle's CPU autograd; the stem stays
    without a gradient; no stock fallback and no layout copy over the step.  Bars: those of test_mnfcos_train_step_matches_oracle_autograd (losses
    rtol 2e-4; gradients relative to the reference's maximum, 2e-3, 2e-2 in the trunk)."""
    hw = CONFIGS[cfg][2]
    sd0, tg, ref_losses, ref_grads = _oracle_step(cfg)
    x, gt, labels = _batch(hw)
    model = _model(cfg)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.enable_training()
    model.to(DEV).train()
    assert not any(b.training for b in model.backbone.modules() if isinstance(b, torch.nn.BatchNorm2d))
    model.zero_grad()
    T.STATS["stock_fallbacks"], T.STATS["cl_copies"] = 0, 0
    out = model(x.to(DEV))
    target = FCOSGenTargets(STRIDES, RANGES)([out, gt.to(DEV), labels.to(DEV)])
    for a, b in zip(target, tg):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-6)
    losses = FCOSLoss("giou")([out, target])
    got_losses = [float(v.detach()) for v in losses]
    print(cfg, "losses", got_losses, "oracle", ref_losses)
    losses[-1].backward()
    torch.cuda.synchronize()
    assert T.STATS["stock_fallbacks"] == 0 and T.STATS["cl_copies"] == 0, T.STATS
    np.testing.assert_allclose(got_losses, ref_losses, rtol=2e-4)
    params = dict(model.named_parameters())
    assert params["backbone.model._conv_stem.weight"].grad is None
    worst, checked, bad = {}, 0, []
    for name, p in params.items():
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        g_ref = ref_grads.get(name)
        assert p.grad is not None and g_ref is not None and p.grad.shape == p.shape, name
        scale = float(g_ref.abs().max()) + 1e-12
        err = float((p.grad.cpu() - g_ref).abs().max()) / scale
        grp = "backbone" if name.startswith("backbone.") else "fpn+head"
        if err > worst.get(grp, ("", 0.0))[1]:
            worst[grp] = (name, err)
        if not err <= (2e-2 if grp == "backbone" else 2e-3):
            bad.append((name, err, scale))
        checked += 1
    print(cfg, "gradients checked:", checked, "worst max |err| / max |ref|:", worst)
    assert checked > 100 and not bad, bad


# ------------------------------------------------------------------------------------------------ 6. errors, and the ResNet trunk
def test_scope_errors():
    x = torch.randn(1, 3, 64, 64, device=DEV)
    model = FCOS([320, 112, 40], 20, 64, efficientnet=True).to(DEV).train()
    with pytest.raises(FdError, match=r"enable_training\(\)"):
        model(x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.enable_training()
        loose = FCOS([320, 112, 40], 20, 64, freeze_bn=False, efficientnet=True).enable_training().to(DEV).train()
    with pytest.raises(FdError, match="freeze_bn"):
        loose(x)
    model.backbone.drop_connect_rate = 0.2
    with pytest.raises(FdError, match="drop_connect_rate"):
        model(x)
    model.backbone.drop_connect_rate = 0.0
    out = model(x)
    assert out[0][0].grad_fn is not None
    with pytest.raises(FdError, match="inference-only"):
        EfficientNetV1(0).to(DEV).train()(x)


def test_enable_training_changes_nothing_on_the_resnet_trunk():
    torch.manual_seed(3)
    model = FCOS([2048, 1024, 512], 20, 64).enable_stem_training().to(DEV).train()      # (the trainable 7x7 stem on its HIP node: FD_STRICT)
    x, gt, labels = _batch((64, 64))
    x, gt, labels = x.to(DEV), gt.to(DEV), labels.to(DEV)

    def step():
        model.zero_grad(set_to_none=True)
        out = model(x)
        loss = FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    l0, g0 = step()
    assert model.enable_training() is model and not model.hip_train
    l1, g1 = step()
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 50
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------------ 7. the B0 step under AMP and as one HIP graph
def _b0_on_device():
    import warnings
    model = _model("b0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.enable_training()
    return model.to(DEV).train()


def test_b0_step_under_autocast_tracks_the_fp32_step():
    """autocast + GradScaler: finite gradients for every trainable parameter and a loss within 1 % of the fp32 step (the bar of
    test_amp_train_step_runs_on_f16_mfma_and_tracks_the_fp32_step)."""
    model = _b0_on_device()
    x, gt, labels = (t.to(DEV) for t in _batch(CONFIGS["b0"][2]))
    gen, crit = FCOSGenTargets(STRIDES, RANGES), FCOSLoss("giou")

    def step(amp):
        model.zero_grad(set_to_none=True)
        scaler = torch.amp.GradScaler("cuda", enabled=amp)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = model(x)
            loss = crit([out, gen([out, gt, labels])])[-1]
        scaler.scale(loss).backward()
        return float(loss.detach()), {n: p.grad for n, p in model.named_parameters() if p.requires_grad}

    T.STATS["stock_fallbacks"] = 0
    l32, _ = step(False)
    l16, g16 = step(True)
    print("B0 step loss fp32", l32, "amp", l16)
    assert T.STATS["stock_fallbacks"] == 0
    assert np.isfinite(l16) and abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in g16.values())


def test_b0_step_as_one_hip_graph_trains_like_the_eager_loop():
    """The whole step (forward, loss, backward, fused SGD) recorded once and replayed: no host sync in the new nodes, the same losses as eager."""
    from pytorch_object_detection_amd.train_graph import GraphedStep
    base = _b0_on_device()
    x, gt, labels = (t.to(DEV) for t in _batch(CONFIGS["b0"][2]))
    gen_t, crit = FCOSGenTargets(STRIDES, RANGES), FCOSLoss("giou")

    def make(model):
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4, fused=True)

        def step(x_, gt_, labels_):
            opt.zero_grad(set_to_none=True)
            out = model(x_)
            losses = crit([out, gen_t([out, gt_, labels_])])
            losses[-1].backward()
            opt.step()
            return losses[-1].detach()
        return step

    N = 3
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)
    assert m_graph.hip_train                                   # the switch survives a deepcopy
    s_eager = make(m_eager)
    losses_e = [float(s_eager(x, gt, labels)) for _ in range(N + 1 + 2)]
    graphed = GraphedStep(make(m_graph), [x, gt, labels], warmup=N)
    losses_g = [float(graphed(x, gt, labels).clone()) for _ in range(3)]
    print("eager", losses_e, "graph", losses_g)
    assert all(np.isfinite(v) for v in losses_e + losses_g)
    np.testing.assert_allclose(losses_g, losses_e[N:], rtol=1e-5)
