"""MNFCOS trains on the HIP path (opt-in: enable_training()): the dilated depthwise weight-gradient kernel against CPU autograd, the
adjoint identities at full size, MNBlock forward / backward against the oracle's autograd with a frozen and a training-mode BatchNorm,
the whole step (targets, losses, gradients) against the oracle, the default train mode's per-level head statistics, the no-stock-op
rule at 16 x 512 x 512, and the step as one HIP graph / under AMP."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd._lib import Segs
from pytorch_object_detection_amd.model.loss import FCOSLoss
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
from pytorch_object_detection_amd.model.modules.modules import MNBlock
from pytorch_object_detection_amd.model.od import MNFCOS
from test_model_gpu import randomize_norms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(atol=1e-4, rtol=1e-4)                    # the output bar of tests/test_mnfcos_gpu.py
KD = [(3, 1), (3, 2), (5, 1), (5, 2), (7, 1)]       # every (kernel, dilation) MNFCOS uses
STRIDES = [8, 16, 32, 64, 128]
RANGES = [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]]


def _rows(ts, C):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, C) for t in ts]).contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the weight-gradient kernel
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("k,dil", KD)
def test_dilated_dw_weight_gradient_pyramid(k, dil, C):
    """Levels smaller than the dilated footprint (most taps fall outside the map) vs CPU fp32 autograd; scale + torch layout; determinism."""
    gen = torch.Generator().manual_seed(100 * k + 10 * dil + C)
    B, hw = 2, [(9, 14), (5, 7), (2, 3), (1, 1)]
    segs = Segs.make(B, hw)
    xs = [torch.randn(B, C, h, w, generator=gen) for h, w in hw]
    wt = torch.randn(C, 1, k, k, generator=gen).requires_grad_(True)
    dys = [torch.randn(B, C, h, w, generator=gen) for h, w in hw]
    sum((F.conv2d(x, wt, None, 1, dil * (k - 1) // 2, dil, C) * dy).sum() for x, dy in zip(xs, dys)).backward()
    xb, db = _rows(xs, C), _rows(dys, C)
    dw = ops.dwconv_dilated_wgrad(ops.Rows(xb), ops.Rows(db), segs, k, dil)              # [k*k][C]
    ref = wt.grad.reshape(C, k * k).t()
    scale = float(ref.abs().max())
    err = float((dw.cpu() - ref).abs().max()) / scale
    print(f"dilated dw wgrad k={k} dil={dil} C={C}: max |err| / max |ref| = {err:.3e}")
    np.testing.assert_allclose(dw.cpu().numpy() / scale, ref.numpy() / scale, atol=2e-5)
    sc = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    d1 = ops.dwconv_dilated_wgrad(ops.Rows(xb), ops.Rows(db), segs, k, dil, sc, torch_layout=True)
    assert tuple(d1.shape) == (C, 1, k, k)
    np.testing.assert_allclose(d1.reshape(C, k * k).cpu().numpy(), (dw * sc[None, :]).t().cpu().numpy(), rtol=1e-6, atol=1e-6)
    again = ops.dwconv_dilated_wgrad(ops.Rows(xb), ops.Rows(db), segs, k, dil)
    assert torch.equal(dw, again)                                                         # bit-identical


# ------------------------------------------------------------------------------------------------ 2. adjoint identities, full size
@pytest.mark.parametrize("k,dil", KD)
def test_dilated_dw_backward_adjoint_identity_full_size(k, dil):
    """<dw(x, w), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)> in fp64 at batch 16, C = 256, levels 64^2 .. 4^2 (the tolerance of
    test_dwconv_backward_adjoint_identity_full_size)."""
    gen = torch.Generator(device=DEV).manual_seed(3 + k + dil)
    B, C = 16, 256
    segs = Segs.make(B, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)])
    x = torch.randn(segs.rows, C, device=DEV, generator=gen)
    w = torch.randn(C, 1, k, k, device=DEV, generator=gen) / k
    dy = torch.randn(segs.rows, C, device=DEV, generator=gen)
    y, dx = ops.new_rows(segs.rows, C, DEV), ops.new_rows(segs.rows, C, DEV)
    ops.dwconv_dilated(ops.Rows(x), ops.pack_dwk_weight(w), y, segs, k, dil)
    ops.dwconv_dilated(ops.Rows(dy), ops.pack_dwk_weight_reversed(w), dx, segs, k, dil)
    dw = ops.dwconv_dilated_wgrad(ops.Rows(x), ops.Rows(dy), segs, k, dil, torch_layout=True)
    s_y = float((y.buf.double() * dy.double()).sum())
    scale = float(y.buf.double().norm() * dy.double().norm())
    e_w = abs(s_y - float((dw.double() * w.double()).sum())) / scale
    e_x = abs(s_y - float((dx.buf.double() * x.double()).sum())) / scale
    print(f"adjoint k={k} dil={dil}: weight {e_w:.3e}  data {e_x:.3e}")
    assert e_w < 2e-6
    assert e_x < 2e-6


# ------------------------------------------------------------------------------------------------ 3. rejections
def test_dilated_dw_weight_gradient_rejects_bad_arguments():
    """k = 4, dil = 9, C % 4 != 0 and a null workspace each return an error with no launch (the output stays untouched)."""
    lib = _lib.lib()
    segs = Segs.make(2, [(8, 8), (4, 4)])
    C = 128
    x = torch.randn(segs.rows, C, device=DEV)
    dy = torch.randn(segs.rows, C, device=DEV)
    dw = torch.full((49, C), 7.0, device=DEV)
    ws = torch.empty(lib.fd_dwconv_dilated_wgrad_workspace_bytes(ctypes.byref(segs), C, 7) // 4, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    fn = lib.fd_dwconv_dilated_bwd_weight_nhwc
    sp = ctypes.byref(segs)
    assert fn(x.data_ptr(), C, 0, dy.data_ptr(), C, 0, dw.data_ptr(), C, 4, 1, None, 0, sp, ws.data_ptr(), st) < 0
    assert fn(x.data_ptr(), C, 0, dy.data_ptr(), C, 0, dw.data_ptr(), C, 3, 9, None, 0, sp, ws.data_ptr(), st) < 0
    assert fn(x.data_ptr(), C, 0, dy.data_ptr(), C, 0, dw.data_ptr(), 126, 3, 1, None, 0, sp, ws.data_ptr(), st) < 0
    assert fn(x.data_ptr(), C, 0, dy.data_ptr(), C, 0, dw.data_ptr(), C, 3, 1, None, 0, sp, None, st) < 0
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all())
    with pytest.raises(_lib.FdError):
        ops.dwconv_dilated_wgrad(ops.Rows(x), ops.Rows(dy), segs, 4, 1)
    assert fn(x.data_ptr(), C, 0, dy.data_ptr(), C, 0, dw.data_ptr(), C, 3, 1, None, 0, sp, ws.data_ptr(), st) == 0      # and the good call runs
    torch.cuda.synchronize()
    assert not bool((dw[:9] == 7.0).any())


# ------------------------------------------------------------------------------------------------ 4. MNBlock
@pytest.mark.parametrize("bn_mode", ["frozen", "train"])
@pytest.mark.parametrize("k,d", KD)
def test_mn_block_trains_like_the_oracle(k, d, bn_mode, monkeypatch):
    """hip_train on: output, input gradient and every parameter gradient vs CPU autograd of R.mn_block; with a training-mode BatchNorm
    also the running statistics after the step."""
    torch.manual_seed(k * 10 + d)
    blk = MNBlock(128, 128, k, d, 2)
    randomize_norms(blk, k + d)
    train = bn_mode == "train"
    if train:
        monkeypatch.setattr(R, "BN_TRAIN_PREFIXES", ("blk.",))
        blk.train()
    else:
        blk.eval()
        for p in blk.BN.parameters():
            p.requires_grad = False
    sd = {"blk." + n: v.clone().requires_grad_(v.is_floating_point() and "running" not in n) for n, v in blk.state_dict().items()}
    x = torch.randn(2, 128, 11, 7)
    gy = torch.randn(2, 128, 11, 7)
    xr = x.clone().requires_grad_(True)
    ref = R.mn_block(sd, "blk.", xr, k, d)
    (ref * gy).sum().backward()

    blk.hip_train = True
    blk.to(DEV)
    xd = x.to(DEV).to(memory_format=torch.channels_last).requires_grad_(True)
    got = blk(xd)
    assert got.grad_fn is not None
    np.testing.assert_allclose(got.detach().cpu().numpy(), ref.detach().numpy(), **TOL)
    (got * gy.to(DEV)).sum().backward()

    def close(a, b, name):
        s = float(b.abs().max()) + 1e-12
        err = float((a.cpu() - b).abs().max()) / s
        print(f"MNBlock k={k} d={d} BN {bn_mode}: {name} max |err| / max |ref| = {err:.3e}")
        np.testing.assert_allclose(a.cpu().numpy() / s, b.numpy() / s, atol=2e-3, err_msg=name)

    close(xd.grad, xr.grad, "input")
    names = [n for n, p in blk.named_parameters() if p.requires_grad]
    assert "DilatedDepthWiseConv.weight" in names and len(names) == (7 if train else 5)
    for n, p in blk.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        assert p.grad is not None and sd["blk." + n].grad is not None, n
        assert p.grad.stride() == p.stride(), n
        close(p.grad, sd["blk." + n].grad, n)
    if train:
        np.testing.assert_allclose(blk.BN.running_mean.cpu().numpy(), sd["blk.BN.running_mean"].numpy(), atol=2e-5, rtol=2e-4)
        np.testing.assert_allclose(blk.BN.running_var.cpu().numpy(), sd["blk.BN.running_var"].numpy(), atol=2e-5, rtol=2e-4)
        assert int(blk.BN.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ 5. the whole step
def _node_names(t):
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def test_mnfcos_train_step_matches_oracle_autograd():
    torch.manual_seed(0)
    model = MNFCOS([2048, 1024, 512], 20, 256)
    gen = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.75)
    x = torch.randn(2, 3, 128, 128)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]])
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]])

    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in model.state_dict().items()}
    outs = R.mnfcos_forward(sd, x)
    tg = R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], STRIDES, RANGES, gt, labels)
    ref = R.fcos_loss(outs, tg, "giou")
    ref[3].backward()

    model.enable_training()
    model.freeze_all_bn = True          # every BatchNorm on its running statistics (the oracle call above does the same)
    model.to(DEV).train()
    assert not any(b.training for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d))
    model.zero_grad()
    n0 = T.STATS["stock_fallbacks"]
    out = model(x.to(DEV))
    assert T.STATS["stock_fallbacks"] == n0
    names = _node_names(out[0][0]) + _node_names(out[2][4])
    n_dw = len([n for n in _node_names(out[0][0]) if n == "_DwDilatedRowsBackward"])
    assert n_dw >= 7, n_dw              # five FPN blocks + the head's two pyramid-wide ones
    assert "_BottleneckRowsBackward" in names and "_GroupNormRowsBackward" in names and "_UpAddRowsBackward" in names
    target = FCOSGenTargets(STRIDES, RANGES)([out, gt.to(DEV), labels.to(DEV)])
    for a, b in zip(target, tg):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-6)
    losses = FCOSLoss("giou")([out, target])
    print("losses", [float(l.detach()) for l in losses], "oracle", [float(l.detach()) for l in ref])
    np.testing.assert_allclose([float(l.detach()) for l in losses], [float(l.detach()) for l in ref], rtol=2e-4)
    losses[-1].backward()
    params = dict(model.named_parameters())
    checked = 0
    for name in ("FeaturePyramidNetwork.MNB7.DilatedDepthWiseConv.weight", "FeaturePyramidNetwork.MNB5.DilatedDepthWiseConv.weight",
                 "FeaturePyramidNetwork.MNB3.PW1.weight", "FeaturePyramidNetwork.C5PW.bias", "head.block1.DilatedDepthWiseConv.weight",
                 "head.cls_logits.weight", "head.scale_exp.4.scale", "backbone.extract_feature.layer4.2.conv3.weight"):
        p, g_ref = params[name], sd[name].grad
        assert p.grad is not None and g_ref is not None, name
        scale = float(g_ref.abs().max()) + 1e-12
        # relative to the gradient's maximum; looser in the trunk: a ReLU-mask element may flip under another fp32 summation order
        # (tests/test_train_gpu.py::test_train_step_matches_oracle_autograd documents the allowance)
        tol = 2e-2 if name.startswith("backbone.") else 2e-3
        print(f"{name}: max |err| / max |ref| = {float((p.grad.cpu() - g_ref).abs().max()) / scale:.3e} (max |ref| {scale:.3e})")
        np.testing.assert_allclose(p.grad.cpu().numpy() / scale, g_ref.numpy() / scale, atol=tol, err_msg=name)
        checked += 1
    assert checked == 8
    assert model.backbone.conv1.weight.grad is None                     # the stem is frozen by enable_training()
    assert params["FeaturePyramidNetwork.MNB1_P3.PW1.weight"].grad is None     # constructed, never called (MNFcos.py:229)


# ------------------------------------------------------------------------------------------------ 6. default train mode
def test_mnfcos_default_train_mode_batchnorm_follows_the_reference(monkeypatch):
    """FPN and head BatchNorms on batch statistics (only the backbone's stay frozen).  The shared head blocks are called once per level in
    the reference: per-level statistics, running statistics updated five times in the order P3 -> P7."""
    torch.manual_seed(2)
    model = MNFCOS([2048, 1024, 512], 20, 256)
    x = torch.randn(4, 3, 256, 256)
    gt = torch.tensor([[[10., 12., 60., 70.]], [[30., 30., 220., 210.]], [[5., 5., 125., 130.]], [[64., 20., 200., 190.]]])
    labels = torch.tensor([[3], [7], [1], [12]])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    monkeypatch.setattr(R, "BN_TRAIN_PREFIXES", ("FeaturePyramidNetwork.", "head."))
    with torch.no_grad():
        outs = R.mnfcos_forward(sd, x)
    ref = R.fcos_loss(outs, R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], STRIDES, RANGES, gt, labels), "giou")
    model.enable_training().to(DEV).train()
    bns = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert all(m.training == (not n.startswith("backbone.")) for n, m in bns.items())
    out = model(x.to(DEV))
    losses = FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt.to(DEV), labels.to(DEV)])])
    print("losses", [float(v.detach()) for v in losses], "oracle", [float(v) for v in ref])
    np.testing.assert_allclose([float(v.detach()) for v in losses], [float(v) for v in ref], rtol=5e-4)
    losses[-1].backward()
    for n in ("head.block1.BN", "head.block2.BN", "FeaturePyramidNetwork.MNB7.BN", "FeaturePyramidNetwork.MNB3.BN"):
        m = bns[n]
        assert float(m.running_mean.abs().max()) > 0
        print(n, "running_mean max |err|", float((m.running_mean.cpu() - sd[n + ".running_mean"]).abs().max()),
              "running_var max |err|", float((m.running_var.cpu() - sd[n + ".running_var"]).abs().max()))
        np.testing.assert_allclose(m.running_mean.cpu().numpy(), sd[n + ".running_mean"].numpy(), atol=2e-5, rtol=2e-4)
        np.testing.assert_allclose(m.running_var.cpu().numpy(), sd[n + ".running_var"].numpy(), atol=2e-5, rtol=2e-4)
    assert int(bns["head.block1.BN"].num_batches_tracked) == 5          # once per level
    assert int(bns["FeaturePyramidNetwork.MNB5.BN"].num_batches_tracked) == 1
    assert float(bns["FeaturePyramidNetwork.MNB1_P3.BN"].running_mean.abs().max()) == 0      # dead in the reference too
    g = model.head.block1.DilatedDepthWiseConv.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. the default step at 16 x 512^2
def test_default_mnfcos_step_runs_no_stock_op_at_full_size():
    assert T.STRICT, "tests run with FD_STRICT=1 (tests/conftest.py)"
    torch.manual_seed(5)
    model = MNFCOS([2048, 1024, 512], 20, 256).enable_training().to(DEV).train()
    B, S = 16, 512
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, 3, S, S, generator=g).to(DEV)
    c = torch.rand(B, 6, 2, generator=g) * (S - 112) + 50
    sz = torch.rand(B, 6, 2, generator=g) * 150 + 20
    gt = torch.cat([c - sz / 2, c + sz / 2], -1).clamp(0, S - 1).to(DEV)
    labels = torch.randint(1, 21, (B, 6), generator=g).to(DEV)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt.zero_grad()
    T.STATS["stock_fallbacks"] = 0
    out = model(x)
    loss = FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]
    loss.backward()
    torch.cuda.synchronize()
    assert T.STATS["stock_fallbacks"] == 0
    assert bool(torch.isfinite(loss.detach()).all())
    w = model.FeaturePyramidNetwork.MNB6.DilatedDepthWiseConv.weight
    assert w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
    before = w.detach().clone()
    opt.step()
    assert not torch.equal(before, w.detach())


# ------------------------------------------------------------------------------------------------ 8. HIP graph and AMP
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_mnfcos_step_as_one_hip_graph_trains_like_the_eager_loop(amp):
    """The whole MNFCOS step (forward, loss, backward, fused SGD, GradScaler under AMP) recorded once and replayed: the new node is
    capture-safe (no host sync) and the replayed losses follow the same steps enqueued eagerly."""
    from pytorch_object_detection_amd.train_graph import GraphedStep
    torch.manual_seed(0)
    base = MNFCOS([2048, 1024, 512], 20, 256).enable_training().to(DEV).train()
    x = torch.randn(2, 3, 128, 128, device=DEV)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]], device=DEV)
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]], device=DEV)
    gen_t = FCOSGenTargets(STRIDES, RANGES)
    crit = FCOSLoss("giou")

    def make(model):
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4, fused=True)
        scaler = torch.amp.GradScaler("cuda", enabled=amp)

        def step(x_, gt_, labels_):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp, cache_enabled=False):
                out = model(x_)
                losses = crit([out, gen_t([out, gt_, labels_])])
            scaler.scale(losses[-1]).backward()
            scaler.step(opt)
            scaler.update()
            return losses[-1].detach()
        return step

    N = 3
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)
    assert m_graph.head.block1.hip_train                       # the switch survives a deepcopy
    s_eager = make(m_eager)
    losses_e = [float(s_eager(x, gt, labels)) for _ in range(N + 1 + 3)]
    graphed = GraphedStep(make(m_graph), [x, gt, labels], warmup=N)
    losses_g = [float(graphed(x, gt, labels).clone()) for _ in range(4)]
    print("eager", losses_e, "graph", losses_g)
    assert all(np.isfinite(v) for v in losses_e + losses_g)
    np.testing.assert_allclose(losses_g, losses_e[N:], rtol=2e-3 if amp else 1e-5)
