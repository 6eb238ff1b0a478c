"""The ResNet-50 trunk trains on batch statistics on the HIP path (PlannedModule.enable_trunk_batch_stats): one bottleneck on rows against the CPU
restatement of tests/resnet_bn_ref.py in fp32 and float64, then the whole models -- HISFCOS-R50, FCOS-R50, MNFCOS -- under FD_STRICT as the suite sets it,
a trunk with frozen stages, one step under autocast + GradScaler, and the untouched default.

Bars.  Block: tests/test_effnet_fulltrain_gpu.py::test_mbconv_block_on_batch_statistics_with_drop_connect's -- per element the file's TOL (atol = rtol =
1e-4) or 4 x the restatement's own fp32-vs-float64 deviation of that tensor, whichever is larger; the cases are clear of the three ReLU kinks by 1e-4 in
float64 (resnet_bn_ref.build_case).  Whole model: the protocol and the numbers of tests/test_train_gpu.py::test_unfrozen_batchnorm_trains_with_hip_convs --
outputs within atol = rtol = 5e-3 of the all-stock graph, per named gradient a median deviation of at most 3 x what the all-stock graph shows against
itself under a 1e-6 perturbation of the input, + 1e-4."""
import numpy as np
import pytest
import torch

import resnet_bn_ref as BR
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd.model.od import FCOS, MNFCOS, HalfInvertedStageFCOS
from test_effnet_fulltrain_gpu import _one_step, _ref_bar
from test_mbconv_train_gpu import TOL, _batch, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW_NODES = ("_BatchNormResRowsBackward",)


def _node_names(out):
    """The autograd node type names of the graph behind a tensor or a model's output groups, each node once."""
    roots = [out] if isinstance(out, torch.Tensor) else [t for grp in out for t in grp]
    seen, names, stack = set(), [], [t.grad_fn for t in roots]
    while stack:
        fn = stack.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            names.append(type(fn).__name__)
            stack.extend(f for f, _ in fn.next_functions)
    return names


def _trunk_bns(model):
    return {n: m for n, m in model.backbone.named_modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.SyncBatchNorm))}


def _weighted_sum(out, seed=9):
    torch.manual_seed(seed)
    return sum((t * torch.randn(t.shape, device=DEV)).sum() for grp in out for t in grp)


# ================================================================================================ 1. one block on rows
@pytest.mark.parametrize("name", list(BR.CASES))
def test_bottleneck_on_batch_statistics(name):
    assert T.STRICT, "the suite runs with FD_STRICT=1"
    blk, x, gy, seed = BR.build_case(name)
    stride = BR.CASES[name][2]
    margin = BR.kink_distance(blk, x, stride)
    assert margin > BR.KINK_MARGIN
    sd, xr, ref, run = BR.reference(blk, x, gy, torch.float32)
    sd64, xr64, ref64, _ = BR.reference(blk, x, gy, torch.float64)
    print(f"bottleneck {name}: seed {seed}, float64 |pre-activation| >= {margin:.3e}, output fp32-vs-float64 {float((ref.double() - ref64).abs().max()):.3e}")

    def close(got, r32, r64, what):
        bar = _ref_bar(r32.detach(), r64.detach())
        err = float((got - r32.detach()).abs().max())
        print(f"bottleneck {name}: {what} max |err| = {err:.3e} (max |ref| {float(r32.detach().abs().max()):.3e}, 4 x fp32-vs-fp64 {bar:.3e})")
        tol = TOL["atol"] + TOL["rtol"] * r32.detach().abs()
        assert bool(((got - r32.detach()).abs() <= torch.clamp(tol, min=bar)).all()), what

    blk.to(DEV)
    N, _, H, W = x.shape
    xd = _rows(x).contiguous().to(DEV).requires_grad_(True)                  # the block's input as rows; the NCHW-shaped tensor below is a view of it
    n0 = T.STATS["stock_fallbacks"]
    got = T.bottleneck(blk, T.from_rows(xd, N, H, W), batch_stats=True)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    names = _node_names(got)
    assert names.count("_BatchNormResRowsBackward") == 1 and "_BottleneckRowsBackward" not in names
    assert not [n for n in names if "NativeBatchNorm" in n or "ConvolutionBackward" in n], names
    close(_rows(got.detach().cpu()), _rows(ref), _rows(ref64), "output")
    (got * gy.to(DEV)).sum().backward()
    assert T.STATS["stock_fallbacks"] == n0
    close(xd.grad.cpu(), _rows(xr.grad), _rows(xr64.grad), "input gradient")
    checked = 0
    for n, p in blk.named_parameters():
        assert p.grad is not None and sd[n].grad is not None and p.grad.shape == p.shape, n
        close(p.grad.cpu(), sd[n].grad, sd64[n].grad, n)
        checked += 1
    assert checked == (12 if blk.downsample is not None else 9)              # 3 (4) convs + the weight and bias of 3 (4) BatchNorms
    mods = dict(blk.named_modules())
    assert len(run) == (4 if blk.downsample is not None else 3)
    for bn_name, (rm, rv) in run.items():
        m = mods[bn_name]
        assert int(m.num_batches_tracked) == 1
        np.testing.assert_allclose(m.running_mean.cpu().numpy(), rm.numpy(), **TOL)
        np.testing.assert_allclose(m.running_var.cpu().numpy(), rv.numpy(), **TOL)


def test_residual_node_refuses_what_it_does_not_differentiate():
    bn = torch.nn.BatchNorm2d(64).to(DEV).train()
    x, r = torch.randn(10, 64, device=DEV), torch.randn(10, 64, device=DEV)
    with pytest.raises(_lib.FdError, match="ACT_NONE / ACT_RELU"):
        T.batchnorm_train_res_rows(bn, x, r, _lib.ACT_SILU)
    with pytest.raises(_lib.FdError, match="residual"):
        T.batchnorm_train_res_rows(bn, x, r[:, :32], _lib.ACT_RELU)
    with pytest.raises(_lib.FdError, match="training mode"):
        T.batchnorm_train_res_rows(bn.eval(), x, r, _lib.ACT_RELU)
    assert int(bn.num_batches_tracked) == 0
    y = T.batchnorm_train_res_rows(bn.train(), x.requires_grad_(True), r.requires_grad_(True), _lib.ACT_NONE)       # act NONE: no mask pass, g is dres
    g = torch.randn_like(y)
    y.backward(g)
    assert torch.equal(r.grad, g) and int(bn.num_batches_tracked) == 1


# ================================================================================================ 2. the whole models
def test_hisfcos_r50_trains_on_batch_statistics_under_strict_mode():
    """Forward + backward with FD_STRICT on and no stock fallback; every trainable parameter gets a finite gradient; every trunk BatchNorm's running
    statistics move; outputs and gradients against the all-stock graph by the protocol of test_unfrozen_batchnorm_trains_with_hip_convs."""
    assert T.STRICT
    torch.manual_seed(4)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats().to(DEV).train()
    x = torch.randn(4, 3, 384, 384, device=DEV)
    bns = _trunk_bns(model)
    assert len(bns) == 53 and all(b.training for b in bns.values())
    T.STATS["stock_fallbacks"] = 0
    moved = {}

    def run(stock, xx):
        T._STOCK = stock
        try:
            model.zero_grad()
            sd = {k: v.clone() for k, v in model.state_dict().items()}      # running stats move: restore afterwards
            out = model(xx)
            names = _node_names(out) if not stock else []
            _weighted_sum(out).backward()
            res = ([t.detach().clone() for grp in out for t in grp], {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, names)
            if not stock:
                for n, b in bns.items():
                    moved[n] = (int(b.num_batches_tracked), not torch.equal(b.running_mean, sd["backbone." + n + ".running_mean"]),
                                not torch.equal(b.running_var, sd["backbone." + n + ".running_var"]))
            model.load_state_dict(sd)
            return res
        finally:
            T._STOCK = False

    o1, g1, names = run(False, x)
    assert T.STATS["stock_fallbacks"] == 0                                   # strict mode on: a fallback would have raised
    assert names.count("_BatchNormResRowsBackward") == 16 and "_BottleneckRowsBackward" not in names
    assert not [n for n in names if "NativeBatchNorm" in n or "ConvolutionBackward" in n]
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    used = trainable - {n for n in trainable if n.startswith("fpn.gn3.")}    # (gn3 exists and is never used, as in the reference)
    assert used <= set(g1) and all(bool(torch.isfinite(g1[n]).all()) for n in used), sorted(used - set(g1))
    assert all(f"backbone.{n}.{w}" in g1 or f"backbone.extract_feature.{n}.{w}" in g1 for n in bns for w in ("weight", "bias"))
    assert all(v == (1, True, True) for v in moved.values()), {n: v for n, v in moved.items() if v != (1, True, True)}
    (o2, g2, _), (_, g3, _) = run(True, x), run(True, x * (1 + 1e-6))
    for a, b in zip(o1, o2):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=5e-3, rtol=5e-3)
    assert g1.keys() == g2.keys() and "backbone.conv1.weight" in g1

    def med(a, b):
        return float(((a - b).abs() / (float(b.abs().max()) + 1e-12)).median())

    for n in ("head.cls_logits.weight", "head.pw1.weight", "fpn.tf1.weight", "backbone.extract_feature.layer3.0.conv2.weight", "backbone.conv1.weight",
              "backbone.extract_feature.layer3.0.bn3.weight", "backbone.extract_feature.layer3.0.downsample.1.weight"):
        print(f"{n}: median deviation from the all-stock graph {med(g1[n], g2[n]):.3e}, the all-stock graph's own under 1e-6 {med(g3[n], g2[n]):.3e}")
        assert med(g1[n], g2[n]) <= 3 * med(g3[n], g2[n]) + 1e-4, (n, med(g1[n], g2[n]), med(g3[n], g2[n]))


def _step_without_fallbacks(model, hw=(128, 128), batch=2):
    assert T.STRICT
    x = torch.randn(batch, 3, *hw, device=DEV)
    T.STATS["stock_fallbacks"] = 0
    model.zero_grad()
    out = model(x)
    names = _node_names(out)
    _weighted_sum(out).backward()
    assert T.STATS["stock_fallbacks"] == 0
    assert not [n for n in names if "NativeBatchNorm" in n or "ConvolutionBackward" in n]
    bns = _trunk_bns(model)
    assert all(int(b.num_batches_tracked) == 1 for b in bns.values() if b.training)
    for n, p in model.backbone.named_parameters():
        assert not p.requires_grad or (p.grad is not None and bool(torch.isfinite(p.grad).all())), n
    return names


def test_fcos_r50_trains_on_batch_statistics_without_fallbacks():
    torch.manual_seed(5)
    model = FCOS([2048, 1024, 512], 20, 64, freeze_bn=False).enable_stem_training().enable_trunk_batch_stats().to(DEV).train()
    names = _step_without_fallbacks(model)
    assert names.count("_BatchNormResRowsBackward") == 16 and "_BottleneckRowsBackward" not in names


def test_mnfcos_trains_on_batch_statistics_without_fallbacks():
    torch.manual_seed(6)
    model = MNFCOS([2048, 1024, 512], 20, 64, freeze_bn=False).enable_training(train_stem=True).enable_trunk_batch_stats().to(DEV).train()
    names = _step_without_fallbacks(model)
    assert names.count("_BatchNormResRowsBackward") == 16 and "_BottleneckRowsBackward" not in names


def test_frozen_stages_keep_the_fused_node_beside_the_new_path():
    """backbone.freeze_stages(2) after construction, those stages in eval mode: the stem and layer1-2 are frozen, layer3-4 run on batch statistics (6 + 3
    blocks).  A block whose parameters are all frozen behind a frozen stem leaves no node in the graph at all, so the conv weights of layer1-2 are made
    trainable again: their BatchNorms stay frozen and the 3 + 4 blocks take _BottleneckRows.  (FCOS-R50: its backbone holds layer1..layer4, which
    freeze_stages walks.)"""
    torch.manual_seed(7)
    model = FCOS([2048, 1024, 512], 20, 64, freeze_bn=False).enable_trunk_batch_stats().to(DEV).train()
    model.backbone.freeze_stages(2)
    trunk = model.backbone.trunk
    assert not trunk.bn1.training and not trunk.layer2.training and trunk.layer3.training and not trunk.conv1.weight.requires_grad
    for part in (trunk.layer1, trunk.layer2):
        for m in part.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.requires_grad_(True)
    names = _step_without_fallbacks(model)
    assert names.count("_BottleneckRowsBackward") == 7 and names.count("_BatchNormResRowsBackward") == 9
    frozen = [b for part in (trunk.layer1, trunk.layer2) for b in part.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(frozen) == 23 and all(int(b.num_batches_tracked) == 0 and b.weight.grad is None for b in frozen) and int(trunk.bn1.num_batches_tracked) == 0


def test_one_step_under_autocast_and_gradscaler(monkeypatch):
    """torch.autocast(float16) + GradScaler: no fallback, finite gradients, and every dense conv launch of the step -- forward, data gradient, weight
    gradient -- runs with f16 operands (FD_PREC_F16), the maps between the nodes of the new path staying fp32."""
    torch.manual_seed(8)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats().to(DEV).train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))
    precs, dprecs, wprecs = [], [], []
    real_launch, real_dgrad, real_wgrad = T._dense_launch, T._dense_dgrad, ops.conv_wgrad

    def launch(x_, segs, w, y, k, stride, pad, dil, prec, *a, **kw):
        precs.append(prec)
        return real_launch(x_, segs, w, y, k, stride, pad, dil, prec, *a, **kw)

    def dgrad(g, x_, w, scale, segs, so, k, stride, pad, dil, prec, *a, **kw):
        dprecs.append(prec)
        return real_dgrad(g, x_, w, scale, segs, so, k, stride, pad, dil, prec, *a, **kw)

    def wgrad(*a, **kw):
        wprecs.append(kw.get("precision"))
        return real_wgrad(*a, **kw)

    monkeypatch.setattr(T, "_dense_launch", launch)
    monkeypatch.setattr(T, "_dense_dgrad", dgrad)
    monkeypatch.setattr(ops, "conv_wgrad", wgrad)
    T.STATS["stock_fallbacks"] = 0
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from test_mbconv_train_gpu import RANGES, STRIDES
    with torch.autocast("cuda", dtype=torch.float16):
        assert T.amp_prec() == _lib.PREC_F16
        out = model(x)
        assert out[0][0].dtype == torch.float32
        loss = FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]
    names = _node_names(out)
    scaler.scale(loss).backward()
    assert T.STATS["stock_fallbacks"] == 0 and names.count("_BatchNormResRowsBackward") == 16
    assert len(precs) >= 52 and set(precs) == {_lib.PREC_F16}, (len(precs), set(precs))          # the trunk's 52 convs behind the stem, and the FPN / head's
    assert len(dprecs) >= 52 and set(dprecs) == {_lib.PREC_F16}, (len(dprecs), set(dprecs))
    assert len(wprecs) >= 52 and set(wprecs) == {_lib.PREC_F16}, (len(wprecs), set(wprecs))
    for n, p in model.named_parameters():
        assert not p.requires_grad or n.startswith("fpn.gn3.") or (p.grad is not None and bool(torch.isfinite(p.grad).all())), n
    scaler.step(opt)
    scaler.update()
    assert np.isfinite(float(loss.detach()))


def test_switch_off_is_todays_graph_bit_for_bit():
    """Two models built the same way that never call the switch -- one of them built after ANOTHER model switched it on, and with the flag written False by
    hand -- give the same loss and gradients bit for bit, build no node of the new path and take today's counted stock BatchNorm fallback."""
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))

    def build(touch):
        torch.manual_seed(3)
        m = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_stem_training()
        if touch:
            m.backbone.hip_bn_train = False
        return m.to(DEV).train()

    T.STRICT = False            # today's default for bn_freeze=False: conv on HIP + stock BatchNorm, a counted fallback (it raises under strict mode)
    try:
        T.STATS["stock_fallbacks"] = 0
        a = build(False)
        l0, g0 = _one_step(a, x, gt, labels)
        n_fallbacks = T.STATS["stock_fallbacks"]
        HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_trunk_batch_stats()
        T.STATS["stock_fallbacks"] = 0
        b = build(True)
        l1, g1 = _one_step(b, x, gt, labels)
        assert T.STATS["stock_fallbacks"] == n_fallbacks >= 52              # the trunk's BatchNorms behind a conv
        names = _node_names(b(x))
    finally:
        T.STRICT = True
    assert not [n for n in names if n in NEW_NODES]
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 50
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    with pytest.raises(_lib.FdError, match="FD_STRICT"):                       # and under strict mode the untouched model still raises, as today
        a(x)
