"""Cfg4: one training step on the GPU — autograd forward whose dense convolutions run on the HIP conv kernel (forward,
data gradient, weight gradient; train_ops.py), FCOSGenTargets + FCOSLoss('giou') as HIP kernels, backward, SGD —
against the CPU oracle's autograd."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from pytorch_object_detection_amd.bulider import Builder, load_config
from pytorch_object_detection_amd.model.loss import FCOSLoss
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("wino", [False, True, 4], ids=["direct", "winograd", "winograd-f4x4"])
def test_train_step_matches_oracle_autograd(wino, monkeypatch):
    """wino=False: every dense conv on the direct kernel (bit-for-bit an fp32 fma chain).  wino=True (the default, FD_WINOGRAD=1): the
    3x3 stride-1 layers -- forward and data gradient -- on the Winograd F(2x2, 3x3) kernel (fp32 too, another rounding).  Same bars.
    Measured on MI355X (tools/train_dev_stats.py, this seed): Winograd path -- all 145 gradients within 5e-6 of their maximum; direct
    path -- 128 of 145 at rounding level, 17 (biases upstream of one flipped ReLU mask element) with a median deviation of 1e-4 .. 3e-4."""
    from pytorch_object_detection_amd import ops
    monkeypatch.setattr(ops, "WINO_MODE", "force" if wino else "0")       # (at 128 x 128 the size rule would send every layer to the direct kernel)
    # wino=4: forward and data gradient of every 3x3 stride-1 layer on Winograd F(4x4, 3x3) (the choice of the batch-16 training step for its wide
    # maps, ops.wino4_choice, forced onto these small ones; its flipped / transposed / BN-scaled data-gradient packing comes from PACKS)
    monkeypatch.setattr(ops, "WINO4_MODE", "force" if wino == 4 else "0")
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256)
    gen = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.75)
    x = torch.randn(2, 3, 128, 128)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]])
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]])
    strides = [8, 16, 32, 64, 128]
    ranges = [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]]

    # oracle: CPU autograd through the functional restatement
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in model.state_dict().items()}
    outs = R.hisfcos_forward(sd, x)
    tg = R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], strides, ranges, gt, labels)
    ref = R.fcos_loss(outs, tg, "giou")
    ref[3].backward()

    model.freeze_all_bn = True          # every BatchNorm on its running statistics (the oracle call above does the same)
    model.to(DEV).train()
    assert not any(b.training for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d))   # frozen BN stays frozen
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt.zero_grad()
    out = model(x.to(DEV))
    # the training graph runs its dense convolutions on the HIP kernels (forward + both backward passes)
    seen, stack, hip = set(), [out[0][0].grad_fn], 0
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        hip += type(fn).__name__ in ("_ConvRowsBackward", "_DwRowsBackward", "_GroupNormRowsBackward", "_BottleneckRowsBackward")
        stack.extend(f for f, _ in fn.next_functions)
    assert hip >= 45, hip
    target = FCOSGenTargets(strides, ranges)([out, gt.to(DEV), labels.to(DEV)])
    for a, b in zip(target, tg):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-6)
    losses = FCOSLoss("giou")([out, target])
    np.testing.assert_allclose([float(l.detach()) for l in losses], [float(l.detach()) for l in ref], rtol=2e-4)
    losses[-1].backward()
    checked = 0
    for name in ("head.cls_logits.weight", "head.reg_pred.bias", "head.scale_exp.2.scale", "head.pw1.weight",
                 "fpn.HisBlock3.conv4.weight", "fpn.tf1.weight", "backbone.extract_feature.layer4.2.conv3.weight",
                 "backbone.extract_feature.layer2.0.conv1.weight"):
        p = dict(model.named_parameters())[name]
        g_ref = sd[name].grad
        assert p.grad is not None and g_ref is not None, name
        scale = float(g_ref.abs().max()) + 1e-12
        # measured on MI355X: every gradient agrees with the CPU autograd to ~1e-6 of its max EXCEPT what sits behind one
        # ReLU whose near-zero input lands on the other side of 0 under a different fp32 summation order (one element of
        # head.reg_conv's channel 208 on this seed: 3 % on that filter, ~0.2 % on everything upstream of it); hence a
        # relative-to-max bar that tolerates a flipped mask element, looser deep in the trunk (~60 ReLU masks)
        tol = 2e-2 if name.startswith("backbone.") else 2e-3
        np.testing.assert_allclose(p.grad.cpu().numpy() / scale, g_ref.numpy() / scale, atol=tol, err_msg=name)
        checked += 1
    assert checked == 8
    # robust-to-a-flip view of the same comparison: for the parameters at or after the towers (nothing upstream of the
    # flipped element) the MEDIAN deviation per parameter is at rounding level
    for name, p in model.head.named_parameters():
        g_ref = sd["head." + name].grad
        if p.grad is None or g_ref is None or g_ref.numel() < 64 or not name.startswith(("cls_", "reg_", "cnt_")):
            continue
        scale = float(g_ref.abs().max()) + 1e-12
        assert float((p.grad.cpu() - g_ref).abs().median()) / scale < 1e-5, name
    # EVERY trainable parameter (not a sample of eight): a gradient exists on both sides, points the same way, agrees to
    # rounding in the bulk (median) and to a flipped-ReLU-mask's worth at worst (see the comment above and
    # test_relu_mask_flips_are_the_only_source_of_large_gradient_deviations)
    n_par, bulk_ok = 0, 0
    for name, p in model.named_parameters():
        g_ref = sd[name].grad
        if not p.requires_grad:
            assert p.grad is None, name
            continue
        assert p.grad is not None and g_ref is not None, name
        a, b = p.grad.cpu().double().flatten(), g_ref.double().flatten()
        scale = float(b.abs().max()) + 1e-30
        if scale < 1e-12:                               # (a conv bias whose only consumer is zero: nothing to compare)
            assert float(a.abs().max()) < 1e-9, name
            continue
        cos = float((a @ b) / (a.norm() * b.norm() + 1e-30))
        d = (a - b).abs() / scale
        assert cos > 0.9995, (name, cos)
        # which near-zero pre-activation lands on the other side of 0 depends on the summation order (block tile, split-K, Winograd):
        # a parameter upstream of a flipped mask element deviates by that element's share everywhere (median up to ~1e-3 of the
        # maximum), all others agree to rounding -- so: a flip's worth for each, rounding level for the bulk of them
        assert float(d.median()) < 1e-3, (name, float(d.median()))
        assert float(d.max()) < 5e-2, (name, float(d.max()))          # (3.4 % measured on the filter that owns a flipped element)
        bulk_ok += float(d.median()) < 5e-5
        n_par += 1
    assert n_par > 120, n_par
    assert bulk_ok >= 0.85 * n_par, (bulk_ok, n_par)
    # layer1 and the stem are frozen (freeze_stages(1), HISFcos.py:67)
    assert model.backbone.extract_feature.layer1[0].conv1.weight.grad is None
    before = model.head.cls_logits.weight.detach().clone()
    opt.step()
    assert not torch.equal(before, model.head.cls_logits.weight.detach())
    # back to inference: the HIP plan picks up the updated weights
    model.eval()
    cls_hip = model(x.to(DEV))[0][0]
    assert torch.isfinite(cls_hip).all()


def test_fcos_baseline_train_step_runs():
    from pytorch_object_detection_amd.model.od import FCOS
    torch.manual_seed(3)
    from pytorch_object_detection_amd import train_ops
    model = FCOS([2048, 1024, 512], 20, 256).to(DEV).train()
    # the FCOS baseline trains its 7x7 stem (the reference freezes no stage of it, Fcos.py:24-36): Cin = 3 has no HIP backward, the stem is
    # the ONE documented stock-op layer of this model -- so this test runs with FD_STRICT off and counts the fallbacks
    train_ops.STRICT, n0 = False, train_ops.STATS["stock_fallbacks"]
    try:
        out = model(torch.randn(1, 3, 128, 128, device=DEV))
        gt = torch.tensor([[[10., 12., 60., 70.]]], device=DEV)
        labels = torch.tensor([[3]], device=DEV)
        ranges = [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 9999999]]
        target = FCOSGenTargets([8, 16, 32, 64, 128], ranges)([out, gt, labels])
        loss = FCOSLoss("iou")([out, target])[-1]
        loss.backward()
    finally:
        train_ops.STRICT = True
    assert train_ops.STATS["stock_fallbacks"] == n0 + 1          # the stem, nothing else
    g = model.head.cls_branch[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_builder_train_objects():
    cfg = load_config()
    cfg["model"]["name"] = "HISFCOS"
    b = Builder(cfg)
    model = b.model_build().to(DEV)
    opt = b.opt_build(model)
    model.train()
    out = model(torch.randn(2, 3, 256, 256, device=DEV))      # (batch-statistic FPN BatchNorm needs > 1 value per channel at P7)
    assert len(out) == 3 and len(out[0]) == 5 and out[0][0].requires_grad
    assert isinstance(opt, torch.optim.SGD)


@pytest.mark.parametrize("which", ["FCOS", "HISFCOS"])
def test_pyramid_head_matches_per_level_head(which):
    """The rows-space training head (one launch per layer over all five levels, HIP GroupNorm backward) against the
    per-level forward that uses torch's GroupNorm / depthwise ops: same outputs, same parameter and input gradients."""
    from pytorch_object_detection_amd.model.od.Fcos import HeadFCOS
    from pytorch_object_detection_amd.model.od.HISFcos import HISFCOSHead
    torch.manual_seed(11)
    head = (HeadFCOS(64, 20) if which == "FCOS" else HISFCOSHead(64, 20)).to(DEV).train()
    for p in head.parameters():                         # the reference's N(0, 0.01) init makes gradients vanish: rescale
        if p.dim() == 4:
            torch.nn.init.normal_(p, std=(2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
    feats = [torch.randn(2, 64, s, s + 1, device=DEV).to(memory_format=torch.channels_last) for s in (12, 6, 3, 2, 1)]
    res = []
    from pytorch_object_detection_amd import train_ops
    for fn in (head.train_forward, head._train_forward_stock):
        head.zero_grad()
        xs = [f.clone().requires_grad_(True) for f in feats]
        train_ops._STOCK = fn.__name__ == "_train_forward_stock"     # the explicit stock-op mode (exempt from FD_STRICT)
        try:
            out = fn(xs)
        finally:
            train_ops._STOCK = False
        torch.manual_seed(5)
        loss = sum((t * torch.randn(t.shape, device=DEV)).sum() for lst in out for t in lst)
        loss.backward()
        res.append(([t.detach().clone() for lst in out for t in lst], [x.grad.clone() for x in xs],
                    {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}))
    (o1, g1, p1), (o2, g2, p2) = res
    for a, b in zip(o1, o2):
        assert a.shape == b.shape
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=2e-4, rtol=2e-4)
    for a, b in zip(g1, g2):
        s = float(b.abs().max())
        np.testing.assert_allclose(a.cpu().numpy() / s, b.cpu().numpy() / s, atol=3e-4)
    assert p1.keys() == p2.keys() and len(p1) > 8
    for n in p1:
        s = float(p2[n].abs().max()) + 1e-12
        np.testing.assert_allclose(p1[n].cpu().numpy() / s, p2[n].cpu().numpy() / s, atol=3e-4, err_msg=n)


def test_amp_and_ddp_train_step():
    """The reference's loop shape (train.py:101-103,175-181): DistributedDataParallel(find_unused_parameters=True) around
    the model, torch.autocast + GradScaler around the step.  World size 1 on RCCL: the DDP reducer hooks and the AMP
    decorators of the HIP autograd nodes are exercised; the nodes keep computing in fp32."""
    import os
    import torch.distributed as dist
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV)
        ddp = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)
        ddp.train()
        opt = torch.optim.SGD([p for p in ddp.parameters() if p.requires_grad], lr=1e-3, momentum=0.9)
        scaler = torch.amp.GradScaler("cuda", enabled=True)
        x = torch.randn(2, 3, 128, 128, device=DEV)
        gt = torch.tensor([[[10., 12., 60., 70.]], [[30., 20., 110., 100.]]], device=DEV)
        labels = torch.tensor([[3], [7]], device=DEV)
        gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 999999]])
        crit = FCOSLoss("giou")
        vals = []
        import warnings
        for amp in (False, True):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                out = ddp(x)
                assert out[0][0].dtype == torch.float32          # HIP nodes stay fp32 under autocast
                losses = crit([out, gen([out, gt, labels])])
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                scaler.scale(losses[-1].mean()).backward()
            # DDP's bucket views want every gradient in its parameter's own strides (the gradient layout contract): a
            # mismatch costs a copy per bucket and the overlap with backward
            off = [(n, tuple(p.grad.shape), p.grad.stride(), p.stride()) for n, p in model.named_parameters()
                   if p.grad is not None and p.grad.stride() != p.stride()]
            assert not off and not [w for w in caught if "strides" in str(w.message)], (off, [str(w.message)[:300] for w in caught])
            g = model.head.cls_conv[0].weight.grad
            assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
            vals.append(float(losses[-1].detach()))
            scaler.step(opt)
            scaler.update()
        assert all(np.isfinite(v) for v in vals)
    finally:
        dist.destroy_process_group()


def test_unfrozen_batchnorm_trains_with_hip_convs():
    """bn_freeze=False (BatchNorm in training mode, batch statistics): the convs stay on the HIP kernels, BatchNorm runs as
    the stock op after them.  Gradients through ~60 batch-statistic BatchNorms are ill-conditioned (a 1e-6 relative change of
    the input moves them by ~1 % of their max on the all-stock graph), so the HIP graph is held to that same noise floor:
    its deviation from the all-stock graph must not exceed what the all-stock graph shows against itself under a 1e-6
    perturbation of the input."""
    from pytorch_object_detection_amd import train_ops
    torch.manual_seed(4)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).to(DEV).train()
    assert any(b.training for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d))
    x = torch.randn(4, 3, 384, 384, device=DEV)

    def run(stock, xx):
        train_ops._STOCK = stock
        try:
            model.zero_grad()
            sd = {k: v.clone() for k, v in model.state_dict().items()}      # running stats move: restore afterwards
            out = model(xx)
            torch.manual_seed(9)
            sum((t * torch.randn(t.shape, device=DEV)).sum() for grp in out for t in grp).backward()
            res = ([t.detach().clone() for grp in out for t in grp],
                   {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
            model.load_state_dict(sd)
            return res
        finally:
            train_ops._STOCK = False

    # bn_freeze=False trains the 7x7 stem and puts the TRUNK's BatchNorms on batch statistics too: both are documented stock-op layers
    # (train_ops module docstring), so this test runs with FD_STRICT off
    train_ops.STRICT = False
    try:
        (o1, g1), (o2, g2), (_, g3) = run(False, x), run(True, x), run(True, x * (1 + 1e-6))
    finally:
        train_ops.STRICT = True
    for i, (a, b) in enumerate(zip(o1, o2)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), atol=5e-3, rtol=5e-3)
    assert g1.keys() == g2.keys() and "backbone.conv1.weight" in g1     # the stem trains too

    def med(a, b):
        return float(((a - b).abs() / (float(b.abs().max()) + 1e-12)).median())

    for n in ("head.cls_logits.weight", "head.pw1.weight", "fpn.tf1.weight", "backbone.extract_feature.layer3.0.conv2.weight",
              "backbone.conv1.weight"):
        assert med(g1[n], g2[n]) <= 3 * med(g3[n], g2[n]) + 1e-4, (n, med(g1[n], g2[n]), med(g3[n], g2[n]))


def test_packed_weight_cache_follows_every_kind_of_update():
    """train_ops.PACKS keeps packed conv weights across steps: after optimizer.step(), after an update through `.data`
    (no version bump) and after load_state_dict the training forward must see the new weights."""
    from pytorch_object_detection_amd import train_ops
    torch.manual_seed(21)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV)
    model.freeze_all_bn = True          # (a 1x128x128 input leaves one value per channel at P7: no batch statistics)
    model.train()
    x = torch.randn(1, 3, 128, 128, device=DEV)

    def fwd():
        return [t.detach().clone() for grp in model(x) for t in grp]

    def stock():
        train_ops._STOCK = True
        try:
            return [t.detach().clone() for grp in model(x) for t in grp]
        finally:
            train_ops._STOCK = False

    def same(a, b):
        for u, v in zip(a, b):
            np.testing.assert_allclose(u.cpu().numpy(), v.cpu().numpy(), atol=2e-4, rtol=2e-4)

    same(fwd(), stock())
    assert len(train_ops.PACKS.entries) > 40
    w = model.backbone.extract_feature.layer3[1].conv2.weight
    with torch.no_grad():
        w.mul_(1.5)                                   # version bump, like an optimizer step
    same(fwd(), stock())
    w.data.mul_(0.5)                                  # no version bump
    same(fwd(), stock())
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["fpn.tf1.weight"] = sd["fpn.tf1.weight"] * 0.25
    model.load_state_dict(sd)
    same(fwd(), stock())


def test_default_train_mode_fpn_batchnorm_follows_the_reference():
    """only the BACKBONE's BatchNorms stay frozen in train(); the randomly initialised FPN BatchNorms run on batch
    statistics and update their running statistics, as the reference's model.train() makes them (train.py:151).  Losses and
    the updated running statistics against the oracle run with the same layers in training mode."""
    torch.manual_seed(2)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256)
    x = torch.randn(4, 3, 256, 256)
    gt = torch.tensor([[[10., 12., 60., 70.]], [[30., 30., 220., 210.]], [[5., 5., 125., 130.]], [[64., 20., 200., 190.]]])
    labels = torch.tensor([[3], [7], [1], [12]])
    strides, ranges = [8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    R.BN_TRAIN_PREFIXES = ("fpn.",)
    try:
        with torch.no_grad():
            outs = R.hisfcos_forward(sd, x)
    finally:
        R.BN_TRAIN_PREFIXES = ()
    ref = R.fcos_loss(outs, R.gen_targets([tuple(o.shape[2:]) for o in outs[0]], strides, ranges, gt, labels), "giou")
    model.to(DEV).train()
    bns = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert all(m.training == n.startswith("fpn.") for n, m in bns.items())
    assert not any(p.requires_grad for m in bns.values() for p in m.parameters())          # affine stays frozen (HISFcos.py:57-68)
    out = model(x.to(DEV))
    losses = FCOSLoss("giou")([out, FCOSGenTargets(strides, ranges)([out, gt.to(DEV), labels.to(DEV)])])
    np.testing.assert_allclose([float(v.detach()) for v in losses], [float(v) for v in ref], rtol=5e-4)
    losses[-1].backward()
    for n in ("fpn.HisBlock3.bn4", "fpn.gn1", "fpn.gn2", "fpn.HisBlock7.bn1"):
        m = bns[n]
        assert float(m.running_mean.abs().max()) > 0                                        # moved away from the init (0, 1)
        np.testing.assert_allclose(m.running_mean.cpu().numpy(), sd[n + ".running_mean"].numpy(), atol=2e-5, rtol=2e-4)
        np.testing.assert_allclose(m.running_var.cpu().numpy(), sd[n + ".running_var"].numpy(), atol=2e-5, rtol=2e-4)
    assert float(bns["fpn.gn3"].running_mean.abs().max()) == 0                              # gn3 is dead in the reference too
    assert float(bns["backbone.extract_feature.layer2.0.bn1"].running_mean.abs().max()) == 0
    g = model.fpn.HisBlock3.conv4.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    model.freeze_all_bn = True
    assert not any(m.training for m in model.train().modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_relu_mask_flips_are_the_only_source_of_large_gradient_deviations():
    """The claim behind the loose end-to-end bars above, as a test: through a fused conv + frozen BN + ReLU node the HIP
    gradients match torch's to 1e-4 of their maximum EVERYWHERE once the upstream gradient is zeroed at the elements whose
    pre-activation is within 1e-5 of zero (the only elements whose ReLU mask can differ between two fp32 summation orders);
    with those elements kept, a flipped mask element shows up as an O(1) relative deviation in its k x k neighbourhood."""
    import torch.nn.functional as F
    from pytorch_object_detection_amd import train_ops as T
    from pytorch_object_detection_amd._lib import ACT_RELU
    torch.manual_seed(8)
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False)
    bn = torch.nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(64) * 0.1); bn.running_var.copy_(torch.rand(64) + 0.5)
        bn.weight.copy_(torch.rand(64) + 0.5); bn.bias.copy_(torch.randn(64) * 0.05)
    for p in bn.parameters():
        p.requires_grad = False
    x = torch.randn(4, 64, 40, 40)
    z64 = bn.double()(conv.double()(x.double())).detach()                    # fp64 pre-activation
    conv.float(); bn.float()
    safe = (z64.abs() >= 1e-5).float()
    assert float(safe.mean()) < 1.0                                            # the guard really removes something
    gy = torch.randn(4, 64, 40, 40) * safe
    xr = x.clone().requires_grad_(True)
    F.relu(bn(conv(xr))).backward(gy)
    gw_ref, gx_ref = conv.weight.grad.clone(), xr.grad.clone()
    conv.zero_grad()
    conv.to(DEV); bn.to(DEV)
    xd = x.to(DEV).to(memory_format=torch.channels_last).requires_grad_(True)
    out = T.conv_bn_act(conv, bn, xd, ACT_RELU)
    out.backward(gy.to(DEV))
    for got, ref in ((conv.weight.grad.cpu(), gw_ref), (xd.grad.cpu(), gx_ref)):
        s = float(ref.abs().max())
        np.testing.assert_allclose(got.numpy() / s, ref.numpy() / s, atol=1e-4)


def test_full_size_batch_gradient_is_the_mean_of_the_per_image_gradients():
    """Cfg4 at the reference's full shape (16 x 512 x 512, voc.yaml:7,38) through a size-independent property: FCOSLoss is a
    mean over images and, with every BatchNorm on its running statistics, images do not interact -- so the gradient of the
    16-image step equals the mean of the sixteen single-image gradients (other block tiles, other split-K, other pixel-range
    splits of the weight-gradient kernels: a real cross-check of the batched kernels, not a tautology)."""
    torch.manual_seed(12)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV)
    model.freeze_all_bn = True
    model.train()
    B, S = 16, 512
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, 3, S, S, generator=g).to(DEV)
    c = torch.rand(B, 6, 2, generator=g) * (S - 112) + 50
    sz = torch.rand(B, 6, 2, generator=g) * 150 + 20
    gt = torch.cat([c - sz / 2, c + sz / 2], -1).clamp(0, S - 1).to(DEV)
    labels = torch.randint(1, 21, (B, 6), generator=g).to(DEV)
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")
    names = [n for n, p in model.named_parameters() if p.requires_grad]

    def grads(sl):
        model.zero_grad(set_to_none=True)
        out = model(x[sl])
        crit([out, gen([out, gt[sl], labels[sl]])])[-1].mean().backward()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    full = grads(slice(0, B))
    acc = None
    for i in range(B):
        gi = grads(slice(i, i + 1))
        acc = gi if acc is None else {n: acc[n] + gi[n] for n in acc}
    assert set(full) == set(acc) == set(names)
    worst, bulk_ok = 0.0, 0
    for n in names:
        a, b = full[n].double().flatten(), (acc[n] / B).double().flatten()
        scale = float(b.abs().max()) + 1e-30
        d = (a - b).abs() / scale
        # fp32 sums over 16 x 5 456 locations in two different orders, and the 1-image plans run their small maps on the direct kernel where
        # the 16-image plan uses Winograd (ops.wino_preferred): rounding level for the bulk, a flipped ReLU-mask element's share at worst
        assert float(d.median()) < 1e-3, (n, float(d.median()))
        bulk_ok += float(d.median()) < 1e-4
        assert float(d.max()) < 5e-2, (n, float(d.max()))       # (a ReLU-mask element may flip between the 1- and 16-image plans)
        worst = max(worst, float(d.max()))
    assert len(names) > 120
    assert bulk_ok >= 0.85 * len(names), (bulk_ok, len(names))


def _graph_node_names(outputs):
    seen, stack = set(), [t.grad_fn for t in outputs if t.grad_fn is not None]
    names = []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


STOCK_NODES = ("ConvolutionBackward", "MiopenConvolution", "CudnnConvolution", "NativeBatchNormBackward", "MiopenBatchNormBackward",
               "CudnnBatchNormBackward", "NativeGroupNormBackward", "NativeLayerNormBackward", "ThresholdBackward", "ReluBackward",
               "SiluBackward", "MaxPool2DWithIndicesBackward", "UpsampleNearest2DBackward")


def test_default_cfg4_step_runs_no_stock_conv_or_norm():
    """the default training step (backbone BN frozen, FPN BatchNorms on batch statistics, the reference's mode) must not
    fall back to stock PyTorch-ROCm convolution / normalisation ops anywhere.  Three views of the same step: the fallback counter of
    train_ops (FD_STRICT=1 -- this suite's default -- would also have raised), the autograd graph's node types, and the device kernels a
    profiled forward + backward launches."""
    from pytorch_object_detection_amd import train_ops as T
    assert T.STRICT, "tests run with FD_STRICT=1 (tests/conftest.py)"
    torch.manual_seed(2)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV).train()
    x = torch.randn(2, 3, 256, 256, device=DEV)
    gt = torch.tensor([[[10., 12., 160., 170.], [30., 30., 220., 110.]], [[5., 5., 125., 130.], [64., 20., 200., 190.]]], device=DEV)
    labels = torch.tensor([[3, 7], [1, 20]], device=DEV)
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")

    def step():
        model.zero_grad(set_to_none=True)
        out = model(x)
        loss = crit([out, gen([out, gt, labels])])[-1]
        loss.backward()
        return out

    T.STATS["stock_fallbacks"] = 0
    out = step()
    torch.cuda.synchronize()
    assert T.STATS["stock_fallbacks"] == 0
    names = _graph_node_names([t for grp in out for t in grp])
    bad = sorted({n for n in names if n.startswith(STOCK_NODES)})
    assert not bad, bad
    hip = [n for n in names if n.startswith(("_ConvRows", "_BottleneckRows", "_GroupNormRows", "_BatchNormTrainRows", "_DwRows", "_SERows", "_ActRows",
                                             "_PoolAddRows", "_UpAddRows"))]
    assert len(hip) >= 100, len(hip)
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            step()
            torch.cuda.synchronize()
        kernels = {e.key for e in prof.key_averages()
                   if (getattr(e, "device_time_total", 0) > 0 or getattr(e, "cuda_time_total", 0) > 0)
                   and not e.key.startswith(("_", "autograd::", "aten::", "Optimizer", "torch"))}       # device kernels, not the CPU-side op ranges
    except Exception as e:      # the profiler is an extra view; the two checks above are the gate
        pytest.skip(f"torch.profiler unavailable here: {e}")
    if not any("conv_igemm_kernel" in k or "conv3x3_wino_kernel" in k for k in kernels):
        pytest.skip("the profiler reported no device kernels")
    banned = ("miopen", "MIOpen", "batch_norm", "group_norm", "Cijk_", "naive_conv", "gridwise_", "Im2Col", "im2col", "threshold")
    bad_k = sorted(k for k in kernels if any(b in k for b in banned))
    assert not bad_k, bad_k


def test_strict_mode_raises_instead_of_falling_back():
    """FD_STRICT=1: a layer the HIP kernels do not cover raises FdError; FD_STRICT=0 (the library default) takes the documented stock
    path.  Case: a TRAINABLE 7x7 stem (Cin = 3 has no HIP backward)."""
    from pytorch_object_detection_amd import train_ops as T
    from pytorch_object_detection_amd._lib import FdError
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV).train()
    model.backbone.conv1.weight.requires_grad_(True)
    x = torch.randn(1, 3, 128, 128, device=DEV)
    with pytest.raises(FdError, match="FD_STRICT"):
        model(x)
    T.STRICT = False
    try:
        n0 = T.STATS["stock_fallbacks"]
        model.freeze_all_bn = True
        model.train()
        out = model(x)
        assert out[0][0].requires_grad and T.STATS["stock_fallbacks"] == n0 + 1
    finally:
        T.STRICT = True


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_whole_step_as_one_hip_graph_trains_like_the_eager_loop(amp):
    """train_graph.GraphedStep: forward + loss + backward + fused SGD (+ GradScaler) recorded once and replayed.  Every node of the HIP training path must be
    capture-safe (no host synchronisation, no data-dependent shapes); the replayed steps must leave the same weights as the same steps enqueued eagerly -- the
    kernels and their order are the same, so the bar is tight (fp32: 1e-6 of the weight scale; AMP: the f16 rounding is the same too)."""
    import copy
    from pytorch_object_detection_amd.train_graph import GraphedStep
    torch.manual_seed(0)
    base = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV).train()
    x = torch.randn(2, 3, 128, 128, device=DEV)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]], device=DEV)
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]], device=DEV)
    gen_t = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
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

    N = 3                                           # GraphedStep's warm-up steps (eager, they train too)
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)
    s_eager = make(m_eager)
    losses_e = [float(s_eager(x, gt, labels)) for _ in range(N + 1 + 3)]            # warm-up + the captured step's own run + three replays
    graphed = GraphedStep(make(m_graph), [x, gt, labels], warmup=N)                 # N eager steps, then ONE step while capturing (recorded, not executed)
    losses_g = [float(graphed(x, gt, labels).clone()) for _ in range(4)]
    # a capture records the step without running it: the graph model has made N + 4 steps as well
    assert all(np.isfinite(v) for v in losses_e + losses_g)
    np.testing.assert_allclose(losses_g, losses_e[N:], rtol=2e-3 if amp else 1e-5)
    for (n, a), (_, b) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        scale = float(a.detach().abs().max()) + 1e-12
        assert float((a.detach() - b.detach()).abs().max()) <= (2e-3 if amp else 1e-5) * scale, n
    with pytest.raises(ValueError):
        graphed(x[:1], gt, labels)
