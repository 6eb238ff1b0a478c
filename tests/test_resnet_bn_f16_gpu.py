"""The ResNet-50 trunk on batch statistics with f16 MAPS under torch.autocast(float16) (enable_trunk_batch_stats(f16_maps=True)): single bottlenecks against
the float64 restatement of tests/resnet_bn_ref.py with the stock modules under the same autocast as the yardstick, then the whole HISFCOS-R50 step -- eager,
replayed from one HIP graph, with the flag on outside autocast, with the flag off under autocast, with frozen stages -- and two ranks under
DistributedDataParallel + SyncBatchNorm.

The block's bar is not fixed in advance.  Two correct f16 pipelines differ by where they round: the same block as plain torch modules under the same autocast
on the same device gives stock's deviation from the float64 restatement per tensor (largest |error| in units of max|reference|), and ours must stay within
TWICE that (the margin of tests/test_optim_gpu.py).  Both figures are printed.

The seeds.  f16 maps carry errors of ~1e-3 of a map's scale, far above the float64 margin of resnet_bn_ref.build_case, and at these sizes (14 000 ReLU inputs)
almost every draw has a pre-activation closer to 0 than that: a ReLU decision that flips moves a gradient by percents of its scale, in stock's run as in ours
(seed 3 of the identity case: both 1e-1 away on the input gradient; seed 53: ours alone; seed 3 of downsample-stride2: stock alone).  Neither pipeline gives
the same bits in every process (stock's convolution algorithms, our autotuned tiles), so no seed can be pinned.  The seeds are walked upward from 0 to the
first one at which float64 is clear (as before), STOCK ITSELF stays clear -- every pre-activation of its autocast run at the three ReLUs has the float64
sign and lies farther than KINK_MARGIN from 0 -- and the three ReLU outputs of OUR run make float64's decisions.  That last condition cannot hide a wrong
decision: one that differs from float64's is tolerated (the walk moves on) only where the float64 pre-activation is within twice stock's own largest error at
that ReLU's input; farther from 0 it fails the test.  The walk and the decisions that differed are printed.
The block input is drawn f16-representable: on this path under AMP a block's input IS an f16 map (the previous block's output), and with an fp32 x the
identity case would round the residual once more in our pipeline than in stock's (which adds the fp32 x) -- an input-format difference, not arithmetic.

Measured on an MI355X: over the three cases and all tensors ours deviates from float64 by at most 9.8e-4 of max|reference| (bn2.weight of
downsample-stride1; stock there 1.7e-3), stock by at most 2.2e-3; seeds taken in two processes: 34 / 34, 112 / 424, 18 / 18."""
import copy
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_bn_ref as BR
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd.model.od import FCOS, HalfInvertedStageFCOS
from test_mbconv_train_gpu import RANGES, STRIDES, _batch, _rows
from test_resnet_bn_train_gpu import _node_names, _trunk_bns
from test_resnet_syncbn_gpu import CHILD_TIME_LIMIT, _spawn_with_time_limit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_RES, H_WIDE, H_SYNC = "_BatchNormResRowsHBackward", "_BatchNormWideRowsHBackward", "_SyncBatchNormApplyHBackward"
FP32_NODES = ("_BatchNormResRowsBackward", "_BatchNormWideRowsBackward", "_BatchNormTrainRowsBackward", "_SyncBatchNormApplyBackward")
AUTOCAST = dict(device_type="cuda", dtype=torch.float16)
MAX_SEED = 4000     # (the identity case has needed up to 424: about 5 ms per seed that float64 lets through)


def _loss(out, gt, labels):
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    return FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]


def _hisfcos(f16_maps, seed=8, switch=True):
    torch.manual_seed(seed)
    m = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_stem_training()
    if switch:
        m.enable_trunk_batch_stats(f16_maps=f16_maps)
    return m


# ================================================================================================ 1. one block on rows
def _stock_forward(m, xs):
    """The block as plain torch modules under autocast: (output, the three ReLU pre-activations)."""
    with torch.autocast(**AUTOCAST):
        z1 = m.bn1(m.conv1(xs))
        z2 = m.bn2(m.conv2(F.relu(z1)))
        idt = xs if m.downsample is None else m.downsample(xs)
        pre = m.bn3(m.conv3(F.relu(z2))) + idt
        return F.relu(pre), (z1, z2, pre)


def _stock_case(name, seed):
    """(block on the CPU, x, gy, float64 pre-activations, the stock copy on the device, its input, output and pre-activations), or None when float64 or
    stock's own autocast run is not clear of the ReLU kinks at this seed."""
    blk, x, gy = BR._make(name, seed)
    x = x.half().float()                              # (an f16 map's values: module docstring)
    with torch.no_grad():
        _, pre64, _ = BR.bottleneck(BR.state(blk, torch.float64), x.double(), BR.CASES[name][2])
    if min(float(p.abs().min()) for p in pre64) <= BR.KINK_MARGIN:
        return None
    m = copy.deepcopy(blk).to(DEV).train()
    xs = x.to(DEV).requires_grad_(True)
    stock, pres = _stock_forward(m, xs)
    pres = [p.detach().double().cpu() for p in pres]
    if not all(bool(((p > 0) == (q > 0)).all()) and float(p.abs().min()) > BR.KINK_MARGIN for p, q in zip(pres, pre64)):
        return None
    return blk, x, gy, pre64, m, xs, stock, pres


def _ours_forward(blk, x):
    """The block on the path under test: (input rows, output, the outputs of its three ReLUs as rows: y1, y2, out)."""
    N, _, H, W = x.shape
    xd = _rows(x).contiguous().to(DEV).requires_grad_(True)
    relus, real = [], T.conv_norm_act_rows

    def spy(m_, bn_, x_, segs_, act_=_lib.ACT_NONE, f16_maps_=False):
        y = real(m_, bn_, x_, segs_, act_, f16_maps_)
        if act_ == _lib.ACT_RELU:
            relus.append(y.detach())
        return y

    T.conv_norm_act_rows = spy
    try:
        with torch.autocast(**AUTOCAST):
            got = T.bottleneck(blk, T.from_rows(xd, N, H, W), batch_stats=True, f16_maps=True)
    finally:
        T.conv_norm_act_rows = real
    assert len(relus) == 2
    return xd, got, relus + [_rows(got.detach())]


@pytest.mark.parametrize("name", list(BR.CASES))
def test_bottleneck_on_f16_maps_against_stock_autocast(name, monkeypatch):
    assert T.STRICT, "the suite runs with FD_STRICT=1"
    grad_types = []
    real = T._bn_node_grad
    monkeypatch.setattr(T, "_bn_node_grad", lambda gy_, y_, st=torch.float32: (grad_types.append((gy_.dtype, st)), real(gy_, y_, st))[1])
    n0 = T.STATS["stock_fallbacks"]
    tried = []
    for seed in range(MAX_SEED):
        case = _stock_case(name, seed)
        if case is None:
            continue
        blk, x, gy, pre64, m, xs, stock, pres = case
        ours = copy.deepcopy(blk).to(DEV)
        xd, got, relus = _ours_forward(ours, x)
        flipped = 0
        for y, q, p in zip(relus, pre64, pres):
            diff = (y.cpu() > 0) != (_rows(q) > 0)
            allow = 2 * float((p - q).abs().max())                  # twice stock's own largest error at this ReLU's input
            assert not bool(diff.any()) or float(_rows(q)[diff].abs().max()) <= allow, (name, seed, float(_rows(q)[diff].abs().max()), allow)
            flipped += int(diff.sum())
        tried.append((seed, flipped))
        if not flipped:
            break
    else:
        raise AssertionError(f"no seed below {MAX_SEED} keeps stock's run and ours of the {name} case clear of the ReLU kinks: {tried}")
    print(f"bottleneck {name}: seeds at which float64 and stock are clear, with the decisions of ours that differ from float64's: {tried}")
    sd64, xr64, ref64, _ = BR.reference(blk, x, gy, torch.float64)
    (stock.float() * gy.to(DEV)).sum().backward()        # stock: the same block as plain torch modules under the same autocast on the same device
    assert got.dtype == torch.float16 and got.shape == ref64.shape and got.is_contiguous(memory_format=torch.channels_last)
    names = _node_names(got)
    n_bn = 4 if ours.downsample is not None else 3
    assert names.count(H_RES) == 1 and names.count(H_WIDE) == n_bn - 1, names
    assert not [n for n in names if n in FP32_NODES or n == "_BottleneckRowsBackward" or "NativeBatchNorm" in n or "ConvolutionBackward" in n], names
    (got.float() * gy.to(DEV)).sum().backward()
    assert T.STATS["stock_fallbacks"] == n0
    assert len(grad_types) == n_bn and all(g == torch.float16 and st == torch.float16 for g, st in grad_types), grad_types

    worst = [0.0, 0.0, ""]

    def within(ours, theirs, ref, what):
        scale = float(ref.abs().max()) + 1e-30
        d_o, d_s = float((ours.double().cpu() - ref).abs().max()) / scale, float((theirs.double().cpu() - ref).abs().max()) / scale
        print(f"bottleneck {name} (seed {seed}): {what}: ours deviates from float64 by {d_o:.3e}, stock autocast by {d_s:.3e} of max|reference|")
        if d_o > worst[0]:
            worst[:] = [d_o, d_s, what]
        return d_o <= 2 * d_s, (what, d_o, d_s)

    checks = [within(_rows(got.detach()), _rows(stock.detach()), _rows(ref64), "output"),
              within(xd.grad, _rows(xs.grad), _rows(xr64.grad), "input gradient")]
    stock_params = dict(m.named_parameters())
    for n, p in ours.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), n
        checks.append(within(p.grad, stock_params[n].grad, sd64[n].grad, n))
    assert len(checks) == 2 + 3 * n_bn
    print(f"bottleneck {name}: largest deviation of ours {worst[0]:.3e} ({worst[2]}; stock there {worst[1]:.3e})")
    bad = [c[1] for c in checks if not c[0]]
    assert not bad, bad
    for mod in ours.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            assert int(mod.num_batches_tracked) == 1 and bool(torch.isfinite(mod.running_mean).all() & torch.isfinite(mod.running_var).all())


def test_momentum_none_keeps_the_fp32_node_inside_an_f16_block():
    """bn2 and bn3 on the cumulative moving average (momentum=None: the `_cma` kernels have no f16 form) keep the fp32 nodes; their neighbours take either
    map type as it comes: no fallback, finite gradients, an fp32 block output."""
    blk, x, gy, _ = BR.build_case("downsample-stride2")
    blk.bn2.momentum = blk.bn3.momentum = None
    blk.to(DEV)
    N, _, H, W = x.shape
    xd = _rows(x).contiguous().to(DEV).requires_grad_(True)
    n0 = T.STATS["stock_fallbacks"]
    with torch.autocast(**AUTOCAST):
        got = T.bottleneck(blk, T.from_rows(xd, N, H, W), batch_stats=True, f16_maps=True)
    names = _node_names(got)
    assert got.dtype == torch.float32 and names.count(H_WIDE) == 2 and names.count(H_RES) == 0, names          # bn1 and the downsample's
    assert names.count("_BatchNormResRowsBackward") == 1 and names.count("_BatchNormTrainRowsBackward") + names.count("_BatchNormWideRowsBackward") == 1, names
    (got * gy.to(DEV)).sum().backward()
    assert T.STATS["stock_fallbacks"] == n0 and bool(torch.isfinite(xd.grad).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in blk.parameters())
    assert int(blk.bn2.num_batches_tracked) == 1 and int(blk.bn3.num_batches_tracked) == 1


# ================================================================================================ 2. the whole model
def _amp_step(model, x, gt, labels, scaler):
    model.zero_grad(set_to_none=True)
    with torch.autocast(**AUTOCAST):
        out = model(x)
        loss = _loss(out, gt, labels)
    scaler.scale(loss).backward()
    return out, loss.detach()


def test_hisfcos_r50_step_under_autocast_and_gradscaler():
    assert T.STRICT
    model = _hisfcos(True).to(DEV).train()
    assert model.backbone.trunk.hip_bn_f16_maps and model.backbone.trunk.hip_bn_train
    bns = _trunk_bns(model)
    before = {n: (b.running_mean.clone(), b.running_var.clone()) for n, b in bns.items()}
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))
    T.STATS["stock_fallbacks"] = 0
    out, loss = _amp_step(model, x, gt, labels, scaler)
    names = _node_names(out)
    assert T.STATS["stock_fallbacks"] == 0
    assert names.count(H_RES) == 16 and names.count(H_WIDE) == 36 and "_BottleneckRowsBackward" not in names          # 16 blocks: 52 BatchNorms behind the stem's
    assert not [n for n in names if n in ("_BatchNormResRowsBackward", "_BatchNormWideRowsBackward") or "NativeBatchNorm" in n or "ConvolutionBackward" in n]
    for n, p in model.named_parameters():
        assert not p.requires_grad or n.startswith("fpn.gn3.") or (p.grad is not None and bool(torch.isfinite(p.grad).all())), n
    assert len(bns) == 53
    for n, b in bns.items():
        assert int(b.num_batches_tracked) == 1, n
        assert bool(torch.isfinite(b.running_mean).all() & torch.isfinite(b.running_var).all()), n
        assert not torch.equal(b.running_mean, before[n][0]) and not torch.equal(b.running_var, before[n][1]), n
    scaler.step(opt)
    scaler.update()
    assert np.isfinite(float(loss))


def test_graph_replay_gives_the_eager_loss_bit_for_bit():
    """The new nodes are capture-safe: the step recorded once by GraphedStep and replayed gives the loss of the same step enqueued eagerly."""
    from pytorch_object_detection_amd.train_graph import GraphedStep
    base = _hisfcos(True).to(DEV).train()
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)
    assert m_graph.backbone.trunk.hip_bn_f16_maps
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))

    def make(model):
        def step(x_, gt_, labels_):
            model.zero_grad(set_to_none=True)
            with torch.autocast(**AUTOCAST):
                loss = _loss(model(x_), gt_, labels_)
            (loss * 1024.0).backward()
            return loss.detach()
        return step

    l_e = make(m_eager)(x, gt, labels).clone()
    graphed = GraphedStep(make(m_graph), [x, gt, labels], warmup=2)
    l_g = graphed(x, gt, labels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(l_e)) and torch.equal(l_e, l_g), (float(l_e), float(l_g))
    ge, gg = dict(m_eager.named_parameters()), dict(m_graph.named_parameters())
    for n in ("backbone.extract_feature.layer3.0.bn3.weight", "backbone.layer1.0.conv1.weight", "backbone.conv1.weight"):
        assert torch.equal(ge[n].grad, gg[n].grad) and float(gg[n].grad.abs().max()) > 0, n


def test_flag_on_without_autocast_is_the_flag_off_graph_bit_for_bit():
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))
    res = []
    for f16_maps in (False, True):
        model = _hisfcos(f16_maps, seed=3).to(DEV).train()
        model.zero_grad(set_to_none=True)
        out = model(x)
        loss = _loss(out, gt, labels)
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, _node_names(out)))
    (l0, g0, n0), (l1, g1, n1) = res
    assert sorted(n0) == sorted(n1) and n1.count("_BatchNormResRowsBackward") == 16 and not [n for n in n1 if n in (H_RES, H_WIDE, H_SYNC)]
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 50
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_flag_off_under_autocast_has_todays_node_names():
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))
    model = _hisfcos(False).to(DEV).train()
    with torch.autocast(**AUTOCAST):
        out = model(x)
    names = _node_names(out)
    assert names.count("_BatchNormResRowsBackward") == 16 and not [n for n in names if n in (H_RES, H_WIDE, H_SYNC)]
    assert out[0][0].dtype == torch.float32


def test_frozen_stages_beside_f16_maps_under_autocast():
    """backbone.freeze_stages(2), the conv weights of layer1-2 trainable again (tests/test_resnet_bn_train_gpu.py's construction): 7 fused frozen blocks, whose
    f16 output the first batch-statistics block takes as it is, and 9 blocks on f16 maps; no fallback, finite gradients."""
    assert T.STRICT
    torch.manual_seed(7)
    model = FCOS([2048, 1024, 512], 20, 64, freeze_bn=False).enable_trunk_batch_stats(f16_maps=True).to(DEV).train()
    model.backbone.freeze_stages(2)
    trunk = model.backbone.trunk
    for part in (trunk.layer1, trunk.layer2):
        for m in part.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.requires_grad_(True)
    x = torch.randn(2, 3, 128, 128, device=DEV)
    T.STATS["stock_fallbacks"] = 0
    model.zero_grad()
    with torch.autocast(**AUTOCAST):
        out = model(x)
    names = _node_names(out)
    torch.manual_seed(9)
    (sum((t.float() * torch.randn(t.shape, device=DEV)).sum() for grp in out for t in grp) * 64.0).backward()
    assert T.STATS["stock_fallbacks"] == 0
    assert names.count("_BottleneckRowsBackward") == 7 and names.count(H_RES) == 9 and "_BatchNormResRowsBackward" not in names
    assert not [n for n in names if "NativeBatchNorm" in n or "ConvolutionBackward" in n]
    for n, p in model.backbone.named_parameters():
        assert not p.requires_grad or (p.grad is not None and bool(torch.isfinite(p.grad).all())), n


# ================================================================================================ 3. two ranks
def _worker(rank, world, init_file, out_dir):
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        model = _hisfcos(True, seed=11).to(dev).train()
        net = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
        model = net.module
        trunk = model.backbone.trunk
        assert trunk.hip_bn_train and trunk.hip_bn_f16_maps and T._is_sync(trunk.layer1[0].bn1)
        x, gt, labels = _batch((128, 128))
        x, gt, labels = x[rank:rank + 1].to(dev), gt[rank:rank + 1].to(dev), labels[rank:rank + 1].to(dev)
        T.STATS["stock_fallbacks"] = 0
        net.zero_grad()
        with torch.autocast(**AUTOCAST):
            out = net(x)
            loss = _loss(out, gt, labels)
        names = _node_names(out)
        (loss * 1024.0).backward()
        torch.cuda.synchronize()
        res = {"loss": float(loss.detach()), "stats": dict(T.STATS), "pending": len(T._PENDING), "strict": T.STRICT, "names": names,
               "finite": all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None),
               "n_grads": sum(p.grad is not None for p in model.parameters()),
               "running": {n: (m.running_mean.cpu(), m.running_var.cpu(), int(m.num_batches_tracked)) for n, m in model.backbone.named_modules()
                           if isinstance(m, torch.nn.SyncBatchNorm)}}
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_f16_maps():
    with tempfile.TemporaryDirectory() as tmp:
        _spawn_with_time_limit(_worker, (2, os.path.join(tmp, "rdzv"), tmp), 2, CHILD_TIME_LIMIT)
        r0, r1 = (torch.load(os.path.join(tmp, f"rank{i}.pt")) for i in range(2))
    for r in (r0, r1):
        assert r["strict"] and r["stats"]["stock_fallbacks"] == 0 and r["pending"] == 0, r["stats"]
        assert r["names"].count(H_SYNC) == 52 and not [n for n in r["names"] if n in (H_RES, H_WIDE, "_BatchNormResRowsBackward")]      # every BatchNorm behind the stem's
        assert r["finite"] and r["n_grads"] > 150 and np.isfinite(r["loss"])
        assert all(v[2] == 1 for v in r["running"].values())
    # one process running both images on the same path (unsynchronised `_h` nodes)
    model = _hisfcos(True, seed=11).to(DEV).train()
    x, gt, labels = (t.to(DEV) for t in _batch((128, 128)))
    with torch.autocast(**AUTOCAST):
        loss = _loss(model(x), gt, labels)
    print("two ranks: losses", r0["loss"], r1["loss"], "one process:", float(loss))
    one = {n: (m.running_mean.cpu(), m.running_var.cpu()) for n, m in model.backbone.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert len(one) == 53 and set(one) <= set(r0["running"])
    worst = 0.0
    for n, (rm, rv) in one.items():
        (m0, v0, _), (m1, v1, _) = r0["running"][n], r1["running"][n]
        assert torch.equal(m0, m1) and torch.equal(v0, v1), n
        worst = max(worst, float((m0 - rm).abs().max()), float((v0 - rv).abs().max()))
        np.testing.assert_allclose(m0.numpy(), rm.numpy(), atol=1e-4, rtol=1e-4, err_msg=n)
        np.testing.assert_allclose(v0.numpy(), rv.numpy(), atol=1e-4, rtol=1e-4, err_msg=n)
    print(f"two ranks vs one process: running statistics differ by at most {worst:.3e}")

