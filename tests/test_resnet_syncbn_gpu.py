"""The ResNet-50 trunk on batch statistics across ranks: HISFCOS-R50 (feature 64) with the stem and the trunk switch on, wrapped in DistributedDataParallel
and converted with SyncBatchNorm.convert_sync_batchnorm (train.py:101-103), one 256 x 256 image per rank -- two processes on cuda:0 over gloo, as
tests/test_effnet_syncbn_gpu.py spawns them, each child under a time limit -- against ONE process running both images.

One process running both images is the reference, in two forms:
    all-stock graph (train_ops._STOCK: stock convolutions and nn.BatchNorm2d, nothing of the path under test in it)
        loss                    rtol 2e-4 (the mean of the ranks' losses: every loss term is a per-image mean)
        running statistics      atol = rtol = 1e-4, every trunk BatchNorm, the stem's bn1 among them; equal on both ranks
    the same switched model on the HIP path
        DDP-averaged gradients  the noise-floor protocol of tests/test_train_gpu.py::test_unfrozen_batchnorm_trains_with_hip_convs: per named gradient the
                                median deviation at most 3 x the all-stock graph's own under a 1e-6 perturbation of the input, + 1e-4
Why the gradients are held against the HIP one-process run: what this test adds is the cross-rank path -- synchronised statistics, deferred collectives,
DDP's averaging -- and that must reproduce the one-process computation; the HIP arithmetic against stock ops is
test_resnet_bn_train_gpu.py::test_hisfcos_r50_trains_on_batch_statistics_under_strict_mode's subject, at the size the protocol's numbers were set for.  At this
size (feature 64, 2 x 256^2) the all-stock graph's own noise figure is not stable enough to serve as a bar for a different arithmetic: on head.pw1.weight it
came out 8.7e-5 in one run and 8.0e-4 in the next (the stock ops are not deterministic), with the one-process HIP graph 2.1e-3 ... 2.3e-3 away from the
all-stock one in both.  Measured on an MI355X: two ranks against the one-process HIP run, median deviation 0 ... 1.9e-8 and maximum <= 4.5e-7 of the tensor's
maximum on the seven names; against the all-stock run they deviate exactly as the one-process HIP run does (2.3e-8 ... 1.3e-2).
and no stock fallback on either rank."""
import os
import tempfile
import time

import numpy as np
import pytest
import torch

from test_mbconv_train_gpu import RANGES, STRIDES, _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW = (256, 256)
CHILD_TIME_LIMIT = 240.0      # seconds per child: far above the few seconds a step takes, and a hung collective ends the test instead of the session
NAMES = ("head.cls_logits.weight", "head.pw1.weight", "fpn.tf1.weight", "backbone.extract_feature.layer3.0.conv2.weight", "backbone.conv1.weight",
         "backbone.extract_feature.layer3.0.bn3.weight", "backbone.extract_feature.layer3.0.downsample.1.weight")


def _model():
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(11)
    return HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats()


def _loss(out, gt, labels):
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    return FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]


def _worker(rank, world, init_file, out_dir):
    import torch.distributed as dist
    from pytorch_object_detection_amd import train_ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        model = _model().to(dev).train()
        net = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)      # as train.py:101
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)                                   # as train.py:103
        model = net.module
        assert not any(type(m) is torch.nn.BatchNorm2d for m in model.modules())
        trunk = model.backbone.trunk
        assert trunk.hip_bn_train and isinstance(trunk.bn1, torch.nn.SyncBatchNorm) and train_ops._is_sync(trunk.bn1)
        x, gt, labels = _batch(HW)
        x, gt, labels = x[rank:rank + 1].to(dev), gt[rank:rank + 1].to(dev), labels[rank:rank + 1].to(dev)
        assert train_ops.stem_rows_ok(trunk, x)
        train_ops.SYNC_TRACE.clear()
        train_ops.STATS["stock_fallbacks"] = 0
        net.zero_grad()
        out = net(x)
        loss = _loss(out, gt, labels)
        loss.backward()
        torch.cuda.synchronize()
        res = {"loss": float(loss.detach()), "stats": dict(train_ops.STATS), "pending": len(train_ops._PENDING), "strict": train_ops.STRICT,
               "trace": [k for k, _ in train_ops.SYNC_TRACE],
               "grads": {n: p.grad.cpu() for n, p in model.named_parameters() if p.grad is not None},
               "running": {n: (m.running_mean.cpu(), m.running_var.cpu(), int(m.num_batches_tracked)) for n, m in model.backbone.named_modules()
                           if isinstance(m, torch.nn.SyncBatchNorm)}}
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn_with_time_limit(fn, args, nprocs, limit):
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > deadline:
                raise AssertionError(f"a rank did not finish within {limit:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
                p.join()


def _single_process():
    """Both images in one process: (loss, gradients, running statistics) of the all-stock graph, its gradients under a 1e-6 perturbation of the input, and
    the gradients of the HIP path."""
    from pytorch_object_detection_amd import train_ops
    model = _model().to(DEV).train()
    x, gt, labels = (t.to(DEV) for t in _batch(HW))

    def run(xx, stock):
        train_ops._STOCK = stock
        try:
            model.zero_grad()
            sd = {k: v.clone() for k, v in model.state_dict().items()}
            loss = _loss(model(xx), gt, labels)
            loss.backward()
            res = (float(loss.detach()), {n: p.grad.clone().cpu() for n, p in model.named_parameters() if p.grad is not None},
                   {n: (m.running_mean.cpu().clone(), m.running_var.cpu().clone()) for n, m in model.backbone.named_modules()
                    if isinstance(m, torch.nn.BatchNorm2d)})
            model.load_state_dict(sd)
            return res
        finally:
            train_ops._STOCK = False

    return run(x, True), run(x * (1 + 1e-6), True), run(x, False)


def test_two_rank_hisfcos_r50_step_on_batch_statistics():
    with tempfile.TemporaryDirectory() as tmp:
        _spawn_with_time_limit(_worker, (2, os.path.join(tmp, "rdzv"), tmp), 2, CHILD_TIME_LIMIT)
        r0, r1 = (torch.load(os.path.join(tmp, f"rank{i}.pt")) for i in range(2))
    for r in (r0, r1):
        assert r["strict"] and r["stats"]["stock_fallbacks"] == 0 and r["pending"] == 0, r["stats"]
        assert all(v[2] == 1 for v in r["running"].values())
        assert r["trace"].count("fwd") == r["trace"].count("bwd") >= 53          # one collective per SyncBatchNorm and direction (the FPN's too)
    (loss, g2, running), (_, g3, _), (loss_hip, g1, _) = _single_process()
    print("two ranks: losses", r0["loss"], r1["loss"], "one process: all-stock", loss, "HIP", loss_hip)
    np.testing.assert_allclose((r0["loss"] + r1["loss"]) / 2, loss, rtol=2e-4)
    # (convert_sync_batchnorm gives the stem's bn1, registered as backbone.bn1 and backbone.extract_feature.bn1, two modules over the same tensors)
    assert len(running) == 53 and set(running) <= set(r0["running"]) and set(r0["running"]) - set(running) == {"extract_feature.bn1"}
    for n, (rm, rv) in running.items():
        (m0, v0, _), (m1, v1, _) = r0["running"][n], r1["running"][n]
        assert torch.equal(m0, m1) and torch.equal(v0, v1), n
        np.testing.assert_allclose(m0.numpy(), rm.numpy(), atol=1e-4, rtol=1e-4, err_msg=n)
        np.testing.assert_allclose(v0.numpy(), rv.numpy(), atol=1e-4, rtol=1e-4, err_msg=n)
    assert set(r0["grads"]) == set(g1) == set(g2), set(r0["grads"]) ^ set(g1)
    for n, g in r0["grads"].items():
        assert torch.equal(g, r1["grads"][n]) and bool(torch.isfinite(g).all()), n     # DDP left both ranks the same averaged gradient

    def med(a, b):
        return float(((a - b).abs() / (float(b.abs().max()) + 1e-12)).median())

    for n in NAMES:
        print(f"{n}: median deviation of the two ranks from the one-process HIP graph {med(r0['grads'][n], g1[n]):.3e} (from the all-stock graph "
              f"{med(r0['grads'][n], g2[n]):.3e}; the one-process HIP graph from it {med(g1[n], g2[n]):.3e}), the all-stock graph's own under 1e-6 {med(g3[n], g2[n]):.3e}")
        assert med(r0["grads"][n], g1[n]) <= 3 * med(g3[n], g2[n]) + 1e-4, (n, med(r0["grads"][n], g1[n]), med(g3[n], g2[n]))
