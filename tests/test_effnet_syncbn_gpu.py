"""SyncBatchNorm at the EfficientNet trunk's widths, end to end: two processes on cuda:0 over gloo, spawned as in tests/test_ddp_gpu.py.

a. the node on uneven shards: nn.SyncBatchNorm(144) + SiLU on rows held at width 160, 512 rows on rank 0 and 768 on rank 1, against a float64 BatchNorm1d
   over the 1280 rows (the tolerances of test_ddp_gpu.test_two_rank_syncbatchnorm_with_different_row_counts_per_rank: the same arithmetic);
a2. the callers' dispatch: conv_norm_act_rows and conv_norm_begin / conv_norm_finish on a 1x1 conv 32 -> 96 + SyncBatchNorm(96) + SiLU, uneven shards: the
   deferred form bit for bit the one-shot form, both against the float64 graph within 4 x the float32 CPU graph's own error + 1e-6 of the maximum;
b. the whole FCOS-B0 step with train_stem, batch_stats and drop-connect on, wrapped in DistributedDataParallel and converted with
   SyncBatchNorm.convert_sync_batchnorm, one image per rank, against the float32 restatement of the two-image step (test_effnet_fulltrain_gpu._ref_step)
   under the bars of that file's _run_step: no new numbers."""
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch

import test_effnet_fulltrain_gpu as FT
from test_mbconv_train_gpu import CONFIGS, RANGES, STRIDES, _batch

pytestmark = pytest.mark.gpu
C, CW = 144, 160


# ================================================================================================ a. the node, uneven shards
def _uneven_rows(rank_or_all):
    g = torch.Generator().manual_seed(78)
    parts = [torch.randn(2 * 16 * 16, C, generator=g) * 1.5 + 0.3, torch.randn(2 * 16 * 24, C, generator=g) * 0.7 - 0.2]
    grads = [torch.randn(p.shape, generator=g) for p in parts]
    return (parts, grads) if rank_or_all is None else (parts[rank_or_all], grads[rank_or_all])


def _affine(n=C):
    g = torch.Generator().manual_seed(9)
    return torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.1


def _node_worker(rank, world, init_file, out_dir):
    import torch.distributed as dist
    from pytorch_object_detection_amd import train_ops
    from pytorch_object_detection_amd._lib import ACT_SILU
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        bn = torch.nn.SyncBatchNorm(C).to(dev).train()
        with torch.no_grad():
            w, b = _affine()
            bn.weight.copy_(w), bn.bias.copy_(b)
        x, gy = _uneven_rows(rank)
        pad = lambda t: torch.nn.functional.pad(t, (0, CW - C))      # noqa: E731  (zero pad channels, as the MBConv trunk holds its maps)
        x = pad(x).to(dev).requires_grad_(True)
        train_ops.SYNC_TRACE.clear()
        assert train_ops._is_sync(bn) and not train_ops._bn_train_ok(bn, x) and train_ops._bn_train_wide_ok(bn, x)
        y = train_ops._bn_wide_rows(bn, x, ACT_SILU)
        y.backward(pad(gy).to(dev) + 1.0)                             # (a non-zero incoming gradient on the pad channels too: dx must not pick it up)
        assert list(train_ops.SYNC_TRACE) == [("fwd", 0), ("bwd", 0)] and not train_ops._PENDING
        torch.save({"y": y.detach().cpu(), "dx": x.grad.cpu(), "dgamma": bn.weight.grad.cpu(), "dbeta": bn.bias.grad.cpu(),
                    "rm": bn.running_mean.cpu(), "rv": bn.running_var.cpu(), "nbt": int(bn.num_batches_tracked),
                    "fallbacks": train_ops.STATS["stock_fallbacks"]}, os.path.join(out_dir, f"u{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_wide_syncbatchnorm_node_on_uneven_shards():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_node_worker, args=(2, os.path.join(tmp, "rdzv"), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, f"u{i}.pt")) for i in range(2)]
    parts, grads = _uneven_rows(None)
    bn = torch.nn.BatchNorm1d(C).double().train()
    with torch.no_grad():
        w, b = _affine()
        bn.weight.copy_(w), bn.bias.copy_(b)
    x = torch.cat(parts).double().requires_grad_(True)
    y = torch.nn.functional.silu(bn(x))
    y.backward(torch.cat(grads).double() + 1.0)
    n0 = parts[0].shape[0]
    for i, sl in enumerate((slice(0, n0), slice(n0, None))):
        assert r[i]["fallbacks"] == 0 and r[i]["y"].shape[1] == CW and r[i]["dx"].shape[1] == CW
        assert bool((r[i]["y"][:, C:] == 0.0).all()) and bool((r[i]["dx"][:, C:] == 0.0).all()), "pad channels must stay exactly 0"
        np.testing.assert_allclose(r[i]["y"][:, :C].numpy(), y[sl].detach().float().numpy(), rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(r[i]["dx"][:, :C].numpy(), x.grad[sl].float().numpy(), rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(r[i]["rm"].numpy(), bn.running_mean.float().numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(r[i]["rv"].numpy(), bn.running_var.float().numpy(), rtol=1e-5, atol=1e-7)
        assert r[i]["nbt"] == 1
    assert torch.equal(r[0]["rm"], r[1]["rm"]) and torch.equal(r[0]["rv"], r[1]["rv"])        # both ranks finished from the same global sums
    # the affine gradients are per-rank sums (DDP averages them): together they are the full batch's
    np.testing.assert_allclose((r[0]["dgamma"] + r[1]["dgamma"]).numpy(), bn.weight.grad.float().numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose((r[0]["dbeta"] + r[1]["dbeta"]).numpy(), bn.bias.grad.float().numpy(), rtol=2e-4, atol=2e-5)


# ================================================================================================ a2. the conv + norm dispatch at a wide width
CIN, COUT = 32, 96          # 96 / 4 = 24 does not divide 256: a width of the any-width family whose data gradient (Cout % 32 == 0) is on the HIP kernels too


def _conv_case():
    g = torch.Generator().manual_seed(79)
    hw = [(16, 16), (16, 24)]                                            # rank 0: 2 x 16 x 16 pixels, rank 1: 2 x 16 x 24
    xs = [torch.randn(2 * h * w, CIN, generator=g) for h, w in hw]
    gys = [torch.randn(2 * h * w, COUT, generator=g) for h, w in hw]
    weight = torch.randn(COUT, CIN, 1, 1, generator=g) * 0.3
    return hw, xs, gys, weight


def _conv_worker(rank, world, init_file, out_dir):
    import copy
    import torch.distributed as dist
    from pytorch_object_detection_amd import train_ops
    from pytorch_object_detection_amd._lib import ACT_SILU, Segs
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        hw, xs, gys, weight = _conv_case()
        conv = torch.nn.Conv2d(CIN, COUT, 1, bias=False).to(dev)
        bn = torch.nn.SyncBatchNorm(COUT).to(dev).train()
        with torch.no_grad():
            w, b = _affine(COUT)
            conv.weight.copy_(weight), bn.weight.copy_(w), bn.bias.copy_(b)
        segs = Segs.make(2, [hw[rank]])
        gy = gys[rank].to(dev)
        out = {}
        for mode in ("one_shot", "begin_finish"):
            m, n = copy.deepcopy(conv), copy.deepcopy(bn)
            x = xs[rank].to(dev).requires_grad_(True)
            train_ops.SYNC_TRACE.clear()
            if mode == "one_shot":                                       # where conv_norm_act_rows used to return None
                y = train_ops.conv_norm_act_rows(m, n, x, segs, ACT_SILU)
            else:                                                        # the collective in flight under an independent launch, the backward deferred
                h = train_ops.conv_norm_begin(m, n, x, segs, ACT_SILU)
                assert h is not None and h.sync is not None and h.sync.wide and h.sync.defer
                train_ops.act_rows(x.detach(), ACT_SILU)
                y = train_ops.conv_norm_finish(h)
            assert y is not None
            y.backward(gy)
            torch.cuda.synchronize()
            tr = list(train_ops.SYNC_TRACE)
            assert [k for k, _ in tr] == ["fwd", "bwd"] and not train_ops._PENDING, tr
            assert (tr[0][1] == 0) if mode == "one_shot" else (tr[0][1] >= 1), tr          # launches enqueued under the forward collective
            out[mode] = {"y": y.detach().cpu(), "dx": x.grad.cpu(), "dw": m.weight.grad.cpu(), "dgamma": n.weight.grad.cpu(), "dbeta": n.bias.grad.cpu(),
                         "rm": n.running_mean.cpu(), "rv": n.running_var.cpu(), "nbt": int(n.num_batches_tracked)}
        out["fallbacks"] = train_ops.STATS["stock_fallbacks"]
        torch.save(out, os.path.join(out_dir, f"c{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_conv_norm_dispatch_takes_the_wide_synchronised_node():
    """conv_norm_act_rows and conv_norm_begin / conv_norm_finish on a 1x1 conv 32 -> 96 + SyncBatchNorm(96) + SiLU, uneven shards: the deferred form is
    bit for bit the one-shot form, and both are the float64 conv + BatchNorm over all rows within FT._bound (4 x the error of the same float32 CPU graph
    + 1e-6 of the reference's maximum)."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_conv_worker, args=(2, os.path.join(tmp, "rdzv"), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, f"c{i}.pt")) for i in range(2)]
    hw, xs, gys, weight = _conv_case()

    def graph(dtype):
        x = torch.cat(xs).to(dtype).requires_grad_(True)
        wt = weight.view(COUT, CIN).to(dtype).requires_grad_(True)
        bn = torch.nn.BatchNorm1d(COUT).to(dtype).train()
        with torch.no_grad():
            w, b = _affine(COUT)
            bn.weight.copy_(w), bn.bias.copy_(b)
        y = torch.nn.functional.silu(bn(x @ wt.t()))
        y.backward(torch.cat(gys).to(dtype))
        return dict(y=y.detach(), dx=x.grad, dw=wt.grad.view(COUT, CIN, 1, 1), dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var)

    ref, f32 = graph(torch.float64), graph(torch.float32)
    n0 = xs[0].shape[0]
    for i in range(2):
        assert r[i]["fallbacks"] == 0
        for k, v in r[i]["one_shot"].items():
            same = torch.equal(v, r[i]["begin_finish"][k]) if isinstance(v, torch.Tensor) else v == r[i]["begin_finish"][k] == 1
            assert same, f"rank {i}: {k} differs between the one-shot and the deferred form"
    got = dict(y=torch.cat([r[0]["one_shot"]["y"], r[1]["one_shot"]["y"]]), dx=torch.cat([r[0]["one_shot"]["dx"], r[1]["one_shot"]["dx"]]),
               rm=r[0]["one_shot"]["rm"], rv=r[0]["one_shot"]["rv"], **{k: r[0]["one_shot"][k] + r[1]["one_shot"][k] for k in ("dw", "dgamma", "dbeta")})
    assert got["y"].shape[0] == n0 + xs[1].shape[0]
    assert torch.equal(r[0]["one_shot"]["rm"], r[1]["one_shot"]["rm"]) and torch.equal(r[0]["one_shot"]["rv"], r[1]["one_shot"]["rv"])
    for k, g in got.items():
        bound, e32 = FT._bound(ref[k].numpy(), f32[k].double().numpy())
        err = float((g.double() - ref[k]).abs().max())
        print(f"conv 32 -> 96 + SyncBatchNorm + SiLU, two ranks, {k}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  max|ref| {float(ref[k].abs().max()):.3e}")
        assert err <= bound, (k, err, e32, bound)


# ================================================================================================ b. the whole step, B0, all switches
def _step_worker(rank, world, init_file, out_dir):
    import torch.distributed as dist
    from pytorch_object_detection_amd import train_ops
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        model = FT._fcos("b0", False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.enable_training(**FT.ALL)
        model.to(dev).train()
        net = torch.nn.parallel.DistributedDataParallel(model, find_unused_parameters=True)      # as train.py:101
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)                                   # as train.py:103
        model = net.module
        # the trunk's SyncBatchNorm modules in training mode: counted, not written down (_bn1 belongs to the classifier head _conv_head / _bn1 / _fc, which
        # the detector never runs)
        n_sync = sum(isinstance(m, torch.nn.SyncBatchNorm) and m.training and m is not model.backbone.model._bn1 for m in model.backbone.modules())
        assert not any(type(m) is torch.nn.BatchNorm2d for m in model.modules())
        x, gt, labels = _batch(CONFIGS["b0"][2])
        drop_u = FT._drop_u("b0")[0]
        x, gt, labels, drop_u = x[rank:rank + 1].to(dev), gt[rank:rank + 1].to(dev), labels[rank:rank + 1].to(dev), drop_u[:, rank:rank + 1].to(dev)
        calls = []
        real = dist.all_reduce
        dist.all_reduce = lambda t, *a, **k: (calls.append((t.dtype, t.numel())), real(t, *a, **k))[1]
        train_ops.SYNC_TRACE.clear()
        train_ops.STATS["stock_fallbacks"], train_ops.STATS["cl_copies"] = 0, 0
        net.zero_grad()
        out = net(x, drop_u=drop_u)
        target = FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])
        losses = FCOSLoss("giou")([out, target])
        losses[-1].backward()
        torch.cuda.synchronize()
        dist.all_reduce = real
        res = {"losses": [float(v.detach()) for v in losses], "n_sync": n_sync, "stat_calls": sum(c[0] == torch.float64 for c in calls),
               "trace": list(train_ops.SYNC_TRACE), "pending": len(train_ops._PENDING), "stats": dict(train_ops.STATS),
               "grads": {n: (p.grad.cpu() if p.grad is not None else None) for n, p in model.named_parameters() if p.requires_grad},
               "frozen": [n for n, p in model.named_parameters() if not p.requires_grad],
               "running": {n: (m.running_mean.cpu(), m.running_var.cpu(), int(m.num_batches_tracked)) for n, m in model.named_modules()
                           if isinstance(m, torch.nn.SyncBatchNorm) and n.startswith("backbone.")}}
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_b0_step_under_ddp_and_convert_sync_batchnorm():
    """FCOS(efficientnet=True, freeze_bn=False).enable_training(all switches) -> DistributedDataParallel -> convert_sync_batchnorm, image r and
    drop_u[:, r] on rank r: zero stock fallbacks, one fp64 all-reduce per trunk SyncBatchNorm and direction, and the loss, every trainable parameter's
    gradient and the running statistics of the two-image restatement under the bars of test_effnet_fulltrain_gpu._run_step."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_step_worker, args=(2, os.path.join(tmp, "rdzv"), tmp), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(tmp, f"rank{i}.pt")) for i in range(2))
    # ---- collective bookkeeping
    for r in (r0, r1):
        assert r["stats"]["stock_fallbacks"] == 0, r["stats"]
        assert r["n_sync"] > 40 and r["stat_calls"] == 2 * r["n_sync"], (r["stat_calls"], r["n_sync"])
        assert len(r["trace"]) == r["stat_calls"] and sum(k == "fwd" for k, _ in r["trace"]) == sum(k == "bwd" for k, _ in r["trace"]) == r["n_sync"]
        assert r["pending"] == 0
    # ---- against the float32 restatement of the two-image step
    _, ref_losses, g32, run = FT._ref_step("b0", "all", torch.float32)
    _, _, g64, _ = FT._ref_step("b0", "all", torch.float64)
    got_losses = [(a + b) / 2 for a, b in zip(r0["losses"], r1["losses"])]
    print("b0 all, two ranks: losses", r0["losses"], r1["losses"], "mean", got_losses, "restatement", ref_losses)
    np.testing.assert_allclose(got_losses[-1], ref_losses[-1], rtol=2e-4)
    top = max(float(g.abs().max()) for g in g64.values())
    zero = {n for n, g in g64.items() if 0.0 < float(g.abs().max()) < 1e-9 * top}
    assert zero == FT._expected_zero_class("b0", "all"), zero ^ FT._expected_zero_class("b0", "all")
    fig = {}
    for n, g in g64.items():
        if n not in zero and float(g.abs().max()) > 0.0:
            fig[FT._group(n)] = max(fig.get(FT._group(n), 0.0), float((g32[n] - g).abs().max()) / float(g.abs().max()))
    zero_bar = 4 * max([float(g32[n].abs().max()) for n in zero], default=0.0)
    print("b0 all, two ranks: restatement fp32-vs-float64 per group:", fig, "| structurally zero:", len(zero), "parameters, bar", zero_bar)
    assert all(n not in g32 for n in r0["frozen"]) and r0["frozen"] == r1["frozen"]
    assert set(r0["grads"]) == set(g32), set(r0["grads"]) ^ set(g32)                              # no trainable parameter is left out
    worst, checked, bad = {}, 0, []
    for name, g in r0["grads"].items():
        g_ref = g32[name]
        assert g is not None and r1["grads"][name] is not None and g.shape == g_ref.shape, name
        assert torch.equal(g, r1["grads"][name]), f"{name}: the ranks hold different gradients"
        checked += 1
        if name in zero:
            if not float(g.abs().max()) <= zero_bar:
                bad.append((name, float(g.abs().max()), zero_bar))
            continue
        grp = FT._group(name)
        scale = float(g_ref.abs().max()) + 1e-12
        err = float((g.double() - g_ref).abs().max()) / scale
        if err > worst.get(grp, ("", 0.0))[1]:
            worst[grp] = (name, err)
        if not err <= max(2e-3 if grp == "fpn+head" else 2e-2, 4 * fig[grp]):
            bad.append((name, err, scale))
    print("b0 all, two ranks: gradients checked:", checked, "worst max |err| / max |ref|:", worst)
    assert checked > 100 and not bad, bad
    # ---- running statistics: equal on both ranks, the restatement's
    assert len(run.stats) == r0["n_sync"] == len([n for n, v in r0["running"].items() if v[2] == 1])
    for bn_name, (rm, rv, cnt) in run.stats.items():
        (m0, v0, c0), (m1, v1, c1) = r0["running"][bn_name], r1["running"][bn_name]
        assert cnt == 1 and c0 == c1 == 1, bn_name
        assert torch.equal(m0, m1) and torch.equal(v0, v1), bn_name
        np.testing.assert_allclose(m0.numpy(), rm.numpy(), atol=1e-4, rtol=1e-4, err_msg=bn_name)
        np.testing.assert_allclose(v0.numpy(), rv.numpy(), atol=1e-4, rtol=1e-4, err_msg=bn_name)
