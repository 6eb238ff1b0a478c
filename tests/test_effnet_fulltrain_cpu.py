"""The full EfficientNet training arithmetic (batch-statistics BatchNorm, drop-connect, trainable stem), the parts that need no GPU: the float64-capable
restatement tests/effnet_train_ref.py against the oracle and nn.BatchNorm2d, drop-connect known answers (restatement and product), the new entry points'
declarations, argument errors and workspace queries, the switch defaults of FCOS.enable_training() and the refusals that remain."""
import os
import re
import warnings

import pytest
import torch

import effnet_train_ref as TR
from effnet_init import init_effnet
from oracle import effnet_ref as E
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.backbone import efficientnetv1 as V
from pytorch_object_detection_amd.model.od import FCOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_batchnorm_train_workspace_bytes", "fd_batchnorm_train_fwd_nhwc", "fd_batchnorm_train_bwd_nhwc", "fd_sample_scale_add_nhwc",
       "fd_stem_conv_wgrad_workspace_bytes", "fd_stem_conv_bwd_weight_nhwc4")


def _b0(freeze_bn=True, seed=5):
    torch.manual_seed(seed)
    model = FCOS([320, 112, 40], 20, 64, freeze_bn=freeze_bn, efficientnet=True).eval()
    init_effnet(model.backbone, seed + 1)
    return model


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_in_eval_mode_is_the_oracle_bit_for_bit():
    model = _b0()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = E.efficientnet_endpoints5(sd, x, 0)
        got = TR.trunk(sd, x, "efficientnet-b0")
        assert len(ref) == len(got) == 5
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        o_ref, o_got = E.fcos_effnet_forward(sd, x, 0), TR.fcos_effnet_forward(sd, x, 0)
    for ga, gb in zip(o_got, o_ref):
        for a, b in zip(ga, gb):
            assert torch.equal(a, b)


def test_restatement_running_statistics_are_batchnorm2ds():
    gen = torch.Generator().manual_seed(2)
    m = torch.nn.BatchNorm2d(24, momentum=V.BN_MOMENTUM, eps=V.BN_EPS).train()
    with torch.no_grad():
        m.running_mean.copy_(torch.randn(24, generator=gen))
        m.running_var.copy_(torch.rand(24, generator=gen) + 0.5)
        m.weight.copy_(torch.rand(24, generator=gen) + 0.5)
        m.bias.copy_(torch.randn(24, generator=gen))
    sd = {"bn." + k: v.clone() for k, v in m.state_dict().items()}
    run = TR.Running()
    for step in range(2):
        x = torch.randn(3, 24, 5, 7, generator=gen) * 2 + 1
        want, got = m(x), TR.bn(sd, "bn", x, True, run)
        assert torch.equal(want, got)
        assert torch.equal(run.stats["bn"][0], m.running_mean) and torch.equal(run.stats["bn"][1], m.running_var)
        assert run.stats["bn"][2] == int(m.num_batches_tracked) == step + 1
    assert not torch.equal(sd["bn.running_mean"], m.running_mean)             # the clones moved, the state dict did not
    assert torch.equal(TR.bn(sd, "bn", x, False, None), torch.nn.functional.batch_norm(x, sd["bn.running_mean"], sd["bn.running_var"], sd["bn.weight"],
                                                                                         sd["bn.bias"], False, 0.0, V.BN_EPS))


def _skip_block():
    k, s, e, cin, cout, nominal = 5, 1, 6, 16, 16, 14
    blk = V._MBConv(k, s, e, cin, cout, 0.25, nominal).eval()
    init_effnet(blk, 11)
    sd = {"blk." + n: v.clone().double() for n, v in blk.state_dict().items()}
    x = torch.randn(3, cin, 6, 5, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    return sd, x, (k, s, e, cin, cout, nominal)


def test_drop_connect_known_answers():
    sd, x, geo = _skip_block()
    p = 0.25
    with torch.no_grad():
        full = TR.mbconv(sd, "blk", x, *geo)
        branch = full - x
        # u < p: floor((1 - p) + u) = 0, the branch is removed; u >= p: floor = 1, the branch is scaled by 1 / (1 - p)
        u = torch.tensor([0.1, 0.9, 0.249])
        sc = TR.drop_scale(p, u, torch.float64)
        assert sc.tolist() == [0.0, 1.0 / 0.75, 0.0]
        got = TR.mbconv(sd, "blk", x, *geo, scale=sc)
        assert torch.equal(got[0], x[0]) and torch.equal(got[2], x[2])
        torch.testing.assert_close(got[1], branch[1] / 0.75 + x[1], rtol=1e-12, atol=1e-12)
    # the product's mask arithmetic is the same expression in fp32
    s32 = T.drop_connect_scale(p, u)
    assert s32.dtype == torch.float32 and s32.tolist() == [0.0, float(torch.tensor(1.0) / torch.tensor(0.75)), 0.0]


def test_drop_connect_rate_scales_per_block_and_block0_never_drops():
    rates = TR.block_rates("efficientnet-b0", 0.2)
    _, blocks, _, _ = E.block_table("efficientnet-b0")
    assert len(rates) == len(blocks) == 16 and rates[0] == 0.0
    for i, (k, s, e, cin, cout, nominal) in enumerate(blocks):
        assert rates[i] == (0.2 * i / 16 if (s == 1 and cin == cout) else 0.0)
    assert sum(r > 0 for r in rates) == 9                     # B0: 9 of the 16 blocks have a skip connection (block 0 does not: 32 -> 16)
    # the product's per-block scales: None where nothing drops, the package's expression elsewhere
    net = _b0().backbone.model
    net.drop_connect_rate = 0.2
    u = torch.rand(16, 3, generator=torch.Generator().manual_seed(6))
    got = V._drop_scales(net, 3, "cpu", u)
    for i, r in enumerate(rates):
        if r == 0.0:
            assert got[i] is None
        else:
            assert torch.equal(got[i], TR.drop_scale(r, u[i], torch.float32))
    # a block 0 WITH a skip connection still never drops: p = rate * 0 / n = 0
    net._blocks[0].skip = True
    assert V._drop_scales(net, 3, "cpu", u)[0] is None
    with pytest.raises(FdError, match="drop_u"):
        V._drop_scales(net, 3, "cpu", u[:, :2])


# ------------------------------------------------------------------------------------------------ the entry points
def test_new_symbols_are_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name


def test_workspace_queries_and_argument_errors_need_no_gpu():
    lib = _lib.lib()
    q = lib.fd_batchnorm_train_workspace_bytes
    for rows, C in ((1, 24), (0, 24), (2 ** 31, 24), (64, 6), (64, 0), (64, 4100), (64, 4104)):
        assert q(rows, C) == -1, (rows, C)
    # double [2][C] + double [nchunk][2][C], nchunk = min(1024, ceil(rows / 32)) re-derived so that no chunk is empty: a function of (rows, C) alone
    for rows, C, nchunk in ((2, 24, 1), (37, 40, 2), (4099, 816, 129), (16 * 256 * 256, 144, 1024), (2 ** 31 - 1, 4096, 1024), (1025 * 32, 4, 994)):
        assert q(rows, C) == (2 * C + nchunk * 2 * C) * 8, (rows, C)
    buf = torch.zeros(4096)                                    # (host memory: every call below must fail before any launch)
    p, n = buf.data_ptr(), buf.numel() * 4
    fwd = lambda rows=64, C=24, act=0, x=p, ws=p, nb=n, cs=24, co=0: lib.fd_batchnorm_train_fwd_nhwc(  # noqa: E731
        x, cs, co, p, p, p, cs, co, rows, C, 1e-3, act, 0.1, None, None, ws, nb, None)
    bwd = lambda rows=64, C=24, act=0, ws=p, fws=p, nb=n: lib.fd_batchnorm_train_bwd_nhwc(  # noqa: E731
        p, C, 0, p, C, 0, p, p, p, C, 0, p, p, rows, C, 1e-3, act, fws, ws, nb, None)
    for fn in (fwd, bwd):
        assert fn(C=6) == _lib.E_UNSUPPORTED and fn(C=4100) == _lib.E_UNSUPPORTED and fn(rows=1) == _lib.E_UNSUPPORTED
        assert fn(act=_lib.ACT_SIGMOID) == _lib.E_UNSUPPORTED
        assert fn(ws=None) == _lib.E_INVAL and fn(nb=q(64, 24) - 8) == _lib.E_INVAL
    assert fwd(x=None) == _lib.E_INVAL and fwd(cs=20) == _lib.E_INVAL and fwd(co=2) == _lib.E_INVAL and bwd(fws=None) == _lib.E_INVAL
    assert b"workspace" in lib.fd_last_error()
    assert lib.fd_batchnorm_train_fwd_nhwc(p, 24, 0, p, p, p, 24, 0, 64, 24, 1e-3, 0, 0.1, p, None, p, n, None) == _lib.E_INVAL     # one running tensor only

    sq = lib.fd_stem_conv_wgrad_workspace_bytes
    assert sq(2, 64, 96, 40, 32, 48) == 2 * 4 * 2 // 8 * 64 * 32 * 4        # 2 images x 4 x 2 tiles of 8 x 32 pixels, 8 tiles per slab of [64][32] floats
    assert sq(1, 6, 6, 32, 3, 3) == 64 * 32 * 4 and sq(3, 64, 64, 48, 32, 32) == 2 * 64 * 32 * 4
    assert sq(1, 6, 6, 68, 3, 3) == -1 and sq(1, 6, 6, 30, 3, 3) == -1 and sq(0, 6, 6, 32, 3, 3) == -1 and sq(1, 6, 6, 32, 0, 3) == -1
    stem = lambda K=3, stride=2, Cout=32, ws=p, nb=n, dy=p, pad=0, Ho=3: lib.fd_stem_conv_bwd_weight_nhwc4(  # noqa: E731
        p, dy, Cout, 0, None, p, ws, nb, 1, 6, 6, Cout, K, stride, pad, pad, Ho, 3, None)
    assert stem(K=5) == _lib.E_UNSUPPORTED and stem(stride=1) == _lib.E_UNSUPPORTED and stem(Cout=68) == _lib.E_UNSUPPORTED and stem(Cout=30) == _lib.E_UNSUPPORTED
    assert stem(ws=None) == _lib.E_INVAL and stem(dy=None) == _lib.E_INVAL and stem(nb=64) == _lib.E_INVAL and stem(pad=3) == _lib.E_INVAL and stem(Ho=5) == _lib.E_INVAL

    ssa = lambda N=2, HW=8, C=24, s=p, a=p, cs=24: lib.fd_sample_scale_add_nhwc(a, cs, 0, s, None, 0, 0, p, cs, 0, N, HW, C, None)  # noqa: E731
    assert ssa(N=0) == _lib.E_INVAL and ssa(C=6) == _lib.E_INVAL and ssa(s=None) == _lib.E_INVAL and ssa(a=None) == _lib.E_INVAL and ssa(cs=20) == _lib.E_INVAL


# ------------------------------------------------------------------------------------------------ the switches
def _trainable(model):
    return {n for n, p in model.named_parameters() if p.requires_grad}


def test_enable_training_defaults_are_todays_call():
    model = _b0()
    before = _trainable(model)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert model.enable_training() is model
    assert any("freezes the EfficientNet stem" in str(i.message) for i in w)
    net = model.backbone.model
    stem_head = {"backbone.model." + n for n in ("_conv_stem.weight", "_conv_head.weight", "_fc.weight", "_fc.bias")}
    assert before - _trainable(model) == stem_head            # (freeze_bn=True froze every BatchNorm already)
    assert model.hip_train and net.drop_connect_rate == 0.0 and model.backbone.drop_connect_rate == 0.0
    # no switch was set: the instance holds none of the new attributes, the class defaults say "off"
    assert not {"train_stem", "batch_stats", "drop_connect_accepted"} & set(vars(net))
    assert (net.train_stem, net.batch_stats, net.drop_connect_accepted) == (False, False, 0.0)
    explicit = _b0()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        explicit.enable_training(train_stem=False, batch_stats=False, drop_connect_rate=0.0)
    assert _trainable(explicit) == _trainable(model) and not {"train_stem", "batch_stats", "drop_connect_accepted"} & set(vars(explicit.backbone.model))
    assert FCOS([2048, 1024, 512], 20, 64).enable_training(train_stem=True, drop_connect_rate=0.2).hip_train is False      # ResNet trunk: nothing to do


def test_switches_set_the_trainable_set():
    model = _b0()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model.enable_training(train_stem=True, drop_connect_rate=0.2)
    assert not w                                              # no freeze, no warning
    net = model.backbone.model
    assert net._conv_stem.weight.requires_grad and not net._bn0.weight.requires_grad          # (_bn0 was frozen by freeze_bn=True)
    assert (net.train_stem, net.batch_stats, net.drop_connect_rate, net.drop_connect_accepted) == (True, False, 0.2, 0.2)
    loose = _b0(freeze_bn=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loose.enable_training(batch_stats=True)
    net = loose.backbone.model
    assert not net._conv_stem.weight.requires_grad and not net._bn0.weight.requires_grad and not net._bn1.weight.requires_grad
    assert all(p.requires_grad for b in net._blocks for p in b.parameters())
    both = _b0(freeze_bn=False).enable_training(train_stem=True, batch_stats=True)
    assert both.backbone.model._bn0.weight.requires_grad and both.backbone.model._conv_stem.weight.requires_grad
    both.train()
    assert all(m.training for m in both.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_refusals_that_remain(monkeypatch):
    with pytest.raises(FdError, match="freeze_bn=False"):
        _b0().enable_training(batch_stats=True)
    with pytest.raises(FdError, match="drop_connect_rate"):
        _b0().enable_training(drop_connect_rate=1.0)
    x = torch.randn(1, 3, 64, 64)
    model = _b0()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.enable_training()
    model.backbone.drop_connect_rate = 0.2                     # by hand, without the switch: today's error
    with pytest.raises(FdError, match="drop_connect_rate=0.2 is not supported"):
        V.trunk_train_forward(model.backbone.model, x)
    model.enable_training(train_stem=True, drop_connect_rate=0.2)
    model.backbone.drop_connect_rate = 0.3                     # ... and a rate other than the accepted one
    with pytest.raises(FdError, match="drop_connect_rate=0.3 is not supported"):
        V.trunk_train_forward(model.backbone.model, x)
    with pytest.raises(FdError, match="inference-only"):
        V.EfficientNetV1(0).train()(x)
    # an nn.SyncBatchNorm spanning ranks at a width only the any-width kernels take
    bn = torch.nn.SyncBatchNorm(144).train()
    monkeypatch.setattr(T, "_is_sync", lambda m: isinstance(m, torch.nn.SyncBatchNorm))
    with pytest.raises(FdError, match="no synchronised form"):
        T.batchnorm_train_wide_rows(bn, torch.zeros(8, 160))
    assert int(bn.num_batches_tracked) == 0
