"""Host side of training the ResNet-50 trunk on batch statistics: the float64 bottleneck restatement of tests/resnet_bn_ref.py held against nn.Module
autograd, the public switch PlannedModule.enable_trunk_batch_stats(), and the two new entry points in the header, the export list and the signature table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_bn_ref as BR
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.od import FCOS, MNFCOS, HalfInvertedStageFCOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_batchnorm_train_res_fwd_nhwc", "fd_batchnorm_train_sync_res_fwd_nhwc")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(BR.CASES))
def test_restatement_is_the_module_forward_and_its_autograd(name):
    """In float64: the restatement's output, input gradient, every parameter gradient and the running statistics against the nn.Conv2d / nn.BatchNorm2d
    modules of the same block run by torch (torchvision's Bottleneck.forward written with the modules)."""
    blk, x, gy, seed = BR.build_case(name)
    stride = BR.CASES[name][2]
    assert BR.kink_distance(blk, x, stride) > BR.KINK_MARGIN
    print(f"{name}: seed {seed}, |pre-activation| >= {BR.kink_distance(blk, x, stride):.3e}")
    sd, xr, out, running = BR.reference(blk, x, gy, torch.float64)
    m = blk.double()
    xm = x.double().requires_grad_(True)
    y = F.relu(m.bn1(m.conv1(xm)))
    y = F.relu(m.bn2(m.conv2(y)))
    idt = xm if m.downsample is None else m.downsample(xm)
    om = F.relu(m.bn3(m.conv3(y)) + idt)
    (om * gy.double()).sum().backward()
    tol = dict(rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(out.numpy(), om.detach().numpy(), **tol)
    np.testing.assert_allclose(xr.grad.numpy(), xm.grad.numpy(), **tol)
    params = dict(m.named_parameters())
    assert len(params) == (12 if m.downsample is not None else 9)
    for n, p in params.items():
        np.testing.assert_allclose(sd[n].grad.numpy(), p.grad.numpy(), err_msg=n, **tol)
    mods = dict(m.named_modules())
    assert set(running) == {n for n, mod in mods.items() if isinstance(mod, torch.nn.BatchNorm2d)}
    for n, (rm, rv) in running.items():
        np.testing.assert_allclose(rm.numpy(), mods[n].running_mean.numpy(), **tol)
        np.testing.assert_allclose(rv.numpy(), mods[n].running_var.numpy(), **tol)
        assert int(mods[n].num_batches_tracked) == 1


def test_case_builder_takes_a_seed_clear_of_the_kinks():
    for name, (_, _, stride, _, _) in BR.CASES.items():
        blk, x, _, seed = BR.build_case(name)
        assert all(BR.kink_distance(*BR._make(name, s)[:2], stride) <= BR.KINK_MARGIN for s in range(seed)), "not the FIRST qualifying seed"
        # the fp32-vs-float64 deviation of the restatement's own output sits far below the margin
        o32 = BR.bottleneck(BR.state(blk, torch.float32), x, stride)[0].detach().double()
        o64 = BR.bottleneck(BR.state(blk, torch.float64), x.double(), stride)[0].detach()
        assert float((o32 - o64).abs().max()) < BR.KINK_MARGIN / 10


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_returns_self_and_sets_the_flag_on_the_trunk():
    for model in (HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False), FCOS([2048, 1024, 512], 20, 64, freeze_bn=False),
                  MNFCOS([2048, 1024, 512], 20, 64, freeze_bn=False)):
        trunk = model.backbone.trunk
        assert trunk.hip_bn_train is False and model.backbone.hip_bn_train is False and "hip_bn_train" not in vars(trunk)
        assert model.enable_trunk_batch_stats() is model
        assert trunk.hip_bn_train is True and model.backbone.hip_bn_train is True
        assert trunk.hip_stem_train is False                     # the sibling switch is its own
    other = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False)
    assert other.backbone.trunk.hip_bn_train is False           # per instance, off by default


def test_switch_refuses_what_it_cannot_serve():
    for model in (HalfInvertedStageFCOS([512, 1024, 2048], 20, 64), FCOS([2048, 1024, 512], 20, 64), MNFCOS([2048, 1024, 512], 20, 64)):
        with pytest.raises(FdError, match=r"bn_freeze=False / freeze_bn=False"):
            model.enable_trunk_batch_stats()
        assert model.backbone.trunk.hip_bn_train is False
    for freeze in (True, False):
        eff = FCOS([320, 112, 40], 20, 64, freeze_bn=freeze, efficientnet=True)
        with pytest.raises(FdError, match=r"enable_training\(batch_stats=True\)"):
            eff.enable_trunk_batch_stats()
    fpn = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).fpn      # a PlannedModule without a backbone
    with pytest.raises(FdError, match="no ResNet-50 trunk"):
        fpn.enable_trunk_batch_stats()


# ------------------------------------------------------------------------------------------------ the entry points
def test_new_symbols_are_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name), name
    # the plain signatures with the residual's (pointer, channel stride, channel offset) behind beta
    for new, old in zip(NEW, ("fd_batchnorm_train_fwd_nhwc", "fd_batchnorm_train_sync_fwd_nhwc")):
        res, args = _lib._SIGS[old]
        assert _lib._SIGS[new] == (res, args[:5] + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + args[5:])


def test_argument_errors_need_no_gpu():
    lib = _lib.lib()
    buf = torch.zeros(4096)                                    # (host memory: every call below must fail before any launch)
    p, n = buf.data_ptr(), buf.numel() * 4
    need = lib.fd_batchnorm_train_workspace_bytes(64, 24)
    plain = lambda act=0, res=p, rcs=24, rco=0, nb=n: lib.fd_batchnorm_train_res_fwd_nhwc(  # noqa: E731
        p, 24, 0, p, p, res, rcs, rco, p, 24, 0, 64, 24, 1e-3, act, 0.1, None, None, p, nb, None)
    sync = lambda act=0, res=p, rcs=24, rco=0, nb=n, phase=2: lib.fd_batchnorm_train_sync_res_fwd_nhwc(  # noqa: E731
        p, 24, 0, p, p, res, rcs, rco, p, 24, 0, 64, 24, 1e-3, act, phase, p, -1.0, 0.1, None, None, p, nb, None)
    for fn in (plain, sync):
        assert fn(act=_lib.ACT_SILU) == _lib.E_UNSUPPORTED
        assert b"activation" in lib.fd_last_error()
        assert fn(res=None) == _lib.E_INVAL and fn(rcs=20) == _lib.E_INVAL and fn(rco=2) == _lib.E_INVAL and fn(res=p + 4) == _lib.E_INVAL
        assert fn(nb=need - 8) == _lib.E_INVAL
        assert b"workspace" in lib.fd_last_error()
    assert sync(act=_lib.ACT_SILU, phase=1) == _lib.E_UNSUPPORTED and sync(phase=0) == _lib.E_UNSUPPORTED
