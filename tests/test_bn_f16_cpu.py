"""Host side of the f16-map batch-statistics BatchNorm (fd_batchnorm_train_*_nhwc_h, enable_trunk_batch_stats(f16_maps=True)): the float64 restatement of
tests/bn_f16_ref.py held against torch's CPU autograd, the six entry points in the library, the header and the signature table, every refusal that is
reachable before a launch with its code, and the public switch."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_f16_ref as R
from pytorch_object_detection_amd import _lib
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.od import FCOS, MNFCOS, HalfInvertedStageFCOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the f16 form -> the fp32 form whose argument list it shares
NEW = {"fd_batchnorm_train_fwd_nhwc_h": "fd_batchnorm_train_fwd_nhwc", "fd_batchnorm_train_res_fwd_nhwc_h": "fd_batchnorm_train_res_fwd_nhwc",
       "fd_batchnorm_train_bwd_nhwc_h": "fd_batchnorm_train_bwd_nhwc", "fd_batchnorm_train_sync_fwd_nhwc_h": "fd_batchnorm_train_sync_fwd_nhwc",
       "fd_batchnorm_train_sync_res_fwd_nhwc_h": "fd_batchnorm_train_sync_res_fwd_nhwc",
       "fd_batchnorm_train_sync_bwd_nhwc_h": "fd_batchnorm_train_sync_bwd_nhwc"}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("act,res", [(R.ACT_NONE, False), (R.ACT_RELU, False), (R.ACT_SILU, False), (R.ACT_NONE, True), (R.ACT_RELU, True)])
def test_restatement_is_torch_autograd_in_float64(act, res):
    """F.batch_norm in training mode (+ residual, + activation) run by torch in float64 on the exact upcasts of f16 inputs, and its autograd.  (The residual
    form has no SiLU.)"""
    gen = torch.Generator().manual_seed(11 + act + 7 * res)
    rows, C, eps, momentum = 37, 12, 1e-3, 0.1
    x_h = (torch.randn(rows, C, generator=gen) * 2 + 0.5).half()
    res_h = torch.randn(rows, C, generator=gen).half() if res else None
    dy_h = torch.randn(rows, C, generator=gen).half()
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    rmean, rvar = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    y, mean, rstd, rm, rv = R.forward(x_h, gamma, beta, eps, act, res_h, rmean, rvar, momentum)

    xt = x_h.double().requires_grad_(True)
    gt, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rt = res_h.double().requires_grad_(True) if res else None
    trm, trv = rmean.double().clone(), rvar.double().clone()
    z = F.batch_norm(xt, trm, trv, gt, bt, True, momentum, eps)
    if res:
        z = z + rt
    yt = {R.ACT_NONE: lambda t: t, R.ACT_RELU: torch.relu, R.ACT_SILU: F.silu}[act](z)
    (yt * dy_h.double()).sum().backward()
    tol = dict(rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(y.numpy(), yt.detach().numpy(), **tol)
    np.testing.assert_allclose(rm.numpy(), trm.numpy(), **tol)
    np.testing.assert_allclose(rv.numpy(), trv.numpy(), **tol)
    if res:                                        # the residual form's backward: the plain one with ACT_NONE on the masked gradient, which is dres too
        g = dy_h.double() * (y > 0) if act == R.ACT_RELU else dy_h.double()
        np.testing.assert_allclose(g.numpy(), rt.grad.numpy(), **tol)
        xh = (x_h.double() - mean) * rstd
        dbeta, dgamma = g.sum(0), (g * xh).sum(0)
        dx = rstd * gamma.double() * (g - dbeta / rows - xh * dgamma / rows)
    else:
        dx, dgamma, dbeta = R.backward(x_h, dy_h, gamma, beta, eps, act)
    np.testing.assert_allclose(dx.numpy(), xt.grad.numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(dgamma.numpy(), gt.grad.numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(dbeta.numpy(), bt.grad.numpy(), rtol=1e-9, atol=1e-10)


def test_round_f16_is_nearest_even_and_overflows_to_inf():
    t = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, -70000.0, 2.0 ** -25, 2.0 ** -25 * 1.01], dtype=torch.float64)
    got = R.round_f16(t).double()
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -9, 65504.0, float("inf"), float("-inf"), 0.0, 2.0 ** -24]
    u = R.f16_ulp(torch.tensor([0.0, 2.0 ** -20, 1.0, 1.5, 2.0, 40000.0], dtype=torch.float64))
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 32.0]


# ------------------------------------------------------------------------------------------------ the entry points
def test_new_symbols_are_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for new, old in NEW.items():
        assert new in declared and new in _lib.EXPORTS and new in _lib._SIGS and hasattr(lib, new), new
        assert _lib._SIGS[new] == _lib._SIGS[old], new                 # the arguments are those of the fp32 entry point
    assert not [n for n in _lib.EXPORTS if n.endswith("_cma_nhwc_h") or re.fullmatch(r"fd_(batchnorm_sync|groupnorm)_.*_h", n)]


class _Call:
    """One of the six entry points with a valid argument list over host memory (every call made here must be refused before a launch): rows = 64, C = 24 on
    channel views at co = 8 of 40-element rows; keyword overrides name the argument to break."""

    def __init__(self, lib, kind, sync):
        self.lib, self.kind, self.sync = lib, kind, sync
        self.buf = torch.zeros(8192)
        self.p = self.buf.data_ptr()
        assert self.p % 16 == 0
        q = lib.fd_batchnorm_train_sync_workspace_bytes if sync else lib.fd_batchnorm_train_workspace_bytes
        self.need = q(64, 24)
        assert self.need > 0

    def __call__(self, **kw):
        p = self.p
        a = dict(x=p, x_cs=40, x_co=8, g=p, g_cs=40, g_co=8, gamma=p, beta=p, out=p, out_cs=40, out_co=8, dgamma=p, dbeta=p, rows=64, C=24, eps=1e-3, act=0,
                 phase=2, sums=p, total=-1.0, mom=0.1, rmean=None, rvar=None, fws=p, ws=p, nb=self.buf.numel() * 4)
        a.update(kw)
        sync = (a["phase"], a["sums"], a["total"]) if self.sync else ()
        name = "fd_batchnorm_train_" + ("sync_" if self.sync else "") + {"fwd": "fwd", "res": "res_fwd", "bwd": "bwd"}[self.kind] + "_nhwc_h"
        fn = getattr(self.lib, name)
        if self.kind == "bwd":
            return fn(a["x"], a["x_cs"], a["x_co"], a["g"], a["g_cs"], a["g_co"], a["gamma"], a["beta"], a["out"], a["out_cs"], a["out_co"], a["dgamma"],
                      a["dbeta"], a["rows"], a["C"], a["eps"], a["act"], *sync, a["fws"], a["ws"], a["nb"], None)
        res = (a["g"], a["g_cs"], a["g_co"]) if self.kind == "res" else ()
        return fn(a["x"], a["x_cs"], a["x_co"], a["gamma"], a["beta"], *res, a["out"], a["out_cs"], a["out_co"], a["rows"], a["C"], a["eps"], a["act"],
                  *sync, a["mom"], a["rmean"], a["rvar"], a["ws"], a["nb"], None)


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("kind", ["fwd", "res", "bwd"])
def test_every_refusal_before_a_launch_has_its_code(kind, sync):
    lib = _lib.lib()
    call = _Call(lib, kind, sync)
    p, U, V = call.p, _lib.E_UNSUPPORTED, _lib.E_INVAL
    # shapes: FD_E_UNSUPPORTED
    assert call(C=22) == U and call(C=0) == U and call(C=2) == U and call(C=4100, x_cs=4200, g_cs=4200, out_cs=4200) == U
    assert call(rows=0) == U and b"unsupported" in lib.fd_last_error()
    assert call(rows=1, nb=0) == (V if sync else U)                  # one row: a shape only the synchronised form takes (refused here for its workspace)
    # the 8-byte rule of f16 views: a pointer aligned to 4 but not to 8 bytes is refused, one aligned to 8 but not to 16 is NOT a view error
    for name in ("x", "out") + (("g",) if kind != "fwd" else ()):
        assert call(**{name: p + 4}) == V, name
        assert b"channel view" in lib.fd_last_error() or b"phase" in lib.fd_last_error()
        assert call(**{name: p + 8, "nb": call.need - 8}) == V and b"workspace" in lib.fd_last_error(), name       # got past the views to the workspace
        for brk in (dict(cs=42), dict(co=6), dict(cs=28)):                                     # cs % 4, co % 4, cs < co + C
            assert call(**{f"{name}_{k}": v for k, v in brk.items()}) == V, (name, brk)
        assert call(**{name: None}) == V
    assert call(gamma=None) == V and call(beta=None) == V
    # activations: SiLU has no residual form; an unknown one nowhere
    assert call(act=_lib.ACT_SILU, nb=0) == (U if kind == "res" else V)      # (elsewhere SiLU gets past the activation check, to the workspace's)
    assert call(act=7) == U and b"activation" in lib.fd_last_error()
    # workspaces
    assert call(nb=call.need - 8) == V and b"workspace" in lib.fd_last_error()
    assert call(ws=None) == V and call(ws=p + 4) == V
    if kind == "bwd":
        assert call(fws=None) == V and call(dgamma=None, phase=1) == V and call(dbeta=None, phase=1) == V
    else:
        assert call(rmean=p) == V and b"go together" in lib.fd_last_error()
        assert call(rvar=p) == V and call(eps=-1.0) == V
    if sync:
        assert call(phase=0) == U and call(phase=3) == U and b"phase" in lib.fd_last_error()
        assert call(sums=None) == V and call(sums=p + 4) == V
        assert call(total=1.0) == V and call(total=32.0) == V and b"total_rows" in lib.fd_last_error()
    # the order of the checks is the fp32 entry point's: shape before activation before views before workspace
    assert call(C=22, act=7, x=None, nb=0) == U and b"rows=" in lib.fd_last_error()
    assert call(act=7, x=None, nb=0) == U and b"activation" in lib.fd_last_error()
    assert call(x=None, nb=0) == V and b"workspace" not in lib.fd_last_error()


def test_wrappers_refuse_mixed_map_types_by_name():
    """ops.batchnorm_train_* take fp32 or f16 Rows; a map of the other type than x is named.  (Rows live on the GPU: here the helper that decides is held
    to stand-ins with the one attribute it reads; tests/test_bn_f16_kernels_gpu.py calls the wrappers.)"""
    from types import SimpleNamespace

    from pytorch_object_detection_amd import ops
    x, y = SimpleNamespace(f16=True), SimpleNamespace(f16=False)
    with pytest.raises(FdError, match=r"y is an fp32 map but x is f16"):
        ops._bn_maps_f16("batchnorm_train_fwd", x, res=None, y=y)
    with pytest.raises(FdError, match=r"dy is an f16 map but x is fp32"):
        ops._bn_maps_f16("batchnorm_train_bwd", y, dy=x, dx=y)
    assert ops._bn_maps_f16("w", x, res=x, y=x) is True and ops._bn_maps_f16("w", y, res=None, y=y) is False


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_sets_both_flags_returns_self_and_defaults_to_off():
    for model in (HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False), FCOS([2048, 1024, 512], 20, 64, freeze_bn=False),
                  MNFCOS([2048, 1024, 512], 20, 64, freeze_bn=False)):
        trunk = model.backbone.trunk
        assert trunk.hip_bn_f16_maps is False and model.backbone.hip_bn_f16_maps is False and "hip_bn_f16_maps" not in vars(trunk)
        assert model.enable_trunk_batch_stats() is model                       # called as today: the new flag stays off
        assert trunk.hip_bn_train is True and trunk.hip_bn_f16_maps is False and model.backbone.hip_bn_f16_maps is False
        assert model.enable_trunk_batch_stats(f16_maps=True) is model
        assert trunk.hip_bn_train is True and trunk.hip_bn_f16_maps is True and model.backbone.hip_bn_f16_maps is True
        assert model.backbone.hip_bn_train is True and trunk.hip_stem_train is False
        import copy
        twin = copy.deepcopy(model)                                            # what AveragedModel does: the switches travel
        assert twin.backbone.trunk.hip_bn_f16_maps is True and twin.backbone.trunk.hip_bn_train is True
        assert model.enable_trunk_batch_stats(f16_maps=False) is model and trunk.hip_bn_f16_maps is False and trunk.hip_bn_train is True
    other = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False)
    assert other.backbone.trunk.hip_bn_f16_maps is False and other.backbone.trunk.hip_bn_train is False         # per instance


def test_switch_keeps_its_three_refusals():
    for model in (HalfInvertedStageFCOS([512, 1024, 2048], 20, 64), FCOS([2048, 1024, 512], 20, 64), MNFCOS([2048, 1024, 512], 20, 64)):
        with pytest.raises(FdError, match=r"bn_freeze=False / freeze_bn=False"):
            model.enable_trunk_batch_stats(f16_maps=True)
        assert model.backbone.trunk.hip_bn_train is False and model.backbone.trunk.hip_bn_f16_maps is False
    for freeze in (True, False):
        eff = FCOS([320, 112, 40], 20, 64, freeze_bn=freeze, efficientnet=True)
        with pytest.raises(FdError, match=r"enable_training\(batch_stats=True\)"):
            eff.enable_trunk_batch_stats(f16_maps=True)
    fpn = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).fpn      # a PlannedModule without a backbone
    with pytest.raises(FdError, match="no ResNet-50 trunk"):
        fpn.enable_trunk_batch_stats(f16_maps=True)
