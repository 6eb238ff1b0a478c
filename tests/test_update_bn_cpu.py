"""Host side of optim.update_bn and the cumulative-average (`_cma`) BatchNorm entry points: the float64 restatement of tests/bn_cma_ref.py held against torch,
the six new symbols in the header, the export list and the signature table, their argument errors (on host pointers: before any launch), and what
optim.update_bn resets, leaves alone and restores on a CPU-constructed detector -- against the stock function on the same model."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import bn_cma_ref as CR
from pytorch_object_detection_amd import _lib, optim
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# new entry point -> (its plain sibling, index of `float momentum` in the sibling's argument list)
NEW = {"fd_batchnorm_update_running_cma": ("fd_batchnorm_update_running", 3),
       "fd_batchnorm_update_running_dev_cma": ("fd_batchnorm_update_running_dev", 3),
       "fd_batchnorm_train_fwd_cma_nhwc": ("fd_batchnorm_train_fwd_nhwc", 12),
       "fd_batchnorm_train_res_fwd_cma_nhwc": ("fd_batchnorm_train_res_fwd_nhwc", 15),
       "fd_batchnorm_train_sync_fwd_cma_nhwc": ("fd_batchnorm_train_sync_fwd_nhwc", 15),
       "fd_batchnorm_train_sync_res_fwd_cma_nhwc": ("fd_batchnorm_train_sync_res_fwd_nhwc", 18)}


# ------------------------------------------------------------------------------------------------ the restatement
def _batches(n=5, C=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2 + k, C, 3, 5, generator=g, dtype=torch.float64) * (1.0 + 0.3 * k) + 0.5 * k for k in range(n)]


def test_restatement_is_batchnorm_with_momentum_none():
    """The recurrence over 5 batches against nn.BatchNorm2d(C, momentum=None).double(), from non-trivial starting statistics; and its closed form."""
    batches = _batches()
    bn = nn.BatchNorm2d(6, momentum=None).double().train()
    bn.running_mean.copy_(torch.linspace(-1, 1, 6))
    bn.running_var.copy_(torch.linspace(0.5, 2, 6))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    for x in batches:
        y = bn(x)
        mean, var, _ = CR.batch_stats(CR.rows_of(x))
        want = (CR.rows_of(x) - mean) / torch.sqrt(var + bn.eps)
        torch.testing.assert_close(CR.rows_of(y.detach()), want, rtol=0, atol=1e-12)
    rm, rv, n = CR.cma(batches, rm0, rv0)
    assert n == int(bn.num_batches_tracked) == 5
    torch.testing.assert_close(rm, bn.running_mean, rtol=0, atol=1e-12)
    torch.testing.assert_close(rv, bn.running_var, rtol=0, atol=1e-12)
    am, av, an = CR.update_bn_ref(batches)                 # the first step has factor 1: the starting statistics drop out
    assert an == 5
    torch.testing.assert_close(am, rm, rtol=0, atol=1e-12)
    torch.testing.assert_close(av, rv, rtol=0, atol=1e-12)


def test_restatement_is_stock_update_bn_on_a_plain_sequential():
    batches = _batches(seed=1)
    net = nn.Sequential(nn.BatchNorm2d(6)).double()
    net[0].running_mean.fill_(3.0)
    torch.optim.swa_utils.update_bn(batches, net)
    am, av, an = CR.update_bn_ref(batches)
    assert int(net[0].num_batches_tracked) == an
    torch.testing.assert_close(am, net[0].running_mean, rtol=0, atol=1e-12)
    torch.testing.assert_close(av, net[0].running_var, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ the entry points
def test_new_symbols_are_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    declared = set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for new, (old, at) in NEW.items():
        assert new in declared and new in _lib.EXPORTS and new in _lib._SIGS and hasattr(lib, new), new
        res, args = _lib._SIGS[old]
        assert args[at] is ctypes.c_float, (old, at)
        assert _lib._SIGS[new] == (res, args[:at] + [ctypes.c_void_p] + args[at + 1:]), new
        # the header: the sibling's declaration with `float momentum` replaced by the counter
        decl = lambda name: re.sub(r"\s+", " ", re.search(r"int32_t " + name + r"\(([^;]*)\);", hdr).group(1))      # noqa: E731
        assert decl(old).count("float momentum") == 1
        assert decl(new) == decl(old).replace("float momentum", "const int64_t* num_batches_tracked"), new


def _calls():
    """name -> call(counter, running_mean, running_var) on host pointers with every other argument well-formed."""
    lib = _lib.lib()
    buf = torch.zeros(4096)                                    # (host memory: every call below must fail before any launch)
    p, n = buf.data_ptr(), buf.numel() * 4
    return p, {
        "fd_batchnorm_update_running_cma": lambda k, rm, rv: lib.fd_batchnorm_update_running_cma(p, 64, 24, k, 1e-3, rm, rv, None),
        "fd_batchnorm_update_running_dev_cma": lambda k, rm, rv: lib.fd_batchnorm_update_running_dev_cma(p, p, 24, k, 1e-3, rm, rv, None),
        "fd_batchnorm_train_fwd_cma_nhwc": lambda k, rm, rv: lib.fd_batchnorm_train_fwd_cma_nhwc(
            p, 24, 0, p, p, p, 24, 0, 64, 24, 1e-3, 0, k, rm, rv, p, n, None),
        "fd_batchnorm_train_res_fwd_cma_nhwc": lambda k, rm, rv: lib.fd_batchnorm_train_res_fwd_cma_nhwc(
            p, 24, 0, p, p, p, 24, 0, p, 24, 0, 64, 24, 1e-3, 0, k, rm, rv, p, n, None),
        "fd_batchnorm_train_sync_fwd_cma_nhwc": lambda k, rm, rv: lib.fd_batchnorm_train_sync_fwd_cma_nhwc(
            p, 24, 0, p, p, p, 24, 0, 64, 24, 1e-3, 0, 2, p, -1.0, k, rm, rv, p, n, None),
        "fd_batchnorm_train_sync_res_fwd_cma_nhwc": lambda k, rm, rv: lib.fd_batchnorm_train_sync_res_fwd_cma_nhwc(
            p, 24, 0, p, p, p, 24, 0, p, 24, 0, 64, 24, 1e-3, 0, 2, p, -1.0, k, rm, rv, p, n, None),
    }


@pytest.mark.parametrize("name", list(NEW))
def test_argument_errors_need_no_gpu(name):
    lib = _lib.lib()
    p, calls = _calls()
    call = calls[name]
    for counter in (None, p + 4):                              # null / not 8-byte aligned, with running tensors
        assert call(counter, p, p) == _lib.E_INVAL
        assert b"num_batches_tracked" in lib.fd_last_error() and name.replace("_nhwc", "").encode() in lib.fd_last_error()
    for rm, rv in ((p, None), (None, p)):                      # one running tensor without the other, with a good counter and without one
        for counter in (p, None):
            assert call(counter, rm, rv) == _lib.E_INVAL
            assert lib.fd_last_error()


# ------------------------------------------------------------------------------------------------ optim.update_bn
def _model():
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 64)
    g = torch.Generator().manual_seed(1)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.num_batches_tracked.fill_(11)
    return model


def _bns(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)}


def _snapshot(model):
    return {n: (m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone(), m.momentum, m.training) for n, m in _bns(model).items()}


def _is_reset(m):
    return bool((m.running_mean == 0).all()) and bool((m.running_var == 1).all()) and int(m.num_batches_tracked) == 0


@pytest.mark.parametrize("was_training", [False, True])
def test_update_bn_leaves_the_frozen_backbone_alone(was_training):
    """An empty loader shows what is reset: the FPN BatchNorms (they run on batch statistics under train()) and nothing of the backbone the constructor
    froze -- which the stock function resets to 0 / 1 and never recomputes: the reason optim.update_bn exists."""
    model = _model().train(was_training)
    before = _snapshot(model)
    frozen = {n for n in before if n.startswith("backbone.")}
    assert frozen and len(frozen) < len(before)
    optim.update_bn([], model)
    assert model.training is was_training
    for n, m in _bns(model).items():
        rm, rv, nbt, momentum, training = before[n]
        assert m.momentum == momentum and momentum is not None and m.training is training, n
        if n in frozen:
            assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv) and torch.equal(m.num_batches_tracked, nbt), n
        else:
            assert _is_reset(m), n
    stock = _model().train(was_training)
    torch.optim.swa_utils.update_bn([], stock)
    assert all(_is_reset(m) for n, m in _bns(stock).items() if n in frozen), "the stock function no longer resets the frozen backbone"


def test_update_bn_with_nothing_on_batch_statistics_returns_with_the_mode_restored():
    model = _model()
    model.freeze_all_bn = True
    model.eval()
    before = _snapshot(model)

    def never():
        raise AssertionError("the loader was read")
        yield

    optim.update_bn(never(), model)
    assert model.training is False
    for n, m in _bns(model).items():
        rm, rv, nbt, momentum, training = before[n]
        assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv) and torch.equal(m.num_batches_tracked, nbt), n
        assert m.momentum == momentum and m.training is training


def test_update_bn_leaves_a_folded_efficientnet_stem_alone():
    """FCOS(efficientnet=True, freeze_bn=False).enable_training(batch_stats=True) without train_stem: the stem's _bn0 is in training mode as far as
    nn.Module knows, but the trunk folds it on its running statistics -- it keeps them; with train_stem=True it runs on batch statistics and is reset."""
    import warnings
    from pytorch_object_detection_amd.model.od import FCOS
    for train_stem in (False, True):
        model = FCOS([320, 112, 40], 20, 64, freeze_bn=False, efficientnet=True, backbone_number=0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.enable_training(train_stem=train_stem, batch_stats=True)
        net = model.backbone.model
        for m in (net._bn0, net._blocks[0]._bn1):
            m.running_mean.fill_(0.25), m.running_var.fill_(2.0), m.num_batches_tracked.fill_(5)
        optim.update_bn([], model)
        assert _is_reset(net._blocks[0]._bn1) and net._bn0.momentum is not None and net._blocks[0]._bn1.momentum is not None
        if train_stem:
            assert _is_reset(net._bn0)
        else:
            assert bool((net._bn0.running_mean == 0.25).all()) and bool((net._bn0.running_var == 2.0).all()) and int(net._bn0.num_batches_tracked) == 5


def test_a_forward_that_raises_leaves_momenta_and_mode_restored():
    model = _model().eval()
    before = _snapshot(model)
    versions = {n: m.running_mean._version for n, m in _bns(model).items()}
    with pytest.raises(FdError):                               # a CPU batch: the detector has no CPU path
        optim.update_bn([[torch.zeros(2, 3, 128, 128), "target"]], model)
    assert model.training is False
    for n, m in _bns(model).items():
        assert m.momentum == before[n][3] and m.momentum is not None and m.training is before[n][4], n
        if not n.startswith("backbone."):
            assert m.running_mean._version > versions[n], n   # what it wrote is marked written
        else:
            assert m.running_mean._version == versions[n], n


def test_update_bn_takes_wrappers_and_the_stock_batch_conventions():
    """The signature of the stock function; an nn.Module that only wraps the detector (as DistributedDataParallel and AveragedModel do) is walked through."""
    import inspect
    assert list(inspect.signature(optim.update_bn).parameters) == list(inspect.signature(torch.optim.swa_utils.update_bn).parameters)
    wrapped = torch.optim.swa_utils.AveragedModel(_model())
    src = copy.deepcopy(wrapped)
    optim.update_bn([], wrapped)
    for (n, m), s in zip(_bns(wrapped).items(), _bns(src).values()):
        if ".backbone." in n:
            assert torch.equal(m.running_mean, s.running_mean) and torch.equal(m.running_var, s.running_var), n
        else:
            assert _is_reset(m), n
        assert m.momentum == s.momentum
    # a plain CPU module runs through: tensor batches and [input, target] batches, against the restatement
    net = nn.Sequential(nn.BatchNorm2d(6)).double()
    batches = _batches(seed=2)
    optim.update_bn([[b, None] for b in batches], net)
    am, av, an = CR.update_bn_ref(batches)
    assert int(net[0].num_batches_tracked) == an and net[0].momentum == 0.1
    torch.testing.assert_close(am, net[0].running_mean, rtol=0, atol=1e-12)
    torch.testing.assert_close(av, net[0].running_var, rtol=0, atol=1e-12)
