"""optim.AveragedModel without a GPU: the float64 reference of tests/avg_ref.py against torch.optim.swa_utils.AveragedModel, the gate schedule against a literal
host loop, the C-ABI's struct layouts and argument errors, constructor refusals, the state-dict keys, the new symbols, and copy.deepcopy of a detector."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import avg_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, optim  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402

NEW = ("fd_avg_begin", "fd_avg_update_f32", "fd_avg_copy_bytes")


def _small():
    torch.manual_seed(5)
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Flatten(), nn.Linear(4, 2)).double()


def _perturb(model, gen):
    """What a training step does to the model, as far as averaging can see: new parameters, new running statistics, a larger counter."""
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.3)
        for b in model.buffers():
            if b.is_floating_point():
                b.add_(torch.rand(b.shape, generator=gen, dtype=b.dtype) * 0.2)
            else:
                b.add_(3)


@pytest.mark.parametrize("use_buffers", [False, True], ids=["copy_buffers", "use_buffers"])
@pytest.mark.parametrize("decay", [None, 0.9, 0.999, 0.0, 1.0], ids=["swa", "ema0.9", "ema0.999", "ema0", "ema1"])
def test_reference_is_the_stock_averaged_model_in_float64(decay, use_buffers):
    model, gen = _small(), torch.Generator().manual_seed(11)
    stock = swa_utils.AveragedModel(model, multi_avg_fn=None if decay is None else swa_utils.get_ema_multi_avg_fn(decay), use_buffers=use_buffers)
    ref = avg_ref.RefAveraged(list(model.parameters()), list(model.buffers()), mode=avg_ref.SWA if decay is None else avg_ref.EMA,
                              decay=0.0 if decay is None else decay, use_buffers=use_buffers)
    for k in range(7):
        _perturb(model, gen)
        stock.update_parameters(model)
        assert ref.update(list(model.parameters()), list(model.buffers()))
        assert ref.n_averaged == int(stock.n_averaged) == k + 1
        for a, want in zip(ref.p, [p.detach() for p in stock.module.parameters()]):
            assert float((a - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
        for a, want in zip(ref.b, stock.module.buffers()):
            if want.is_floating_point():
                assert float((a - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
            elif not use_buffers:      # with use_buffers the stock class blends integer buffers through a truncating fallback; ours copies them (not followed)
                assert torch.equal(a, want)
            else:
                assert torch.equal(a, dict(model.named_buffers())["1.num_batches_tracked"])


@pytest.mark.parametrize("start_step,every", [(0, 1), (3, 1), (3, 4), (12, 5)])
def test_gate_schedule_against_a_literal_loop(start_step, every):
    skipped, want, n, seen = (3, 7), [], 0, []
    for g in range(0, 13):
        if g in skipped:
            continue
        if g < start_step:
            continue
        if (g - start_step) % every != 0:
            continue
        want.append(g)
    assert avg_ref.gate_schedule(range(0, 13), start_step, every, skipped) == want
    for g in range(0, 13):           # n_averaged counts the applied calls only, and the weights are the SWA ones
        apply, w, n2 = avg_ref.begin(n, avg_ref.SWA, skip=g in skipped, global_step=g, start_step=start_step, every=every)
        assert apply == (g in want) and n2 == n + int(apply) and w == (1.0 / (n + 1) if apply else 0.0)
        n = n2
        seen.append(apply)
    assert n == len(want)
    assert {(0, 1): 11, (3, 1): 8, (3, 4): 1, (12, 5): 1}[(start_step, every)] == len(want)      # (3, 4): 3 and 7 are the skipped steps, 11 remains


def test_reference_weights_and_copy_case():
    assert avg_ref.begin(0, avg_ref.EMA, decay=0.9) == (True, 1.0, 1) and avg_ref.begin(4, avg_ref.EMA, decay=0.9)[1] == 1.0 - 0.9
    assert avg_ref.begin(4, avg_ref.SWA) == (True, 0.2, 5) and avg_ref.begin(4, avg_ref.SWA, skip=True) == (False, 0.0, 4)
    a, p = torch.tensor([1.0, float("nan"), 3.0], dtype=torch.float64), torch.tensor([2.0, 5.0, 3.0], dtype=torch.float64)
    assert torch.equal(avg_ref.update(a, p, 1.0), p)
    out = avg_ref.update(a, p, 0.25)
    assert out[0] == 1.25 and out[2] == 3.0 and torch.isnan(out[1])


def test_avg_struct_layouts_match_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "fcosdet.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(fd_avg_state), offsetof(fd_avg_state, weight),
        offsetof(fd_avg_state, weight_f32), sizeof(fd_avg_begin_params), offsetof(fd_avg_begin_params, decay), offsetof(fd_avg_begin_params, start_step),
        offsetof(fd_avg_begin_params, every), sizeof(fd_avg_chunk), offsetof(fd_avg_chunk, avg), offsetof(fd_avg_chunk, p), offsetof(fd_avg_chunk, numel),
        sizeof(fd_avg_copy_chunk), offsetof(fd_avg_copy_chunk, src), offsetof(fd_avg_copy_chunk, nbytes), FD_AVG_SWA, FD_AVG_EMA); return 0; }'''
    exe = os.path.join(ROOT, "oracle", "_build", "abi_probe_avg")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    S, B, K, Y = _lib.AvgState, _lib.AvgBeginParams, _lib.AvgChunk, _lib.AvgCopyChunk
    assert vals == [ctypes.sizeof(S), S.weight.offset, S.weight_f32.offset, ctypes.sizeof(B), B.decay.offset, B.start_step.offset, B.every.offset,
                    ctypes.sizeof(K), K.avg.offset, K.p.offset, K.numel.offset, ctypes.sizeof(Y), Y.src.offset, Y.nbytes.offset, _lib.AVG_SWA, _lib.AVG_EMA]
    assert ctypes.sizeof(S) % 16 == 0 and S.apply.offset == 0
    assert ctypes.sizeof(K) == ctypes.sizeof(Y) == 1544              # of the 4 KB kernel-argument segment


def test_avg_abi_argument_errors_without_gpu():
    """Every entry validates on the host before any launch: FD_E_INVAL and a message, no GPU needed."""
    lib = _lib.lib()
    ptr = ctypes.c_void_p(4096)

    def params(**over):
        bp = _lib.AvgBeginParams()
        bp.mode, bp.decay, bp.start_step, bp.every = _lib.AVG_EMA, 0.9, 0, 1
        for k, v in over.items():
            setattr(bp, k, v)
        return bp

    def bad_begin(word, state=ptr, n=ptr, step=ptr, bp=None, **over):
        bp = params(**over) if bp is None else bp
        assert lib.fd_avg_begin(state, n, None, step, ctypes.byref(bp) if bp is not False else None, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    bad_begin(b"null state block", state=None)
    bad_begin(b"null n_averaged", n=None)
    bad_begin(b"null params", bp=False)
    bad_begin(b"mode", mode=2)
    bad_begin(b"mode", mode=-1)
    for d in (-0.001, 1.001, float("nan"), float("inf")):
        bad_begin(b"decay", decay=d)
    bad_begin(b"every", every=0)
    bad_begin(b"global_step", step=None, start_step=3)
    bad_begin(b"global_step", step=None, every=2)

    def chunk(cls, n=1, **over):
        c = cls()
        c.n = n
        a, b, s = [f[0] for f in cls._fields_[2:]]
        for i in range(max(0, min(n, _lib.OPTIM_MAX_TENSORS))):
            getattr(c, a)[i], getattr(c, b)[i], getattr(c, s)[i] = 4096, 8192, 8
        for k, v in over.items():
            getattr(c, k)[0] = v
        return c

    def bad(fn, c, word, state=ptr):
        assert fn(ctypes.byref(c) if c is not None else None, state, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    K, Y = _lib.AvgChunk, _lib.AvgCopyChunk
    for fn, cls, dst, src, size in ((lib.fd_avg_update_f32, K, "avg", "p", "numel"), (lib.fd_avg_copy_bytes, Y, "dst", "src", "nbytes")):
        bad(fn, None, b"null chunk")
        bad(fn, chunk(cls), b"null state block", state=None)
        bad(fn, chunk(cls, 0), b"outside")
        bad(fn, chunk(cls, _lib.OPTIM_MAX_TENSORS + 1), b"outside")
        bad(fn, chunk(cls, **{size: -1}), b"negative")
        bad(fn, chunk(cls, **{dst: None}), b"null")
        bad(fn, chunk(cls, 3, **{src: None}), b"null")
        # legal without a launch: a chunk of empty tensors has nothing to do, and their pointers are not looked at
        empty = chunk(cls, **{dst: None, src: None, size: 0})
        assert fn(ctypes.byref(empty), ptr, None) == 0
    bad(lib.fd_avg_update_f32, chunk(K, avg=4098), b"4-byte aligned")


def test_constructor_refusals():
    model = _small().float()
    opt = optim.SGD(model.parameters(), lr=0.1)
    for kw, name in (({"avg_fn": swa_utils.get_ema_avg_fn(0.9)}, "avg_fn"), ({"multi_avg_fn": swa_utils.get_ema_multi_avg_fn(0.9)}, "multi_avg_fn"),
                     ({"decay": 1.5}, "decay"), ({"decay": -0.1}, "decay"), ({"decay": float("nan")}, "decay"), ({"decay": "0.9"}, "decay"),
                     ({"optimizer": torch.optim.SGD(model.parameters(), lr=0.1)}, "optimizer"), ({"start_step": 3}, "start_step"), ({"every": 2}, "every"),
                     ({"optimizer": opt, "every": 0}, "every"), ({"optimizer": opt, "start_step": 1.5}, "start_step")):
        with pytest.raises(ValueError, match=name):
            optim.AveragedModel(model, **kw)
    avg = optim.AveragedModel(model, decay=0.9, optimizer=opt, start_step=3, every=4, use_buffers=True)
    assert isinstance(avg, swa_utils.AveragedModel) and avg.use_buffers and avg.decay == 0.9 and (avg.start_step, avg.every) == (3, 4)
    assert avg.n_averaged.dtype == torch.int64 and avg.n_averaged.dim() == 0 and int(avg.n_averaged) == 0
    assert avg.module is not model and all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(avg.module.parameters(), model.parameters()))
    bp = avg._begin_params()
    assert (bp.mode, bp.decay, bp.start_step, bp.every) == (_lib.AVG_EMA, 0.9, 3, 4)
    assert optim.AveragedModel(model)._begin_params().mode == _lib.AVG_SWA
    # CPU tensors are refused by update_parameters(): there is no CPU fallback
    with pytest.raises(_lib.FdError, match="GPU only"):
        optim.AveragedModel(model).update_parameters(model)


def test_update_refusals_name_the_model():
    """The pair checks run on the host before any launch (here on CPU tensors, with the device check last in line for them)."""
    model = _small().float()
    avg = optim.AveragedModel(model)
    bigger = nn.Sequential(*list(_small().float()), nn.Linear(2, 2))
    with pytest.raises(ValueError, match="model"):
        avg.update_parameters(bigger)


def test_state_dict_keys_are_the_stock_class():
    model = _small().float()
    ours, stock = optim.AveragedModel(model, decay=0.9), swa_utils.AveragedModel(model, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(0.9))
    sd, want = ours.state_dict(), stock.state_dict()
    assert list(sd) == list(want) and "n_averaged" in sd and all(k == "n_averaged" or k.startswith("module.") for k in sd)
    assert all(sd[k].dtype == want[k].dtype and sd[k].shape == want[k].shape for k in want)
    with torch.no_grad():
        for p in ours.module.parameters():
            p.add_(1.0)
        ours.n_averaged.fill_(5)
    stock.load_state_dict(ours.state_dict())          # both ways
    assert int(stock.n_averaged) == 5 and all(torch.equal(a, b) for a, b in zip(stock.module.parameters(), ours.module.parameters()))
    with torch.no_grad():
        stock.n_averaged.fill_(9)
    ours.load_state_dict(stock.state_dict())
    assert int(ours.n_averaged) == 9


def test_avg_symbols_are_declared_exported_and_built():
    with open(os.path.join(ROOT, "include", "fcosdet.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name), name
    for struct in ("fd_avg_state", "fd_avg_begin_params", "fd_avg_chunk", "fd_avg_copy_chunk"):
        assert "typedef struct " + struct in header, struct
    assert header.index("fd_avg_begin(") > header.index("fd_grad_clip_finish(")          # after the clipping section


def test_deepcopy_of_a_detector_starts_with_empty_plans():
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256)
    model.conv_precision = "f16x3"
    model.backbone.trunk.hip_bn_train = True                      # a plain-attribute switch (enable_trunk_batch_stats sets it)
    sentinel = object()
    model._plans[("model", 1, 64, 64, "cpu", None)] = (0, sentinel)
    model.head._plans[("head",)] = (0, sentinel)
    twin = copy.deepcopy(model)
    assert twin._plans == {} and all(m._plans == {} for m in twin.modules() if hasattr(m, "_plans"))
    assert model._plans[("model", 1, 64, 64, "cpu", None)][1] is sentinel and model.head._plans[("head",)][1] is sentinel     # the source's stay
    assert twin.conv_precision == "f16x3" and twin.backbone.trunk.hip_bn_train is True and twin.backbone_freeze == model.backbone_freeze
    sd, td = model.state_dict(), twin.state_dict()
    assert list(sd) == list(td) and all(torch.equal(sd[k], td[k]) and sd[k].data_ptr() != td[k].data_ptr() for k in sd)
    assert [p.requires_grad for p in twin.parameters()] == [p.requires_grad for p in model.parameters()]
    assert [m.training for m in twin.modules()] == [m.training for m in model.modules()]
    assert type(optim.AveragedModel(model).module) is HalfInvertedStageFCOS
