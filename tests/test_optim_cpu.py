"""pytorch_object_detection_amd.optim without a GPU: the float64 references of tests/optim_ref.py against torch's own optimizers, the two learning-rate rules at
their boundary steps, the C-ABI's argument errors and struct layouts, constructor rejections and the state-dict layout."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import optim_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, optim  # noqa: E402
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402

PY_STEPS = (1, 2, 499, 500, 501, 502, 20000, 20001, 20002, 50000, 50001, 50002)
NEW_STEPS = PY_STEPS + (0, 119999, 120000, 159999, 160000)


def _inputs(steps=5):
    gen = torch.Generator().manual_seed(3)
    shapes = [(7,), (3, 5), (2, 3, 2, 2)]
    params = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    grads = [[torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes] for _ in range(steps)]
    return params, grads


def _run_torch(make, params, grads):
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = make(ps)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    return [p.detach() for p in ps]


def _close(a, b, rel=1e-12):
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= rel * float(y.abs().max())


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.0, 0.0, False), (0.9, 1e-4, False), (0.9, 1e-4, True)])
def test_sgd_reference_is_torch_sgd_in_float64(momentum, wd, nesterov):
    params, grads = _inputs()
    want = _run_torch(lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov, foreach=False), params, grads)
    ref = optim_ref.RefSGD(params, momentum, wd, nesterov)
    for gs in grads:
        ref.step(gs, 0.05)
    _close(ref.p, want)


@pytest.mark.parametrize("cls,wd,decoupled", [(torch.optim.Adam, 1e-4, False), (torch.optim.AdamW, 1e-2, True)])
def test_adam_reference_is_torch_adam_in_float64(cls, wd, decoupled):
    params, grads = _inputs()
    want = _run_torch(lambda ps: cls(ps, lr=1e-2, weight_decay=wd, foreach=False), params, grads)
    ref = optim_ref.RefAdam(params, weight_decay=wd, decoupled=decoupled)
    for gs in grads:
        ref.step(gs, 1e-2)
    _close(ref.p, want)


def test_reference_skip_unscale_and_applied_count():
    params, grads = _inputs(3)
    a, b = optim_ref.RefAdam(params, weight_decay=1e-4), optim_ref.RefAdam(params, weight_decay=1e-4)
    a.step(grads[0], 1e-2)
    assert not b.step(grads[1], 1e-2, found_inf=True) and b.applied == 0 and all(torch.equal(x, y) for x, y in zip(b.p, params))
    b.step([g * 1024 for g in grads[0]], 1e-2, grad_scale=1024.0)
    assert b.applied == 1
    _close(b.p, a.p)
    c = optim_ref.RefSGD(params, 0.9)
    c.step([grads[0][0], None, grads[0][2]], 0.1)
    assert torch.equal(c.p[1], params[1]) and float(c.buf[1].abs().max()) == 0.0


def test_train_py_lr_at_its_boundary_steps():
    """TrainPyLR.at (closed form) and the reference restatement (the loop) against a literal transcription of the loop body, run from step 1."""
    lr_init, lr, seen = 0.01, 0.01, {}
    for G in range(1, max(PY_STEPS) + 1):
        if G < 501:
            lr = float(G / 501 * lr_init)
        if G == 20001:
            lr = lr_init * 0.1
        if G == 50001:
            lr = lr_init * 0.01
        if G in PY_STEPS:
            seen[G] = lr
    rule = optim.TrainPyLR(lr_init)
    for G in PY_STEPS:
        assert optim_ref.train_py_lr(G, lr_init) == seen[G], G
        assert rule.at(G, lr_init) == seen[G], G
    assert seen[501] == seen[20000] == 500 / 501 * lr_init          # the warm-up never reaches lr_init: the reference's behaviour, kept
    assert seen[20001] == lr_init * 0.1 and seen[50002] == lr_init * 0.01
    assert rule.at(0, 0.3) == 0.3 and optim_ref.train_py_lr(0, lr_init, lr_before=0.3) == 0.3


def test_train_new_lr_at_its_boundary_steps():
    lr_init, sched = 0.01, [120000, 160000]

    def lr_func(step):
        lr = lr_init
        if step < 500:
            alpha = float(step) / 500
            warmup_factor = (1.0 / 3.0) * (1.0 - alpha) + alpha
            lr = lr * warmup_factor
        else:
            for i in range(len(sched)):
                if step < sched[i]:
                    break
                lr *= 0.1
        return float(lr)

    rule = optim.TrainNewLR(lr_init)
    for G in NEW_STEPS:
        assert optim_ref.train_new_lr(G, lr_init) == lr_func(G), G
        assert rule.at(G, 0.5) == lr_func(G), G
    assert lr_func(0) == lr_init * (1.0 / 3.0) and lr_func(160000) == lr_init * 0.1 * 0.1


def test_optim_struct_layouts_match_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "fcosdet.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(fd_optim_state), offsetof(fd_optim_state, lr),
        offsetof(fd_optim_state, applied), offsetof(fd_optim_state, bc2), sizeof(fd_optim_chunk), offsetof(fd_optim_chunk, g), offsetof(fd_optim_chunk, s1),
        offsetof(fd_optim_chunk, numel), sizeof(fd_optim_hyper), offsetof(fd_optim_hyper, momentum), offsetof(fd_optim_hyper, eps),
        sizeof(fd_optim_begin_params), offsetof(fd_optim_begin_params, drop_factor), offsetof(fd_optim_begin_params, lr_ptr),
        offsetof(fd_optim_begin_params, beta2), FD_OPTIM_MAX_TENSORS, FD_OPTIM_MAX_GROUPS, FD_OPTIM_MAX_DROPS); return 0; }'''
    exe = os.path.join(ROOT, "oracle", "_build", "abi_probe_optim")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    S, K, H, B = _lib.OptimState, _lib.OptimChunk, _lib.OptimHyper, _lib.OptimBeginParams
    assert vals == [ctypes.sizeof(S), S.lr.offset, S.applied.offset, S.bc2.offset, ctypes.sizeof(K), K.g.offset, K.s1.offset, K.numel.offset,
                    ctypes.sizeof(H), H.momentum.offset, H.eps.offset, ctypes.sizeof(B), B.drop_factor.offset, B.lr_ptr.offset, B.beta2.offset,
                    _lib.OPTIM_MAX_TENSORS, _lib.OPTIM_MAX_GROUPS, _lib.OPTIM_MAX_DROPS]
    assert ctypes.sizeof(K) + ctypes.sizeof(H) + 16 <= 3072             # well under the 4 KB kernel-argument segment


def test_optim_abi_argument_errors_without_gpu():
    """Every entry validates on the host before any launch: FD_E_INVAL and a message, no GPU needed."""
    lib = _lib.lib()
    ptr, hyper = ctypes.c_void_p(4096), _lib.OptimHyper()

    def chunk(n=1, **over):
        c = _lib.OptimChunk()
        c.n = n
        for i in range(max(0, min(n, _lib.OPTIM_MAX_TENSORS))):
            c.p[i], c.g[i], c.s0[i], c.s1[i], c.numel[i] = 4096, 4096, 4096, 4096, 8
        for k, v in over.items():
            getattr(c, k)[0] = v
        return c

    def bad(fn, c, h=hyper, state=ptr, word=b""):
        assert fn(ctypes.byref(c), ctypes.byref(h), state, None, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    for fn in (lib.fd_optim_sgd_f32, lib.fd_optim_adam_f32):
        bad(fn, chunk(0), word=b"outside")
        bad(fn, chunk(_lib.OPTIM_MAX_TENSORS + 1), word=b"outside")
        bad(fn, chunk(p=None), word=b"null p / g")
        bad(fn, chunk(g=None), word=b"null p / g")
        bad(fn, chunk(numel=-1), word=b"negative numel")
        bad(fn, chunk(), state=None, word=b"null state block")
        h = _lib.OptimHyper()
        h.group = _lib.OPTIM_MAX_GROUPS
        bad(fn, chunk(), h=h, word=b"group")
    with_momentum = _lib.OptimHyper()
    with_momentum.momentum = 0.9
    bad(lib.fd_optim_sgd_f32, chunk(s0=None), h=with_momentum, word=b"null s0")
    bad(lib.fd_optim_adam_f32, chunk(s0=None), word=b"null s0")
    bad(lib.fd_optim_adam_f32, chunk(s1=None), word=b"null s1")
    # legal without a launch: plain SGD needs no state pointer, and a chunk of empty tensors has nothing to do (their pointers are not looked at)
    empty = chunk(p=None, g=None, numel=0)
    assert lib.fd_optim_sgd_f32(ctypes.byref(empty), ctypes.byref(hyper), ptr, None, None) == 0
    bp = _lib.OptimBeginParams()
    bp.n_groups = 1
    assert lib.fd_optim_begin(None, None, ctypes.byref(bp), None) == _lib.E_INVAL and b"null state block" in lib.fd_last_error()
    assert lib.fd_optim_begin(ptr, None, None, None) == _lib.E_INVAL
    bp.n_groups = _lib.OPTIM_MAX_GROUPS + 1
    assert lib.fd_optim_begin(ptr, None, ctypes.byref(bp), None) == _lib.E_INVAL and b"n_groups" in lib.fd_last_error()
    bp.n_groups, bp.rule = 1, 7
    assert lib.fd_optim_begin(ptr, None, ctypes.byref(bp), None) == _lib.E_INVAL and b"rule" in lib.fd_last_error()
    bp.rule, bp.n_drops = _lib.OPTIM_LR_TRAIN_PY, _lib.OPTIM_MAX_DROPS + 1
    assert lib.fd_optim_begin(ptr, None, ctypes.byref(bp), None) == _lib.E_INVAL and b"n_drops" in lib.fd_last_error()


def test_constructor_rejections():
    w = [torch.nn.Parameter(torch.zeros(4))]
    for kw, name in (({"dampening": 0.1}, "dampening"), ({"maximize": True}, "maximize"), ({"differentiable": True}, "differentiable")):
        with pytest.raises(ValueError, match=name):
            optim.SGD(w, lr=0.1, momentum=0.9, **kw)
    for cls in (optim.Adam, optim.AdamW):
        for kw, name in (({"amsgrad": True}, "amsgrad"), ({"maximize": True}, "maximize"), ({"differentiable": True}, "differentiable")):
            with pytest.raises(ValueError, match=name):
                cls(w, lr=0.1, **kw)
    with pytest.raises(ValueError, match="params"):
        optim.SGD([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError, match="params"):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))], lr=0.1)
    with pytest.raises(ValueError, match="lr_schedule"):
        optim.SGD(w, lr=0.1, lr_schedule=lambda s: 0.1)
    with pytest.raises(ValueError, match="param_groups"):
        optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(_lib.OPTIM_MAX_GROUPS + 1)], lr=0.1)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="one device"):
            optim.SGD([torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4, device="cuda"))], lr=0.1)
    # CPU parameters are refused by step(): there is no CPU fallback
    opt = optim.SGD(w, lr=0.1)
    w[0].grad = torch.ones(4)
    with pytest.raises(_lib.FdError, match="GPU only"):
        opt.step()
    assert isinstance(opt, torch.optim.SGD) and isinstance(optim.AdamW(w), torch.optim.AdamW) and isinstance(optim.AdamW(w), torch.optim.Adam)
    assert optim.AdamW(w).defaults["decoupled_weight_decay"] and not optim.Adam(w).defaults["decoupled_weight_decay"]
    assert all(getattr(c, "_step_supports_amp_scaling") for c in (optim.SGD, optim.Adam, optim.AdamW))


def _stepped(cls, n=2, **kw):
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    opt = cls([{"params": ps[:1]}, {"params": ps[1:], "weight_decay": 0.0}], **kw)
    for _ in range(n):
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
    return opt


@pytest.mark.parametrize("ours,parent,kw", [(optim.SGD, torch.optim.SGD, {"lr": 0.1, "momentum": 0.9}), (optim.Adam, torch.optim.Adam, {"lr": 0.1}),
                                           (optim.AdamW, torch.optim.AdamW, {"lr": 0.1})], ids=["sgd", "adam", "adamw"])
def test_state_dict_layout_is_the_parents(ours, parent, kw):
    """A checkpoint of the parent loads, and what state_dict() gives back has the parent's keys, types and values (Adam's `step` included)."""
    sd = _stepped(parent, **kw).state_dict()
    ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]
    mine = ours([{"params": ps[:1]}, {"params": ps[1:], "weight_decay": 0.0}], **kw)
    fresh = mine.state_dict()
    assert fresh["state"] == {} and [set(g) for g in fresh["param_groups"]] == [set(g) for g in sd["param_groups"]]
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert set(back) == set(sd) and back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"])
    for idx, st in sd["state"].items():
        assert set(back["state"][idx]) == set(st)
        for k, v in st.items():
            b = back["state"][idx][k]
            assert type(b) is type(v) and b.dtype == v.dtype and b.shape == v.shape and torch.equal(b, v), (idx, k)
    # the parent takes it back
    again = _stepped(parent, n=0, **kw)
    again.load_state_dict(back)
    assert again.state_dict()["state"].keys() == sd["state"].keys()


def test_adam_load_refuses_step_counts_that_disagree_within_a_group():
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3))]
    opt = torch.optim.Adam(ps, lr=0.1)
    ps[0].grad = torch.randn(5)
    opt.step()                                  # parameter 0: one step
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()                                  # parameter 0: two steps, parameter 1: one
    with pytest.raises(ValueError, match="step"):
        optim.Adam([torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3))], lr=0.1).load_state_dict(opt.state_dict())


def test_scheduled_lr_is_a_tensor_of_the_state_block():
    w = [torch.nn.Parameter(torch.zeros(4))]
    opt = optim.SGD(w, lr=0.01, momentum=0.9, lr_schedule=optim.TrainPyLR(0.01))
    lr = opt.param_groups[0]["lr"]
    assert isinstance(lr, torch.Tensor) and lr.dtype == torch.float64 and lr.dim() == 0 and lr.item() == 0.01
    assert int(opt.global_step) == 0 and int(optim.Adam(w, lr_schedule=optim.TrainNewLR(0.01)).global_step) == -1
    opt.set_global_step(20001)
    assert int(opt.global_step) == 20001 and opt.param_groups[0]["lr"].item() == 0.01 * 0.1
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lr"].item() == 0.01 * 0.1 and sd["param_groups"][0]["lr"].data_ptr() != lr.data_ptr()
    opt.set_global_step(3)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"].data_ptr() == lr.data_ptr() and lr.item() == 0.01 * 0.1


def test_builder_hands_out_the_hip_optimizers_on_request():
    cfg = load_config()
    m = Builder(cfg).model_build()
    opt = Builder(cfg).opt_build(m, hip=True)
    block = cfg[cfg["model"]["name"]]["optimizer"]
    assert isinstance(opt, optim.SGD) and isinstance(opt, torch.optim.SGD) and opt.defaults["weight_decay"] == block["weight_decay"]
    assert opt._fd_schedule == optim.TrainPyLR(block["lr"])
    assert type(Builder(cfg).opt_build(m)) is torch.optim.SGD
    for name, cls in (("Adam", optim.Adam), ("AdamW", optim.AdamW)):
        block["name"] = name
        assert type(Builder(cfg).opt_build(m, hip=True)) is cls
    block["name"] = "RAdam"
    assert isinstance(Builder(cfg).opt_build(m), torch.optim.RAdam)
    with pytest.raises(NotImplementedError):
        Builder(cfg).opt_build(m, hip=True)
