"""Gradient-norm clipping inside the HIP optimizer step, without a GPU: the float64 restatement of tests/clip_ref.py against torch.nn.utils.clip_grad_norm_, the
C-ABI's struct layouts and argument errors, constructor rejections, the state-dict layout, the Builder's config key and the new symbols."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import clip_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, optim  # noqa: E402
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402

NEW = ("fd_grad_sumsq_slots", "fd_grad_norm_workspace_bytes", "fd_grad_sumsq_f32", "fd_grad_clip_finish")
SHAPES = [(7,), (3, 5), (2, 3, 2, 2), (0,)]


def _grads(norm=None, zero=False):
    gen = torch.Generator().manual_seed(4)
    gs = [torch.zeros(s, dtype=torch.float64) if zero else torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    if norm is not None:
        have = math.sqrt(sum(float((g * g).sum()) for g in gs))
        gs = [g * (norm / have) for g in gs]
    return gs


@pytest.mark.parametrize("case,norm", [("below", 3.0), ("above", 80.0), ("at", 35.0), ("zero", None)])
@pytest.mark.parametrize("scale", [None, 1024.0])
def test_reference_is_torch_clip_grad_norm_in_float64(case, norm, scale):
    max_norm = 35.0
    gs = _grads(norm, zero=case == "zero")
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
    ref = clip_ref.clip([g * scale for g in gs] if scale is not None else gs, max_norm, grad_scale=scale)
    assert not ref.found
    assert abs(ref.total_norm - total) <= 1e-12 * max(total, 1.0)
    if case in ("below", "zero"):
        assert ref.clip_coef == 1.0 and ref.eff_scale == (scale or 1.0)
    if case == "above":
        assert ref.clip_coef < 0.5
    if case == "at":
        assert 1.0 - 1e-7 < ref.clip_coef < 1.0           # the 1e-6 in the denominator: a norm exactly at max_norm is already scaled, as in torch
    # what the update kernels see, g / eff_scale, is what torch left in p.grad
    for p, g in zip(ps, gs):
        mine = (g * scale if scale is not None else g) / ref.eff_scale
        assert float((mine - p.grad).abs().max() if g.numel() else 0.0) <= 1e-12 * max(float(p.grad.abs().max()) if g.numel() else 0.0, 1e-300)
    assert clip_ref.sumsq([None, gs[0]]) == pytest.approx(float((gs[0] * gs[0]).sum()), rel=1e-14)


def test_reference_found_flag():
    gs = _grads(3.0)
    for bad in (float("inf"), float("-inf"), float("nan")):
        g2 = [g.clone() for g in gs]
        g2[1][0, 2] = bad
        r = clip_ref.clip(g2, 35.0, grad_scale=8.0)
        assert r.found and r.clip_coef == 1.0 and r.eff_scale == 8.0 and not math.isfinite(r.sumsq)
    r = clip_ref.clip(gs, 1.0, found_inf=True)
    assert r.found and r.clip_coef == 1.0 and r.eff_scale == 1.0 and math.isfinite(r.total_norm)
    # squares that overflow fp32 are ordinary numbers here
    big = [torch.full((4,), 3e20, dtype=torch.float32), torch.full((5,), -3e20, dtype=torch.float32)]
    r = clip_ref.clip(big, 35.0)
    assert not r.found and r.total_norm == pytest.approx(3.0 * float(torch.tensor(3e20, dtype=torch.float32)), rel=1e-14)


def test_clip_struct_layouts_match_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "fcosdet.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fd_grad_chunk), offsetof(fd_grad_chunk, n), offsetof(fd_grad_chunk, g),
        offsetof(fd_grad_chunk, numel), sizeof(fd_grad_clip), offsetof(fd_grad_clip, sumsq), offsetof(fd_grad_clip, total_norm), offsetof(fd_grad_clip, clip_coef),
        offsetof(fd_grad_clip, eff_scale), offsetof(fd_grad_clip, found), offsetof(fd_grad_clip, total_norm_f32)); return 0; }'''
    exe = os.path.join(ROOT, "oracle", "_build", "abi_probe_clip")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    K, B = _lib.GradChunk, _lib.GradClip
    assert vals == [ctypes.sizeof(K), K.n.offset, K.g.offset, K.numel.offset, ctypes.sizeof(B), B.sumsq.offset, B.total_norm.offset, B.clip_coef.offset,
                    B.eff_scale.offset, B.found.offset, B.total_norm_f32.offset]
    assert ctypes.sizeof(K) + 16 <= 3072 and ctypes.sizeof(B) % 8 == 0      # by value in the kernel arguments; the block is viewed as float64 words


def test_clip_abi_argument_errors_without_gpu():
    """Every entry validates on the host before any launch: FD_E_INVAL and a message, no GPU needed."""
    lib = _lib.lib()
    ptr = ctypes.c_void_p(4096)

    def chunk(n=1, **over):
        c = _lib.GradChunk()
        c.n = n
        for i in range(max(0, min(n, _lib.OPTIM_MAX_TENSORS))):
            c.g[i], c.numel[i] = 4096, 8
        for k, v in over.items():
            getattr(c, k)[0] = v
        return c

    def bad(c, partials=ptr, first=0, word=b""):
        assert lib.fd_grad_sumsq_f32(ctypes.byref(c) if c is not None else None, partials, first, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    bad(None, word=b"null chunk")
    bad(chunk(0), word=b"outside")
    bad(chunk(_lib.OPTIM_MAX_TENSORS + 1), word=b"outside")
    bad(chunk(g=None), word=b"null g")
    bad(chunk(numel=-1), word=b"negative numel")
    bad(chunk(g=4098), word=b"4-byte aligned")
    bad(chunk(), partials=None, word=b"null partials")
    bad(chunk(), first=-1, word=b"first_slot")
    for c in (chunk(0), chunk(g=None), chunk(numel=-1), chunk(g=4098)):
        assert lib.fd_grad_sumsq_slots(ctypes.byref(c)) == -1
    assert lib.fd_grad_sumsq_slots(None) == -1
    # slots: one block per tensor up to 4096 elements, following the chunk's largest tensor; an empty tensor's pointer is not looked at
    assert lib.fd_grad_sumsq_slots(ctypes.byref(chunk(3))) == 3
    assert lib.fd_grad_sumsq_slots(ctypes.byref(chunk(3, g=None, numel=0))) == 3
    assert lib.fd_grad_sumsq_slots(ctypes.byref(chunk(3, numel=4097))) == 6
    most = lib.fd_grad_sumsq_slots(ctypes.byref(chunk(_lib.OPTIM_MAX_TENSORS, numel=2 ** 40)))
    assert lib.fd_grad_norm_workspace_bytes(1) == 8 * most and lib.fd_grad_norm_workspace_bytes(5) == 40 * most
    assert lib.fd_grad_norm_workspace_bytes(0) == 0 and lib.fd_grad_norm_workspace_bytes(-1) == -1

    def bad_finish(partials=ptr, n_slots=4, max_norm=35.0, out=ptr, word=b""):
        assert lib.fd_grad_clip_finish(partials, n_slots, None, None, max_norm, out, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    bad_finish(partials=None, word=b"null partials")
    bad_finish(out=None, word=b"null clip block")
    bad_finish(n_slots=-1, word=b"n_slots")
    for v in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        bad_finish(max_norm=v, word=b"max_norm")


def test_clip_constructor_rejections():
    w = [torch.nn.Parameter(torch.zeros(4))]
    for cls, kw in ((optim.SGD, {"lr": 0.1, "momentum": 0.9}), (optim.Adam, {"lr": 0.1}), (optim.AdamW, {"lr": 0.1})):
        for v in (0, 0.0, -35.0, float("inf"), float("nan"), "35", True):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(w, max_grad_norm=v, **kw)
        opt = cls(w, max_grad_norm=35, **kw)
        assert opt.max_grad_norm == 35.0 and isinstance(opt.max_grad_norm, float)
        assert "max_grad_norm" not in opt.defaults and all("max_grad_norm" not in g for g in opt.param_groups)
        assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.dim() == 0
        plain = cls(w, **kw)
        assert plain.max_grad_norm is None
        with pytest.raises(AttributeError, match="max_grad_norm"):
            plain.grad_norm
    # CPU parameters are refused by step() with the keyword too: there is no CPU fallback
    opt = optim.SGD(w, lr=0.1, max_grad_norm=1.0)
    w[0].grad = torch.ones(4)
    with pytest.raises(_lib.FdError, match="GPU only"):
        opt.step()


@pytest.mark.parametrize("ours,parent,kw", [(optim.SGD, torch.optim.SGD, {"lr": 0.1, "momentum": 0.9}), (optim.Adam, torch.optim.Adam, {"lr": 0.1}),
                                           (optim.AdamW, torch.optim.AdamW, {"lr": 0.1})], ids=["sgd", "adam", "adamw"])
def test_state_dict_with_max_grad_norm_has_the_parents_keys(ours, parent, kw):
    def groups():
        ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))]
        return [{"params": ps[:1]}, {"params": ps[1:], "weight_decay": 0.0}]
    theirs = parent(groups(), **kw)
    for g in theirs.param_groups:
        for p in g["params"]:
            p.grad = torch.ones_like(p)
    theirs.step()
    sd = theirs.state_dict()
    mine = ours(groups(), max_grad_norm=35.0, **kw)
    fresh = mine.state_dict()
    assert set(fresh) == set(sd) and fresh["state"] == {} and [set(g) for g in fresh["param_groups"]] == [set(g) for g in sd["param_groups"]]
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert set(back) == set(sd) and back["param_groups"] == sd["param_groups"]
    assert {i: set(st) for i, st in back["state"].items()} == {i: set(st) for i, st in sd["state"].items()}
    assert mine.max_grad_norm == 35.0


def test_builder_passes_max_grad_norm_when_the_config_has_it():
    cfg = load_config()
    m = Builder(cfg).model_build()
    block = cfg[cfg["model"]["name"]]["optimizer"]
    assert "max_grad_norm" not in block                                  # the shipped configs do not clip
    assert Builder(cfg).opt_build(m, hip=True).max_grad_norm is None
    block["max_grad_norm"] = 35
    for name, cls in (("SGD", optim.SGD), ("Adam", optim.Adam), ("AdamW", optim.AdamW)):
        block["name"] = name
        opt = Builder(cfg).opt_build(m, hip=True)
        assert type(opt) is cls and opt.max_grad_norm == 35.0 and opt._fd_schedule == optim.TrainPyLR(block["lr"])
    block["name"] = "SGD"
    assert type(Builder(cfg).opt_build(m)) is torch.optim.SGD            # the stock optimizer ignores the key
    block["max_grad_norm"] = -1
    with pytest.raises(ValueError, match="max_grad_norm"):
        Builder(cfg).opt_build(m, hip=True)


def test_clip_symbols_are_declared_exported_and_built():
    with open(os.path.join(ROOT, "include", "fcosdet.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name), name
    assert "typedef struct fd_grad_chunk" in header and "typedef struct fd_grad_clip" in header
