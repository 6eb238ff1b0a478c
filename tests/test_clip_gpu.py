"""Gradient-norm clipping inside the HIP optimizer step, on the GPU: the sum-of-squares kernel at every size / alignment path and across the chunk boundary,
non-finite gradients at the places a kernel can lose them, the step with and without an active clip against the float64 references (tests/clip_ref.py for
the clip block, tests/optim_ref.py for the update rules), chunking over two param groups, graph capture and the model step under GradScaler.

Bounds.  The norm: fp64 accumulation of at most 1e8 exact squares loses far less than the final rounding to fp32, so total_norm_f32 is within 1 fp32 ulp of
the float64 value and sumsq within 1e-12 of it.  The updated tensors: the rule of tests/test_optim_gpu.py -- the stock sequence (unscale, torch.nn.utils.
clip_grad_norm_, torch's optimizer of the same name) runs on the same device and inputs, its largest deviation from float64 is taken per tensor in units of
max|reference|, and ours must stay within twice that with a floor of 4 fp32 ulps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import clip_ref  # noqa: E402
import optim_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, ops, optim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1234.5
ULP4 = 4 * 2.0 ** -23
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4097, 65537, 2 ** 20 + 3, 0)
BIG = 2 ** 20 + 3
_C = _lib.GradClip


class Bank:
    """Tensors carved out of one sentinel-filled fp32 buffer.  Slot i holds `numel` elements starting `off` elements (0..3) past a 16-byte boundary, with at
    least four sentinel words on either side."""

    def __init__(self, specs, dev=DEV):
        pos, self.ranges = 0, []
        for n, off in specs:
            a = pos + 4 + off
            self.ranges.append((a, a + n))
            pos = (a + n + 4 + 3) // 4 * 4
        self.flat = torch.full((pos + 4,), SENT, dtype=torch.float32, device=dev)
        assert self.flat.data_ptr() % 16 == 0

    def view(self, i):
        a, b = self.ranges[i]
        return self.flat[a:b]

    def fill(self, values):
        """values: one flat tensor holding every slot's elements in slot order."""
        pos = 0
        for a, b in self.ranges:
            self.flat[a:b] = values[pos:pos + b - a]
            pos += b - a

    def views(self):
        return [self.view(i) for i in range(len(self.ranges))]

    def assert_sentinels(self, what):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for a, b in self.ranges:
            keep[a:b] = False
        assert bool((self.flat[keep] == SENT).all()), f"{what}: a word outside the tensors was written"


def _block(clip):
    """The clip block (a float64 device tensor laid out as fd_grad_clip) -> its fields on the host."""
    d, f = clip.cpu(), clip.view(torch.float32).cpu()
    return dict(sumsq=float(d[_C.sumsq.offset // 8]), total_norm=float(d[_C.total_norm.offset // 8]), clip_coef=float(d[_C.clip_coef.offset // 8]),
                eff_scale=np.float32(f[_C.eff_scale.offset // 4].item()), found=float(f[_C.found.offset // 4]),
                norm32=np.float32(f[_C.total_norm_f32.offset // 4].item()))


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32).clone()


def _within_ulp(got, want64, ulps=1):
    want = np.float32(want64)
    return abs(float(got) - float(want)) <= ulps * float(np.spacing(np.abs(want)))


def _norm_launches(views, max_norm=35.0, grad_scale=None):
    """ops.grad_sumsq + ops.grad_clip_finish over a list of views with a workspace of exactly the documented size, poisoned with NaN beforehand (the launches
    must write every slot they later read).  -> (clip block tensor, launches)."""
    chunks = -(-len(views) // _lib.OPTIM_MAX_TENSORS)
    partials = torch.full((_lib.lib().fd_grad_norm_workspace_bytes(chunks) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    clip = torch.zeros(ctypes.sizeof(_C) // 8, dtype=torch.float64, device=DEV)
    n, slots = ops.grad_sumsq([v.data_ptr() for v in views], [v.numel() for v in views], partials)
    ops.grad_clip_finish(partials, slots, grad_scale, None, max_norm, clip)
    return clip, n


def _norm_specs(count):
    if count == "sizes":                                   # every size at every offset: 48 tensors
        return [(n, off) for n in SIZES for off in range(4)]
    return [(SIZES[i % len(SIZES)], (i // len(SIZES) + i) % 4) for i in range(count)]


@pytest.mark.parametrize("count", ["sizes", 1, 64, 65, 129])
def test_sumsq_kernel_against_float64(count):
    specs = _norm_specs(count)
    torch.manual_seed(21)
    bank = Bank(specs)
    values = torch.randn(sum(n for n, _ in specs), device=DEV)
    bank.fill(values)
    views = bank.views()
    assert all(v.data_ptr() % 16 == 4 * off for v, (n, off) in zip(views, specs) if n)
    clip, launches = _norm_launches(views)
    again, _ = _norm_launches(views)
    got = _block(clip)
    want = clip_ref.clip(views, 35.0)
    print(f"sumsq {count}: sumsq {got['sumsq']!r} (float64 {want.sumsq!r}), norm {got['norm32']!r} (float64 {want.total_norm!r})")
    assert launches == -(-len(specs) // _lib.OPTIM_MAX_TENSORS)
    assert abs(got["sumsq"] - want.sumsq) <= 1e-12 * want.sumsq
    assert _within_ulp(got["norm32"], want.total_norm) and abs(got["total_norm"] - want.total_norm) <= 1e-12 * want.total_norm
    assert got["found"] == 0.0 and abs(got["clip_coef"] - want.clip_coef) <= 1e-12 and _within_ulp(got["eff_scale"], want.eff_scale)
    if want.clip_coef == 1.0:
        assert got["clip_coef"] == 1.0 and got["eff_scale"] == np.float32(1.0)
    assert torch.equal(_bits(clip), _bits(again)), "two runs on the same inputs differ"
    bank.assert_sentinels("sumsq")
    assert torch.equal(torch.cat(views), values), "a gradient was written"


def test_sumsq_of_elements_whose_squares_overflow_fp32():
    specs = [(1023, 1), (4097, 0), (5, 3)]
    bank = Bank(specs)
    total = sum(n for n, _ in specs)
    sign = torch.where(torch.arange(total, device=DEV) % 3 == 0, -1.0, 1.0)
    bank.fill(sign * 3e20)
    scale = torch.tensor(1024.0, device=DEV)
    clip, _ = _norm_launches(bank.views(), max_norm=35.0, grad_scale=scale)
    got, want = _block(clip), clip_ref.clip(bank.views(), 35.0, grad_scale=1024.0)
    assert float((bank.view(0) * bank.view(0)).sum()) == float("inf")           # what an fp32 accumulator returns
    assert np.isfinite(got["norm32"]) and got["found"] == 0.0
    assert abs(got["sumsq"] - want.sumsq) <= 1e-12 * want.sumsq and _within_ulp(got["norm32"], want.total_norm)
    assert _within_ulp(got["eff_scale"], want.eff_scale) and abs(got["clip_coef"] - want.clip_coef) <= 1e-12 * want.clip_coef


# ---------------------------------------------------------------------------------------------------------------------------------------
# the step
RULES = {
    "sgd-momentum": dict(kind="sgd", momentum=0.9, weight_decay=1e-4, nesterov=False),
    "sgd-nesterov": dict(kind="sgd", momentum=0.9, weight_decay=1e-4, nesterov=True),
    "adam": dict(kind="adam", weight_decay=1e-4),
    "adamw": dict(kind="adamw", weight_decay=1e-2),
}


def _make(rule, params, lr, ours, **kw):
    r = dict(RULES[rule])
    kind = r.pop("kind")
    mod = optim if ours else torch.optim
    cls = {"sgd": mod.SGD, "adam": mod.Adam, "adamw": mod.AdamW}[kind]
    return cls(params, lr=lr, **r, **kw)


def _make_ref(rule, params):
    r = dict(RULES[rule])
    kind = r.pop("kind")
    if kind == "sgd":
        return optim_ref.RefSGD(params, **r)
    return optim_ref.RefAdam(params, weight_decay=r["weight_decay"], decoupled=kind == "adamw")


def _state_names(rule):
    return ("momentum_buffer",) if RULES[rule]["kind"] == "sgd" else ("exp_avg", "exp_avg_sq")


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).double().cpu().numpy()


def _starts(ts):
    return np.cumsum([0] + [t.numel() for t in ts[:-1]])


def _seg_max(a, starts):
    return np.maximum.reduceat(np.abs(a), starts)


def _assert_within_measured(ours, theirs, ref, starts, what, scale=None):
    """ours / theirs / ref: flat float64 arrays, segments starting at `starts`.  -> (largest deviation of the stock sequence, of ours), in units of max|ref|
    per tensor (`scale` replaces max|ref| for a state tensor: its rounding errors are ulps of the largest gradient term, whatever the sum cancels to)."""
    scale = np.maximum(_seg_max(ref, starts) if scale is None else scale, 1e-30)
    d_t, d_o = _seg_max(theirs - ref, starts) / scale, _seg_max(ours - ref, starts) / scale
    bound = np.maximum(2 * d_t, ULP4)
    worst = int(np.argmax(d_o - bound))
    print(f"{what}: stock deviates by up to {d_t.max():.3e}, ours by up to {d_o.max():.3e} of max|reference| per tensor ({len(starts)} tensors)")
    assert (d_o <= bound).all(), f"{what}: tensor {worst} deviates by {d_o[worst]:.3e}, stock by {d_t[worst]:.3e} (bound {bound[worst]:.3e})"
    return float(d_t.max()), float(d_o.max())


def _stock_step(t_params, t_opt, grads, scale, max_norm):
    """The sequence a user runs today: unscale (GradScaler multiplies by the reciprocal), clip in place, torch's optimizer."""
    for p, g in zip(t_params, grads):
        p.grad = None if g is None else g.clone()
        if g is not None and scale is not None:
            p.grad.mul_(1.0 / scale)
    torch.nn.utils.clip_grad_norm_(t_params, max_norm)
    t_opt.step()


NF_N = 70          # tensors: more than one chunk, the one-element tensors sort last and land in the second
NF_SPECS = [(BIG, 1), (4097, 2), (1023, 3), (257, 0)] + [(1 + i % 5, i % 4) for i in range(NF_N - 4 - 3)] + [(1, 0), (1, 1), (1, 3)]


def _nf_positions():
    """(tensor, element) of the places a kernel can lose a non-finite value."""
    head_big = (4 - 1) % 4
    return {
        "head": (0, 0),                                              # first of the 3 head elements of the tensor that starts 4 bytes past a boundary
        "tail": (1, 4097 - 1),                                       # offset 2: head 2, 1023 vectors, 3 tail elements
        "last-vector": (0, head_big + ((BIG - head_big) // 4) * 4 - 1),  # the last element of the last 16-byte load of the 2^20 + 3 tensor
        "one-element-second-chunk": (NF_N - 1, 0),
    }


@pytest.fixture(scope="module")
def nf_data():
    gen = torch.Generator(device=DEV).manual_seed(31)
    total = sum(n for n, _ in NF_SPECS)
    p0 = torch.randn(total, device=DEV, generator=gen)
    grads = [torch.randn(total, device=DEV, generator=gen) for _ in range(3)]
    return p0, grads


def _nf_run(p0, feeds, scaler_style, found_flags):
    """One optimizer over NF_SPECS whose gradients are Bank views; feeds: flat gradient tensors (unscaled); found_flags: found_inf per step (scaler_style)."""
    bank = Bank(NF_SPECS)
    pos, params = 0, []
    for n, _ in NF_SPECS:
        params.append(torch.nn.Parameter(p0[pos:pos + n].clone()))
        pos += n
    opt = optim.SGD(params, lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=35.0)
    for i, p in enumerate(params):
        p.grad = bank.view(i)
    scale = 1024.0 if scaler_style else None
    if scaler_style:
        opt.grad_scale, opt.found_inf = torch.tensor(scale, device=DEV), torch.zeros((), device=DEV)
    trace = []
    for g, flag in zip(feeds, found_flags):
        bank.fill(g * scale if scaler_style else g)
        if scaler_style:
            opt.found_inf.fill_(flag)
        before = [p.detach().clone() for p in params] + [s.clone() for p in params for s in opt.state[p].values()]
        opt.step()
        after = [p.detach() for p in params] + [s for p in params for s in opt.state[p].values()]
        same = len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
        trace.append(dict(block=_block(opt._fd_clip), unchanged=same, global_step=int(opt.global_step), applied=int(opt._applied(0))))
    bank.assert_sentinels("gradients")
    return params, opt, trace


@pytest.fixture(scope="module")
def nf_twins(nf_data):
    """The optimizers that never saw the bad step: two finite steps, per scaler style."""
    p0, grads = nf_data
    return {s: _nf_run(p0, [grads[0], grads[2]], s, [0.0, 0.0]) for s in (False, True)}


def _nf_check(run, twin):
    params, opt, trace = run
    t_params, t_opt, t_trace = twin
    assert [t["block"]["found"] for t in trace] == [0.0, 1.0, 0.0]
    bad = trace[1]
    assert bad["unchanged"], "a skipped step wrote a parameter or a state tensor"
    assert bad["block"]["clip_coef"] == 1.0 and np.isfinite(bad["block"]["eff_scale"])
    assert [t["global_step"] for t in trace] == [1, 2, 3] and [t["applied"] for t in trace] == [1, 1, 2]
    assert not trace[0]["unchanged"] and not trace[2]["unchanged"]
    # the next finite step is the next step of the run that never saw the bad one, bit for bit
    for a, b in zip(params, t_params):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(opt.state[a]["momentum_buffer"], t_opt.state[b]["momentum_buffer"])
    assert trace[2]["block"] == t_trace[1]["block"]


@pytest.mark.parametrize("scaler_style", [False, True], ids=["no-scaler", "found_inf-tensor"])
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["head", "tail", "last-vector", "one-element-second-chunk"])
def test_non_finite_gradient_skips_the_step(nf_data, nf_twins, where, value, scaler_style):
    p0, grads = nf_data
    tensor, elem = _nf_positions()[where]
    flat_index = sum(n for n, _ in NF_SPECS[:tensor]) + elem
    poisoned = grads[1].clone()
    poisoned[flat_index] = value
    run = _nf_run(p0, [grads[0], poisoned, grads[2]], scaler_style, [0.0, 0.0, 0.0])
    assert not np.isfinite(run[2][1]["block"]["sumsq"])
    _nf_check(run, nf_twins[scaler_style])


def test_found_inf_alone_skips_the_step(nf_data, nf_twins):
    p0, grads = nf_data
    run = _nf_run(p0, grads, True, [0.0, 1.0, 0.0])
    blk = run[2][1]["block"]
    assert np.isfinite(blk["sumsq"]) and blk["eff_scale"] == np.float32(1024.0)          # nothing but the plain scale is published
    _nf_check(run, nf_twins[True])


SHAPES = [(3,), (17, 5), (4, 4, 3, 3), (1,), (1030,), (257,)]


def _twin_params(seed=5):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in SHAPES]


@pytest.mark.parametrize("scale", [None, 1024.0], ids=["unscaled", "scale1024"])
@pytest.mark.parametrize("rule", ["sgd-momentum", "adam"])
def test_a_norm_below_max_norm_changes_nothing(rule, scale):
    """clip_coef == 1 publishes the scale bit for bit: three steps are those of an optimizer built without the keyword."""
    a, b = _twin_params(), _twin_params()
    oa, ob = _make(rule, a, 0.05, ours=True, max_grad_norm=1e4), _make(rule, b, 0.05, ours=True)
    for o in (oa, ob):
        if scale is not None:
            o.grad_scale, o.found_inf = torch.tensor(scale, device=DEV), torch.zeros((), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(6)
    for _ in range(3):
        gs = [torch.randn(p.shape, device=DEV, generator=gen) * (scale or 1.0) for p in a]
        for ps, o in ((a, oa), (b, ob)):
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            o.step()
        blk = _block(oa._fd_clip)
        assert blk["clip_coef"] == 1.0 and blk["eff_scale"] == np.float32(scale or 1.0) and blk["found"] == 0.0
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        for name in _state_names(rule):
            assert torch.equal(oa.state[p][name], ob.state[q][name])
    assert torch.equal(oa._fd_state_i, ob._fd_state_i)
    assert oa.launches == ob.launches + 2 and ob.launches == 2                          # one sum-of-squares launch and the finish launch


@pytest.mark.parametrize("mode", ["above", "at"])
@pytest.mark.parametrize("scale", [None, 1024.0], ids=["unscaled", "scale1024"])
@pytest.mark.parametrize("rule", list(RULES))
def test_clipped_steps_against_float64(rule, scale, mode):
    """above: five steps whose norm (about 50) is far above max_norm = 1.  at: one step whose norm is max_norm to within an fp32 ulp, where the 1e-6 of the
    coefficient's denominator decides."""
    max_norm, lr = 1.0, 0.05 if RULES[rule]["kind"] == "sgd" else 1e-2
    params = _twin_params()
    opt = _make(rule, params, lr, ours=True, max_grad_norm=max_norm)
    if scale is not None:
        opt.grad_scale, opt.found_inf = torch.tensor(scale, device=DEV), torch.zeros((), device=DEV)
    t_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    t_opt = _make(rule, t_params, lr, ours=False)
    ref = _make_ref(rule, params)
    starts = _starts(params)
    g_max = np.zeros(len(params))
    gen = torch.Generator(device=DEV).manual_seed(8)
    for step in range(5 if mode == "above" else 1):
        gs = [torch.randn(p.shape, device=DEV, generator=gen) for p in params]
        if mode == "at":
            have = np.sqrt(clip_ref.sumsq(gs))
            gs = [(g.double() * (max_norm / have)).float() for g in gs]
        scaled = [g * scale for g in gs] if scale is not None else gs            # a power of two: exact
        want = clip_ref.clip(scaled, max_norm, grad_scale=scale)
        assert (want.clip_coef < 0.05) if mode == "above" else (abs(want.total_norm - max_norm) <= 2.0 ** -23 and want.clip_coef < 1.0)
        for p, g in zip(params, scaled):
            p.grad = g.clone()
        opt.step()
        _stock_step(t_params, t_opt, scaled, scale, max_norm)
        ref.step(scaled, lr, grad_scale=want.eff_scale)
        g_max = np.maximum(g_max, _seg_max(_flat(gs), starts) * want.clip_coef)
        blk = _block(opt._fd_clip)
        assert _within_ulp(float(opt.grad_norm), want.total_norm) and blk["norm32"] == np.float32(float(opt.grad_norm))
        assert abs(blk["clip_coef"] - want.clip_coef) <= 1e-12 and _within_ulp(blk["eff_scale"], want.eff_scale) and blk["found"] == 0.0
        for p, g in zip(params, scaled):
            assert torch.equal(p.grad, g), "p.grad was written"
    tag = f"clip {mode} {rule} {'scale1024' if scale else 'unscaled'}"
    _assert_within_measured(_flat(params), _flat(t_params), _flat(ref.p), starts, f"{tag} p")
    for k, name in enumerate(_state_names(rule)):
        _assert_within_measured(_flat([opt.state[p][name] for p in params]), _flat([t_opt.state[p][name] for p in t_params]), _flat(ref.state()[k]), starts,
                                f"{tag} {name}", scale=g_max ** 2 if name == "exp_avg_sq" else g_max)


def test_one_global_norm_over_two_groups_with_missing_gradients():
    torch.manual_seed(7)
    sizes = [1 + i % 7 for i in range(300)] + [65537]
    params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in sizes]
    no_grad, frozen, empty, cut = 150, 151, 152, 170
    params[frozen].requires_grad_(False)
    params[empty] = torch.nn.Parameter(torch.zeros(0, device=DEV))
    other = {"lr": 0.01, "weight_decay": 1e-2, "momentum": 0.5}
    max_norm = 2.0
    opt = optim.SGD([{"params": params[:cut]}, dict(params=params[cut:], **other)], lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=max_norm)
    t_params = [torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in params]
    t_opt = torch.optim.SGD([{"params": t_params[:cut]}, dict(params=t_params[cut:], **other)], lr=0.05, momentum=0.9, weight_decay=1e-4)
    refs = [optim_ref.RefSGD(params[:cut], 0.9, 1e-4), optim_ref.RefSGD(params[cut:], 0.5, 1e-2)]
    grads = [None if i in (no_grad, frozen) else torch.randn_like(p) for i, p in enumerate(params)]
    for p, g in zip(params, grads):
        p.grad = g
    before = [params[i].detach().clone() for i in (no_grad, frozen)]
    opt.step()
    _stock_step(t_params, t_opt, grads, None, max_norm)
    want = clip_ref.clip(grads, max_norm)
    assert want.clip_coef < 0.05                                        # one norm over both groups (about 260), far above max_norm
    refs[0].step(grads[:cut], 0.05, grad_scale=want.eff_scale)
    refs[1].step(grads[cut:], 0.01, grad_scale=want.eff_scale)
    # live gradients: 168 in group 0, 131 in group 1 (the empty tensor among them): 5 sum-of-squares launches over the 299, the finish launch, the begin
    # launch, 3 + 3 update launches
    live_0, live_1 = cut - 2, len(params) - cut
    cap = _lib.OPTIM_MAX_TENSORS
    assert opt.launches == -(-(live_0 + live_1) // cap) + 1 + 1 + -(-live_0 // cap) + -(-live_1 // cap) == 13
    assert _within_ulp(float(opt.grad_norm), want.total_norm)
    for i, b in zip((no_grad, frozen), before):
        assert torch.equal(params[i].detach(), b) and len(opt.state[params[i]]) == 0
    live = [i for i in range(len(params)) if i != empty]
    _assert_within_measured(_flat([params[i] for i in live]), _flat([t_params[i] for i in live]), _flat([(refs[0].p + refs[1].p)[i] for i in live]),
                            _starts([params[i] for i in live]), "two groups, clipped p")
    assert int(opt._applied(0)) == 1 and int(opt._applied(1)) == 1


def test_max_grad_norm_set_after_construction_is_refused():
    """The clip block is allocated by the constructor: switching clipping on afterwards is refused by step() before any launch."""
    w = torch.nn.Parameter(torch.ones(8, device=DEV))
    w.grad = torch.ones(8, device=DEV)
    opt = optim.SGD([w], lr=0.1)
    opt.max_grad_norm = 1.0
    with pytest.raises(_lib.FdError, match="constructor"):
        opt.step()
    assert int(opt.global_step) == 0 and torch.equal(w.detach(), torch.ones(8, device=DEV))
    opt.max_grad_norm = None
    opt.step()
    assert int(opt.global_step) == 1


def test_captured_clipped_step_replays_like_eager_calls():
    """One step() of SGD + TrainPyLR + max_grad_norm captured after an eager step, replayed six times with other gradients, one of them holding an inf:
    parameters, state, the state block and the clip block are those of six eager calls, bit for bit."""
    sizes = (1, 2, 3, 5, 8, 13, 64, 100, 255, 256, 257, 1031)

    def twin():
        torch.manual_seed(9)
        params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in sizes]
        opt = _make("sgd-momentum", params, 0.01, ours=True, lr_schedule=optim.TrainPyLR(0.01), max_grad_norm=5.0)
        opt.set_global_step(497)                      # the replays cross the end of the warm-up
        for p in params:
            p.grad = torch.zeros_like(p)
        opt.grad_scale, opt.found_inf = torch.full((), 4.0, device=DEV), torch.zeros((), device=DEV)
        src = [torch.zeros_like(p) for p in params]

        def body():
            for p, s in zip(params, src):
                p.grad.copy_(s)
            opt.step()
        return params, opt, src, body

    gen = torch.Generator(device=DEV).manual_seed(2)
    feeds = [[torch.randn(n, device=DEV, generator=gen) * 4.0 for n in sizes] for _ in range(7)]
    feeds[3][9][17] = float("inf")
    feeds[5] = [f * 1e-3 for f in feeds[5]]           # one step below max_norm: the coefficient is 1 there

    def feed(src, k):
        for s, f in zip(src, feeds[k]):
            s.copy_(f)

    pe, oe, se, body_e = twin()
    pg, og, sg, body_g = twin()
    for src, body in ((se, body_e), (sg, body_g)):      # one eager step each: the state tensors exist before the capture
        feed(src, 0)
        body()
    found_e, coef_e = [], []
    for k in range(1, 7):
        feed(se, k)
        body_e()
        blk = _block(oe._fd_clip)
        found_e.append(blk["found"])
        coef_e.append(blk["clip_coef"])
    assert found_e == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0] and coef_e[4] == 1.0 and all(c < 1.0 for c in coef_e[:2] + coef_e[3:4] + coef_e[5:])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body_g()
    for k in range(1, 7):
        feed(sg, k)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(oe.state[a]["momentum_buffer"], og.state[b]["momentum_buffer"])
    assert torch.equal(oe._fd_state_i, og._fd_state_i)
    assert torch.equal(_bits(oe._fd_clip), _bits(og._fd_clip))
    assert int(og.global_step) == 497 + 7 and int(og._applied(0)) == 6
    assert og.param_groups[0]["lr"].item() == optim_ref.train_py_lr(504, 0.01)


def test_model_step_with_clipping_under_gradscaler():
    """The tiny model, batch and step function of test_optim_gpu's model step, with torch.amp.GradScaler and a max_grad_norm small enough to clip: four steps,
    finite losses, and opt.grad_norm is torch.nn.utils.clip_grad_norm_'s norm of a cloned, unscaled copy of the gradients -- within twice what torch's foreach
    and per-tensor implementations differ by on those gradients (floor: 4 fp32 ulps)."""
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV).train()
    x = torch.randn(2, 3, 128, 128, device=DEV)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]], device=DEV)
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]], device=DEV)
    gen_t = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")
    ps = [p for p in model.parameters() if p.requires_grad]
    max_norm = 0.5
    opt = optim.SGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4, max_grad_norm=max_norm)
    scaler = torch.amp.GradScaler("cuda")
    clipped = 0
    for step in range(4):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, cache_enabled=False):
            out = model(x)
            losses = crit([out, gen_t([out, gt, labels])])
        scaler.scale(losses[-1]).backward()
        inv = 1.0 / scaler.get_scale()
        norms = []
        for foreach in (True, False):
            twins = [torch.nn.Parameter(torch.empty_like(p.grad)) for p in ps if p.grad is not None]
            for t, g in zip(twins, [p.grad for p in ps if p.grad is not None]):
                t.grad = g.clone().mul_(inv)
            norms.append(float(torch.nn.utils.clip_grad_norm_(twins, max_norm, foreach=foreach)))
        kept = [p.grad.clone() for p in ps if p.grad is not None]
        scaler.step(opt)
        scaler.update()
        assert np.isfinite(float(losses[-1].detach()))
        blk = _block(opt._fd_clip)
        assert all(torch.equal(p.grad, k) for p, k in zip([p for p in ps if p.grad is not None], kept)), "p.grad was written"
        if not np.isfinite(norms[1]):                  # an overflow of the f16 backward at the scaler's first scale: the step is skipped
            assert blk["found"] == 1.0 and blk["clip_coef"] == 1.0
            print(f"model step {step}: non-finite gradients, skipped")
            continue
        mine = float(opt.grad_norm)
        bound = max(2 * abs(norms[0] - norms[1]) / norms[1], ULP4)
        print(f"model step {step}: grad_norm {mine!r}, torch foreach {norms[0]!r} / per-tensor {norms[1]!r}, clip_coef {blk['clip_coef']:.4e}, bound {bound:.3e}")
        assert blk["found"] == 0.0 and abs(mine - norms[1]) <= bound * norms[1]
        clipped += blk["clip_coef"] < 1.0
    assert clipped >= 1, "max_norm was never reached: the test did not clip"
