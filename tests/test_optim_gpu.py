"""pytorch_object_detection_amd.optim on the GPU: the update kernels against the float64 references of tests/optim_ref.py at every size / alignment path, the
skipped step, chunking, the learning-rate rules evaluated on the device, graph capture, the model step and checkpoints in both directions.

The bound of every comparison with float64 is measured, not fixed: torch's optimizer of the same name runs on the same device and inputs, its largest deviation
from the float64 reference is taken per tensor relative to max|reference|, and ours must stay within twice that with a floor of 4 fp32 ulps (two stock
implementations of one rule already differ by 1 - 2 ulps after a few steps; the factor 2 allows another, equally valid, operation order)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import optim_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, optim  # noqa: E402
from test_optim_cpu import NEW_STEPS, PY_STEPS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1234.5
ULP4 = 4 * 2.0 ** -23
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4097, 65537, 2 ** 20 + 3)


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

    def gather(self):
        return torch.cat([self.flat[a:b] for a, b in self.ranges]).double().cpu().numpy()

    def assert_sentinels(self, what):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for a, b in self.ranges:
            keep[a:b] = False
        assert bool((self.flat[keep] == SENT).all()), f"{what}: a word outside the tensors was written"


def _specs(nstate):
    """(numel, offsets of p, g, state...) for case 1.  Up to 4 097 elements (257 with two state tensors): every combination of the offsets 0..3.  The kernel decides
    on `all offsets equal` alone and then only the head length 4 - offset matters, so the two large sizes (several blocks, the grid-stride loop) take the four
    equal combinations and four mixed ones."""
    from itertools import product
    out = []
    few = [(k,) * (2 + nstate) for k in range(4)] + [tuple((a + i * b) % 4 for i in range(2 + nstate)) for a, b in ((0, 1), (3, 1), (0, 2), (1, 3))]
    for n in SIZES:
        full = n <= (4097 if nstate < 2 else 257)
        for offs in (product(range(4), repeat=2 + nstate) if full else few):
            out.append((n, tuple(offs)))
    return out


def _seg_max(a, starts):
    return np.maximum.reduceat(np.abs(a), starts)


def _assert_within_measured(ours, theirs, ref, starts, what, scale=None):
    """ours / theirs / ref: flat float64 arrays, segments starting at `starts`.  -> (largest deviation of torch, of ours), in units of max|ref| per tensor.
    `scale` replaces max|ref| for a state tensor: a momentum buffer or a moment is a weighted sum of the gradients seen so far, so its rounding errors are ulps
    of the largest gradient term, whatever the sum cancels to (a one-element buffer can end arbitrarily close to zero)."""
    scale = np.maximum(_seg_max(ref, starts) if scale is None else scale, 1e-30)
    d_t, d_o = _seg_max(theirs - ref, starts) / scale, _seg_max(ours - ref, starts) / scale
    bound = np.maximum(2 * d_t, ULP4)
    worst = int(np.argmax(d_o - bound))
    print(f"{what}: torch deviates by up to {d_t.max():.3e}, ours by up to {d_o.max():.3e} of max|reference| per tensor ({len(starts)} tensors)")
    assert (d_o <= bound).all(), f"{what}: tensor {worst} deviates by {d_o[worst]:.3e}, torch by {d_t[worst]:.3e} (bound {bound[worst]:.3e})"
    return float(d_t.max()), float(d_o.max())


RULES = {
    "sgd": dict(kind="sgd", momentum=0.0, weight_decay=0.0, nesterov=False),
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
    r = RULES[rule]
    return (("momentum_buffer",) if r["momentum"] else ()) if r["kind"] == "sgd" else ("exp_avg", "exp_avg_sq")


@pytest.mark.parametrize("lr_tensor", [False, True], ids=["lr-float", "lr-tensor"])
@pytest.mark.parametrize("scale", [None, 1024.0], ids=["unscaled", "scale1024"])
@pytest.mark.parametrize("rule", list(RULES))
def test_update_kernels_against_float64(rule, scale, lr_tensor):
    names = _state_names(rule)
    specs = _specs(len(names))
    torch.manual_seed(11)
    total = sum(n for n, _ in specs)
    starts = np.cumsum([0] + [n for n, _ in specs[:-1]])
    banks = [Bank([(n, offs[k]) for n, offs in specs]) for k in range(2 + len(names))]
    p0 = torch.randn(total, device=DEV)
    banks[0].fill(p0)
    for b in banks[2:]:
        b.fill(torch.zeros(total, device=DEV))
    params = [torch.nn.Parameter(banks[0].view(i)) for i in range(len(specs))]
    assert params[0].data_ptr() == banks[0].view(0).data_ptr()
    lr_value = 0.05 if RULES[rule]["kind"] == "sgd" else 1e-2
    lr = torch.tensor(lr_value, dtype=torch.float32 if RULES[rule]["kind"] == "sgd" else torch.float64, device=DEV) if lr_tensor else lr_value
    lr_value = float(lr)
    opt = _make(rule, params, lr, ours=True)
    for i, p in enumerate(params):
        p.grad = banks[1].view(i)
        for k, name in enumerate(names):
            opt.state[p][name] = banks[2 + k].view(i)
    if scale is not None:
        opt.grad_scale, opt.found_inf = torch.tensor(scale, device=DEV), torch.zeros((), device=DEV)
    t_param = torch.nn.Parameter(p0.clone())
    t_opt = _make(rule, [t_param], lr_value, ours=False)
    ref = _make_ref(rule, [p0])
    g_max = np.zeros(len(specs))
    for step in range(5):
        g = torch.randn(total, device=DEV)
        g_max = np.maximum(g_max, _seg_max(g.double().cpu().numpy(), starts))
        banks[1].fill(g * scale if scale is not None else g)         # a power of two: the scaled gradient is exact
        opt.step()
        t_param.grad = g.clone()
        t_opt.step()
        ref.step([g], lr_value)
    assert opt.launches == 1 + -(-len(specs) // _lib.OPTIM_MAX_TENSORS)
    for b, what in zip(banks, ("p", "g") + names):
        b.assert_sentinels(f"{rule} {what}")
    assert np.array_equal(banks[1].gather(), ((g * scale if scale is not None else g).double().cpu().numpy()))      # gradients are read only
    _assert_within_measured(banks[0].gather(), t_param.detach().double().cpu().numpy(), ref.p[0].cpu().numpy(), starts, f"{rule} p")
    t_state = t_opt.state[t_param]
    for k, name in enumerate(names):
        _assert_within_measured(banks[2 + k].gather(), t_state[name].double().cpu().numpy(), ref.state()[k][0].cpu().numpy(), starts, f"{rule} {name}",
                                scale=g_max ** 2 if name == "exp_avg_sq" else g_max)
    assert int(opt.global_step) == 5 and int(opt._applied(0)) == 5


def _small(rule, n_tensors=5, lr=0.05, **kw):
    torch.manual_seed(5)
    shapes = [(3,), (17, 5), (4, 4, 3, 3), (1,), (1030,)][:n_tensors]
    params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    return params, _make(rule, params, lr, ours=True, **kw)


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).double().cpu().numpy()


def _starts(ts):
    return np.cumsum([0] + [t.numel() for t in ts[:-1]])


@pytest.mark.parametrize("rule", ["sgd-momentum", "adam"])
def test_skipped_step_leaves_everything_but_the_global_step(rule):
    params, opt = _small(rule)
    t_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    t_opt = _make(rule, t_params, 0.05, ours=False)
    ref = _make_ref(rule, params)
    grads = [[torch.randn_like(p) for p in params] for _ in range(3)]
    opt.grad_scale, opt.found_inf = torch.ones((), device=DEV), torch.zeros((), device=DEV)

    def ours(gs):
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()

    ours(grads[0])
    before = [p.detach().clone() for p in params] + [s.clone() for p in params for s in opt.state[p].values()]
    opt.found_inf.fill_(1.0)
    ours(grads[1])
    after = [p.detach() for p in params] + [s for p in params for s in opt.state[p].values()]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert int(opt.global_step) == 2 and int(opt._applied(0)) == 1
    opt.found_inf.fill_(0.0)
    ours(grads[2])
    assert int(opt.global_step) == 3 and int(opt._applied(0)) == 2
    for gs in (grads[0], grads[2]):
        for p, g in zip(t_params, gs):
            p.grad = g.clone()
        t_opt.step()
        ref.step(gs, 0.05)
    assert not ref.step(grads[1], 0.05, found_inf=True) and ref.applied == 2
    _assert_within_measured(_flat(params), _flat(t_params), _flat(ref.p), _starts(params), f"{rule} after a skipped step")


def test_chunking_missing_gradients_empty_tensors_and_two_groups():
    torch.manual_seed(7)
    sizes = [1 + i % 7 for i in range(700)] + [2 ** 20 + 3]
    params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in sizes]
    no_grad, frozen, empty = 350, 351, 352
    params[frozen].requires_grad_(False)
    params[empty] = torch.nn.Parameter(torch.zeros(0, device=DEV))
    groups = [{"params": params[:400]}, {"params": params[400:], "lr": 0.01, "weight_decay": 1e-2, "momentum": 0.5}]
    opt = optim.SGD(groups, lr=0.05, momentum=0.9, weight_decay=1e-4)
    t_params = [torch.nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in params]
    t_opt = torch.optim.SGD([{"params": t_params[:400]}, {"params": t_params[400:], "lr": 0.01, "weight_decay": 1e-2, "momentum": 0.5}],
                            lr=0.05, momentum=0.9, weight_decay=1e-4)
    refs = [optim_ref.RefSGD(params[:400], 0.9, 1e-4), optim_ref.RefSGD(params[400:], 0.5, 1e-2)]
    grads = [None if i in (no_grad, frozen) else torch.randn_like(p) for i, p in enumerate(params)]
    for p, t, g in zip(params, t_params, grads):
        p.grad = g
        t.grad = None if g is None else g.clone()
    before = [params[i].detach().clone() for i in (no_grad, frozen)]
    opt.step()
    t_opt.step()
    refs[0].step(grads[:400], 0.05)
    refs[1].step(grads[400:], 0.01)
    # 398 tensors with a gradient in group 0 and 301 in group 1: 7 + 5 update launches and the begin launch
    assert opt.launches == 1 + 7 + 5
    for i, b in zip((no_grad, frozen), before):
        assert torch.equal(params[i].detach(), b) and len(opt.state[params[i]]) == 0
    live = [i for i in range(len(params)) if i != empty]
    _assert_within_measured(_flat([params[i] for i in live]), _flat([t_params[i] for i in live]), _flat([(refs[0].p + refs[1].p)[i] for i in live]),
                            _starts([params[i] for i in live]), "chunked sgd p")
    with_state = [i for i in live if i not in (no_grad, frozen)]
    _assert_within_measured(_flat([opt.state[params[i]]["momentum_buffer"] for i in with_state]),
                            _flat([t_opt.state[t_params[i]]["momentum_buffer"] for i in with_state]),
                            _flat([(refs[0].buf + refs[1].buf)[i] for i in with_state]), _starts([params[i] for i in with_state]), "chunked sgd buf",
                            scale=_seg_max(_flat([grads[i] for i in with_state]), _starts([params[i] for i in with_state])))
    assert int(opt._applied(0)) == 1 and int(opt._applied(1)) == 1


@pytest.mark.parametrize("lr_init", [0.01, 0.003])
def test_lr_rules_on_the_device_are_the_host_rules_bit_for_bit(lr_init):
    w = torch.nn.Parameter(torch.ones(8, device=DEV))
    w.grad = torch.ones(8, device=DEV)
    opt = optim.SGD([w], lr=lr_init, lr_schedule=optim.TrainPyLR(lr_init))
    for n in PY_STEPS:
        opt.set_global_step(n - 1)
        opt.step()
        got = opt.param_groups[0]["lr"]
        assert got.dtype == torch.float64 and got.is_cuda and got.item() == optim_ref.train_py_lr(n, lr_init), n
        assert int(opt.global_step) == n
    opt = optim.Adam([w], lr=lr_init, lr_schedule=optim.TrainNewLR(lr_init))
    assert int(opt.global_step) == -1
    for n in NEW_STEPS:
        opt.set_global_step(n - 1)
        opt.step()
        assert opt.param_groups[0]["lr"].item() == optim_ref.train_new_lr(n, lr_init), n
    # the rate the kernels used is the scalar's: one SGD step from ones with gradient ones moves every element by exactly fl32(lr)
    w2 = torch.nn.Parameter(torch.ones(8, device=DEV))
    w2.grad = torch.ones(8, device=DEV)
    opt = optim.SGD([w2], lr=lr_init, lr_schedule=optim.TrainPyLR(lr_init))
    opt.set_global_step(20000)
    opt.step()
    want = np.float32(1.0) - np.float32(lr_init * 0.1) * np.float32(1.0)
    assert float(w2.detach()[0]) == float(want) and w2._version >= 1


@pytest.mark.parametrize("rule", ["sgd-momentum", "adam"])
def test_captured_step_replays_like_eager_calls(rule):
    """One step() captured on one stream, replayed six times with other gradients and found_inf flipped through its captured tensor: bit-identical to six eager
    calls -- the kernels and their arguments are the same."""
    def twin():
        torch.manual_seed(9)
        params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (1, 2, 3, 5, 8, 13, 64, 100, 255, 256, 257, 1031)]
        sched = optim.TrainPyLR(0.01) if rule == "sgd-momentum" else optim.TrainNewLR(0.01)
        opt = _make(rule, params, 0.01, ours=True, lr_schedule=sched)
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
    feeds = [[torch.randn(n, device=DEV, generator=gen) for n in (1, 2, 3, 5, 8, 13, 64, 100, 255, 256, 257, 1031)] for _ in range(7)]
    infs = [0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0]

    def feed(src, opt, k):
        for s, f in zip(src, feeds[k]):
            s.copy_(f)
        opt.found_inf.fill_(infs[k])

    pe, oe, se, body_e = twin()
    pg, og, sg, body_g = twin()
    for src, opt, body in ((se, oe, body_e), (sg, og, body_g)):      # one eager step each: the state tensors exist before the capture
        feed(src, opt, 0)
        body()
    for k in range(1, 7):
        feed(se, oe, k)
        body_e()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body_g()
    for k in range(1, 7):
        feed(sg, og, k)
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert torch.equal(a.detach(), b.detach())
        for name in _state_names(rule):
            assert torch.equal(oe.state[a][name], og.state[b][name])
    assert torch.equal(oe._fd_state_i, og._fd_state_i)              # counters, skip flag, lr and bias corrections, bit for bit
    assert int(og.global_step) == 497 + 7 and int(og._applied(0)) == 4
    assert og.param_groups[0]["lr"].item() == (optim_ref.train_py_lr(504, 0.01) if rule == "sgd-momentum" else optim_ref.train_new_lr(504, 0.01))


def test_state_is_not_created_inside_a_capture(monkeypatch):
    """A state tensor allocated while capturing would be zeroed again by every replay: step() refuses (no capture is started here, the query is patched)."""
    w = torch.nn.Parameter(torch.ones(8, device=DEV))
    w.grad = torch.ones(8, device=DEV)
    opt = optim.SGD([w], lr=0.1, momentum=0.9)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.FdError, match="eager step first"):
        opt.step()
    monkeypatch.undo()
    opt.step()
    assert "momentum_buffer" in opt.state[w] and int(opt.global_step) == 1


def test_step_rejections():
    w = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
    opt = optim.SGD([w], lr=0.1)
    w.grad = torch.ones(6, 4, device=DEV).t()
    with pytest.raises(_lib.FdError, match="grad"):
        opt.step()
    w.grad = None
    w.grad = torch.ones(4, 6, device=DEV).to_sparse()
    with pytest.raises(_lib.FdError, match="grad"):
        opt.step()
    w.grad = None
    opt.step()                                                        # nothing to update: legal, the global step still counts
    assert int(opt.global_step) == 1 and int(opt._applied(0)) == 0 and opt.launches == 1


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_model_step_with_the_hip_optimizer(amp):
    """The model, batch and step function of test_train_gpu's whole-step test.  Four steps with optim.SGD against four with torch.optim.SGD(fused=True), within
    twice what fused and foreach=False -- two stock implementations of one rule -- differ by in the same run (floors: 1e-6 of the weight scale, 2e-3 under AMP):
    per tensor where both move the same gradients, over the whole model where each trains on its own (see (a) and (b) below, and DESIGN 4.3k for the figures);
    then the step replayed from one HIP graph over Builder.opt_build(hip=True) + GradScaler against the same steps enqueued eagerly (1e-5 / 2e-3)."""
    from pytorch_object_detection_amd.bulider import Builder, load_config
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    from pytorch_object_detection_amd.train_graph import GraphedStep
    torch.manual_seed(0)
    base = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV).train()
    x = torch.randn(2, 3, 128, 128, device=DEV)
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]], device=DEV)
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]], device=DEV)
    gen_t = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")

    def make(model, opt, after_backward=None):
        scaler = torch.amp.GradScaler("cuda", enabled=amp)

        def step(x_, gt_, labels_):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp, cache_enabled=False):
                out = model(x_)
                losses = crit([out, gen_t([out, gt_, labels_])])
            scaler.scale(losses[-1]).backward()
            if after_backward is not None:
                after_backward()
            scaler.step(opt)
            scaler.update()
            return losses[-1].detach()
        return step

    kw = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)
    builders = {"fused": lambda ps: torch.optim.SGD(ps, fused=True, **kw), "loop": lambda ps: torch.optim.SGD(ps, foreach=False, **kw),
                "ours": lambda ps: optim.SGD(ps, **kw)}

    def run(which, shadows=(), steps=4):
        """-> (weights, losses, {shadow: weights}).  A shadow is a copy of the weights that another optimizer moves with THIS run's gradients."""
        model = copy.deepcopy(base)
        ps = [p for p in model.parameters() if p.requires_grad]
        twins = {k: [torch.nn.Parameter(p.detach().clone()) for p in ps] for k in shadows}
        opts = {k: builders[k](v) for k, v in twins.items()}

        def feed():
            for k, tw in twins.items():
                for t, p in zip(tw, ps):
                    t.grad = None if p.grad is None else p.grad.clone()
                opts[k].step()
        step = make(model, builders[which](ps), feed if shadows else None)
        losses = [float(step(x, gt, labels)) for _ in range(steps)]
        return [p.detach() for p in ps], losses, {k: [t.detach() for t in tw] for k, tw in twins.items()}

    def dev(ws, ref):
        return np.array([float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12) for a, b in zip(ws, ref)])

    floor = 2e-3 if amp else 1e-6
    tag = "amp" if amp else "fp32"
    # (a) the update alone: on the fused run's own gradients ours and foreach=False move copies of the weights; per tensor, ours is as close to fused as
    # torch's other implementation is.  fp32 only: under AMP the gradients a shadow would take are still scaled and only a fused step unscales them.
    w_fused, l_fused, sh = run("fused", shadows=() if amp else ("ours", "loop"))
    if not amp:
        d_o, d_s = dev(sh["ours"], w_fused), dev(sh["loop"], w_fused)
        print(f"model step ({tag}), same gradients, 4 steps: ours differs from fused by up to {d_o.max():.3e} of the weight scale, foreach=False by up to {d_s.max():.3e}")
        assert (d_o <= np.maximum(2 * d_s, floor)).all(), (int(np.argmax(d_o - 2 * d_s)), d_o.max(), d_s.max())
    # (b) the training runs themselves.  The step is deterministic (two fused runs give the same bits), and it amplifies: one ulp in a weight after step 1
    # is 1e-5 of the weight scale after step 2 and 1e-2 after step 4, for foreach=False as for ours, at tensors that differ from run to run.  So `the
    # deviation between two stock implementations` is taken over the whole model -- the largest over the weights in units of each weight's scale, the
    # largest over the steps for the loss -- and ours stays within twice that.
    w_loop, l_loop, _ = run("loop")
    w_ours, l_ours, _ = run("ours")
    assert all(np.isfinite(v) for v in l_fused + l_loop + l_ours)
    rel = lambda ls: max(abs(a - b) / abs(b) for a, b in zip(ls, l_fused))  # noqa: E731
    d_o, d_s = dev(w_ours, w_fused), dev(w_loop, w_fused)
    print(f"model step ({tag}), 4 training steps: weights differ from the fused run by up to {d_o.max():.3e} (ours) / {d_s.max():.3e} (foreach=False) of the "
          f"weight scale, losses by up to {rel(l_ours):.3e} (ours) / {rel(l_loop):.3e} (foreach=False)")
    assert rel(l_ours) <= max(2 * rel(l_loop), floor), (l_ours, l_fused, l_loop)
    assert d_o.max() <= max(2 * d_s.max(), floor), (d_o.max(), d_s.max())

    # the whole step from one graph, with the optimizer the Builder hands out
    cfg = load_config()
    N = 3
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)
    o_eager, o_graph = Builder(cfg).opt_build(m_eager, hip=True), Builder(cfg).opt_build(m_graph, hip=True)
    s_eager = make(m_eager, o_eager)
    losses_e = [float(s_eager(x, gt, labels)) for _ in range(N + 1 + 3)]
    graphed = GraphedStep(make(m_graph, o_graph), [x, gt, labels], warmup=N)
    losses_g = [float(graphed(x, gt, labels).clone()) for _ in range(4)]
    assert all(np.isfinite(v) for v in losses_e + losses_g)
    np.testing.assert_allclose(losses_g, losses_e[N:], rtol=2e-3 if amp else 1e-5)
    for (n, a), (_, b) in zip(m_eager.named_parameters(), m_graph.named_parameters()):
        scale = float(a.detach().abs().max()) + 1e-12
        assert float((a.detach() - b.detach()).abs().max()) <= (2e-3 if amp else 1e-5) * scale, n
    lr_init = cfg[cfg["model"]["name"]]["optimizer"]["lr"]
    for o in (o_eager, o_graph):
        assert int(o.global_step) == N + 4 and o.param_groups[0]["lr"].item() == optim_ref.train_py_lr(N + 4, lr_init)
    assert torch.equal(o_eager._fd_state_i, o_graph._fd_state_i)


def test_checkpoints_move_between_ours_and_torchs_adam():
    torch.manual_seed(13)
    shapes = [(5,), (33, 7), (8, 4, 3, 3), (1029,)]
    params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    kw = dict(lr=1e-2, weight_decay=1e-4)
    opt = optim.Adam(params, **kw)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
    sd = opt.state_dict()
    assert all(float(st["step"]) == 3.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    ref = optim_ref.RefAdam(params, weight_decay=1e-4, applied=3, exp_avg=[sd["state"][i]["exp_avg"] for i in range(4)],
                            exp_avg_sq=[sd["state"][i]["exp_avg_sq"] for i in range(4)])
    # into torch's fused Adam (the saved param groups decide how the load treats `step`, so they say fused) ...
    t_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    t_opt = torch.optim.Adam(t_params, fused=True, **kw)
    to_torch = copy.deepcopy(sd)
    for g in to_torch["param_groups"]:
        g["fused"] = True
    t_opt.load_state_dict(to_torch)
    # ... and from there back into a fresh one of ours
    b_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    back = optim.Adam(b_params, **kw)
    back.load_state_dict(copy.deepcopy(t_opt.state_dict()))             # (a load may alias the tensors it is given)
    assert int(back._applied(0)) == 3
    for _ in range(2):
        gs = [torch.randn_like(p) for p in params]
        for ps, o in ((t_params, t_opt), (b_params, back)):
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            o.step()
        ref.step(gs, 1e-2)
    _assert_within_measured(_flat(b_params), _flat(t_params), _flat(ref.p), _starts(params), "adam after the round trip")
    assert all(float(st["step"]) == 5.0 for st in back.state_dict()["state"].values())
    assert all(float(st["step"]) == 5.0 for st in t_opt.state_dict()["state"].values())
