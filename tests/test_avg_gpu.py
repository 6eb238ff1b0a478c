"""optim.AveragedModel on the GPU: fd_avg_update_f32 / fd_avg_copy_bytes against the float64 reference of tests/avg_ref.py at every alignment, the gate and the
optimizer's skip flag on the device, a captured step + update against eager calls, and the averaged copy of a whole detector."""
import copy
import math
import os
import sys
from itertools import product

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import avg_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, ops, optim  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 1234.5
ULP4 = 4 * 2.0 ** -23
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4097, 65537, 2 ** 20 + 3)


class Bank:
    """Tensors carved out of one sentinel-filled fp32 buffer.  Slot i holds `numel` elements starting `off` elements (0..3) past a 16-byte boundary, with at
    least four sentinel words on either side."""

    def __init__(self, specs):
        pos, self.ranges = 0, []
        for n, off in specs:
            a = pos + 4 + off
            self.ranges.append((a, a + n))
            pos = (a + n + 4 + 3) // 4 * 4
        self.flat = torch.full((pos + 4,), SENT, dtype=torch.float32, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.index = torch.cat([torch.arange(a, b, device=DEV) for a, b in self.ranges])

    def ptrs(self):
        return [self.flat.data_ptr() + 4 * a for a, _ in self.ranges]

    def fill(self, values):
        self.flat[self.index] = values

    def gather(self):
        return self.flat[self.index]

    def assert_sentinels(self, what):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        keep[self.index] = False
        assert bool((self.flat[keep] == SENT).all()), f"{what}: a word outside the tensors was written"


def _specs():
    """(numel, offset of avg, offset of p).  Up to 4 097 elements every combination of the offsets 0..3; above that (several blocks, the grid-stride loop) two
    equal and two mixed ones: the kernel decides on `offsets equal` alone, and then only the head length 4 - offset matters."""
    out = []
    for n in SIZES:
        for oa, op in (product(range(4), repeat=2) if n <= 4097 else ((0, 0), (3, 3), (0, 1), (2, 3))):
            out.append((n, oa, op))
    return out


class Holder(nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(t.clone()) for t in tensors])


def _launch(bank_a, bank_p, numels, n_avg, state, decay):
    bp = _lib.AvgBeginParams()
    bp.mode, bp.decay, bp.start_step, bp.every = (_lib.AVG_SWA, 0.0, 0, 1) if decay is None else (_lib.AVG_EMA, decay, 0, 1)
    ops.avg_begin(state, n_avg, None, None, bp)
    return ops.avg_update(bank_a.ptrs(), bank_p.ptrs(), numels, state)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _seg_max(a, starts):
    return np.maximum.reduceat(np.abs(a), starts)


@pytest.mark.parametrize("decay", [None, 0.9, 0.999], ids=["swa", "ema0.9", "ema0.999"])
def test_update_kernel_against_float64(decay):
    """Ten updates of 152 tensors with fresh p each time (half of its elements equal to the current average) through fd_avg_begin + fd_avg_update_f32, and the
    same values through torch.optim.swa_utils.AveragedModel on the same device.  The bound is measured here: per tensor, ours stays within twice the stock
    class's largest deviation from float64, in units of max|reference|, with a floor of 4 fp32 ulps."""
    specs = _specs()
    numels = [n for n, _, _ in specs]
    starts = np.concatenate([[0], np.cumsum(numels)[:-1]])
    total = sum(numels)
    bank_a, bank_p = Bank([(n, oa) for n, oa, _ in specs]), Bank([(n, op) for n, _, op in specs])
    gen = torch.Generator(device=DEV).manual_seed(3)
    first = torch.randn(total, device=DEV, generator=gen)
    bank_a.fill(torch.randn(total, device=DEV, generator=gen))              # what the copy held before: the first update must overwrite it
    holder = Holder([first[s:s + n] for s, n in zip(starts, numels)])
    stock = swa_utils.AveragedModel(holder, multi_avg_fn=None if decay is None else swa_utils.get_ema_multi_avg_fn(decay))
    ref = avg_ref.RefAveraged([first], mode=avg_ref.SWA if decay is None else avg_ref.EMA, decay=decay or 0.0)
    n_avg, state = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    worst_t = worst_o = 0.0
    for k in range(10):
        if k == 0:
            p = first
        else:
            cur = bank_a.gather()
            keep = torch.rand(total, device=DEV, generator=gen) < 0.5
            p = torch.where(keep, cur, torch.randn(total, device=DEV, generator=gen) * (1.0 + k))
        bank_p.fill(p)
        before = bank_a.gather()
        assert _launch(bank_a, bank_p, numels, n_avg, state, decay) == math.ceil(len(specs) / _lib.OPTIM_MAX_TENSORS)
        with torch.no_grad():
            for q, s, n in zip(holder.ps, starts, numels):
                q.copy_(p[s:s + n])
        stock.update_parameters(holder)
        assert ref.update([p])
        ours = bank_a.gather()
        bank_a.assert_sentinels(f"update {k}: avg")
        bank_p.assert_sentinels(f"update {k}: p")
        assert torch.equal(bank_p.gather(), p)
        if k == 0:
            assert torch.equal(_bits(ours), _bits(p)), "the first update copies bit for bit"
        else:
            assert torch.equal(_bits(ours[keep]), _bits(before[keep])), f"update {k}: an element with p == avg changed"
        theirs = torch.cat([q.detach().reshape(-1) for q in stock.module.ps]).double().cpu().numpy()
        want = ref.p[0].cpu().numpy()
        scale = np.maximum(_seg_max(want, starts), 1e-30)
        d_t, d_o = _seg_max(theirs - want, starts) / scale, _seg_max(ours.double().cpu().numpy() - want, starts) / scale
        bound = np.maximum(2 * d_t, ULP4)
        worst = int(np.argmax(d_o - bound))
        assert (d_o <= bound).all(), f"update {k}: tensor {worst} {specs[worst]} deviates by {d_o[worst]:.3e}, torch by {d_t[worst]:.3e} (bound {bound[worst]:.3e})"
        worst_t, worst_o = max(worst_t, float(d_t.max())), max(worst_o, float(d_o.max()))
    assert int(n_avg) == int(stock.n_averaged) == ref.n_averaged == 10
    print(f"update kernel ({'swa' if decay is None else decay}), 10 updates: torch deviates by up to {worst_t:.3e}, ours by up to {worst_o:.3e} of max|reference| "
          f"per tensor ({len(specs)} tensors)")


@pytest.mark.parametrize("decay", [0.0, 1.0])
def test_update_kernel_bitwise_cases(decay):
    """decay = 0 is a copy on every update, NaN payloads included; decay = 1 leaves the average as the first update set it, bit for bit."""
    specs = [s for s in _specs() if s[0] <= 4097]
    numels = [n for n, _, _ in specs]
    total = sum(numels)
    bank_a, bank_p = Bank([(n, oa) for n, oa, _ in specs]), Bank([(n, op) for n, _, op in specs])
    gen = torch.Generator(device=DEV).manual_seed(4)
    n_avg, state = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    first = None
    for k in range(3):
        p = torch.randn(total, device=DEV, generator=gen)
        if decay == 0.0:
            pi = _bits(p)
            pi[k::97] = 0x7FC00000 + 0x1234 + k              # quiet NaNs with a payload
            pi[(k + 40)::97] = -0x400000 + 0x55              # 0xFFC00055: sign bit set, another payload
            p = pi.view(torch.float32)                       # (decay = 1 stays finite: (p - avg) * 0 is 0 only then)
        first = p if first is None else first
        bank_p.fill(p)
        _launch(bank_a, bank_p, numels, n_avg, state, decay)
        want = p if decay == 0.0 else first
        assert torch.equal(_bits(bank_a.gather()), _bits(want)), k
        bank_a.assert_sentinels(f"update {k}")
    assert int(n_avg) == 3


def _expected_fp32(a, p, w):
    """The kernel's arithmetic with torch's elementwise fp32 kernels (one rounding per operation, no contraction across them): bit-exact."""
    return p.clone() if w == 1.0 else a + (p - a) * torch.tensor(w, dtype=torch.float64).to(torch.float32).to(a.device)


@pytest.mark.parametrize("count", [1, 64, 65, 129])
def test_chunking_with_an_empty_tensor(count):
    torch.manual_seed(count)
    shapes = [(0,) if i == count // 2 and count > 1 else ((i % 7) + 1, (i % 3) + 1) for i in range(count)]
    model = Holder([torch.randn(s, device=DEV) for s in shapes])
    avg = optim.AveragedModel(model, decay=0.9)
    assert avg.n_averaged.device == model.ps[0].device
    want = [p.detach().clone() for p in model.ps]
    for k in range(3):
        with torch.no_grad():
            for p in model.ps:
                p.add_(torch.randn_like(p))
        avg.update_parameters(model)
        assert avg.launches == 1 + math.ceil(count / _lib.OPTIM_MAX_TENSORS)          # begin + one update launch per 64 tensors, no buffers
        want = [_expected_fp32(a, p.detach(), 1.0 if k == 0 else 1.0 - 0.9) for a, p in zip(want, model.ps)]
        for a, b in zip(avg.module.ps, want):
            assert torch.equal(_bits(a.detach()), _bits(b)), (k, tuple(a.shape))
    assert int(avg.n_averaged) == 3


@pytest.mark.parametrize("nbytes", [1, 7, 8, 9, 4095, 65537])
def test_copy_bytes_at_every_alignment(nbytes):
    """All 64 combinations of the byte offsets 0..7 of dst and src in ONE launch; exact results, every byte outside the destinations intact."""
    combos = list(product(range(8), repeat=2))
    pitch = (nbytes + 8 + 32 + 15) // 16 * 16
    dst = torch.full((len(combos) * pitch,), 0xA5, dtype=torch.uint8, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(nbytes)
    src = torch.randint(0, 256, (len(combos) * pitch,), dtype=torch.uint8, device=DEV, generator=gen)
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    d_off = [i * pitch + 16 + od for i, (od, _) in enumerate(combos)]
    s_off = [i * pitch + 16 + os_ for i, (_, os_) in enumerate(combos)]
    state, n_avg = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    bp = _lib.AvgBeginParams()
    bp.mode, bp.every = _lib.AVG_SWA, 1
    src_before = src.clone()
    # apply == 0 (a zeroed state block): nothing is written
    assert ops.avg_copy([dst.data_ptr() + o for o in d_off], [src.data_ptr() + o for o in s_off], [nbytes] * len(combos), state) == 1
    assert bool((dst == 0xA5).all())
    ops.avg_begin(state, n_avg, None, None, bp)
    ops.avg_copy([dst.data_ptr() + o for o in d_off], [src.data_ptr() + o for o in s_off], [nbytes] * len(combos), state)
    keep = torch.ones_like(dst, dtype=torch.bool)
    for d, s in zip(d_off, s_off):
        assert torch.equal(dst[d:d + nbytes], src[s:s + nbytes]), (nbytes, d % 16, s % 16)
        keep[d:d + nbytes] = False
    assert bool((dst[keep] == 0xA5).all()) and torch.equal(src, src_before)


def test_copy_bytes_of_int64_scalars():
    """0-dim int64 tensors (BatchNorm's num_batches_tracked), as views at 8-byte offsets and as tensors of their own."""
    pool_d, pool_s = torch.full((8,), -7, dtype=torch.int64, device=DEV), torch.arange(100, 108, dtype=torch.int64, device=DEV)
    dst = [pool_d[1], pool_d[4], torch.tensor(-7, dtype=torch.int64, device=DEV)]
    src = [pool_s[2], pool_s[5], torch.tensor(2 ** 40 + 3, dtype=torch.int64, device=DEV)]
    assert all(t.dim() == 0 for t in dst + src)
    state, n_avg = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    bp = _lib.AvgBeginParams()
    bp.mode, bp.every = _lib.AVG_SWA, 1
    ops.avg_begin(state, n_avg, None, None, bp)
    ops.avg_copy([t.data_ptr() for t in dst], [t.data_ptr() for t in src], [8] * 3, state)
    assert pool_d.tolist() == [-7, 102, -7, -7, 105, -7, -7, -7] and int(dst[2]) == 2 ** 40 + 3


def _toy(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5), nn.Flatten(), nn.Linear(5, 3)).to(DEV)


def _train_like(model, opt, gen):
    """What a step does, without a backward: fresh gradients, opt.step(), and the running statistics move."""
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device=DEV, generator=gen)
    with torch.no_grad():
        for b in model.buffers():
            if b.is_floating_point():
                b.add_(torch.rand(b.shape, device=DEV, generator=gen))
            else:
                b.add_(1)
    opt.step()


def _snapshot(m):
    return [t.detach().clone() for t in list(m.parameters()) + list(m.buffers())]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_skipped_step_leaves_the_average_untouched():
    """found_inf set as GradScaler sets it: the optimizer skips, and the update that follows leaves avg and n_averaged bit-identical; the next clean step
    averages with the weight of n_averaged + 1."""
    model, gen = _toy(), torch.Generator(device=DEV).manual_seed(1)
    opt = optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    avg = optim.AveragedModel(model, optimizer=opt)               # SWA
    opt.grad_scale, opt.found_inf = torch.ones((), device=DEV), torch.zeros((), device=DEV)
    for _ in range(2):
        _train_like(model, opt, gen)
        avg.update_parameters(model)
    assert int(avg.n_averaged) == 2
    held, versions = _snapshot(avg.module), [p._version for p in avg.module.parameters()]
    opt.found_inf.fill_(1.0)
    _train_like(model, opt, gen)
    avg.update_parameters(model)
    assert int(avg.n_averaged) == 2 and _same(_snapshot(avg.module), held)
    assert all(p._version > v for p, v in zip(avg.module.parameters(), versions))       # host only; a re-pack too many is harmless
    opt.found_inf.fill_(0.0)
    _train_like(model, opt, gen)
    avg.update_parameters(model)
    assert int(avg.n_averaged) == 3
    n_p = len(list(model.parameters()))
    for a, was, p in zip(avg.module.parameters(), held[:n_p], model.parameters()):
        assert torch.equal(a.detach(), _expected_fp32(was, p.detach(), 1.0 / 3.0))
    assert _same(list(avg.module.buffers()), list(model.buffers()))                     # copied on every applied call


@pytest.mark.parametrize("start_step,every", [(0, 1), (3, 1), (3, 4), (12, 5)])
def test_gate_on_the_device_follows_the_reference_schedule(start_step, every):
    model, gen = _toy(), torch.Generator(device=DEV).manual_seed(2)
    opt = optim.SGD(model.parameters(), lr=0.1)
    avg = optim.AveragedModel(model, decay=0.9, optimizer=opt, start_step=start_step, every=every, use_buffers=True)
    opt.grad_scale, opt.found_inf = torch.ones((), device=DEV), torch.zeros((), device=DEV)
    skipped = (3, 7)
    ref = avg_ref.RefAveraged(list(model.parameters()), list(model.buffers()), mode=avg_ref.EMA, decay=0.9, use_buffers=True, start_step=start_step,
                              every=every, rounded=True)
    applied = []
    for g in range(1, 13):                                        # the optimizer's global step counts from 1
        opt.found_inf.fill_(1.0 if g in skipped else 0.0)
        _train_like(model, opt, gen)
        before = int(avg.n_averaged)
        avg.update_parameters(model)
        if int(avg.n_averaged) != before:
            applied.append(g)
        assert ref.update(list(model.parameters()), list(model.buffers()), skip=g in skipped, global_step=g) == (applied[-1:] == [g])
        assert int(opt.global_step) == g and int(avg.n_averaged) == ref.n_averaged
    assert applied == avg_ref.gate_schedule(range(1, 13), start_step, every, skipped)
    for a, want in zip(list(avg.module.parameters()) + list(avg.module.buffers()), ref.p + ref.b):
        if a.is_floating_point():
            # the reference blends with the same fp32 weight; what is left is rounding: at most 0.5 ulp for the sum and 0.1 * 1 ulp for (p - avg) * w per update,
            # and an update keeps 0.9 of the error before it: 0.6 / (1 - 0.9) = 6 ulps at the worst, 8 allowed
            assert float((a.detach().double() - want).abs().max()) <= 2 * ULP4 * max(float(want.abs().max()), 1e-30)
        else:
            assert torch.equal(a, want)
    if not applied:                                               # never applied: still the deep copy the constructor made
        assert int(avg.n_averaged) == 0


def test_without_optimizer_every_call_applies():
    model, gen = _toy(), torch.Generator(device=DEV).manual_seed(3)
    avg = optim.AveragedModel(model)
    stock = swa_utils.AveragedModel(model)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for k in range(4):
        _train_like(model, opt, gen)
        avg.update_parameters(model)
        stock.update_parameters(model)
        assert int(avg.n_averaged) == k + 1 and avg.launches == 3
    for a, b in zip(avg.module.parameters(), stock.module.parameters()):
        a, b = a.detach(), b.detach()
        assert float((a - b).abs().max()) <= 2 * ULP4 * float(b.abs().max())      # three blends of at most 1 ulp in either implementation
    assert _same(list(avg.module.buffers()), list(stock.module.buffers()))


def test_update_rejections_on_the_device():
    model = _toy()
    avg = optim.AveragedModel(model)
    with pytest.raises(_lib.FdError, match="GPU only"):
        avg.update_parameters(copy.deepcopy(model).cpu())
    with pytest.raises(ValueError, match="model.*fp32"):
        avg.update_parameters(copy.deepcopy(model).double())
    other = nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5), nn.Flatten(), nn.Linear(5, 4)).to(DEV)
    with pytest.raises(ValueError, match="model.*shape"):
        avg.update_parameters(other)
    cl = nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5), nn.Flatten(), nn.Linear(5, 3)).to(DEV).to(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="model.*strides"):
        avg.update_parameters(cl)
    strided = copy.deepcopy(model)
    strided[3].weight = nn.Parameter(torch.zeros(3, 10, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="model"):
        optim.AveragedModel(strided).update_parameters(strided)
    bigger = nn.Sequential(*list(copy.deepcopy(model)), nn.Linear(3, 2).to(DEV))
    with pytest.raises(ValueError, match="model.*parameters"):
        avg.update_parameters(bigger)
    assert int(avg.n_averaged) == 0


def test_captured_step_and_update_replay_like_eager_calls():
    """opt.step(); avg.update_parameters(model) captured after one eager step, on one stream, and replayed five times with other gradients (one of them holding
    an inf): the average, the parameters and n_averaged are those of five eager calls, bit for bit."""
    sizes = (1, 2, 3, 5, 8, 13, 64, 100, 255, 256, 257, 1031)

    def twin():
        torch.manual_seed(9)
        model = Holder([torch.randn(n, device=DEV) for n in sizes])
        model.register_buffer("counter", torch.zeros((), dtype=torch.int64, device=DEV))
        model.register_buffer("stat", torch.zeros(7, device=DEV))
        opt = optim.SGD(model.parameters(), lr=0.01, momentum=0.9, max_grad_norm=5.0)
        avg = optim.AveragedModel(model, decay=0.9, optimizer=opt, start_step=2, every=2)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        opt.grad_scale, opt.found_inf = torch.full((), 4.0, device=DEV), torch.zeros((), device=DEV)
        src = [torch.zeros_like(p) for p in model.parameters()]

        def body():
            for p, s in zip(model.parameters(), src):
                p.grad.copy_(s)
            model.counter.add_(1)
            model.stat.add_(src[6][:7])
            opt.step()
            avg.update_parameters(model)
        return model, opt, avg, src, body

    gen = torch.Generator(device=DEV).manual_seed(2)
    feeds = [[torch.randn(n, device=DEV, generator=gen) * 4.0 for n in sizes] for _ in range(6)]
    feeds[3][9][17] = float("inf")                    # global step 4 is skipped inside the replays: the gate would have applied there

    def feed(src, k):
        for s, f in zip(src, feeds[k]):
            s.copy_(f)

    me, oe, ae, se, body_e = twin()
    mg, og, ag, sg, body_g = twin()
    for src, body in ((se, body_e), (sg, body_g)):      # one eager step each: the optimizer's state and the averager's block exist before the capture
        feed(src, 0)
        body()
    for k in range(1, 6):
        feed(se, k)
        body_e()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body_g()
    for k in range(1, 6):
        feed(sg, k)
        graph.replay()
    torch.cuda.synchronize()
    assert int(ae.n_averaged) == int(ag.n_averaged) == 2 and int(og.global_step) == 6        # applied at steps 2 and 6
    assert torch.equal(ae._fd_state, ag._fd_state) and torch.equal(oe._fd_state_i, og._fd_state_i)
    for a, b in zip(_snapshot(ae.module) + _snapshot(me), _snapshot(ag.module) + _snapshot(mg)):
        assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
    assert int(ag.module.counter) == 6 and not _same(list(ag.module.ps), list(mg.ps))


@pytest.mark.parametrize("use_buffers", [False, True], ids=["copy_buffers", "use_buffers"])
def test_whole_model_average(use_buffers):
    """HISFCOS-R50 after a forward (plans built): the copy, three SGD steps with an EMA gated by the optimizer, the averaged state dict against float64 over the
    per-step snapshots (bound: twice the stock class's deviation, floor 4 fp32 ulps), frozen tensors bit-equal, the copy's eval forward against a fresh model
    loaded with its state dict, the state dict through the stock class and back."""
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS

    def fresh():
        if use_buffers:      # the running statistics move: a model whose BatchNorms train, on the HIP batch-statistics nodes
            return HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats()
        return HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).enable_stem_training()

    torch.manual_seed(0)
    model = fresh().to(DEV).eval()
    x = torch.randn(2, 3, 128, 128, device=DEV)            # the smallest input this detector admits: its stride-128 level is 1 x 1 here, and empty below
    gt = torch.tensor([[[10., 12., 60., 70.], [30., 30., 120., 110.], [-1, -1, -1, -1]],
                       [[5., 5., 25., 30.], [0., 0., 127., 127.], [64., 20., 100., 90.]]], device=DEV)
    labels = torch.tensor([[3, 7, -1], [1, 20, 12]], device=DEV)
    y_before = [[t.clone() for t in grp] for grp in model(x)]              # plans exist before the copy
    assert model._plans
    opt = optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4)
    avg = optim.AveragedModel(model, decay=0.9, optimizer=opt, use_buffers=use_buffers)
    stock = swa_utils.AveragedModel(model, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(0.9), use_buffers=use_buffers)
    assert avg.module._plans == {} and model._plans and avg.module.backbone.hip_stem_train
    assert getattr(avg.module.backbone.trunk, "hip_bn_train", False) == use_buffers
    for grp, want in zip(model(x), y_before):                              # the source's plans survived the copy
        assert all(torch.equal(a, b) for a, b in zip(grp, want))

    gen_t = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")
    names = [k for k, _ in model.named_parameters()] + [k for k, _ in model.named_buffers()]
    n_p = len(list(model.parameters()))
    ref = avg_ref.RefAveraged(list(model.parameters()), list(model.buffers()), mode=avg_ref.EMA, decay=0.9, use_buffers=use_buffers)
    model.train()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        out = model(x)
        loss = crit([out, gen_t([out, gt, labels])])[-1]
        loss.backward()
        opt.step()
        avg.update_parameters(model)
        stock.update_parameters(model)
        assert ref.update(list(model.parameters()), list(model.buffers()))
    assert math.isfinite(float(loss.detach())) and int(avg.n_averaged) == 3
    n_avg_t = n_p + (sum(b.is_floating_point() for b in model.buffers()) if use_buffers else 0)
    n_copy = len(list(model.buffers())) - (n_avg_t - n_p)
    assert avg.launches == 1 + math.ceil(n_avg_t / 64) + math.ceil(n_copy / 64)
    mine = list(avg.module.parameters()) + list(avg.module.buffers())
    theirs = list(stock.module.parameters()) + list(stock.module.buffers())
    live = list(model.parameters()) + list(model.buffers())
    worst_t = worst_o = 0.0
    moved = 0
    for name, a, t, want, cur in zip(names, mine, theirs, ref.p + ref.b, live):
        a, t, cur = a.detach(), t.detach(), cur.detach()
        if not a.is_floating_point():
            assert torch.equal(a, cur), name                  # integer buffers are copied, with either use_buffers
            continue
        scale = max(float(want.abs().max()), 1e-30)
        d_t, d_o = float((t.double() - want).abs().max()) / scale, float((a.double() - want).abs().max()) / scale
        assert d_o <= max(2 * d_t, ULP4), f"{name}: deviates by {d_o:.3e}, torch by {d_t:.3e}"
        worst_t, worst_o = max(worst_t, d_t), max(worst_o, d_o)
        moved += int(not torch.equal(a, cur))
    print(f"whole model (use_buffers={use_buffers}), 3 EMA updates: torch deviates by up to {worst_t:.3e}, ours by up to {worst_o:.3e} of max|reference| per tensor")
    assert moved > 30
    # tensors that never train are bit-equal to the model's: frozen parameters, and (without use_buffers) every buffer
    for (name, a), cur in zip(list(avg.module.named_parameters()) + list(avg.module.named_buffers()), live):
        if (isinstance(cur, nn.Parameter) and not cur.requires_grad) or (not use_buffers and not isinstance(cur, nn.Parameter)):
            assert torch.equal(_bits(a.detach()) if a.dtype == torch.float32 else a, _bits(cur.detach()) if a.dtype == torch.float32 else cur), name
    assert use_buffers or any(not p.requires_grad for p in model.parameters())

    # the copy's own plans: its eval forward is that of a freshly constructed model holding its state dict
    y_avg = [[t.clone() for t in grp] for grp in avg.module.eval()(x)]
    twin = fresh().to(DEV).eval()
    twin.load_state_dict(avg.module.state_dict())
    for grp, want in zip(twin(x), y_avg):
        assert all(torch.equal(a, b) for a, b in zip(grp, want))
    assert not all(torch.equal(a, b) for grp, want in zip(y_avg, y_before) for a, b in zip(grp, want))
    # the checkpoint through the stock class and back
    via = swa_utils.AveragedModel(fresh().to(DEV))
    via.load_state_dict(avg.state_dict())
    back = optim.AveragedModel(fresh().to(DEV), decay=0.9)
    back.load_state_dict(via.state_dict())
    sd, bd = avg.state_dict(), back.state_dict()
    assert list(sd) == list(bd) == list(via.state_dict()) and all(torch.equal(sd[k], bd[k]) for k in sd) and int(back.n_averaged) == 3
