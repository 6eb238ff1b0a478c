"""The cumulative-average (`_cma`) BatchNorm entry points on the device: nn.BatchNorm2d(momentum=None) on every HIP batch-statistics node.

Stated equality (include/fcosdet.h): for a counter holding n >= 1 a `_cma` call is BIT FOR BIT its plain sibling called with momentum = float32(1 / n) --
y, the workspace with the statistics block, both running tensors; n < 1 writes neither running tensor and y as always.  All six entry points through the
ops wrappers (a tensor in place of the float momentum selects the `_cma` symbol), the synchronised forms over 2 ranks simulated on one device as in
tests/test_syncbn_wide_kernels_gpu.py (unequal rows, the count from sums[2C]).

Module level: the three training nodes on an nn.BatchNorm2d(C, momentum=None) over 6 batches against the float64 restatement of tests/bn_cma_ref.py.  The
bound is measured: per tensor, twice the deviation of stock nn.BatchNorm2d(momentum=None) in fp32 on the same device and values, in units of
max |reference|, with a floor of 4 fp32 ulps (the convention of tests/test_avg_gpu.py).  Measured on an MI355X: ours 6.5e-8 .. 9.2e-8, stock
5.7e-8 .. 1.5e-7 of max |reference| over the six tensors, so the floor of 4.8e-7 is the bound everywhere.

Capture: a narrow + wide + residual stack with momentum=None captured by torch.cuda.graph and replayed follows the counter, bit for bit with eager calls."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_cma_ref as CR
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd.ops import Rows, Segs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-3
SENTINEL = -77.25
ULP4 = 4 * 2.0 ** -23
WIDTHS = [4, 32, 40, 1024, 2048]
NARROW = [4, 32, 1024]                        # C / 4 divides 256: the widths of the GroupNorm-route family
ROWS = [2, 3, 257, 4099]
COUNTS = [1, 2, 3, 7, 1000]
DEAD = [0, -1]


def _inputs(C, rows, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 1000 * C + rows)
    x = torch.randn(rows, C, generator=g, device=DEV) * 1.5 + 0.25
    res = torch.randn(rows, C, generator=g, device=DEV)
    gm = torch.rand(C, generator=g, device=DEV) + 0.5
    bt = torch.randn(C, generator=g, device=DEV) * 0.1
    rm = torch.randn(C, generator=g, device=DEV) * 0.3
    rv = torch.rand(C, generator=g, device=DEV) + 0.5
    return x, res, gm, bt, rm, rv


def _running(rm, rv, off):
    """running_mean / running_var at element offset `off` inside sentinel-filled buffers: (buffers, views)."""
    C = rm.numel()
    bufs = [torch.full((C + 8,), SENTINEL, device=DEV) for _ in range(2)]
    views = [b[off:off + C] for b in bufs]
    views[0].copy_(rm)
    views[1].copy_(rv)
    return bufs, views


def _sentinels_intact(bufs, off, C):
    return all(bool((b[:off] == SENTINEL).all()) and bool((b[off + C:] == SENTINEL).all()) for b in bufs)


def _shards(rows):
    r1 = max(1, rows // 3)
    return [rows - r1, r1]                    # 2 -> (1, 1), 3 -> (2, 1), 257 -> (172, 85), 4099 -> (2733, 1366)


# ---- one runner per entry point: run(momentum, rm_view, rv_view) -> list of tensors to compare (y first)
def _narrow_runner(dev_count, x, gm, bt):
    rows, C = x.shape
    segs = Segs.make(1, [(rows, 1)])
    count = torch.tensor([float(rows)], dtype=torch.float64, device=DEV)

    def run(momentum, rm, rv):
        y = torch.empty_like(x)
        ws = ops.groupnorm_workspace(segs, C, DEV).zero_()
        ops.groupnorm_act(Rows(x), gm, bt, Rows(y), segs, C, _lib.ACT_RELU, ws, EPS)
        if dev_count:
            ops.batchnorm_update_running_dev(ws, count, C, momentum, EPS, rm, rv)
        else:
            ops.batchnorm_update_running(ws, rows, C, momentum, EPS, rm, rv)
        return [y, ws]
    return run


def _wide_runner(res, x, gm, bt):
    rows, C = x.shape

    def run(momentum, rm, rv):
        y = torch.empty_like(x)
        ws = ops.batchnorm_train_workspace(rows, C, DEV).zero_()
        if res is None:
            ops.batchnorm_train_fwd(Rows(x), gm, bt, Rows(y), EPS, _lib.ACT_SILU, momentum, rm, rv, ws=ws)
        else:
            ops.batchnorm_train_res_fwd(Rows(x), gm, bt, Rows(res), Rows(y), EPS, _lib.ACT_RELU, momentum, rm, rv, ws=ws)
        return [y, ws]
    return run


def _sync_runner(family, res, x, gm, bt):
    """2 simulated ranks; rank 0 carries the running tensors under test, rank 1 runs without any (and, in the `_cma` run, without a counter)."""
    rows, C = x.shape
    shards = _shards(rows)
    xs = [t.contiguous() for t in x.split(shards)]
    rs = [t.contiguous() for t in res.split(shards)] if res is not None else [None, None]
    fwd = {"narrow": ops.batchnorm_sync_fwd, "wide": ops.batchnorm_train_sync_fwd}[family]

    def workspace(r):
        if family == "narrow":
            return ops.groupnorm_workspace(Segs.make(1, [(shards[r], 1)]), C, DEV).zero_()
        return ops.batchnorm_train_sync_workspace(shards[r], C, DEV).zero_()

    def run(momentum, rm, rv):
        sums = [torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV) for _ in shards]
        wss = [workspace(r) for r in range(2)]
        for r in range(2):
            if res is None:
                fwd(1, Rows(xs[r]), sums[r], act_id=_lib.ACT_RELU, ws=wss[r])
            else:                                        # phase 1 ignores the counter as it ignores the momentum, and never reads res
                ops.batchnorm_train_sync_res_fwd(1, Rows(xs[r]), sums[r], act_id=_lib.ACT_RELU, momentum=momentum, ws=wss[r])
            sums[r][2 * C] = float(shards[r])
        red = torch.stack(sums).sum(0)                   # the all-reduce
        ys = []
        for r in range(2):
            sums[r].copy_(red)
            y = torch.empty_like(xs[r])
            run_args = (momentum, rm, rv) if r == 0 else (None, None, None)
            if res is None:
                fwd(2, Rows(xs[r]), sums[r], gm, bt, Rows(y), EPS, _lib.ACT_RELU, -1.0, *run_args, ws=wss[r])
            else:
                ops.batchnorm_train_sync_res_fwd(2, Rows(xs[r]), sums[r], gm, bt, Rows(rs[r]), Rows(y), EPS, _lib.ACT_RELU, -1.0, *run_args, ws=wss[r])
            ys.append(y)
        assert float(sums[0][2 * C]) == float(rows)
        return [torch.cat(ys, 0)] + wss
    return run


ENTRIES = {
    "update_running": (NARROW, lambda x, res, gm, bt: _narrow_runner(False, x, gm, bt)),
    "update_running_dev": (NARROW, lambda x, res, gm, bt: _narrow_runner(True, x, gm, bt)),
    "update_running_dev_sync": (NARROW, lambda x, res, gm, bt: _sync_runner("narrow", None, x, gm, bt)),
    "train_fwd": (WIDTHS, lambda x, res, gm, bt: _wide_runner(None, x, gm, bt)),
    "train_res_fwd": (WIDTHS, lambda x, res, gm, bt: _wide_runner(res, x, gm, bt)),
    "train_sync_fwd": (WIDTHS, lambda x, res, gm, bt: _sync_runner("wide", None, x, gm, bt)),
    "train_sync_res_fwd": (WIDTHS, lambda x, res, gm, bt: _sync_runner("wide", res, x, gm, bt)),
}
CASES = [(e, C, rows) for e, (widths, _) in ENTRIES.items() for C in widths for rows in ROWS]


@pytest.mark.parametrize("entry,C,rows", CASES, ids=[f"{e}-C{C}-rows{r}" for e, C, r in CASES])
def test_cma_is_the_plain_sibling_at_one_over_n_bit_for_bit(entry, C, rows):
    x, res, gm, bt, rm, rv = _inputs(C, rows)
    run = ENTRIES[entry][1](x, res, gm, bt)
    launches = []
    for off in (0, 1):
        for n in COUNTS + DEAD:
            counter = torch.tensor(n, dtype=torch.int64, device=DEV)
            bufs_c, views_c = _running(rm, rv, off)
            at = ops.LAUNCHES[0]
            got = run(counter, *views_c)
            launches.append(ops.LAUNCHES[0] - at)
            assert int(counter) == n, "the counter was written"
            assert _sentinels_intact(bufs_c, off, C), f"n={n} off={off}: words around the running tensors were written"
            if n >= 1:
                momentum = float(np.float32(1.0 / n))
                bufs_p, views_p = _running(rm, rv, off)
                at = ops.LAUNCHES[0]
                want = run(momentum, *views_p)
                launches.append(ops.LAUNCHES[0] - at)
                assert all(torch.equal(a, b) for a, b in zip(views_c, views_p)), f"n={n} off={off}: running statistics differ from momentum={momentum!r}"
                assert not torch.equal(views_c[0], rm) and not torch.equal(views_c[1], rv)
                if n == 1:                                # factor 1: the batch statistics themselves, whatever was there
                    mean, _, unbiased = CR.batch_stats(x)
                    assert float((views_c[0].double().cpu() - mean.cpu()).abs().max()) <= 2.0 ** -23 * float(mean.abs().max())
                    assert float((views_c[1].double().cpu() - unbiased.cpu()).abs().max()) <= 4 * 2.0 ** -23 * float(unbiased.abs().max())
            else:
                want = run(0.1, *_running(rm, rv, off)[1])
                assert torch.equal(views_c[0], rm) and torch.equal(views_c[1], rv), f"n={n}: a counter below 1 moved the running statistics"
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), f"n={n} off={off}: y / workspace differ"
    assert len(set(launches)) == 1, f"the `_cma` form and its sibling enqueue different numbers of launches: {sorted(set(launches))}"


def test_counter_checks_of_the_wrappers():
    x, res, gm, bt, rm, rv = _inputs(32, 64)
    y = Rows(torch.empty_like(x))
    for bad in (torch.tensor(3, dtype=torch.int32, device=DEV), torch.tensor([3, 4], dtype=torch.int64, device=DEV), torch.tensor(3, dtype=torch.int64)):
        with pytest.raises(_lib.FdError, match="num_batches_tracked"):
            ops.batchnorm_train_fwd(Rows(x), gm, bt, y, EPS, _lib.ACT_NONE, bad, rm.clone(), rv.clone())
    # without running tensors a counter is not looked at (and may be absent): y as always
    ops.batchnorm_train_fwd(Rows(x), gm, bt, y, EPS, _lib.ACT_NONE, None, None, None)
    y2 = Rows(torch.empty_like(x))
    ops.batchnorm_train_fwd(Rows(x), gm, bt, y2, EPS, _lib.ACT_NONE, torch.tensor(3, dtype=torch.int64, device=DEV), None, None)
    assert torch.equal(y.buf, y2.buf)


# ------------------------------------------------------------------------------------------------ module level
NODES = {"narrow": (32, lambda bn, x, res: T.batchnorm_train_rows(bn, x, _lib.ACT_RELU)),
         "wide": (40, lambda bn, x, res: T._bn_wide_rows(bn, x, _lib.ACT_SILU)),
         "residual": (2048, lambda bn, x, res: T.batchnorm_train_res_rows(bn, x, res, _lib.ACT_RELU))}


@pytest.mark.parametrize("node", list(NODES))
def test_nodes_on_momentum_none_against_float64(node):
    C, call = NODES[node]
    g = torch.Generator().manual_seed(7)
    batches = [torch.randn(37 + 50 * k, C, generator=g) * (1.0 + 0.4 * k) + 0.3 * k for k in range(6)]
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    ours, stock = nn.BatchNorm2d(C, momentum=None, eps=EPS).to(DEV).train(), nn.BatchNorm2d(C, momentum=None, eps=EPS).to(DEV).train()
    for bn in (ours, stock):
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    at = ops.LAUNCHES[0]
    with torch.no_grad():
        for x in batches:
            xd = x.to(DEV)
            y = call(ours, xd, torch.zeros_like(xd))
            ys = stock(xd.view(xd.shape[0], C, 1, 1))
        mean, var, _ = CR.batch_stats(batches[-1])
        act = torch.relu if node != "wide" else nn.functional.silu
        want_y = act((batches[-1].double() - mean) / torch.sqrt(var + EPS))
        assert float((y.cpu().double() - want_y).abs().max()) <= 1e-5 * float(want_y.abs().max())
        assert ys.shape[0] == y.shape[0]
    assert ops.LAUNCHES[0] - at == 6 * (2 if node == "narrow" else 1), "the node left the HIP path"      # (C-ABI calls: forward [+ running statistics])
    assert int(ours.num_batches_tracked) == int(stock.num_batches_tracked) == 6
    ref = dict(zip(("running_mean", "running_var"), CR.cma(batches, rm0, rv0)[:2]))
    for name, want in ref.items():
        scale = float(want.abs().max())
        d_o = float((getattr(ours, name).double().cpu() - want).abs().max()) / scale
        d_t = float((getattr(stock, name).double().cpu() - want).abs().max()) / scale
        print(f"momentum=None {node} C={C} {name}: ours {d_o:.3e}  stock fp32 {d_t:.3e}  bound {max(2 * d_t, ULP4):.3e}  (of max|ref| = {scale:.3e})")
        assert d_o <= max(2 * d_t, ULP4), f"{name}: deviates by {d_o:.3e}, torch by {d_t:.3e}"


def test_a_batchnorm_without_its_counter_is_refused():
    bn = nn.BatchNorm2d(32, momentum=None).to(DEV).train()
    bn.num_batches_tracked = None
    with pytest.raises(_lib.FdError, match="num_batches_tracked"):
        T.batchnorm_train_rows(bn, torch.randn(64, 32, device=DEV))


# ------------------------------------------------------------------------------------------------ capture
class _Stack(nn.Module):
    """narrow -> wide -> residual, every BatchNorm with momentum=None, on [rows, 32] maps."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.bns = nn.ModuleList(nn.BatchNorm2d(32, momentum=None, eps=EPS) for _ in range(3))
        for bn in self.bns:
            bn.weight.data.copy_(torch.rand(32, generator=g) + 0.5)
            bn.bias.data.copy_(torch.randn(32, generator=g) * 0.1)

    def forward(self, x):
        t = T.batchnorm_train_rows(self.bns[0], x, _lib.ACT_RELU)
        t = T._bn_wide_rows(self.bns[1], t, _lib.ACT_SILU)
        return T.batchnorm_train_res_rows(self.bns[2], t, x, _lib.ACT_RELU)


def test_a_captured_forward_follows_the_counter():
    g = torch.Generator().manual_seed(5)
    inputs = [(torch.randn(300, 32, generator=g) * (1 + k) + k).to(DEV) for k in range(5)]
    captured, eager = _Stack().to(DEV).train(), _Stack().to(DEV).train()
    with torch.no_grad():
        want_y = [eager(x).clone() for x in inputs]
        static = inputs[0].clone()
        captured(static)                                  # one eager forward first
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = captured(static)
        torch.cuda.current_stream().wait_stream(side)
        # (capturing enqueues nothing: the counters still say 1)
        assert [int(bn.num_batches_tracked) for bn in captured.bns] == [1, 1, 1]
        for k in range(1, 5):
            static.copy_(inputs[k])
            graph.replay()
            assert torch.equal(out, want_y[k]), f"replay {k}: the output differs from the eager call"
    torch.cuda.synchronize()
    for a, b in zip(captured.bns, eager.bns):
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 5
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    # against the float64 restatement of the first layer: the factor did not freeze at capture time (1 / 2 for ever would not give the mean)
    rm, rv, _ = CR.cma([x.cpu() for x in inputs], torch.zeros(32), torch.ones(32))
    assert float((captured.bns[0].running_mean.double().cpu() - rm).abs().max()) <= 16 * 2.0 ** -23 * float(rm.abs().max())
    assert float((captured.bns[0].running_var.double().cpu() - rv).abs().max()) <= 16 * 2.0 ** -23 * float(rv.abs().max())
