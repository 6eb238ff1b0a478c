"""optim.update_bn on whole models (2 x 3 x 128 x 128, the smallest input the stride-128 level admits; 3 batches):

  a. HalfInvertedStageFCOS as constructed: frozen backbone, the FPN BatchNorms on batch statistics
  b. the same with bn_freeze=False + enable_trunk_batch_stats() (and enable_stem_training(), which the train forward of such a model needs under
     FD_STRICT): the ResNet trunk on batch statistics too, stem included
  c. FCOS(efficientnet=True, backbone_number=0, freeze_bn=False).enable_training(train_stem=True, batch_stats=True)
  and optim.update_bn(loader, avg) on an optim.AveragedModel of (a) after two EMA updates.

For each: the call enqueues per batch exactly the C-ABI launches of an ordinary float-momentum train forward (no layer left the HIP path); every running
tensor that a train forward moves equals the float64 arithmetic mean of the per-batch statistics -- obtained on a twin, each batch alone through the existing
float-momentum path with momentum = 1.0 -- within 4 * k * 2^-24 * max_j |b_j| per channel, k = 3 batches (one fp32 rounding of the blend and one of the
factor per step, carried with weight <= 1: <= 3k * 2^-24 * M; the factor 4 is the margin; a layer that a forward applies twice, fpn.gn2 on two pyramid
levels, takes two blend steps per batch, so its k is 6 and its b_j are the statistics of all six applications); every other BatchNorm is bit-equal to before; momenta and modes are
restored; an eval forward after the call is bit-equal to a fresh model loaded from the state dict (plans and folds re-packed).

Two gloo ranks on one GPU (fresh child processes, as tests/test_effnet_syncbn_gpu.py): a four-layer nn.SyncBatchNorm stack under optim.update_bn, different
rows per rank: both ranks end bit-identical, within the same bound of the float64 restatement (tests/bn_cma_ref.py) over the concatenated rows."""
import copy
import os
import tempfile
import warnings

import pytest
import torch
import torch.nn as nn

import bn_cma_ref as CR
from effnet_init import init_effnet
from pytorch_object_detection_amd import _lib, ops, optim
from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd.model.od import FCOS, HalfInvertedStageFCOS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 3


def tol(k):
    """4 * k * 2^-24 for k blend steps."""
    return 4 * k * 2.0 ** -24


TOL = tol(K)


def _build(cfg):
    if cfg == "hisfcos":
        return HalfInvertedStageFCOS([512, 1024, 2048], 20, 64)
    if cfg == "hisfcos_trunk":
        # (enable_stem_training: with bn_freeze=False the 7x7 stem trains too, and only that switch puts it on the HIP node -- without it the train forward
        # raises under FD_STRICT, on any statistics; with it the stem's bn1 runs on batch statistics as well)
        return HalfInvertedStageFCOS([512, 1024, 2048], 20, 64, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats()
    model = FCOS([320, 112, 40], 20, 64, freeze_bn=False, efficientnet=True, backbone_number=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return model.enable_training(train_stem=True, batch_stats=True)


def _model(cfg, seed=0):
    torch.manual_seed(seed)
    model = _build(cfg)
    if cfg == "effnet":
        init_effnet(model.backbone, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
            m.num_batches_tracked.fill_(11)
    return model.to(DEV)


def _batches():
    g = torch.Generator().manual_seed(17)
    return [(torch.randn(2, 3, 128, 128, generator=g) * (1.0 + 0.25 * k) + 0.1 * k).to(DEV) for k in range(K)]


def _bns(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)}


def _state(model):
    return {n: (m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone(), m.momentum, m.training) for n, m in _bns(model).items()}


def _same(a, b):
    return all(torch.equal(s, t) for grp, want in zip(a, b) for s, t in zip(grp, want))


def _check(cfg, root, call, loader_of=lambda xs: xs):
    """root: the detector whose BatchNorms are looked at; call(loader): optim.update_bn on it or on its wrapper."""
    assert T.STRICT
    batches = _batches()
    root.eval()
    y_before = [[t.clone() for t in grp] for grp in root(batches[0])]            # plans and folds exist before the call
    # ---- a twin: the launches of an ordinary float-momentum train forward, and the per-batch statistics (momentum = 1.0, each batch alone)
    twin = copy.deepcopy(root).train()
    with torch.no_grad():
        twin(batches[0])                                                          # (the first forward packs weights)
        nbt = {n: int(m.num_batches_tracked) for n, m in _bns(twin).items()}
        at = ops.LAUNCHES[0]
        twin(batches[0])
        per_forward = ops.LAUNCHES[0] - at
        runs = {n for n, m in _bns(twin).items() if int(m.num_batches_tracked) != nbt[n]}      # the BatchNorms a train forward runs on batch statistics
        assert runs and all(_bns(twin)[n].training for n in runs) and per_forward > 0
        for n in runs:
            _bns(twin)[n].momentum = 1.0
        # momentum = 1.0 leaves the batch statistics themselves in the running tensors: read them after EVERY application (fpn.gn2 normalises two levels
        # per forward: two blend steps per batch), by wrapping the three node functions for the twin's forwards
        names = {id(m): n for n, m in _bns(twin).items()}
        stats = {n: ([], []) for n in runs}
        nodes = ("batchnorm_train_rows", "batchnorm_train_wide_rows", "batchnorm_train_res_rows")
        plain = {f: getattr(T, f) for f in nodes}

        def recording(fn):
            def wrapper(bn, *args, **kw):
                y = fn(bn, *args, **kw)
                stats[names[id(bn)]][0].append(bn.running_mean.double().cpu())
                stats[names[id(bn)]][1].append(bn.running_var.double().cpu())
                return y
            return wrapper

        try:
            for f in nodes:
                setattr(T, f, recording(plain[f]))
            for x in batches:
                twin(x)
        finally:
            for f in nodes:
                setattr(T, f, plain[f])
        assert all(len(stats[n][0]) % K == 0 and len(stats[n][0]) >= K for n in runs)
    with torch.no_grad():                                                         # (the model's own weights are packed too before launches are counted)
        root.train()(batches[0])
    # what train() leaves in training mode is reset; of that, what a forward never runs (fpn.gn3, the EfficientNet's _bn1: built for checkpoint parity)
    # stays reset, as with the stock function; everything else is frozen and must not move
    selected = {n for n, m in _bns(root).items() if m.training and m.track_running_stats}
    root.eval()
    before = _state(root)
    frozen, idle = set(before) - selected, selected - runs
    assert runs <= selected
    if cfg == "hisfcos":
        assert frozen == {n for n in before if n.startswith("backbone.")} and idle == {"fpn.gn3"}
    if cfg == "hisfcos_trunk":
        assert sum(n.startswith("backbone.") for n in runs) == 53 and not frozen and idle == {"fpn.gn3"}
    if cfg == "effnet":
        assert sum(n.startswith("backbone.") for n in runs) == 48 and not frozen and idle == {"backbone.model._bn1"}

    # ---- the call, with the launches between the loader's yields
    marks = []

    def loader():
        for x in batches:
            marks.append(ops.LAUNCHES[0])
            yield x
        marks.append(ops.LAUNCHES[0])

    T.STATS["stock_fallbacks"] = 0
    call(loader_of(loader()))
    per_batch = [b - a for a, b in zip(marks, marks[1:])]
    assert len(per_batch) == K and per_batch == [per_forward] * K, f"launches per batch {per_batch}, an ordinary train forward: {per_forward}"
    assert T.STATS["stock_fallbacks"] == 0, "a layer left the HIP path"
    assert root.training is False

    # ---- the arithmetic mean of the per-batch statistics; untouched layers; restored state
    worst = 0.0
    for n, m in _bns(root).items():
        rm, rv, nb, momentum, training = before[n]
        assert m.momentum == momentum and m.training is training, n
        if n in frozen:
            assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv) and torch.equal(m.num_batches_tracked, nb), f"{n}: a frozen layer moved"
            continue
        if n in idle:
            assert bool((m.running_mean == 0).all()) and bool((m.running_var == 1).all()) and int(m.num_batches_tracked) == 0, f"{n}: not left reset"
            continue
        k = len(stats[n][0])                                                      # blend steps: K, or 2 K for a layer applied twice per forward
        assert int(m.num_batches_tracked) == k, n
        for got, per in ((m.running_mean, stats[n][0]), (m.running_var, stats[n][1])):
            b = torch.stack(per)
            want, scale = b.mean(0), b.abs().max(0).values.clamp_min(1e-300)
            err = (got.double().cpu() - want).abs() / scale
            worst = max(worst, float(err.max()) / k)
            assert bool((err <= tol(k)).all()), f"{n}: off the arithmetic mean by {float(err.max()):.3e} of max|b| (bound {tol(k):.3e}, {k} steps)"
    print(f"update_bn {cfg}: {len(runs)} BatchNorms updated, {len(frozen)} untouched, {per_forward} launches per batch, "
          f"worst |r - mean b| / max|b| per step = {worst:.3e} (bound {tol(1):.3e} per step)")

    # ---- plans and folds re-packed: the eval forward is that of a fresh model holding the state dict
    y_after = [[t.clone() for t in grp] for grp in root(batches[0])]
    fresh = _build(cfg).to(DEV).eval()
    fresh.load_state_dict(root.state_dict())
    assert _same(fresh(batches[0]), y_after)
    assert not _same(y_after, y_before)


@pytest.mark.parametrize("cfg", ["hisfcos", "hisfcos_trunk", "effnet"])
def test_update_bn_on_the_detectors(cfg):
    model = _model(cfg)
    _check(cfg, model, lambda loader: optim.update_bn(loader, model))


def test_update_bn_on_an_averaged_model():
    """The main use: the averaged copy's batch-statistics BatchNorms after two EMA updates, batches as [input, target] lists; the source model stays."""
    model = _model("hisfcos")
    avg = optim.AveragedModel(model, decay=0.9)
    g = torch.Generator(device=DEV).manual_seed(3)
    with torch.no_grad():
        for _ in range(2):
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g, device=DEV) * 1e-3)
            avg.update_parameters(model)
    src = {k: v.clone() for k, v in model.state_dict().items()}
    src_momenta = [m.momentum for m in _bns(model).values()]
    avg.eval()
    _check("hisfcos", avg.module, lambda loader: optim.update_bn(loader, avg), loader_of=lambda xs: ([x, None] for x in xs))
    assert int(avg.n_averaged) == 2 and avg.training is False
    now = model.state_dict()
    assert all(torch.equal(src[k], now[k]) for k in src) and [m.momentum for m in _bns(model).values()] == src_momenta


# ================================================================================================ two ranks
C = 32
ROWS = ((200, 64, 333), (120, 301, 2))          # rows of batch j on rank r: different on every rank and batch


class _SyncStack(nn.Module):
    """narrow -> wide -> residual -> narrow on [rows, 32] maps: both kernel families, plain and residual."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(31)
        self.bns = nn.ModuleList(nn.SyncBatchNorm(C, eps=1e-3) for _ in range(4))
        for bn in self.bns:
            bn.weight.data.copy_(torch.rand(C, generator=g) + 0.5)
            bn.bias.data.copy_(torch.randn(C, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(C, generator=g))
        self.seen = None                          # a list: every layer's input rows of every forward

    def forward(self, x):
        t0 = T.batchnorm_train_rows(self.bns[0], x, _lib.ACT_RELU)
        t1 = T._bn_wide_rows(self.bns[1], t0, _lib.ACT_SILU)
        t2 = T.batchnorm_train_res_rows(self.bns[2], t1, x, _lib.ACT_RELU)
        t3 = T.batchnorm_train_rows(self.bns[3], t2, _lib.ACT_NONE)
        if self.seen is not None:
            self.seen.append([t.cpu() for t in (x, t0, t1, t2)])
        return t3


def _rank_batches(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return [torch.randn(rows, C, generator=g) * (1.0 + 0.5 * j) + 0.2 * j - rank for j, rows in enumerate(ROWS[rank])]


def _rank_worker(rank, world, init_file, out_dir):
    import torch.distributed as dist
    from pytorch_object_detection_amd import optim as O
    from pytorch_object_detection_amd import train_ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        net = _SyncStack().to(dev).eval()
        net.seen = []
        assert all(bn.momentum == 0.1 for bn in net.bns)
        O.update_bn(_rank_batches(rank), net, device=dev)
        assert all(bn.momentum == 0.1 and not bn.training for bn in net.bns) and not net.training
        torch.save({"rm": [bn.running_mean.cpu() for bn in net.bns], "rv": [bn.running_var.cpu() for bn in net.bns],
                    "nbt": [int(bn.num_batches_tracked) for bn in net.bns], "seen": net.seen, "fallbacks": train_ops.STATS["stock_fallbacks"]},
                   os.path.join(out_dir, f"r{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_end_with_identical_global_statistics():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_rank_worker, args=(2, os.path.join(tmp, "rdzv"), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, f"r{i}.pt")) for i in range(2)]
    for key in ("rm", "rv"):
        assert all(torch.equal(a, b) for a, b in zip(r[0][key], r[1][key])), f"{key}: the ranks differ"
    assert r[0]["nbt"] == r[1]["nbt"] == [K] * 4 and r[0]["fallbacks"] == r[1]["fallbacks"] == 0
    for rank in range(2):                         # every rank passed its own shard
        assert all(torch.equal(seen[0], x) for seen, x in zip(r[rank]["seen"], _rank_batches(rank)))
    for layer in range(4):                        # the restatement over the concatenated rows each layer saw
        rm, rv, n = CR.update_bn_ref([torch.cat([r[0]["seen"][j][layer], r[1]["seen"][j][layer]], 0) for j in range(K)])
        per = [CR.batch_stats(torch.cat([r[0]["seen"][j][layer], r[1]["seen"][j][layer]], 0)) for j in range(K)]
        assert n == K
        for got, want, scale in ((r[0]["rm"][layer], rm, torch.stack([p[0] for p in per]).abs().max(0).values),
                                 (r[0]["rv"][layer], rv, torch.stack([p[2] for p in per]).abs().max(0).values)):
            err = (got.double() - want).abs()
            print(f"two ranks, layer {layer}: worst |r - mean b| / max|b| = {float((err / scale).max()):.3e} (bound {TOL:.3e})")
            assert bool((err <= TOL * scale).all()), (layer, float((err / scale).max()))
