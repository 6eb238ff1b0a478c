"""The float64 rank-set BatchNorm of tests/layer_ref.py (bn_sync_fwd / bn_sync_bwd / bn_running) at the shapes of tests/test_syncbn_wide_kernels_gpu.py,
against float64 AUTOGRAD of a plain nn.BatchNorm1d + activation over the ranks' rows concatenated: the GPU tests of the synchronised any-width kernels lean
on the closed forms, this file holds the closed forms against an independent statement of the same maths.  No GPU.

Tolerance: both sides are float64 and differ in the order of sums over at most 338 rows, i.e. by a few hundred roundings of 1.1e-16 relative to the largest
term; 1e-11 of the tensor's maximum leaves three decades."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R

EPS, MOM = 1e-3, 0.01
SHARDS = (300, 37, 1)            # a one-row rank included
ACTS = {"none": R.ACT_NONE, "relu": R.ACT_RELU, "silu": R.ACT_SILU}


def _close(got, ref, what):
    bar = 1e-11 * (float(ref.abs().max()) + 1e-300)
    err = float((got - ref).abs().max())
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("C", [40, 144, 260])
def test_rank_set_closed_forms_match_float64_autograd(C, act):
    gen = torch.Generator().manual_seed(17 * C + len(act))
    xs = [(torch.randn(r, C, generator=gen) * (torch.rand(C, generator=gen) + 0.5) + torch.randn(C, generator=gen)).double() for r in SHARDS]
    dys = [torch.randn(r, C, generator=gen).double() for r in SHARDS]
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).double(), (torch.randn(C, generator=gen) * 0.3).double()
    rmean, rvar = (torch.randn(C, generator=gen) * 0.1).double(), (torch.rand(C, generator=gen) + 0.5).double()

    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rmean), bn.running_var.copy_(rvar)
    x = torch.cat(xs, 0).clone().requires_grad_(True)
    z = bn(x)
    y = F.relu(z) if act == "relu" else (F.silu(z) if act == "silu" else z)
    y.backward(torch.cat(dys, 0))
    if act == "relu":
        assert float(z.detach().abs().min()) > 0.0              # (no pre-activation ON the kink, where the two derivatives are conventions)

    ys, mean, var, n = R.bn_sync_fwd(xs, gamma, beta, EPS, ACTS[act])
    per_rank = R.bn_sync_bwd(xs, dys, gamma, beta, EPS, ACTS[act])
    assert n == sum(SHARDS) and len(ys) == len(per_rank) == len(SHARDS)
    r0 = 0
    for r, rows in enumerate(SHARDS):
        _close(ys[r], y.detach()[r0:r0 + rows], f"y of rank {r}")
        _close(per_rank[r][0], x.grad[r0:r0 + rows], f"dx of rank {r}")
        r0 += rows
    _close(sum(p[1] for p in per_rank), bn.weight.grad, "dgamma summed over the ranks")
    _close(sum(p[2] for p in per_rank), bn.bias.grad, "dbeta summed over the ranks")
    rm, rv = R.bn_running(rmean, rvar, mean, var, n, MOM)
    _close(rm, bn.running_mean, "running_mean")
    _close(rv, bn.running_var, "running_var")
    assert int(bn.num_batches_tracked) == 1
