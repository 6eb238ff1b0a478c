"""The closed-form float64 references of tests/layer_ref.py against torch float64 autograd / nn modules on the CPU, at the shapes the
GPU tests (test_layer_views_gpu.py, test_syncbn_kernels_gpu.py) use.  Agreement is to float64 rounding."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
from layer_ref import ACT_EXP, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU

PYR = [(7, 10), (2, 3), (1, 1)]


def eq(a, b, rtol=1e-12, atol=1e-12):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def t_act(x, act, p):
    return {ACT_NONE: lambda v: v, ACT_RELU: F.relu, ACT_SILU: F.silu, ACT_EXP: lambda v: torch.exp(v * p), ACT_SIGMOID: torch.sigmoid}[act](x)


@pytest.mark.parametrize("act,p", [(ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_SILU, 0.0), (ACT_EXP, 1.0), (ACT_EXP, 0.37), (ACT_SIGMOID, 0.0)])
def test_activations_and_derivatives(act, p):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(50, 24, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    y = t_act(x, act, p)
    y.backward(torch.ones_like(y))
    eq(R.act_fwd(x, act, p), y.detach())
    eq(R.act_deriv(x, act, p), x.grad)


@pytest.mark.parametrize("k,s,pad", [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize("H,W", [(11, 14), (5, 7)])
def test_maxpool_with_tied_maxima(k, s, pad, H, W):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, H, W, 8, generator=g, dtype=torch.float64).round(decimals=1)        # ties exist
    xr = nchw(x).clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, pad)
    add = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y + add).backward(dy)
    got, idx = R.maxpool_fwd(x, k, s, pad, nhwc(add))
    assert torch.equal(got, nhwc((y + add).detach()))
    eq(R.maxpool_bwd(x, nhwc(dy), k, s, pad), nhwc(xr.grad))
    # there ARE tied windows, and the index is the first of the tied positions
    _, tidx = F.max_pool2d(nchw(x), k, s, pad, return_indices=True)
    assert torch.equal(idx, nhwc(tidx))
    xp = F.pad(nchw(x), (pad, pad, pad, pad), value=float("-inf"))
    win = xp.unfold(2, k, s).unfold(3, k, s).reshape(*y.shape, k * k)
    assert int(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).sum()) > 0


def test_upsample2x_add_and_block_sum():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, 8, generator=g, dtype=torch.float64)
    lat = torch.randn(2, 10, 14, 8, generator=g, dtype=torch.float64)
    dy = torch.randn(2, 10, 14, 8, generator=g, dtype=torch.float64)
    xr = nchw(x).clone().requires_grad_(True)
    y = F.interpolate(xr, scale_factor=2, mode="nearest") + nchw(lat)
    y.backward(nchw(dy))
    eq(R.upsample2x_add(x, lat), nhwc(y.detach()))
    eq(R.upsample2x_bwd(dy), nhwc(xr.grad))


@pytest.mark.parametrize("K,dil", [(3, 1), (5, 2), (7, 1), (3, 8)])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU])
def test_dwconv_same_padding_over_the_pyramid(K, dil, act):
    g = torch.Generator().manual_seed(4)
    B, C = 2, 4
    w = torch.randn(K * K, C, generator=g, dtype=torch.float64)
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(C, generator=g, dtype=torch.float64)
    wt = w.t().reshape(C, 1, K, K).clone().requires_grad_(True)
    for H, W in PYR:
        x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
        dy = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
        xr = nchw(x).clone().requires_grad_(True)
        wt.grad = None
        z = F.conv2d(xr, wt, None, 1, dil * (K - 1) // 2, dil, C) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        y = t_act(z, act, 0.0)
        y.backward(nchw(dy))
        eq(R.dwconv_fwd(x, w, K, dil, scale=scale, shift=shift, act=act), nhwc(y.detach()))
        dx, dw = R.dwconv_bwd(x, w, dy, K, dil, scale=scale, shift=shift, act=act)
        eq(dx, nhwc(xr.grad))
        eq(dw, wt.grad.reshape(C, K * K).t())
    # the pyramid weight gradient (no activation, scale outside) is the sum over the levels
    xs = [torch.randn(B, H, W, C, generator=g, dtype=torch.float64) for H, W in PYR]
    dys = [torch.randn(B, H, W, C, generator=g, dtype=torch.float64) for H, W in PYR]
    wt.grad = None
    for x, dy in zip(xs, dys):
        F.conv2d(nchw(x), wt, None, 1, dil * (K - 1) // 2, dil, C).backward(nchw(dy))
    eq(R.dwconv_wgrad_pyramid(R.join_levels(xs), R.join_levels(dys), B, PYR, K, dil, scale), wt.grad.reshape(C, K * K).t() * scale)


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv2d_asymmetric_padding(K, stride):
    g = torch.Generator().manual_seed(5)
    B, H, W, C = 2, 7, 10, 4
    pt, pb, pl, pr = (K - 1) // 2, K // 2 + 1, (K - 1) // 2 - 1, K // 2           # pad_top != pad_bottom, pad_left != pad_right
    Ho, Wo = (H + pt + pb - K) // stride + 1, (W + pl + pr - K) // stride + 1
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(K * K, C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, Ho, Wo, C, generator=g, dtype=torch.float64)
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(C, generator=g, dtype=torch.float64)
    xr = nchw(x).clone().requires_grad_(True)
    wt = w.t().reshape(C, 1, K, K).clone().requires_grad_(True)
    y = F.silu(F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wt, None, stride, 0, 1, C) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    assert y.shape[2:] == (Ho, Wo)
    y.backward(nchw(dy))
    eq(R.dwconv_fwd(x, w, K, 1, stride, pt, pl, Ho, Wo, scale, shift, ACT_SILU), nhwc(y.detach()))
    dx, dw = R.dwconv_bwd(x, w, dy, K, 1, stride, pt, pl, scale, shift, ACT_SILU)
    eq(dx, nhwc(xr.grad))
    eq(dw, wt.grad.reshape(C, K * K).t())


GN_CASES = [(256, (7, 10), 64), (256, (7, 10), 1), (8, (7, 10), 8), (8, (1, 1), 2), (1024, (2, 3), 256), (16, (1, 1), 4), (16, (1, 1), 1)]


@pytest.mark.parametrize("C,hw,G", GN_CASES)
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU])
def test_groupnorm_act_forward_backward(C, hw, G, act):
    g = torch.Generator().manual_seed(6)
    B, (H, W) = 2, hw
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    dy = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    gn = torch.nn.GroupNorm(G, C).double()
    with torch.no_grad():
        gn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
        gn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.2)
    xr = nchw(x).clone().requires_grad_(True)
    y = t_act(gn(xr), act, 0.0)
    y.backward(nchw(dy))
    eq(R.gn_fwd(x, gn.weight, gn.bias, G, gn.eps, act), nhwc(y.detach()))
    dx, dgamma, dbeta = R.gn_bwd(x, dy, gn.weight, gn.bias, G, gn.eps, act)
    eq(dx, nhwc(xr.grad))
    eq(dgamma, gn.weight.grad)
    eq(dbeta, gn.bias.grad)
    a, b = R.gn_coef(x, gn.weight, gn.bias, G, gn.eps)
    eq(R.act_fwd(x * a.view(B, 1, 1, C) + b.view(B, 1, 1, C), act), nhwc(y.detach()))


def test_groupnorm_reference_is_well_conditioned_at_mean_100_std_001():
    """The variance 1e-4 under a mean of 100: the two-pass float64 reference keeps it (relative error of the statistics ~1e-12), stays finite,
    and agrees with nn.GroupNorm in float64 to 1e-7 of the normalised values (nn.GroupNorm's own one-pass variance loses ~1e-8 there)."""
    g = torch.Generator().manual_seed(7)
    B, H, W, C, G = 2, 7, 10, 256, 64
    x = (torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 0.01 + 100.0).float().double()       # fp32-representable, as the kernel sees it
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    mean, rstd = R.gn_stats(x, G, 1e-5)
    var = 1.0 / rstd ** 2 - 1e-5
    assert torch.isfinite(rstd).all() and float(var.min()) > 5e-5 and float(var.max()) < 2e-4
    y = R.gn_fwd(x, gamma, beta, G, 1e-5, ACT_NONE)
    assert torch.isfinite(y).all() and float(((y - beta) / gamma).abs().max()) < 6.0
    ref = F.group_norm(nchw(x), G, gamma, beta, 1e-5)
    eq(y, nhwc(ref), rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("C,Cr", [(16, 4), (144, 6), (128, 32)])
@pytest.mark.parametrize("HW", [1, 35])
def test_se_scale_forward_backward(C, Cr, HW):
    g = torch.Generator().manual_seed(8)
    N = 3
    x = torch.randn(N, HW, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, HW, C, generator=g, dtype=torch.float64)
    ps = [torch.randn(Cr, C, generator=g, dtype=torch.float64) / C ** 0.5, torch.randn(Cr, generator=g, dtype=torch.float64) * 0.1,
          torch.randn(C, Cr, generator=g, dtype=torch.float64) / Cr ** 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.1]
    xr = x.clone().requires_grad_(True)
    w1, b1, w2, b2 = [p.clone().requires_grad_(True) for p in ps]
    gate = torch.sigmoid(F.linear(F.silu(F.linear(xr.mean(1), w1, b1)), w2, b2))
    y = xr * gate.unsqueeze(1)
    y.backward(dy)
    got, gt = R.se_fwd(x, *ps)
    eq(got, y.detach())
    eq(gt, gate.detach())
    for a, b in zip(R.se_bwd(x, dy, *ps), (xr.grad, w1.grad, b1.grad, w2.grad, b2.grad)):
        eq(a, b)


@pytest.mark.parametrize("shards", [(37,), (37, 5), (37, 5, 1)])
@pytest.mark.parametrize("C", [4, 64, 1024])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU])
def test_batchnorm_over_ranks(shards, C, act):
    """The rank-set reference against nn.BatchNorm1d on the concatenated rows: y and dx are the whole-batch ones cut into shards, the ranks'
    dgamma / dbeta (local sums) ADD UP to the whole-batch gradients, the running statistics are nn.BatchNorm's."""
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(r, C, generator=g, dtype=torch.float64) * 2 + 0.3 for r in shards]
    dys = [torch.randn(r, C, generator=g, dtype=torch.float64) for r in shards]
    bn = torch.nn.BatchNorm1d(C, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5); bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.1)
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64) * 0.1); bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    xr = torch.cat(xs).requires_grad_(True)
    y = t_act(bn(xr), act, 0.0)
    y.backward(torch.cat(dys))
    ys, mean, var, n = R.bn_sync_fwd(xs, bn.weight, bn.bias, bn.eps, act)
    assert n == sum(shards)
    eq(torch.cat(ys), y.detach())
    outs = R.bn_sync_bwd(xs, dys, bn.weight, bn.bias, bn.eps, act)
    eq(torch.cat([o[0] for o in outs]), xr.grad)
    eq(sum(o[1] for o in outs), bn.weight.grad)
    eq(sum(o[2] for o in outs), bn.bias.grad)
    rm, rv = R.bn_running(rm0, rv0, mean, var, n, 0.1)
    eq(rm, bn.running_mean)
    eq(rv, bn.running_var)


def test_pyramid_split_and_join_round_trip():
    rows = torch.arange(2 * (70 + 6 + 1) * 4, dtype=torch.float64).view(-1, 4)
    lv = R.split_levels(rows, 2, PYR)
    assert [tuple(t.shape) for t in lv] == [(2, 7, 10, 4), (2, 2, 3, 4), (2, 1, 1, 4)]
    assert torch.equal(R.join_levels(lv), rows)
