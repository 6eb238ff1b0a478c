"""The channel-view contract of the layer kernels (csrc/fd_layers.hip, fd_dwconv2d_nhwc): every map is a view (ptr, cs, co, C) -- C channels
from channel `co` of a buffer with `cs` channels per row -- and the plan builder hands these kernels slices of shared buffers everywhere.

Every kernel runs on contiguous operands and then with EVERY operand on its own view geometry (distinct co from {0, 4, 8, 12}, distinct cs,
tail >= 4, NaN in all neighbour channels of inputs and outputs), in one assignment per operand that puts THAT operand on co = 0 with cs > C and
the others on co > 0 (so inputs and outputs each meet both):
  (a) the view result is BIT-IDENTICAL to the contiguous one: cs / co enter only the address computation of these kernels, work partition and
      summation order depend on rows, H, W, C, G alone -- no kernel was found where the order depends on the view, so (a) holds for all;
  (b) nothing outside an output view is written and no input buffer changes (bitwise);
  (c) the aliasing forms of the plans: output = another channel slice of the input's buffer (all kernels), output = the input view itself
      (the kernels the plans run in place: groupnorm_act, groupnorm_apply, coef_apply, act, se_scale);
  (d) the contiguous result against the float64 reference of tests/layer_ref.py (tolerances below), for every kernel -- the first direct
      check of upsample2x_bwd, se_scale_bwd, groupnorm_act_bwd, act / act_bwd with EXP and SIGMOID, nhwc_to_nchw.
Illegal views and widths must raise FdError before any launch and leave NaN-prefilled outputs untouched."""
import numpy as np
import pytest
import torch

import layer_ref as R
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import ACT_EXP, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, FdError, Segs

pytestmark = pytest.mark.gpu
DEV = R.DEV
ATOL, RTOL = 1e-4, 1e-5                 # outputs: the bar of test_layers_gpu.py
GRAD, PGRAD = 2e-5, 5e-5                # gradients / parameter gradients relative to the largest reference magnitude: close() of test_train_nodes_gpu.py
NAN = float("nan")
GEOMS = [(0, 4), (4, 4), (8, 4), (12, 4)]       # (co, tail) per operand: cs = C + 4, C + 8, C + 12, C + 16
PYR = [(7, 10), (2, 3), (1, 1)]                  # a level of one pixel and one smaller than a dilated footprint
EPS = 1e-5


def close(a, b, tol):
    s = float(b.abs().max()) + 1e-12
    np.testing.assert_allclose(a.double().cpu().numpy() / s, b.numpy() / s, atol=tol)


def check_ref(got, ref, how):
    if how == "exact":
        assert torch.equal(got.cpu(), ref.to(got.dtype))
    elif how == "out":
        np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=ATOL, rtol=RTOL)
    elif how == "grad":
        close(got, ref, GRAD)
    elif how == "pgrad":
        close(got, ref, PGRAD)
    else:
        how(got, ref)


class Case:
    """ins: name -> CPU [rows, C] tensor; outs: name -> rows (NaN-prefilled [rows, C] views); run(v) launches on the name -> ops.Rows map and
    returns further results (device tensors that are no views); ref() -> name -> (float64 reference, "exact" | "out" | "grad" | "pgrad" | fn).
    prep(v, launch) -> state: the calls that must precede the one under test (the forward that fills a backward's workspace); run is then
    run(v, state).  The rejection trials run prep on LEGAL views (launch=False: allocate only, for a width the forward itself refuses), so that the
    call that raises is the entry point under test."""

    def __init__(self, C, ins, outs, run, ref=None, alias=None, inplace=None, dtype=torch.float32, reject=("co", "cs"), prep=None):
        self.C, self.ins, self.outs, self.ref, self.alias, self.inplace, self.dtype, self.reject, self.prep = C, ins, outs, ref, alias, inplace, dtype, reject, prep
        self.run = run if prep is not None else (lambda v, state=None: run(v))


class BadRows:
    """An ops.Rows look-alike that may describe an illegal view (ops.Rows itself refuses to)."""

    def __init__(self, buf, co, cs, C):
        self.buf, self.co, self.cs, self.C, self.rows, self.ptr, self.f16 = buf, co, cs, C, buf.shape[0], buf.data_ptr(), buf.dtype == torch.float16


def rnd(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen).to(dtype)


def launch(case, geoms, alias=False, inplace=False):
    """Place every operand (geoms: name -> (co, tail)), run, assert (b), return name -> result."""
    v, bufs = {}, {}
    names = list(case.ins) + list(case.outs)
    shared = set()
    if alias:                   # first name = buf[:, 0:C], second = buf[:, C + 4 : 2C + 4] of ONE buffer
        a, b = case.alias
        ra = case.ins[a].shape[0]
        rb = case.ins[b].shape[0] if b in case.ins else case.outs[b]
        buf = torch.full((max(ra, rb), 2 * case.C + 8), NAN, dtype=case.dtype, device=DEV)
        buf[:ra, :case.C] = case.ins[a].to(DEV)
        if b in case.ins:
            buf[:rb, case.C + 4:2 * case.C + 4] = case.ins[b].to(DEV)
        v[a], v[b] = ops.Rows(buf, 0, case.C), ops.Rows(buf, case.C + 4, case.C)
        bufs[a] = bufs[b] = buf
        shared = {a, b}
    for n in names:
        if n in v:
            continue
        co, tail = geoms[n]
        if n in case.ins:
            v[n], bufs[n] = R.make_view(case.ins[n], co, tail)
        else:
            v[n], bufs[n] = R.make_view(torch.full((case.outs[n], case.C), NAN, dtype=case.dtype), co, tail)
    if inplace:
        a, b = case.inplace
        v[b], bufs[b] = v[a], bufs[a]
        shared = {a, b}
    before = {n: bufs[n].clone() for n in names}
    extras = case.run(v, case.prep(v, True) if case.prep else None) or {}
    torch.cuda.synchronize()
    for n in case.ins:
        if n not in shared:
            assert R.unchanged(bufs[n], before[n]), f"input {n} changed"
    for n, rows in case.outs.items():
        assert R.outside_untouched(bufs[n], v[n].co, case.C, before[n], rows), f"write outside the view of {n}"
    if shared and not any(n in case.outs for n in shared):
        assert R.unchanged(bufs[case.alias[0]], before[case.alias[0]])
    res = {n: v[n].tensor()[:rows].clone() for n, rows in case.outs.items()}
    res.update({k: t.clone() for k, t in extras.items()})
    return res


def same(res, base, what):
    for k in base:
        assert res[k].shape == base[k].shape and torch.equal(res[k], base[k]), f"{what}: {k} differs from the contiguous run " \
            f"(max |diff| {float((res[k].double() - base[k].double()).abs().max())})"


def check_case(case):
    names = list(case.ins) + list(case.outs)
    base = launch(case, {n: (0, 0) for n in names})
    for k, t in base.items():
        assert not torch.isnan(t.float()).any(), f"{k}: NaN in the contiguous result"
    if case.ref is not None:
        for k, (ref, how) in case.ref().items():                                  # (d)
            check_ref(base[k].reshape(ref.shape), ref, how)
    for rot in sorted({(-i) % 4 for i in range(len(names))} | ({1} if len(names) == 1 else set())):     # (a) + (b): each operand in turn on co = 0, cs > C
        same(launch(case, {n: GEOMS[(i + rot) % 4] for i, n in enumerate(names)}), base, f"views (rotation {rot})")
    if case.alias is not None:                                                    # (c) another slice of the same buffer
        same(launch(case, {n: GEOMS[(i + 2) % 4] for i, n in enumerate(names)}, alias=True), base, "slices of one buffer")
    if case.inplace is not None:                                                  # (c) in place
        same(launch(case, {n: GEOMS[(i + 1) % 4] for i, n in enumerate(names)}, inplace=True), base, "in place")
    return base


def check_rejections(build, bad_C):
    """co % 4 != 0 and cs < co + C on each operand in turn, then the unsupported width: FdError, outputs untouched."""
    case = build()
    names = list(case.ins) + list(case.outs)
    trials = [(mode, n) for mode in case.reject for n in names]
    if bad_C is not None:
        trials.append(("C", None))
    for mode, bad in trials:
        c = build(bad_C) if mode == "C" else case
        v, bufs = {}, {}
        for i, n in enumerate(names):
            t = c.ins[n] if n in c.ins else torch.full((c.outs[n], c.C), NAN, dtype=c.dtype)
            if mode == "C":
                v[n], bufs[n] = R.make_view(t, 0, (-c.C) % 4 + 4)
            elif n != bad:
                v[n], bufs[n] = R.make_view(t, *GEOMS[i % 4])
            else:
                _, bufs[n] = R.make_view(t, 0, 8)            # [rows, C + 8]; the declared view: co = 2, or co = 8 in rows of cs = C + 4 < co + C
                v[n] = BadRows(bufs[n], 2, c.C + 8, c.C) if mode == "co" else BadRows(bufs[n], 8, c.C + 4, c.C)
        state = None
        if c.prep is not None:           # the preceding calls on legal views of the same data: only the entry point under test sees the bad one
            state = c.prep({n: R.make_view(t, *GEOMS[i % 4])[0] for i, (n, t) in enumerate(c.ins.items())}, mode != "C")
        before = {n: bufs[n].clone() for n in names}
        with pytest.raises(FdError):
            c.run(v, state)
        torch.cuda.synchronize()
        for n in names:
            assert R.unchanged(bufs[n], before[n]), f"{mode} on {bad}: {n} changed by a rejected call"


# ---------------------------------------------------------------------------------------------------- case builders
def d(t):
    return None if t is None else t.to(DEV)


def pool_case(k, s, pad, H, W, add, C=8):
    gen = torch.Generator().manual_seed(10 * k + H)
    B = 2
    Ho, Wo = R.pool_out(H, k, s, pad), R.pool_out(W, k, s, pad)
    ins = {"x": rnd(gen, B * H * W, C).round(decimals=1)}                        # rounded: tied maxima exist
    if add:
        ins["add"] = rnd(gen, B * Ho * Wo, C)

    def run(v):
        ops.maxpool(v["x"], v["y"], B, H, W, k, s, pad, add=v.get("add"))

    def ref():
        y, _ = R.maxpool_fwd(ins["x"].view(B, H, W, C), k, s, pad, ins["add"].view(B, Ho, Wo, C) if add else None)
        return {"y": (y.reshape(-1, C), "exact")}
    return Case(C, ins, {"y": B * Ho * Wo}, run, ref, alias=("x", "y"))


def pool_bwd_case(k, s, pad, H, W, C=8):
    gen = torch.Generator().manual_seed(20 * k + H)
    B = 2
    Ho, Wo = R.pool_out(H, k, s, pad), R.pool_out(W, k, s, pad)
    ins = {"x": rnd(gen, B * H * W, C).round(decimals=1), "dy": rnd(gen, B * Ho * Wo, C)}

    def run(v):
        ops.maxpool_bwd(v["x"], v["dy"], v["dx"], B, H, W, k, s, pad)

    def ref():
        return {"dx": (R.maxpool_bwd(ins["x"].view(B, H, W, C), ins["dy"].view(B, Ho, Wo, C), k, s, pad).reshape(-1, C), "grad")}
    return Case(C, ins, {"dx": B * H * W}, run, ref, alias=("x", "dx"))


def up_case(C=8):
    gen = torch.Generator().manual_seed(30)
    B, H, W = 2, 5, 7
    ins = {"x": rnd(gen, B * H * W, C), "lat": rnd(gen, B * 4 * H * W, C)}

    def run(v):
        ops.upsample2x_add(v["x"], v["lat"], v["y"], B, H, W)

    def ref():
        return {"y": (R.upsample2x_add(ins["x"].view(B, H, W, C), ins["lat"].view(B, 2 * H, 2 * W, C)).reshape(-1, C), "exact")}
    return Case(C, ins, {"y": B * 4 * H * W}, run, ref, alias=("x", "y"))


def up_bwd_case(C=8):
    gen = torch.Generator().manual_seed(31)
    B, H, W = 3, 5, 7
    ins = {"dy": rnd(gen, B * 4 * H * W, C)}

    def run(v):
        ops.upsample2x_bwd(v["dy"], v["dx"], B, H, W)

    def ref():
        return {"dx": (R.upsample2x_bwd(ins["dy"].view(B, 2 * H, 2 * W, C)).reshape(-1, C), "grad")}
    return Case(C, ins, {"dx": B * H * W}, run, ref, alias=("dy", "dx"))


def dw_params(gen, K, C):
    return rnd(gen, K * K, C) / K, torch.rand(C, generator=gen) + 0.5, rnd(gen, C) * 0.2


def dw3_case(C):
    gen = torch.Generator().manual_seed(40 + C)
    B, segs = 2, Segs.make(2, PYR)
    w, scale, shift = dw_params(gen, 3, C)
    ins = {"x": rnd(gen, segs.rows, C)}
    wd, sc, sf = d(w), d(scale), d(shift)

    def run(v):
        ops.dwconv3x3(v["x"], wd, v["y"], segs, sc, sf, ACT_SILU)

    def ref():
        return {"y": (R.over_levels(lambda t: R.dwconv_fwd(t, w, 3, scale=scale, shift=shift, act=ACT_SILU), ins["x"], B, PYR), "out")}
    return Case(C, ins, {"y": segs.rows}, run, ref, alias=("x", "y"))


def dw3_gn_case(C, G, coef, in_act=ACT_RELU):
    gen = torch.Generator().manual_seed(50 + C + G)
    B, segs = 2, Segs.make(2, PYR)
    w = rnd(gen, 9, C) / 3
    ins = {"x": rnd(gen, segs.rows, C)}
    cf = torch.stack([torch.rand(len(PYR) * B, C, generator=gen) + 0.5, rnd(gen, len(PYR) * B, C) * 0.3], 1).contiguous() if coef else None   # [imgs][2][C]
    wd, cfd = d(w), d(cf)

    def run(v):
        st = torch.full((segs.rows, G, 2), NAN, device=DEV) if G else None
        ops.dwconv3x3_gn(v["x"], wd, v["y"], segs, cfd, in_act, st, G)
        return {"gn_stats": st} if G else {}

    def ref():
        lv = R.split_levels(R.f64(ins["x"]), B, PYR)
        if coef:
            lv = [R.act_fwd(t * R.f64(cf[s * B:(s + 1) * B, 0]).view(B, 1, 1, C) + R.f64(cf[s * B:(s + 1) * B, 1]).view(B, 1, 1, C), in_act) for s, t in enumerate(lv)]
        return {"y": (R.join_levels([R.dwconv_fwd(t, w, 3) for t in lv]), "out")}
    return Case(C, ins, {"y": segs.rows}, run, ref, alias=("x", "y"))


def dwd_case(C, K, dil):
    gen = torch.Generator().manual_seed(60 + C + 7 * K + dil)
    B, segs = 2, Segs.make(2, PYR)
    w, scale, shift = dw_params(gen, K, C)
    ins = {"x": rnd(gen, segs.rows, C)}
    wd, sc, sf = d(w), d(scale), d(shift)

    def run(v):
        ops.dwconv_dilated(v["x"], wd, v["y"], segs, K, dil, sc, sf, ACT_RELU)

    def ref():
        return {"y": (R.over_levels(lambda t: R.dwconv_fwd(t, w, K, dil, scale=scale, shift=shift, act=ACT_RELU), ins["x"], B, PYR), "out")}
    return Case(C, ins, {"y": segs.rows}, run, ref, alias=("x", "y"))


def dw2d_case(C, K, stride):
    gen = torch.Generator().manual_seed(70 + C + 7 * K + stride)
    B, H, W = 2, 7, 10
    pt, pb, pl, pr = (K - 1) // 2, K // 2 + 1, (K - 1) // 2 - 1, K // 2              # pad_top != pad_bottom, pad_left != pad_right
    Ho, Wo = (H + pt + pb - K) // stride + 1, (W + pl + pr - K) // stride + 1
    w, scale, shift = dw_params(gen, K, C)
    ins = {"x": rnd(gen, B * H * W, C)}
    wd, sc, sf = d(w), d(scale), d(shift)

    def run(v):
        ops.dwconv2d(v["x"], wd, v["y"], B, H, W, K, stride, pt, pl, Ho, Wo, sc, sf, ACT_SILU)

    def ref():
        return {"y": (R.dwconv_fwd(ins["x"].view(B, H, W, C), w, K, 1, stride, pt, pl, Ho, Wo, scale, shift, ACT_SILU).reshape(-1, C), "out")}
    return Case(C, ins, {"y": B * Ho * Wo}, run, ref, alias=("x", "y"))


def dw_wgrad_case(C, K, dil, dilated):
    gen = torch.Generator().manual_seed(80 + C + 7 * K + dil)
    B, segs = 2, Segs.make(2, PYR)
    scale = torch.rand(C, generator=gen) + 0.5
    ins = {"x": rnd(gen, segs.rows, C), "dy": rnd(gen, segs.rows, C)}
    sc = d(scale)

    def run(v):
        if dilated:
            return {"dw": ops.dwconv_dilated_wgrad(v["x"], v["dy"], segs, K, dil, sc), "dw_t": ops.dwconv_dilated_wgrad(v["x"], v["dy"], segs, K, dil, None, True)}
        return {"dw": ops.dwconv3x3_wgrad(v["x"], v["dy"], segs, sc), "dw_t": ops.dwconv3x3_wgrad(v["x"], v["dy"], segs, None, True)}

    def ref():
        dw = R.dwconv_wgrad_pyramid(ins["x"], ins["dy"], B, PYR, K, dil)
        return {"dw": (dw * R.f64(scale), "pgrad"), "dw_t": (dw.t().reshape(C, 1, K, K), "pgrad")}
    return Case(C, ins, {}, run, ref, alias=("x", "dy"))


def gn_data(gen, segs, C, hot):
    x = rnd(gen, segs.rows, C)
    return x * 0.01 + 100.0 if hot else x * 1.5 + 0.3, torch.rand(C, generator=gen) + 0.5, rnd(gen, C) * 0.2


def gn_stat_view(ws, segs, G):
    """(mean, rstd) per (level, image, group): the tail of the GroupNorm workspace."""
    imgs = segs.nseg * segs.batch        # (ws holds exactly fd_groupnorm_workspace_bytes: chunk partials first, the statistics last)
    return ws[ws.numel() - imgs * G * 2:].view(imgs, G, 2)


def hot_tol(got, ref):
    """mean 100, std 0.01: y = x * a + b with |x * a| = |b| ~ 100 * rstd * gamma ~ 1.5e4 cancelling to O(1): the fp32 roundings of a, of the product
    of mean and of the product and difference that form b are each up to 2^-24 of that magnitude (8.9e-4) -- five roundings, together below 4.5e-3;
    the bound used is 5e-3 on outputs of size O(1).  A lost variance would be off by orders of magnitude, and the statistics themselves
    are checked to 1e-6 in test_groupnorm_keeps_a_small_variance_under_a_large_mean."""
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=5e-3)


def hot_grad(got, ref):
    """mean 100, std 0.01, backward: relative to the largest reference magnitude, 1e-3.  The kernel forms xhat = (x - (float)mean) * rstd: the fp32 rounding
    of a mean of 100 (3.8e-6) times rstd (95) is 3.6e-4 in xhat (|xhat| <= 4), which enters dgamma = sum dz * xhat as 3.6e-4 * |sum dz| against
    |dgamma| ~ sqrt(rows) -- a few 1e-4 -- and dx through the group mean of dz * gamma * xhat; dx = k1 * dz + p * x + q with |p * x| = |q| ~
    rstd^2 * 100 * |mean(dz gamma xhat)| ~ 1e5 cancelling to O(500): five fp32 roundings of 6e-3 each, 1e-4 of max |dx|.  Together below 5e-4; a lost
    variance (rstd wrong by orders of magnitude) is off by O(1)."""
    close(got, ref, 1e-3)


def gn_ref_levels(fn, x, B, hw):
    return R.join_levels([fn(t) for t in R.split_levels(R.f64(x), B, hw)])


def gn_case(kind, C, hw, G, act=ACT_SILU, hot=False):
    gen = torch.Generator().manual_seed(90 + C + G + len(hw))
    B, segs = 2, Segs.make(2, hw)
    x, gamma, beta = gn_data(gen, segs, C, hot)
    ins = {"x": x}
    gm, bt = d(gamma), d(beta)
    how = hot_tol if hot else "out"
    imgs = len(hw) * B

    def fwd_ref():
        return {"y": (gn_ref_levels(lambda t: R.gn_fwd(t, gamma, beta, G, EPS, act), x, B, hw), how)}

    if kind == "act":
        def run(v):
            ops.groupnorm_act(v["x"], gm, bt, v["y"], segs, G, act, ops.groupnorm_workspace(segs, G, DEV), EPS)
        return Case(C, ins, {"y": segs.rows}, run, fwd_ref, alias=("x", "y"), inplace=("x", "y"))
    if kind == "apply":
        def prep(v, launch):
            ws = ops.groupnorm_workspace(segs, G, DEV)
            if launch:
                ops.groupnorm_stats(v["x"], gm, bt, segs, G, ws, EPS)
            return ws

        def run(v, ws):
            ops.groupnorm_apply(v["x"], gm, bt, v["y"], segs, G, act, ws, EPS)
        return Case(C, ins, {"y": segs.rows}, run, fwd_ref, alias=("x", "y"), inplace=("x", "y"), prep=prep)
    if kind == "stats":
        def run(v):
            ws = ops.groupnorm_workspace(segs, G, DEV)
            coef = torch.full((imgs, 2, C), NAN, device=DEV)
            ops.groupnorm_stats(v["x"], gm, bt, segs, G, ws, EPS, coef)
            return {"gstat": gn_stat_view(ws, segs, G), "coef": coef}

        def ref():
            ab = [R.gn_coef(t, gamma, beta, G, EPS) for t in R.split_levels(R.f64(x), B, hw)]
            return {"coef": (torch.cat([torch.stack(p, 1) for p in ab], 0), how)}
        return Case(C, ins, {}, run, ref)
    if kind == "coef":
        ca, cb = torch.rand(imgs, C, generator=gen) + 0.5, rnd(gen, imgs, C) * 0.3
        coef = d(torch.stack([ca, cb], 1).contiguous())

        def run(v):
            ops.coef_apply(v["x"], coef[:, 0], coef[:, 1], v["y"], segs, act)

        def ref():
            lv = R.split_levels(R.f64(x), B, hw)
            return {"y": (R.join_levels([R.act_fwd(t * R.f64(ca[s * B:(s + 1) * B]).view(B, 1, 1, C) + R.f64(cb[s * B:(s + 1) * B]).view(B, 1, 1, C), act)
                                         for s, t in enumerate(lv)]), "out")}
        return Case(C, ins, {"y": segs.rows}, run, ref, alias=("x", "y"), inplace=("x", "y"))
    assert kind == "bwd"
    ins["dy"] = rnd(gen, segs.rows, C)

    def prep(v, launch):
        ws = ops.groupnorm_workspace(segs, G, DEV)
        if launch:
            ops.groupnorm_act(v["x"], gm, bt, ops.new_rows(segs.rows, C, DEV), segs, G, act, ws, EPS)
        return ws

    def run(v, ws):
        dgamma, dbeta = ops.groupnorm_act_bwd(v["x"], v["dy"], gm, bt, v["dx"], segs, G, act, ws, EPS)
        return {"dgamma": dgamma, "dbeta": dbeta}

    def ref():
        parts = [R.gn_bwd(t, g, gamma, beta, G, EPS, act) for t, g in zip(R.split_levels(R.f64(x), B, hw), R.split_levels(R.f64(ins["dy"]), B, hw))]
        g = hot_grad if hot else "grad"
        return {"dx": (R.join_levels([p[0] for p in parts]), g), "dgamma": (sum(p[1] for p in parts), hot_grad if hot else "pgrad"), "dbeta": (sum(p[2] for p in parts), "pgrad")}
    return Case(C, ins, {"dx": segs.rows}, run, ref, alias=("x", "dx"), prep=prep)


def se_case(kind, C, Cr, HW):
    gen = torch.Generator().manual_seed(100 + C + HW)
    N = 3
    ps = [rnd(gen, Cr, C) / C ** 0.5, rnd(gen, Cr) * 0.1, rnd(gen, C, Cr) / Cr ** 0.5, rnd(gen, C) * 0.1]
    pd = [d(p) for p in ps]
    ins = {"x": rnd(gen, N * HW, C)}
    if kind == "fwd":
        def run(v):
            ops.se_scale(v["x"], *pd, v["y"], N, HW, Cr, ops.se_workspace(N, HW, C, DEV))

        def ref():
            return {"y": (R.se_fwd(ins["x"].view(N, HW, C), *ps)[0].reshape(-1, C), "out")}
        return Case(C, ins, {"y": N * HW}, run, ref, alias=("x", "y"), inplace=("x", "y"))
    ins["dy"] = rnd(gen, N * HW, C)

    def prep(v, launch):
        ws = ops.se_workspace(N, HW, C, DEV)
        if launch:
            ops.se_scale(v["x"], *pd, ops.new_rows(N * HW, C, DEV), N, HW, Cr, ws)
        return ws

    def run(v, ws):
        return dict(zip(("dw1", "db1", "dw2", "db2"), ops.se_scale_bwd(v["x"], v["dy"], *pd, v["dx"], N, HW, Cr, ws)))

    def ref():
        dx, dw1, db1, dw2, db2 = R.se_bwd(ins["x"].view(N, HW, C), ins["dy"].view(N, HW, C), *ps)
        return {"dx": (dx.reshape(-1, C), "grad"), "dw1": (dw1, "pgrad"), "db1": (db1, "pgrad"), "dw2": (dw2, "pgrad"), "db2": (db2, "pgrad")}
    return Case(C, ins, {"dx": N * HW}, run, ref, alias=("x", "dx"), prep=prep)


def h_ordered(t):
    """f16 bit patterns as integers that count representable values in order."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def act_case(kind, C, act, p=0.0):
    gen = torch.Generator().manual_seed(110 + C + act)
    rows = 50
    dt = torch.float16 if kind == "bwd_h" else torch.float32
    ins = {"x": rnd(gen, rows, C, dtype=dt)}
    if kind == "fwd":
        def run(v):
            ops.act(v["x"], v["y"], act, p)

        def ref():
            return {"y": (R.act_fwd(ins["x"], act, p), "exact" if act in (ACT_RELU, ACT_NONE) else "out")}
        return Case(C, ins, {"y": rows}, run, ref, alias=("x", "y"), inplace=("x", "y"))
    ins["dy"] = rnd(gen, rows, C, dtype=dt)

    def run(v):
        ops.act_bwd(v["x"], v["dy"], v["dx"], act, p)

    def one_ulp(got, ref):
        want = ref.to(torch.float16)                 # the float64 product of the f16 inputs, rounded ONCE
        diff = (h_ordered(got.cpu()) - h_ordered(want)).abs()
        assert int(diff.max()) <= 1

    def ref():
        r = R.f64(ins["dy"]) * R.act_deriv(ins["x"], act, p)
        return {"dx": (r, one_ulp if kind == "bwd_h" else ("exact" if act in (ACT_RELU, ACT_NONE) else "grad"))}
    return Case(C, ins, {"dx": rows}, run, ref, alias=("x", "dx"), dtype=dt)


def nchw_case(C, HW):
    gen = torch.Generator().manual_seed(120 + C)
    N = 2
    ins = {"x": rnd(gen, N * HW, C)}

    def run(v):
        out = torch.full((N, C, HW), NAN, device=DEV)
        ops.nhwc_to_nchw(v["x"], N, HW, out)
        return {"out": out}

    def ref():
        return {"out": (R.f64(ins["x"]).view(N, HW, C).permute(0, 2, 1), "exact")}
    return Case(C, ins, {}, run, ref, reject=("cs",))        # (scalar loads: any co is legal)


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("k,s,pad", [(3, 2, 1), (2, 2, 0)])
@pytest.mark.parametrize("H,W", [(11, 14), (5, 7)])
def test_maxpool_views(k, s, pad, H, W):
    check_case(pool_case(k, s, pad, H, W, add=True))
    check_case(pool_case(k, s, pad, H, W, add=False))
    check_case(pool_bwd_case(k, s, pad, H, W))


def test_upsample2x_add_and_bwd_views():
    check_case(up_case())
    check_case(up_bwd_case())


@pytest.mark.parametrize("C", [4, 128])
def test_dwconv3x3_views(C):
    check_case(dw3_case(C))
    check_case(dw_wgrad_case(C, 3, 1, dilated=False))


@pytest.mark.parametrize("C,G,coef,in_act", [(128, 32, True, ACT_RELU), (128, 32, False, ACT_NONE), (128, 0, True, ACT_SILU), (4, 1, True, ACT_RELU), (4, 0, False, ACT_NONE)])
def test_dwconv3x3_gn_views(C, G, coef, in_act):
    """G = 0: no gn_stats.  The row-group sums are part of the bit-identity (they come out of shuffles over the lanes of a pixel)."""
    base = check_case(dw3_gn_case(C, G, coef, in_act))
    if G:       # the sums are those of the stored output (fp32 sums of C / G <= 4 ... 32 values: 1e-5 as in test_conv_epilogue_row_group_statistics)
        yv = base["y"].double().view(-1, G, C // G)
        np.testing.assert_allclose(base["gn_stats"][..., 0].cpu().numpy(), yv.sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(base["gn_stats"][..., 1].cpu().numpy(), (yv * yv).sum(-1).cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K,dil", [(3, 1), (5, 2), (7, 1), (3, 8)])
@pytest.mark.parametrize("C", [4, 128])
def test_dwconv_dilated_views(C, K, dil):
    check_case(dwd_case(C, K, dil))
    check_case(dw_wgrad_case(C, K, dil, dilated=True))


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [4, 128])
def test_dwconv2d_views(C, K, stride):
    check_case(dw2d_case(C, K, stride))


# C = 256 at 7 x 10 (4 row lanes: the four-deep body and the tail of the partial loop), C = 8 (more row lanes than rows per chunk), C = 1024 at 2 x 3
# (the upper bound); G in {1, C / 4, C}, the one-pixel level only where a group keeps >= 2 elements there
GN_SHAPES = [(256, PYR, 1), (256, PYR, 64), (256, PYR[:1], 256), (8, PYR, 1), (8, PYR, 2), (8, PYR[:2], 8), (1024, PYR[1:2], 1), (1024, PYR[1:2], 256),
             (1024, PYR[1:2], 1024)]


@pytest.mark.parametrize("C,hw,G", GN_SHAPES)
@pytest.mark.parametrize("kind", ["act", "apply", "stats", "coef"])
def test_groupnorm_forward_views(kind, C, hw, G):
    check_case(gn_case(kind, C, hw, G))


@pytest.mark.parametrize("C,hw,G", GN_SHAPES)
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU])
def test_groupnorm_act_bwd_views(C, hw, G, act):
    check_case(gn_case("bwd", C, hw, G, act))


@pytest.mark.parametrize("kind", ["act", "apply", "stats", "bwd"])
def test_groupnorm_keeps_a_small_variance_under_a_large_mean(kind):
    """Inputs of mean 100 and std 0.01 (variance 1e-4, E[x^2] = 1e4): the partial sums are fp64, so the statistics come out to fp32 rounding of
    rstd (a single-precision sum of squares would lose the variance altogether: 1e4 * 2^-24 = 6e-4 > 1e-4)."""
    C, hw, G = 256, PYR[:1], 64
    case = gn_case(kind, C, hw, G, ACT_NONE, hot=True)
    base = check_case(case)
    if kind == "stats":
        lv = R.split_levels(R.f64(case.ins["x"]), 2, hw)
        mean, rstd = R.gn_stats(lv[0], G, EPS)
        got = base["gstat"].cpu()
        np.testing.assert_allclose(got[..., 0].numpy(), mean.numpy(), rtol=1e-12)
        np.testing.assert_allclose(got[..., 1].numpy(), rstd.numpy(), rtol=1e-6)         # (rstd is stored rounded to fp32: 6e-8)


@pytest.mark.parametrize("C,Cr", [(16, 4), (144, 6), (128, 32)])
@pytest.mark.parametrize("HW", [1, 35])
@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_se_scale_views(kind, C, Cr, HW):
    check_case(se_case(kind, C, Cr, HW))


ACTS = [(ACT_RELU, 0.0), (ACT_SILU, 0.0), (ACT_EXP, 1.0), (ACT_EXP, 0.37), (ACT_SIGMOID, 0.0)]


@pytest.mark.parametrize("act,p", ACTS)
@pytest.mark.parametrize("C", [4, 24])
@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_act_views(kind, C, act, p):
    check_case(act_case(kind, C, act, p))


@pytest.mark.parametrize("act,p", ACTS)
@pytest.mark.parametrize("C", [4, 24])
def test_act_bwd_f16_views(C, act, p):
    """fd_act_bwd_nhwc_h against the float64 product of the f16 inputs rounded once to f16: at most 1 f16 ulp apart.  The kernel evaluates the
    derivative in fp32 (relative error ~1e-6, far below half an f16 ulp, 4.9e-4), so only products that close to a rounding boundary can land on
    the neighbouring value.  Share of elements that differ at all: 0 of the 7 000 elements of these ten cases with the kernel's arithmetic (fp32
    derivative, fp32 product, one rounding to f16) carried out by torch in fp32 on the CPU -- the expected order is the derivative's relative
    error over the ulp, 1e-6 / 9.8e-4 = 1e-3 of the elements."""
    check_case(act_case("bwd_h", C, act, p))


@pytest.mark.parametrize("C,HW", [(4, 1), (24, 35), (40, 70)])
def test_nhwc_to_nchw_views(C, HW):
    check_case(nchw_case(C, HW))


REJECT = {
    "maxpool": (lambda C=8: pool_case(3, 2, 1, 5, 7, True, C), 6),
    "maxpool_bwd": (lambda C=8: pool_bwd_case(3, 2, 1, 5, 7, C), 6),
    "upsample2x_add": (lambda C=8: up_case(C), 6),
    "upsample2x_bwd": (lambda C=8: up_bwd_case(C), 6),
    "dwconv3x3": (lambda C=8: dw3_case(C), 6),
    "dwconv3x3_gn": (lambda C=8: dw3_gn_case(C, 0, True), 6),
    "dwconv_dilated": (lambda C=8: dwd_case(C, 5, 2), 6),
    "dwconv2d": (lambda C=8: dw2d_case(C, 3, 2), 6),
    "dwconv3x3_wgrad": (lambda C=8: dw_wgrad_case(C, 3, 1, False), 6),
    "dwconv_dilated_wgrad": (lambda C=8: dw_wgrad_case(C, 5, 2, True), 6),
    "groupnorm_act": (lambda C=16: gn_case("act", C, PYR, 4), 48),            # C = 48: 12 does not divide 256
    "groupnorm_apply": (lambda C=16: gn_case("apply", C, PYR, 4), 48),
    "groupnorm_stats": (lambda C=16: gn_case("stats", C, PYR, 4), 48),
    "coef_apply": (lambda C=16: gn_case("coef", C, PYR, 4), 48),
    "groupnorm_act_bwd": (lambda C=16: gn_case("bwd", C, PYR, 4), 48),
    "se_scale": (lambda C=16: se_case("fwd", C, 4, 35), 6),
    "se_scale_bwd": (lambda C=16: se_case("bwd", C, 4, 35), 6),
    "act": (lambda C=8: act_case("fwd", C, ACT_SILU), 6),
    "act_bwd": (lambda C=8: act_case("bwd", C, ACT_SILU), 6),
    "act_bwd_f16": (lambda C=8: act_case("bwd_h", C, ACT_SILU), 6),
    "nhwc_to_nchw": (lambda C=8: nchw_case(C, 35), None),
}


@pytest.mark.parametrize("kernel", sorted(REJECT))
def test_illegal_views_are_rejected_before_any_launch(kernel):
    """Argument checks that return before a launch: nothing here runs a kernel on a bad view."""
    check_rejections(*REJECT[kernel])


def test_groupnorm_act_bwd_rejects_an_activation_without_backward():
    case = gn_case("bwd", 16, PYR, 4, ACT_EXP)
    names = list(case.ins) + list(case.outs)
    v, bufs = {}, {}
    for i, n in enumerate(names):
        v[n], bufs[n] = R.make_view(case.ins[n] if n in case.ins else torch.full((case.outs[n], 16), NAN), *GEOMS[i])
    segs = Segs.make(2, PYR)
    ws = ops.groupnorm_workspace(segs, 4, DEV)
    gm, bt = torch.ones(16, device=DEV), torch.zeros(16, device=DEV)
    ops.groupnorm_act(v["x"], gm, bt, ops.new_rows(segs.rows, 16, DEV), segs, 4, ACT_NONE, ws, EPS)
    before = bufs["dx"].clone()
    with pytest.raises(FdError):
        ops.groupnorm_act_bwd(v["x"], v["dy"], gm, bt, v["dx"], segs, 4, ACT_EXP, ws, EPS)
    torch.cuda.synchronize()
    assert R.unchanged(bufs["dx"], before)
