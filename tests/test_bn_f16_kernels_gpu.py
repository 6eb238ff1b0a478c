"""The f16-map forms of the any-width batch-statistics BatchNorm kernels (fd_batchnorm_train_*_nhwc_h) against their acceptance rule: for f16 inputs and
their exact fp32 upcasts, y_h / dx_h equal round_f16(the fp32 entry point's y / dx) BIT FOR BIT, and the statistics block, the coefficient block, the running
statistics, dgamma / dbeta and the phase-1 sums equal the fp32 entry point's bit for bit.  No tolerance.  Every map operand is a channel view at a non-zero
channel offset inside a wider buffer filled with NaN, which must come back untouched outside the view.

Second opinion: the f16 results within ONE f16 unit in the last place of |ref| (floor 2^-24) of the float64 restatement tests/bn_f16_ref.py.  That bound
presumes that the fp32 kernel's own error stays below half an f16 step: an fp32 result carries about three roundings of 2^-24 relative to its TERMS
(xhat * gamma, beta, the residual; rstd * gamma * dz, c1, xhat * c2), so where an output is a near-cancelling sum of terms of size t its error is ~3 * 2^-24 * t
whatever the output's size, against a floor of 2^-24.  The bound therefore holds on data whose terms stay below ~1/6, and the `small` data set (gamma, beta,
the residual and dy scaled by 2^-5) is built for it; on the `natural` data set (terms of order 1 .. 10) the bitwise rule is asserted and the deviation from
the restatement is printed (it exceeds one unit only at outputs that cancel to less than 2^-12 of their terms).  Measured on an MI355X: at most 0.56
unit on the small data set over every case, up to 3.2 units on the natural one."""
import pytest
import torch

import bn_f16_ref as R
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd.ops import Rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-3, 0.1
SHAPES = [(rows, C) for C in (4, 8, 260, 2048) for rows in (2, 37, 300)] + [(40000, 4)]      # 260: ntile 2, QT 33, idle threads; (40000, 4): 1024 chunks
NAN = float("nan")


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ in their bits"


class _Map:
    """A [rows, C] map as a channel view at `co` of a NaN-filled buffer, once as f16 and once as its exact fp32 upcast (same geometry)."""

    def __init__(self, rows, C, co, pad, data_h=None):
        self.co, self.C = co, C
        self.h = torch.full((rows, co + C + pad), NAN, dtype=torch.float16, device=DEV)
        if data_h is not None:
            self.h[:, co:co + C] = data_h.to(DEV)
        self.f = self.h.float()
        self.h0, self.f0 = self.h.clone(), self.f.clone()

    def rows(self, half, lo=0, hi=None):
        buf = self.h if half else self.f
        return Rows(buf[lo:hi], self.co, self.C)

    def view(self, half):
        return (self.h if half else self.f)[:, self.co:self.co + self.C]

    def untouched(self, what):                          # an input: the whole buffer; an output: everything outside the view
        _same(self.h, self.h0, what + " (f16 buffer)")
        _same(self.f, self.f0, what + " (fp32 buffer)")

    def outside_untouched(self, what):
        for buf in (self.h, self.f):
            out = torch.cat([buf[:, :self.co], buf[:, self.co + self.C:]], 1)
            assert bool(out.isnan().all()), what + ": written outside the view"


def _data(rows, C, small, seed):
    """f16 maps x, res, dy and fp32 gamma, beta, running statistics; small: every term of an output below ~1/6 (module docstring)."""
    gen = torch.Generator().manual_seed(seed)
    s = 2.0 ** -5 if small else 1.0
    x = (torch.randn(rows, C, generator=gen) * 2 + 0.5).half()
    res = (torch.randn(rows, C, generator=gen) * s).half()
    dy = (torch.randn(rows, C, generator=gen) * s).half()
    gamma = ((torch.rand(C, generator=gen) + 0.5) * s).to(DEV)
    beta = (torch.randn(C, generator=gen) * 0.3 * s).to(DEV)
    rmean, rvar = (torch.randn(C, generator=gen) * 0.1).to(DEV), (torch.rand(C, generator=gen) + 0.5).to(DEV)
    return x, res, dy, gamma, beta, rmean, rvar


def _ref_check(got_h, ref64, what, assert_it):
    """max |got - ref| in f16 units in the last place of |ref| (floor 2^-24); asserted <= 1 where the bound's premise holds."""
    got, ref = got_h.double().cpu(), ref64
    fin = torch.isfinite(ref) & (ref.abs() < 65504)
    assert bool(torch.isfinite(got[fin]).all()), what
    ulps = float(((got[fin] - ref[fin]).abs() / R.f16_ulp(ref[fin])).max()) if bool(fin.any()) else 0.0
    print(f"  {what}: max deviation from the float64 restatement {ulps:.3f} f16 ulp" + ("" if assert_it else " (natural data: printed, not asserted)"))
    if assert_it:
        assert ulps <= 1.0, (what, ulps)


def _forward_pair(kind, act, x, res, y, gamma, beta, rmean, rvar, rows, C):
    """The fp32 and the `_h` forward on the same data; returns the two workspaces and the two pairs of running tensors."""
    out = []
    for half in (False, True):
        rm, rv = rmean.clone(), rvar.clone()
        if kind == "res":
            ws = ops.batchnorm_train_res_fwd(x.rows(half), gamma, beta, res.rows(half), y.rows(half), EPS, act, MOM, rm, rv)
        else:
            ws = ops.batchnorm_train_fwd(x.rows(half), gamma, beta, y.rows(half), EPS, act, MOM, rm, rv)
        out.append((ws, rm, rv))
    return out


@pytest.mark.parametrize("small", [False, True], ids=["natural", "small"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_h_launch_is_the_fp32_launch_rounded_once(rows, C, small):
    xh, resh, dyh, gamma, beta, rmean, rvar = _data(rows, C, small, 100 * C + rows)
    x, res, dy = _Map(rows, C, 4, 8, xh), _Map(rows, C, 8, 4, resh), _Map(rows, C, 12, 0, dyh)
    print(f"rows {rows} C {C} ({'small' if small else 'natural'} data)")
    for kind, act in [("fwd", _lib.ACT_NONE), ("fwd", _lib.ACT_RELU), ("fwd", _lib.ACT_SILU), ("res", _lib.ACT_NONE), ("res", _lib.ACT_RELU)]:
        what = f"{kind} act {act}"
        y = _Map(rows, C, 4, 4)
        (ws32, rm32, rv32), (wsh, rmh, rvh) = _forward_pair(kind, act, x, res, y, gamma, beta, rmean, rvar, rows, C)
        _same(y.view(True), y.view(False).half(), what + ": y_h vs round_f16(fp32 y)")
        _same(wsh[:2 * C], ws32[:2 * C], what + ": statistics block")
        _same(rmh, rm32, what + ": running_mean")
        _same(rvh, rv32, what + ": running_var")
        assert not torch.equal(rmh, rmean) and bool(torch.isfinite(rmh).all() & torch.isfinite(rvh).all())
        y.outside_untouched(what + ": y")
        ref, _, _, rm_ref, rv_ref = R.forward(xh, gamma.cpu(), beta.cpu(), EPS, act, resh if kind == "res" else None, rmean.cpu(), rvar.cpu(), MOM)
        _ref_check(y.view(True), ref, what + " y", small)
        torch.testing.assert_close(rmh.double().cpu(), rm_ref, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(rvh.double().cpu(), rv_ref, rtol=1e-6, atol=1e-7)
        if kind == "res":
            continue                                    # (no backward of its own: the plain one with ACT_NONE on the masked gradient)
        dx = _Map(rows, C, 8, 8)
        got = []
        for half, fws in ((False, ws32), (True, wsh)):
            ws = ops.batchnorm_train_workspace(rows, C, DEV)
            dgamma, dbeta = ops.batchnorm_train_bwd(x.rows(half), dy.rows(half), gamma, beta, dx.rows(half), EPS, act, fws, ws)
            got.append((dgamma, dbeta, ws))
        _same(dx.view(True), dx.view(False).half(), what + ": dx_h vs round_f16(fp32 dx)")
        _same(got[1][0], got[0][0], what + ": dgamma")
        _same(got[1][1], got[0][1], what + ": dbeta")
        _same(got[1][2][:2 * C], got[0][2][:2 * C], what + ": coefficient block")
        dx.outside_untouched(what + ": dx")
        dx_ref, dgamma_ref, dbeta_ref = R.backward(xh, dyh, gamma.cpu(), beta.cpu(), EPS, act)
        _ref_check(dx.view(True), dx_ref, what + " dx", small)
        scale = float(dgamma_ref.abs().max()) + float(dbeta_ref.abs().max()) + 1e-30
        assert float((got[1][0].double().cpu() - dgamma_ref).abs().max()) <= 1e-5 * scale and float((got[1][1].double().cpu() - dbeta_ref).abs().max()) <= 1e-5 * scale
    for m, name in ((x, "x"), (res, "res"), (dy, "dy")):
        m.untouched(name)


def test_dx_beyond_the_f16_range_becomes_inf():
    """gamma of 4e4 on gradients of order 1: the fp32 dx passes 65504 and the f16 dx is +-inf exactly there (not saturated), bit for bit round_f16(fp32 dx)."""
    rows, C = 37, 8
    xh, _, dyh, _, beta, _, _ = _data(rows, C, False, 7)
    gamma = torch.full((C,), 4.0e4, device=DEV)
    x, dy, y, dx = _Map(rows, C, 4, 4, xh), _Map(rows, C, 4, 4, dyh), _Map(rows, C, 4, 4), _Map(rows, C, 4, 4)
    (ws32, _, _), (wsh, _, _) = _forward_pair("fwd", _lib.ACT_NONE, x, None, y, gamma, beta, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), rows, C)
    for half, fws in ((False, ws32), (True, wsh)):
        ops.batchnorm_train_bwd(x.rows(half), dy.rows(half), gamma, beta, dx.rows(half), EPS, _lib.ACT_NONE, fws)
    d32, dh = dx.view(False), dx.view(True)
    over = d32.abs() >= 65520.0                          # (65504 + half a step: what rounds to inf)
    assert int(over.sum()) > 0 and int((~over).sum()) > 0
    assert bool(torch.isinf(dh[over]).all()) and bool(torch.isfinite(dh[~over]).all()) and bool((torch.sign(dh[over]) == torch.sign(d32[over])).all())
    _same(dh, d32.half(), "dx_h vs round_f16(fp32 dx)")


@pytest.mark.parametrize("C", [8, 260])
def test_sync_forms_over_simulated_ranks(C):
    """Three ranks on one device with shards of 300, 37 and 1 rows; the sums are added on the device in rank order (what an all-reduce does).  Phase 1 of the
    `_h` form writes exactly what the fp32 phase 1 writes, phase 2 obeys the bit rule, forward (plain and residual form) and backward."""
    shards = (300, 37, 1)
    total = sum(shards)
    xh, resh, dyh, gamma, beta, rmean, rvar = _data(total, C, False, 31 + C)
    x, res, dy = _Map(total, C, 4, 8, xh), _Map(total, C, 8, 4, resh), _Map(total, C, 12, 0, dyh)
    bounds = [(sum(shards[:i]), sum(shards[:i + 1])) for i in range(len(shards))]
    for kind, act in (("fwd", _lib.ACT_SILU), ("fwd", _lib.ACT_RELU), ("res", _lib.ACT_RELU)):
        what = f"sync {kind} act {act} C {C}"
        y, dx = _Map(total, C, 4, 4), _Map(total, C, 8, 8)
        per = {}
        for half in (False, True):
            fwd = (lambda ph, xr, sums, rr, yr, rm, rv, ws: ops.batchnorm_train_sync_res_fwd(ph, xr, sums, gamma, beta, rr, yr, EPS, act, -1.0, MOM, rm, rv, ws)) \
                if kind == "res" else (lambda ph, xr, sums, rr, yr, rm, rv, ws: ops.batchnorm_train_sync_fwd(ph, xr, sums, gamma, beta, yr, EPS, act, -1.0, MOM, rm, rv, ws))
            sums, wss = [], []
            for lo, hi in bounds:                                   # phase 1 on every rank
                s = torch.full((2 * C + 1,), -7.0, dtype=torch.float64, device=DEV)
                wss.append(fwd(1, x.rows(half, lo, hi), s, None, None, None, None, None))
                assert float(s[2 * C]) == -7.0                      # the count slot is the caller's
                sums.append(s)
            tot = sums[0].clone()
            for s in sums[1:]:
                tot += s
            tot[2 * C] = float(total)
            runs = []
            for (lo, hi), ws in zip(bounds, wss):                   # phase 2 on every rank with the global sums
                rm, rv = rmean.clone(), rvar.clone()
                fwd(2, x.rows(half, lo, hi), tot.clone(), res.rows(half, lo, hi) if kind == "res" else None, y.rows(half, lo, hi), rm, rv, ws)
                runs.append((rm, rv))
            bact = _lib.ACT_NONE if kind == "res" else act          # (the residual form's backward: ACT_NONE on a gradient the caller masked)
            bsums, bwss, grads = [], [], []
            for (lo, hi), ws in zip(bounds, wss):
                s = torch.full((2 * C + 1,), -7.0, dtype=torch.float64, device=DEV)
                dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
                bwss.append(ops.batchnorm_train_sync_bwd(1, x.rows(half, lo, hi), dy.rows(half, lo, hi), gamma, beta, s, ws, None, dgamma, dbeta, EPS, bact))
                bsums.append(s)
                grads.append((dgamma, dbeta))
            btot = bsums[0].clone()
            for s in bsums[1:]:
                btot += s
            btot[2 * C] = float(total)
            for (lo, hi), ws, bws in zip(bounds, wss, bwss):
                ops.batchnorm_train_sync_bwd(2, x.rows(half, lo, hi), dy.rows(half, lo, hi), gamma, beta, btot.clone(), ws, dx.rows(half, lo, hi), None, None, EPS,
                                             bact, -1.0, ws=bws)
            per[half] = (sums, wss, runs, bsums, bwss, grads)
        f, h = per[False], per[True]
        for r in range(len(shards)):
            _same(h[0][r], f[0][r], f"{what}: rank {r} forward phase-1 sums")
            _same(h[1][r][:2 * C], f[1][r][:2 * C], f"{what}: rank {r} statistics block")
            _same(h[2][r][0], f[2][r][0], f"{what}: rank {r} running_mean")
            _same(h[2][r][1], f[2][r][1], f"{what}: rank {r} running_var")
            _same(h[2][r][0], h[2][0][0], f"{what}: running_mean rank {r} vs rank 0")
            _same(h[3][r], f[3][r], f"{what}: rank {r} backward phase-1 sums")
            _same(h[4][r][:2 * C], f[4][r][:2 * C], f"{what}: rank {r} coefficient block")
            _same(h[5][r][0], f[5][r][0], f"{what}: rank {r} dgamma")
            _same(h[5][r][1], f[5][r][1], f"{what}: rank {r} dbeta")
        _same(y.view(True), y.view(False).half(), what + ": y_h vs round_f16(fp32 y)")
        _same(dx.view(True), dx.view(False).half(), what + ": dx_h vs round_f16(fp32 dx)")
        y.outside_untouched(what + ": y")
        dx.outside_untouched(what + ": dx")
        ref = R.forward(xh, gamma.cpu(), beta.cpu(), EPS, act, resh if kind == "res" else None)[0]        # the statistics of all 338 rows
        _ref_check(y.view(True), ref, what + " y", False)
    for m, name in ((x, "x"), (res, "res"), (dy, "dy")):
        m.untouched(name)


@pytest.mark.parametrize("kind,act", [("fwd", _lib.ACT_SILU), ("res", _lib.ACT_RELU)])
def test_one_rank_of_the_sync_form_is_the_unsynchronised_h_launch(kind, act):
    rows, C = 37, 260
    xh, resh, dyh, gamma, beta, rmean, rvar = _data(rows, C, False, 5)
    x, res, dy = _Map(rows, C, 4, 8, xh), _Map(rows, C, 8, 4, resh), _Map(rows, C, 12, 0, dyh)
    y, dx, ys, dxs = _Map(rows, C, 4, 4), _Map(rows, C, 8, 8), _Map(rows, C, 4, 4), _Map(rows, C, 8, 8)
    (_, (ws, rm, rv)) = _forward_pair(kind, act, x, res, y, gamma, beta, rmean, rvar, rows, C)
    bact = _lib.ACT_NONE if kind == "res" else act
    bws = ops.batchnorm_train_workspace(rows, C, DEV)
    dgamma, dbeta = ops.batchnorm_train_bwd(x.rows(True), dy.rows(True), gamma, beta, dx.rows(True), EPS, bact, ws, bws)
    sums = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
    rms, rvs = rmean.clone(), rvar.clone()
    if kind == "res":
        w1 = ops.batchnorm_train_sync_res_fwd(1, x.rows(True), sums)
        ops.batchnorm_train_sync_res_fwd(2, x.rows(True), sums, gamma, beta, res.rows(True), ys.rows(True), EPS, act, float(rows), MOM, rms, rvs, w1)
    else:
        w1 = ops.batchnorm_train_sync_fwd(1, x.rows(True), sums)
        ops.batchnorm_train_sync_fwd(2, x.rows(True), sums, gamma, beta, ys.rows(True), EPS, act, float(rows), MOM, rms, rvs, w1)
    bs = torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV)
    dgs, dbs = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    b1 = ops.batchnorm_train_sync_bwd(1, x.rows(True), dy.rows(True), gamma, beta, bs, w1, None, dgs, dbs, EPS, bact)
    ops.batchnorm_train_sync_bwd(2, x.rows(True), dy.rows(True), gamma, beta, bs, w1, dxs.rows(True), None, None, EPS, bact, float(rows), ws=b1)
    for a, b, what in ((ys.view(True), y.view(True), "y"), (w1[:2 * C], ws[:2 * C], "statistics block"), (rms, rm, "running_mean"), (rvs, rv, "running_var"),
                       (dxs.view(True), dx.view(True), "dx"), (dgs, dgamma, "dgamma"), (dbs, dbeta, "dbeta"), (b1[:2 * C], bws[:2 * C], "coefficient block")):
        _same(a, b, f"one rank, {kind}: {what}")


def test_wrappers_refuse_mixed_map_types_and_the_cumulative_average():
    rows, C = 8, 8
    h = lambda: Rows(torch.zeros(rows, C, dtype=torch.float16, device=DEV))      # noqa: E731
    f = lambda: Rows(torch.zeros(rows, C, device=DEV))                           # noqa: E731
    g = torch.ones(C, device=DEV)
    with pytest.raises(_lib.FdError, match="y is an fp32 map but x is f16"):
        ops.batchnorm_train_fwd(h(), g, g, f(), EPS)
    with pytest.raises(_lib.FdError, match="res is an f16 map but x is fp32"):
        ops.batchnorm_train_res_fwd(f(), g, g, h(), f(), EPS, _lib.ACT_RELU)
    ws = ops.batchnorm_train_fwd(h(), g, g, h(), EPS)
    with pytest.raises(_lib.FdError, match="dy is an fp32 map but x is f16"):
        ops.batchnorm_train_bwd(h(), f(), g, g, h(), EPS, _lib.ACT_NONE, ws)
    with pytest.raises(_lib.FdError, match="dx is an fp32 map but x is f16"):
        ops.batchnorm_train_bwd(h(), h(), g, g, f(), EPS, _lib.ACT_NONE, ws)
    with pytest.raises(_lib.FdError, match="y is an f16 map but x is fp32"):
        ops.batchnorm_train_sync_fwd(2, f(), torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV), g, g, h(), EPS)
    nbt = torch.ones((), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.FdError, match="no f16-map form"):
        ops.batchnorm_train_fwd(h(), g, g, h(), EPS, _lib.ACT_NONE, nbt, g.clone(), g.clone())
