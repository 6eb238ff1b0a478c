"""fd_batchnorm_train_sync_fwd_nhwc / _bwd_nhwc (SyncBatchNorm at any width C % 4 == 0 up to 4096: two phases per direction, cut around an all-reduce the
caller issues) at kernel level, modelled on tests/test_syncbn_kernels_gpu.py: R ranks are simulated on ONE device, without torch.distributed -- every rank
is a shard of rows with its own sums buffer and workspaces, the all-reduce is a sum of the ranks' buffers on the device.  The calls go through the C ABI.

Reference: the float64 rank-set BatchNorm of tests/layer_ref.py (bn_sync_fwd / bn_sync_bwd / bn_running; held against autograd by
tests/test_syncbn_wide_cpu.py).  Tolerance: nothing fixed -- the bound of the any-width test, test_effnet_fulltrain_gpu._bound: 4 * e32 + 1e-6 * max |ref64|
with e32 = the error of torch's own fp32 CPU BatchNorm over the ranks' rows CONCATENATED against that float64 reference, measured here per quantity (for a
rank's local dgamma / dbeta: the e32 of the global dgamma / dbeta, with the rank's own max |ref64|).  The cases are those of that test's _bn_case over the
concatenated rows, so the ReLU cases are clear of the kink by RELU_MARGIN.

Widths: 4 (one quad), 40 (QT = 10, 6 idle threads), 144 (QT = 36, 4 idle threads), 260 (two tiles, the second one quad short: the q < C / 4 guard),
1392 (six tiles), 4096 (the limit).  Shards (300, 37, 1): 10 chunks (all four interleaved chunk lanes), 2 chunks, a one-row rank."""
import functools

import numpy as np
import pytest
import torch

import layer_ref as R
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd._lib import FdError
from test_effnet_fulltrain_gpu import ACTS, EPS, MOM, RELU_MARGIN, SENTINEL, _bn_case, _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SHARDS = (300, 37, 1)
WIDTHS = [4, 40, 144, 260, 1392, 4096]
# (pad, co) of the buffers of x, dy, y, dx: each on its own channel view inside a NaN-filled [rows, C + pad] buffer / contiguous / a padded-width map
VIEWS = dict(x=(12, 8), dy=(8, 4), y=(8, 4), dx=(16, 12))
FLAT = dict.fromkeys(("x", "dy", "y", "dx"), (0, 0))
PAD16 = dict.fromkeys(("x", "dy", "y", "dx"), (16, 0))          # C = 144 held at 160, the MBConv trunk's round32(C) maps
KEYS = ("y", "dx", "dgamma", "dbeta", "rm", "rv", "mean", "rstd", "coef")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_eq(a, b):
    return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def _place(t, pad, co):
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=torch.float32, device=DEV)
    buf[:, co:co + t.shape[1]] = t.to(DEV)
    return buf


@functools.lru_cache(maxsize=2)
def _case(C, nranks, act):
    """_bn_case over the concatenated rows + the float64 rank-set reference and torch's fp32 run of the same rows, per quantity: name -> (ref64, fp32)."""
    shards = SHARDS[:nranks]
    c = dict(_bn_case(C, sum(shards), act))
    xs, dys = list(c["x"].split(shards)), list(c["dy"].split(shards))
    ys, mean, var, n = R.bn_sync_fwd(xs, c["gamma"], c["beta"], EPS, ACTS[act])
    per_rank = R.bn_sync_bwd(xs, dys, c["gamma"], c["beta"], EPS, ACTS[act])
    rm, rv = R.bn_running(c["rm"], c["rv"], mean, var, n, MOM)
    assert n == sum(shards)
    f32 = dict(zip(("y", "dx", "dgamma", "dbeta", "rm", "rv"), c["f32"]), mean=c["mean32"], rstd=c["rstd32"])
    ref = dict(y=torch.cat(ys, 0), dx=torch.cat([p[0] for p in per_rank], 0), dgamma=sum(p[1] for p in per_rank), dbeta=sum(p[2] for p in per_rank),
               rm=rm, rv=rv, mean=mean, rstd=1.0 / torch.sqrt(var + EPS))
    c["refs"] = {k: (ref[k].numpy(), f32[k]) for k in ref}
    c["local"] = dict(dgamma=[p[1].numpy() for p in per_rank], dbeta=[p[2].numpy() for p in per_rank])
    c["shards"], c["xs"], c["dys"] = shards, xs, dys
    if act == "relu":
        z = (torch.cat(xs, 0).double() - mean) / torch.sqrt(var + EPS) * c["gamma"].double() + c["beta"].double()
        assert float(z.abs().min()) > RELU_MARGIN
    return c


def _run(c, act_id, host_total=False, geom=VIEWS, unsync=False, with_running=True, after_fwd_phase1=None):
    """The protocol over the ranks of the case (unsync: one rank through fd_batchnorm_train_fwd_nhwc / _bwd_nhwc instead), every output behind canaries.
    Returns per-rank lists of CPU tensors under KEYS."""
    lib = _lib.lib()
    shards, C, n = c["shards"], c["x"].shape[1], len(c["shards"])
    assert not unsync or n == 1
    total = float(sum(shards)) if host_total else -1.0
    gm, bt = c["gamma"].to(DEV), c["beta"].to(DEV)
    size = lib.fd_batchnorm_train_workspace_bytes if unsync else lib.fd_batchnorm_train_sync_workspace_bytes
    nbs = [size(rows, C) for rows in shards]
    assert all(nb > 0 and nb % 8 == 0 for nb in nbs)
    (px, ox), (pg, og), (py, oy), (pd, od) = (geom[k] for k in ("x", "dy", "y", "dx"))
    xb = [_place(x, px, ox) for x in c["xs"]]
    gb = [_place(d, pg, og) for d in c["dys"]]
    yb = [torch.full((rows, C + py), NAN, device=DEV) for rows in shards]
    dxb = [torch.full((rows, C + pd), NAN, device=DEV) for rows in shards]
    run, par = [], []
    for _ in shards:
        t = torch.full((2, C + 64), SENTINEL, device=DEV)                    # running_mean / running_var at [32, 32 + C)
        t[0, 32:32 + C], t[1, 32:32 + C] = c["rm"].to(DEV), c["rv"].to(DEV)
        run.append(t)
        par.append(torch.full((2, C + 64), SENTINEL, device=DEV))            # dgamma / dbeta at [32, 32 + C)
    ws = [torch.full((nb // 8 + 32,), SENTINEL, dtype=torch.float64, device=DEV) for nb in nbs]
    bws = [torch.full((nb // 8 + 32,), SENTINEL, dtype=torch.float64, device=DEV) for nb in nbs]
    sums = [torch.full((2 * C + 1 + 8,), NAN, dtype=torch.float64, device=DEV) for _ in shards]
    bsums = [torch.full((2 * C + 1 + 8,), NAN, dtype=torch.float64, device=DEV) for _ in shards]
    keep = [t.clone() for t in xb + gb + [gm, bt]]
    rp = lambda r, i: run[r][i, 32:].data_ptr() if with_running else None      # noqa: E731

    def fwd(r, phase):
        return lib.fd_batchnorm_train_sync_fwd_nhwc(xb[r].data_ptr(), C + px, ox, gm.data_ptr() if phase == 2 else None, bt.data_ptr() if phase == 2 else None,
                                                    yb[r].data_ptr() if phase == 2 else None, C + py if phase == 2 else 0, oy if phase == 2 else 0, shards[r], C, EPS,
                                                    act_id, phase, sums[r].data_ptr(), total if phase == 2 else -1.0, MOM, rp(r, 0), rp(r, 1), ws[r].data_ptr(),
                                                    nbs[r], _stream())

    def bwd(r, phase):
        return lib.fd_batchnorm_train_sync_bwd_nhwc(xb[r].data_ptr(), C + px, ox, gb[r].data_ptr(), C + pg, og, gm.data_ptr(), bt.data_ptr(),
                                                    dxb[r].data_ptr() if phase == 2 else None, C + pd if phase == 2 else 0, od if phase == 2 else 0,
                                                    par[r][0, 32:].data_ptr() if phase == 1 else None, par[r][1, 32:].data_ptr() if phase == 1 else None, shards[r], C,
                                                    EPS, act_id, phase, bsums[r].data_ptr(), total if phase == 2 else -1.0, ws[r].data_ptr(), bws[r].data_ptr(), nbs[r],
                                                    _stream())

    if unsync:
        rc = lib.fd_batchnorm_train_fwd_nhwc(xb[0].data_ptr(), C + px, ox, gm.data_ptr(), bt.data_ptr(), yb[0].data_ptr(), C + py, oy, shards[0], C, EPS, act_id, MOM,
                                             rp(0, 0), rp(0, 1), ws[0].data_ptr(), nbs[0], _stream())
        assert rc == 0, lib.fd_last_error()
        rc = lib.fd_batchnorm_train_bwd_nhwc(xb[0].data_ptr(), C + px, ox, gb[0].data_ptr(), C + pg, og, gm.data_ptr(), bt.data_ptr(), dxb[0].data_ptr(), C + pd, od,
                                             par[0][0, 32:].data_ptr(), par[0][1, 32:].data_ptr(), shards[0], C, EPS, act_id, ws[0].data_ptr(), bws[0].data_ptr(),
                                             nbs[0], _stream())
        assert rc == 0, lib.fd_last_error()
    else:
        for r in range(n):                                                   # forward phase 1, then this rank's row count behind the sums
            assert fwd(r, 1) == 0, lib.fd_last_error()
        if after_fwd_phase1 is not None:
            torch.cuda.synchronize()
            after_fwd_phase1(sums=sums, ws=ws, run=run, yb=yb)
        for r in range(n):
            sums[r][2 * C] = float(shards[r])
        if n > 1:                                                            # the all-reduce (one rank: the buffer passes from phase 1 to phase 2 untouched)
            red = torch.stack([s[:2 * C + 1] for s in sums]).sum(0)
            for r in range(n):
                sums[r][:2 * C + 1].copy_(red)
        for r in range(n):
            assert fwd(r, 2) == 0, lib.fd_last_error()
        for r in range(n):                                                   # backward phase 1; the global count is copied, not reduced again
            assert bwd(r, 1) == 0, lib.fd_last_error()
            bsums[r][2 * C:2 * C + 1].copy_(sums[r][2 * C:2 * C + 1])
        if n > 1:
            red = torch.stack([s[:2 * C] for s in bsums]).sum(0)             # the all-reduce of sums[:2C] only
            for r in range(n):
                bsums[r][:2 * C].copy_(red)
        for r in range(n):
            assert bwd(r, 2) == 0, lib.fd_last_error()
    torch.cuda.synchronize()
    for r in range(n):
        assert bool(torch.isnan(yb[r][:, :oy]).all()) and bool(torch.isnan(yb[r][:, oy + C:]).all()), "y: written outside the channel view"
        assert bool(torch.isnan(dxb[r][:, :od]).all()) and bool(torch.isnan(dxb[r][:, od + C:]).all()), "dx: written outside the channel view"
        for t in (run[r], par[r]):
            assert bool((t[:, :32] == SENTINEL).all()) and bool((t[:, 32 + C:] == SENTINEL).all()), "words around the per-channel outputs were written"
        if not with_running:
            assert torch.equal(run[r][0, 32:32 + C].cpu(), c["rm"]) and torch.equal(run[r][1, 32:32 + C].cpu(), c["rv"])
        assert bool((ws[r][nbs[r] // 8:] == SENTINEL).all()) and bool((bws[r][nbs[r] // 8:] == SENTINEL).all()), "words past the declared workspace size were written"
        if not unsync:
            assert bool(torch.isnan(sums[r][2 * C + 1:]).all()) and bool(torch.isnan(bsums[r][2 * C + 1:]).all()), "words past sums[2C] were written"
    assert all(_nan_eq(a, b) for a, b in zip(xb + gb + [gm, bt], keep)), "an input was modified"
    out = dict(y=[yb[r][:, oy:oy + C].cpu() for r in range(n)], dx=[dxb[r][:, od:od + C].cpu() for r in range(n)],
               dgamma=[par[r][0, 32:32 + C].cpu() for r in range(n)], dbeta=[par[r][1, 32:32 + C].cpu() for r in range(n)],
               rm=[run[r][0, 32:32 + C].cpu() for r in range(n)], rv=[run[r][1, 32:32 + C].cpu() for r in range(n)],
               mean=[ws[r][:C].cpu() for r in range(n)], rstd=[ws[r][C:2 * C].cpu() for r in range(n)], coef=[bws[r][:2 * C].cpu() for r in range(n)])
    if not unsync:
        out["count"] = float(sums[0][2 * C].cpu())
    return out


def _assert_same(a, b, what):
    for k in KEYS:
        assert len(a[k]) == len(b[k])
        for r, (s, t) in enumerate(zip(a[k], b[k])):
            assert torch.equal(s, t), f"{what}: {k} of rank {r} differs"


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_two_phase_protocol_over_simulated_ranks(nranks, C, act):
    c = _case(C, nranks, act)
    got = _run(c, ACTS[act], host_total=False)
    assert got["count"] == float(sum(c["shards"]))
    _assert_same(got, _run(c, ACTS[act], host_total=True), "total_rows as a host value against -1 (read on the device)")
    _assert_same(got, _run(c, ACTS[act], host_total=False), "two runs")
    cat = dict(y=torch.cat(got["y"], 0), dx=torch.cat(got["dx"], 0))
    for k, (ref, f32) in c["refs"].items():
        bound, e32 = _bound(ref, f32)
        if k in ("dgamma", "dbeta"):        # each rank's LOCAL sums, held to the e32 of the global ones and the rank's own magnitude
            for r, loc in enumerate(c["local"][k]):
                g = got[k][r].double().numpy()
                b = 4 * e32 + 1e-6 * float(np.abs(loc).max())
                err = float(np.abs(g - loc).max())
                print(f"sync batchnorm C={C} ranks={nranks} {act} {k}[rank {r}]: err {err:.3e}  e32 {e32:.3e}  bound {b:.3e}  max|ref| {np.abs(loc).max():.3e}")
                assert np.isfinite(g).all() and err <= b, (k, r, err, e32, b)
            continue
        for r in range(nranks if k not in ("y", "dx") else 1):                # y / dx: the ranks concatenated; per-channel results: every rank's copy
            g = (cat[k] if k in cat else got[k][r]).double().numpy()
            err = float(np.abs(g - ref).max())
            print(f"sync batchnorm C={C} ranks={nranks} {act} {k}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  max|ref| {np.abs(ref).max():.3e}")
            if act == "relu" and k == "y":
                assert bound < RELU_MARGIN
            assert np.isfinite(g).all() and err <= bound, (k, err, e32, bound)
    for k in ("rm", "rv", "mean", "rstd"):                                    # every rank finishes from the same global sums: the same bits
        assert all(torch.equal(got[k][0], t) for t in got[k][1:]), k


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("C", WIDTHS)
def test_one_rank_is_the_unsynchronised_launch_bit_for_bit(C, act):
    """y, the statistics block, the running statistics, dx, dgamma, dbeta and the coefficient block, with total_rows in either form; and without running
    statistics."""
    c = _case(C, 1, act)
    want = _run(c, ACTS[act], unsync=True)
    _assert_same(_run(c, ACTS[act], host_total=False), want, "device count")
    _assert_same(_run(c, ACTS[act], host_total=True), want, "host count")
    if C == 144:
        _assert_same(_run(c, ACTS[act], with_running=False), _run(c, ACTS[act], unsync=True, with_running=False), "without running statistics")


@pytest.mark.parametrize("geom", ["views", "pad160"])
def test_protocol_on_channel_views(geom):
    """x, y, dy, dx each on its own view inside NaN-filled buffers (and C = 144 held at 160): bit-identical to the contiguous run through the ops wrappers;
    _run asserts that nothing outside y / dx, the per-channel outputs, the declared workspace and sums[0 .. 2C] is written and that the inputs stay.  Forward
    phase 1 writes sums[0 .. 2C) and nothing else."""
    C, act = 144, "silu"
    c = _case(C, 3, act)

    def phase1_wrote_only_the_sums(sums, ws, run, yb):
        for r in range(3):
            assert bool(torch.isfinite(sums[r][:2 * C]).all()) and bool(torch.isnan(sums[r][2 * C:]).all()), "forward phase 1 wrote sums[2C] or past it"
            assert bool((ws[r][:2 * C] == SENTINEL).all()), "forward phase 1 wrote the statistics block"
            assert torch.equal(run[r][0, 32:32 + C].cpu(), c["rm"]) and torch.equal(run[r][1, 32:32 + C].cpu(), c["rv"]), "forward phase 1 moved the running statistics"
            assert bool((run[r][:, :32] == SENTINEL).all()) and bool((run[r][:, 32 + C:] == SENTINEL).all())
            assert bool(torch.isnan(yb[r]).all()), "forward phase 1 wrote y"

    got = _run(c, ACTS[act], geom=VIEWS if geom == "views" else PAD16, after_fwd_phase1=phase1_wrote_only_the_sums)
    _assert_same(got, _run(c, ACTS[act], geom=FLAT), "views against contiguous")
    # the same protocol through the ops wrappers on contiguous tensors
    n, gm, bt = 3, c["gamma"].to(DEV), c["beta"].to(DEV)
    xs, dys = [ops.Rows(x.to(DEV).contiguous()) for x in c["xs"]], [ops.Rows(d.to(DEV).contiguous()) for d in c["dys"]]
    ys, dxs = [ops.Rows(torch.empty_like(x.buf)) for x in xs], [ops.Rows(torch.empty_like(x.buf)) for x in xs]
    rms, rvs = [c["rm"].to(DEV).clone() for _ in range(n)], [c["rv"].to(DEV).clone() for _ in range(n)]
    sums = [torch.empty(2 * C + 1, dtype=torch.float64, device=DEV) for _ in range(n)]
    wss = [ops.batchnorm_train_sync_fwd(1, xs[r], sums[r], act_id=ACTS[act]) for r in range(n)]
    for r in range(n):
        sums[r][2 * C] = float(c["shards"][r])
    red = torch.stack(sums).sum(0)
    for r in range(n):
        sums[r].copy_(red)
        assert ops.batchnorm_train_sync_fwd(2, xs[r], sums[r], gm, bt, ys[r], EPS, ACTS[act], -1.0, MOM, rms[r], rvs[r], ws=wss[r]) is wss[r]
    bsums = [torch.empty(2 * C + 1, dtype=torch.float64, device=DEV) for _ in range(n)]
    dgs, dbs = [torch.empty(C, device=DEV) for _ in range(n)], [torch.empty(C, device=DEV) for _ in range(n)]
    bwss = [ops.batchnorm_train_sync_bwd(1, xs[r], dys[r], gm, bt, bsums[r], wss[r], None, dgs[r], dbs[r], EPS, ACTS[act]) for r in range(n)]
    for r in range(n):
        bsums[r][2 * C:].copy_(sums[r][2 * C:])
    red = torch.stack([s[:2 * C] for s in bsums]).sum(0)
    for r in range(n):
        bsums[r][:2 * C].copy_(red)
        ops.batchnorm_train_sync_bwd(2, xs[r], dys[r], gm, bt, bsums[r], wss[r], dxs[r], None, None, EPS, ACTS[act], -1.0, ws=bwss[r])
    torch.cuda.synchronize()
    wrapped = dict(y=[t.buf.cpu() for t in ys], dx=[t.buf.cpu() for t in dxs], dgamma=[t.cpu() for t in dgs], dbeta=[t.cpu() for t in dbs], rm=[t.cpu() for t in rms],
                   rv=[t.cpu() for t in rvs], mean=[w[:C].cpu() for w in wss], rstd=[w[C:2 * C].cpu() for w in wss], coef=[w[:2 * C].cpu() for w in bwss])
    _assert_same(got, wrapped, "C ABI against the ops wrappers")


def test_workspace_query_admits_a_one_row_rank():
    lib = _lib.lib()
    for C in WIDTHS:
        for rows in (2, 37, 300, 4099):
            assert lib.fd_batchnorm_train_sync_workspace_bytes(rows, C) == lib.fd_batchnorm_train_workspace_bytes(rows, C) > 0
        assert lib.fd_batchnorm_train_sync_workspace_bytes(1, C) == (2 * C + 2 * C) * 8 and lib.fd_batchnorm_train_workspace_bytes(1, C) == -1
    for rows, C in ((0, 24), (37, 6), (37, 0), (37, 4100), (1 << 31, 24)):
        assert lib.fd_batchnorm_train_sync_workspace_bytes(rows, C) == -1
    with pytest.raises(FdError):
        ops.batchnorm_train_sync_workspace(0, 24, DEV)


def test_rejections_leave_the_outputs_untouched():
    """Every rejection returns its code before any launch: y / dx, the per-channel outputs, sums and the workspaces keep their fill."""
    lib = _lib.lib()
    rows, C, W = 64, 24, 4104
    nb = lib.fd_batchnorm_train_sync_workspace_bytes(rows, C)
    x = torch.randn(rows, W, device=DEV)
    out = torch.full((rows, W), SENTINEL, device=DEV)
    vec = torch.full((4, W), SENTINEL, device=DEV)                            # running_mean, running_var, dgamma, dbeta
    gm = torch.ones(W, device=DEV)
    ws = torch.full((lib.fd_batchnorm_train_sync_workspace_bytes(rows, 4096) // 8,), SENTINEL, dtype=torch.float64, device=DEV)
    fws = torch.full_like(ws, 1.0)                                            # the backward's fwd_workspace: an input
    sums = torch.full((2 * 4096 + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    good = dict(xp=x.data_ptr(), cs=W, co=0, rows=rows, C=C, act=_lib.ACT_NONE, phase=2, total=-1.0, wsp=ws.data_ptr(), nbytes=nb, sp=sums.data_ptr(),
                rm=vec[0].data_ptr(), rv=vec[1].data_ptr(), outp=out.data_ptr())

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.fd_batchnorm_train_sync_fwd_nhwc(a["xp"], a["cs"], a["co"], gm.data_ptr(), gm.data_ptr(), a["outp"], W, 0, a["rows"], a["C"], EPS, a["act"], a["phase"],
                                                    a["sp"], a["total"], MOM, a["rm"], a["rv"], a["wsp"], a["nbytes"], _stream())

    def bwd(**kw):
        a = dict(good, **kw)
        return lib.fd_batchnorm_train_sync_bwd_nhwc(a["xp"], a["cs"], a["co"], x.data_ptr(), W, 0, gm.data_ptr(), gm.data_ptr(), a["outp"], W, 0, vec[2].data_ptr(),
                                                    vec[3].data_ptr(), a["rows"], a["C"], EPS, a["act"], a["phase"], a["sp"], a["total"], fws.data_ptr(), a["wsp"],
                                                    a["nbytes"], _stream())

    unsupported = [dict(C=6), dict(C=0), dict(C=4100), dict(rows=0), dict(act=_lib.ACT_SIGMOID), dict(act=_lib.ACT_EXP), dict(phase=0), dict(phase=3)]
    invalid = [dict(total=float(rows - 1)), dict(total=0.5), dict(xp=None), dict(xp=x.data_ptr() + 4), dict(cs=C - 4), dict(cs=W + 2), dict(co=2), dict(co=-4),
               dict(sp=None), dict(sp=sums.data_ptr() + 4), dict(wsp=None), dict(wsp=ws.data_ptr() + 4), dict(nbytes=nb - 8), dict(outp=None)]
    for fn in (fwd, bwd):
        for phase in (1, 2):
            for kw in unsupported:
                assert fn(**dict(dict(phase=phase), **kw)) == _lib.E_UNSUPPORTED, (fn.__name__, phase, kw)
            for kw in invalid:
                if phase == 1 and "outp" in kw:                               # (y / dx may be NULL in phase 1)
                    continue
                assert fn(**dict(kw, phase=phase)) == _lib.E_INVAL, (fn.__name__, phase, kw)
    assert fwd(rv=None) == _lib.E_INVAL and fwd(rm=None) == _lib.E_INVAL and fwd(rv=None, phase=1) == _lib.E_INVAL       # running_mean without running_var
    torch.cuda.synchronize()
    for t in (out, vec, ws, sums):
        assert bool((t == SENTINEL).all()), "a rejected call wrote an output"
    xr = ops.Rows(x, 0, C)
    with pytest.raises(FdError):
        ops.batchnorm_train_sync_fwd(1, xr, torch.empty(2 * C, dtype=torch.float64, device=DEV))                        # sums one element short
    with pytest.raises(FdError):
        ops.batchnorm_train_sync_fwd(3, xr, sums[:2 * C + 1])
    with pytest.raises(FdError):
        ops.batchnorm_train_sync_fwd(2, xr, sums[:2 * C + 1], gm[:C], gm[:C], ops.Rows(out, 0, C), EPS, _lib.ACT_NONE, float(rows - 1))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sums == SENTINEL).all())
    assert fwd(phase=1) == 0                                                  # and the good call runs
    torch.cuda.synchronize()
    assert not bool((sums[:2 * C] == SENTINEL).any()) and bool((sums[2 * C:] == SENTINEL).all()) and bool((out == SENTINEL).all())
