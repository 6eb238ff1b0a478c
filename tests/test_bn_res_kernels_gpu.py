"""fd_batchnorm_train_res_fwd_nhwc / fd_batchnorm_train_sync_res_fwd_nhwc -- y = act((x - mean) * rstd * gamma + beta + res), act in {NONE, RELU}: the
residual form of the any-width batch-statistics BatchNorm forward (the ResNet bottleneck's output) -- at kernel level through the C ABI, in the style of
tests/test_syncbn_wide_kernels_gpu.py: R ranks are simulated on ONE device, every rank a shard of rows with its own sums buffer and workspace, the
all-reduce a sum of the ranks' buffers on the device.

Reference: float64 act(bn(x) + r) built from tests/layer_ref.py (bn_sync_fwd without activation, act_fwd, bn_running).  Tolerance: nothing fixed -- the
bound of test_effnet_fulltrain_gpu._bound, 4 * e32 + 1e-6 * max |ref64| with e32 = the error of torch's own fp32 CPU op (F.batch_norm + r, ReLU) over the
ranks' rows CONCATENATED against that float64 reference, measured here per quantity.  ReLU cases: r is built so that every float64 z + r is farther than
RELU_MARGIN from 0 (r does not move the statistics: one nudge pass; asserted when the case is built).

Widths: 4 (one quad), 256 (one tile, QT = 64), 260 (two tiles, the second one quad short), 2048 (eight tiles: layer4).  Shards (300, 37, 1): 10 chunks,
2 chunks, a one-row rank.  Every operand sits on its own channel view inside a NaN-filled buffer."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd._lib import FdError
from test_effnet_fulltrain_gpu import ACTS, EPS, MOM, RELU_MARGIN, SENTINEL, _bn_case, _bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SHARDS = (300, 37, 1)
WIDTHS = [4, 256, 260, 2048]
RES_ACTS = ("none", "relu")
VIEWS = dict(x=(12, 8), res=(16, 4), y=(8, 4))          # (pad, co) of each operand's buffer
FLAT = dict.fromkeys(("x", "res", "y"), (0, 0))
KEYS = ("y", "rm", "rv", "mean", "rstd")


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
    """x, gamma, beta and the running statistics of _bn_case over the concatenated rows, a residual r, the float64 reference and torch's fp32 run of the same
    rows per quantity: name -> (ref64, fp32)."""
    shards = SHARDS[:nranks]
    rows = sum(shards)
    c = dict(_bn_case(C, rows, "none"))
    xs = list(c["x"].split(shards))
    zs, mean, var, n = R.bn_sync_fwd(xs, c["gamma"], c["beta"], EPS, _lib.ACT_NONE)
    assert n == rows
    z = torch.cat(zs, 0)
    r = torch.randn(rows, C, generator=torch.Generator().manual_seed(77 * C + rows))
    if act == "relu":       # r does not move the statistics: ONE nudge pass clears the kink
        pre = z + r.double()
        close = pre.abs() < 4 * RELU_MARGIN
        r = torch.where(close, r + torch.where(pre >= 0, 16 * RELU_MARGIN, -16 * RELU_MARGIN).float(), r)
        assert float((z + r.double()).abs().min()) > RELU_MARGIN, "could not build a ReLU case clear of the kink"
    y64 = R.act_fwd(z + r.double(), ACTS[act])
    rm, rv = R.bn_running(c["rm"], c["rv"], mean, var, n, MOM)
    rm32, rv32 = c["rm"].clone(), c["rv"].clone()
    y32 = F.batch_norm(c["x"], rm32, rv32, c["gamma"], c["beta"], True, MOM, EPS) + r
    y32 = F.relu(y32) if act == "relu" else y32
    c["refs"] = dict(y=(y64.numpy(), y32.double().numpy()), rm=(rm.numpy(), rm32.double().numpy()), rv=(rv.numpy(), rv32.double().numpy()),
                     mean=(mean.numpy(), c["mean32"]), rstd=((1.0 / torch.sqrt(var + EPS)).numpy(), c["rstd32"]))
    c["shards"], c["xs"], c["rs"] = shards, xs, list(r.split(shards))
    return c


def _run(c, act_id, geom=VIEWS, unsync=False, host_total=False, plain_phase1=False, stop_after_phase1=False, res_in_phase1=False):
    """The forward over the ranks of the case (unsync: one rank through fd_batchnorm_train_res_fwd_nhwc), every output behind canaries; plain_phase1: phase 1
    through fd_batchnorm_train_sync_fwd_nhwc instead.  Returns per-rank lists of CPU tensors under KEYS, plus the raw buffers."""
    lib = _lib.lib()
    shards, C, n = c["shards"], c["x"].shape[1], len(c["shards"])
    assert not unsync or n == 1
    total = float(sum(shards)) if host_total else -1.0
    gm, bt = c["gamma"].to(DEV), c["beta"].to(DEV)
    size = lib.fd_batchnorm_train_workspace_bytes if unsync else lib.fd_batchnorm_train_sync_workspace_bytes
    nbs = [size(rows, C) for rows in shards]
    assert all(nb > 0 and nb % 8 == 0 for nb in nbs)
    (px, ox), (pr, orr), (py, oy) = (geom[k] for k in ("x", "res", "y"))
    xb = [_place(x, px, ox) for x in c["xs"]]
    rb = [_place(r, pr, orr) for r in c["rs"]]
    yb = [torch.full((rows, C + py), NAN, device=DEV) for rows in shards]
    run = []
    for _ in shards:
        t = torch.full((2, C + 64), SENTINEL, device=DEV)                    # running_mean / running_var at [32, 32 + C)
        t[0, 32:32 + C], t[1, 32:32 + C] = c["rm"].to(DEV), c["rv"].to(DEV)
        run.append(t)
    ws = [torch.full((nb // 8 + 32,), SENTINEL, dtype=torch.float64, device=DEV) for nb in nbs]
    sums = [torch.full((2 * C + 1 + 8,), NAN, dtype=torch.float64, device=DEV) for _ in shards]
    keep = [t.clone() for t in xb + rb + [gm, bt]]

    def fwd(r, phase):
        two = phase == 2
        if plain_phase1 and not two:
            return lib.fd_batchnorm_train_sync_fwd_nhwc(xb[r].data_ptr(), C + px, ox, None, None, None, 0, 0, shards[r], C, EPS, act_id, 1, sums[r].data_ptr(), -1.0,
                                                        MOM, run[r][0, 32:].data_ptr(), run[r][1, 32:].data_ptr(), ws[r].data_ptr(), nbs[r], _stream())
        with_res = two or res_in_phase1
        return lib.fd_batchnorm_train_sync_res_fwd_nhwc(xb[r].data_ptr(), C + px, ox, gm.data_ptr() if two else None, bt.data_ptr() if two else None,
                                                        rb[r].data_ptr() if with_res else None, C + pr if with_res else 0, orr if with_res else 0,
                                                        yb[r].data_ptr() if two else None, C + py if two else 0, oy if two else 0, shards[r], C, EPS, act_id,
                                                        phase, sums[r].data_ptr(), total if two else -1.0, MOM, run[r][0, 32:].data_ptr(),
                                                        run[r][1, 32:].data_ptr(), ws[r].data_ptr(), nbs[r], _stream())

    if unsync:
        rc = lib.fd_batchnorm_train_res_fwd_nhwc(xb[0].data_ptr(), C + px, ox, gm.data_ptr(), bt.data_ptr(), rb[0].data_ptr(), C + pr, orr, yb[0].data_ptr(), C + py,
                                                 oy, shards[0], C, EPS, act_id, MOM, run[0][0, 32:].data_ptr(), run[0][1, 32:].data_ptr(), ws[0].data_ptr(), nbs[0],
                                                 _stream())
        assert rc == 0, lib.fd_last_error()
    else:
        for r in range(n):
            assert fwd(r, 1) == 0, lib.fd_last_error()
        if not stop_after_phase1:
            for r in range(n):
                sums[r][2 * C] = float(shards[r])
            if n > 1:                                                        # the all-reduce (one rank: the buffer passes from phase 1 to phase 2 untouched)
                red = torch.stack([s[:2 * C + 1] for s in sums]).sum(0)
                for r in range(n):
                    sums[r][:2 * C + 1].copy_(red)
            for r in range(n):
                assert fwd(r, 2) == 0, lib.fd_last_error()
    torch.cuda.synchronize()
    for r in range(n):
        assert bool(torch.isnan(yb[r][:, :oy]).all()) and bool(torch.isnan(yb[r][:, oy + C:]).all()), "y: written outside the channel view"
        assert bool((run[r][:, :32] == SENTINEL).all()) and bool((run[r][:, 32 + C:] == SENTINEL).all()), "words around the running statistics were written"
        assert bool((ws[r][nbs[r] // 8:] == SENTINEL).all()), "words past the declared workspace size were written"
        if not unsync:
            assert bool(torch.isnan(sums[r][2 * C + 1:]).all()), "words past sums[2C] were written"
    assert all(_nan_eq(a, b) for a, b in zip(xb + rb + [gm, bt], keep)), "an input was modified"
    return dict(y=[yb[r][:, oy:oy + C].cpu() for r in range(n)], rm=[run[r][0, 32:32 + C].cpu() for r in range(n)], rv=[run[r][1, 32:32 + C].cpu() for r in range(n)],
                mean=[ws[r][:C].cpu() for r in range(n)], rstd=[ws[r][C:2 * C].cpu() for r in range(n)],
                raw=dict(yb=[t.cpu() for t in yb], ws=[t.cpu() for t in ws], sums=[t.cpu() for t in sums], run=[t.cpu() for t in run]))


def _assert_same(a, b, what):
    for k in KEYS:
        assert len(a[k]) == len(b[k])
        for r, (s, t) in enumerate(zip(a[k], b[k])):
            assert torch.equal(s, t), f"{what}: {k} of rank {r} differs"


@pytest.mark.parametrize("act", RES_ACTS)
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_residual_forward_over_simulated_ranks(nranks, C, act):
    c = _case(C, nranks, act)
    got = _run(c, ACTS[act])
    _assert_same(got, _run(c, ACTS[act], host_total=True), "total_rows as a host value against -1 (read on the device)")
    _assert_same(got, _run(c, ACTS[act], geom=FLAT), "views against contiguous")
    cat = dict(y=torch.cat(got["y"], 0))
    for k, (ref, f32) in c["refs"].items():
        bound, e32 = _bound(ref, f32)
        for r in range(nranks if k != "y" else 1):                           # y: the ranks concatenated; per-channel results: every rank's copy
            g = (cat[k] if k in cat else got[k][r]).double().numpy()
            err = float(np.abs(g - ref).max())
            print(f"residual batchnorm C={C} ranks={nranks} {act} {k}: err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  max|ref| {np.abs(ref).max():.3e}")
            if act == "relu" and k == "y":
                assert bound < RELU_MARGIN
            assert np.isfinite(g).all() and err <= bound, (k, err, e32, bound)
    for k in ("rm", "rv", "mean", "rstd"):                                   # every rank finishes from the same global sums: the same bits
        assert all(torch.equal(got[k][0], t) for t in got[k][1:]), k


@pytest.mark.parametrize("act", RES_ACTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_one_rank_is_the_unsynchronised_launch_bit_for_bit(C, act):
    """y, the statistics block and the running statistics, with total_rows in either form."""
    c = _case(C, 1, act)
    want = _run(c, ACTS[act], unsync=True)
    _assert_same(_run(c, ACTS[act]), want, "device count")
    _assert_same(_run(c, ACTS[act], host_total=True), want, "host count")


@pytest.mark.parametrize("C", [256, 260])
def test_phase_1_is_the_plain_phase_1_and_writes_nothing_else(C):
    """Phase 1 of the residual form, with and without a residual pointer, leaves every buffer -- sums, the whole workspace, y, the running statistics -- bit
    for bit as fd_batchnorm_train_sync_fwd_nhwc's phase 1 leaves it: sums[0 .. 2C) written, the statistics block, sums[2C], y and the running statistics not."""
    c = _case(C, 3, "relu")
    plain = _run(c, ACTS["relu"], plain_phase1=True, stop_after_phase1=True)["raw"]
    for with_res in (False, True):
        got = _run(c, ACTS["relu"], stop_after_phase1=True, res_in_phase1=with_res)["raw"]
        for k in ("yb", "ws", "sums", "run"):
            assert all(_nan_eq(a, b) for a, b in zip(got[k], plain[k])), (k, with_res)
        for r in range(3):
            assert bool(torch.isfinite(got["sums"][r][:2 * C]).all()) and bool(torch.isnan(got["sums"][r][2 * C:]).all()), "phase 1 wrote sums[2C] or past it"
            assert bool((got["ws"][r][:2 * C] == SENTINEL).all()), "phase 1 wrote the statistics block"
            assert torch.equal(got["run"][r][0, 32:32 + C], c["rm"]) and torch.equal(got["run"][r][1, 32:32 + C], c["rv"]), "phase 1 moved the running statistics"
            assert bool(torch.isnan(got["yb"][r]).all()), "phase 1 wrote y"


@pytest.mark.parametrize("C", [260, 2048])
def test_zero_residual_is_the_plain_forward_and_the_ops_wrappers_agree(C):
    """act NONE with res = 0 gives the plain forward's y (z + 0 is z), its statistics block and running statistics; the ops wrappers give the C ABI's bits."""
    c = _case(C, 1, "none")
    rows = c["shards"][0]
    x, gm, bt = c["x"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV)
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    rm = [c["rm"].to(DEV).clone() for _ in range(2)]
    rv = [c["rv"].to(DEV).clone() for _ in range(2)]
    w0 = ops.batchnorm_train_fwd(ops.Rows(x), gm, bt, ops.Rows(y0), EPS, _lib.ACT_NONE, MOM, rm[0], rv[0])
    w1 = ops.batchnorm_train_res_fwd(ops.Rows(x), gm, bt, ops.Rows(torch.zeros_like(x)), ops.Rows(y1), EPS, _lib.ACT_NONE, MOM, rm[1], rv[1])
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(w0, w1) and torch.equal(rm[0], rm[1]) and torch.equal(rv[0], rv[1])
    for act in RES_ACTS:
        cc = _case(C, 1, act)
        want = _run(cc, ACTS[act], unsync=True)
        r = cc["rs"][0].to(DEV)
        y, rm2, rv2 = torch.empty_like(x), c["rm"].to(DEV).clone(), c["rv"].to(DEV).clone()
        ws = ops.batchnorm_train_res_fwd(ops.Rows(x), gm, bt, ops.Rows(r), ops.Rows(y), EPS, ACTS[act], MOM, rm2, rv2)
        ys, rm3, rv3 = torch.empty_like(x), c["rm"].to(DEV).clone(), c["rv"].to(DEV).clone()
        sums = torch.empty(2 * C + 1, dtype=torch.float64, device=DEV)
        wss = ops.batchnorm_train_sync_res_fwd(1, ops.Rows(x), sums, act_id=ACTS[act])
        sums[2 * C] = float(rows)
        assert ops.batchnorm_train_sync_res_fwd(2, ops.Rows(x), sums, gm, bt, ops.Rows(r), ops.Rows(ys), EPS, ACTS[act], -1.0, MOM, rm3, rv3, ws=wss) is wss
        torch.cuda.synchronize()
        for got_y, got_rm, got_rv, got_ws in ((y, rm2, rv2, ws), (ys, rm3, rv3, wss)):
            assert torch.equal(got_y.cpu(), want["y"][0]) and torch.equal(got_rm.cpu(), want["rm"][0]) and torch.equal(got_rv.cpu(), want["rv"][0])
            assert torch.equal(got_ws[:C].cpu(), want["mean"][0]) and torch.equal(got_ws[C:2 * C].cpu(), want["rstd"][0])


def test_rejections_leave_the_outputs_untouched():
    """SiLU, a bad residual view, a short workspace and a NULL residual in phase 2 return their codes before any launch: y, the running statistics, sums and
    the workspace keep their fill."""
    lib = _lib.lib()
    rows, C, W = 64, 24, 4104
    nb = lib.fd_batchnorm_train_sync_workspace_bytes(rows, C)
    assert nb == lib.fd_batchnorm_train_workspace_bytes(rows, C)
    x = torch.randn(rows, W, device=DEV)
    res = torch.randn(rows, W, device=DEV)
    out = torch.full((rows, W), SENTINEL, device=DEV)
    vec = torch.full((2, W), SENTINEL, device=DEV)                            # running_mean, running_var
    gm = torch.ones(W, device=DEV)
    ws = torch.full((nb // 8 + 8,), SENTINEL, dtype=torch.float64, device=DEV)
    sums = torch.full((2 * C + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    good = dict(rp=res.data_ptr(), rcs=W, rco=0, C=C, act=_lib.ACT_RELU, phase=2, nbytes=nb, wsp=ws.data_ptr(), outp=out.data_ptr())

    def sync(**kw):
        a = dict(good, **kw)
        return lib.fd_batchnorm_train_sync_res_fwd_nhwc(x.data_ptr(), W, 0, gm.data_ptr(), gm.data_ptr(), a["rp"], a["rcs"], a["rco"], a["outp"], W, 0, rows, a["C"],
                                                        EPS, a["act"], a["phase"], sums.data_ptr(), -1.0, MOM, vec[0].data_ptr(), vec[1].data_ptr(), a["wsp"],
                                                        a["nbytes"], _stream())

    def plain(**kw):
        a = dict(good, **kw)
        return lib.fd_batchnorm_train_res_fwd_nhwc(x.data_ptr(), W, 0, gm.data_ptr(), gm.data_ptr(), a["rp"], a["rcs"], a["rco"], a["outp"], W, 0, rows, a["C"], EPS,
                                                   a["act"], MOM, vec[0].data_ptr(), vec[1].data_ptr(), a["wsp"], a["nbytes"], _stream())

    unsupported = [dict(act=_lib.ACT_SILU), dict(act=_lib.ACT_SIGMOID), dict(C=6), dict(C=4100)]
    invalid = [dict(rp=None), dict(rp=res.data_ptr() + 4), dict(rcs=C - 4), dict(rcs=W + 2), dict(rco=2), dict(rco=-4), dict(nbytes=nb - 8), dict(wsp=None),
               dict(wsp=ws.data_ptr() + 4), dict(outp=None)]
    for fn in (sync, plain):
        for kw in unsupported:
            assert fn(**kw) == _lib.E_UNSUPPORTED, (fn.__name__, kw)
        for kw in invalid:
            assert fn(**kw) == _lib.E_INVAL, (fn.__name__, kw)
    assert sync(act=_lib.ACT_SILU, phase=1) == _lib.E_UNSUPPORTED and sync(nbytes=nb - 8, phase=1) == _lib.E_INVAL and sync(phase=3) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (out, vec, ws, sums):
        assert bool((t == SENTINEL).all()), "a rejected call wrote an output"
    xr, rr, yr = ops.Rows(x, 0, C), ops.Rows(res, 0, C), ops.Rows(out, 0, C)
    with pytest.raises(FdError) as e:
        ops.batchnorm_train_res_fwd(xr, gm[:C], gm[:C], rr, yr, EPS, _lib.ACT_SILU)
    assert e.value.rc == _lib.E_UNSUPPORTED
    with pytest.raises(FdError):
        ops.batchnorm_train_res_fwd(xr, gm[:C], gm[:C], ops.Rows(res, 0, C + 4), yr, EPS, _lib.ACT_RELU)                 # a residual of another width
    with pytest.raises(FdError):
        ops.batchnorm_train_sync_res_fwd(2, xr, sums, gm[:C], gm[:C], None, yr, EPS, _lib.ACT_RELU)                      # phase 2 without a residual
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sums == SENTINEL).all())
    assert sync(phase=1, rp=None) == 0 and plain() == 0                       # and the good calls run
    torch.cuda.synchronize()
    assert not bool((sums[:2 * C] == SENTINEL).any()) and bool((sums[2 * C:] == SENTINEL).all())
    assert not bool((out[:, :C] == SENTINEL).any()) and bool((out[:, C:] == SENTINEL).all())
