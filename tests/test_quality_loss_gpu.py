"""fd_ltrb_quality / fd_quality_loss_fwd / fd_quality_loss_bwd on the device against the numpy restatement
(tests/quality_loss_ref.py) on the cases of tests/quality_loss_cases.py (test_quality_loss_cpu.py proves what each case holds).

quality         bit for bit the fp32 restatement (IEEE operations only, contraction off on both sides)
qsum            the float64 sum of the device's own q, rounded to fp32: exact
loss, gradient  against the float64 restatement, by Q.rel_err (largest elementwise relative error, magnitudes floored at fp32
                epsilon times the tensor's largest), within FACTOR = 8 times what the fp32 numpy restatement deviates from float64
                over all cases: the device's expf / log1pf differ from numpy's by a few ulp (the margin tests/test_simota_gpu.py
                gives pair_cost for the same reason).  Both figures are printed.
then saturated rows, guard floats round every output with a NaN workspace at three alignments, two eager runs and a graph replay
bit for bit, FCOSLoss end to end on the 341-location pyramid, and one training step on SimOTA targets with cls_mode="qfl"."""
import numpy as np
import pytest
import torch

import quality_loss_cases as K
import quality_loss_ref as Q
import simota_cases as SK
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd.model.loss import FCOSLoss, compute_cls_loss_quality, flatten_levels
from pytorch_object_detection_amd.model.modules.head import SimOTAGenTargets
from pytorch_object_detection_amd.model.od.HISFcos import HalfInvertedStageFPN, HISFCOSHead

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
FACTOR = 8
EPS32 = float(np.finfo(np.float32).eps)
_REF, _DEV = {}, {}


def tensors(c):
    return {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in c.items()}


def ref(name):
    """Per case, computed once and read-only: q (fp32 restatement) and per kind (loss, qsum, grad) in float64 and in fp32."""
    if name not in _REF:
        c = K.get(name)
        q = Q.quality(c["reg_pred"], c["reg_target"], c["labels"])
        r = {"q": q}
        for kind in Q.KINDS:
            r[kind] = {d: Q.loss_and_grad(kind, c["logits"], c["labels"], q, c["gscale"], dtype=d) for d in (np.float64, np.float32)}
            for t in r[kind].values():
                for v in t:
                    v.setflags(write=False)
        q.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def device(name):
    """One device run per case: q and per kind (loss, qsum, grad), as numpy."""
    if name not in _DEV:
        t = tensors(K.get(name))
        q = ops.ltrb_quality(t["reg_pred"], t["reg_target"], t["labels"])
        r = {"q": q.cpu().numpy()}
        for kind in Q.KINDS:
            loss, qsum = ops.quality_loss_fwd(t["logits"], t["labels"], q, kind)
            grad = ops.quality_loss_bwd(t["logits"], t["labels"], q, t["gscale"], kind)
            r[kind] = tuple(v.cpu().numpy() for v in (loss, qsum, grad))
        _DEV[name] = r
    return _DEV[name]


def yardstick(kind, what, measure=Q.rel_err):
    """What the fp32 numpy restatement deviates from the float64 one, the largest over all cases; what: 0 the loss, 2 the gradient."""
    key = ("y", kind, what, measure.__name__)
    if key not in _REF:
        _REF[key] = max(measure(ref(n)[kind][np.float32][what], ref(n)[kind][np.float64][what]) for n in K.ALL)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- the three kernels
@pytest.mark.parametrize("name", K.ALL)
def test_quality_bit_for_bit(name):
    c = K.get(name)
    q = device(name)["q"]
    assert q.dtype == np.float32 and q.shape == c["labels"].shape
    np.testing.assert_array_equal(q.view(np.int32), ref(name)["q"].view(np.int32))
    # labels as the assigners emit them, [B, L, 1], give the same
    t = tensors(c)
    assert torch.equal(ops.ltrb_quality(t["reg_pred"], t["reg_target"], t["labels"][..., None]).cpu(), torch.from_numpy(np.array(q)))


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", K.ALL)
def test_loss_qsum_and_gradient_against_float64(name, kind):
    c = K.get(name)
    loss, qsum, grad = device(name)[kind]
    l64, q64, g64 = ref(name)[kind][np.float64]
    l32, _, g32 = ref(name)[kind][np.float32]
    assert loss.dtype == qsum.dtype == grad.dtype == np.float32 and grad.shape == c["logits"].shape and loss.shape == qsum.shape == c["gscale"].shape
    np.testing.assert_array_equal(qsum, device(name)["q"].astype(np.float64).sum(1).astype(F))
    np.testing.assert_array_equal(qsum, q64.astype(F))
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    yl, yg = yardstick(kind, 0), yardstick(kind, 2)
    dl, dg = Q.rel_err(loss, l64), Q.rel_err(grad, g64)
    print(f"{name} {kind}: loss: fp32 numpy deviates from float64 by at most {yl:.3e} over all cases (this case {Q.rel_err(l32, l64):.3e}), the device by "
          f"{dl:.3e} (ratio {dl / yl:.2f}); gradient: {yg:.3e} (this case {Q.rel_err(g32, g64):.3e}), the device {dg:.3e} (ratio {dg / yg:.2f})")
    assert dl <= FACTOR * yl
    assert dg <= FACTOR * yg
    # The elementwise measure is dominated by the few elements where y - s cancels (an absolute error of one fp32 epsilon in an
    # element a hundred times the floor is 1e-2 relatively), so it says little about the others.  Beside it: the largest absolute
    # error over the tensor's largest magnitude, device against 8 times numpy's over all cases -- a yardstick of a few epsilon.
    al, ag = yardstick(kind, 0, Q.max_err), yardstick(kind, 2, Q.max_err)
    print(f"   largest error / largest magnitude: loss numpy {al:.3e} device {Q.max_err(loss, l64):.3e}; gradient numpy {ag:.3e} device {Q.max_err(grad, g64):.3e}")
    assert 0 < yl and 0 < yg and 0 < al < 16 * EPS32 and 0 < ag < 16 * EPS32           # yardsticks of fp32 rounding, not of something broken
    assert Q.max_err(loss, l64) <= FACTOR * al and Q.max_err(grad, g64) <= FACTOR * ag


@pytest.mark.parametrize("kind", Q.KINDS)
def test_saturated_rows(kind):
    """Images of one pinned logit each (0, +-90, +-200; without and with positives): finite wherever float64 is, and exactly zero where
    the float64 value rounds to zero in fp32 (negatives at -90 and -200: s^2 * bce underflows)."""
    loss, _, grad = device("saturated")[kind]
    l64, _, g64 = ref("saturated")[kind][np.float64]
    assert np.isfinite(l64).all() and np.isfinite(g64).all() and np.isfinite(loss).all() and np.isfinite(grad).all()
    zl, zg = l64.astype(F) == 0, g64.astype(F) == 0
    assert zl.sum() == 2 and zg.sum() >= 2 * 12
    assert not loss[zl].any() and not grad[zg].any()
    assert (loss[~zl] > 0).all()
    # and the pinned rows inside a random case, elementwise
    c = K.get("b3_l341_c80")
    g = device("b3_l341_c80")[kind][2]
    g64 = ref("b3_l341_c80")[kind][np.float64][2]
    rows = slice(K.PIN_POS0, K.PIN_NEG0 + len(K.PINS))
    assert np.isfinite(g[0, rows]).all() and not g[0, rows][g64[0, rows].astype(F) == 0].any()
    assert (np.abs(c["logits"][0, rows]) >= 90).sum() >= 8 * 80


# ---------------------------------------------------------------------------------------------------- memory and capture
@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name,shift", [("b3_l341_c80", 0), ("b3_l341_c80", 1), ("b3_l341_c80", 2), ("b1_l502_c81", 0), ("b3_l502_c6", 2)])
def test_nothing_outside_the_outputs_changes_and_the_workspace_may_hold_anything(name, shift, kind):
    """The C ABI on buffers cut out of larger ones, `shift` floats off a 16-byte boundary (C = 80 is read in 16-, 4- and 8-byte pieces at
    shifts 0, 1, 2): the guard floats round q, loss, qsum, grad and the workspace keep their pattern; the workspace starts as NaN."""
    c = K.get(name)
    t = tensors(c)
    B, L, C = c["logits"].shape
    G = 64
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def guarded(n, fill=777.0, off=0, dtype=torch.float32):
        buf = torch.full((n + 2 * G + off,), fill, dtype=dtype, device=DEV)
        return buf, buf[G + off:G + off + n]
    lg_b, lg = guarded(B * L * C, 0.0, shift)
    lg.copy_(t["logits"].reshape(-1))
    bufs = {"q": guarded(B * L), "loss": guarded(B), "qsum": guarded(B), "grad": guarded(B * L * C, off=shift),
            "ws": guarded(lib.fd_quality_loss_workspace_bytes(B) // 8, float("nan"), dtype=torch.float64)}
    v = {k: b[1] for k, b in bufs.items()}
    assert lg.data_ptr() % 16 == (4 * shift) % 16 and v["grad"].data_ptr() % 16 == (4 * shift) % 16
    _lib.check(lib.fd_ltrb_quality(t["reg_pred"].data_ptr(), t["reg_target"].data_ptr(), t["labels"].data_ptr(), B, L, v["q"].data_ptr(), st), "fd_ltrb_quality")
    k = ops.QUALITY_KIND[kind]
    _lib.check(lib.fd_quality_loss_fwd(lg.data_ptr(), t["labels"].data_ptr(), v["q"].data_ptr(), B, L, C, k, 0.75, 2.0, v["loss"].data_ptr(),
                                       v["qsum"].data_ptr(), v["ws"].data_ptr(), st), "fd_quality_loss_fwd")
    _lib.check(lib.fd_quality_loss_bwd(lg.data_ptr(), t["labels"].data_ptr(), v["q"].data_ptr(), t["gscale"].data_ptr(), B, L, C, k, 0.75, 2.0,
                                       v["grad"].data_ptr(), st), "fd_quality_loss_bwd")
    torch.cuda.synchronize()
    for key, (buf, view) in bufs.items():
        lo, hi = buf[:view.data_ptr() // buf.element_size() - buf.data_ptr() // buf.element_size()], buf[-G:]
        ok = (lambda x: bool(torch.isnan(x).all())) if key == "ws" else (lambda x: bool((x == 777.0).all()))
        assert lo.numel() >= G and ok(lo) and ok(hi), key
    assert bool((lg_b[:G + shift] == 0).all()) and bool((lg_b[-G:] == 0).all())
    want = device(name)
    np.testing.assert_array_equal(v["q"].cpu().numpy().reshape(B, L).view(np.int32), want["q"].view(np.int32))
    np.testing.assert_array_equal(v["grad"].cpu().numpy().reshape(B, L, C).view(np.int32), want[kind][2].view(np.int32))
    np.testing.assert_array_equal(v["qsum"].cpu().numpy(), want[kind][1])
    if shift == 0:
        np.testing.assert_array_equal(v["loss"].cpu().numpy().view(np.int32), want[kind][0].view(np.int32))
    else:                   # other pieces, another (fixed) order of the same fp32 terms in the double sum
        assert Q.rel_err(v["loss"].cpu().numpy(), ref(name)[kind][np.float64][0]) <= FACTOR * yardstick(kind, 0)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_two_eager_runs_and_a_graph_replay_are_bit_identical(kind):
    t = tensors(K.get("b3_l341_c80"))
    other = tensors(K.get("b1_l255_c80"))

    def run():
        q = ops.ltrb_quality(t["reg_pred"], t["reg_target"], t["labels"])
        loss, qsum = ops.quality_loss_fwd(t["logits"], t["labels"], q, kind)
        return q, loss, qsum, ops.quality_loss_bwd(t["logits"], t["labels"], q, t["gscale"], kind)
    first, second = run(), run()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = run()
    torch.cuda.current_stream().wait_stream(side)
    for o in out:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b, g, w in zip(first, second, out, (device("b3_l341_c80")["q"],) + device("b3_l341_c80")[kind]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), g.view(torch.int32))
        np.testing.assert_array_equal(a.cpu().numpy().view(np.int32), w.view(np.int32))
    # the graph replays on new contents of the same buffers
    t["logits"][0].copy_(other["logits"][0, :1].expand_as(t["logits"][0]))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, run()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(out[1], first[1])


def test_wrapper_refusals():
    t = tensors(K.get("b3_l255_c3"))
    q = ops.ltrb_quality(t["reg_pred"], t["reg_target"], t["labels"])
    for bad in (lambda: ops.quality_loss_fwd(t["logits"], t["labels"], q, "focal"),
                lambda: ops.quality_loss_fwd(t["logits"].half(), t["labels"], q, "qfl"),
                lambda: ops.quality_loss_fwd(t["logits"], t["labels"].int(), q, "qfl"),
                lambda: ops.quality_loss_fwd(t["logits"], t["labels"], q[:, :-1], "vfl"),
                lambda: ops.quality_loss_fwd(t["logits"].transpose(0, 1), t["labels"].t(), q.t(), "vfl"),
                lambda: ops.quality_loss_fwd(t["logits"], t["labels"], q, "qfl", gamma=1.5),
                lambda: ops.quality_loss_bwd(t["logits"], t["labels"], q, t["gscale"][:2], "qfl"),
                lambda: ops.quality_loss_bwd(t["logits"], t["labels"], q, t["gscale"], "vfl", gamma=3.0),
                lambda: ops.ltrb_quality(t["reg_pred"][..., :3], t["reg_target"], t["labels"]),
                lambda: ops.ltrb_quality(t["reg_pred"].double(), t["reg_target"], t["labels"]),
                lambda: ops.ltrb_quality(t["reg_pred"].cpu(), t["reg_target"].cpu(), t["labels"].cpu())):
        with pytest.raises(_lib.FdError):
            bad()
    with pytest.raises(_lib.FdError) as e:
        ops.quality_loss_fwd(t["logits"], t["labels"], q, "qfl", gamma=1.5)
    assert e.value.rc == _lib.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------- FCOSLoss end to end
def as_maps(c, dtype=torch.float32):
    """The flattened predictions of a SimOTA case cut back into the head's three lists of NCHW maps, requiring grad."""
    cl, cn, rp = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("cls", "cnt", "reg"))
    B = cl.shape[0]
    out, start = ([], [], []), 0
    for h, w in c["level_hw"]:
        for lst, t in zip(out, (cl, cn[..., None], rp)):
            lst.append(t[:, start:start + h * w].reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous().to(dtype).requires_grad_(True))
        start += h * w
    return out


def pyramid341():
    c = SK.get("rand128x128_q10")
    assert sum(h * w for h, w in c["level_hw"]) == 341 and c["cls"].shape == (3, 341, 20)
    gt, labels = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("gt", "labels"))
    return c, gt, labels


@pytest.mark.parametrize("quality,norm", [("iou", "num_pos"), ("cnt", "num_pos"), ("iou", "quality"), ("cnt", "quality")])
@pytest.mark.parametrize("kind", Q.KINDS)
def test_fcos_loss_end_to_end(kind, quality, norm):
    """The 341-location pyramid of a 128 x 128 image, 20 classes, targets by SimOTAGenTargets(quality="iou"), whose cnt target is what
    quality="cnt" reads.  The cls term against the float64 restatement fed the same tensors: 8 x the loss yardstick plus four fp32
    roundings (the stored sum, the division by the normaliser, the sum and the division of the mean), its gradient on the cls maps
    within 8 x the gradient yardstick, and no contribution at all to the reg maps' gradient."""
    c, gt, labels = pyramid341()
    out = as_maps(c)
    target = SimOTAGenTargets(c["strides"], quality="iou")([out, gt, labels])
    assert int((target[0] > 0).sum(1).min()) >= 1
    losses = FCOSLoss("giou", cls_mode=kind, quality=quality, cls_norm=norm)([out, target])
    assert all(bool(torch.isfinite(v)) for v in losses) and torch.equal(losses[3], losses[0] + losses[1] + losses[2])
    lab = target[0][..., 0].cpu().numpy()
    reg_flat = flatten_levels(out[2]).detach()
    if quality == "iou":
        q = Q.quality(reg_flat.cpu().numpy(), target[2].cpu().numpy(), lab)
        assert torch.equal(ops.ltrb_quality(reg_flat, target[2], target[0]).cpu(), torch.from_numpy(q))
    else:
        q = np.where(lab > 0, np.maximum(target[1][..., 0].cpu().numpy(), F(0)), F(0))
    assert ((q > 0) & (q < 1)).any()
    logits = flatten_levels(out[0]).detach().cpu().numpy()
    l64, qs64, g64 = Q.loss_and_grad(kind, logits, lab, q)
    B = l64.shape[0]
    nrm = np.maximum((lab > 0).sum(1), 1).astype(np.float64) if norm == "num_pos" else np.maximum(qs64, 1.0)
    want = float((l64 / nrm).mean())
    got = float(losses[0].detach())
    print(f"{kind} {quality} {norm}: cls loss {got!r}, float64 {want!r}, relative difference {abs(got / want - 1):.3e}")
    assert abs(got / want - 1) <= FACTOR * yardstick(kind, 0) + 4 * EPS32
    # the parent's other two terms are untouched
    base = FCOSLoss("giou")([out, target])
    assert torch.equal(base[1], losses[1]) and torch.equal(base[2], losses[2])
    # backward reaches the cls maps ...
    gcls = torch.autograd.grad(losses[0], out[0], retain_graph=True)
    gflat = flatten_levels(gcls).cpu().numpy()
    gwant = g64 / (B * nrm)[:, None, None]
    dg = Q.rel_err(gflat, gwant)
    print(f"   gradient on the cls maps: device {dg:.3e}, bound {FACTOR * yardstick(kind, 2) + 2 * EPS32:.3e}")
    assert np.abs(gflat).max() > 0 and dg <= FACTOR * yardstick(kind, 2) + 2 * EPS32
    assert Q.max_err(gflat, gwant) <= FACTOR * yardstick(kind, 2, Q.max_err) + 2 * EPS32
    # ... and nothing of the cls term reaches the reg maps (q is a target) or the cnt maps
    assert all(g is None for g in torch.autograd.grad(losses[0], out[2] + out[1], retain_graph=True, allow_unused=True))
    with_cls = torch.autograd.grad(losses[3], out[2], retain_graph=True)
    without = torch.autograd.grad(losses[1] + losses[2], out[2], retain_graph=True)
    for a, b in zip(with_cls, without):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert any(bool(a.any()) for a in with_cls)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_fcos_loss_on_f16_maps(kind):
    """AMP maps: read as fp32, so the values are those of the rounded maps, and the gradients come back in the maps' dtype."""
    c, gt, labels = pyramid341()
    half = as_maps(c, torch.float16)
    full = [[t.detach().float().requires_grad_(True) for t in lst] for lst in half]
    target = SimOTAGenTargets(c["strides"])([half, gt, labels])
    lh = FCOSLoss("giou", cls_mode=kind)([half, target])
    lf = FCOSLoss("giou", cls_mode=kind)([full, target])
    assert lh[0].dtype == torch.float32 and torch.equal(lh[0], lf[0])
    gh = torch.autograd.grad(lh[3], half[0] + half[2])
    gf = torch.autograd.grad(lf[3], full[0] + full[2])
    for a, b in zip(gh, gf):
        assert a.dtype == torch.float16 and torch.equal(a, b.half()) and bool(torch.isfinite(a).all())


def test_default_fcos_loss_is_the_parent_code_path():
    c, gt, labels = pyramid341()
    out = as_maps(c)
    target = SimOTAGenTargets(c["strides"])([out, gt, labels])
    n0 = ops.LAUNCHES[0]
    losses = FCOSLoss("giou")([out, target])
    assert ops.LAUNCHES[0] - n0 == 3                    # focal, bce, ltrb forward: nothing of the quality path
    num_pos = (target[1][..., 0] > -1).sum(1).clamp(min=1).float()
    want = (ops.focal_loss_fwd(flatten_levels(out[0]).detach().contiguous(), target[0][..., 0].contiguous()) / num_pos).mean()
    assert torch.equal(losses[0].detach(), want)
    assert torch.equal(FCOSLoss()([out, target])[3], losses[3])
    n0 = ops.LAUNCHES[0]
    FCOSLoss("giou", cls_mode="qfl")([out, target])
    assert ops.LAUNCHES[0] - n0 == 4                    # + fd_ltrb_quality


def test_compute_cls_loss_quality_takes_a_quality_of_the_callers():
    t = tensors(K.get("b3_l341_c80"))
    q = torch.rand(3, 341, device=DEV)
    mask = t["labels"] > 0
    logits = t["logits"].clone().requires_grad_(True)
    loss = compute_cls_loss_quality(logits, t["labels"][..., None], q, mask, "vfl", "quality")
    l64, qs64, g64 = Q.loss_and_grad("vfl", t["logits"].cpu().numpy(), t["labels"].cpu().numpy(), q.cpu().numpy())
    np.testing.assert_allclose(loss.detach().cpu().numpy(), l64 / np.maximum(qs64, 1.0), rtol=FACTOR * yardstick("vfl", 0) + 2 * EPS32)
    loss.sum().backward()
    assert Q.rel_err(logits.grad.cpu().numpy(), g64 / np.maximum(qs64, 1.0)[:, None, None]) <= FACTOR * yardstick("vfl", 2) + 2 * EPS32


def test_one_training_step_on_simota_targets_with_qfl():
    """A HalfInvertedStageFPN + HISFCOSHead of width 64 in train() mode on a 128 x 128 image, as tests/test_simota_gpu.py builds it."""
    c, gt, labels = pyramid341()
    torch.manual_seed(3)
    fpn, head = HalfInvertedStageFPN([64, 128, 256], 64).to(DEV).train(), HISFCOSHead(64, 20, 0.01).to(DEV).train()
    feats = [torch.randn(3, ch, 128 // s, 128 // s, device=DEV) for ch, s in ((64, 8), (128, 16), (256, 32))]
    params = [p for mod in (fpn, head) for n, p in mod.named_parameters() if p.requires_grad and not n.startswith("gn3.")]
    out = head(fpn(feats))
    assert [tuple(t.shape[2:]) for t in out[0]] == c["level_hw"]
    target = SimOTAGenTargets(c["strides"])([out, gt, labels])
    assert int((target[0] > 0).sum(1).min()) >= 1
    losses = FCOSLoss("giou", cls_mode="qfl")([out, target])
    grads = torch.autograd.grad(losses[-1], params, allow_unused=False)
    print("losses", [float(v.detach()) for v in losses])
    assert all(bool(torch.isfinite(v)) for v in losses) and float(losses[0].detach()) > 0
    assert all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
