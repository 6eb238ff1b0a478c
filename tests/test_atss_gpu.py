"""fd_atss_gen_targets on the device against the numpy restatement (tests/atss_ref.py) on the cases of tests/atss_cases.py
(test_atss_cpu.py proves what each case exercises): cls / reg / npos exactly, thr bit for bit, cnt within rtol 1e-6 (the bar
tests/test_loss_edges_gpu.py sets for the same centre-ness expression).  Then the candidates' IoUs against ops.pairwise_iou, guard
bytes around every output and a poisoned workspace, capture in a torch.cuda.graph, and FCOSLoss('giou') with its backward."""
import ctypes

import numpy as np
import pytest
import torch

import atss_cases as K
import atss_ref as A
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd.model.loss import FCOSLoss
from pytorch_object_detection_amd.model.modules.head import ATSSGenTargets
from pytorch_object_detection_amd.model.od.HISFcos import HalfInvertedStageFPN, HISFCOSHead

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CNT_RTOL = 1e-6
_REF = {}


def ref(name):
    """One restatement per case, shared by every test and never modified."""
    if name not in _REF:
        c = K.get(name)
        r = A.atss_gen_targets(c["gt"], c["labels"], c["level_hw"], c["strides"], c["topk"], c["anchor_scale"], c["inside_eps"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = (c, r)
    return _REF[name]


def dev(c):
    return torch.from_numpy(c["gt"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV)


def same_bits(got, want, what):
    """fp64 arrays equal bit for bit; NaN (padding rows) must sit in the same places."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.int64), want[ok].view(np.int64), err_msg=what)


def check_triple(cls, cnt, reg, r, what):
    B, L = r["cls"].shape
    assert cls.shape == (B, L, 1) and cls.dtype == torch.int64 and cnt.shape == (B, L, 1) and reg.shape == (B, L, 4), what
    np.testing.assert_array_equal(cls[..., 0].cpu().numpy(), r["cls"], err_msg=what)
    np.testing.assert_array_equal(reg.cpu().numpy(), r["reg"], err_msg=what)
    got = cnt[..., 0].cpu().numpy()
    pos = r["cls"] > 0
    if pos.any():
        print(what, "cnt max rel err", float(np.abs(got[pos] / r["cnt"][pos] - 1).max()))
    np.testing.assert_allclose(got, r["cnt"], rtol=CNT_RTOL, atol=0, err_msg=what)


@pytest.mark.parametrize("name", K.ALL)
def test_targets_threshold_and_counts_equal_the_restatement(name):
    c, r = ref(name)
    gt, labels = dev(c)
    cls, cnt, reg, thr, npos = ops.atss_gen_targets(gt, labels, c["level_hw"], c["strides"], c["topk"], c["anchor_scale"], c["inside_eps"],
                                                    return_stats=True)
    check_triple(cls, cnt, reg, r, name + " ops")
    assert thr.dtype == torch.float64 and npos.dtype == torch.int32
    np.testing.assert_array_equal(npos.cpu().numpy(), r["npos"])
    same_bits(thr.cpu().numpy(), r["thr"], name + " thr")
    # the module form: level sizes read from out[0], the call contract of FCOSGenTargets
    out = [[torch.zeros(labels.shape[0], 1, h, w, device=DEV) for h, w in c["level_hw"]]]
    triple = ATSSGenTargets(c["strides"], c["topk"], c["anchor_scale"], c["inside_eps"])([out, gt, labels])
    assert len(triple) == 3
    check_triple(*triple, r, name + " module")
    for a, b in zip(triple, (cls, cnt, reg)):
        assert torch.equal(a, b)


def test_defaults_are_topk_9_scale_8_eps_001():
    c, r = ref("rand64x96_k9_a8")
    gt, labels = dev(c)
    check_triple(*ops.atss_gen_targets(gt, labels, c["level_hw"], c["strides"]), r, "ops defaults")
    out = [[torch.zeros(3, 1, h, w, device=DEV) for h, w in c["level_hw"]]]
    check_triple(*ATSSGenTargets(c["strides"])([out, gt, labels]), r, "module defaults")


@pytest.mark.parametrize("name", ["rand64x96_k9_a8", "rand256x320_k16_a4", "equal_ious", "grid5_k16"])
def test_candidate_ious_are_those_of_pairwise_iou(name):
    """The kernel publishes no IoU, but thr and npos are functions of the candidates' IoUs alone: with the IoUs that
    ops.pairwise_iou (no "+1") gives on the same anchors and boxes, the fp64 statistics must reproduce the device's thr bit for
    bit and its npos exactly -- and those IoUs are the restatement's, bit for bit."""
    c, r = ref(name)
    gt, labels = dev(c)
    *_, thr, npos = ops.atss_gen_targets(gt, labels, c["level_hw"], c["strides"], c["topk"], c["anchor_scale"], c["inside_eps"], return_stats=True)
    thr, npos = thr.cpu().numpy(), npos.cpu().numpy()
    cx, cy, lv, _ = A.centres(c["level_hw"], c["strides"])
    st = np.asarray(c["strides"])[lv]
    rows = sorted(r["cand"])
    assert rows
    anchors, spans, start = [], [], 0
    for b, m in rows:
        loc = r["cand"][(b, m)]
        rad = (F(c["anchor_scale"]) * st[loc].astype(F)) / F(2)
        spans.append((start, start + len(loc)))
        start += len(loc)
        anchors.append(np.stack([cx[loc] - rad, cy[loc] - rad, cx[loc] + rad, cy[loc] + rad], 1))
    boxes = np.stack([c["gt"][b, m] for b, m in rows])
    iou = ops.pairwise_iou(torch.from_numpy(np.concatenate(anchors)).to(DEV), torch.from_numpy(boxes).to(DEV), False).cpu().numpy()
    for j, (b, m) in enumerate(rows):
        loc = r["cand"][(b, m)]
        v = iou[spans[j][0]:spans[j][1], j]
        np.testing.assert_array_equal(v.view(np.int32), A.anchor_iou(cx[loc], cy[loc], st[loc], c["anchor_scale"], c["gt"][b, m]).view(np.int32))
        t = A.threshold(v)
        same_bits([thr[b, m]], [t], f"{name} row {(b, m)}")
        box = c["gt"][b, m]
        inside = np.minimum(np.minimum(cx[loc] - box[0], cy[loc] - box[1]), np.minimum(box[2] - cx[loc], box[3] - cy[loc]))
        assert int(((v.astype(np.float64) >= t) & (inside > F(c["inside_eps"]))).sum()) == npos[b, m]


@pytest.mark.parametrize("name", ["rand64x96_k16_a8", "twin_rows", "skipped_rows"])
def test_nothing_outside_the_outputs_changes_and_the_workspace_may_hold_anything(name):
    """The C ABI on buffers cut out of larger ones: guard elements before and after each output keep their pattern, the workspace starts
    as non-zero bytes (the call clears it itself) and its guards stay too."""
    c, r = ref(name)
    gt, labels = dev(c)
    B, M = c["labels"].shape
    L = r["cls"].shape[1]
    G = 64                                            # guard elements on each side (a multiple of 4 floats: reg stays 16-byte aligned)

    def guarded(n, dtype, fill):
        t = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
        return t, t[G:G + n]
    cls_b, cls = guarded(B * L, torch.int64, 0x5A5A5A5A5A5A5A5A)
    cnt_b, cnt = guarded(B * L, torch.float32, 777.0)
    reg_b, reg = guarded(B * L * 4, torch.float32, 777.0)
    thr_b, thr = guarded(B * M, torch.float64, 777.0)
    npos_b, npos = guarded(B * M, torch.int32, 0x5A5A5A5A)
    assert _lib.lib().fd_atss_workspace_bytes(B, L) == B * L * 8
    ws_b, ws = guarded(B * L, torch.int64, -0x5A5A5A5A5A5A5A5B)      # every byte 0xA5
    segs = _lib.Segs.make(B, c["level_hw"])
    st = (ctypes.c_int32 * len(c["strides"]))(*c["strides"])
    _lib.check(_lib.lib().fd_atss_gen_targets(gt.data_ptr(), labels.data_ptr(), M, ctypes.byref(segs), st, c["topk"], c["anchor_scale"], c["inside_eps"],
                                              cls.data_ptr(), cnt.data_ptr(), reg.data_ptr(), thr.data_ptr(), npos.data_ptr(), ws.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "fd_atss_gen_targets")
    torch.cuda.synchronize()
    for buf, fill in ((cls_b, 0x5A5A5A5A5A5A5A5A), (cnt_b, 777.0), (reg_b, 777.0), (thr_b, 777.0), (npos_b, 0x5A5A5A5A), (ws_b, -0x5A5A5A5A5A5A5A5B)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    check_triple(cls.view(B, L, 1), cnt.view(B, L, 1), reg.view(B, L, 4), r, name + " guarded")
    np.testing.assert_array_equal(npos.view(B, M).cpu().numpy(), r["npos"])
    same_bits(thr.view(B, M).cpu().numpy(), r["thr"], name + " thr")
    # what the call leaves in the workspace: 0 where nothing was claimed, (iou bits, ~row) of the owner elsewhere -- no poison
    words = ws.view(B, L).cpu().numpy()
    assert ((words == 0) == (r["owner"] < 0)).all()
    own = r["owner"] >= 0
    np.testing.assert_array_equal(~(words[own] & 0xFFFFFFFF).astype(np.uint32), r["owner"][own].astype(np.uint32))


def test_captured_call_replays_on_new_boxes():
    c0, _ = ref("rand64x96_k9_a8")
    others = [ref(n) for n in ("rand64x96_k9_a4", "rand64x96_k16_a8")]        # same shapes, other boxes and labels
    gt, labels = (t.clone() for t in dev(c0))
    args = (c0["level_hw"], c0["strides"], 9, 8.0, 0.01)
    ops.atss_gen_targets(gt, labels, *args, return_stats=True)               # one eager call first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ops.atss_gen_targets(gt, labels, *args, return_stats=True)
    torch.cuda.current_stream().wait_stream(side)
    for c, _ in others:
        gt.copy_(torch.from_numpy(c["gt"]))
        labels.copy_(torch.from_numpy(c["labels"]))
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.atss_gen_targets(gt.clone(), labels.clone(), *args, return_stats=True)
        r = A.atss_gen_targets(c["gt"], c["labels"], *args)
        check_triple(*out[:3], r, "replay")
        for a, b in zip(out, eager):
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_fcos_loss_and_backward_on_atss_targets():
    """A HalfInvertedStageFPN + HISFCOSHead of width 64 (channels 64 / 128 / 256 -> 64) in train() mode on a 128 x 128 image, the
    smallest whose five levels (16, 8, 4, 2, 1) the FPN's 2 x 2 pools produce.  Width 64 is the narrowest that trains on the HIP nodes
    alone: at the width of fixture g8 (32) the HisBlocks hold 16-channel convs whose data gradient is a stock op, which FD_STRICT=1
    (tests/conftest.py) refuses."""
    c, r = ref("rand128x128_k9_a8")
    torch.manual_seed(3)
    fpn, head = HalfInvertedStageFPN([64, 128, 256], 64).to(DEV).train(), HISFCOSHead(64, 20, 0.01).to(DEV).train()
    feats = [torch.randn(3, ch, 128 // s, 128 // s, device=DEV) for ch, s in ((64, 8), (128, 16), (256, 32))]
    out = head(fpn(feats))
    assert [tuple(t.shape[2:]) for t in out[0]] == c["level_hw"]
    gt, labels = dev(c)
    target = ATSSGenTargets(c["strides"])([out, gt, labels])
    check_triple(*target, r, "module on the model's output")
    assert (r["cls"] > 0).sum(1).min() >= 1 and (r["claims"] >= 2).any()
    losses = FCOSLoss("giou")([out, target])
    ref_target = (torch.from_numpy(r["cls"].copy())[..., None].to(DEV), torch.from_numpy(r["cnt"].copy())[..., None].to(DEV),
                  torch.from_numpy(r["reg"].copy()).to(DEV))
    want = FCOSLoss("giou")([out, ref_target])
    for k, (a, b) in enumerate(zip(losses, want)):
        assert bool(torch.isfinite(a).all())
        print("loss", k, float(a.detach()), float(b.detach()))
        # cls and reg targets are equal; cnt targets agree within CNT_RTOL and enter the centre-ness loss linearly (softplus(x) - t x)
        np.testing.assert_allclose(float(a.detach()), float(b.detach()), rtol=1e-6 if k in (0, 2) else 1e-5)
    assert float(losses[0].detach()) > 0 and float(losses[2].detach()) > 0
    losses[-1].backward()
    n = 0
    for mod in (fpn, head):
        for pname, p in mod.named_parameters():
            if p.requires_grad and not pname.startswith("gn3."):         # the FPN's gn3 exists and is never used, as in the reference
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), pname
                n += 1
    assert n > 20
