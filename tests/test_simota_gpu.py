"""fd_simota_gen_targets on the device against the numpy restatement (tests/simota_ref.py) on the cases of tests/simota_cases.py
(test_simota_cpu.py proves what each case exercises and the margins of the random ones).

pair matrices   pair_iou bit for bit (IEEE operations only); pair_cost against the float64 restatement relative to 1 + |cost|,
                within 8 times what the fp32 numpy restatement deviates from it on the same cases (both figures are printed)
selection       cls / reg / k / ncand exactly select() of the device's own pair matrices; cnt within 1e-6 (centre-ness, the bound
                of tests/test_atss_gpu.py for the same expression) or bit for bit the winning pair_iou (quality "iou")
whole assigner  on the random and the hand-derived cases cls / reg / k exactly the all-numpy pipeline
then guard bytes round every output with a poisoned workspace, capture in a torch.cuda.graph, the module on lists of NCHW maps
(f16, requiring grad), and FCOSLoss('giou') with its backward on SimOTA targets."""
import ctypes

import numpy as np
import pytest
import torch

import simota_cases as K
import simota_ref as S
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd.model.loss import FCOSLoss, flatten_levels
from pytorch_object_detection_amd.model.modules.head import SimOTAGenTargets
from pytorch_object_detection_amd.model.od.HISFcos import HalfInvertedStageFPN, HISFCOSHead

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CNT_RTOL = 1e-6
COST_FACTOR = 8           # the device may deviate from float64 this many times as far as fp32 numpy does: a few ulp per expf / logf over <= 81 terms
QUALITY = {0: "centerness", 1: "iou"}
EXACT = ["equal_cost_pair", "preferred_beats_cheaper", "two_exact", "two_exact_q16", "all_zero_iou", "few_candidates", "no_candidates",
         "inside_boundary", "twin_rows", "no_rows"]       # hand-derived: equal inputs give equal costs on any evaluation, so nothing needs a margin
_REF, _DEV = {}, {}


def ref(name):
    """One restatement per case (fp32 pipeline, and the pair matrices with the cost in float64), shared by every test, read-only."""
    if name not in _REF:
        c = K.get(name)
        a = (c["cls"], c["cnt"], c["reg"], c["gt"], c["labels"], c["level_hw"], c["strides"])
        r = S.simota_gen_targets(*a, **K.args(c))
        p64 = S.pairs(*a, c["centre_radius"], c["iou_weight"], c["inside_eps"], cost64=True)
        for d in (r, r["pairs"], p64):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _REF[name] = (c, r, p64)
    return _REF[name]


def rel_dev(cost, cost64, cand):
    if not cand.any():
        return 0.0
    return float((np.abs(cost[cand].astype(np.float64) - cost64[cand]) / (1.0 + np.abs(cost64[cand]))).max())


def yardstick():
    """The largest deviation of the fp32 numpy cost from the float64 one over every case, relative to 1 + |cost|."""
    if "y" not in _REF:
        _REF["y"] = max(rel_dev(ref(n)[1]["pairs"]["cost"], ref(n)[2]["cost"], ref(n)[2]["cand"]) for n in K.ALL)
    return _REF["y"]


def tensors(c):
    return tuple(torch.from_numpy(np.array(c[k])).to(DEV) for k in ("cls", "cnt", "reg", "gt", "labels"))


def call(c, return_stats=True, **kw):
    a = dict(top_q=c["top_q"], centre_radius=c["centre_radius"], iou_weight=c["iou_weight"], inside_eps=c["inside_eps"], quality=QUALITY[c["quality"]])
    a.update(kw)
    return ops.simota_gen_targets(*tensors(c), c["level_hw"], c["strides"], return_stats=return_stats, **a)


def device(name):
    """One device run per case with the statistics, as numpy."""
    if name not in _DEV:
        out = call(K.get(name))
        torch.cuda.synchronize()
        _DEV[name] = tuple(t.cpu().numpy() for t in out)
        for v in _DEV[name]:
            v.setflags(write=False)
    return _DEV[name]


def check_against(got, want, quality, what):
    """got: (cls [B,L,1], cnt [B,L,1], reg [B,L,4], ..., k, ncand) numpy; want: a select() dict."""
    cls, cnt, reg = got[0][..., 0], got[1][..., 0], got[2]
    np.testing.assert_array_equal(cls, want["cls"], err_msg=what)
    np.testing.assert_array_equal(reg, want["reg"], err_msg=what)
    if len(got) > 3:
        np.testing.assert_array_equal(got[5], want["k"], err_msg=what)
        np.testing.assert_array_equal(got[6], want["ncand"], err_msg=what)
    assert not np.isnan(cnt).any() and not np.isnan(reg).any(), what
    if quality:
        np.testing.assert_array_equal(cnt.view(np.int32), want["cnt"].view(np.int32), err_msg=what)
    else:
        pos = want["cls"] > 0
        if pos.any():
            print(what, "cnt max rel err", float(np.abs(cnt[pos] / want["cnt"][pos] - 1).max()))
        np.testing.assert_allclose(cnt, want["cnt"], rtol=CNT_RTOL, atol=0, err_msg=what)


# ---------------------------------------------------------------------------------------------------- pair matrices
@pytest.mark.parametrize("name", K.ALL)
def test_pair_iou_bit_for_bit_and_pair_cost_within_the_measured_bound(name):
    c, r, p64 = ref(name)
    got = device(name)
    piou, pcost = got[3], got[4]
    B, M = c["labels"].shape
    L = c["cls"].shape[1]
    assert piou.shape == pcost.shape == (B, M, L) and piou.dtype == pcost.dtype == np.float32
    np.testing.assert_array_equal(piou.view(np.int32), r["pairs"]["iou"].view(np.int32))
    cand = p64["cand"]
    np.testing.assert_array_equal(np.isfinite(pcost), cand)                   # a candidate's cost is at most FLT_MAX
    assert np.isposinf(pcost[~cand]).all() and not piou[~cand].any() and not np.signbit(pcost).any()
    y, d = yardstick(), rel_dev(pcost, p64["cost"], cand)
    print(f"{name}: fp32 numpy deviates from float64 by at most {y:.3e} over all cases (this case {rel_dev(r['pairs']['cost'], p64['cost'], cand):.3e}); "
          f"the device by {d:.3e}; bound {COST_FACTOR * y:.3e}")
    assert 0 < y < 1e-5                        # a yardstick of fp32 rounding, not of something broken
    assert d <= COST_FACTOR * y


# ---------------------------------------------------------------------------------------------------- selection and outputs
@pytest.mark.parametrize("name", K.ALL)
def test_selection_is_select_of_the_devices_own_pair_matrices(name):
    c, r, p64 = ref(name)
    got = device(name)
    piou, pcost = got[3], got[4]
    want = S.select(piou, pcost, np.isfinite(pcost), r["pairs"]["pref"], c["gt"], c["labels"], c["level_hw"], c["strides"], c["top_q"], c["quality"])
    assert got[0].dtype == np.int64 and got[5].dtype == got[6].dtype == np.int32
    check_against(got, want, c["quality"], name)


@pytest.mark.parametrize("name", list(K.RANDOM) + EXACT)
def test_whole_assigner_equals_the_numpy_pipeline(name):
    c, r, _ = ref(name)
    check_against(device(name), r, c["quality"], name)
    # without the statistics the same triple comes back (pair matrices in the workspace only)
    triple = call(c, return_stats=False)
    assert len(triple) == 3
    for a, b in zip(triple, device(name)):
        assert a.shape == b.shape and np.array_equal(a.cpu().numpy(), b, equal_nan=True)


def test_defaults():
    c, r, _ = ref("rand64x96_q10_v0")
    assert (c["top_q"], c["centre_radius"], c["iou_weight"], c["inside_eps"], c["quality"]) == (10, 2.5, 3.0, 0.01, 0)
    got = ops.simota_gen_targets(*tensors(c), c["level_hw"], c["strides"])
    check_against(tuple(t.cpu().numpy() for t in got), r, 0, "ops defaults")


@pytest.mark.parametrize("top_q", [1, 10, 16])
@pytest.mark.parametrize("quality", [0, 1])
def test_top_q_and_quality_on_one_case(top_q, quality):
    """The 256 x 320 case of 80 classes under every top_q and both cnt targets: select() of the device's own matrices."""
    c = dict(K.get("rand256x320_q10_v0"), top_q=top_q, quality=quality)
    _, r, _ = ref("rand256x320_q10_v0")
    got = tuple(t.cpu().numpy() for t in call(c))
    np.testing.assert_array_equal(got[3].view(np.int32), device("rand256x320_q10_v0")[3].view(np.int32))
    np.testing.assert_array_equal(got[4].view(np.int32), device("rand256x320_q10_v0")[4].view(np.int32))
    want = S.select(got[3], got[4], np.isfinite(got[4]), r["pairs"]["pref"], c["gt"], c["labels"], c["level_hw"], c["strides"], top_q, quality)
    check_against(got, want, quality, f"top_q {top_q} quality {quality}")
    assert (want["k"].max() == 1) == (top_q == 1) and (want["cls"] > 0).any()


# ---------------------------------------------------------------------------------------------------- memory and capture
@pytest.mark.parametrize("name", ["rand64x96_q16_v1", "twin_rows", "skipped_rows", "non_finite_q1"])
@pytest.mark.parametrize("poison", ["nan", "ff"])
def test_nothing_outside_the_outputs_changes_and_the_workspace_may_hold_anything(name, poison):
    """The C ABI on buffers cut out of larger ones: guard elements before and after each output keep their pattern; the workspace starts
    as NaN floats or 0xFF bytes (the call initialises what it reads) and its guards stay too."""
    c, r, _ = ref(name)
    want = device(name)
    cl, cn, rp, gt, labels = tensors(c)
    B, M = c["labels"].shape
    L, Cn = c["cls"].shape[1], c["cls"].shape[2]
    G = 64                                            # guard elements on each side (a multiple of 4 floats: reg stays 16-byte aligned)

    def guarded(n, dtype, fill):
        t = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
        return t, t[G:G + n]
    bufs = {"cls": guarded(B * L, torch.int64, 0x5A5A5A5A5A5A5A5A), "cnt": guarded(B * L, torch.float32, 777.0),
            "reg": guarded(B * L * 4, torch.float32, 777.0), "piou": guarded(B * M * L, torch.float32, 777.0),
            "pcost": guarded(B * M * L, torch.float32, 777.0), "k": guarded(B * M, torch.int32, 0x5A5A5A5A), "ncand": guarded(B * M, torch.int32, 0x5A5A5A5A)}
    fills = {"cls": 0x5A5A5A5A5A5A5A5A, "cnt": 777.0, "reg": 777.0, "piou": 777.0, "pcost": 777.0, "k": 0x5A5A5A5A, "ncand": 0x5A5A5A5A}
    nbytes = _lib.lib().fd_simota_workspace_bytes(B, M, L)
    assert nbytes == 8 * B * L * (1 + M)
    if poison == "nan":
        ws_b = torch.full((nbytes // 4 + 2 * G,), float("nan"), dtype=torch.float32, device=DEV)
        ws = ws_b[G:G + nbytes // 4]
        intact = lambda t: bool(torch.isnan(t).all())  # noqa: E731
    else:
        ws_b = torch.full((nbytes // 8 + 2 * G,), -1, dtype=torch.int64, device=DEV)
        ws = ws_b[G:G + nbytes // 8]
        intact = lambda t: bool((t == -1).all())  # noqa: E731
    segs = _lib.Segs.make(B, c["level_hw"])
    st = (ctypes.c_int32 * len(c["strides"]))(*c["strides"])
    v = {k: b[1] for k, b in bufs.items()}
    _lib.check(_lib.lib().fd_simota_gen_targets(cl.data_ptr(), cn.data_ptr(), rp.data_ptr(), Cn, gt.data_ptr(), labels.data_ptr(), M, ctypes.byref(segs), st,
                                                c["top_q"], c["centre_radius"], c["iou_weight"], c["inside_eps"], c["quality"], v["cls"].data_ptr(),
                                                v["cnt"].data_ptr(), v["reg"].data_ptr(), v["piou"].data_ptr(), v["pcost"].data_ptr(), v["k"].data_ptr(),
                                                v["ncand"].data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "fd_simota_gen_targets")
    torch.cuda.synchronize()
    for key, (buf, _) in bufs.items():
        assert bool((buf[:G] == fills[key]).all()) and bool((buf[-G:] == fills[key]).all()), key
    assert intact(ws_b[:G]) and intact(ws_b[-G:])
    got = (v["cls"].view(B, L, 1), v["cnt"].view(B, L, 1), v["reg"].view(B, L, 4), v["piou"].view(B, M, L), v["pcost"].view(B, M, L), v["k"].view(B, M),
           v["ncand"].view(B, M))
    for a, b in zip(got, want):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else a.dtype), b.view(np.int32 if b.dtype == np.float32 else b.dtype))


def test_captured_call_replays_on_new_predictions_and_boxes():
    c0 = K.get("rand64x96_q10_v0")
    others = [K.get(n) for n in ("rand64x96_q16_v1", "rand64x96_q1_v1")]        # same shapes (C = 80), other predictions, boxes and labels
    bufs = [t.clone() for t in tensors(c0)]
    args = (c0["level_hw"], c0["strides"], 10, 2.5, 3.0, 0.01, "iou")
    ops.simota_gen_targets(*bufs, *args, return_stats=True)               # one eager call first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ops.simota_gen_targets(*bufs, *args, return_stats=True)
    torch.cuda.current_stream().wait_stream(side)
    for c in others:
        for dst, src in zip(bufs, tensors(c)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.simota_gen_targets(*(t.clone() for t in bufs), *args, return_stats=True)
        assert bool((eager[0] > 0).any())
        for a, b in zip(out, eager):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---------------------------------------------------------------------------------------------------- module
def as_maps(c, dtype=torch.float32):
    """The flattened predictions of a case cut back into the head's three lists of NCHW maps."""
    cl, cn, rp = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("cls", "cnt", "reg"))
    B = cl.shape[0]
    out, start = ([], [], []), 0
    for h, w in c["level_hw"]:
        for lst, t in zip(out, (cl, cn[..., None], rp)):
            lst.append(t[:, start:start + h * w].reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous().to(dtype))
        start += h * w
    return out


@pytest.mark.parametrize("name", ["rand64x96_q10_v0", "rand256x320_q16_v1", "no_rows"])
def test_module_on_lists_of_nchw_maps(name):
    c, r, _ = ref(name)
    gt, labels = tensors(c)[3:]
    mod = SimOTAGenTargets(c["strides"], c["top_q"], c["centre_radius"], c["iou_weight"], c["inside_eps"], QUALITY[c["quality"]])
    out = as_maps(c)
    for lst in out:
        for t in lst:
            t.requires_grad_(True)
    triple = mod([out, gt, labels])
    assert len(triple) == 3 and not any(t.requires_grad for t in triple) and all(t.grad_fn is None for t in triple)
    check_against(tuple(t.cpu().numpy() for t in triple), r, c["quality"], name + " module")
    flat = [flatten_levels(lst).detach() for lst in out]
    for a, b in zip(triple, ops.simota_gen_targets(*flat, gt, labels, c["level_hw"], c["strides"], c["top_q"], c["centre_radius"], c["iou_weight"],
                                                    c["inside_eps"], QUALITY[c["quality"]])):
        assert torch.equal(a, b)
    # f16 maps (AMP): read as fp32, so the result is that of the rounded predictions
    half = as_maps(c, torch.float16)
    triple_h = mod([half, gt, labels])
    flat_h = [flatten_levels(lst).float() for lst in half]
    for a, b in zip(triple_h, ops.simota_gen_targets(*flat_h, gt, labels, c["level_hw"], c["strides"], c["top_q"], c["centre_radius"], c["iou_weight"],
                                                      c["inside_eps"], QUALITY[c["quality"]])):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert triple_h[1].dtype == torch.float32


def test_module_defaults_and_bad_arguments():
    c, r, _ = ref("rand64x96_q10_v0")
    gt, labels = tensors(c)[3:]
    check_against(tuple(t.cpu().numpy() for t in SimOTAGenTargets(c["strides"])([as_maps(c), gt, labels])), r, 0, "module defaults")
    cl, cn, rp = tensors(c)[:3]
    with pytest.raises(_lib.FdError):
        ops.simota_gen_targets(cl, cn, rp, gt, labels, c["level_hw"], c["strides"], quality="giou")
    with pytest.raises(_lib.FdError):
        ops.simota_gen_targets(cl.half(), cn, rp, gt, labels, c["level_hw"], c["strides"])
    with pytest.raises(_lib.FdError):
        ops.simota_gen_targets(cl[:, :-1], cn, rp, gt, labels, c["level_hw"], c["strides"])
    with pytest.raises(_lib.FdError):
        ops.simota_gen_targets(cl, cn, rp, gt, labels, c["level_hw"], c["strides"], top_q=17)


def test_fcos_loss_and_backward_on_simota_targets():
    """A HalfInvertedStageFPN + HISFCOSHead of width 64 in train() mode on a 128 x 128 image, as tests/test_atss_gpu.py builds it (the
    narrowest that trains on the HIP nodes alone).  One step on SimOTA targets of the model's own output: losses and gradients are finite
    and equal those of a step fed the same targets precomputed by ops.simota_gen_targets."""
    c = K.get("rand128x128_q10")
    torch.manual_seed(3)
    fpn, head = HalfInvertedStageFPN([64, 128, 256], 64).to(DEV).train(), HISFCOSHead(64, 20, 0.01).to(DEV).train()
    feats = [torch.randn(3, ch, 128 // s, 128 // s, device=DEV) for ch, s in ((64, 8), (128, 16), (256, 32))]
    gt, labels = tensors(c)[3:]
    params = [p for mod in (fpn, head) for n, p in mod.named_parameters() if p.requires_grad and not n.startswith("gn3.")]
    assert len(params) > 20

    def step(make_target):
        out = head(fpn(feats))
        assert [tuple(t.shape[2:]) for t in out[0]] == c["level_hw"]
        target = make_target(out)
        losses = FCOSLoss("giou")([out, target])
        grads = torch.autograd.grad(losses[-1], params, allow_unused=False)
        return out, target, losses, grads
    out, target, losses, grads = step(lambda o: SimOTAGenTargets(c["strides"])([o, gt, labels]))
    assert not any(t.requires_grad for t in target)
    npos = (target[0] > 0).sum(1)
    print("positives per image", npos.flatten().tolist(), "losses", [float(x.detach()) for x in losses])
    assert int(npos.min()) >= 1
    # the numpy pipeline on the model's own predictions agrees with select() of its own matrices: checked through ops
    flat = [flatten_levels([t.detach() for t in lst]).float() for lst in out]
    pre = ops.simota_gen_targets(*flat, gt, labels, c["level_hw"], c["strides"])
    for a, b in zip(target, pre):
        assert torch.equal(a, b)
    _, _, losses2, grads2 = step(lambda o: tuple(t.clone() for t in pre))
    for k, (a, b) in enumerate(zip(losses, losses2)):
        assert bool(torch.isfinite(a).all())
        # equal targets on equal predictions: what may differ is the summation order of the loss and gradient kernels' atomics
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-7)
    assert float(losses[0].detach()) > 0 and float(losses[2].detach()) > 0
    for g, g2 in zip(grads, grads2):
        assert bool(torch.isfinite(g).all())
        torch.testing.assert_close(g, g2, rtol=1e-4, atol=1e-6)
