"""The designed inputs of tests/loss_edge_cases.py hit the comparisons they claim to, and the tolerances of
test_loss_edges_gpu.py are meetable: oracle/torch_ref.py in fp32 stays inside them against the same functions in
float64 on the same inputs.  Runs without a GPU."""
import numpy as np
import pytest
import torch

import loss_edge_cases as E
from oracle import torch_ref as R


def _finite(*arrays):
    for a in arrays:
        assert np.isfinite(a).all()


# ---------------------------------------------------------------------------------------------------- LTRB
def ltrb_edges(p, t):
    """The oracle's intermediate quantities (iou_loss / giou_loss) on [N, 4] float64 rows -> {edge: bool [N]}.  An edge
    counts only where the term it decides reaches the loss, so that the comparison alone decides the gradient."""
    mn = torch.min(p, t)
    s_lr, s_tb = mn[:, 2] + mn[:, 0], mn[:, 3] + mn[:, 1]                # pre-clamp intersection width / height
    wi, hi = s_lr.clamp(min=0), s_tb.clamp(min=0)
    ov = wi * hi
    a1 = (p[:, 2] + p[:, 0]) * (p[:, 3] + p[:, 1])
    a2 = (t[:, 2] + t[:, 0]) * (t[:, 3] + t[:, 1])
    union = a1 + a2 - ov
    iou = ov / union
    mx = torch.max(p, t)
    wg, hg = (mx[:, 2] + mx[:, 0]).clamp(min=0), (mx[:, 3] + mx[:, 1]).clamp(min=0)
    g = wg * hg
    tie = p == t
    lr, tb = tie[:, 0] | tie[:, 2], tie[:, 1] | tie[:, 3]
    lr_open = (p[:, 0] <= t[:, 0]) | (p[:, 2] <= t[:, 2])               # min() routes some gradient to pred on this axis
    tb_open = (p[:, 1] <= t[:, 1]) | (p[:, 3] <= t[:, 3])
    return {
        "union_nonzero": union != 0, "enclosing_nonzero": g != 0,
        "min_tie": (lr & (s_lr >= 0) & (hi > 0)) | (tb & (s_tb >= 0) & (wi > 0)),
        "min_tie_unclamped_iou": ((lr & (s_lr >= 0) & (hi > 0)) | (tb & (s_tb >= 0) & (wi > 0))) & (iou >= 1e-6),
        "four_way_tie": tie.all(1),
        "partial_tie": tie.any(1) & ~tie.all(1),
        "enclosing_tie": ((lr & (hg > 0)) | (tb & (wg > 0))) & (g >= 1e-10),
        "zero_width": ((s_lr == 0) & (hi > 0) & lr_open) | ((s_tb == 0) & (wi > 0) & tb_open),
        "negative_sum": (s_lr < 0) | (s_tb < 0),
        "iou_clamped": iou < 1e-6,
        "iou_just_above_clamp": (iou >= 1e-6) & (iou < 1e-5),
        "enclosing_clamped": g < 1e-10,
    }


LTRB_EDGES = ("min_tie", "min_tie_unclamped_iou", "four_way_tie", "partial_tie", "enclosing_tie", "zero_width", "negative_sum",
              "iou_clamped", "iou_just_above_clamp", "enclosing_clamped")


@pytest.mark.parametrize("L", E.LS)
def test_ltrb_case_hits_every_edge(L):
    pred, tgt, mask = E.ltrb_case(L)
    assert mask.sum(1).tolist() == [0, L if L >= len(E.LTRB_ROWS) else 1, 1] and mask[2, L - 1]
    assert (pred[~mask] == 0).all() and (tgt[~mask] == 0).all()          # degenerate boxes wherever the mask is off
    edges = ltrb_edges(pred[mask].double(), tgt[mask].double())
    assert edges["union_nonzero"].all() and edges["enclosing_nonzero"].all()
    counts = {k: int(edges[k].sum()) for k in LTRB_EDGES}
    print(L, counts)
    for k in (LTRB_EDGES if L >= 255 else ("min_tie", "partial_tie", "enclosing_tie", "zero_width")):
        assert counts[k] >= 1, k
    if L > 256:                                                          # designed rows on both sides of the 256-thread stride
        full = ltrb_edges(pred[1].double(), tgt[1].double())
        rows = full["four_way_tie"] | full["zero_width"] | full["iou_clamped"]
        assert rows[:256].any() and rows[256:].any()


def test_ltrb_moderate_rows_fit_fp16():
    pred, tgt, mask = E.ltrb_case(257, E.LTRB_ROWS_MODERATE)
    assert (pred.half().float() == pred)[mask][-len(E.LTRB_ROWS_MODERATE):].all()
    for mode in ("iou", "giou"):
        loss, grad = E.ltrb_ref(pred.half().float(), tgt, mask, mode)
        _finite(loss, grad)
        assert np.abs(grad).max() < 60000


@pytest.mark.parametrize("mode", ["iou", "giou"])
@pytest.mark.parametrize("L", E.LS)
def test_ltrb_fp32_oracle_within_tolerance(L, mode):
    pred, tgt, mask = E.ltrb_case(L)
    loss, grad = E.ltrb_ref(pred, tgt, mask, mode)
    _finite(loss, grad)
    loss32, grad32 = E.ltrb_ref(pred, tgt, mask, mode, torch.float32)
    print(L, mode, "loss rel", np.abs(loss32 - loss).max() / np.abs(loss).max(), "grad abs", np.abs(grad32 - grad).max())
    np.testing.assert_allclose(loss32, loss, rtol=E.LOSS_RTOL)
    np.testing.assert_allclose(grad32, grad, **E.GRAD_TOL)
    assert loss[0] == 0 and (grad[0] == 0).all() and (grad[~mask.numpy()] == 0).all()
    # a perfect prediction: loss 0 and no gradient, in float64 up to its own rounding
    perfect = (pred == tgt).all(-1) & mask
    assert np.abs(grad[perfect.numpy()]).max(initial=0) < 1e-12 * max(1.0, np.abs(grad).max())


# ---------------------------------------------------------------------------------------------------- BCE
@pytest.mark.parametrize("L", E.LS)
def test_bce_case_covers_the_grid(L):
    x, t, mask = E.bce_case(L)
    npos = mask.sum(1)
    assert npos.tolist() == [0, L if L >= 40 else 1, 1]
    gscale = torch.tensor(E.IMG_W) / npos.clamp(min=1)
    seen = {(float(a), float(b)) for a, b in zip(x[mask], t[mask])}
    want = {(float(np.float32(a)), float(np.float32(b))) for a, b in E.BCE_COMBOS}
    if L >= 255:
        assert seen == want | {(-30.0, 0.5)}
    for a, b in E.BCE_CANCELLING:
        hit = mask & (x == a) & (t == b)
        assert (gscale[:, None].expand_as(x)[hit] <= 0.2).all()
    assert np.isfinite(x.numpy()).all() and (x[~mask].abs() == 100).all()


def test_bce_grid_gscale_is_small():
    x, t, gs = E.bce_grid()
    assert x.shape == (4, 10) and (gs <= 0.2).all() and len(set(gs.tolist())) == 4


@pytest.mark.parametrize("L", E.LS)
def test_bce_fp32_within_tolerance(L):
    x, t, mask = E.bce_case(L)
    loss, grad = E.bce_ref(x, t, mask)
    _finite(loss, grad)
    loss32, grad32 = E.bce_ref(x, t, mask, torch.float32)
    print(L, "loss rel", np.abs(loss32 - loss).max() / np.abs(loss).max(), "grad abs", np.abs(grad32 - grad).max())
    np.testing.assert_allclose(loss32, loss, rtol=E.LOSS_RTOL)
    np.testing.assert_allclose(grad32, grad, **E.GRAD_TOL)


def test_bce_grid_fp32_within_tolerance():
    loss, grad = E.bce_grid_ref()
    _finite(loss, grad)
    loss32, grad32 = E.bce_grid_ref(torch.float32)
    np.testing.assert_allclose(loss32, loss, rtol=E.LOSS_RTOL)
    np.testing.assert_allclose(grad32, grad, **E.GRAD_TOL)


# ---------------------------------------------------------------------------------------------------- focal
def _nchunk(L, C):
    return max(1, min(64, (L * C + 16383) // 16384))


def test_focal_shapes_reach_the_chunking_paths():
    per = {s: -(-s[0] * s[1] // _nchunk(*s)) for s in E.FOCAL_SHAPES}
    assert [_nchunk(*s) for s in E.FOCAL_SHAPES] == [1, 1, 2, 2, 64, 2]
    assert per[(205, 80)] % 80 != 0                                      # the chunk boundary splits a row
    assert 13200 * 80 > 64 * 16384 and per[(13200, 80)] > 16384          # the cap on the chunk count is reached
    assert per[(341, 81)] % 81 != 0


@pytest.mark.parametrize("L,C", E.FOCAL_SHAPES)
def test_focal_case_hits_both_sides_of_the_clip(L, C):
    logits, labels = E.focal_case(L, C)
    onehot = E.focal_onehot(labels, C).bool()
    assert np.isfinite(logits.numpy()).all()
    assert (logits[~onehot] <= 16.0).all() and (logits[onehot] <= 40.0).all()
    assert ((logits - E.FOCAL_CLIP_LOGIT).abs() >= 0.15).all()          # one ulp of sigmoid cannot flip the side of the clip
    if L * C == 1:
        assert labels[:, 0].tolist() == [1, 0, -1] and logits[0, 0, 0] < E.FOCAL_CLIP_LOGIT
        return
    below, above = logits < E.FOCAL_CLIP_LOGIT, logits > E.FOCAL_CLIP_LOGIT
    counts = {"pos_below": int((onehot & below).sum()), "pos_above": int((onehot & above).sum()), "pos_saturated": int((onehot & (logits >= 16)).sum()),
              "bg_below": int((~onehot & below).sum()), "bg_at_15.94": int((~onehot & (logits > 15.9)).sum()),
              **{f"label_{v}": int((labels == v).sum()) for v in E.focal_special_labels(C)}}
    print(L, C, counts)
    assert all(v >= 1 for v in counts.values()), counts
    for v in E.FOCAL_POS_LOGITS:
        assert (onehot & (logits == v)).any(), v
    for v in E.FOCAL_BG_LOGITS:
        assert (~onehot & (logits == np.float32(v))).any(), v
    assert not onehot[(labels == -1) | (labels == C + 1) | (labels == 0)].any()
    assert len({b for b in range(E.B) if (onehot[b] & below[b]).any()}) >= 2     # clipped positives in more than one image


@pytest.mark.parametrize("alpha", [0.25, 0.5])
@pytest.mark.parametrize("L,C", E.FOCAL_SHAPES)
def test_focal_fp32_oracle_within_tolerance(L, C, alpha):
    logits, labels = E.focal_case(L, C)
    loss, grad = E.focal_ref(logits, labels, alpha)
    _finite(loss, grad)
    loss32, grad32 = E.focal_ref(logits, labels, alpha, torch.float32)
    print(L, C, alpha, "loss rel", (np.abs(loss32 - loss) / np.abs(loss)).max(), "grad err / tol",
          (np.abs(grad32 - grad) / (E.FOCAL_GRAD_TOL["atol"] + E.FOCAL_GRAD_TOL["rtol"] * np.abs(grad))).max())
    np.testing.assert_allclose(loss32, loss, rtol=E.FOCAL_LOSS_RTOL)
    np.testing.assert_allclose(grad32, grad, **E.FOCAL_GRAD_TOL)
    clipped = (E.focal_onehot(labels, C).bool() & (logits < E.FOCAL_CLIP_LOGIT)).numpy()
    assert (grad[clipped] == 0).all()                                    # exactly 0 below the clip for t = 1


# ---------------------------------------------------------------------------------------------------- target assignment
def target_terms(hw, stride, rng, gt, radius=1.5):
    """The oracle's intermediate quantities (gen_targets) of one level in float64 -> dict of [B, HW, M] arrays."""
    xy = torch.from_numpy(R.coords_fcos(hw[0], hw[1], stride)).double()
    x, y = xy[:, 0][None, :, None], xy[:, 1][None, :, None]
    g = gt.double()[:, None]
    off = torch.stack([x - g[..., 0], y - g[..., 1], g[..., 2] - x, g[..., 3] - y], -1)
    omin, omax = off.min(-1)[0], off.max(-1)[0]
    cx, cy = (g[..., 0] + g[..., 2]) / 2, (g[..., 1] + g[..., 3]) / 2
    cmax = torch.stack([x - cx, y - cy, cx - x, cy - y], -1).max(-1)[0]
    c = {"omin": omin > 0, "lo": omax > rng[0], "hi": omax <= rng[1], "cmax": cmax < stride * radius}
    pos = c["omin"] & c["lo"] & c["hi"] & c["cmax"]
    area = (off[..., 0] + off[..., 2]) * (off[..., 1] + off[..., 3])
    return dict(omin=omin, omax=omax, cmax=cmax, cond=c, pos=pos, area=area, real=(gt[:, None, :, 0] >= 0).expand_as(pos))


def target_edge_counts(hw, stride, rng, gt, labels):
    k = target_terms(hw, stride, rng, gt)
    inf = torch.full_like(k["area"], float("inf"))
    pos_area = torch.where(k["pos"], k["area"], inf)
    best = pos_area.min(-1, keepdim=True)[0]                             # smallest positive area at the location
    others = lambda name: torch.stack([v for n, v in k["cond"].items() if n != name]).all(0)
    # an excluded edge: the box is negative by this comparison alone, and admitting it would change the winner
    flips = k["area"] < best
    counts = {
        "omin==0": (k["omin"] == 0) & others("omin") & flips,
        "omax==lo": (k["omax"] == rng[0]) & others("lo") & flips,
        "cmax==ratio": (k["cmax"] == stride * 1.5) & others("cmax") & flips,
        # the included edge: the box is positive by this comparison alone and is the winner
        "omax==hi": (k["omax"] == rng[1]) & k["pos"] & (k["area"] == best) & ((pos_area == best).sum(-1, keepdim=True) == 1),
    }
    is_best = k["pos"] & (k["area"] == best)
    lab = labels[:, None, :].expand_as(is_best)
    first = torch.where(is_best, lab, torch.full_like(lab, 10 ** 6)).min(-1)[0]      # labels ascend with the index in these cases
    last = torch.where(is_best, lab, torch.full_like(lab, -10 ** 6)).max(-1)[0]
    counts["equal_area_tie"] = ((is_best.sum(-1) >= 2) & (first != last))[..., None]
    raw = torch.where(k["real"] & k["cond"]["omin"], k["area"], inf)      # boxes that contain the location
    counts["min_area_not_positive"] = (k["pos"].any(-1) & (raw.min(-1)[0] < best[..., 0]))[..., None]
    counts["larger_listed_first"] = (k["pos"].any(-1) & (pos_area.argmin(-1) > torch.where(k["pos"], 0, 1).argmin(-1)))[..., None]
    return {n: int(v.sum()) for n, v in counts.items()}


def test_targets_case_hits_every_boundary_on_every_level():
    gt, labels = E.targets_case()
    assert sum(h * w for h, w in E.TGT_HW) == 336
    pad = (gt == -1).all(-1)
    assert (labels[pad] == -1).all() and (labels[~pad] >= 1).all()
    assert (pad[0, 2], pad[0, 5], pad[1, 3]) == (True, True, True) and pad[2, 1:].all()     # -1 rows in the middle and at the tail
    assert ((gt * 2) == (gt * 2).round()).all()
    table = {}
    for lvl, (hw, s, rg) in enumerate(zip(E.TGT_HW, E.TGT_STRIDES, E.TGT_RANGES)):
        table[lvl] = target_edge_counts(hw, s, rg, gt, labels)
        print(lvl, table[lvl])
    for lvl in range(3):
        for name in ("omin==0", "cmax==ratio", "equal_area_tie"):
            assert table[lvl][name] >= 1, (lvl, name)
    # omax == lo needs omax > 0 > -1 on level 0; omax == 9999999 with the centre within 48 px does not exist on level 2
    assert table[1]["omax==lo"] >= 1 and table[2]["omax==lo"] >= 1
    assert table[0]["omax==hi"] >= 1 and table[1]["omax==hi"] >= 1
    assert sum(t["min_area_not_positive"] for t in table.values()) >= 1
    assert sum(t["larger_listed_first"] for t in table.values()) >= 1


def test_targets_odd_stride_case_hits_its_edges():
    gt, labels = E.targets_case_odd_stride()
    xy = R.coords_fcos(9, 9, 7)
    assert xy[0].tolist() == [3.0, 3.0] and xy[10].tolist() == [10.0, 10.0]          # stride // 2, not stride / 2
    c = target_edge_counts(E.ODD_HW[0], E.ODD_STRIDE[0], E.ODD_RANGE[0], gt, labels)
    print(c)
    assert c["omin==0"] >= 1 and c["cmax==ratio"] >= 1 and c["equal_area_tie"] >= 1
    assert ((gt * 2) % 2 == 1).any()                                                 # half-integer boxes


@pytest.mark.parametrize("case", ["targets_case", "targets_case_empty", "targets_case_m1", "targets_case_odd_stride"])
def test_targets_fp32_oracle_equals_float64(case):
    gt, labels = getattr(E, case)()
    geom = (E.ODD_HW, E.ODD_STRIDE, E.ODD_RANGE) if case == "targets_case_odd_stride" else (E.TGT_HW, E.TGT_STRIDES, E.TGT_RANGES)
    exp = R.gen_targets(*geom, gt.double(), labels)
    got = R.gen_targets(*geom, gt, labels)
    _finite(exp[1].numpy(), exp[2].numpy())
    np.testing.assert_array_equal(got[0].numpy(), exp[0].numpy())
    np.testing.assert_array_equal(got[2].numpy(), exp[2].numpy())
    np.testing.assert_allclose(got[1].numpy(), exp[1].numpy(), rtol=1e-6)
    assert (exp[0] > 0).any()
    if case == "targets_case_empty":
        assert (exp[0][1] == 0).all() and (exp[1][1] == -1).all() and (exp[2][1] == -1).all()
    if case == "targets_case":
        # the designed locations: level 0 (36,36) takes box 0 at omax == hi; level 1 (40,72) stays negative at omax == lo
        cls = exp[0][..., 0]
        assert cls[0, 4 * 16 + 4] == 1 and cls[0, 256 + 4 * 8 + 2] == 0
        assert cls[1, 256 + 64 + 1 * 4 + 1] == 8                                     # identical boxes 8 / 9: the first wins
        assert cls[1, 6 * 16 + 6] == 11                                              # smaller box listed after the larger one wins, and before its twin
        assert cls[1, 256 + 1 * 8 + 5] == 14                                         # the area minimum (13) is not positive
