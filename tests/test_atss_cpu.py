"""ATSS target assignment without a GPU: hand-derived known answers of the numpy restatement (tests/atss_ref.py), an
independent torch transcription on tie-free inputs, the preconditions of the random cases the GPU file runs, and the C ABI
of fd_atss_workspace_bytes / fd_atss_gen_targets (symbols, workspace size, every refusal before anything is enqueued)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import atss_cases as K
import atss_ref as A
from pytorch_object_detection_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def run(case):
    return A.atss_gen_targets(case["gt"], case["labels"], case["level_hw"], case["strides"], case["topk"], case["anchor_scale"],
                              case["inside_eps"])


# ---------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("topk", [9, 16])
def test_grid_point_ties_go_to_the_lower_index(topk):
    c = K.grid5(topk)
    cx, cy, _, _ = A.centres(c["level_hw"], c["strides"])
    d2 = (cx - F(20)) ** 2 + (cy - F(20)) ** 2
    assert sorted(d2.tolist()) == [0.0] + [64.0] * 4 + [128.0] * 4 + [256.0] * 4 + [320.0] * 8 + [512.0] * 4    # 4-way and 8-way ties
    assert A.candidates(c["gt"][0, 0], c["level_hw"], c["strides"], topk).tolist() == K.GRID5_PICKS16[:topk]
    r = run(c)
    assert r["cand"][(0, 0)].tolist() == K.GRID5_PICKS16[:topk]
    # side 64 anchors around a 28 x 28 box: the IoU falls with the distance, the centre always passes
    assert r["npos"][0, 0] >= 1 and r["cls"][0, 12] == 4


def test_equal_ious_are_all_positive_by_greater_equal():
    c = K.equal_ious()
    r = run(c)
    cx, cy, lv, _ = A.centres(c["level_hw"], c["strides"])
    iou = A.anchor_iou(cx, cy, np.full(9, 8), 8.0, c["gt"][0, 0])
    v = F(4096.0) / F(90000.0)
    assert (iou == v).all()
    assert r["thr"][0, 0] == float(v)                        # mean == v exactly, std == 0
    assert r["npos"][0, 0] == 9 and (r["cls"][0] == 2).all()
    assert not any(float(x) > r["thr"][0, 0] for x in iou)   # a `>` implementation has no positive here
    np.testing.assert_array_equal(r["reg"][0, 4], [112., 112., 188., 188.])


def test_single_location_level():
    c = K.single_location()
    r = run(c)
    iou = A.anchor_iou(np.array([64], F), np.array([64], F), np.array([128]), 8.0, c["gt"][0, 0])
    assert r["thr"][0, 0] == float(iou[0]) and r["npos"][0, 0] == 1 and r["cls"].tolist() == [[7]]
    np.testing.assert_array_equal(r["reg"][0, 0], [54., 54., 36., 56.])
    assert r["cnt"][0, 0] == np.sqrt(F(36 * 54) / (F(54 * 56) + F(1e-10)))


def test_levels_shorter_than_topk():
    c = K.short_levels()
    r = run(c)
    cand = r["cand"][(0, 0)]
    assert len(cand) == 8 and sorted(cand[:6].tolist()) == list(range(6)) and sorted(cand[6:].tolist()) == [6, 7]
    # box centre (11.5, 8.5): level 0 centres (4 | 12 | 20, 4 | 12) -> nearest first (12, 12) = pix 4, then (12, 4) = pix 1
    assert cand[:2].tolist() == [4, 1]
    assert r["npos"][0, 0] >= 1


def test_inside_eps_boundary():
    c = K.inside_boundary()
    e = F(K.EPS)
    assert F(0) - c["gt"][0, 0, 0] == e and F(0) - c["gt"][1, 0, 0] == np.nextafter(e, F(1))
    r = run(c)
    assert r["npos"].tolist() == [[0], [1]]
    assert r["cls"].tolist() == [[0], [3]] and r["cnt"][0, 0] == -1 and (r["reg"][0] == -1).all()
    assert r["reg"][1, 0, 0] == np.nextafter(e, F(1))
    assert np.isfinite(r["thr"]).all()                    # both rows are valid; only step 4 differs


def test_identical_rows_go_to_the_lower_row():
    c = K.twin_rows()
    r = run(c)
    assert r["npos"][0, 0] == r["npos"][0, 1] >= 1 and r["thr"][0, 0] == r["thr"][0, 1]
    pos = r["claims"][0] > 0
    assert (r["claims"][0][pos] == 2).all() and (r["cls"][0][pos] == 5).all() and (r["owner"][0][pos] == 0).all()


def test_padding_degenerate_and_non_finite_rows_are_skipped():
    c = K.skipped_rows()
    r, only = run(c), run(K.skipped_rows_valid_only())
    assert np.isnan(r["thr"][0, [0, 1, 2, 4, 5, 6, 7]]).all() and (r["npos"][0, [0, 1, 2, 4, 5, 6, 7]] == 0).all()
    assert r["npos"][0, 3] == only["npos"][0, 0] >= 1 and r["thr"][0, 3] == only["thr"][0, 0]
    for k in ("cls", "cnt", "reg"):
        np.testing.assert_array_equal(r[k], only[k])
    assert set(np.unique(r["cls"])) == {0, 6}


def test_no_rows_is_all_negative():
    r = run(K.no_rows())
    L = sum(h * w for h, w in K.pyramid(64, 96))
    assert r["cls"].shape == (2, L) and not r["cls"].any() and (r["cnt"] == -1).all() and (r["reg"] == -1).all()
    assert r["thr"].shape == (2, 0) and r["npos"].shape == (2, 0)


# ---------------------------------------------------------------------------------------------------- torch transcription
def torch_atss(gt, labels, level_hw, strides, topk, anchor_scale, inside_eps):
    """A second transcription with torch.topk / torch.std over [M, L] tensors, one image at a time.  torch.topk leaves the order
    of equal distances open and torch.std sums in its own order: it is compared on tie-free inputs, thr within fp64 rounding."""
    gt, labels = torch.as_tensor(gt), torch.as_tensor(labels)
    B, M = labels.shape
    cs, ss = [], []
    for (h, w), s in zip(level_hw, strides):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        cs.append(torch.stack([xs.reshape(-1) * s + s // 2, ys.reshape(-1) * s + s // 2], 1).float())
        ss.append(torch.full((h * w,), float(s)))
    c, s = torch.cat(cs), torch.cat(ss)
    L = c.shape[0]
    r = anchor_scale * s / 2
    anchors = torch.cat([c - r[:, None], c + r[:, None]], 1)
    cls, cnt, reg = torch.zeros(B, L, dtype=torch.int64), -torch.ones(B, L), -torch.ones(B, L, 4)
    thr_out, npos_out = torch.full((B, M), float("nan"), dtype=torch.float64), torch.zeros(B, M, dtype=torch.int32)
    for b in range(B):
        ok = (labels[b] >= 0) & torch.isfinite(gt[b]).all(1) & (gt[b, :, 2] > gt[b, :, 0]) & (gt[b, :, 3] > gt[b, :, 1])
        rows = torch.nonzero(ok)[:, 0]
        if not len(rows):
            continue
        g = gt[b, rows]
        lt, rb = torch.max(anchors[None, :, :2], g[:, None, :2]), torch.min(anchors[None, :, 2:], g[:, None, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        a1 = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
        a2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        iou = inter / (a1[None] + a2[:, None] - inter)                                    # [R, L]
        gc = (g[:, :2] + g[:, 2:]) / 2
        d2 = ((c[None] - gc[:, None]) ** 2).sum(-1)
        idx, start = [], 0
        for h, w in level_hw:
            k = min(topk, h * w)
            idx.append(torch.topk(d2[:, start:start + h * w], k, dim=1, largest=False)[1] + start)
            start += h * w
        idx = torch.cat(idx, 1)
        ciou = torch.gather(iou, 1, idx).double()
        thr = ciou.mean(1) + (ciou.std(1) if idx.shape[1] > 1 else 0.0)
        off = torch.cat([c[None] - g[:, None, :2], g[:, None, 2:] - c[None]], -1)        # [R, L, 4]
        is_cand = torch.zeros_like(iou, dtype=torch.bool).scatter_(1, idx, True)
        pos = is_cand & (iou.double() >= thr[:, None]) & (off.min(-1)[0] > inside_eps)
        thr_out[b, rows], npos_out[b, rows] = thr, pos.sum(1).int()
        score = torch.where(pos, iou, torch.full_like(iou, -1.0))
        best, who = score.max(0)
        for loc in torch.nonzero(best >= 0)[:, 0]:
            m = int(torch.nonzero(score[:, loc] == best[loc])[0, 0])                      # first maximum: lowest row
            o = off[m, loc]
            cls[b, loc], reg[b, loc] = labels[b, rows[m]], o
            cnt[b, loc] = torch.sqrt(torch.min(o[0], o[2]) * torch.min(o[1], o[3]) / (torch.max(o[0], o[2]) * torch.max(o[1], o[3]) + 1e-10))
    return cls.numpy(), cnt.numpy(), reg.numpy(), thr_out.numpy(), npos_out.numpy()


def _tie_free(case):
    """No two locations of a level are equally far from a valid row's centre."""
    cx, cy, lv, _ = A.centres(case["level_hw"], case["strides"])
    for b in range(case["labels"].shape[0]):
        for m in range(case["labels"].shape[1]):
            box = case["gt"][b, m]
            if A.row_valid(box, case["labels"][b, m]):
                gx, gy = (box[0] + box[2]) / F(2), (box[1] + box[3]) / F(2)
                d2 = (cx - gx) * (cx - gx) + (cy - gy) * (cy - gy)
                for l in range(len(case["level_hw"])):
                    if len(np.unique(d2[lv == l])) != (lv == l).sum():
                        return False
    return True


@pytest.mark.parametrize("name", ["rand64x96_k9_a8", "rand64x96_k1_a4", "rand256x320_k16_a4", "rand256x320_k9_a8", "short_levels", "single_location"])
def test_restatement_equals_a_torch_transcription_on_tie_free_inputs(name):
    c = K.get(name)
    assert _tie_free(c), "the transcription leaves tie order open: this case must not tie"
    r = run(c)
    cls, cnt, reg, thr, npos = torch_atss(c["gt"], c["labels"], c["level_hw"], c["strides"], c["topk"], c["anchor_scale"], c["inside_eps"])
    np.testing.assert_array_equal(cls, r["cls"])
    np.testing.assert_array_equal(reg, r["reg"])
    np.testing.assert_array_equal(npos, r["npos"])
    np.testing.assert_allclose(cnt, r["cnt"], rtol=1e-6)
    np.testing.assert_allclose(thr, r["thr"], rtol=1e-12, equal_nan=True)     # torch sums pairwise and fuses: a few fp64 roundings


# ---------------------------------------------------------------------------------------------------- preconditions of the GPU cases
@pytest.mark.parametrize("name", list(K.RANDOM))
def test_random_cases_have_positives_and_contested_locations(name):
    c = K.get(name)
    r = run(c)
    B, M = c["labels"].shape
    assert (B, M) == (3, 7) and c["labels"].max() <= 20 and len(c["level_hw"]) == 5
    if name.startswith("rand64x96"):
        assert c["level_hw"] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    valid = np.array([[A.row_valid(c["gt"][b, m], c["labels"][b, m]) for m in range(M)] for b in range(B)])
    assert (c["labels"] < 0).any() and ((c["labels"] >= 0) & ~valid).any()                 # padding and a degenerate row
    h, w = (64, 96) if name.startswith("rand64x96") else (256, 320)
    gcx, gcy = (c["gt"][..., 0] + c["gt"][..., 2]) / 2, (c["gt"][..., 1] + c["gt"][..., 3]) / 2
    assert (valid & ((gcx == 0) | (gcy == h))).any() and (valid & ((gcx > w) | (gcy < 0))).any()   # centres on the border and outside
    pos = (r["cls"] > 0).sum(1)
    contested = (r["claims"] >= 2).sum(1)
    print(name, "positives per image", pos.tolist(), "contested locations per image", contested.tolist(), "npos", r["npos"].tolist())
    assert (pos[valid.any(1)] >= 1).all()
    assert contested.sum() >= 1
    assert np.isnan(r["thr"][~valid]).all() and np.isfinite(r["thr"][valid]).all()


# ---------------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fcosdet.h")).read()
    lib = _lib.lib()
    for name in ("fd_atss_workspace_bytes", "fd_atss_gen_targets"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name)
    assert re.search(r"#define\s+FD_ATSS_MAX_TOPK\s+16\b", hdr)
    from pytorch_object_detection_amd import ops
    assert ops.ATSS_MAX_TOPK == 16


def test_workspace_bytes():
    lib = _lib.lib()
    assert lib.fd_atss_workspace_bytes(16, 8525) == 16 * 8525 * 8 and lib.fd_atss_workspace_bytes(1, 1) == 8
    assert lib.fd_atss_workspace_bytes(65535, 2 ** 31 - 1) == 65535 * (2 ** 31 - 1) * 8          # 64-bit arithmetic
    assert lib.fd_atss_workspace_bytes(0, 10) == -1 and lib.fd_atss_workspace_bytes(2, 0) == -1 and lib.fd_atss_workspace_bytes(-1, -1) == -1


def test_every_refusal_comes_before_anything_is_enqueued():
    """Fake pointers throughout: a call that got past the checks would fault, so ONLY refused calls may be listed here."""
    lib = _lib.lib()
    P = ctypes.c_void_p
    segs = _lib.Segs.make(2, [(4, 4), (2, 2)])
    st = (ctypes.c_int32 * 2)(8, 16)
    ok = dict(gt=P(4096), labels=P(8192), M=3, segs=ctypes.byref(segs), strides=st, topk=9, scale=8.0, eps=0.01, cls=P(12288), cnt=P(16384),
              reg=P(20480), thr=None, npos=None, ws=P(24576))

    def call(**kw):
        a = {**ok, **kw}
        rc = lib.fd_atss_gen_targets(a["gt"], a["labels"], a["M"], a["segs"], a["strides"], a["topk"], a["scale"], a["eps"], a["cls"], a["cnt"],
                                     a["reg"], a["thr"], a["npos"], a["ws"], None)
        return rc, lib.fd_last_error()

    for k in ("gt", "labels", "strides", "cls", "cnt", "reg", "ws"):
        rc, msg = call(**{k: None})
        assert rc == _lib.E_INVAL and b"null pointer" in msg, (k, rc, msg)
    rc, msg = call(M=0, gt=None, labels=None, ws=None)              # M == 0 frees gt / labels only
    assert rc == _lib.E_INVAL and b"null pointer" in msg
    assert call(M=-1)[0] == _lib.E_INVAL
    bad = _lib.Segs.make(2, [(4, 4), (2, 2)])
    bad.m_start[2] += 1
    for s in (None, ctypes.byref(bad), ctypes.byref(_lib.Segs.make(70000, [(1, 1)]))):
        rc, msg = call(segs=s, strides=st)
        assert rc == _lib.E_INVAL and b"bad level table" in msg, (rc, msg)
    for stride in ((0, 16), (8, -16), (2 ** 30, 16)):
        rc, msg = call(strides=(ctypes.c_int32 * 2)(*stride))
        assert rc == _lib.E_INVAL and b"bad level table" in msg, (stride, rc, msg)
    for topk, code in ((0, _lib.E_INVAL), (-3, _lib.E_INVAL), (17, _lib.E_UNSUPPORTED), (1000, _lib.E_UNSUPPORTED)):
        rc, msg = call(topk=topk)
        assert rc == code and b"topk" in msg, (topk, rc, msg)
    for scale in (0.0, -8.0, math.inf, math.nan):
        rc, msg = call(scale=scale)
        assert rc == _lib.E_INVAL and b"anchor_scale" in msg, (scale, rc, msg)
    for eps in (-0.01, math.inf, -math.inf, math.nan):
        rc, msg = call(eps=eps)
        assert rc == _lib.E_INVAL and b"inside_eps" in msg, (eps, rc, msg)
    for k, v in (("gt", P(4096 + 8)), ("reg", P(20480 + 4)), ("ws", P(24576 + 4))):
        rc, msg = call(**{k: v})
        assert rc == _lib.E_INVAL and b"aligned" in msg, (k, rc, msg)
