"""SimOTA target assignment restated in numpy, brute force -- the checker of fd_simota_gen_targets.

Definition (this project's own).  Levels, strides and the location order (levels concatenated, row-major inside a level) are
those of fd_fcos_gen_targets; p is a location's index in that order, 0 <= p < L, and c = ((float)(px*s) + (float)(s//2), same
for y) its centre.  Inputs per image: cls_logits [L, C], cnt_logits [L], reg_pred [L, 4] = (l, t, r, b) in pixels, gt [M, 4]
xyxy, labels [M].  A row is VALID when 1 <= label <= C, its four coordinates are finite and x2 > x1, y2 > y1; its class is
column label - 1.  Every fp32 operation below is one np.float32 operation (rounded once, no fused multiply-add).

1. per location   s_c = 1 / (1 + exp(-cls_c)), z = 1 / (1 + exp(-cnt)), q_c = sqrt(s_c * z); nl(x) = -log(x) where that is
                  < 100, else 100 (log(0) and NaN give 100); N = sum_c nl(1 - q_c), sequentially, c ascending
2. per pair       candidate: min(cx-x1, cy-y1, x2-cx, y2-cy) > inside_eps
                  preferred: a candidate with max(|cx-gx|, |cy-gy|) < centre_radius * (float)s, g = ((x1+x2)/2, (y1+y2)/2)
                  iou: box (cx-l, cy-t, cx+r, cy+b) against the row, operation order of fd_pairwise_iou(plus_one = 0):
                  inter / ((area_pred + area_row) - inter); !(iou > 0) -> 0, iou > 1 -> 1
                  cost = ((N - nl(1 - q_g)) + nl(q_g)) + iou_weight * (0 - log(iou + 1e-8)); !(cost < FLT_MAX) -> FLT_MAX
3. dynamic k      n = number of candidates; the min(top_q, n) largest iou summed in fp32 in descending order;
                  k = min(max(int(sum), 1), n)  (n == 0: k = 0)
4. selection      the k candidates with the smallest (not preferred, cost, p) are positive for the row
5. contest        a location positive for several rows goes to the smallest (not preferred, cost, row)
6. outputs        cls [B, L] int64 label (0 negative), reg [B, L, 4] = (cx-x1, cy-y1, x2-cx, y2-cy) (-1 negative),
                  cnt [B, L] = sqrt(min(l,r)*min(t,b) / (max(l,r)*max(t,b) + 1e-10)) (quality 0) or the winner's iou
                  (quality 1), -1 negative

pairs() is steps 1-2 (fp32 in the stated order, or with the cost in float64 on the same fp32 inputs and the same fp32 iou);
select() is steps 3-6 as a pure function of the pair matrices, so it can be fed the device's own."""
import numpy as np

from atss_ref import centres

F = np.float32
FLT_MAX = np.finfo(F).max


def row_valid(box, label, C):
    return bool(1 <= label <= C and np.all(np.isfinite(box)) and box[2] > box[0] and box[3] > box[1])


def valid_rows(gt, labels, C):
    return np.array([[row_valid(gt[b, m], labels[b, m], C) for m in range(labels.shape[1])] for b in range(labels.shape[0])],
                    dtype=bool).reshape(labels.shape)


def _nl(x, T):
    v = -np.log(x)
    return np.where(v < T(100), v, T(100)).astype(T)


def _sigmoid(v, T):
    return (T(1) / (T(1) + np.exp(-v))).astype(T)


def pair_geometry(gt_b, valid_b, cx, cy, st, centre_radius, inside_eps):
    """-> candidate [M, L], preferred [M, L] of one image, in fp32."""
    M, L = len(gt_b), len(cx)
    cand, pref = np.zeros((M, L), bool), np.zeros((M, L), bool)
    radius = F(centre_radius) * st.astype(F)
    for m in range(M):
        if not valid_b[m]:
            continue
        x1, y1, x2, y2 = gt_b[m]
        inside = np.minimum(np.minimum(cx - x1, cy - y1), np.minimum(x2 - cx, y2 - cy))
        cand[m] = inside > F(inside_eps)
        gx, gy = (x1 + x2) / F(2), (y1 + y2) / F(2)
        pref[m] = cand[m] & (np.maximum(np.abs(cx - gx), np.abs(cy - gy)) < radius)
    return cand, pref


def pred_iou(reg_b, box, cx, cy):
    """fp32 IoU of the predicted boxes [L] with one row; NaN / <= 0 -> 0, > 1 -> 1."""
    bx1, by1, bx2, by2 = cx - reg_b[:, 0], cy - reg_b[:, 1], cx + reg_b[:, 2], cy + reg_b[:, 3]
    ltx, lty = np.fmax(bx1, box[0]), np.fmax(by1, box[1])
    rbx, rby = np.fmin(bx2, box[2]), np.fmin(by2, box[3])
    w, h = np.fmax(rbx - ltx, F(0)), np.fmax(rby - lty, F(0))
    inter = w * h
    a1 = (bx2 - bx1) * (by2 - by1)
    a2 = (box[2] - box[0]) * (box[3] - box[1])
    iou = (inter / ((a1 + a2) - inter)).astype(F)
    iou = np.where(iou > F(0), iou, F(0))
    return np.where(iou > F(1), F(1), iou).astype(F)


def pairs(cls_logits, cnt_logits, reg_pred, gt, labels, level_hw, strides, centre_radius=2.5, iou_weight=3.0, inside_eps=0.01, cost64=False):
    """Steps 1-2 -> dict(iou [B, M, L] f32, cost [B, M, L] f32 (or f64 with cost64), cand, pref [B, M, L] bool, valid [B, M] bool).
    Non-candidates and padding rows hold iou 0, cost +inf.  With cost64 the sigmoids, the square roots, the logarithms and the sums
    of the cost run in float64 on the fp32 logits and the fp32 iou; nothing else changes."""
    cls_logits = np.asarray(cls_logits, F)
    B, L, C = cls_logits.shape
    cnt_logits = np.asarray(cnt_logits, F).reshape(B, L)
    reg_pred = np.asarray(reg_pred, F).reshape(B, L, 4)
    labels = np.asarray(labels, np.int64)
    M = labels.shape[1]
    gt = np.asarray(gt, F).reshape(B, M, 4)
    cx, cy, lv, _ = centres(level_hw, strides)
    assert len(cx) == L
    st = np.asarray(strides)[lv]
    T = np.float64 if cost64 else F
    valid = valid_rows(gt, labels, C)
    iou = np.zeros((B, M, L), F)
    cost = np.full((B, M, L), np.inf, T)
    cand, pref = np.zeros((B, M, L), bool), np.zeros((B, M, L), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            z = _sigmoid(cnt_logits[b].astype(T), T)
            q = np.sqrt(_sigmoid(cls_logits[b].astype(T), T) * z[:, None]).astype(T)           # [L, C]
            terms = _nl(T(1) - q, T)
            N = np.zeros(L, T)
            for c in range(C):
                N = (N + terms[:, c]).astype(T)
            cand[b], pref[b] = pair_geometry(gt[b], valid[b], cx, cy, st, centre_radius, inside_eps)
            for m in range(M):
                if not valid[b, m]:
                    continue
                g = int(labels[b, m]) - 1
                v = pred_iou(reg_pred[b], gt[b, m], cx, cy)
                ilog = np.log(v + F(1e-8)).astype(F) if not cost64 else np.log(v.astype(T) + T(1e-8))
                c_ = ((N - terms[:, g]) + _nl(q[:, g], T)) + T(iou_weight) * (T(0) - ilog)
                c_ = np.where(c_ < T(FLT_MAX), c_, T(FLT_MAX)).astype(T)
                iou[b, m] = np.where(cand[b, m], v, F(0))
                cost[b, m] = np.where(cand[b, m], c_, T(np.inf))
    return dict(iou=iou, cost=cost, cand=cand, pref=pref, valid=valid)


def dynamic_k(iou_row, cand_row, top_q):
    """Step 3 for one row -> (k, n, the fp32 sum)."""
    v = np.sort(iou_row[cand_row].astype(F))[::-1][:top_q]
    total = F(0)
    for x in v:
        total = F(total + x)
    n = int(cand_row.sum())
    return (min(max(int(total), 1), n) if n else 0), n, total


def select(iou, cost, cand, pref, gt, labels, level_hw, strides, top_q=10, quality=0):
    """Steps 3-6 on given pair matrices [B, M, L] -> dict(cls [B, L], cnt [B, L], reg [B, L, 4], k [B, M], ncand [B, M],
    owner [B, L] (-1 negative), claims [B, L] rows positive at the location, positive [B, M, L] bool before the contest).
    Rows without a candidate take no part, so padding rows need no flag of their own.  Keys compare as Python tuples: exact."""
    B, M, L = iou.shape
    labels = np.asarray(labels, np.int64)
    gt = np.asarray(gt, F).reshape(B, M, 4)
    cx, cy, _, _ = centres(level_hw, strides)
    cls = np.zeros((B, L), np.int64)
    cnt = np.full((B, L), -1, F)
    reg = np.full((B, L, 4), -1, F)
    k = np.zeros((B, M), np.int32)
    ncand = np.zeros((B, M), np.int32)
    owner = np.full((B, L), -1, np.int64)
    claims = np.zeros((B, L), np.int32)
    positive = np.zeros((B, M, L), bool)
    for b in range(B):
        best = {}
        for m in range(M):
            k[b, m], ncand[b, m], _ = dynamic_k(iou[b, m], cand[b, m], top_q)
            locs = np.nonzero(cand[b, m])[0]
            order = sorted(locs, key=lambda p: (not pref[b, m, p], float(cost[b, m, p]), int(p)))
            for p in order[:k[b, m]]:
                positive[b, m, p] = True
                claims[b, p] += 1
                key = (not pref[b, m, p], float(cost[b, m, p]), m)
                if p not in best or key < best[p]:
                    best[p] = key
        for p, key in best.items():
            m = key[2]
            box = gt[b, m]
            off = np.array([cx[p] - box[0], cy[p] - box[1], box[2] - cx[p], box[3] - cy[p]], dtype=F)
            owner[b, p] = m
            cls[b, p] = labels[b, m]
            reg[b, p] = off
            if quality:
                cnt[b, p] = iou[b, m, p]
            else:
                lr_min, lr_max = min(off[0], off[2]), max(off[0], off[2])
                tb_min, tb_max = min(off[1], off[3]), max(off[1], off[3])
                with np.errstate(all="ignore"):
                    cnt[b, p] = np.sqrt((lr_min * tb_min) / (lr_max * tb_max + F(1e-10)))
    return dict(cls=cls, cnt=cnt, reg=reg, k=k, ncand=ncand, owner=owner, claims=claims, positive=positive)


def simota_gen_targets(cls_logits, cnt_logits, reg_pred, gt, labels, level_hw, strides, top_q=10, centre_radius=2.5, iou_weight=3.0,
                       inside_eps=0.01, quality=0, cost64=False):
    """The whole assigner: pairs() then select() -> select()'s dict plus the pair matrices under "pairs"."""
    pr = pairs(cls_logits, cnt_logits, reg_pred, gt, labels, level_hw, strides, centre_radius, iou_weight, inside_eps, cost64)
    out = select(pr["iou"], pr["cost"], pr["cand"], pr["pref"], gt, labels, level_hw, strides, top_q, quality)
    out["pairs"] = pr
    return out


def decision_margins(iou, cost, cand, pref, top_q):
    """How far every decision of steps 3-5 is from going the other way, for pair matrices with the cost in float64:
    sum       the smallest distance of a row's top-q IoU sum (fp32 values summed in float64) from an integer
    select    the smallest (c' - c) / (1 + max(|c|, |c'|)) between a row's k-th and (k+1)-th key where both have one preference
    contest   the same between the two best claims of a location positive for several rows
    (inf where no such decision exists)."""
    B, M, L = iou.shape
    out = dict(sum=np.inf, select=np.inf, contest=np.inf)

    def gap(a, b):
        return abs(b - a) / (1.0 + max(abs(a), abs(b)))
    for b in range(B):
        claims = {}
        for m in range(M):
            k, n, _ = dynamic_k(iou[b, m], cand[b, m], top_q)
            if n == 0:
                continue
            total = float(np.sum(np.sort(iou[b, m][cand[b, m]].astype(np.float64))[::-1][:top_q]))
            out["sum"] = min(out["sum"], abs(total - round(total)))
            order = sorted(np.nonzero(cand[b, m])[0], key=lambda p: (not pref[b, m, p], float(cost[b, m, p]), int(p)))
            if k < n and pref[b, m, order[k - 1]] == pref[b, m, order[k]]:
                out["select"] = min(out["select"], gap(float(cost[b, m, order[k - 1]]), float(cost[b, m, order[k]])))
            for p in order[:k]:
                claims.setdefault(int(p), []).append((not pref[b, m, p], float(cost[b, m, p]), m))
        for c in claims.values():
            if len(c) > 1:
                c.sort()
                if c[0][0] == c[1][0]:
                    out["contest"] = min(out["contest"], gap(c[0][1], c[1][1]))
    return out
