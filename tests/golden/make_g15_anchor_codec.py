"""tests/golden/make_g15_anchor_codec.py — the anchor codec fixture g15_anchor_codec.npz from the REAL reference.

Run ONLY in the build container (needs the reference tree, read-only; FD_REFERENCE overrides its path):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g15_anchor_codec.py

Imports the reference's utill/utills.py with make_golden.py's stub finder and records what its DataEncoder returns on
torch-CPU.  Stores data only; the zip entries carry a fixed timestamp, so a second run reproduces the file byte for byte.

  anchors_<w>x<h>            DataEncoder._get_anchor_boxes at (64, 64), (96, 64), (100, 72);  anchor_wh [5, 9, 2]
  enc_<case>_{boxes, labels, size, loc, cls}
                             DataEncoder.encode; cases m1, m5, m70 (more boxes than a wavefront has lanes), tie (two identical
                             boxes, labels 4 and 9: the first wins) and exact (integer boxes for which the largest IoU of some
                             anchor is 0.5 exactly in fp32, found by the search below: such an anchor is a positive)
  dec_<case>_{boxes, labels, n_cand}
                             DataEncoder.decode at (64, 64); cases c20, c80 (275 candidates), c3, zero (no candidate) and
                             saturated (one row with logits >= 20 in several classes).  The INPUTS are not stored: tests/anchor_ref.py
                             regenerates them (decode_case) from tests/golden/lcg.py.

The decode cases must not hinge on how a platform rounds exp: asserted here, on the reference's own tensors, are
  - no |max logit| < 1e-3 and the two largest logits of a row >= 1e-3 apart (outside the saturated row),
  - candidate scores pairwise >= 1e-5 apart,
  - no pairwise '+1' IoU between candidates within 1e-4 of 0.5 (a superset of the IoUs the NMS evaluates),
  - at most 1000 candidates.
The reference's two defects are confirmed, not recorded: decode with one candidate (case "single") and encode with M = 0 raise.
"""
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402  (installs the stub finder and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import anchor_ref  # noqa: E402  (tests/anchor_ref.py: the deterministic decode inputs only)

ref_ut = make_golden.ref_ut
ENC = ref_ut.DataEncoder()


def rnd_boxes(rng, n, w, h):
    xy = rng.uniform(0, 0.6, (n, 2)) * [w, h]
    wh = rng.uniform(0.15, 0.6, (n, 2)) * [w, h]
    return np.round(np.concatenate([xy, np.minimum(xy + wh, [w - 1, h - 1])], 1), 2).astype(np.float32)


def find_exact_half():
    """Integer boxes whose IoU with some anchor of the (64, 64) set is 0.5 exactly in fp32 and is that anchor's largest: searched over
    boxes against the reference's own _box_iou.  Returns (boxes [2, 4], anchor rows)."""
    anchors = ENC._get_anchor_boxes(torch.Tensor([64, 64]))
    best = None
    for x1 in range(0, 40, 1):
        cand = np.array([[x1, y1, x2, y2] for y1 in range(0, 40, 2) for x2 in range(x1 + 8, 64, 1) for y2 in range(y1 + 8, 64, 2)], np.float32)
        xywh = ENC._change_box_order(torch.from_numpy(cand), 'xyxy2xywh')
        iou = ENC._box_iou(anchors, xywh, order='xywh')                      # [A, n]
        hit = (iou == 0.5).nonzero()
        if hit.numel():
            j = int(hit[0, 1])
            best = cand[j]
            break
    if best is None:
        return None
    far = np.array([best, [50, 50, 62, 62]], np.float32)                       # a second box, so the maximum is over M = 2
    return far


def encode_cases():
    rng = np.random.default_rng(15)
    cases = {"m1": (np.array([[20.25, 10.5, 70, 60.75]], np.float32), np.array([7]), (100, 72)),
             "m5": (rnd_boxes(rng, 5, 96, 64), np.array([3, 0, 19, 7, 7]), (96, 64)),
             "m70": (rnd_boxes(rng, 70, 64, 64), rng.integers(0, 80, 70), 64),
             "tie": (np.array([[10, 12, 40, 44], [10, 12, 40, 44], [30, 5, 60, 30]], np.float32), np.array([4, 9, 2]), 64)}
    exact = find_exact_half()
    assert exact is not None, "no integer box with an IoU of exactly 0.5 found: widen the search"
    cases["exact"] = (exact, np.array([11, 5]), 64)
    out = {}
    for name, (boxes, labels, size) in cases.items():
        loc, cls = ENC.encode(torch.from_numpy(boxes), torch.from_numpy(np.asarray(labels, np.int64)), size)
        assert loc.dtype == torch.float32 and cls.dtype == torch.int64
        out[f"enc_{name}_boxes"], out[f"enc_{name}_labels"] = boxes, np.asarray(labels, np.int64)
        out[f"enc_{name}_size"] = np.array([size, size] if isinstance(size, int) else size, np.int64)
        out[f"enc_{name}_loc"], out[f"enc_{name}_cls"] = loc.numpy(), cls.numpy()
        assert (cls.numpy() > 0).any() and (cls.numpy() == 0).any(), name
    assert (out["enc_m70_cls"] == -1).any()
    t = out["enc_tie_cls"]
    assert (t == 5).any() and not (t == 10).any()                              # the first of two identical boxes wins
    # the exact case: some anchor's largest IoU is 0.5f and it is a positive
    anchors = ENC._get_anchor_boxes(torch.Tensor([64, 64]))
    iou = ENC._box_iou(anchors, ENC._change_box_order(torch.from_numpy(exact), 'xyxy2xywh'), order='xywh').max(1)[0]
    rows = (iou == 0.5).nonzero().flatten()
    assert rows.numel() >= 1 and (out["enc_exact_cls"][rows.numpy()] > 0).all()
    out["enc_exact_rows"] = rows.numpy()
    try:
        ENC.encode(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), 64)
        raise AssertionError("the reference encodes M = 0 after all")
    except (IndexError, RuntimeError):
        pass
    return out


def decode_cases():
    out = {}
    for name, (C, n, _) in anchor_ref.DECODE_CASES.items():
        loc, cls = (torch.from_numpy(a) for a in anchor_ref.decode_case(name))
        if name == "single":
            try:
                ENC.decode(loc, cls, 64)
                raise AssertionError("the reference decodes one candidate after all")
            except IndexError:
                continue
        sat = np.zeros(cls.shape[0], bool)
        if name == "saturated":
            sat[anchor_ref.SATURATED_ROW] = True
        top2 = cls.topk(2, 1)[0].numpy()[~sat]
        assert (np.abs(top2[:, 0]) >= 1e-3).all() and (top2[:, 0] - top2[:, 1] >= 1e-3).all(), name
        score, _ = cls.sigmoid().max(1)
        ids = (score > 0.5).nonzero().flatten()
        assert ids.numel() <= 1000
        if name == "zero":
            assert ids.numel() == 0
            try:                                                               # (the reference's own NMS cannot take an empty set either)
                boxes, labels = ENC.decode(loc, cls, 64)
                boxes, labels = boxes.numpy().reshape(-1, 4), labels.numpy().reshape(-1)
            except (IndexError, RuntimeError):
                boxes, labels = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
            assert boxes.shape[0] == 0
        else:
            s = np.sort(score[ids].numpy().astype(np.float64))
            assert (np.diff(s) >= 1e-5).all(), name
            anchors = ENC._get_anchor_boxes(torch.Tensor([64, 64]))
            xy = loc[:, :2] * anchors[:, 2:] + anchors[:, :2]
            wh = loc[:, 2:].exp() * anchors[:, 2:]
            cand = torch.cat([xy - wh / 2, xy + wh / 2], 1)[ids]
            iou = ENC._box_iou(cand, cand).numpy()
            assert (np.abs(iou - 0.5) > 1e-4).all(), name
            boxes, labels = ENC.decode(loc, cls, 64)
            boxes, labels = boxes.numpy(), labels.numpy()
            assert 0 < boxes.shape[0] < ids.numel(), (name, boxes.shape, ids.numel())     # the NMS removed something
        if name == "saturated":
            assert float(score[anchor_ref.SATURATED_ROW]) == 1.0 and labels[0] == min(c for c, _ in anchor_ref.SATURATED_LOGITS)
        if name == "c80":
            assert ids.numel() == 275
        out[f"dec_{name}_boxes"], out[f"dec_{name}_labels"] = boxes.astype(np.float32), labels.astype(np.int64)
        out[f"dec_{name}_n_cand"] = np.array(ids.numel(), np.int64)
    return out


def main():
    arrays = {"anchor_wh": ENC.anchor_wh.numpy()}
    for w, h in [(64, 64), (96, 64), (100, 72)]:
        a = ENC._get_anchor_boxes(torch.Tensor([w, h]))
        assert a.dtype == torch.float32
        arrays[f"anchors_{w}x{h}"] = a.numpy()
    assert [arrays[k].shape[0] for k in ("anchors_64x64", "anchors_96x64", "anchors_100x72")] == [774, 1161, 1521]
    arrays.update(encode_cases())
    arrays.update(decode_cases())
    arrays["source"] = np.array("reference utill/utills.py DataEncoder on torch-CPU " + torch.__version__)
    path = os.path.join(HERE, "g15_anchor_codec.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size <= 200 * 1024, size
    print(f"g15_anchor_codec.npz  {size / 1024:.1f} KB  " + ", ".join(f"{k[4:-7]}={int(v)}" for k, v in arrays.items() if k.endswith("_n_cand")))


if __name__ == "__main__":
    main()
