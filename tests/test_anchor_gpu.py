"""The anchor codec on the device (fd_anchor.hip): DataEncoder's anchors / encode / decode against the REAL
reference's recorded outputs (g15_anchor_codec.npz), and against tests/anchor_ref.py where the reference raises or has no
counterpart (one candidate, an image without boxes, the max_candidates cap)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import anchor_ref  # noqa: E402
from pytorch_object_detection_amd._lib import FdError  # noqa: E402
from pytorch_object_detection_amd.utill.utills import DataEncoder  # noqa: E402

pytestmark = pytest.mark.gpu

G15 = np.load(os.path.join(HERE, "golden", "g15_anchor_codec.npz"))
ENC_CASES = ["m1", "m5", "m70", "tie", "exact"]
DEC_CASES = ["c20", "c80", "c3", "zero", "saturated"]
ULP_BOUND = 4         # log / exp at <= 1 ulp on each side = 2 ulp of distance; 4 as margin for the final rounding (derived, not tuned)
ENC = DataEncoder()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def box_tolerance(ref_boxes: np.ndarray) -> np.ndarray:
    """4 * 2^-23 * (|xy| + wh) per coordinate, xy / wh the centre and size of the reference box along that axis."""
    ref_boxes = ref_boxes.astype(np.float64)
    c = np.abs((ref_boxes[:, :2] + ref_boxes[:, 2:]) / 2)
    wh = ref_boxes[:, 2:] - ref_boxes[:, :2]
    t = 4 * 2.0 ** -23 * (c + wh)
    return np.concatenate([t, t], 1)


def check_loc_cls(loc, cls, ref_loc, ref_cls, what):
    loc, cls = loc.cpu().numpy(), cls.cpu().numpy()
    assert loc.dtype == np.float32 and cls.dtype == np.int64
    np.testing.assert_array_equal(cls, ref_cls, err_msg=what)
    assert loc[:, :2].tobytes() == ref_loc[:, :2].tobytes(), what
    d = anchor_ref.ulp_distance(loc[:, 2:], ref_loc[:, 2:])
    print(f"{what}: max ulp distance of loc_wh = {int(d.max())}")
    assert d.max() <= ULP_BOUND, what


def check_detections(boxes, labels, ref_boxes, ref_labels, what):
    boxes, labels = boxes.cpu().numpy(), labels.cpu().numpy()
    assert labels.dtype == np.int64 and boxes.dtype == np.float32
    assert boxes.shape == ref_boxes.shape and labels.shape == ref_labels.shape, (what, boxes.shape, ref_boxes.shape)     # the kept count
    np.testing.assert_array_equal(labels, ref_labels, err_msg=what)
    if len(ref_boxes):
        err = np.abs(boxes.astype(np.float64) - ref_boxes)
        tol = box_tolerance(ref_boxes)
        print(f"{what}: max |box - reference| / tolerance = {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), what


@pytest.mark.parametrize("size", [(64, 64), (96, 64), (100, 72)])
def test_anchors_bit_exact(size):
    ref = G15[f"anchors_{size[0]}x{size[1]}"]
    got = ENC._get_anchor_boxes(size)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    assert got.cpu().numpy().tobytes() == ref.tobytes()
    if size[0] == size[1]:
        assert ENC._get_anchor_boxes(size[0]).cpu().numpy().tobytes() == ref.tobytes()                   # an int
        assert ENC._get_anchor_boxes(torch.Tensor(list(size))).cpu().numpy().tobytes() == ref.tobytes()  # the reference's tensor form


@pytest.mark.parametrize("case", ENC_CASES)
def test_encode_matches_the_reference(case):
    boxes, labels, size = (G15[f"enc_{case}_{k}"] for k in ("boxes", "labels", "size"))
    loc, cls = ENC.encode(dev(boxes), dev(labels), tuple(int(v) for v in size))
    check_loc_cls(loc, cls, G15[f"enc_{case}_loc"], G15[f"enc_{case}_cls"], f"encode {case}")


def test_encode_batch_matches_the_reference_per_image():
    """m70, tie and exact share the (64, 64) anchors: one launch, padded to M = 75 with the padding rows (label -1, boxes that
    would win if they were read) at the front, spread through and at the back."""
    names, M = ["m70", "tie", "exact"], 75
    gt = np.tile(np.array([0, 0, 63, 63], np.float32), (len(names), M, 1))
    lab = np.full((len(names), M), -1, np.int64)
    for i, name in enumerate(names):
        b, l = G15[f"enc_{name}_boxes"], G15[f"enc_{name}_labels"]
        pos = {0: np.arange(5, 5 + len(b)), 1: np.arange(len(b)) * 30 + 3, 2: np.arange(len(b))}[i]       # the order of the rows is kept
        gt[i, pos], lab[i, pos] = b, l
    loc, cls = ENC.encode_batch(dev(gt), dev(lab), 64)
    assert tuple(loc.shape) == (3, 774, 4) and tuple(cls.shape) == (3, 774)
    for i, name in enumerate(names):
        check_loc_cls(loc[i], cls[i], G15[f"enc_{name}_loc"], G15[f"enc_{name}_cls"], f"encode_batch {name}")


def test_encode_image_without_boxes_inside_a_batch():
    b, l = G15["enc_m5_boxes"], G15["enc_m5_labels"]
    gt = np.zeros((2, 7, 4), np.float32)
    lab = np.full((2, 7), -1, np.int64)
    gt[0] = [10, 10, 50, 40]                  # image 0: seven rows of padding only
    gt[1, 2:], lab[1, 2:] = b, l              # image 1: two rows of padding, then the five boxes
    loc, cls = ENC.encode_batch(dev(gt), dev(lab), (96, 64))
    assert not loc[0].any() and not cls[0].any()
    check_loc_cls(loc[1], cls[1], G15["enc_m5_loc"], G15["enc_m5_cls"], "encode_batch m5 beside an empty image")
    loc0, cls0 = ENC.encode(torch.zeros(0, 4).cuda(), torch.zeros(0, dtype=torch.int64).cuda(), (96, 64))       # M = 0: the reference raises
    assert tuple(loc0.shape) == (1161, 4) and not loc0.any() and not cls0.any()
    with pytest.raises(FdError) as ei:
        ENC.encode_batch(torch.zeros(1, 257, 4).cuda(), torch.zeros(1, 257, dtype=torch.int64).cuda(), 64)
    assert ei.value.rc == -2 and "256" in str(ei.value)


@pytest.mark.parametrize("case", DEC_CASES)
def test_decode_matches_the_reference(case):
    loc, cls = anchor_ref.decode_case(case)
    boxes, labels = ENC.decode(dev(loc), dev(cls), 64)
    check_detections(boxes, labels, G15[f"dec_{case}_boxes"], G15[f"dec_{case}_labels"], f"decode {case}")
    if case == "saturated":
        assert int(labels[0]) == 2                 # logits 30, 20, 25, 88 in classes 5, 2, 9, 17 all give 1.0f: the lowest class


def test_decode_batch_matches_the_reference_per_image():
    names = ["c20", "zero", "saturated", "c20"]                     # C = 20 throughout
    pairs = [anchor_ref.decode_case(n) for n in names]
    loc, cls = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    boxes, labels, scores, counts, n_cand = ENC.decode_batch(loc, cls, 64)
    assert tuple(boxes.shape) == (4, 774, 4) and tuple(labels.shape) == tuple(scores.shape) == (4, 774)
    assert counts.dtype == n_cand.dtype == torch.int32
    assert n_cand.tolist() == [int(G15[f"dec_{n}_n_cand"]) for n in names]
    for i, name in enumerate(names):
        n = int(counts[i])
        check_detections(boxes[i, :n], labels[i, :n], G15[f"dec_{name}_boxes"], G15[f"dec_{name}_labels"], f"decode_batch {name}")
        assert (labels[i, n:] == -1).all() and not scores[i, n:].any() and not boxes[i, n:].any()
        s = scores[i, :n].cpu().numpy()
        assert (np.diff(s) < 0).all() and (s > 0.5).all()
    assert float(scores[2, 0]) == 1.0
    for c, name in ((80, "c80"), (3, "c3")):                        # the float4 path with G = 32 and the scalar path
        l1, c1 = anchor_ref.decode_case(name)
        b, lb, _, cnt, nc = ENC.decode_batch(dev(l1)[None], dev(c1)[None], 64, max_candidates=1000)
        assert c1.shape[1] == c and int(nc[0]) == int(G15[f"dec_{name}_n_cand"])
        check_detections(b[0, :int(cnt[0])], lb[0, :int(cnt[0])], G15[f"dec_{name}_boxes"], G15[f"dec_{name}_labels"], f"decode_batch {name}")


def test_decode_unaligned_logits_take_the_scalar_path():
    """C = 20 logits that start 4 bytes into an allocation: C % 4 == 0 but not 16-byte aligned, so no float4 loads."""
    loc, cls = anchor_ref.decode_case("c20")
    buf = torch.zeros(cls.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(774, 20)
    view.copy_(dev(cls))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    boxes, labels = ENC.decode(dev(loc), view, 64)
    check_detections(boxes, labels, G15["dec_c20_boxes"], G15["dec_c20_labels"], "decode c20, unaligned")


def test_decode_single_candidate():
    """The reference raises IndexError on one candidate (.squeeze() to 0-d); here that box comes back."""
    loc, cls = anchor_ref.decode_case("single")
    ref_boxes, ref_labels, _, n_cand = anchor_ref.decode(loc, cls, 64)
    assert n_cand == 1
    boxes, labels = ENC.decode(dev(loc), dev(cls), 64)
    check_detections(boxes, labels, ref_boxes, ref_labels, "decode single")
    _, _, _, counts, nc = ENC.decode_batch(dev(loc)[None], dev(cls)[None], 64)
    assert counts.tolist() == [1] and nc.tolist() == [1]


def test_decode_max_candidates_cap_is_reported():
    loc, cls = anchor_ref.decode_case("c80")
    ref_boxes, ref_labels, ref_scores, n_cand = anchor_ref.decode(loc, cls, 64, max_candidates=64)
    assert n_cand == 275
    boxes, labels, scores, counts, nc = ENC.decode_batch(dev(loc)[None], dev(cls)[None], 64, max_candidates=64)
    assert tuple(boxes.shape) == (1, 64, 4) and nc.tolist() == [275]            # 275 passed the threshold, 64 went on: the caller can see it
    n = int(counts[0])
    check_detections(boxes[0, :n], labels[0, :n], ref_boxes, ref_labels, "decode_batch c80, max_candidates = 64")
    s = scores[0, :n].cpu().numpy()
    assert (np.diff(s) < 0).all() and s[-1] > 0.5 and abs(float(s[0]) - float(ref_scores[0])) < 1e-6
    with pytest.raises(FdError):
        ENC.decode_batch(dev(loc)[None], dev(cls)[None], 64, max_candidates=1025)
