"""CPU-side checks of the anchor codec: the numpy restatement tests/anchor_ref.py against the REAL reference's
recorded outputs (g15_anchor_codec.npz), the new C-ABI entries, their argument checks (all before any launch: no GPU needed)
and the layout of fd_anchor_params."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import anchor_ref  # noqa: E402
from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd._lib import FdError  # noqa: E402
from pytorch_object_detection_amd.utill.utills import DataEncoder  # noqa: E402

G15 = np.load(os.path.join(HERE, "golden", "g15_anchor_codec.npz"))
ENC_CASES = ["m1", "m5", "m70", "tie", "exact"]
DEC_CASES = ["c20", "c80", "c3", "zero", "saturated"]
# log / exp are documented at <= 1 ulp on each side: 2 ulp of distance, 4 allowed as margin for the final rounding (derived, not tuned)
ULP_BOUND = 4


def box_tolerance(ref_boxes: np.ndarray) -> np.ndarray:
    """4 * 2^-23 * (|xy| + wh) per coordinate, xy / wh the centre and size of the reference box along that axis."""
    c = np.abs((ref_boxes[:, :2] + ref_boxes[:, 2:]) / 2)
    wh = ref_boxes[:, 2:] - ref_boxes[:, :2]
    t = 4 * 2.0 ** -23 * (c + wh)
    return np.concatenate([t, t], 1)


@pytest.mark.parametrize("size", [(64, 64), (96, 64), (100, 72)])
def test_restated_anchors_are_the_reference_bit_for_bit(size):
    ref = G15[f"anchors_{size[0]}x{size[1]}"]
    got = anchor_ref.anchor_boxes(size)
    assert got.dtype == np.float32 and got.shape == ref.shape == (anchor_ref.num_anchors(size), 4)
    assert got.tobytes() == ref.tobytes()
    assert anchor_ref.anchor_wh().tobytes() == G15["anchor_wh"].tobytes()


def test_anchor_counts_and_grid():
    assert [anchor_ref.num_anchors(s) for s in (64, (96, 64), (100, 72), 640)] == [774, 1161, 1521, 76725]
    p = ops.anchor_params((100, 72), anchor_ref.anchor_wh())
    assert (p.fm_w[0], p.fm_h[0], p.num_anchors) == (13, 9, 1521)
    assert p.grid_w[0] == np.float32(100) / np.float32(13) and p.grid_h[0] == 8.0        # the grid is not the stride
    assert np.array(p.wh, np.float32).tobytes() == G15["anchor_wh"].tobytes()
    enc = DataEncoder()
    assert enc.anchor_wh.numpy().tobytes() == G15["anchor_wh"].tobytes() and enc.anchor_wh.shape == (5, 9, 2)
    assert enc._anchor_params(64) is enc._anchor_params((64, 64)) and enc._anchor_params(torch.Tensor([64, 64])).num_anchors == 774


@pytest.mark.parametrize("case", ENC_CASES)
def test_restated_encode_matches_the_reference(case):
    boxes, labels, size = (G15[f"enc_{case}_{k}"] for k in ("boxes", "labels", "size"))
    loc, cls, _ = anchor_ref.encode(boxes, labels, tuple(int(v) for v in size))
    ref_loc, ref_cls = G15[f"enc_{case}_loc"], G15[f"enc_{case}_cls"]
    np.testing.assert_array_equal(cls, ref_cls)
    assert loc[:, :2].tobytes() == ref_loc[:, :2].tobytes()
    d = anchor_ref.ulp_distance(loc[:, 2:], ref_loc[:, 2:])
    print(f"{case}: max ulp distance of loc_wh (numpy log vs the reference's) = {int(d.max())}")
    assert d.max() <= ULP_BOUND


def test_encode_fixture_holds_the_decisive_cases():
    assert G15["enc_m70_boxes"].shape[0] == 70 and (G15["enc_m70_cls"] == -1).any()
    t = G15["enc_tie_cls"]
    assert (t == 5).any() and not (t == 10).any()                  # two identical boxes, labels 4 and 9: the first wins
    _, cls, mx = anchor_ref.encode(G15["enc_exact_boxes"], G15["enc_exact_labels"], 64)
    rows = G15["enc_exact_rows"]
    assert len(rows) >= 1 and (mx[rows] == np.float32(0.5)).all() and (cls[rows] > 0).all()      # max_iou == 0.5 exactly: a positive


@pytest.mark.parametrize("case", DEC_CASES)
def test_restated_decode_matches_the_reference(case):
    loc, cls = anchor_ref.decode_case(case)
    boxes, labels, scores, n_cand = anchor_ref.decode(loc, cls, anchor_ref.DECODE_SIZE)
    ref_boxes, ref_labels = G15[f"dec_{case}_boxes"], G15[f"dec_{case}_labels"]
    assert n_cand == int(G15[f"dec_{case}_n_cand"]) and cls.shape[1] == anchor_ref.DECODE_CASES[case][0]
    np.testing.assert_array_equal(labels, ref_labels)
    assert boxes.shape == ref_boxes.shape and (np.diff(scores) <= 0).all()
    assert (np.abs(boxes.astype(np.float64) - ref_boxes) <= box_tolerance(ref_boxes.astype(np.float64))).all()
    if case == "saturated":
        assert scores[0] == 1.0 and labels[0] == 2 and cls[anchor_ref.SATURATED_ROW].argmax() == 17      # an argmax over logits is wrong
    if case == "c80":
        assert n_cand == 275


def test_restatement_of_what_the_reference_lacks():
    loc, cls = anchor_ref.decode_case("single")
    boxes, labels, _, n_cand = anchor_ref.decode(loc, cls, 64)
    assert n_cand == 1 and boxes.shape == (1, 4) and labels.shape == (1,)
    loc, cls = anchor_ref.decode_case("c80")
    full = anchor_ref.decode(loc, cls, 64)
    cut = anchor_ref.decode(loc, cls, 64, max_candidates=64)
    assert cut[3] == 275 and 0 < len(cut[1]) < len(full[1])
    np.testing.assert_array_equal(cut[0][:5], full[0][:5])          # the best candidates are the same either way
    l0, c0, _ = anchor_ref.encode(np.zeros((3, 4)), [-1, -1, -1], 64)
    assert not l0.any() and not c0.any()


def test_new_exports_are_declared():
    lib = _lib.lib()
    for name in ("fd_anchor_boxes", "fd_anchor_encode", "fd_anchor_decode", "fd_anchor_decode_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("anchor_params", "anchor_boxes", "anchor_encode", "anchor_decode"):
        assert callable(getattr(ops, name))
    for name in ("_get_anchor_wh", "_get_anchor_boxes", "_meshgrid", "_change_box_order", "encode", "decode", "encode_batch", "decode_batch",
                 "_box_iou", "_box_nms"):
        assert callable(getattr(DataEncoder, name))


def test_struct_layout_matches_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "fcosdet.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(fd_anchor_params), offsetof(fd_anchor_params, fm_w),
        offsetof(fd_anchor_params, fm_h), offsetof(fd_anchor_params, grid_w), offsetof(fd_anchor_params, grid_h),
        offsetof(fd_anchor_params, wh) * 1000 + offsetof(fd_anchor_params, num_anchors), FD_ANCHOR_LEVELS, FD_ANCHOR_PER_CELL,
        FD_ANCHOR_MAX_GT, FD_ANCHOR_MAX_CLASSES, FD_ANCHOR_MAX_CAND); return 0; }'''
    exe = os.path.join(ROOT, "oracle", "_build", "abi_probe_anchor")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    P = _lib.AnchorParams
    assert vals == [ctypes.sizeof(P), P.fm_w.offset, P.fm_h.offset, P.grid_w.offset, P.grid_h.offset, P.wh.offset * 1000 + P.num_anchors.offset,
                    ops.ANCHOR_LEVELS, ops.ANCHOR_PER_CELL, _lib.ANCHOR_MAX_GT, _lib.ANCHOR_MAX_CLASSES, _lib.ANCHOR_MAX_CAND]
    assert ctypes.sizeof(P) == 4 * (20 + 90 + 1)


def test_argument_errors_come_before_any_launch():
    """Every call below must be refused by the host-side checks: this machine may have no GPU, and a launch would fail differently."""
    lib = _lib.lib()
    p = ops.anchor_params(64, anchor_ref.anchor_wh())
    A, ok16, odd = p.num_anchors, 4096, 4100          # never dereferenced: the checks refuse the call first
    ref = ctypes.byref(p)

    def refused(rc, code, word):
        assert rc == code, (rc, lib.fd_last_error())
        assert word.encode() in lib.fd_last_error(), lib.fd_last_error()

    refused(lib.fd_anchor_boxes(None, ok16, A, None), _lib.E_INVAL, "null")
    refused(lib.fd_anchor_boxes(ref, None, A, None), _lib.E_INVAL, "null")
    refused(lib.fd_anchor_boxes(ref, odd, A, None), _lib.E_INVAL, "aligned")
    refused(lib.fd_anchor_boxes(ref, ok16, A + 9, None), _lib.E_INVAL, "774")
    refused(lib.fd_anchor_encode(ref, ok16, ok16, 1, 4, A, None, ok16, None), _lib.E_INVAL, "null")
    refused(lib.fd_anchor_encode(ref, None, ok16, 1, 4, A, ok16, ok16, None), _lib.E_INVAL, "null")
    refused(lib.fd_anchor_encode(ref, ok16, ok16, 0, 4, A, ok16, ok16, None), _lib.E_INVAL, "B=0")
    refused(lib.fd_anchor_encode(ref, ok16, ok16, 1, -1, A, ok16, ok16, None), _lib.E_INVAL, "M=-1")
    refused(lib.fd_anchor_encode(ref, ok16, ok16, 1, _lib.ANCHOR_MAX_GT + 1, A, ok16, ok16, None), _lib.E_UNSUPPORTED, "256")
    refused(lib.fd_anchor_encode(ref, odd, ok16, 1, 4, A, ok16, ok16, None), _lib.E_INVAL, "aligned")
    refused(lib.fd_anchor_encode(ref, ok16, ok16, 1, 4, A - 9, ok16, ok16, None), _lib.E_INVAL, "774")
    dec = lambda **k: lib.fd_anchor_decode(*[k.get(n, d) for n, d in (("p", ref), ("loc", ok16), ("cls", ok16), ("B", 1), ("A", A), ("C", 20), ("ct", 0.5),  # noqa: E731
                                                                    ("nt", 0.5), ("mc", 1000), ("boxes", ok16), ("labels", ok16), ("scores", ok16),
                                                                    ("counts", ok16), ("n_cand", ok16), ("ws", ok16), ("stream", None))])
    refused(dec(ws=None), _lib.E_INVAL, "null")
    refused(dec(cls=None), _lib.E_INVAL, "null")
    refused(dec(B=70000), _lib.E_INVAL, "B=70000")
    refused(dec(C=0), _lib.E_INVAL, "C=0")
    refused(dec(C=129), _lib.E_UNSUPPORTED, "128")
    refused(dec(mc=0), _lib.E_INVAL, "max_candidates")
    refused(dec(mc=1025), _lib.E_UNSUPPORTED, "1024")
    refused(dec(ct=1.5), _lib.E_INVAL, "cls_thresh")
    refused(dec(loc=odd), _lib.E_INVAL, "aligned")
    refused(dec(ws=ok16 + 16), _lib.E_INVAL, "aligned")
    refused(dec(A=A + 9), _lib.E_INVAL, "774")
    bad = ops.anchor_params(64, anchor_ref.anchor_wh())
    bad.fm_w[2] = 0
    refused(lib.fd_anchor_boxes(ctypes.byref(bad), ok16, A, None), _lib.E_INVAL, "fd_anchor_params")
    bad = ops.anchor_params(64, anchor_ref.anchor_wh())
    bad.num_anchors = A + 1
    refused(lib.fd_anchor_boxes(ctypes.byref(bad), ok16, A, None), _lib.E_INVAL, "774")
    assert lib.fd_anchor_decode_workspace_bytes(1, A, 1000) > 774 * 24
    assert lib.fd_anchor_decode_workspace_bytes(16, 76725, 1000) < 16 * 76725 * 24 + (1 << 20)
    for bad_args in ((0, A, 1000), (1, 0, 1000), (1, A, 0), (1, A, 1025), (70000, A, 10)):
        assert lib.fd_anchor_decode_workspace_bytes(*bad_args) == -1, bad_args


def test_wrappers_refuse_what_is_not_cuda_fp32_int64(monkeypatch):
    enc = DataEncoder()
    with pytest.raises(FdError):
        enc.encode(torch.rand(2, 4), torch.zeros(2, dtype=torch.int64), 64)                 # CPU tensors
    with pytest.raises(FdError):
        enc.decode(torch.rand(774, 4), torch.rand(774, 20), 64)
    with pytest.raises(FdError):
        enc._get_anchor_boxes(64, device="cpu")
    with pytest.raises(FdError):
        enc.encode([[0, 0, 1, 1]], [1], 64)                                                   # not tensors
    with pytest.raises(FdError):
        ops.anchor_params(0, anchor_ref.anchor_wh())
    with pytest.raises(FdError):
        ops.anchor_params(64, np.ones((5, 8, 2)))

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)       # dtype / shape checks, with the device check bypassed
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(FdError):
        enc.encode_batch(torch.rand(1, 2, 4, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.int64), 64)
    with pytest.raises(FdError):
        enc.encode_batch(torch.rand(1, 2, 4), torch.zeros(1, 2, dtype=torch.int32), 64)
    with pytest.raises(FdError):
        enc.encode_batch(torch.rand(1, 2, 4), torch.zeros(1, 3, dtype=torch.int64), 64)
    with pytest.raises(FdError):
        enc.decode_batch(torch.rand(1, 774, 4), torch.rand(1, 774, 20).half(), 64)
    with pytest.raises(FdError):
        enc.decode_batch(torch.rand(1, 773, 4), torch.rand(1, 773, 20), 64)
    with pytest.raises(FdError):
        enc.decode_batch(torch.rand(1, 774, 4), torch.rand(1, 774, 40)[:, :, ::2], 64)        # not contiguous


def test_host_helpers_keep_the_reference_semantics():
    enc = DataEncoder()
    m = enc._meshgrid(3, 2)
    assert m.dtype == torch.int64 and m.tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]]
    assert enc._meshgrid(3, 2, row_major=False).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2]]
    b = torch.tensor([[10., 12., 40., 44.]])
    xywh = enc._change_box_order(b, 'xyxy2xywh')
    assert xywh.tolist() == [[25., 28., 31., 33.]]
    assert enc._change_box_order(xywh, 'xywh2xyxy').tolist() == [[9.5, 11.5, 40.5, 44.5]]      # half a pixel larger than the input
    with pytest.raises(AssertionError):
        enc._change_box_order(b, 'xyxy')
