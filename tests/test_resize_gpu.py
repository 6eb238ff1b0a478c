"""GPU checks of the on-device resize (csrc/fd_resize.hip): fd_resize_u8 / fd_resize_collate_u8_nhwc4 /
fd_boxes_scale_batch and PlannedModule.forward_raw / detect_raw on top of them.  Every comparison is exact: the kernels against
the numpy restatement (tests/resize_ref.py), the fused launch against kernels that are already tested (collate_u8,
boxes_rescale_xywh_), the raw-image model paths against forward_images / detect_padded on the separately resized images."""
import os

import numpy as np
import pytest
import torch

import resize_ref
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.modules.head import ClipBoxes, FCOSHead
from pytorch_object_detection_amd.model.od import FCOS, HalfInvertedStageFCOS
from pytorch_object_detection_amd.utill.utills import pad32, resize_rule
from test_model_gpu import randomize_norms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_resize_rule.npz")


def rand_img(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("src,dst", [((480, 640), (800, 1066)), ((1200, 1600), (800, 1066)), ((37, 53), (357, 512)), ((289, 333), (799, 921)),
                                     ((5, 7), (5, 7)), ((1, 9), (4, 30)), ((640, 427), (1199, 800)), ((1, 1), (3, 5)), ((33, 65), (1, 1))])
def test_resize_u8_equals_the_restatement_bit_for_bit(src, dst):
    img = rand_img(np.random.default_rng(src[0] + dst[1]), *src)
    got = ops.resize_u8(torch.from_numpy(img).to(DEV), *dst)
    assert got.dtype == torch.uint8 and tuple(got.shape) == dst + (3,)
    got = got.cpu().numpy()
    exp = resize_ref.resize_u8(img, *dst)
    print(f"{src} -> {dst}: {int((got != exp).sum())} differing levels")
    np.testing.assert_array_equal(got, exp)          # no pixel excluded
    if src == dst:
        np.testing.assert_array_equal(got, img)


def test_resize_collate_equals_resize_then_collate():
    rng = np.random.default_rng(21)
    raws = [rand_img(rng, h, w) for h, w in [(120, 160), (160, 120), (75, 100), (37, 53), (200, 90)]]
    dst = [(96, 128), (171, 128), (96, 128), (60, 86), (159, 71)]       # up, up, non-uniform, odd, down
    H, W = max(pad32(a) for a, _ in dst), max(pad32(b) for _, b in dst)
    assert (H, W) == (192, 160)
    dev = [torch.from_numpy(im).to(DEV) for im in raws]
    got, _ = ops.resize_collate_u8(dev, dst, H, W, MEAN, STD)
    resized = [ops.resize_u8(t, a, b) for t, (a, b) in zip(dev, dst)]
    exp, _ = ops.collate_u8(resized, H, W, MEAN, STD)
    assert torch.equal(got, exp)
    # ... and against the host restatement; the padding zone is (0 - mean) / std, channel 3 is zero everywhere
    g = got.cpu().numpy().reshape(len(raws), H, W, 4)
    pad = resize_ref.normalise(np.zeros((1, 3), np.uint8), MEAN, STD)[0]
    for n, (im, (a, b)) in enumerate(zip(raws, dst)):
        np.testing.assert_array_equal(g[n, :a, :b], resize_ref.normalise(resize_ref.resize_u8(im, a, b), MEAN, STD))
        assert (g[n, a:, :] == pad).all() and (g[n, :, b:] == pad).all()
        assert g[n, a:, :].size > 0 and g[n, :, b:].size > 0
    assert (g[..., 3] == 0).all()
    # every dst_hw == src_hw: the plain collate of the raw images
    same, _ = ops.resize_collate_u8(dev, [im.shape[:2] for im in raws], 224, 192, MEAN, STD)
    plain, _ = ops.collate_u8(dev, 224, 192, MEAN, STD)
    assert torch.equal(same, plain)


def _models():
    torch.manual_seed(5)
    his = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval()
    randomize_norms(his, 7)
    fcos = FCOS([2048, 1024, 512], 20, 256).eval()
    randomize_norms(fcos, 8)
    return [("HISFCOS", his.to(DEV)), ("FCOS", fcos.to(DEV))]


# two mixed-aspect batches of raw images and the (min_side, max_side) that puts them on two different canvases
RAW_BATCHES = [([(60, 80), (80, 60), (75, 100), (37, 53)], (96, 160)),
               ([(120, 90), (50, 131), (64, 64)], (128, 224))]


def _resized_by_rule(dev_imgs, size):
    rules = [resize_rule(int(t.shape[0]), int(t.shape[1]), size) for t in dev_imgs]
    return rules, [ops.resize_u8(t, nh, nw) for t, (_, nh, nw) in zip(dev_imgs, rules)]


def test_forward_raw_equals_forward_images_on_resized_images():
    g = np.load(G13)
    table = {tuple(r): tuple(v) for r, v in zip(g["shapes"].tolist(), g["resized"].tolist())}
    assert resize_rule(289, 333, (800, 1333))[1:] == table[(289, 333, 800, 1333)] == (799, 921)      # the rule the fixture pins
    rng = np.random.default_rng(31)
    canvases = set()
    for name, model in _models():
        for sizes, rs in RAW_BATCHES:
            dev = [torch.from_numpy(rand_img(rng, h, w)).to(DEV) for h, w in sizes]
            rules, resized = _resized_by_rule(dev, rs)
            exp = [[t.clone() for t in grp] for grp in model.forward_images(resized)]
            got = model.forward_raw(dev, rs)
            plan = model.raw_plan_for(dev, rs)
            assert plan.input_mode == "resize" and plan.canvas_hw == model.plan_for(resized).canvas_hw
            assert plan.resized_hw == [(nh, nw) for _, nh, nw in rules]
            np.testing.assert_array_equal(plan.scales.cpu().numpy(), np.array([s for s, _, _ in rules], np.float64).astype(np.float32))
            canvases.add(plan.canvas_hw)
            for ge, gg in zip(exp, got):
                for u, v in zip(ge, gg):
                    assert torch.equal(u, v), name
    assert len(canvases) == 2, canvases


def test_detect_raw_equals_the_separate_steps():
    rng = np.random.default_rng(41)
    head = FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64, 128])
    name, model = _models()[0]
    sizes, rs = RAW_BATCHES[0]
    dev = [torch.from_numpy(rand_img(rng, h, w)).to(DEV) for h, w in sizes]
    rules, resized = _resized_by_rule(dev, rs)
    H, W = model.plan_for(resized).canvas_hw
    s0, c0, b0, n0 = head.detect_padded(model.forward_images(resized))
    b0 = ops.clip_boxes_(b0.contiguous(), H, W)           # ClipBoxes()(batch_imgs, boxes) with batch_imgs [B, 3, H, W]
    s0, c0, b0, n0 = s0.clone(), c0.clone(), b0.clone(), n0.clone()
    counts = n0.cpu().numpy()
    print("detections per image:", counts.tolist())
    assert counts.sum() > 0

    # xywh in source coordinates: the existing single-scale launch, image by image
    exp = b0.clone()
    for b, (sc, _, _) in enumerate(rules):
        ops.boxes_rescale_xywh_(exp[b], sc)
    s1, c1, b1, n1, scales = model.detect_raw(dev, head, rs, source_coords=True, xywh=True)
    assert torch.equal(s1, s0) and torch.equal(c1, c0) and torch.equal(n1, n0)
    assert torch.equal(b1, exp)
    f32 = np.array([sc for sc, _, _ in rules], np.float64).astype(np.float32)     # the rule's double rounded once to fp32
    np.testing.assert_array_equal(scales.cpu().numpy(), f32)

    # xyxy in source coordinates: IEEE fp32 division on the host
    _, _, b2, n2, _ = model.detect_raw(dev, head, rs, source_coords=True, xywh=False)
    host = b0.cpu().numpy()
    for b in range(len(dev)):
        host[b, :counts[b]] = host[b, :counts[b]] / f32[b]
    np.testing.assert_array_equal(b2.cpu().numpy(), host)
    for b in range(len(dev)):
        assert (b2[b, counts[b]:] == 0).all()             # rows beyond counts: still detect_padded's zeros

    # canvas coordinates: nothing but the clip
    _, _, b3, _, _ = model.detect_raw(dev, head, rs, source_coords=False)
    assert torch.equal(b3, b0)
    _, _, b4, _, _ = model.detect_raw(dev, head, rs, clip=False, source_coords=False)
    assert torch.equal(ClipBoxes()(torch.empty(len(dev), 3, H, W, device=DEV), b4.clone()), b0)


def test_boxes_scale_batch_counts_and_ground_truth_side():
    g = np.load(G13)
    # invert = False: the reference's scaled ground-truth boxes (fp32 product), every g13 row one "image" with 4 boxes
    boxes = torch.from_numpy(g["boxes_in"].copy()).to(DEV)
    scales = torch.from_numpy(g["scale"].astype(np.float32)).to(DEV)
    out = ops.boxes_scale_batch_(boxes, scales, invert=False)
    assert out is boxes
    np.testing.assert_array_equal(out.cpu().numpy(), g["boxes_out"])
    # counts: rows at or beyond counts[b] keep whatever they held; invert + xywh on the rest
    rng = np.random.default_rng(51)
    B, K = 5, 37
    raw = rng.uniform(-50, 900, (B, K, 4)).astype(np.float32)
    cnt = np.array([0, 1, 17, 36, 37], np.int32)
    sc = np.array([0.5, 1.6660000085830688, 1.0, 2.4, 0.3125], np.float32)
    exp = raw.copy()
    for b in range(B):
        v = exp[b, :cnt[b]] / sc[b]
        v[:, 2] = v[:, 2] - v[:, 0]
        v[:, 3] = v[:, 3] - v[:, 1]
        exp[b, :cnt[b]] = v
    got = ops.boxes_scale_batch_(torch.from_numpy(raw.copy()).to(DEV), torch.from_numpy(sc).to(DEV), torch.from_numpy(cnt).to(DEV), invert=True, xywh=True)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    # counts = None: all K rows, against the single-scale launch
    allrows = ops.boxes_scale_batch_(torch.from_numpy(raw.copy()).to(DEV), torch.from_numpy(sc).to(DEV), None, invert=True, xywh=True)
    one = torch.from_numpy(raw.copy()).to(DEV)
    for b in range(B):
        ops.boxes_rescale_xywh_(one[b], float(sc[b]))
    assert torch.equal(allrows, one)


def test_rejections_launch_nothing():
    img = torch.zeros(8, 9, 3, dtype=torch.uint8, device=DEV)
    out = torch.full((32 * 32, 4), 7.0, device=DEV)
    boxes = torch.full((2, 3, 4), 5.0, device=DEV)
    scales = torch.full((2,), 2.0, device=DEV)
    bad_images = [img.cpu(), img.float(), img[0], img[:, :, :2], torch.zeros(0, 9, 3, dtype=torch.uint8, device=DEV), img.permute(1, 0, 2)]
    for t in bad_images:
        with pytest.raises(FdError):
            ops.resize_u8(t, 4, 4)
        with pytest.raises(FdError):
            ops.resize_collate_u8([img, t], [(8, 9), (8, 9)], 32, 32, MEAN, STD, out=torch.cat([out, out]))
    with pytest.raises(FdError):
        ops.resize_u8(img, 0, 4)
    for dst in ([(8, 9)], [(8, 9), (33, 9)], [(8, 9), (8, 0)]):      # one size too few, taller than the canvas, empty
        with pytest.raises(FdError):
            ops.resize_collate_u8([img, img], dst, 32, 32, MEAN, STD, out=torch.cat([out, out]))
    with pytest.raises(FdError):
        ops.resize_collate_u8([], [], 32, 32, MEAN, STD)
    with pytest.raises(FdError):
        ops.resize_collate_u8([img], [(8, 9)], 32, 32, MEAN, STD, out=out[:-1])
    for args in [(boxes.cpu(), scales), (boxes, scales.cpu()), (boxes, scales[:1]), (boxes, torch.ones(3, device=DEV)), (boxes[0], scales),
                 (boxes.double(), scales), (boxes, scales.double()), (boxes, scales, torch.zeros(3, dtype=torch.int32, device=DEV)),
                 (boxes, scales, torch.zeros(2, dtype=torch.int64, device=DEV)), (boxes, scales, torch.zeros(2, dtype=torch.int32))]:
        with pytest.raises(FdError):
            ops.boxes_scale_batch_(*args)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (boxes == 5.0).all()        # nothing was launched on the buffers handed in
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval().to(DEV)
    big = torch.zeros(100, 120, 3, dtype=torch.uint8, device=DEV)
    for bad in ([], [big.cpu()], [big.float()], [big[0]], big):
        with pytest.raises(FdError):
            model.forward_raw(bad, (96, 160))
    model.forward_raw([big, big], (96, 160))
    plan = model.raw_plan_for([big, big], (96, 160))
    assert plan.canvas_hw == (128, 128) and plan.resized_hw == [(96, 115)] * 2
    with pytest.raises(FdError, match="resize"):
        plan.capture_graph()
    assert plan.graph is None
    # a list handed to forward_images still means ALREADY RESIZED images: another plan, canvas from the images' own sizes
    other = model.plan_for([big, big])
    assert other is not plan and other.input_mode == "collate" and other.canvas_hw == (128, 128)
