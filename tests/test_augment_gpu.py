"""GPU checks of the on-device training augmentations (csrc/fd_augment.hip, data/augment.py).  Every comparison is
exact: the single-step kernels against the numpy restatement (tests/augment_ref.py) and against the pixels PIL returned
(tests/golden/g14_augment.npz), the L sums against integer sums, the fused launch against the single steps chained on the
device and against the already tested resize_collate_u8, collate_train_raw against the reference's boxes of the fixture."""
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as A
import resize_ref
from pytorch_object_detection_amd import ops
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.data.augment import collate_train_raw, sample_params
from pytorch_object_detection_amd.utill.utills import pad32, resize_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
G14 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_augment.npz")
B, C_, S, HUE = ops.AUG_OP_BRIGHTNESS, ops.AUG_OP_CONTRAST, ops.AUG_OP_SATURATION, ops.AUG_OP_HUE
FULL = [(S, 1.07), (B, 0.93), (HUE, 20), (C_, 1.09)]


def rand_img(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_rotate_u8_equals_restatement_and_pil():
    g = np.load(G14)
    for k, (i, d) in enumerate(zip(g["rot_img"], g["rot_d"])):
        got = ops.rotate_u8(dev(g[f"img{int(i)}"]), float(d)).cpu().numpy()
        np.testing.assert_array_equal(got, g[f"rot_out_{k}"], err_msg=f"PIL pixels, d={d}")
    rng = np.random.default_rng(3)
    for (h, w), d in [((37, 53), 9.99), ((1, 9), -5.0), ((9, 1), 3.0), ((1, 1), 7.0), ((240, 320), -10.0), ((301, 199), 89.9), ((64, 64), -45.0),
                      ((50, 70), 1e-9)]:
        img = rand_img(rng, h, w)
        got = ops.rotate_u8(dev(img), d).cpu().numpy()
        exp = A.rotate_u8(img, d)
        print(f"rotate {h}x{w} d={d}: {int((got != exp).any(-1).sum())} differing pixels")
        np.testing.assert_array_equal(got, exp)
    img = dev(rand_img(rng, 20, 30))
    same = ops.rotate_u8(img, 0.0)
    assert torch.equal(same, img) and same.data_ptr() != img.data_ptr()


def test_color_jitter_u8_equals_restatement_and_pil():
    g = np.load(G14)
    for k, (i, op, arg) in enumerate(zip(g["enh_img"], g["enh_op"], g["enh_arg"])):
        op = int(op)
        a = int(arg) if op == HUE else float(arg)
        got = ops.color_jitter_u8(dev(g[f"img{int(i)}"]), [(op, a)]).cpu().numpy()
        print(f"op {op} arg {a}: {int((got != g[f'enh_out_{k}']).sum())} differing levels against PIL")
        np.testing.assert_array_equal(got, g[f"enh_out_{k}"])
    rng = np.random.default_rng(4)
    chains = [FULL, [(C_, 0.91), (HUE, 231), (B, 1.1), (S, 0.9)], [(HUE, 128), (S, 1.1)], [(B, 1.5)], [(S, 0.0)], [(C_, 2.0)], [(HUE, 0)], []]
    for chain in chains:
        for h, w in [(33, 47), (1, 5), (120, 77)]:
            img = rand_img(rng, h, w)
            got = ops.color_jitter_u8(dev(img), chain).cpu().numpy()
            np.testing.assert_array_equal(got, A.color_jitter_u8(img, chain), err_msg=str(chain))
    # the colour cube sampled on a lattice that holds every grey, every primary edge and 64^3 other colours: hue alone, both shifts
    c = np.arange(0, 256, 4, dtype=np.uint8)
    cube = np.stack(np.meshgrid(c, c + 1, c + 3, indexing="ij"), -1).reshape(512, 512, 3)
    for shift in (0, 25, 231, 128):
        np.testing.assert_array_equal(ops.color_jitter_u8(dev(cube), [(HUE, shift)]).cpu().numpy(), A.color_jitter_u8(cube, [(HUE, shift)]))


def _tables(images, recs):
    ptrs = torch.tensor([t.data_ptr() for t in images], dtype=torch.int64).to(DEV)
    return ptrs, torch.tensor(recs, dtype=torch.int32).to(DEV)


def test_jitter_l_sums_are_the_integer_sums():
    rng = np.random.default_rng(6)
    sizes = [(37, 53), (300, 451), (1, 1), (64, 96), (641, 359), (5, 7)]
    chains = [[(B, 0.9), (HUE, 25), (C_, 1.05), (S, 1.1)], [(C_, 1.1)], [(HUE, 3)], [(S, 1.1), (B, 1.02), (HUE, 250), (C_, 0.9)], [], [(B, 1.1), (C_, 1.0)]]
    raws = [rand_img(rng, h, w) for h, w in sizes]
    raws[1] = np.full_like(raws[1], 255)                       # contrast first in its chain: the raw image's L, the largest sum per pixel
    images = [dev(r) for r in raws]
    recs = [ops.augment_record(h, w, chain=c) for (h, w), c in zip(sizes, chains)]
    ptrs, recs_dev = _tables(images, recs)
    sums = torch.full((len(sizes),), -5, dtype=torch.int64, device=DEV)
    out = ops.jitter_l_sums(images, recs_dev, ptrs, sums)
    assert out is sums
    got, got_recs = sums.cpu().numpy(), recs_dev.cpu().numpy()
    for n, (raw, chain) in enumerate(zip(raws, chains)):
        s, m = A.l_sum_and_mean(raw, chain)
        assert int(got[n]) == s, (n, int(got[n]), s)
        assert int(got_recs[n, 25]) == m
        exp = np.array(recs[n])
        exp[25] = m
        np.testing.assert_array_equal(got_recs[n], exp)        # nothing else in the record moved
    assert int(got[1]) == 255 * 300 * 451 and int(got_recs[1, 25]) == 255


# flip, jitter chain, rotation, crop (x, y, cw, ch), raw size, resized size: every combination of the four switches occurs, odd sizes,
# a 1-pixel-wide and a 1-pixel-high crop, up- and down-scaling, contrast first / last / in the middle / absent
def _mixed_batch():
    chains = [FULL, [(C_, 1.08), (B, 0.95)], [(HUE, 240), (S, 1.1), (B, 1.04)], [(B, 1.1), (C_, 0.92), (HUE, 12)]]
    sizes = [(37, 53), (60, 80), (80, 60), (75, 101), (33, 47), (120, 90), (51, 131), (64, 64)]
    out = []
    for k in range(16):
        flip, jit, rot, crop = bool(k & 1), bool(k & 2), bool(k & 4), bool(k & 8)
        h, w = sizes[k % 8]
        rect = None
        if crop:
            rect = [(3, 5, w - 11, h - 9), (w - 1, 0, 1, h), (0, h - 1, w, 1), (7, 2, 20, 30)][(k >> 1) & 3]
        ch, cw = (rect[3], rect[2]) if rect else (h, w)
        nh, nw = [(ch * 2 + 1, cw * 2 - 1), (max(1, ch // 2), max(1, cw // 2 + 1)), (ch, cw), (ch + 17, max(1, cw - 3))][k % 4]
        out.append(dict(flip=flip, chain=chains[(k >> 2) & 3] if jit else [], d=[7.3, -10.0, 2.5, -0.8][k & 3] if rot else 0.0, crop=rect, nh=nh, nw=nw,
                        hw=(h, w)))
    return out


def test_fused_launch_equals_the_single_steps_chained():
    rng = np.random.default_rng(8)
    cases = _mixed_batch()
    raws = [rand_img(rng, *c["hw"]) for c in cases]
    params = [{k: v for k, v in c.items() if k != "hw"} for c in cases]
    H, W = max(pad32(p["nh"]) for p in params), max(pad32(p["nw"]) for p in params)
    images = [dev(r) for r in raws]
    got, _ = ops.augment_resize_collate_u8(images, params, H, W, MEAN, STD)
    assert got.shape == (16, 3, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    # single steps on the device: flip -> colour chain -> rotation -> crop (a slice) -> resize -> collate (NHWC4), re-laid to planar
    stepped = []
    for t, p in zip(images, params):
        u = torch.flip(t, [1]).contiguous() if p["flip"] else t
        u = ops.color_jitter_u8(u, p["chain"])
        u = ops.rotate_u8(u, p["d"])
        if p["crop"]:
            x, y, cw, ch = p["crop"]
            u = u[y:y + ch, x:x + cw].contiguous()
        stepped.append(ops.resize_u8(u, p["nh"], p["nw"]))
    rows, _ = ops.collate_u8(stepped, H, W, MEAN, STD)
    exp = rows.view(16, H, W, 4)[..., :3].permute(0, 3, 1, 2).contiguous()
    diff = (got != exp).flatten(1).sum(1).cpu().tolist()
    print("differing values per image:", diff)
    assert torch.equal(got, exp)
    # ... and the host restatement of the whole path
    g = got.cpu().numpy()
    for n, (raw, p) in enumerate(zip(raws, params)):
        e = A.fused_planar(raw, p["nh"], p["nw"], H, W, MEAN, STD, flip=p["flip"], chain=p["chain"], d=p["d"], crop=p["crop"])
        np.testing.assert_array_equal(g[n], e, err_msg=f"image {n}: {p}")


def test_identity_parameters_equal_resize_collate_u8():
    rng = np.random.default_rng(21)
    raws = [rand_img(rng, h, w) for h, w in [(120, 160), (160, 120), (75, 100), (37, 53), (200, 90)]]
    dst = [(96, 128), (171, 128), (96, 128), (60, 86), (159, 71)]
    H, W = 192, 160
    images = [dev(r) for r in raws]
    exp, _ = ops.resize_collate_u8(images, dst, H, W, MEAN, STD)
    exp = exp.view(5, H, W, 4)[..., :3].permute(0, 3, 1, 2).contiguous()
    out = torch.full((5, 3, H, W), 9.0, device=DEV)
    got, _ = ops.augment_resize_collate_u8(images, [dict(nh=a, nw=b) for a, b in dst], H, W, MEAN, STD, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, exp)


def test_collate_train_raw_against_the_reference_rows():
    g = np.load(G14)
    rs = (96, 160)
    small = [i for i in range(len(g["a_seed"])) if tuple(g["a_hw"][i]) in ((37, 53), (64, 96))]
    seen = set()
    rng = np.random.default_rng(9)
    for i in small[:48]:
        h, w = (int(v) for v in g["a_hw"][i])
        n = int(g["a_nbox"][i])
        raw = rand_img(rng, h, w)
        classes = np.arange(3, 3 + n)
        imgs, boxes, cls, params = collate_train_raw([dev(raw)], [g["a_boxes_in"][i, :n].copy()], [classes], rs, rng=random.Random(int(g["a_seed"][i])),
                                                     return_params=True)
        p = params[0]
        oh, ow = (int(v) for v in g["a_out_hw"][i])
        scale, nh, nw = resize_rule(oh, ow, rs)
        exp_b = g["a_boxes_out"][i, :n].copy()
        exp_b[:, [0, 2]] = exp_b[:, [0, 2]] * scale
        exp_b[:, [1, 3]] = exp_b[:, [1, 3]] * scale
        assert boxes.shape == (1, n, 4) and boxes.dtype == torch.float32 and cls.shape == (1, n) and cls.dtype == torch.int64
        np.testing.assert_array_equal(boxes[0].cpu().numpy(), exp_b)
        np.testing.assert_array_equal(cls[0].cpu().numpy(), classes)
        H, W = pad32(nh), pad32(nw)
        assert imgs.shape == (1, 3, H, W)
        e = A.fused_planar(raw, nh, nw, H, W, MEAN, STD, flip=p.flip, chain=list(p.chain), d=p.d, crop=p.crop)
        np.testing.assert_array_equal(imgs[0].cpu().numpy(), e, err_msg=f"row {i}")
        seen.add((p.flip, bool(p.chain), p.d != 0.0, p.crop is not None))
    assert len(seen) >= 12, seen


def test_collate_train_raw_batch_padding_and_plain_collate():
    rng = np.random.default_rng(10)
    sizes = [(60, 80), (80, 60), (75, 100), (37, 53)]
    raws = [rand_img(rng, h, w) for h, w in sizes]
    boxes = [np.array([[5, 6, 30, 40], [20, 10, 60, 44], [1, 1, 9, 9]], np.float32), np.zeros((0, 4), np.float32),
             np.array([[10, 10, 50, 60]], np.float32), np.array([[0, 0, 52, 36], [3, 3, 20, 20]], np.float32)]
    classes = [np.array([1, 2, 3]), np.array([], np.int64), np.array([7]), np.array([4, 5])]
    rs = (96, 160)
    r1, r2 = random.Random(77), random.Random(77)
    imgs, bb, cc, params = collate_train_raw([dev(r) for r in raws], [b.copy() for b in boxes], classes, rs, rng=r1, return_params=True)
    exp_params, exp_boxes, dsts = [], [], []
    for (h, w), b in zip(sizes, boxes):
        p, ob = sample_params(h, w, b.copy(), r2)
        scale, nh, nw = resize_rule(p.out_hw[0], p.out_hw[1], rs)
        ob[:, [0, 2]] = ob[:, [0, 2]] * scale
        ob[:, [1, 3]] = ob[:, [1, 3]] * scale
        exp_params.append(p), exp_boxes.append(ob), dsts.append((nh, nw))
    assert params == exp_params and r1.random() == r2.random()
    H, W = max(pad32(a) for a, _ in dsts), max(pad32(b) for _, b in dsts)
    assert imgs.shape == (4, 3, H, W) and bb.shape == (4, 3, 4) and cc.shape == (4, 3)
    bbn, ccn, im = bb.cpu().numpy(), cc.cpu().numpy(), imgs.cpu().numpy()
    for n in range(4):
        k = len(classes[n])
        np.testing.assert_array_equal(bbn[n, :k], exp_boxes[n])
        np.testing.assert_array_equal(ccn[n, :k], classes[n])
        assert (bbn[n, k:] == -1).all() and (ccn[n, k:] == -1).all()
        p = exp_params[n]
        np.testing.assert_array_equal(im[n], A.fused_planar(raws[n], dsts[n][0], dsts[n][1], H, W, MEAN, STD, flip=p.flip, chain=list(p.chain), d=p.d, crop=p.crop))
    # the plain training collate: no rng needed, equals the evaluation-side launch on the same images
    imgs0, bb0, cc0 = collate_train_raw([dev(r) for r in raws], boxes, classes, rs, rng=None, augment=False, flip_p=0)
    rules = [resize_rule(h, w, rs) for h, w in sizes]
    H0, W0 = max(pad32(r[1]) for r in rules), max(pad32(r[2]) for r in rules)
    exp, _ = ops.resize_collate_u8([dev(r) for r in raws], [(r[1], r[2]) for r in rules], H0, W0, MEAN, STD)
    assert torch.equal(imgs0, exp.view(4, H0, W0, 4)[..., :3].permute(0, 3, 1, 2).contiguous())
    np.testing.assert_array_equal(bb0[0].cpu().numpy(), boxes[0] * np.float32(rules[0][0]))


def test_rejections_launch_nothing():
    img = torch.full((8, 9, 3), 3, dtype=torch.uint8, device=DEV)
    out = torch.full((2, 3, 32, 32), 7.0, device=DEV)
    ok = dict(nh=8, nw=9)
    for t in [img.cpu(), img.float(), img[0], img[:, :, :2], torch.zeros(0, 9, 3, dtype=torch.uint8, device=DEV), img.permute(1, 0, 2)]:
        with pytest.raises(FdError):
            ops.rotate_u8(t, 5.0)
        with pytest.raises(FdError):
            ops.color_jitter_u8(t, [(B, 1.1)])
        with pytest.raises(FdError):
            ops.augment_resize_collate_u8([img, t], [ok, ok], 32, 32, MEAN, STD, out=out)
        with pytest.raises(FdError):
            collate_train_raw([img, t], [np.zeros((0, 4), np.float32)] * 2, [[], []], (32, 32), rng=random.Random(0))
    five = [(B, 1.0), (C_, 1.0), (S, 1.0), (HUE, 0), (B, 1.0)]
    for bad in [dict(crop=(0, 0, 10, 8)), dict(crop=(2, 2, 8, 6)), dict(nh=33, nw=9), dict(nh=8, nw=33), dict(nh=0, nw=9), dict(chain=five),
                dict(d=90.0), dict(d=-95.0), dict(chain=[(9, 1.0)])]:
        with pytest.raises(FdError):
            ops.augment_resize_collate_u8([img, img], [ok, dict(ok, **bad)], 32, 32, MEAN, STD, out=out)
    with pytest.raises(FdError):
        ops.augment_resize_collate_u8([img], [ok, ok], 32, 32, MEAN, STD)
    with pytest.raises(FdError):
        ops.augment_resize_collate_u8([], [], 32, 32, MEAN, STD)
    with pytest.raises(FdError):
        ops.augment_resize_collate_u8([img, img], [ok, ok], 32, 32, MEAN, STD, out=out.flatten()[:-1])
    with pytest.raises(FdError):
        ops.color_jitter_u8(img, five)
    for d in (90.0, -90.0, 180.0, float("nan")):
        with pytest.raises(FdError):
            ops.rotate_u8(img, d)
    wide = torch.zeros(1, ops.AUG_MAX_ROT_SIDE + 1, 3, dtype=torch.uint8, device=DEV)          # a side above the limit of the rotation path
    with pytest.raises(FdError):
        ops.rotate_u8(wide, 5.0)
    with pytest.raises(FdError):
        ops.augment_resize_collate_u8([wide], [dict(d=5.0, crop=(0, 0, 9, 1), nh=1, nw=9)], 32, 32, MEAN, STD, out=out[:1])
    with pytest.raises(FdError):
        collate_train_raw([img], [np.zeros((2, 4), np.float32)], [[1]], (32, 32), rng=random.Random(0))
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (img == 3).all()          # nothing was launched on the buffers handed in


def test_one_training_step_from_raw_images():
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(3)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV)
    model.train()
    rng = np.random.default_rng(12)
    sizes = [(120, 160), (160, 120)]
    raws = [dev(rand_img(rng, h, w)) for h, w in sizes]
    boxes = [np.array([[10, 12, 90, 100], [30, 30, 150, 110]], np.float32), np.array([[20, 40, 100, 140]], np.float32)]
    classes = [np.array([3, 7]), np.array([11])]
    imgs, bb, cc = collate_train_raw(raws, boxes, classes, (128, 192), rng=random.Random(5))
    assert imgs.shape[0] == 2 and imgs.shape[2] % 32 == 0 and imgs.shape[3] % 32 == 0
    strides, ranges = [8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]]
    out = model(imgs)
    target = FCOSGenTargets(strides, ranges)([out, bb, cc])
    losses = FCOSLoss("giou")([out, target])
    vals = [float(v.detach()) for v in losses]
    print("losses:", vals)
    assert all(np.isfinite(v) for v in vals) and vals[-1] > 0
    losses[-1].backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 50 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
