"""GPU checks of mosaic (csrc/fd_augment.hip: fd_mosaic_collate_u8; ops.mosaic_collate_u8; data.augment.collate_train_mosaic;
DESIGN §4.2i).  Every comparison is bit for bit: integers and correctly rounded fp32 only.  The checker is the numpy restatement
(tests/mosaic_ref.py); the cases are those of tests/mosaic_cases.py, whose coverage tests/test_mosaic_cpu.py shows."""
import ctypes
import random

import numpy as np
import pytest
import torch

import mosaic_cases as MC
import mosaic_ref as M
from pytorch_object_detection_amd import _lib, ops
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.data.augment import collate_train_mosaic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = MC.MEAN, MC.STD
GUARD = 4096


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def srcs():
    raws = MC.sources()
    return raws, [dev(r) for r in raws]


def guarded(N, H, W, poison=-7.0):
    """An output of N * 3 * H * W floats with GUARD poisoned floats on either side."""
    buf = torch.full((N * 3 * H * W + 2 * GUARD,), poison, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + N * 3 * H * W]


def assert_guards(buf, poison=-7.0):
    assert bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all()), "guard floats around y were written"


@pytest.mark.parametrize("k", [0, 1, 2])
def test_kernel_equals_restatement(srcs, k):
    raws, images = srcs
    H, W, centres, tiles = MC.kernel_case(k)
    fill = (114, 114, 114) if k == 1 else (0, 0, 0)
    # what the case holds: centres on 0 / 1 / side - 1 / side and inside, tiles short of the centre, larger than the quadrant, negative offsets
    assert {c[0] for c in centres} >= {0, 1, W - 1, W} and {c[1] for c in centres} >= {0, 1, H - 1, H}
    flat = [q for quad in tiles for q in quad]
    assert any(q["px"] < 0 for q in flat) and any(q["py"] < 0 for q in flat) and any(q["nh"] > H and q["nw"] > W for q in flat)
    assert any(q["flip"] for q in flat) and any(q["d"] != 0 for q in flat) and any(q["crop"] for q in flat)
    assert {op for q in flat for op, _ in q["chain"]} == {1, 2, 3, 4}
    assert all(len({(str(q["chain"]), n) for n, quad in enumerate(tiles) for q in quad if q["src"] == s}) >= 3 for s in range(5))    # sources repeat
    buf, out = guarded(5, H, W)
    got, keep = ops.mosaic_collate_u8(images, tiles, centres, H, W, MEAN, STD, fill=fill, out=out)
    assert got.shape == (5, 3, H, W) and got.data_ptr() == out.data_ptr() and keep[1] is not None          # the L-sum launch ran (4N records)
    g = got.cpu().numpy()
    assert_guards(buf)
    shown = 0
    for n in range(5):
        e = M.mosaic_planar(raws, tiles[n], centres[n], H, W, MEAN, STD, fill)
        bad = int((g[n].view(np.uint32) != e.view(np.uint32)).sum())
        print(f"canvas {H}x{W} output {n} centre {centres[n]}: {bad} differing values")
        np.testing.assert_array_equal(g[n].view(np.uint32), e.view(np.uint32), err_msg=f"output {n}")
        lv = M.mosaic_levels(raws, [dict(q, chain=[], d=0.0, crop=None, flip=False, src=0) for q in tiles[n]], centres[n], H, W, (1, 2, 3))
        shown += int((lv == (1, 2, 3)).all(-1).sum())
    assert shown > 0, "no fill pixel shows in this case"


def test_one_output_grey_fill_and_contrast_free_records(srcs):
    raws, images = srcs
    H, W = 32, 32
    tiles = [[dict(src=2, px=-20, py=-3, nh=21, nw=30, flip=True, d=-4.0), dict(src=1, px=19, py=2, nh=5, nw=4), dict(src=4, px=1, py=15, nh=64, nw=5, crop=(5, 6, 7, 50)),
              dict(src=0, px=12, py=14, nh=3, nw=25, chain=[(ops.AUG_OP_HUE, 77)])]]
    buf, out = guarded(1, H, W)
    got, keep = ops.mosaic_collate_u8(images, tiles, [(10, 14)], H, W, MEAN, STD, fill=(114, 114, 114), out=out)
    assert keep[1] is None                                   # no contrast: the L-sum launch is skipped
    full = [dict(dict(flip=False, chain=[], d=0.0, crop=None), **q) for q in tiles[0]]
    e = M.mosaic_planar(raws, full, (10, 14), H, W, MEAN, STD, (114, 114, 114))
    np.testing.assert_array_equal(got[0].cpu().numpy().view(np.uint32), e.view(np.uint32))
    assert_guards(buf)


def test_degenerate_centre_equals_the_fused_launch(srcs):
    raws, images = srcs
    H, W = 64, 96
    other = dict(src=0, px=-3, py=5, nh=20, nw=20, flip=True, chain=MC.CHAINS[1], d=5.0)
    cases = [(2, dict(flip=True, chain=MC.CHAINS[1], d=7.3, crop=(3, 5, 42, 28), nh=50, nw=77)), (3, dict(nh=64, nw=52)),
             (1, dict(chain=MC.CHAINS[2], d=-10.0, crop=(1, 1, 3, 4), nh=64, nw=96)), (0, dict(flip=True, nh=1, nw=1)), (4, dict(chain=MC.CHAINS[4], nh=33, nw=95))]
    exp, _ = ops.augment_resize_collate_u8([images[s] for s, _ in cases], [kw for _, kw in cases], H, W, MEAN, STD)
    tiles = [[other, other, other, dict(kw, src=s, px=0, py=0)] for s, kw in cases]
    got, _ = ops.mosaic_collate_u8(images, tiles, [(0, 0)] * len(cases), H, W, MEAN, STD)
    assert torch.equal(got, exp)


def test_raw_tables_any_placement_word_is_safe_and_bad_sizes_give_fill(srcs):
    """The C entry point on hand-built tables, as a caller without the Python validation could hand them over: extreme centres
    and offsets, records with zero or negative sizes (fill), and a record that UNDERSTATES its source (fewer rows than the
    buffer holds; no record here claims more pixels than its buffer has)."""
    raws, images = srcs
    H, W, N = 32, 32, 3
    big, small = 2 ** 31 - 1, -2 ** 31
    ok = ops.augment_record(37, 53, nh=20, nw=30)
    under = ops.augment_record(20, 53, nh=20, nw=30, flip=True)                 # rows 0 .. 19 of the 37 x 53 buffer
    zero_h, neg_nw, zero_crop = list(ok), list(ok), list(ok)
    zero_h[0] = 0
    neg_nw[15] = -4
    zero_crop[12] = 0
    recs = [ok, under, ok, ok, zero_h, neg_nw, zero_crop, under, ok, ok, under, ok]
    place = [[big, small, 0x00302010, small, 0, 0, 0, small, small, 0, 0, 0],         # all pixels: tile 2, lx beyond any width: fill
             [16, 16, 0x00090807, 0, 0, 16, 0, 0, 16, 16, 16, 0],                     # three records of no size, then the understated one
             [-5, big, 0x00010203, 0, 0, 2, 3, big, big, small, small, 0]]            # all pixels: tile 1
    ptrs = torch.tensor([images[2].data_ptr()] * 12, dtype=torch.int64).to(DEV)
    recs_dev = torch.tensor(recs, dtype=torch.int32).to(DEV)
    place_dev = torch.from_numpy(np.array(place, np.int64).astype(np.int32)).to(DEV)
    buf, out = guarded(N, H, W)
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    _lib.check(_lib.lib().fd_mosaic_collate_u8(ptrs.data_ptr(), recs_dev.data_ptr(), place_dev.data_ptr(), out.data_ptr(), N, H, W, m3, s3,
                                               torch.cuda.current_stream().cuda_stream), "fd_mosaic_collate_u8")
    g = out.view(N, 3, H, W).cpu().numpy()
    assert_guards(buf)
    norm = lambda lv: M.resize_ref.normalise(lv, MEAN, STD)[..., :3].transpose(2, 0, 1)      # noqa: E731
    e0 = np.empty((H, W, 3), np.uint8)
    e0[...] = (0x10, 0x20, 0x30)
    np.testing.assert_array_equal(g[0], norm(e0))
    e1 = np.empty((H, W, 3), np.uint8)
    e1[...] = (7, 8, 9)
    e1[16:, 16:] = M.A.fused_levels(raws[2][:20], 20, 30, 20, 30, flip=True)[:16, :16]
    np.testing.assert_array_equal(g[1], norm(e1))
    e2 = np.empty((H, W, 3), np.uint8)
    e2[...] = (3, 2, 1)
    e2[3:23, 2:32] = M.A.fused_levels(raws[2], 20, 30, 20, 30)
    np.testing.assert_array_equal(g[2], norm(e2))


@pytest.mark.parametrize("case", range(len(MC.COLLATE_CASES)))
def test_collate_train_mosaic_equals_restatement(case):
    seed, kw = MC.COLLATE_CASES[case]
    raws, boxes, classes = MC.batch()
    images = [dev(r) for r in raws]
    sizes, H, W = MC.BATCH_SIZES, 64, 96
    imgs, bb, cc, params = collate_train_mosaic(images, [b.copy() for b in boxes], classes, (H, W), rng=random.Random(seed), return_params=True, **kw)
    again = collate_train_mosaic(images, [b.copy() for b in boxes], classes, (H, W), rng=random.Random(seed), **kw)
    assert torch.equal(imgs, again[0]) and torch.equal(bb, again[1]) and torch.equal(cc, again[2])          # equally seeded: equal
    assert imgs.shape == (5, 3, H, W) and imgs.dtype == torch.float32 and bb.dtype == torch.float32 and cc.dtype == torch.int64
    rng = random.Random(seed)
    eb, ec = [], []
    g = imgs.cpu().numpy()
    fill = kw.get("fill", (0, 0, 0))
    for n in range(5):
        e = MC.replay(sizes, boxes, n, H, W, rng, group=None if "groups" not in kw else kw["groups"][n])
        p = params[n]
        assert p.centre == e["centre"] and p.sources == e["sources"] and list(p.tiles) == e["tiles"] and list(p.gains) == e["gains"]
        assert list(p.placements) == e["placements"] and list(p.sizes) == e["sizes"]
        inputs = [(e["aug_boxes"][t], classes[p.sources[t]], e["scales"][t], *p.placements[t], *e["sizes"][t]) for t in range(4)]
        b, c, _ = M.output_boxes(inputs, p.centre, H, W, min_visible=kw.get("min_visible", 0.2))
        eb.append(b), ec.append(c)
        exp = M.mosaic_planar(raws, MC.tile_dicts(p), p.centre, H, W, MEAN, STD, fill)
        np.testing.assert_array_equal(g[n].view(np.uint32), exp.view(np.uint32), err_msg=f"output {n}")
    pb, pc = M.pad_batch(eb, ec)
    print(f"seed {seed}: boxes per output {[b.shape[0] for b in eb]}")
    assert min(b.shape[0] for b in eb) < pb.shape[1], "no padding row in this case"
    np.testing.assert_array_equal(bb.cpu().numpy().view(np.uint32), pb.view(np.uint32))                     # padding rows are -1
    np.testing.assert_array_equal(cc.cpu().numpy(), pc)


def test_collate_train_mosaic_without_any_box_returns_the_empties():
    raws, _, _ = MC.batch()
    images = [dev(r) for r in raws]
    none, nocls = [np.zeros((0, 4), np.float32)] * 5, [np.zeros(0, np.int64)] * 5
    imgs, bb, cc = collate_train_mosaic(images, none, nocls, (32, 64), rng=random.Random(2))
    assert imgs.shape == (5, 3, 32, 64) and bb.shape == (5, 0, 4) and bb.dtype == torch.float32 and cc.shape == (5, 0) and cc.dtype == torch.int64
    assert bb.is_cuda and cc.is_cuda
    # boxes that all fall away (degenerate) give the same empties
    deg = [np.array([[3, 3, 3, 9]], np.float32)] * 5
    _, bb, cc = collate_train_mosaic(images, deg, [np.array([4])] * 5, (32, 64), rng=random.Random(2))
    assert bb.shape == (5, 0, 4) and cc.shape == (5, 0)


def test_refusals_launch_nothing(srcs):
    _, images = srcs
    img = images[1]
    out = torch.full((2, 3, 32, 32), 7.0, device=DEV)
    tile = dict(src=1, px=0, py=0, nh=8, nw=9)
    quad = [tile] * 4

    def refused(imgs=images, tiles=(quad, quad), centres=((4, 4), (5, 5)), H=32, W=32, std=STD, **kw):
        with pytest.raises(FdError):
            ops.mosaic_collate_u8(list(imgs), [list(q) for q in tiles], list(centres), H, W, MEAN, std, out=kw.pop("out", out), **kw)

    for t in [img.cpu(), img.float(), img[0], img[:, :, :2], torch.zeros(0, 9, 3, dtype=torch.uint8, device=DEV), img.permute(1, 0, 2)]:
        refused(imgs=[images[0], t])
    for bad in (dict(px=65537), dict(py=-65537), dict(src=5), dict(src=-1), dict(nh=0), dict(nw=65537), dict(crop=(0, 0, 10, 8)), dict(d=90.0),
                dict(chain=[(9, 1.0)]), dict(chain=[(1, 1.0), (2, 1.0), (3, 1.0), (4, 0), (1, 1.0)])):
        refused(tiles=(quad, [tile, tile, tile, dict(tile, **bad)]))
    for c in ((-1, 4), (4, -1), (33, 4), (4, 33)):
        refused(centres=((4, 4), c))
    refused(centres=((4, 4),))
    refused(tiles=(quad, [tile] * 3))
    refused(std=(0.229, 0.0, 0.225))
    refused(fill=(0, 0, 256))
    refused(H=64)                                             # out does not hold 2 * 3 * 64 * 32
    refused(out=out.flatten()[:-1])
    refused(out=out.double())
    refused(out=out.cpu())
    refused(out=out.permute(0, 1, 3, 2))
    # the C entry point itself, with real buffers behind the pointers
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    ptrs = torch.tensor([img.data_ptr()] * 8, dtype=torch.int64).to(DEV)
    recs = torch.tensor([ops.augment_record(7, 5)] * 8, dtype=torch.int32).to(DEV)
    place = torch.zeros(2, ops.MOSAIC_WORDS, dtype=torch.int32, device=DEV)
    m3, s3, z3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD), (ctypes.c_float * 3)(0.2, 0.0, 0.2)
    ok = [ptrs.data_ptr(), recs.data_ptr(), place.data_ptr(), out.data_ptr(), 2, 32, 32, m3, s3, st]
    for i, v in [(0, None), (1, None), (2, None), (3, None), (7, None), (8, None), (3, out.data_ptr() + 2), (1, recs.data_ptr() + 1), (2, place.data_ptr() + 2),
                 (0, ptrs.data_ptr() + 4), (4, 0), (4, -2), (4, 16384), (5, 0), (6, -1), (5, 65537), (8, z3)]:
        a = list(ok)
        a[i] = v
        assert lib.fd_mosaic_collate_u8(*a) == _lib.E_INVAL, (i, v)
    a = list(ok)
    a[5], a[6] = 65536, 32768
    assert lib.fd_mosaic_collate_u8(*a) == _lib.E_INVAL
    for size in ((64, 72), (40, 64)):
        with pytest.raises(FdError):
            collate_train_mosaic([img], [np.zeros((0, 4), np.float32)], [[]], out_size=size, rng=random.Random(0))
    with pytest.raises(FdError):
        collate_train_mosaic([img], [np.zeros((2, 4), np.float32)], [[1]], out_size=(32, 32), rng=random.Random(0))
    with pytest.raises(FdError):
        collate_train_mosaic([img, img.cpu()], [np.zeros((0, 4), np.float32)] * 2, [[], []], out_size=(32, 32), rng=random.Random(0))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == dev(MC.sources()[1])).all())        # nothing was launched on the buffers handed in


def test_one_training_step_from_a_mosaic_batch():
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(3)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(DEV)
    model.train()
    rng = np.random.default_rng(12)
    sizes = [(120, 160), (160, 120)]
    raws = [dev(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
    boxes = [np.array([[10, 12, 90, 100], [30, 30, 150, 110]], np.float32), np.array([[20, 40, 100, 140]], np.float32)]
    classes = [np.array([3, 7]), np.array([11])]
    imgs, bb, cc = collate_train_mosaic(raws, boxes, classes, (128, 192), rng=random.Random(5), fill=(114, 114, 114))
    assert imgs.shape == (2, 3, 128, 192) and bb.shape[1] >= 1
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
