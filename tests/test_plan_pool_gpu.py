"""The plan's buffer pool under poison (tests/plan_poison.py): every shipped plan builder must give, bit for bit, the outputs of its
uninstrumented plan while every buffer the pool has back -- and every torch.empty workspace -- holds NaN until its next owner writes it.

engine.Pool's contract is "a buffer is put only after the plan.add of its last reader".  A put one line too early only shows where best
fit hands the buffer to a layer planned in between, which depends on batch, image size, class count, precision and kernel family; under
poison it shows at every shape.  The same run catches a kernel that reads part of a pooled output nobody wrote, a workspace whose first
use depends on its content, and a workspace that a run does not leave reusable (run 2 against run 1).  The bar is torch.equal against the
plain plan of the same commit (same kernels, same order): no tolerance.  A NaN scan would not do -- a ReLU or max-pool epilogue turns a
poisoned operand into a clean-looking zero.

Which builder branches each configuration is there for (the plan.names / plan.tiles assertions below pin them):

  HISFCOS 2x128x128, 1x160x224 (odd 5x7 C5, 1x1 top level)
    f32              res_up-fused laterals (fpn.tf2+up1_add), GroupNorm folded into its neighbours (head.gn1.stats: the rgs1 / rgs2 row
                     statistics buffers), split-K Winograd F(2x2) scratch taken and handed straight back (layer3, the FPN, the tower),
                     conv3+downsample dual-source launches, the 8-wide cnt_reg buffer
    f16x3            unfused upsample-add (fpn.tf2 + fpn.up1_add), the three-pass GroupNorms (head.gn1 / head.gn2), the generic stem with its
                     own max-pool step (y1), the direct kernel's split-K scratch on every layer
    mixed            GroupNorm folded, unfused upsample-add
    f32 WINO force   Winograd F(2x2) without split on every 3x3 stride-1 layer, tiny levels included
    f32 WINO + WINO4 force   F(4x4) on every dilation-1 3x3 stride-1 layer (whole-float4 stores on ragged tiles), plan.sk_ws allocated
    f32 WINO4 = "0"  the F(2x2)-only plan
    f32 GN_FUSED off the three-pass GroupNorms on the exact-fp32 plan
    f32 W4_SK off    no persistent launches, no sk workspace
    f32 B2B_MIN_ROWS = 1     the back-to-back conv3 + conv1 launch of layer1 and its o1_ready hand-over (.conv3+layer1.)
    f32 + persistent F(4x4)  (WINO + WINO4 force, the persistent stream-K form put on the pyramid-wide head layers): the flag header
                     every launch must leave zero, the NaN body of the workspace.  The shipped table holds that form for the
                     16x640x640 layers only, so wino4_sk_choice is replaced to reach it at a small shape.
  HISFCOS 26x128x128 f32     the narrow predictor (130 tiles of 16x16 >= NARROW_MIN_TILES): head.tower_gn.stats, the box half normalised in
                     the predictor's loader; split-K F(4x4) on HisBlock conv4
  FCOS-R50 f32 / f16x3       build_fcos_fpn (levels written in place, P6 / P7 strided convs), build_fcos_head's buffer ring
  FCOS EfficientNet-B3 / B0  build_efficientnet with keep = (2, 3, 4): the fused expand + depthwise launch with its pooling partials, SE
                     workspaces, endpoints 0 / 1 released, widths 48 / 136 / 40 / 112 that are no multiple of 32
  EfficientNetV1(3), (0)     keep = all five endpoints
  MNFCOS, MNBlock (3, 1), (5, 2)   build_mn_fpn / build_mn_head / add_mn_block; MNBlock.forward stages its input outside the plan
  input paths      add_input's u8 / collate / resize modes (x4 taken and released), add_postprocess appended to a built plan, capture_graph
  stand-alone FPN / head plans     _run_fpn / _run_head staging from outside the plan; padded_input's pooled (C % 4 == 0) and dedicated branch
  TwoLanePipeline  two slot plans built under poison, steps cut at a mark and interleaved on two streams

Not reached at a small shape: the persistent stream-K launch as the SHIPPED rule picks it (table hits exist for 16x640x640 only; see above),
and the head tower's whole-rounds + tail split (add_conv: needs >= 4 * CU count workgroups, i.e. the 16x640x640 tower).  Neither takes or
releases a pool buffer."""
import os

import pytest
import torch

from pytorch_object_detection_amd import _lib, engine, ops
from pytorch_object_detection_amd._lib import Segs
from pytorch_object_detection_amd.model.backbone.efficientnetv1 import EfficientNetV1
from pytorch_object_detection_amd.model.modules.head import ClipBoxes, FCOSHead
from pytorch_object_detection_amd.model.modules.modules import MNBlock
from pytorch_object_detection_amd.model.od import FCOS, HalfInvertedStageFCOS
from pytorch_object_detection_amd.model.od.Fcos import FeaturePyramidNetwork
from pytorch_object_detection_amd.model.od.HISFcos import HalfInvertedStageFPN
from pytorch_object_detection_amd.model.od.MNFcos import MNFCOS, LieghtWeightFeaturePyramid_old
from effnet_init import init_effnet
from plan_poison import POISON_STEP, poisoned_pool
from test_model_gpu import randomize_norms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRIDES = [8, 16, 32, 64, 128]


def flat(out):
    """(cls, cnt, reg) lists -> one tuple of tensors."""
    return tuple(t for grp in out for t in grp)


def clones(ts):
    return [t.clone() for t in ts]


def same(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: output {i} differs ({int((u != v).sum())} of {u.numel()} values)"


# ------------------------------------------------------------------------------------------------ a. the pool and the instrument
def test_pool_best_fit_total_and_reuse():
    pool = engine.Pool(DEV)
    a, b, c = pool.get(100, 4), pool.get(50, 4), pool.get(25, 4)
    assert pool.total == (400 + 200 + 100) * 4 and pool.free == []
    for r in (a, b, c):
        pool.put(r)
    g = pool.get(30, 4)                       # 120 floats: 200 is the smallest flat that holds them
    assert g._flat is b._flat and tuple(g.buf.shape) == (30, 4) and g.buf.data_ptr() == b._flat.data_ptr()
    h = pool.get(10, 4)
    assert h._flat is c._flat
    k = pool.get(100, 4)                      # exactly a's size
    assert k._flat is a._flat and pool.total == 700 * 4 and pool.free == []
    big = pool.get(1000, 4)                   # nothing is free: an allocation
    pool.put(k)
    big2 = pool.get(101, 4)                   # 404 floats, larger than every free flat (a's 400): an allocation too
    assert big2._flat is not a._flat and pool.total == (700 + 4000 + 404) * 4       # total counts allocations only
    pool.put(big)
    again = pool.get(1000, 4)                 # put, then get of the same size: the same storage
    assert again._flat is big._flat and again.buf.data_ptr() == big.buf.data_ptr() and pool.total == (700 + 4000 + 404) * 4


def toy_plan(early: bool):
    """Plain torch steps on pool buffers: a = src; b = 2a; c = b + 1 (c reuses a's flat); d = 3 c[:16] (d reuses b's flat).  `early` puts b
    BEFORE its reader is added -- after c was got, so that no layer planned in between receives it: invisible without the instrument."""
    plan = engine.Plan(DEV)
    pool = plan.pool
    src = torch.arange(64 * 8, dtype=torch.float32, device=DEV).view(64, 8)
    a = pool.get(64, 8)
    plan.add("load", lambda: a.buf.copy_(src))
    b = pool.get(64, 8)
    plan.add("double", lambda: torch.mul(a.buf, 2.0, out=b.buf))
    pool.put(a)
    c = pool.get(64, 8)
    assert c._flat is a._flat
    if early:
        pool.put(b)
    plan.add("plus1", lambda: torch.add(b.buf, 1.0, out=c.buf))
    if not early:
        pool.put(b)
    d = pool.get(16, 8)
    assert d._flat is b._flat
    plan.add("triple", lambda: torch.mul(c.buf[:16], 3.0, out=d.buf))
    return plan, (c, d)


def run_toy(early: bool):
    plan, outs = toy_plan(early)
    plan.run()
    first = [o.buf.clone() for o in outs]
    plan.run()
    second = [o.buf.clone() for o in outs]
    assert all(torch.equal(u, v) or bool((torch.isnan(u) == torch.isnan(v)).all()) for u, v in zip(first, second))
    return plan, first


def test_instrument_is_silent_on_a_correct_plan_and_flags_an_early_put():
    _, good = run_toy(False)
    src = torch.arange(64 * 8, dtype=torch.float32, device=DEV).view(64, 8)
    assert torch.equal(good[0], 2 * src + 1) and torch.equal(good[1], 3 * (2 * src[:16] + 1))
    _, hidden = run_toy(True)
    same(hidden, good, "early put without the instrument (the gap this file closes)")
    with poisoned_pool() as pp:
        plan, got = run_toy(False)
        same(got, good, "correct toy plan under poison")
        assert pp.poison_steps(plan) == 2 and pp.free_duplicates(plan) == [] and pp.out_shapes(plan) == [(16, 8), (64, 8)]
        assert [o.fresh for o in pp.still_out(plan)] == [False, False] and pp.total(plan) == 2 * 64 * 8 * 4
        _, bad = run_toy(True)
        assert not torch.equal(bad[0], good[0]) and bool(torch.isnan(bad[0]).all())
    assert len(pp.plans) == 2


def test_instrument_raises_at_build_time_on_a_double_or_foreign_put():
    with poisoned_pool():
        plan = engine.Plan(DEV)
        a = plan.pool.get(8, 4)
        plan.pool.put(a)
        with pytest.raises(AssertionError, match="not out"):
            plan.pool.put(a)
        other = engine.Plan(DEV).pool.get(8, 4)
        with pytest.raises(AssertionError, match="not out"):
            plan.pool.put(other)
        # a flat that reached the free list twice behind the instrument's back is caught when it is handed out the second time
        plan.pool.free.append(plan.pool.free[0])
        assert len(plan.pool.free) == 2
        plan.pool.get(8, 4)
        with pytest.raises(AssertionError, match="free list twice"):
            plan.pool.get(8, 4)


def test_instrument_fills_eagerly_and_restores_what_it_patched():
    before = (engine.Plan.__init__, engine.Pool.get, engine.Pool.put, engine.padded_input, ops.groupnorm_workspace, ops.se_workspace,
              ops.mbconv_pool_buffer, ops.sk_workspace)
    with poisoned_pool():
        plan = engine.Plan(DEV)
        a = plan.pool.get(8, 4)
        assert bool(torch.isnan(a._flat).all()) and plan.steps == []        # at build time, not as a step
        a.buf.fill_(1.0)
        plan.pool.put(a)
        assert plan.names == [POISON_STEP] and bool((a._flat == 1.0).all())  # the release poison IS a step ...
        b = plan.pool.get(4, 4)
        assert b._flat is a._flat and bool((a._flat == 1.0).all())           # ... and a reused flat is not filled at build time
        plan.run()
        assert bool(torch.isnan(a._flat).all())                              # the whole flat, not only the [:need] view
        segs = Segs.make(2, [(4, 4), (2, 2)])
        assert bool(torch.isnan(ops.groupnorm_workspace(segs, 32, DEV)).all()) and bool(torch.isnan(ops.se_workspace(2, 16, 64, DEV)).all())
        sk = ops.sk_workspace(256, DEV)
        assert int(sk[:2048].view(torch.int32).abs().sum()) == 0 and bool(torch.isnan(sk[2048:]).all())
    after = (engine.Plan.__init__, engine.Pool.get, engine.Pool.put, engine.padded_input, ops.groupnorm_workspace, ops.se_workspace,
             ops.mbconv_pool_buffer, ops.sk_workspace)
    assert all(x is y for x, y in zip(before, after))
    with pytest.raises(ValueError):
        with poisoned_pool():
            raise ValueError("restored on an exception too")
    assert engine.Pool.get is before[1]


# ------------------------------------------------------------------------------------------------ b. every shipped plan under poison
def check(run, owners=(), kept=None, plans=1, what=""):
    """run() -> tuple of output tensors of one forward.  Plain twice (run 2 bitwise equal to run 1: nothing left behind in a workspace; all
    finite), then twice under poisoned_pool(): bitwise equal to the plain result.  After the build: no duplicate on the free list, and the
    buffers still out are exactly kept(plan) (sorted (rows, C) pairs).  Leaves no plan cached.  Returns the session."""
    def drop():
        for m in owners:
            m.invalidate_plans()
    drop()
    try:
        with torch.no_grad():
            ref = clones(run())
            again = clones(run())
        same(again, ref, what + " plain run 2 vs run 1")
        assert all(bool(torch.isfinite(t).all()) for t in ref), what + ": non-finite plain output"
        drop()
        with poisoned_pool() as pp, torch.no_grad():
            got1 = clones(run())
            got2 = clones(run())
            torch.cuda.synchronize()
        same(got1, ref, what + " under poison, run 1")
        same(got2, ref, what + " under poison, run 2")
        assert len(pp.plans) == plans, (len(pp.plans), plans)
        for plan in pp.plans:
            assert pp.free_duplicates(plan) == []
            assert pp.poison_steps(plan) > 0
            if kept is not None:
                assert pp.out_shapes(plan) == sorted(kept(plan)), (pp.out_shapes(plan), sorted(kept(plan)))
    finally:
        drop()
    return pp


def detector_keeps(F: int, ncls: int):
    """What a detector plan holds at the end: the pyramid (its head reads it last), the last tower buffer and the two predictor buffers the
    outputs are views of (the class map padded to 4 channels, centre-ness + box in an 8-wide one)."""
    def kept(plan):
        M = plan.segs.rows
        return [(M, F), (M, 2 * F), (M, (ncls + 3) // 4 * 4), (M, 8)]
    return kept


def outputs_are_out(pp, plan):
    out = {o.flat.untyped_storage().data_ptr() for o in pp.still_out(plan)}
    assert all(r.buf.untyped_storage().data_ptr() in out for r in plan.outs)


def wino_split(plan):
    return [n for n, t in plan.tiles.items() if ops.tile_split(t)[0] in (_lib.WINO_TILE, _lib.WINO4_TILE) and ops.tile_split(t)[1] > 1]


def on_tile(plan, tile):
    return [n for n, t in plan.tiles.items() if ops.tile_split(t)[0] == tile]


@pytest.fixture(scope="module")
def his():
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).eval()
    randomize_norms(model, 1)
    return model.to(DEV)


def image(B, H, W, seed=3):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _persistent_everywhere(call, key, ws, reps=5):
    """wino4_sk_choice with the shipped table's entry for the pyramid-wide layers (the head tower, cls_logits, cnt_reg) at any shape."""
    return 256 if ops.W4_SK and "+" in key else 0


# id -> (precision, [(module, attribute, value)], names that must be planned, names that must not)
HIS_CASES = {
    "f32": ("f32", [], ["fpn.tf2+up1_add", "fpn.tf3+up2_add", "head.gn1.stats", "head.gn2.stats"], ["fpn.up1_add", "head.gn1"]),
    "f16x3": ("f16x3", [], ["fpn.tf2", "fpn.up1_add", "fpn.up2_add", "head.gn1", "head.gn2", "backbone.maxpool"], ["fpn.tf2+up1_add", "head.gn1.stats"]),
    "mixed": ("mixed", [], ["fpn.up1_add", "head.gn1.stats"], ["fpn.tf2+up1_add"]),
    "f32-wino": ("f32", [(ops, "WINO_MODE", "force"), (ops, "WINO4_MODE", "0")], ["fpn.tf2+up1_add"], []),
    "f32-wino4": ("f32", [(ops, "WINO_MODE", "force"), (ops, "WINO4_MODE", "force")], ["fpn.tf2+up1_add"], []),
    "f32-no-wino4": ("f32", [(ops, "WINO4_MODE", "0")], ["head.gn1.stats"], []),
    "f32-gn-three-pass": ("f32", [(engine, "GN_FUSED", False)], ["head.gn1", "head.gn2", "fpn.tf2+up1_add"], ["head.gn1.stats"]),
    "f32-no-w4sk": ("f32", [(ops, "W4_SK", False)], ["head.gn1.stats"], []),
    "f32-b2b": ("f32", [(engine, "B2B_MIN_ROWS", 1)], ["head.gn1.stats"], []),
    "f32-persistent-w4": ("f32", [(ops, "WINO_MODE", "force"), (ops, "WINO4_MODE", "force"), (ops, "wino4_sk_choice", _persistent_everywhere)], [], []),
}


@pytest.mark.parametrize("shape", [(2, 128, 128), (1, 160, 224)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", list(HIS_CASES))
def test_hisfcos_under_poison(his, case, shape, monkeypatch):
    prec, knobs, must, must_not = HIS_CASES[case]
    for mod, attr, value in knobs:
        monkeypatch.setattr(mod, attr, value)
    x = image(*shape)
    his.conv_precision = prec
    try:
        pp = check(lambda: flat(his(x)), [his], detector_keeps(256, 20), what=f"HISFCOS {shape} {case}")
    finally:
        his.conv_precision = None
    plan = pp.plans[0]
    outputs_are_out(pp, plan)
    assert [tuple(s) for s in plan.segs.level_hw()][2:] == [(shape[1] // 32, shape[2] // 32), (shape[1] // 64, shape[2] // 64), (shape[1] // 128, shape[2] // 128)]
    for n in must:
        assert n in plan.names, (n, "not planned")
    for n in must_not:
        assert n not in plan.names, (n, "planned")
    if case in ("f32", "mixed", "f32-no-wino4"):
        assert wino_split(plan), "no split-K Winograd launch (its scratch is taken from the pool and handed straight back)"
    if case == "f32-wino":
        assert "head.tower3x3" in on_tile(plan, _lib.WINO_TILE) and not on_tile(plan, _lib.WINO4_TILE) and not wino_split(plan)
    if case in ("f32-wino4", "f32-persistent-w4"):
        assert "head.tower3x3" in on_tile(plan, _lib.WINO4_TILE) and getattr(plan, "sk_ws", None) is not None
    if case == "f32-no-wino4":
        assert not on_tile(plan, _lib.WINO4_TILE)
    if case == "f32-no-w4sk":
        assert not getattr(plan, "sk_of", None)
    if case == "f32-b2b":
        assert any(".conv3+layer1." in n for n in plan.names), "the back-to-back conv3 + conv1 launch was not planned"
    else:
        assert not any(".conv3+layer1." in n for n in plan.names)
    if case == "f32-persistent-w4":
        assert {"head.tower3x3", "head.cls_logits"} <= set(plan.sk_of), plan.sk_of
        assert int(plan.sk_ws[:2048].view(torch.int32).abs().sum()) == 0, "a persistent launch left a flag / queue head non-zero"
    assert any("conv3+downsample" in n for n in plan.names) == (prec == "f32")


def test_hisfcos_narrow_predictor_under_poison(his):
    """26 x 128 x 128: 130 tiles of 16 x 16, the smallest batch at which the vector-unit predictor runs at this image size."""
    x = image(26, 128, 128)
    pp = check(lambda: flat(his(x)), [his], detector_keeps(256, 20), what="HISFCOS 26x128x128")
    plan = pp.plans[0]
    assert "head.tower_gn.stats" in plan.names and "head.tower_gn" in plan.names and on_tile(plan, _lib.NARROW_TILE) == ["head.cnt_reg"]
    assert any(ops.tile_split(plan.tiles[n])[0] == _lib.WINO4_TILE for n in wino_split(plan)), "no split-K F(4x4) launch"


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_fcos_r50_under_poison(prec):
    torch.manual_seed(1)
    model = FCOS([2048, 1024, 512], 80, 256).eval()
    model.conv_precision = prec
    randomize_norms(model, 2)
    with torch.no_grad():
        for m in model.head.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(8.0)
    model.to(DEV)
    x = image(1, 128, 160)
    pp = check(lambda: flat(model(x)), [model], detector_keeps(256, 80), what=f"FCOS-R50 {prec}")
    plan = pp.plans[0]
    outputs_are_out(pp, plan)
    assert "FPN.P5_Up_add" in plan.names and "head.tower3_gn" in plan.names


def _fcos_effnet(widths, ncls, feature, number, seed):
    torch.manual_seed(seed)
    model = FCOS(widths, ncls, feature, efficientnet=True, backbone_number=number).eval()
    init_effnet(model.backbone, seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    for m in model.head.modules():
        if isinstance(m, torch.nn.GroupNorm):
            m.weight.data.copy_(torch.rand(m.num_channels, generator=gen) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_channels, generator=gen) * 0.1)
        if isinstance(m, torch.nn.Conv2d):
            with torch.no_grad():
                m.weight.mul_(8.0)
    return model.to(DEV)


def test_fcos_efficientnet_b3_under_poison():
    model = _fcos_effnet([384, 136, 48], 80, 256, 3, 20)
    x = image(1, 128, 192)
    pp = check(lambda: flat(model(x)), [model], detector_keeps(256, 80), what="FCOS EfficientNet-B3")
    names = pp.plans[0].names
    assert any(n.endswith("._expand+depthwise") for n in names) and any(n.endswith("._expand_conv") for n in names)


def test_fcos_efficientnet_b0_under_poison():
    torch.manual_seed(2)
    model = FCOS([320, 112, 40], 20, 64, efficientnet=True).eval()        # (as the reference constructs it: test_effnet_gpu.py)
    init_effnet(model.backbone, 3)
    model.to(DEV)
    x = image(1, 160, 128)
    check(lambda: flat(model(x)), [model], detector_keeps(64, 20), what="FCOS EfficientNet-B0")


@pytest.mark.parametrize("number,shape", [(3, (1, 128, 192)), (0, (2, 96, 64))])
def test_efficientnet_trunk_alone_under_poison(number, shape):
    """All five endpoints kept: another `keep` set than the detector's (2, 3, 4)."""
    net = EfficientNetV1(number).eval()
    init_effnet(net, 11 + number)
    net.to(DEV)
    x = image(*shape, seed=5)
    pp = check(lambda: tuple(net(x)), [net], lambda plan: [(s.rows, r.C) for r, s in plan.endpoints], what=f"EfficientNetV1({number})")
    assert len(pp.plans[0].endpoints) == 5 and all(e is not None for e in pp.plans[0].endpoints)


@pytest.fixture(scope="module")
def mn(tmp_path_factory):
    """MNFCOS through Builder(load_config(...)), as test_mnfcos_gpu.py constructs it."""
    import pytorch_object_detection_amd as pkg
    from pytorch_object_detection_amd.bulider import Builder, load_config
    cfg_dir = os.path.join(os.path.dirname(pkg.__file__), "config")
    main = tmp_path_factory.mktemp("mn") / "config" / "main.yaml"
    main.parent.mkdir()
    main.write_text(open(os.path.join(cfg_dir, "main.yaml")).read().replace("dataset: COCO", "dataset: VOC").replace("model: HISFCOS", "model: MNFCOS")
                    .replace("config/voc.yaml", os.path.join(cfg_dir, "voc.yaml")))
    cfg = load_config(str(main))
    torch.manual_seed(6)
    model = Builder(cfg).model_build().eval()
    assert isinstance(model, MNFCOS)
    randomize_norms(model, 7)
    with torch.no_grad():
        for m in (model.head.cls_logits, model.head.cnt_logits, model.head.reg_pred):
            m.weight.mul_(3.0)
    return model.to(DEV)


def test_mnfcos_under_poison(mn):
    x = image(2, 128, 128)
    F, ncls = mn.head.cls_logits.weight.shape[1], mn.head.cls_logits.weight.shape[0]
    pp = check(lambda: flat(mn(x)), [mn], detector_keeps(F, ncls), what="MNFCOS")
    assert "FeaturePyramidNetwork.MNB7.PW2" in pp.plans[0].names and "head.block2.PW2" in pp.plans[0].names


@pytest.mark.parametrize("k,d", [(3, 1), (5, 2)])
def test_mn_block_alone_under_poison(k, d):
    """MNBlock.forward builds a plan per call and copies its input into a freshly got buffer outside the plan."""
    torch.manual_seed(k * 10 + d)
    blk = MNBlock(128, 128, k, d, 2).eval()
    randomize_norms(blk, k + d)
    blk.to(DEV)
    x = torch.randn(2, 128, 11, 7, generator=torch.Generator().manual_seed(k)).to(DEV)
    pp = check(lambda: (blk(x),), [], lambda plan: [(2 * 11 * 7, 128)] * 2, plans=2, what=f"MNBlock k={k} d={d}")
    for plan in pp.plans:
        assert all(o.fresh for o in pp.still_out(plan)), "the staged input must be a fresh flat"


# ---- input paths (HISFCOS)
def test_uint8_input_under_poison(his):
    x = torch.randint(0, 256, (2, 128, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
    pp = check(lambda: flat(his(x)), [his], detector_keeps(256, 20), what="uint8 input")
    assert pp.plans[0].names[0] == "input.preprocess_u8"


def _u8_images(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).to(DEV) for h, w in sizes]


def test_forward_images_under_poison(his):
    imgs = _u8_images([(100, 83), (83, 100), (96, 96)], 12)
    pp = check(lambda: flat(his.forward_images(imgs)), [his], detector_keeps(256, 20), what="forward_images")
    assert pp.plans[0].names[0] == "input.collate_u8" and pp.plans[0].canvas_hw == (128, 128)


def test_forward_raw_under_poison(his):
    imgs = _u8_images([(60, 90), (120, 70)], 13)
    pp = check(lambda: flat(his.forward_raw(imgs, (96, 160))), [his], detector_keeps(256, 20), what="forward_raw")
    assert pp.plans[0].names[0] == "input.resize_collate_u8" and pp.plans[0].canvas_hw == (192, 160)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_detect_under_poison(his, graph):
    """model.detect: the post-processing steps are appended to an already built plan; with use_graph the poison steps are captured too."""
    head = FCOSHead(0.05, 0.6, 1000, STRIDES)
    x = image(2, 128, 160, seed=14)
    his.use_graph = graph
    try:
        pp = check(lambda: tuple(his.detect(x, head)), [his], detector_keeps(256, 20), what=f"detect graph={graph}")
    finally:
        his.use_graph = False
    plan = pp.plans[0]
    assert plan.names[-1] == "post.clip" and (plan.graph is not None) == graph
    with torch.no_grad():               # ... and the detections are the ones of the three separate calls
        s, c, b, n = head.detect_padded(his(x))
        ref = clones((s, c, ClipBoxes()(x, b.contiguous()), n))
        same(clones(his.detect(x, head)), ref, "detect vs model + FCOSHead + ClipBoxes")
    his.invalidate_plans()


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
def test_forward_as_hip_graph_under_poison(his, u8):
    x = torch.randint(0, 256, (1, 128, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(15)).to(DEV) if u8 else image(1, 128, 160, seed=15)
    with torch.no_grad():
        eager = clones(flat(his(x)))
    his.use_graph = True
    try:
        pp = check(lambda: flat(his(x.clone())), [his], detector_keeps(256, 20), what="forward as a HIP graph")
    finally:
        his.use_graph = False
    assert pp.plans[0].graph is not None
    with torch.no_grad():
        same(clones(flat(his(x))), eager, "eager plan after the graph plans")
    his.invalidate_plans()


# ---- stand-alone sub-module plans
def _feats(B, widths, h5, w5, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, h5 * m, w5 * m, generator=gen).to(DEV) for c, m in zip(widths, (4, 2, 1))]


def _fpn_keeps(feats, F):
    """The pooled staging buffers (C % 4 == 0; other widths get a dedicated zero-padded buffer outside the pool) and the pyramid."""
    def kept(plan):
        B, _, h3, w3 = feats[0].shape
        h5, w5 = feats[2].shape[2:]
        lv = [(h3, w3), (h3 // 2, w3 // 2), (h5, w5)] + ([((h5 - 1) // 2 + 1, (w5 - 1) // 2 + 1), (((h5 - 1) // 2 + 1 - 1) // 2 + 1, ((w5 - 1) // 2 + 1 - 1) // 2 + 1)]
                                                         if plan.names[0].startswith("FPN.") else [(h5 // 2, w5 // 2), (h5 // 4, w5 // 4)])
        return [(B * t.shape[2] * t.shape[3], t.shape[1]) for t in feats if t.shape[1] % 4 == 0] + [(B * sum(h * w for h, w in lv), F)]
    return kept


def _head_keeps(pyr, ncls):
    def kept(plan):
        M, F = sum(t.shape[0] * t.shape[2] * t.shape[3] for t in pyr), pyr[0].shape[1]
        return [(M, F), (M, 2 * F), (M, (ncls + 3) // 4 * 4), (M, 8)]
    return kept


def _check_parts(fpn, head, feats, F, ncls, what):
    """fpn((c3, c4, c5)) and head(pyramid) as plans of their own, fed from caller-owned NCHW tensors."""
    pp = check(lambda: tuple(fpn(feats)), [fpn], _fpn_keeps(feats, F), what=what + " FPN alone")
    assert all(o.fresh for o in pp.still_out(pp.plans[0]))
    with torch.no_grad():
        pyr = clones(fpn(feats))
    fpn.invalidate_plans()
    pp = check(lambda: flat(head(pyr)), [head], _head_keeps(pyr, ncls), what=what + " head alone")
    first = pp.still_out(pp.plans[0])[0]
    assert first.fresh and (first.rows, first.C) == _head_keeps(pyr, ncls)(None)[0], "the staged pyramid must be the first, fresh buffer"


def test_hisfcos_parts_alone_under_poison(his):
    _check_parts(his.fpn, his.head, _feats(2, (512, 1024, 2048), 4, 4, 21), 256, 20, "HISFCOS")


def test_fcos_parts_alone_under_poison():
    torch.manual_seed(8)
    model = FCOS([2048, 1024, 512], 20, 256).eval()
    randomize_norms(model, 9)
    model.to(DEV)
    _check_parts(model.FPN, model.head, _feats(1, (512, 1024, 2048), 5, 3, 22), 256, 20, "FCOS")


def test_mnfcos_parts_alone_under_poison(mn):
    F, ncls = mn.head.cls_logits.weight.shape[1], mn.head.cls_logits.weight.shape[0]
    _check_parts(mn.FeaturePyramidNetwork, mn.head, _feats(2, (512, 1024, 2048), 4, 4, 23), F, ncls, "MNFCOS")


@pytest.mark.parametrize("kind", ["his", "fcos", "mn"])
def test_fpn_alone_with_a_width_that_is_no_multiple_of_4(kind):
    """padded_input's other branch: C3 with 30 channels is staged into a dedicated zero-padded 32-wide buffer, C4 / C5 come from the pool."""
    torch.manual_seed(31)
    fpn = {"his": lambda: HalfInvertedStageFPN([30, 64, 128], 32), "fcos": lambda: FeaturePyramidNetwork([128, 64, 30], 32),
           "mn": lambda: LieghtWeightFeaturePyramid_old([128, 64, 30], 32)}[kind]().eval()
    randomize_norms(fpn, 32)
    fpn.to(DEV)
    feats = _feats(2, (30, 64, 128), 4, 4, 33)
    pp = check(lambda: tuple(fpn(feats)), [fpn], _fpn_keeps(feats, 32), what=f"{kind} FPN, C3 width 30")
    assert len(pp.still_out(pp.plans[0])) == 3
    feats2 = [f * 0.5 + 0.1 for f in feats]          # new data through the cached plan: the zero channels stay zero
    with torch.no_grad():
        a = clones(fpn(feats2))
        fpn.invalidate_plans()
        same(clones(fpn(feats2)), a, "cached plan vs fresh plan on new data")
    fpn.invalidate_plans()


# ---- two plans in flight
def test_two_lane_pipeline_under_poison(his):
    from pytorch_object_detection_amd.pipeline import TwoLanePipeline
    head = FCOSHead(0.05, 0.6, 1000, STRIDES)

    def post(out, x, tag):
        s, c, b, n = head.detect_padded(out)
        return clones((s, c, ClipBoxes()(x, b), n)) + [tag]

    xs = [image(2, 128, 160, seed=40 + i) for i in range(4)]
    his.invalidate_plans()
    try:
        with torch.no_grad():
            serial = [post(his(x), x, i) for i, x in enumerate(xs)]
            his.invalidate_plans()
            with poisoned_pool() as pp:
                pipe = TwoLanePipeline(his, post)
                got = [r for r in (pipe.submit(x, tag=i) for i, x in enumerate(xs)) if r is not None]
                got.append(pipe.drain())
                torch.cuda.synchronize()
        assert [g[4] for g in got] == [0, 1, 2, 3] and 0 <= pipe.cut <= pipe.lo < pipe.hi
        for a, b in zip(serial, got):
            same(b[:4], a[:4], f"pipelined step {a[4]}")
        assert len(pp.plans) == 2 and pp.plans[0] is not pp.plans[1]
        for plan in pp.plans:
            assert pp.free_duplicates(plan) == [] and pp.poison_steps(plan) > 0 and pp.out_shapes(plan) == sorted(detector_keeps(256, 20)(plan))
    finally:
        his.invalidate_plans()
