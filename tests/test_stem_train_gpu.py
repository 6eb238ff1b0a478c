"""The trainable 7x7 stem on its HIP node (train_ops.stem_rows: fd_stem7x7_nhwc4 forward, fd_stem7x7_bwd_weight_nhwc4 backward) at model level:
FCOS([2048, 1024, 512], 20, 256) -- the detector the reference's train.py builds with every stage trainable -- with enable_stem_training()."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_object_detection_amd import train_ops as T
from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.model.loss import FCOSLoss
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
from pytorch_object_detection_amd.model.od import FCOS, MNFCOS

pytestmark = pytest.mark.gpu
DEV = "cuda"
STRIDES = [8, 16, 32, 64, 128]
RANGES = [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 9999999]]
INPUTS = {
    "1x128x128": ((1, 3, 128, 128), [[[10., 12., 60., 70.], [30., 30., 120., 110.]]], [[3, 7]]),
    "2x64x96": ((2, 3, 64, 96), [[[4., 6., 40., 50.], [-1, -1, -1, -1]], [[10., 2., 90., 60.], [30., 20., 70., 44.]]], [[3, -1], [1, 20]]),
}


MARGIN = {False: 2e-6, True: 8e-6}      # 3 x the largest fp32 error of bn1's output at these shapes: 6.7e-7 with bn1 frozen, 2.6e-6 on batch statistics


def _clear_of_decision_boundaries(x, model):
    """True when, in float64 and for bn1 frozen as well as on batch statistics, no ReLU input of the stem lies within MARGIN[mode] of 0 and no max-pool window with a
    positive maximum has its two largest values within it of each other.  Inside that margin an fp32 forward may take the other branch than the float64
    restatement (observed: |input| = 3.6e-7 against an fp32 error of 2.5e-6), and the restatement's gradient is then not the gradient of what was computed."""
    bn, w = model.backbone.bn1, model.backbone.conv1.weight.detach().double()
    t = F.conv2d(x.double(), w, stride=2, padding=3)
    for bn_train in (False, True):
        b = F.batch_norm(t, None if bn_train else bn.running_mean.double(), None if bn_train else bn.running_var.double(), bn.weight.detach().double(),
                         bn.bias.detach().double(), training=bn_train, eps=bn.eps)
        if float(b.abs().min()) < MARGIN[bn_train]:
            return False
        r = F.relu(b)
        win = F.unfold(r, 3, padding=1, stride=2).view(r.shape[0], r.shape[1], 9, -1)
        top = win.topk(2, dim=2).values
        if bool(((top[:, :, 0] > 0) & (top[:, :, 0] - top[:, :, 1] < MARGIN[bn_train])).any()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _batch_cpu(key):
    """The first image batch of a fixed seed sequence that keeps the stem's ReLU / max-pool decisions clear of rounding (the model's weights are those of _model())."""
    shape, gt, labels = INPUTS[key]
    torch.manual_seed(3)
    model = FCOS([2048, 1024, 512], 20, 256)
    for seed in range(shape[2] + shape[3], shape[2] + shape[3] + 5000):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
        if _clear_of_decision_boundaries(x, model):
            return x
    raise AssertionError("no image batch clear of the decision boundaries among 5000 seeds")


def _batch(key):
    _, gt, labels = INPUTS[key]
    return _batch_cpu(key).to(DEV), torch.tensor(gt, device=DEV), torch.tensor(labels, device=DEV)


def _model(seed=3):
    torch.manual_seed(seed)
    return FCOS([2048, 1024, 512], 20, 256).to(DEV).train()


def _loss(model, x, gt, labels):
    out = model(x)
    return FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1]


class _PoolGrad:
    """Records the gradient that reaches the stem segment's output (the max-pooled map = the first bottleneck's input)."""

    def __init__(self, monkeypatch):
        self.g, self.armed = None, False
        real = T.bottleneck

        def wrapped(blk, x):
            if self.armed:
                self.armed = False
                x.register_hook(lambda g: setattr(self, "g", g.detach().clone()))
            return real(blk, x)
        monkeypatch.setattr(T, "bottleneck", wrapped)


def _stem_segment_ref64(model, x, g_pool, bn_train):
    """conv1.weight.grad of maxpool(relu(bn1(conv1(x)))) for the pooled map's gradient g_pool, in float64 on the CPU."""
    bn = model.backbone.bn1
    w = model.backbone.conv1.weight.detach().double().cpu().requires_grad_(True)
    t = F.conv2d(x.double().cpu(), w, stride=2, padding=3)
    t = F.batch_norm(t, None if bn_train else bn.running_mean.double().cpu(), None if bn_train else bn.running_var.double().cpu(),
                     bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu(), training=bn_train, eps=bn.eps)
    F.max_pool2d(F.relu(t), 3, 2, 1).backward(g_pool.double().cpu().contiguous())
    return w.grad.numpy()


def test_strict_mode_trains_the_stem_without_a_fallback():
    assert T.STRICT, "tests run with FD_STRICT=1 (tests/conftest.py)"
    for key in INPUTS:
        model = _model()
        assert model.enable_stem_training() is model
        n0 = T.STATS["stock_fallbacks"]
        _loss(model, *_batch(key)).backward()
        assert T.STATS["stock_fallbacks"] == n0
        g = model.backbone.conv1.weight.grad
        assert g is not None and g.shape == (64, 3, 7, 7) and torch.isfinite(g).all() and float(g.abs().max()) > 0


@pytest.mark.parametrize("bn_train", [False, True], ids=["bn1-frozen", "bn1-batch-stats"])
@pytest.mark.parametrize("key", list(INPUTS))
def test_hip_stem_matches_the_stock_stem(key, bn_train, monkeypatch):
    """Same loss, same gradients as the stock-op stem.  conv1.weight.grad: each path's error is taken against the float64 restatement of the stem segment
    on the gradient that reached ITS pooled map; the HIP node may be 4 x as far off as the stock ops (MIOpen, native BatchNorm) plus 1e-6 of the tensor."""
    x, gt, labels = _batch(key)
    base = _model()
    if bn_train:
        base.backbone.bn1.train()
        for p in base.backbone.bn1.parameters():
            p.requires_grad_(True)
    rec = _PoolGrad(monkeypatch)
    res = {}
    for which in ("hip", "stock"):
        m = copy.deepcopy(base)
        if which == "hip":
            m.enable_stem_training()
        n0 = T.STATS["stock_fallbacks"]
        T.STRICT = which == "hip"
        try:
            rec.armed, rec.g = True, None
            loss = _loss(m, x, gt, labels)
            loss.backward()
        finally:
            T.STRICT = True
        assert T.STATS["stock_fallbacks"] - n0 == (0 if which == "hip" else 1)
        ref = _stem_segment_ref64(m, x, rec.g, bn_train)
        grads = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.grad is not None}
        res[which] = (float(loss.detach()), grads, np.abs(grads["backbone.conv1.weight"].astype(np.float64) - ref).max(), np.abs(ref).max())
    (l_h, g_h, e_h, s_h), (l_s, g_s, e_s, _) = res["hip"], res["stock"]
    print(f"stem train {key} bn_train={bn_train}: loss hip {l_h:.7f} stock {l_s:.7f}; conv1.weight.grad err vs fp64: hip {e_h:.3e} stock {e_s:.3e} "
          f"ratio {e_h / max(e_s, 1e-300):.3f} max|ref| {s_h:.3e}")
    np.testing.assert_allclose(l_h, l_s, rtol=2e-4)
    assert e_h <= 4 * e_s + 1e-6 * s_h, (e_h, e_s, s_h)
    assert g_h.keys() == g_s.keys() and "backbone.conv1.weight" in g_h
    for n in g_h:                                       # (the bar tests/test_train_gpu.py holds between the HIP and the stock head)
        s = float(np.abs(g_s[n]).max()) + 1e-12
        np.testing.assert_allclose(g_h[n] / s, g_s[n] / s, atol=3e-4, err_msg=n)


def test_amp_step_has_finite_gradients():
    x, gt, labels = _batch("2x64x96")
    model = _model().enable_stem_training()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9)
    scaler = torch.amp.GradScaler("cuda")
    n0 = T.STATS["stock_fallbacks"]
    with torch.autocast("cuda", dtype=torch.float16):
        loss = _loss(model, x, gt, labels)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    g = model.backbone.conv1.weight.grad
    assert T.STATS["stock_fallbacks"] == n0 and g.dtype == torch.float32
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    scaler.step(opt)
    scaler.update()
    assert torch.isfinite(model.backbone.conv1.weight).all()


def test_graph_replay_gives_the_eager_gradient_bit_for_bit():
    from pytorch_object_detection_amd.train_graph import GraphedStep
    x, gt, labels = _batch("2x64x96")
    base = _model().enable_stem_training()
    m_eager, m_graph = copy.deepcopy(base), copy.deepcopy(base)

    def make(model):
        def step(x_, gt_, labels_):
            model.zero_grad(set_to_none=True)
            loss = _loss(model, x_, gt_, labels_)
            loss.backward()
            return loss.detach()
        return step
    l_e = make(m_eager)(x, gt, labels)
    graphed = GraphedStep(make(m_graph), [x, gt, labels], warmup=2)
    l_g = graphed(x, gt, labels)
    torch.cuda.synchronize()
    assert torch.equal(l_e, l_g)
    assert torch.equal(m_eager.backbone.conv1.weight.grad, m_graph.backbone.conv1.weight.grad)
    assert float(m_graph.backbone.conv1.weight.grad.abs().max()) > 0


def test_mnfcos_trains_its_stem():
    x, gt, labels = _batch("1x128x128")
    torch.manual_seed(0)
    model = MNFCOS([2048, 1024, 512], 20, 256).enable_training(train_stem=True)
    model.freeze_all_bn = True
    model.to(DEV).train()
    n0 = T.STATS["stock_fallbacks"]
    out = model(x)
    FCOSLoss("giou")([out, FCOSGenTargets(STRIDES, RANGES)([out, gt, labels])])[-1].backward()
    g = model.backbone.conv1.weight.grad
    assert T.STATS["stock_fallbacks"] == n0
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_input_gradient_keeps_the_fallback():
    """An image that needs a gradient is not the node's case: the stock fallback (strict mode: the error) applies exactly as without the switch."""
    x, gt, labels = _batch("2x64x96")
    model = _model().enable_stem_training()
    xg = x.clone().requires_grad_(True)
    with pytest.raises(FdError, match="FD_STRICT"):
        model(xg)
    T.STRICT = False
    try:
        n0 = T.STATS["stock_fallbacks"]
        _loss(model, xg, gt, labels).backward()
        assert T.STATS["stock_fallbacks"] == n0 + 1
    finally:
        T.STRICT = True
    assert xg.grad is not None and torch.isfinite(xg.grad).all()
