"""EfficientNet-B0..B7 trunk on MI355X behind the reference's wrapper API (model/backbone/efficientnetv1.py:11-26):
`EfficientNetV1(backbone_number)(x) -> [reduction_1, ..., reduction_5]`.

The reference delegates to the pip package efficientnet_pytorch (pinned 0.7.1, README.md:16: `EfficientNet.from_pretrained`,
`set_swish`, `extract_endpoints`), which is third-party, absent from the reference tree and from this image.  The modules
below only HOLD the parameters under efficientnet_pytorch's names (`model._conv_stem`, `model._bn0`,
`model._blocks.{i}._expand_conv / _bn0 / _depthwise_conv / _bn1 / _se_reduce / _se_expand / _project_conv / _bn2`,
`model._conv_head`, `model._bn1`, `model._fc`), so a reference checkpoint loads with strict=True; the arithmetic
(MBConv: expand 1x1 -> depthwise k x k stride s with static TF-"SAME" padding -> SE -> project 1x1 (+ skip), BN eps 1e-3,
swish) runs in engine.build_efficientnet on the HIP kernels.  There is no network here, hence no pretrained download:
parameters keep torch's default initialisation until a state_dict is loaded (`from_pretrained` in the reference).
"""
from __future__ import annotations

import math
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import engine, ops
from ... import train_ops as T
from ..._lib import FdError, Segs
from ..od._planned import PlannedModule

VALID_MODELS = ('efficientnet-b0', 'efficientnet-b1', 'efficientnet-b2', 'efficientnet-b3', 'efficientnet-b4',
                'efficientnet-b5', 'efficientnet-b6', 'efficientnet-b7', 'efficientnet-b8', 'efficientnet-l2')

# compound-scaling coefficients: name -> (width, depth, nominal resolution, dropout)
_COEFF = {'efficientnet-b0': (1.0, 1.0, 224, 0.2), 'efficientnet-b1': (1.0, 1.1, 240, 0.2),
          'efficientnet-b2': (1.1, 1.2, 260, 0.3), 'efficientnet-b3': (1.2, 1.4, 300, 0.3),
          'efficientnet-b4': (1.4, 1.8, 380, 0.4), 'efficientnet-b5': (1.6, 2.2, 456, 0.4),
          'efficientnet-b6': (1.8, 2.6, 528, 0.5), 'efficientnet-b7': (2.0, 3.1, 600, 0.5),
          'efficientnet-b8': (2.2, 3.6, 672, 0.5), 'efficientnet-l2': (4.3, 5.3, 800, 0.5)}
# the seven B0 stages "r{repeat}_k{kernel}_s{stride}{stride}_e{expand}_i{in}_o{out}_se0.25"
_STAGES = ('r1_k3_s11_e1_i32_o16_se0.25', 'r2_k3_s22_e6_i16_o24_se0.25', 'r2_k5_s22_e6_i24_o40_se0.25',
           'r3_k3_s22_e6_i40_o80_se0.25', 'r3_k5_s11_e6_i80_o112_se0.25', 'r4_k5_s22_e6_i112_o192_se0.25',
           'r1_k3_s11_e6_i192_o320_se0.25')
BN_EPS, BN_MOMENTUM = 1e-3, 1.0 - 0.99


def _scaled_width(filters: int, width: float, divisor: int = 8) -> int:
    f = filters * width
    out = max(divisor, int(f + divisor / 2) // divisor * divisor)
    return int(out + divisor) if out < 0.9 * f else int(out)


def _decode(stage: str) -> dict:
    d = {}
    for tok in stage.split('_'):
        key = 'se' if tok.startswith('se') else tok[0]
        d[key] = tok[len(key):]
    return dict(repeat=int(d['r']), kernel=int(d['k']), stride=int(d['s'][0]), expand=int(d['e']), cin=int(d['i']),
                cout=int(d['o']), se=float(d['se']))


def static_same_padding(nominal: int, kernel: int, stride: int) -> Tuple[int, int]:
    """(before, after) zero padding of efficientnet_pytorch's Conv2dStaticSamePadding for a square nominal image size:
    TF 'SAME' computed once for the size the model was BUILT for, then applied to whatever input arrives."""
    out = int(math.ceil(nominal / stride))
    pad = max((out - 1) * stride + kernel - nominal, 0)
    return pad // 2, pad - pad // 2


class _MBConv(nn.Module):
    """Parameter container of one MBConvBlock; `pad` is the depthwise conv's static (before, after) padding."""

    def __init__(self, kernel: int, stride: int, expand: int, cin: int, cout: int, se_ratio: float, nominal: int):
        super().__init__()
        mid = cin * expand
        self.kernel, self.stride, self.expand, self.cin, self.cout = kernel, stride, expand, cin, cout
        self.pad = static_same_padding(nominal, kernel, stride)
        self.skip = stride == 1 and cin == cout
        if expand != 1:
            self._expand_conv = nn.Conv2d(cin, mid, 1, bias=False)
            self._bn0 = nn.BatchNorm2d(mid, momentum=BN_MOMENTUM, eps=BN_EPS)
        self._depthwise_conv = nn.Conv2d(mid, mid, kernel, stride, groups=mid, bias=False)
        self._bn1 = nn.BatchNorm2d(mid, momentum=BN_MOMENTUM, eps=BN_EPS)
        squeezed = max(1, int(cin * se_ratio))
        self._se_reduce = nn.Conv2d(mid, squeezed, 1)
        self._se_expand = nn.Conv2d(squeezed, mid, 1)
        self._project_conv = nn.Conv2d(mid, cout, 1, bias=False)
        self._bn2 = nn.BatchNorm2d(cout, momentum=BN_MOMENTUM, eps=BN_EPS)


class _EfficientNet(nn.Module):
    """`EfficientNet.from_name(model_name)` as a parameter container (state_dict keys of efficientnet_pytorch 0.7.1)."""

    # the opt-in switches of FCOS.enable_training(train_stem, batch_stats, drop_connect_rate); set on the instance only by that call
    train_stem = False
    batch_stats = False
    drop_connect_accepted = 0.0

    def __init__(self, model_name: str):
        super().__init__()
        if model_name not in _COEFF:
            raise FdError(f"unknown EfficientNet '{model_name}'")
        width, depth, res, _ = _COEFF[model_name]
        self.model_name, self.image_size = model_name, res
        # efficientnet_pytorch applies stochastic depth (drop_connect_rate 0.2) in train mode; the HIP training path trains without it unless
        # FCOS.enable_training(drop_connect_rate=r) opts in: 0.0 here, and trunk_train_forward refuses any value that call did not accept
        self.drop_connect_rate = 0.0
        stem = _scaled_width(32, width)
        self._conv_stem = nn.Conv2d(3, stem, 3, 2, bias=False)
        self.stem_pad = static_same_padding(res, 3, 2)
        self._bn0 = nn.BatchNorm2d(stem, momentum=BN_MOMENTUM, eps=BN_EPS)
        size = int(math.ceil(res / 2))
        blocks = []
        for st in map(_decode, _STAGES):
            cin, cout = _scaled_width(st['cin'], width), _scaled_width(st['cout'], width)
            for r in range(int(math.ceil(depth * st['repeat']))):
                first = r == 0
                blocks.append(_MBConv(st['kernel'], st['stride'] if first else 1, st['expand'], cin if first else cout, cout,
                                      st['se'], size))
                if first:
                    size = int(math.ceil(size / st['stride']))
        self._blocks = nn.ModuleList(blocks)
        head = _scaled_width(1280, width)
        self._conv_head = nn.Conv2d(blocks[-1].cout, head, 1, bias=False)   # reduction_6: built for checkpoint parity, never run
        self._bn1 = nn.BatchNorm2d(head, momentum=BN_MOMENTUM, eps=BN_EPS)
        self._fc = nn.Linear(head, 1000)

    def bn_on_running_stats(self):
        """The BatchNorms that a training forward runs on their running statistics whatever their .training flag says: without train_stem the stem's _bn0,
        folded into the stem launch (trunk_train_forward).  optim.update_bn leaves these alone."""
        return [] if self.train_stem else [self._bn0]


def _out_hw(h: int, w: int, k: int, s: int, pad) -> Tuple[int, int]:
    return (h + pad[0] + pad[1] - k) // s + 1, (w + pad[0] + pad[1] - k) // s + 1


def _drop_scales(net: "_EfficientNet", B: int, device, drop_u):
    """Per block the drop-connect scales [B] (train_ops.drop_connect_scale) or None: p = rate * idx / len(blocks), applied only to skip blocks and only when
    p > 0 (block 0 never drops).  drop_u: optional [len(blocks), B] uniform numbers (tests); else torch.rand on the device, one draw per dropping block."""
    blocks = list(net._blocks)
    rate = float(net.drop_connect_rate)
    if drop_u is not None and (drop_u.dim() != 2 or tuple(drop_u.shape) != (len(blocks), B)):
        raise FdError(f"EfficientNet trunk: drop_u must be [len(blocks), B] = [{len(blocks)}, {B}] (got {tuple(drop_u.shape)})")
    out = []
    for i, blk in enumerate(blocks):
        p = rate * i / len(blocks)
        if not (blk.skip and p > 0):
            out.append(None)
            continue
        u = drop_u[i].to(device) if drop_u is not None else torch.rand(B, dtype=torch.float32, device=device)
        out.append(T.drop_connect_scale(p, u))
    return out


def _trunk_stock(net: "_EfficientNet", x: torch.Tensor, drop_u=None):
    """The trunk on stock PyTorch-ROCm ops (FD_TRAIN_STOCK_CONV=1 only: the diagnostic mode that times the HIP step against them); follows the train_stem /
    batch_stats / drop-connect switches of enable_training with the same drop_u."""
    swish = lambda t: t * torch.sigmoid(t)  # noqa: E731
    frozen = lambda m, t: F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)  # noqa: E731

    def batch(m, t):
        if m.num_batches_tracked is not None:
            m.num_batches_tracked.add_(1)
        # (momentum=None, the cumulative average of optim.update_bn: this diagnostic path reads the counter on the host, as nn.BatchNorm2d.forward does)
        momentum = m.momentum if m.momentum is not None else 1.0 / float(m.num_batches_tracked)
        return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, True, momentum, m.eps)

    bn = batch if net.batch_stats else frozen
    same = lambda t, pad: F.pad(t, (pad[0], pad[1], pad[0], pad[1])) if (pad[0] or pad[1]) else t  # noqa: E731
    if net.train_stem:
        x = swish(bn(net._bn0, F.conv2d(same(x, net.stem_pad), net._conv_stem.weight, None, 2)))
    else:
        with torch.no_grad():
            x = swish(frozen(net._bn0, F.conv2d(same(x, net.stem_pad), net._conv_stem.weight, None, 2)))
    ends, blocks = [], list(net._blocks)
    scales = _drop_scales(net, x.shape[0], x.device, drop_u)
    for i, blk in enumerate(blocks):
        inp = x
        if blk.expand != 1:
            x = swish(bn(blk._bn0, F.conv2d(x, blk._expand_conv.weight)))
        x = swish(bn(blk._bn1, F.conv2d(same(x, blk.pad), blk._depthwise_conv.weight, None, blk.stride, 0, 1, x.shape[1])))
        sq = swish(F.conv2d(F.adaptive_avg_pool2d(x, 1), blk._se_reduce.weight, blk._se_reduce.bias))
        x = torch.sigmoid(F.conv2d(sq, blk._se_expand.weight, blk._se_expand.bias)) * x
        x = bn(blk._bn2, F.conv2d(x, blk._project_conv.weight))
        if blk.skip:
            x = (x if scales[i] is None else x * scales[i].view(-1, 1, 1, 1)) + inp
        if i + 1 == len(blocks) or blocks[i + 1].stride > 1:
            ends.append(x)
    return tuple(ends[-3:])


def trunk_train_forward(net: "_EfficientNet", x: torch.Tensor, drop_u=None):
    """The EfficientNet trunk of a training step on the HIP autograd nodes: image batch [B, 3, H, W] -> (C3, C4, C5), the endpoints reduction_3/4/5 as
    NCHW-shaped channels-last views.  As FCOS.enable_training() leaves the model, the stem (_conv_stem + _bn0 + swish) is frozen and runs on the inference
    kernel without a graph, and every MBConv block is train_ops.mbconv_rows on frozen BatchNorm layers.  The switches of enable_training change that:
    net.train_stem (the stem is train_ops.effnet_stem_rows, with its weight gradient), net.batch_stats (every BatchNorm of the blocks, and the stem's when it
    trains, on batch statistics) and a drop_connect_rate accepted there (stochastic depth on the skip blocks; drop_u: optional [len(blocks), B] uniform
    numbers that replace the torch.rand draws).  Every map from the stem output to the endpoints is held at its width ROUNDED UP TO 32 with pad channels that
    are exactly zero (forward and backward), so the returned maps are round32(48 / 136 / 384) wide: FeaturePyramidNetwork.train_forward pads its lateral
    weights."""
    if net.drop_connect_rate and net.drop_connect_rate != net.drop_connect_accepted:
        raise FdError(f"EfficientNet trunk: drop_connect_rate={net.drop_connect_rate} is not supported on the HIP training path (it trains without "
                      "stochastic depth: set model.drop_connect_rate = 0.0)")
    if not net.train_stem and not net.batch_stats and (not T.bn_is_frozen(net._bn0) or net._conv_stem.weight.requires_grad):
        raise FdError("EfficientNet trunk: the HIP training path needs a frozen stem (_conv_stem, _bn0) and frozen BatchNorm layers "
                      "(FCOS(..., freeze_bn=True).enable_training(); batch statistics in the MBConv trunk are out of scope)")
    if not net.train_stem and (net._conv_stem.weight.requires_grad or net._bn0.weight.requires_grad):
        raise FdError("EfficientNet trunk: without train_stem the stem (_conv_stem, _bn0) must not require gradients (FCOS.enable_training() freezes it)")
    if x.dim() != 4 or x.shape[1] != 3 or not T._f32(x) or x.requires_grad:
        raise FdError("EfficientNet trunk: expected an image batch [B, 3, H, W] that needs no gradient")
    if T._STOCK:
        return _trunk_stock(net, x.float(), drop_u)
    B, _, H, W = x.shape
    dev = x.device
    C0 = net._conv_stem.out_channels
    h, w = _out_hw(H, W, 3, 2, net.stem_pad)
    if h < 1 or w < 1:
        raise FdError("EfficientNet: input too small")
    if net.train_stem:
        buf = T.effnet_stem_rows(net, x.float(), h, w, net.batch_stats)
    else:
        with torch.no_grad():           # (folded on the running statistics whatever _bn0.training says)
            x4 = torch.empty(B * H * W, 4, dtype=torch.float32, device=dev)
            ops.nchw3_to_nhwc4(x.float().contiguous(), x4)
            sc, sf = T._bn_fold(net._bn0)
            buf = (torch.zeros if T.round32(C0) != C0 else torch.empty)(B * h * w, T.round32(C0), dtype=torch.float32, device=dev)
            ops.stem_conv3(x4, ops.pack_stem3_weight(net._conv_stem.weight), ops.Rows(buf, 0, C0), B, H, W, 3, 2, net.stem_pad[0], net.stem_pad[0], h, w,
                           sc, sf, ops.ACT_SILU)
    t, segs = buf, Segs.make(B, [(h, w)])
    ends, blocks = [], list(net._blocks)
    scales = _drop_scales(net, B, dev, drop_u) if net.drop_connect_rate else [None] * len(blocks)
    for i, blk in enumerate(blocks):
        if net.batch_stats or scales[i] is not None:
            t, segs = T.mbconv_rows(blk, t, segs, batch_stats=net.batch_stats, drop_scale=scales[i])
        else:
            t, segs = T.mbconv_rows(blk, t, segs)
        if i + 1 == len(blocks) or blocks[i + 1].stride > 1:
            ends.append(T.from_rows(t, B, segs.H[0], segs.W[0]))
    return tuple(ends[-3:])


class EfficientNetV1(PlannedModule):
    """Reference model/backbone/efficientnetv1.py:11-26.  forward(x [B,3,H,W] fp32 CUDA) -> list of the five endpoints
    reduction_1..reduction_5 (strides 2, 4, 8, 16, 32; B3: 24, 32, 48, 136, 384 channels) as NCHW-shaped channels-last
    views of plan-owned buffers.  Stand-alone the wrapper is inference only (BatchNorm folded, eval); the trunk TRAINS inside FCOS(efficientnet=True)
    after enable_training(), through trunk_train_forward (MBConv blocks on the HIP autograd nodes; frozen stem and BatchNorm and no drop-connect unless that
    call's train_stem / batch_stats / drop_connect_rate switches opt in)."""

    def __init__(self, backbone_number: int, memory_efficient: bool = False):
        super().__init__()
        self.model = _EfficientNet(VALID_MODELS[backbone_number])
        self.memory_efficient = memory_efficient      # swish variant of the reference: same forward arithmetic

    @property
    def drop_connect_rate(self) -> float:
        """Stochastic-depth rate of the training path: 0.0 (efficientnet_pytorch trains at 0.2); the HIP path refuses any value that
        FCOS.enable_training(drop_connect_rate=r) did not accept."""
        return self.model.drop_connect_rate

    @drop_connect_rate.setter
    def drop_connect_rate(self, v: float) -> None:
        self.model.drop_connect_rate = float(v)

    @property
    def endpoint_channels(self) -> List[int]:
        blocks = list(self.model._blocks)
        ch = [b.cout for b, nxt in zip(blocks, blocks[1:]) if nxt.stride > 1]
        return ch + [blocks[-1].cout]

    def build_plan(self, B: int, H: int, W: int, device):
        plan = engine.Plan(device, self.conv_precision)
        plan.image_ref = [None]
        plan.input_u8 = None
        plan.endpoints = engine.build_efficientnet(plan, self.model, B, H, W, plan.image_ref, keep=(0, 1, 2, 3, 4))
        return plan

    def forward(self, x: torch.Tensor):
        if self.training:
            raise FdError("EfficientNet backbones are inference-only on the HIP path (call .eval()); the reference never "
                          "trains them in its shipped scripts (train.py:92-97)")
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise FdError("expected a float32 image batch [B, 3, H, W]")
        if not x.is_cuda:
            raise FdError("pytorch_object_detection_amd runs on the GPU only; there is no CPU fallback (got a CPU tensor)")
        B, _, H, W = x.shape
        plan = self._get_plan(("effnet", B, H, W, str(x.device)), lambda: self.build_plan(B, H, W, x.device))
        plan.image_ref[0] = x.contiguous()
        plan.run()
        outs = []
        for rows, segs in plan.endpoints:
            h, w = segs.H[0], segs.W[0]
            outs.append(rows.tensor().view(B, h, w, rows.C).permute(0, 3, 1, 2))
        return outs
