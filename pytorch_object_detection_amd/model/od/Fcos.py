"""FCOS-R50 baseline on MI355X — mirrors the reference's model/od/Fcos.py (FCOS :12-58,
FeaturePyramidNetwork :61-91, HeadFCOS :94-133): same constructors and state_dict keys, HIP plan forward."""
from __future__ import annotations

from typing import List

import numpy as np
import torch
import torch.nn as nn

from ... import engine
from ..._lib import FdError
import torch.nn.functional as F

from ...ops import ACT_RELU
from ... import train_ops as T
from ...train_ops import conv2d as tconv, conv_bn_act as cba
from ..backbone.resnet50 import ResNet50
from ..modules.modules import ScaleExp, init_conv_kaiming, init_conv_random_normal
from ._planned import PlannedModule


class FeaturePyramidNetwork(PlannedModule):
    def __init__(self, in_channel: List[int], feature: int = 256):
        super().__init__()
        self.P5 = nn.Conv2d(in_channel[0], feature, 1, 1, 'same')
        self.P4 = nn.Conv2d(in_channel[1], feature, 1, 1, 'same')
        self.P3 = nn.Conv2d(in_channel[2], feature, 1, 1, 'same')
        self.P5_c1 = nn.Conv2d(feature, feature, 3, 1, 'same')
        self.P4_c1 = nn.Conv2d(feature, feature, 3, 1, 'same')
        self.P3_c1 = nn.Conv2d(feature, feature, 3, 1, 'same')
        self.P6_c1 = nn.Conv2d(feature, feature, 3, 2, 1)
        self.P7_c1 = nn.Conv2d(feature, feature, 3, 2, 1)
        self.apply(init_conv_kaiming)

    @staticmethod
    def _lateral(m: nn.Conv2d, c: torch.Tensor) -> torch.Tensor:
        """m(c); a map WIDER than m.in_channels is an EfficientNet endpoint held at its width rounded up to 32 with zero pad channels
        (trunk_train_forward): the lateral weight gets zero input columns inside the autograd graph (train_ops.conv_rows_wide)."""
        if c.shape[1] == m.in_channels or T._STOCK:
            return tconv(m, c)
        T._need_cuda(c)
        B, _, H, W = c.shape
        return T.from_rows(T.conv_rows_wide(m, T.to_rows(c), T.Segs.make(B, [(H, W)])), B, H, W)[:, :m.out_channels]

    def train_forward(self, x):
        c3, c4, c5 = x
        up = lambda t: F.interpolate(t, scale_factor=2.0, mode="nearest")  # noqa: E731
        p5 = self._lateral(self.P5, c5)
        p4 = tconv(self.P4_c1, up(p5) + self._lateral(self.P4, c4))
        p3 = tconv(self.P3_c1, up(p4) + self._lateral(self.P3, c3))
        p5 = tconv(self.P5_c1, p5)
        p6 = cba(self.P6_c1, None, p5, ACT_RELU)   # the reference's in-place ReLU rectifies the returned P6 (Fcos.py:90)
        return p3, p4, p5, p6, tconv(self.P7_c1, p6)

    def forward(self, x):
        return self.train_forward(x) if self.training else self._run_fpn(engine.build_fcos_fpn, x)


class HeadFCOS(PlannedModule):
    def __init__(self, feature: int, num_class: int, prior: float = 0.01):
        super().__init__()
        self.class_num, self.prior = num_class, prior
        cls_branch, reg_branch = [], []
        for _ in range(4):
            cls_branch += [nn.Conv2d(feature, feature, 3, padding=1, bias=False), nn.GroupNorm(32, feature), nn.ReLU(True)]
            reg_branch += [nn.Conv2d(feature, feature, 3, padding=1, bias=False), nn.GroupNorm(32, feature), nn.ReLU(True)]
        self.cls_branch = nn.Sequential(*cls_branch)
        self.reg_branch = nn.Sequential(*reg_branch)
        self.cls_logits = nn.Conv2d(feature, num_class, 3, padding=1)
        self.cnt_logits = nn.Conv2d(feature, 1, 3, padding=1)
        self.reg_pred = nn.Conv2d(feature, 4, 3, padding=1)
        self.apply(init_conv_random_normal)
        nn.init.constant_(self.cls_logits.bias, -np.log((1 - prior) / prior))
        self.scale_exp = nn.ModuleList([ScaleExp(1.0) for _ in range(5)])

    def train_forward(self, inputs):
        """Training-time autograd forward: the five levels as one rows buffer, every tower layer (3x3 conv, GroupNorm +
        ReLU) and the predictors one HIP launch over the whole pyramid, forward and backward (train_ops)."""
        x0 = inputs[0]
        gns = [self.cls_branch[3 * k + 1] for k in range(4)] + [self.reg_branch[3 * k + 1] for k in range(4)]
        if not T.covered(self.cls_branch[0], None, x0) or not all(T._gn_ok(g, x0) for g in gns):
            return self._train_forward_stock(inputs)
        f, segs = T.pyramid_rows(inputs)
        c, r = f, f
        for k in range(4):
            c = T.groupnorm_rows(self.cls_branch[3 * k + 1], T.conv_rows(self.cls_branch[3 * k], c, segs), segs,
                                 self.cls_branch[3 * k + 2])
            r = T.groupnorm_rows(self.reg_branch[3 * k + 1], T.conv_rows(self.reg_branch[3 * k], r, segs), segs,
                                 self.reg_branch[3 * k + 2])
        return T.predictor_rows(self.cls_logits, self.reg_pred, self.cnt_logits, c, r, segs, self.scale_exp)

    def _train_forward_stock(self, inputs):
        T.stock_fallback("the HeadFCOS GroupNorm layers (widths outside the rows kernels)")
        cls_l, cnt_l, reg_l = [], [], []
        for i, f in enumerate(inputs):
            c, r = f, f
            for k in range(4):
                c = self.cls_branch[3 * k + 2](self.cls_branch[3 * k + 1](tconv(self.cls_branch[3 * k], c)))
                r = self.reg_branch[3 * k + 2](self.reg_branch[3 * k + 1](tconv(self.reg_branch[3 * k], r)))
            cls_l.append(tconv(self.cls_logits, c))
            cnt_l.append(self.cnt_logits(r))
            reg_l.append(torch.exp(tconv(self.reg_pred, r) * self.scale_exp[i].scale))
        return cls_l, cnt_l, reg_l

    def forward(self, inputs):
        return self.train_forward(inputs) if self.training else self._run_head(engine.build_fcos_head, inputs)


class FCOS(PlannedModule):
    """FCOS(in_channel [C5, C4, C3 widths], num_class, feature, freeze_bn, efficientnet) — reference Fcos.py:12-58.

    `efficientnet=True` selects the EfficientNet trunk.  As shipped the reference hard-codes `EfficientNetV1(0)` (B0,
    Fcos.py:31-32) and then unpacks the wrapper's FIVE endpoints into three names (Fcos.py:78), which raises; the authors'
    recorded runs ("ef-B0", Result/propose_giou_50_61.1:77-99) imply the three deepest endpoints feed the FPN.  Here:
    `backbone_number` (extra keyword, default 0 = the reference's B0; 3 = BASELINE Cfg5's B3) picks the model and
    reduction_3/4/5 (strides 8/16/32) go to the FPN as (C3, C4, C5); in_channel must be their widths reversed
    (B0 [320, 112, 40], B3 [384, 136, 48])."""

    hip_train = False       # efficientnet=True: opt-in training on the HIP autograd nodes (enable_training())

    def __init__(self, in_channel: List[int], num_class: int, feature: int, freeze_bn: bool = True,
                 efficientnet: bool = False, backbone_number: int = 0):
        super().__init__()
        self.efficientnet = bool(efficientnet)
        if efficientnet:
            from ..backbone.efficientnetv1 import EfficientNetV1    # (lazy: that module imports this package's _planned)
            self.backbone = EfficientNetV1(backbone_number)
            want = self.backbone.endpoint_channels[:1:-1]
            if list(in_channel) != want:
                raise FdError(f"FCOS(efficientnet=True, backbone_number={backbone_number}) needs in_channel={want} "
                              f"(reduction_5/4/3 widths), got {list(in_channel)}")
            blocks = list(self.backbone.model._blocks)
            # widest stride-2 activation: the stem output or the first stride-2 block's expanded input (plan_batch_limit)
            self._largest_map_channels = max([self.backbone.model._conv_stem.out_channels] +
                                             [b._depthwise_conv.in_channels for b in blocks[:next(i for i, b in enumerate(blocks) if b.stride > 1) + 1]])
        else:
            self.backbone = ResNet50(3)
        self.FPN = FeaturePyramidNetwork(in_channel, feature)
        self.head = HeadFCOS(feature, num_class, 0.01)
        self.backbone_freeze = freeze_bn
        if self.backbone_freeze:
            self.freeze_batchnorm()

    def _parts(self):
        return self.FPN, engine.build_fcos_fpn, engine.build_fcos_head

    def _build_trunk(self, plan, B: int, H: int, W: int):
        if self.efficientnet:
            return engine.build_efficientnet(plan, self.backbone.model, B, H, W, plan.image_ref, keep=(2, 3, 4))[2:]
        return super()._build_trunk(plan, B, H, W)

    def enable_stem_training(self):
        """Opt in to the HIP node for the trainable 7x7 stem (backbone.hip_stem_train: the stem kernel forward, fd_stem7x7_bwd_weight_nhwc4 backward)
        instead of the stock-op fallback.  Off by default.  Returns self."""
        if self.efficientnet:
            raise FdError("FCOS(efficientnet=True) has no ResNet stem to train")
        self.backbone.hip_stem_train = True
        return self

    def enable_training(self, train_stem: bool = False, batch_stats: bool = False, drop_connect_rate: float = 0.0):
        """FCOS(efficientnet=True): opt in to training on the HIP autograd nodes (the MBConv trunk through train_ops.mbconv_rows).  As called without
        arguments it freezes the stem (_conv_stem, _bn0) -- the one departure from the reference's trainable set -- and the never-run _conv_head / _bn1 /
        _fc, so that DDP needs no find_unused_parameters, and trains on frozen BatchNorm layers without drop-connect.  Three switches close those departures
        from how efficientnet_pytorch trains:
          train_stem=True          _conv_stem stays trainable (fd_stem_conv_bwd_weight_nhwc4), and _bn0 with it when batch_stats is on
          batch_stats=True         the trunk's BatchNorm layers run on batch statistics with trainable affine parameters (fd_batchnorm_train_*); needs a model
                                   constructed with freeze_bn=False.  With train_stem=False the stem stays folded on its running statistics
          drop_connect_rate=r      stochastic depth on the skip blocks at the package's per-block rate r * idx / len(blocks) (fd_sample_scale_add_nhwc)
        Build the optimizer after this call.  With the ResNet trunk, which trains as constructed, it does nothing.  Returns self."""
        if not self.efficientnet:
            return self
        net = self.backbone.model
        if batch_stats and self.backbone_freeze:
            raise FdError("FCOS.enable_training(batch_stats=True) needs a model constructed with freeze_bn=False (this one froze its BatchNorm layers)")
        if not 0.0 <= float(drop_connect_rate) < 1.0:
            raise FdError(f"FCOS.enable_training: drop_connect_rate must be in [0, 1) (got {drop_connect_rate})")
        stem_on = bool(train_stem)
        if not stem_on and net._conv_stem.weight.requires_grad:
            import warnings
            warnings.warn("FCOS.enable_training() freezes the EfficientNet stem (backbone.model._conv_stem / _bn0); an optimizer built before this call "
                          "holds a parameter that no longer receives a gradient", stacklevel=2)
        frozen = (net._conv_head, net._bn1, net._fc) + (() if stem_on else (net._conv_stem, net._bn0))
        for m in frozen:
            for p in m.parameters():
                p.requires_grad = False
        if stem_on or batch_stats or drop_connect_rate:
            net.train_stem, net.batch_stats = stem_on, bool(batch_stats)
            net.drop_connect_rate = net.drop_connect_accepted = float(drop_connect_rate)
        self.hip_train = True
        return self

    def _train_forward_effnet(self, x: torch.Tensor, drop_u=None):
        from ..backbone.efficientnetv1 import trunk_train_forward
        self._check_train_input(x)
        if not self.backbone_freeze and not self.backbone.model.batch_stats:
            raise FdError("FCOS(efficientnet=True, freeze_bn=False): the HIP training path folds the backbone's BatchNorm layers frozen; batch statistics "
                          "in the MBConv trunk are out of scope (construct the model with freeze_bn=True)")
        T.PACKS.refresh()
        return self.head.train_forward(self.FPN.train_forward(trunk_train_forward(self.backbone.model, x, drop_u)))

    def forward(self, x: torch.Tensor, events=None, drop_u=None):
        if not self.training:
            return self._eval_forward(x, events)
        if self.efficientnet:
            if not self.hip_train:
                raise FdError("FCOS(efficientnet=True) is inference-only on the HIP path as constructed; call model.eval(), or opt in to training on "
                              "the HIP autograd nodes with model.enable_training() (frozen stem and BatchNorm, no drop-connect)")
            return self._train_forward_effnet(x, drop_u)
        return self._train_forward(x)
