"""MNFCOS on MI355X -- mirrors the reference's model/od/MNFcos.py (MNFCOS :11-36, LieghtWeightFeaturePyramid_old :222-256,
MNHeadFCOS :259-297; the detector config/main.yaml:2 selects and Test_coco.py:201 builds): same constructors and state_dict keys,
HIP plan forward.  SURVEY section 8f n4.

As shipped the reference's forward raises: MNBlock pads its dilated depthwise conv with `dilation` (modules.py:203), which keeps the
map size only for k = 3, and LieghtWeightFeaturePyramid_old uses k = 5 and 7 (MNFcos.py:233-235), so the first residual add
(modules.py:215) fails (tests/golden/g10_mnfcos_parts.npz records it).  Here the padding is 'same' -- identical for the k = 3 blocks
(the whole head, pinned against the reference by g10), the evident intent for the others.

Training is opt-in.  As constructed the model is inference-only (`train()` + forward raises, as it always did).  `model.enable_training()` sets
`hip_train` on the model, its FPN, its head and every MNBlock, and a forward in train() then builds an autograd graph of HIP rows nodes like
HalfInvertedStageFCOS does: the trunk's fused bottlenecks, the 1x1 laterals, the MNBlocks (train_ops.mn_block_rows: dilated depthwise conv with its data
and weight gradient kernels), upsample / max-pool nodes, the head over the whole pyramid per launch.  BatchNorm follows PlannedModule.train(): the
backbone's stays frozen, the FPN's and the head's run on batch statistics (per level in the shared head blocks, as the reference calls them once per
level) unless `freeze_all_bn` pins them.  enable_training() freezes the 7x7 stem (backbone.freeze_stages(0)) by default, the one departure from the
reference's trainable set; enable_training(train_stem=True) keeps it trainable on the HIP stem node (train_ops.stem_rows)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch
import torch.nn as nn

from ... import engine
from ... import train_ops as T
from ..._lib import FdError, Segs
from ..backbone.resnet50 import ResNet50v2
from ..modules.modules import MNBlock, ScaleExp
from ._planned import PlannedModule


def _enable_blocks(root: nn.Module) -> None:
    """hip_train on `root` and on every MNBlock / MNFCOS container below it."""
    for m in root.modules():
        if isinstance(m, (MNBlock, LieghtWeightFeaturePyramid_old, MNHeadFCOS, MNFCOS)):
            m.hip_train = True


class LieghtWeightFeaturePyramid_old(PlannedModule):
    hip_train = False       # opt-in training on the HIP autograd nodes (enable_training())

    def __init__(self, in_channel: List[int], feature: int = 128):
        super().__init__()
        self.C5PW = nn.Conv2d(in_channel[0], feature, 1, 1, 'same')
        self.C4PW = nn.Conv2d(in_channel[1], feature, 1, 1, 'same')
        self.C3PW = nn.Conv2d(in_channel[2], feature, 1, 1, 'same')
        self.MNB1_P3 = MNBlock(feature, feature, 3, 2, 2)          # (constructed, never called: MNFcos.py:229)
        self.DownSample_1 = nn.MaxPool2d(2, 2)
        self.DownSample_2 = nn.MaxPool2d(2, 2)
        self.UpSample_1 = nn.Upsample(scale_factor=2)
        self.UpSample_2 = nn.Upsample(scale_factor=2)
        self.MNB7 = MNBlock(feature, feature, 7, 1, 2)
        self.MNB6 = MNBlock(feature, feature, 5, 1, 2)
        self.MNB5 = MNBlock(feature, feature, 5, 2, 2)
        self.MNB4 = MNBlock(feature, feature, 3, 2, 2)
        self.MNB3 = MNBlock(feature, feature, 3, 1, 2)

    def enable_training(self):
        _enable_blocks(self)
        return self

    def train_forward(self, x):
        """The FPN on NHWC rows, every op a differentiable HIP node: 1x1 laterals (+ bias), MNB5 -> up + add -> MNB4 -> up + add -> MNB3,
        max-pool -> MNB6 -> max-pool -> MNB7 (MNFcos.py:239-256).  A shape the nodes do not cover raises: there is no stock-op path."""
        c3, c4, c5 = x
        for t in x:
            self._check_train_input(t)
        B = c5.shape[0]
        h5, w5 = c5.shape[2], c5.shape[3]
        hw = [tuple(c3.shape[2:]), tuple(c4.shape[2:]), (h5, w5), (h5 // 2, w5 // 2), (h5 // 4, w5 // 4)]
        if hw[1] != (2 * h5, 2 * w5) or hw[0] != (4 * h5, 4 * w5) or hw[4][0] < 1 or hw[4][1] < 1:
            raise FdError("MNFCOS FPN: H and W must be multiples of 32 and at least 128")
        for m, t in ((self.C3PW, c3), (self.C4PW, c4), (self.C5PW, c5)):
            if not T._dense_ok(m, t):
                raise FdError(f"MNFCOS FPN lateral {tuple(m.weight.shape)}: the HIP training nodes cover Cin % 32 == 0, Cout % 4 == 0, fp32")
        sg = [Segs.make(B, [h]) for h in hw]
        pool = lambda t, lv: T._PoolAddRows.apply(t, None, (B, hw[lv][0], hw[lv][1], 2, 2, 0))  # noqa: E731
        up_add = lambda t, lat, lv: T._UpAddRows.apply(t, lat, (B, hw[lv][0], hw[lv][1]))      # noqa: E731  (lv: the LOW-resolution level)
        p5 = T.mn_block_rows(self.MNB5, T.conv_rows(self.C5PW, T.to_rows(c5), sg[2]), sg[2])
        p4 = T.mn_block_rows(self.MNB4, up_add(p5, T.conv_rows(self.C4PW, T.to_rows(c4), sg[1]), 2), sg[1])
        p3 = T.mn_block_rows(self.MNB3, up_add(p4, T.conv_rows(self.C3PW, T.to_rows(c3), sg[0]), 1), sg[0])
        p6 = T.mn_block_rows(self.MNB6, pool(p5, 2), sg[3])
        p7 = T.mn_block_rows(self.MNB7, pool(p6, 3), sg[4])
        return tuple(T.from_rows(t, B, h, w) for t, (h, w) in zip((p3, p4, p5, p6, p7), hw))

    def forward(self, x):
        if self.training and self.hip_train:
            return self.train_forward(x)
        self._check_eval()
        return self._run_fpn(engine.build_mn_fpn, x)


class MNHeadFCOS(PlannedModule):
    hip_train = False       # opt-in training on the HIP autograd nodes (enable_training())

    def __init__(self, feature: int, num_class: int, prior: float = 0.01):
        super().__init__()
        self.class_num, self.prior = num_class, prior
        self.block1 = MNBlock(feature, feature, 3, 2, 2)
        self.block2 = MNBlock(feature, feature, 3, 2, 2)
        self.cls_conv = nn.Sequential(nn.Conv2d(feature, feature, kernel_size=3, padding=1, bias=False), nn.GroupNorm(32, feature), nn.SiLU(True))
        self.reg_conv = nn.Sequential(nn.Conv2d(feature, feature, kernel_size=3, padding=1, bias=False), nn.GroupNorm(32, feature), nn.SiLU(True))
        self.cls_logits = nn.Conv2d(feature, num_class, kernel_size=1)
        self.cnt_logits = nn.Conv2d(feature, 1, kernel_size=1)
        self.reg_pred = nn.Conv2d(feature, 4, kernel_size=1)
        nn.init.constant_(self.cls_logits.bias, -np.log((1 - prior) / prior))
        self.scale_exp = nn.ModuleList([ScaleExp(1.0) for _ in range(5)])

    def enable_training(self):
        _enable_blocks(self)
        return self

    def train_forward(self, inputs):
        """MNHeadFCOS.forward (MNFcos.py:285-297) as an autograd graph of HIP rows nodes.  The five levels share the head's weights, so they are
        one rows buffer and every layer is one launch over the whole pyramid, forward and backward: the two MNBlocks (their BatchNorm per level
        when it runs on batch statistics), the 3x3 + GroupNorm + SiLU towers, the 1x1 predictors zero-padded to 32 output channels (centre-ness
        and box regression share a launch: both read the regression tower); exp(reg * scale_i) per level."""
        for t in inputs:
            self._check_train_input(t)
        x0 = inputs[0]
        if len(inputs) != 5 or not all(T._gn_ok(g, x0) for g in (self.cls_conv[1], self.reg_conv[1])) or not all(
                T._dense_ok(m, x0, pad_out=True) for m in (self.cls_conv[0], self.reg_conv[0], self.cls_logits, self.cnt_logits, self.reg_pred)):
            raise FdError("MNHeadFCOS: the HIP training nodes cover five fp32 levels with feature % 32 == 0 and GroupNorm widths the rows kernels take")
        f, segs = T.pyramid_rows(inputs)
        f = T.mn_block_rows(self.block2, T.mn_block_rows(self.block1, f, segs), segs)
        c = T.groupnorm_rows(self.cls_conv[1], T.conv_rows(self.cls_conv[0], f, segs), segs, self.cls_conv[2])
        r = T.groupnorm_rows(self.reg_conv[1], T.conv_rows(self.reg_conv[0], f, segs), segs, self.reg_conv[2])
        return T.predictor_rows(self.cls_logits, self.reg_pred, self.cnt_logits, c, r, segs, self.scale_exp)

    def forward(self, inputs):
        if self.training and self.hip_train:
            return self.train_forward(inputs)
        self._check_eval()
        return self._run_head(engine.build_mn_head, inputs)


class MNFCOS(PlannedModule):
    """MNFCOS(in_channel [C5, C4, C3 widths], num_class, feature, freeze_bn) -- reference MNFcos.py:11-36."""

    hip_train = False       # opt-in training on the HIP autograd nodes (enable_training())

    def __init__(self, in_channel: List[int], num_class: int, feature: int, freeze_bn: bool = True):
        super().__init__()
        self.backbone = ResNet50v2()
        self.FeaturePyramidNetwork = LieghtWeightFeaturePyramid_old(in_channel, feature)
        self.head = MNHeadFCOS(feature, num_class, 0.01)
        self.backbone_freeze = freeze_bn
        if self.backbone_freeze:
            self.freeze_batchnorm()

    def _parts(self):
        return self.FeaturePyramidNetwork, engine.build_mn_fpn, engine.build_mn_head

    def enable_training(self, train_stem: bool = False):
        """Opt in to training on the HIP autograd nodes: hip_train on the model, its FPN, its head and every MNBlock.  By default the 7x7 stem (Cin = 3)
        is frozen here (backbone.freeze_stages(0): conv1 + bn1), as HalfInvertedStageFCOS freezes it at construction -- build the optimizer after this
        call.  `train_stem=True` keeps the reference's trainable set instead: the stem stays trainable and runs on the HIP node (backbone.hip_stem_train:
        the stem kernel forward, fd_stem7x7_bwd_weight_nhwc4 backward); nothing is frozen and nothing is warned about.  Returns self."""
        _enable_blocks(self)
        if train_stem:
            self.backbone.hip_stem_train = True
            return self
        if self.backbone.conv1.weight.requires_grad:
            import warnings
            warnings.warn("MNFCOS.enable_training() freezes the 7x7 stem (backbone.conv1 / bn1); pass train_stem=True to train it on the HIP node; "
                          "an optimizer built before this call holds a parameter that no longer receives a gradient", stacklevel=2)
        self.backbone.freeze_stages(0)
        return self

    def forward(self, x: torch.Tensor, events=None):
        if not self.training:
            return self._eval_forward(x, events)
        if not self.hip_train:
            raise FdError("MNFCOS is inference-only on the HIP path as constructed (as shipped the reference's own forward raises, "
                          "MNFcos.py:233-235 / modules.py:203,215); call model.eval(), or opt in to training on the HIP autograd nodes "
                          "with model.enable_training()")
        return self._train_forward(x)      # an autograd graph whose nodes are the HIP kernels, like HalfInvertedStageFCOS.forward
