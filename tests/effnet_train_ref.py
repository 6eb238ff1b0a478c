"""Torch restatement, runnable in float64, of the EfficientNet trunk in TRAIN mode as efficientnet_pytorch 0.7.1 runs it, and of FCOS on it: BatchNorm on
batch statistics (F.batch_norm(training=True) on clones of the running statistics, returned to the caller), the package's drop-connect from given uniform
numbers, and a stem that is part of the autograd graph.  With every switch off it is oracle.effnet_ref's eval-mode arithmetic, bit for bit.

TEST INFRASTRUCTURE ONLY.  State-dict keys and the block table are oracle.effnet_ref's."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import effnet_ref as E
from oracle import torch_ref as R

BN_MOMENTUM = 1.0 - 0.99


class Running:
    """Clones of the running statistics that the train-mode BatchNorms update: {prefix: (mean, var, updates)}."""

    def __init__(self):
        self.stats: Dict[str, list] = {}

    def get(self, sd, p):
        if p not in self.stats:
            self.stats[p] = [sd[p + ".running_mean"].detach().clone(), sd[p + ".running_var"].detach().clone(), 0]
        return self.stats[p]


def bn(sd, p: str, x: torch.Tensor, batch: bool, running: Optional[Running]) -> torch.Tensor:
    if not batch:
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, E.BN_EPS)
    st = running.get(sd, p)
    st[2] += 1
    return F.batch_norm(x, st[0], st[1], sd[p + ".weight"], sd[p + ".bias"], True, BN_MOMENTUM, E.BN_EPS)


def drop_scale(p: float, u: torch.Tensor, dtype) -> torch.Tensor:
    """efficientnet_pytorch.utils.drop_connect's per-sample factor from the uniform numbers u [B]: floor((1 - p) + u) / (1 - p)."""
    keep = 1.0 - p
    return torch.floor(keep + u.to(dtype)) / keep


def mbconv(sd, p: str, x, k, s, e, cin, cout, nominal, batch=False, running=None, scale=None):
    """oracle.effnet_ref.mbconv with BatchNorm on batch statistics when `batch`, and the branch scaled per sample by `scale` [B] before the skip add."""
    inputs = x
    if e != 1:
        x = E._swish(bn(sd, p + "._bn0", E._conv_same(sd, p + "._expand_conv", x, nominal), batch, running))
    x = E._swish(bn(sd, p + "._bn1", E._conv_same(sd, p + "._depthwise_conv", x, nominal, s, groups=x.shape[1]), batch, running))
    sq = F.adaptive_avg_pool2d(x, 1)
    sq = E._swish(F.conv2d(sq, sd[p + "._se_reduce.weight"], sd[p + "._se_reduce.bias"]))
    sq = F.conv2d(sq, sd[p + "._se_expand.weight"], sd[p + "._se_expand.bias"])
    x = torch.sigmoid(sq) * x
    x = bn(sd, p + "._bn2", E._conv_same(sd, p + "._project_conv", x, int(math.ceil(nominal / s))), batch, running)
    if s == 1 and cin == cout:
        if scale is not None:
            x = x * scale.view(-1, 1, 1, 1)
        x = x + inputs
    return x


def block_rates(name: str, rate: float):
    """Per block the drop probability the package uses, rate * idx / len(blocks), or 0.0 where the block has no skip connection."""
    _, blocks, _, _ = E.block_table(name)
    return [rate * i / len(blocks) if (s == 1 and cin == cout) else 0.0 for i, (k, s, e, cin, cout, nominal) in enumerate(blocks)]


def trunk(sd, x, name: str, prefix: str = "backbone.model.", train_stem: bool = False, batch_stats: bool = False, drop_rate: float = 0.0, drop_u=None,
          running: Optional[Running] = None):
    """[reduction_1 ... reduction_5] of the train-mode trunk.  train_stem: the stem is differentiated (else it runs under no_grad on its running
    statistics, as a frozen stem); batch_stats: every block BatchNorm, and the stem's when it trains, on batch statistics; drop_rate with drop_u
    [len(blocks), B]: drop-connect on the skip blocks."""
    _, blocks, _, res = E.block_table(name)
    if batch_stats and running is None:
        running = Running()

    def stem(x):
        return E._swish(bn(sd, prefix + "_bn0", E._conv_same(sd, prefix + "_conv_stem", x, res, 2), batch_stats and train_stem, running))

    if train_stem:
        x = stem(x)
    else:
        with torch.no_grad():
            x = stem(x)
    rates = block_rates(name, drop_rate)
    ends, prev = [], x
    for idx, (k, s, e, cin, cout, nominal) in enumerate(blocks):
        sc = drop_scale(rates[idx], drop_u[idx], x.dtype) if (rates[idx] > 0 and drop_u is not None) else None
        x = mbconv(sd, f"{prefix}_blocks.{idx}", x, k, s, e, cin, cout, nominal, batch_stats, running, sc)
        if prev.size(2) > x.size(2):
            ends.append(prev)
        elif idx == len(blocks) - 1:
            ends.append(x)
        prev = x
    return ends


def fcos_effnet_forward(sd, x, backbone_number: int, **kw):
    """oracle.effnet_ref.fcos_effnet_forward on the train-mode trunk (keywords of `trunk`)."""
    f = trunk(sd, x, E.VALID_MODELS[backbone_number], **kw)
    return R.fcos_head(sd, R.fcos_fpn(sd, f[2:]))
