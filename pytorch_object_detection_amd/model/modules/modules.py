"""Layers used by HISFCOS (reference model/modules/modules.py:40-49,65-73,107-121,170-176) under the reference's names.
Inside a detector their arithmetic is fused into the HIP plan (engine.py) or the rows-based training forward; called on
their own -- the reference exposes them as ordinary layers -- `forward` runs the same HIP kernels (C-ABI), forward and
backward, and raises FdError for a configuration the kernels do not cover: there is no silent stock-op fallback."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..._lib import FdError


def _layer_conv(m: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """m(x) on the HIP kernels: dense convs (Cin % 32 == 0) and depthwise 3x3 stride 1 with autograd (train_ops nodes);
    other depthwise shapes (k in {3,5,7}, stride 1 / 2, padding k//2) without a backward.  Padding rule (train_ops._dense_ok): dense convs take any
    symmetric zero padding -- an int, 'valid' (= 0), or 'same' with dilation * (k - 1) even; a 'same' that torch pads asymmetrically (an even kernel at an
    odd dilation) raises FdError, as does every other module the kernels do not cover.  A tensor of another shape than m(x) is never returned."""
    from ... import ops, train_ops as T
    T._need_cuda(x)
    if T._STOCK:
        return nn.Conv2d.forward(m, x)           # FD_TRAIN_STOCK_CONV=1: the explicit stock-op diagnostic mode
    if (m.groups == 1 and T._dense_ok(m, x)) or T._dw_ok(m, x):
        return T.conv_bn_act(m, None, x)
    k, s = m.kernel_size[0], m.stride[0]
    if (m.groups == m.in_channels == m.out_channels and m.in_channels % 4 == 0 and T._square(m) and k in (3, 5, 7) and s in (1, 2)
            and m.dilation == (1, 1) and T._pad_of(m) == k // 2 and x.dtype == torch.float32):
        if torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad):
            raise FdError("this depthwise shape has a HIP forward only (backward: 3x3 stride 1); run it under torch.no_grad()")
        B, C, H, W = x.shape
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        xr = T.to_rows(x).contiguous()
        y = torch.empty(B * Ho * Wo, C, dtype=torch.float32, device=x.device)
        ops.dwconv2d(ops.Rows(xr), ops.pack_dwk_weight(m.weight), ops.Rows(y), B, H, W, k, s, p, p, Ho, Wo,
                     None, m.bias.detach() if m.bias is not None else None)
        return T.from_rows(y, B, Ho, Wo)
    raise FdError(f"{type(m).__name__}{tuple(m.weight.shape)}: not covered by the HIP kernels (dense: Cin % 32 == 0, Cout % 4 == 0, "
                  "square kernel, symmetric zero padding, fp32; depthwise: C % 4 == 0, k in {3,5,7}, stride 1 / 2, padding k//2)")


class DepthWiseConv2d(nn.Conv2d):
    def __init__(self, in_channel: int, kernel: int, st: int = 1, bs: bool = False):
        super().__init__(in_channel, in_channel, kernel, st, kernel // 2, groups=in_channel, bias=bs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _layer_conv(self, x)


class PointWiseConv(nn.Conv2d):
    def __init__(self, in_channel: int, out_channel: int, kernel: int = 1, st: int = 1, bs: bool = False):
        super().__init__(in_channel, out_channel, kernel, st, kernel // 2, bias=bs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _layer_conv(self, x)


class SEBlock(nn.Module):
    """x * sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2); excitation.{0,2} are the two 1x1 convs (fd_se_scale_nhwc / _bwd)."""

    def __init__(self, n_in: int, r: int = 4):
        super().__init__()
        self.squeeze = nn.AdaptiveAvgPool2d(1)
        self.excitation = nn.Sequential(nn.Conv2d(n_in, n_in // r, 1), nn.SiLU(), nn.Conv2d(n_in // r, n_in, 1),
                                        nn.Sigmoid())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ... import train_ops as T
        T._need_cuda(x)
        if not T._se_ok(self, x) and not T._STOCK:
            raise FdError("SEBlock: not covered by the HIP kernels (C % 4 == 0, C <= 4096, C/r <= 1024, fp32)")
        if T._STOCK:
            return x * self.excitation(self.squeeze(x))
        B, _, H, W = x.shape
        return T.from_rows(T.se_rows(self, T.to_rows(x), B, H * W), B, H, W)


class ScaleExp(nn.Module):
    """exp(x * scale): fused into the reg_pred conv epilogue (FD_ACT_EXP) inside the detector plans; on its own an
    elementwise HIP launch (fd_act_nhwc) when no gradient is needed, plain tensor ops when one is (the scale is trainable)."""

    def __init__(self, init_value: float = 1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor([init_value], dtype=torch.float32))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ... import ops, train_ops as T
        T._need_cuda(x)
        if torch.is_grad_enabled() and (x.requires_grad or self.scale.requires_grad) or x.dtype != torch.float32 or x.shape[1] % 4:
            return torch.exp(x * self.scale)
        B, C, H, W = x.shape
        xr = T.to_rows(x).contiguous()
        y = torch.empty_like(xr)
        ops.act(ops.Rows(xr), ops.Rows(y), ops.ACT_EXP, float(self.scale.detach()))
        return T.from_rows(y, B, H, W)


class MNBlock(nn.Module):
    """x + PW2(SiLU(PW1(BN(dilated depthwise k x k (x))))) -- reference model/modules/modules.py:195-216, the block MNFCOS is built from
    (model/od/MNFcos.py:222-297).  As shipped the reference pads the depthwise conv with `dilated`, which keeps the map size only for
    k = 3, so its own residual add raises for the k = 5 / 7 blocks; here the padding is 'same' (dilated * (kernel - 1) / 2): identical
    for k = 3, the evident intent for 5 / 7.  Inside a detector plan the block is three HIP launches (engine.add_mn_block); called on
    its own (eval, no gradient) it runs the same launches.

    Training is opt-in: with `hip_train = True` (set by `enable_training()` of MNFCOS / its FPN / its head, or directly) a forward in
    train() -- or one that wants a gradient -- builds an autograd graph of HIP rows nodes (train_ops.mn_block_rows: the dilated depthwise
    conv with its data and weight gradient kernels, BatchNorm folded when frozen or on batch statistics, the two 1x1 convs, SiLU)."""

    hip_train = False

    def __init__(self, in_ch: int, out_ch: int, kernel: int, dilated: int, alpha: int = 1):
        super().__init__()
        self.DilatedDepthWiseConv = nn.Conv2d(in_ch, in_ch, kernel, 1, dilated * (kernel - 1) // 2, dilated, in_ch, False)
        self.BN = nn.BatchNorm2d(in_ch)
        self.PW1 = nn.Conv2d(in_ch, in_ch * alpha, 1, 1, 0, 1, 1, True)
        self.ACT1 = nn.SiLU(True)
        self.PW2 = nn.Conv2d(in_ch * alpha, out_ch, 1, 1, 0, 1, 1, True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ... import engine, train_ops as T
        from ..._lib import Segs
        T._need_cuda(x)
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or self.PW1.weight.requires_grad)):
            if not self.hip_train:
                raise FdError("MNBlock has a HIP forward only (MNFCOS is inference-only on the HIP path): call .eval() and run it under torch.no_grad(), "
                              "or opt in to the HIP training nodes with hip_train = True (MNFCOS.enable_training())")
            B, C, H, W = x.shape
            return T.from_rows(T.mn_block_rows(self, T.to_rows(x), Segs.make(B, [(H, W)])), B, H, W)
        if x.dtype != torch.float32 or x.shape[1] % 4 or self.PW2.weight.shape[0] != x.shape[1]:
            raise FdError("MNBlock: fp32 input with C % 4 == 0 and out_ch == in_ch (the residual add) expected")
        B, C, H, W = x.shape
        plan = engine.Plan(x.device)
        segs = Segs.make(B, [(H, W)])
        xin, out = plan.pool.get(B * H * W, C), plan.pool.get(B * H * W, C)
        engine.add_mn_block(plan, "MNBlock", self, xin, segs, out)
        xin.tensor().view(B, H, W, C).copy_(x.permute(0, 2, 3, 1))
        plan.run()
        return out.tensor().view(B, H, W, C).permute(0, 3, 1, 2).clone()


def _nhwc_rows(t: torch.Tensor) -> torch.Tensor:
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, Cc)


def deform_conv2d(input: torch.Tensor, offset: torch.Tensor, weight: torch.Tensor, bias=None, stride=1, padding=0, dilation=1, mask=None) -> torch.Tensor:
    """Modulated deformable convolution (DCNv2) on the HIP kernels, with the argument order of torchvision.ops.deform_conv2d, which it stands in for
    (torchvision is not part of this stack).  NCHW in and out: input [B, Cin, H, W], offset [B, 2*K*K, Ho, Wo] (channel 2t = row offset, 2t + 1 = column
    offset of tap t = i*K + j), mask [B, K*K, Ho, Wo] (already activated) or None, weight [Cout, Cin, K, K], bias [Cout] or None.  The sampling rule is
    stated in include/fcosdet.h (fd_deform_im2col_nhwc) and DESIGN 4.3f.  Differentiable in input, offset, mask, weight and bias; the input gradient is
    summed with fp32 atomics and is not bit-reproducible, everything else is.  Coverage: Cin % 32 == 0, square kernel, groups = offset_groups = 1,
    1 <= K <= 7, 1 <= stride, dilation <= 4, 0 <= padding <= 7, fp32 CUDA tensors; anything else raises FdError."""
    from ... import ops, train_ops as T
    for t in (input, offset, weight, bias, mask):
        if t is not None:
            T._need_cuda(t)

    def one(v, what):
        if isinstance(v, (tuple, list)):
            if len(v) != 2 or v[0] != v[1]:
                raise FdError(f"deform_conv2d: {what} must be the same in both directions (got {tuple(v)})")
            v = v[0]
        return int(v)

    s, p, d = one(stride, "stride"), one(padding, "padding"), one(dilation, "dilation")
    if input.dim() != 4 or offset.dim() != 4 or weight.dim() != 4 or (mask is not None and mask.dim() != 4):
        raise FdError("deform_conv2d: NCHW tensors expected")
    B, C, H, W = input.shape
    Cout, Cw, K, K2 = weight.shape
    if K != K2 or Cw != C:
        raise FdError(f"deform_conv2d: square kernel and groups = 1 expected (input has {C} channels, weight is {tuple(weight.shape)})")
    if not (1 <= K <= 7 and 1 <= s <= 4 and 0 <= p <= 7 and 1 <= d <= 4):
        raise FdError(f"deform_conv2d: 1 <= K <= 7, 1 <= stride <= 4, 0 <= padding <= 7, 1 <= dilation <= 4 expected (K={K} stride={s} padding={p} dilation={d})")
    Ho, Wo = ops.deform_out_hw(H, W, K, s, p, d)
    if tuple(offset.shape) != (B, 2 * K * K, Ho, Wo):
        raise FdError(f"deform_conv2d: offset must be {(B, 2 * K * K, Ho, Wo)} (offset_groups = 1), got {tuple(offset.shape)}")
    if mask is not None and tuple(mask.shape) != (B, K * K, Ho, Wo):
        raise FdError(f"deform_conv2d: mask must be {(B, K * K, Ho, Wo)}, got {tuple(mask.shape)}")
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise FdError(f"deform_conv2d: bias must be [{Cout}]")
    y = T.deform_conv_rows(_nhwc_rows(input), _nhwc_rows(offset), _nhwc_rows(mask) if mask is not None else None, weight, bias, B, H, W, s, p, d)
    return T.from_rows(y, B, Ho, Wo)


class DeformableConv2d(nn.Module):
    """Modulated deformable convolution layer of the reference (model/modules/modules.py:219-277; imported by model/od/MNFcos.py:6): offset_conv predicts
    2*K*K offsets per output pixel, modulator_conv K*K logits m, and regular_conv's weights are applied to the input sampled bilinearly at the offset tap
    positions, each tap weighted by 2 * sigmoid(m) (deform_conv2d above).  Same constructor, attributes and state-dict keys as the reference; both side
    convs start at zero, so a fresh layer computes the plain convolution.  forward runs on the HIP kernels with autograd (train_ops.deformable_conv2d:
    three launches forward), also under torch.autocast and inside a captured training step.  Coverage: in_channels % 32 == 0, square kernel, fp32
    parameters, a CUDA input; anything else raises FdError.  FD_TRAIN_STOCK_CONV=1 raises too: the stock-op form of this layer is torchvision's op, and
    torchvision is not part of this stack."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False):
        super().__init__()
        if isinstance(kernel_size, int):
            kernel_size = (kernel_size, kernel_size)
        if not isinstance(kernel_size, tuple):
            raise TypeError(f"kernel_size: an int or a tuple expected, got {type(kernel_size).__name__}")
        kk = kernel_size[0] * kernel_size[1]
        self.stride = stride if isinstance(stride, tuple) else (stride, stride)
        self.padding = padding
        self.offset_conv = nn.Conv2d(in_channels, 2 * kk, kernel_size=kernel_size, stride=stride, padding=self.padding, bias=True)
        self.modulator_conv = nn.Conv2d(in_channels, kk, kernel_size=kernel_size, stride=stride, padding=self.padding, bias=True)
        for side in (self.offset_conv, self.modulator_conv):
            nn.init.constant_(side.weight, 0.)
            nn.init.constant_(side.bias, 0.)
        self.regular_conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=self.padding, bias=bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ... import train_ops as T
        T._need_cuda(x)
        if T._STOCK:
            raise FdError("DeformableConv2d: FD_TRAIN_STOCK_CONV=1 has no stock op to route this layer to (torchvision.ops.deform_conv2d is not part of this stack)")
        m = self.regular_conv
        k = m.kernel_size
        if m.groups != 1 or self.offset_conv.groups != 1 or self.modulator_conv.groups != 1:
            raise FdError("DeformableConv2d: groups = 1 expected")
        if k[0] != k[1] or not (T._square(m) and T._square(self.offset_conv) and T._square(self.modulator_conv)):
            raise FdError(f"DeformableConv2d: square kernel, stride and padding expected (kernel {tuple(k)}, stride {tuple(m.stride)}, padding {m.padding})")
        if m.in_channels % 32 or x.dim() != 4 or x.shape[1] != m.in_channels:
            raise FdError(f"DeformableConv2d: in_channels % 32 == 0 and an NCHW input of that width expected (in_channels={m.in_channels}, input {tuple(x.shape)})")
        if self.offset_conv.out_channels != 2 * k[0] * k[0] or self.modulator_conv.out_channels != k[0] * k[0]:
            raise FdError(f"DeformableConv2d: offset_conv must have 2*K*K = {2 * k[0] * k[0]} output channels, modulator_conv K*K = {k[0] * k[0]}")
        if any(c.weight.dtype != torch.float32 for c in (m, self.offset_conv, self.modulator_conv)) or not T._f32(x):
            raise FdError("DeformableConv2d: fp32 parameters and an fp32 input (any float type under torch.autocast) expected")
        if not (1 <= k[0] <= 7 and 1 <= m.stride[0] <= 4 and 0 <= m.padding[0] <= 7) or m.dilation != (1, 1):
            raise FdError(f"DeformableConv2d: 1 <= K <= 7, 1 <= stride <= 4, 0 <= padding <= 7, dilation 1 expected (K={k[0]} stride={m.stride[0]} padding={m.padding[0]})")
        return T.deformable_conv2d(self, x)


def init_conv_random_normal(module: nn.Module, std: float = 0.01):
    if isinstance(module, nn.Conv2d):
        nn.init.normal_(module.weight, std=std)
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)


def init_conv_kaiming(module: nn.Module):
    if isinstance(module, nn.Conv2d):
        nn.init.kaiming_uniform_(module.weight, a=1)
        if module.bias is not None:
            nn.init.constant_(module.bias, 0)
