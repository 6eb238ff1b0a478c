"""float64 reference of the project's modulated deformable convolution (include/fcosdet.h fd_deform_im2col_nhwc) in plain torch:
gather + weights, so autograd supplies every gradient (floor() is held constant; at an integer coordinate the derivative is the one on the
ly = 0 side; a fully outside sample gives zero to everything).  Also the seeded inputs test_deform_cpu.py / test_deform_gpu.py share."""
import torch

# (H, W, K, stride, pad): the smallest shapes at which the lane / channel mapping, the borders and the strides can go wrong
GEOMS = [(7, 10, 3, 1, 1), (7, 10, 3, 2, 1), (5, 6, 3, 1, 0), (6, 5, 5, 1, 2), (4, 4, 1, 1, 0), (1, 1, 3, 1, 1)]
BATCH = 2
INTEGER_GEOM = GEOMS[0]       # the one case run with whole-number offsets as well


def out_hw(H, W, K, stride, pad, dil=1):
    return (H + 2 * pad - dil * (K - 1) - 1) // stride + 1, (W + 2 * pad - dil * (K - 1) - 1) // stride + 1


def coords(offset, H, W, K, stride, pad, dil=1):
    """Sampling coordinates (y, x), each [B, K*K, Ho, Wo], of offset [B, 2*K*K, Ho, Wo] (channel 2t: row offset, 2t + 1: column offset)."""
    B, _, Ho, Wo = offset.shape
    t = torch.arange(K * K)
    base_y = (torch.arange(Ho) * stride - pad).view(1, 1, Ho, 1) + ((t // K) * dil).view(1, -1, 1, 1)
    base_x = (torch.arange(Wo) * stride - pad).view(1, 1, 1, Wo) + ((t % K) * dil).view(1, -1, 1, 1)
    return base_y.to(offset.dtype) + offset[:, 0::2], base_x.to(offset.dtype) + offset[:, 1::2]


def tap_classes(offset, H, W, K, stride, pad, dil=1):
    """Shares of the taps that are (fully outside, partially outside, fully inside the map)."""
    y, x = coords(offset.double(), H, W, K, stride, pad, dil)
    inside = (y > -1) & (y < H) & (x > -1) & (x < W)
    y0, x0 = torch.floor(y), torch.floor(x)
    full = inside & (y0 >= 0) & (y0 + 1 <= H - 1) & (x0 >= 0) & (x0 + 1 <= W - 1)
    n = float(inside.numel())
    return float((~inside).sum()) / n, float((inside & ~full).sum()) / n, float(full.sum()) / n


def deform_cols(x, offset, mask, K, stride, pad, dil=1):
    """x [B, C, H, W], offset [B, 2*K*K, Ho, Wo], mask [B, K*K, Ho, Wo] (activated) or None -> columns [B*Ho*Wo, K*K*C], tap major then channel."""
    B, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, K, stride, pad, dil)
    assert offset.shape == (B, 2 * K * K, Ho, Wo)
    xr = x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    y, xx = coords(offset, H, W, K, stride, pad, dil)
    inside = (y > -1) & (y < H) & (xx > -1) & (xx < W)
    y0, x0 = torch.floor(y).detach(), torch.floor(xx).detach()
    ly, lx = y - y0, xx - x0
    s = 0
    for dy, dx, wgt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
        cy, cx = y0 + dy, x0 + dx
        ok = inside & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long().reshape(B, -1, 1).expand(-1, -1, C)        # [B, K*K*Ho*Wo, C]
        s = s + (wgt * ok).reshape(B, -1, 1) * torch.gather(xr, 1, idx)
    s = s.reshape(B, K * K, Ho * Wo, C)
    if mask is not None:
        s = s * mask.reshape(B, K * K, Ho * Wo, 1)
    return s.permute(0, 2, 1, 3).reshape(B * Ho * Wo, K * K * C)


def deform_conv2d(x, offset, weight, bias=None, stride=1, padding=0, dilation=1, mask=None):
    """NCHW in and out; returns (output, columns)."""
    B, C, H, W = x.shape
    Cout, _, K, _ = weight.shape
    Ho, Wo = out_hw(H, W, K, stride, padding, dilation)
    cols = deform_cols(x, offset, mask, K, stride, padding, dilation)
    y = cols @ weight.permute(0, 2, 3, 1).reshape(Cout, -1).t()
    if bias is not None:
        y = y + bias
    return y.reshape(B, Ho, Wo, Cout).permute(0, 3, 1, 2), cols


SEEDS = (0, 1)      # the seeds the GPU tests use (kernel tests: 0, functional: 1); test_deform_cpu.py checks the offsets of both


def make_inputs(geom, C, seed=0, integer=False, B=BATCH):
    """Seeded fp32 CPU inputs of one geometry: x randn; offsets odd eighths in about +-3 -- exact in fp32, never on an integer coordinate -- or, with
    `integer`, whole numbers in [-3, 3] (the ly = 0 side); modulator logits randn."""
    H, W, K, stride, pad = geom
    Ho, Wo = out_hw(H, W, K, stride, pad)
    g = torch.Generator().manual_seed(1 + 1000 * seed + 17 * H + 5 * W + K + stride + pad)      # offsets and logits do not depend on C: the CPU checks hold for every width
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1000 * seed + C))
    if integer:
        offset = torch.randint(-3, 4, (B, 2 * K * K, Ho, Wo), generator=g).float()
    else:
        offset = (2 * torch.randint(-12, 12, (B, 2 * K * K, Ho, Wo), generator=g) + 1).float() / 8
    logits = torch.randn(B, K * K, Ho, Wo, generator=g)
    return x, offset, logits


def rows(t):
    """NCHW -> [B*H*W, C] rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
