"""float64 restatements of the layer ops of csrc/fd_layers.hip (forward and closed-form backward) on the CPU, and the channel-view
helpers of the view tests.  Maps are NHWC: one level is [B, H, W, C]; a pyramid in rows form is the levels' [B * H * W, C] blocks
concatenated level-major (fd_segs).  Nothing here needs a GPU except make_view / outside_untouched, which place tensors on it.

The backward formulas are written out (no autograd), so that tests/test_layer_ref_cpu.py can hold them against autograd as an independent
statement of the same maths."""
import torch

ACT_NONE, ACT_RELU, ACT_SILU, ACT_EXP, ACT_SIGMOID = 0, 1, 2, 3, 4
DEV = "cuda:0"


def f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


# ---------------------------------------------------------------------------------------------------- activations
def act_fwd(x, act, param=0.0):
    x = f64(x)
    if act == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    if act == ACT_EXP:
        return torch.exp(x * param)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-x))
    return x.clone()


def act_deriv(x, act, param=0.0):
    x = f64(x)
    if act == ACT_RELU:
        return (x > 0).to(torch.float64)
    if act == ACT_SILU:
        sg = 1.0 / (1.0 + torch.exp(-x))
        return sg * (1.0 + x * (1.0 - sg))
    if act == ACT_EXP:
        return param * torch.exp(x * param)
    if act == ACT_SIGMOID:
        sg = 1.0 / (1.0 + torch.exp(-x))
        return sg * (1.0 - sg)
    return torch.ones_like(x)


# ---------------------------------------------------------------------------------------------------- pyramids
def split_levels(rows, B, hw):
    """[sum B*H*W, C] -> list of [B, H, W, C] (views)."""
    out, m = [], 0
    for h, w in hw:
        out.append(rows[m:m + B * h * w].reshape(B, h, w, -1))
        m += B * h * w
    assert m == rows.shape[0]
    return out


def join_levels(levels):
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in levels], 0)


def over_levels(fn, rows, B, hw):
    return join_levels([fn(t) for t in split_levels(rows, B, hw)])


# ---------------------------------------------------------------------------------------------------- max-pool (+ add)
def pool_out(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def maxpool_fwd(x, k, s, pad, add=None):
    """nn.MaxPool2d(k, s, pad) on [B, H, W, C] (+ add in output geometry).  Returns (y, idx): idx = h * W + w of the FIRST maximum of each
    window in row-major scan order (a later tap replaces the running maximum only if strictly greater: maxpool_bwd_kernel's tie rule)."""
    x = f64(x)
    B, H, W, C = x.shape
    Ho, Wo = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    xp = torch.full((B, H + 2 * pad + s, W + 2 * pad + s, C), float("-inf"), dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    hh = torch.arange(Ho).view(1, Ho, 1, 1) * s - pad
    ww = torch.arange(Wo).view(1, 1, Wo, 1) * s - pad
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    idx = torch.zeros((B, Ho, Wo, C), dtype=torch.int64)
    for r in range(k):
        for c in range(k):
            cand = xp[:, r:r + s * Ho:s, c:c + s * Wo:s][:, :Ho, :Wo]
            take = cand > best
            best = torch.where(take, cand, best)
            idx = torch.where(take, ((hh + r) * W + (ww + c)).expand_as(idx), idx)
    y = best if add is None else best + f64(add)
    return y, idx


def maxpool_bwd(x, dy, k, s, pad):
    """dx[p] = sum of dy over the windows whose first maximum is p."""
    x, dy = f64(x), f64(dy)
    B, H, W, C = x.shape
    _, idx = maxpool_fwd(x, k, s, pad)
    dx = torch.zeros(B, H * W, C, dtype=torch.float64)
    dx.scatter_add_(1, idx.reshape(B, -1, C), dy.reshape(B, -1, C))
    return dx.reshape(B, H, W, C)


# ---------------------------------------------------------------------------------------------------- nearest x2 upsample (+ add)
def upsample2x_add(x, lat):
    x = f64(x)
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2) + f64(lat)


def upsample2x_bwd(dy):
    dy = f64(dy)
    B, H2, W2, C = dy.shape
    return dy.reshape(B, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4))


# ---------------------------------------------------------------------------------------------------- depthwise convs
def _dw_taps(H, W, K, dil, stride, pad_t, pad_l, Ho, Wo):
    """The zero-padded frame of a depthwise conv and, per tap, the slices of it that the Ho x Wo outputs read."""
    bot = max(0, (Ho - 1) * stride - pad_t + (K - 1) * dil - (H - 1))
    rgt = max(0, (Wo - 1) * stride - pad_l + (K - 1) * dil - (W - 1))
    Hp, Wp = pad_t + H + bot, pad_l + W + rgt
    taps = []
    for r in range(K):
        for c in range(K):
            taps.append((slice(r * dil, r * dil + (Ho - 1) * stride + 1, stride), slice(c * dil, c * dil + (Wo - 1) * stride + 1, stride)))
    return Hp, Wp, taps


def dwconv_fwd(x, w, K, dil=1, stride=1, pad_t=None, pad_l=None, Ho=None, Wo=None, scale=None, shift=None, act=ACT_NONE, pre=False):
    """Depthwise K x K on [B, H, W, C]; w [K*K, C] (tap-major, the packed layout).  Default geometry: stride 1, 'same' padding.
    z = conv * scale + shift, y = act(z); pre=True returns z."""
    x, w = f64(x), f64(w)
    B, H, W, C = x.shape
    if pad_t is None:
        pad_t = pad_l = dil * (K - 1) // 2
        Ho, Wo = H, W
    Hp, Wp, taps = _dw_taps(H, W, K, dil, stride, pad_t, pad_l, Ho, Wo)
    xp = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    z = torch.zeros(B, Ho, Wo, C, dtype=torch.float64)
    for t, (sh, sw) in enumerate(taps):
        z += xp[:, sh, sw] * w[t]
    if scale is not None:
        z = z * f64(scale)
    if shift is not None:
        z = z + f64(shift)
    return z if pre else act_fwd(z, act)


def dwconv_bwd(x, w, dy, K, dil=1, stride=1, pad_t=None, pad_l=None, scale=None, shift=None, act=ACT_NONE):
    """(dx, dw [K*K, C]) of dwconv_fwd w.r.t. x and w given dy (the gradient of y)."""
    x, w, dy = f64(x), f64(w), f64(dy)
    B, H, W, C = x.shape
    Ho, Wo = dy.shape[1:3]
    if pad_t is None:
        pad_t = pad_l = dil * (K - 1) // 2
    z = dwconv_fwd(x, w, K, dil, stride, pad_t, pad_l, Ho, Wo, scale, shift, pre=True)
    g = dy * act_deriv(z, act)
    if scale is not None:
        g = g * f64(scale)
    Hp, Wp, taps = _dw_taps(H, W, K, dil, stride, pad_t, pad_l, Ho, Wo)
    xp = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    dxp = torch.zeros_like(xp)
    dw = torch.zeros(K * K, C, dtype=torch.float64)
    for t, (sh, sw) in enumerate(taps):
        dxp[:, sh, sw] += g * w[t]
        dw[t] = (xp[:, sh, sw] * g).sum((0, 1, 2))
    return dxp[:, pad_t:pad_t + H, pad_l:pad_l + W].clone(), dw


def dwconv_wgrad_pyramid(x_rows, dy_rows, B, hw, K, dil, scale=None):
    """Weight gradient [K*K, C] of the stride-1 'same' depthwise conv over a pyramid given dy (no activation; `scale` multiplies per channel)."""
    dw = 0
    for x, dy in zip(split_levels(f64(x_rows), B, hw), split_levels(f64(dy_rows), B, hw)):
        dw = dw + dwconv_bwd(x, torch.zeros(K * K, x.shape[-1]), dy, K, dil)[1]
    return dw if scale is None else dw * f64(scale)


# ---------------------------------------------------------------------------------------------------- GroupNorm + act
def gn_stats(x, G, eps):
    """x [B, H, W, C] -> (mean, rstd) [B, G] over (H, W, C / G), biased variance."""
    x = f64(x)
    B, H, W, C = x.shape
    xg = x.reshape(B, H * W, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, G, 1)) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def _per_channel(stat, C):
    B, G = stat.shape
    return stat.repeat_interleave(C // G, 1).view(B, 1, 1, C)


def gn_fwd(x, gamma, beta, G, eps, act, stats=None):
    x = f64(x)
    C = x.shape[-1]
    mean, rstd = gn_stats(x, G, eps) if stats is None else stats
    return act_fwd((x - _per_channel(mean, C)) * _per_channel(rstd, C) * f64(gamma) + f64(beta), act)


def gn_bwd(x, dy, gamma, beta, G, eps, act):
    """(dx, dgamma, dbeta) of one level: dz = dy * act'(z); dgamma = sum dz * xhat, dbeta = sum dz (over images and pixels);
    dx = rstd * (dz gamma - mean_g(dz gamma) - xhat * mean_g(dz gamma xhat)) per image and group."""
    x, dy, gamma, beta = f64(x), f64(dy), f64(gamma), f64(beta)
    B, H, W, C = x.shape
    mean, rstd = gn_stats(x, G, eps)
    mean_c, rstd_c = _per_channel(mean, C), _per_channel(rstd, C)
    xh = (x - mean_c) * rstd_c
    dz = dy * act_deriv(xh * gamma + beta, act)
    dgamma, dbeta = (dz * xh).sum((0, 1, 2)), dz.sum((0, 1, 2))
    t = dz * gamma
    m1 = t.reshape(B, H * W, G, C // G).mean((1, 3))
    m2 = (t * xh).reshape(B, H * W, G, C // G).mean((1, 3))
    dx = rstd_c * (t - _per_channel(m1, C) - xh * _per_channel(m2, C))
    return dx, dgamma, dbeta


def gn_coef(x, gamma, beta, G, eps):
    """The per-(image, channel) affine (a, b) with GroupNorm(x) * gamma + beta = x * a + b: [B, C] each."""
    C = x.shape[-1]
    mean, rstd = gn_stats(x, G, eps)
    a = rstd.repeat_interleave(C // G, 1) * f64(gamma)
    return a, f64(beta) - mean.repeat_interleave(C // G, 1) * a


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
def se_fwd(x, w1, b1, w2, b2):
    """x [N, HW, C]; w1 [Cr, C], w2 [C, Cr].  y = x * sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2).  Returns (y, gate [N, C])."""
    x, w1, b1, w2, b2 = f64(x), f64(w1), f64(b1), f64(w2), f64(b2)
    m = x.mean(1)
    h = m @ w1.t() + b1
    g = act_fwd(act_fwd(h, ACT_SILU) @ w2.t() + b2, ACT_SIGMOID)
    return x * g.unsqueeze(1), g


def se_bwd(x, dy, w1, b1, w2, b2):
    """(dx, dw1, db1, dw2, db2)."""
    x, dy, w1, b1, w2, b2 = f64(x), f64(dy), f64(w1), f64(b1), f64(w2), f64(b2)
    HW = x.shape[1]
    m = x.mean(1)
    h = m @ w1.t() + b1
    s = act_fwd(h, ACT_SILU)
    g = act_fwd(s @ w2.t() + b2, ACT_SIGMOID)
    dz = (dy * x).sum(1) * g * (1.0 - g)            # [N, C]
    dh = (dz @ w2) * act_deriv(h, ACT_SILU)         # [N, Cr]
    dm = dh @ w1                                    # [N, C]
    dx = dy * g.unsqueeze(1) + dm.unsqueeze(1) / HW
    return dx, dh.t() @ m, dh.sum(0), dz.t() @ s, dz.sum(0)


# ---------------------------------------------------------------------------------------------------- BatchNorm (train) over ranks
def bn_sync_fwd(xs, gamma, beta, eps, act):
    """xs: one [rows_r, C] shard per rank.  Returns (ys, mean, biased var, total rows): statistics over ALL ranks' rows."""
    xs = [f64(x) for x in xs]
    allx = torch.cat(xs, 0)
    n = allx.shape[0]
    mean = allx.mean(0)
    var = ((allx - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return [act_fwd((x - mean) * rstd * f64(gamma) + f64(beta), act) for x in xs], mean, var, n


def bn_sync_bwd(xs, dys, gamma, beta, eps, act):
    """Per rank (dx, dgamma, dbeta): dgamma / dbeta from the rank's LOCAL sums of dz * xhat / dz, dx from the GLOBAL means:
    dx = rstd * (gamma dz - mean_all(gamma dz) - xhat * mean_all(gamma dz xhat))."""
    xs, dys, gamma, beta = [f64(x) for x in xs], [f64(d) for d in dys], f64(gamma), f64(beta)
    _, mean, var, n = bn_sync_fwd(xs, gamma, beta, eps, ACT_NONE)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhs = [(x - mean) * rstd for x in xs]
    dzs = [d * act_deriv(xh * gamma + beta, act) for d, xh in zip(dys, xhs)]
    m1 = sum((dz * gamma).sum(0) for dz in dzs) / n
    m2 = sum((dz * gamma * xh).sum(0) for dz, xh in zip(dzs, xhs)) / n
    return [(rstd * (dz * gamma - m1 - xh * m2), (dz * xh).sum(0), dz.sum(0)) for dz, xh in zip(dzs, xhs)]


def bn_running(rmean, rvar, mean, var, n, momentum):
    """nn.BatchNorm's update: the running variance takes the UNBIASED batch variance."""
    unbiased = var * n / (n - 1) if n > 1 else var
    return (1 - momentum) * f64(rmean) + momentum * mean, (1 - momentum) * f64(rvar) + momentum * unbiased


# ---------------------------------------------------------------------------------------------------- channel views
def make_view(t, co, tail, fill=float("nan")):
    """Put a [rows, C] tensor into a [rows, co + C + tail] device buffer whose other channels hold `fill`; returns (ops.Rows view, buffer)."""
    from pytorch_object_detection_amd import ops
    rows, C = t.shape
    buf = torch.full((rows, co + C + tail), fill, dtype=t.dtype, device=DEV)
    buf[:, co:co + C] = t.to(DEV)
    return ops.Rows(buf, co, C), buf


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def outside_untouched(buf, co, C, before, rows=None):
    """Bitwise: every element of `buf` outside the view's channels [co, co + C) of its first `rows` rows (default: all) equals `before`."""
    same = bits(buf) == bits(before)
    same[:buf.shape[0] if rows is None else rows, co:co + C] = True
    return bool(same.all())


def unchanged(buf, before):
    return bool((bits(buf) == bits(before)).all())
