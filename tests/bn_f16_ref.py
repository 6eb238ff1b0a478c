"""What the f16-map batch-statistics BatchNorm kernels (fd_batchnorm_train_*_nhwc_h) compute, as code on the CPU: the f16 inputs are upcast exactly, the
batch-norm forward / residual forward / backward run in float64 on [rows, C] maps, and round_f16 rounds once, to nearest even, overflow becoming inf.
The kernels' own acceptance rule is bitwise against the fp32 kernels (tests/test_bn_f16_kernels_gpu.py); this restatement is the independent second
opinion, held against torch's CPU autograd by tests/test_bn_f16_cpu.py."""
import torch

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2


def upcast(t: torch.Tensor) -> torch.Tensor:
    """An f16 map as float64: every f16 value is a float64 value."""
    assert t.dtype == torch.float16
    return t.double()


def round_f16(t: torch.Tensor) -> torch.Tensor:
    """One rounding to f16, to nearest even; a magnitude beyond 65504 (+ half a step) becomes inf."""
    return t.to(torch.float16)


def _act(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    return z


def _act_grad(z, act):
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_SILU:
        sg = torch.sigmoid(z)
        return sg * (1 + z * (1 - sg))
    return torch.ones_like(z)


def stats(x64: torch.Tensor, eps: float):
    """(mean, rstd, biased variance) per channel of a float64 [rows, C] map."""
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    return mean, 1.0 / torch.sqrt(var + eps), var


def forward(x_h, gamma, beta, eps, act=ACT_NONE, res_h=None, rmean=None, rvar=None, momentum=0.1, mean_rstd=None):
    """float64 y = act((x - mean) * rstd * gamma + beta [+ res]) of the f16 map x_h (and f16 residual); with rmean / rvar also the running statistics
    after the momentum update with the UNBIASED variance.  mean_rstd: statistics given from outside (a SyncBatchNorm rank: the global ones).
    Returns (y64, mean, rstd, running_mean', running_var')."""
    x = upcast(x_h)
    mean, rstd, var = stats(x, eps)
    if mean_rstd is not None:
        mean, rstd = mean_rstd
    z = (x - mean) * rstd * gamma.double() + beta.double()
    if res_h is not None:
        z = z + upcast(res_h)
    rm = rv = None
    if rmean is not None:
        n = x.shape[0]
        rm = (1 - momentum) * rmean.double() + momentum * mean
        rv = (1 - momentum) * rvar.double() + momentum * var * n / (n - 1)
    return _act(z, act), mean, rstd, rm, rv


def backward(x_h, dy_h, gamma, beta, eps, act=ACT_NONE):
    """float64 (dx, dgamma, dbeta) of y = act(BatchNorm(x)) on batch statistics for the f16 maps x_h, dy_h.  The residual form's backward is this one with
    ACT_NONE on dy * [y > 0]."""
    x, dy = upcast(x_h), upcast(dy_h)
    mean, rstd, _ = stats(x, eps)
    xh = (x - mean) * rstd
    g = gamma.double()
    dz = dy * _act_grad(xh * g + beta.double(), act)
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    n = x.shape[0]
    dx = rstd * g * (dz - dbeta / n - xh * dgamma / n)
    return dx, dgamma, dbeta


def f16_ulp(ref64: torch.Tensor) -> torch.Tensor:
    """One f16 unit in the last place at |ref|, floor 2^-24 (the subnormal spacing): 2^(floor(log2 |ref|) - 10), at least 2^-24."""
    a = ref64.abs().clamp(min=2.0 ** -14)
    return torch.clamp(2.0 ** (torch.floor(torch.log2(a)) - 10), min=2.0 ** -24)
