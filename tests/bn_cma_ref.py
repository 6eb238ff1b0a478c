"""Float64 restatement of nn.BatchNorm2d(momentum=None), the cumulative moving average of the running statistics, on [rows, C] maps -- the reference of
tests/test_update_bn_cpu.py (which holds it against torch), tests/test_bn_cma_kernels_gpu.py and tests/test_update_bn_gpu.py.

    per batch     mean, biased variance (what the forward normalises with), unbiased variance = biased * rows / (rows - 1) (what the running variance takes)
    recurrence    r_n = (1 - 1/n) r_{n-1} + (1/n) b_n,  n = 1, 2, ... = num_batches_tracked after its increment
    closed form   r_N = the arithmetic mean of b_1 .. b_N whatever r_0 was (the first step has factor 1)
"""
import torch


def batch_stats(x: torch.Tensor):
    """(mean, biased variance, unbiased variance) per channel of x [rows, C], float64."""
    x = x.double()
    rows = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, var * rows / (rows - 1)


def rows_of(x: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> [N * H * W, C]; a [rows, C] map passes."""
    return x if x.dim() == 2 else x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def cma_step(r: torch.Tensor, b: torch.Tensor, n: int) -> torch.Tensor:
    """One step of the recurrence with the counter at n >= 1 (already incremented)."""
    return (1.0 - 1.0 / n) * r.double() + (1.0 / n) * b.double()


def cma(batches, rm0: torch.Tensor, rv0: torch.Tensor):
    """(running_mean, running_var, num_batches_tracked) after the batches, from the recurrence, starting at (rm0, rv0, 0)."""
    rm, rv, n = rm0.double(), rv0.double(), 0
    for x in batches:
        mean, _, unbiased = batch_stats(rows_of(x))
        n += 1
        rm, rv = cma_step(rm, mean, n), cma_step(rv, unbiased, n)
    return rm, rv, n


def update_bn_ref(batches):
    """What update_bn leaves in one BatchNorm that saw `batches`: the arithmetic mean of the per-batch means and unbiased variances, and the batch count."""
    stats = [batch_stats(rows_of(x)) for x in batches]
    return torch.stack([s[0] for s in stats]).mean(0), torch.stack([s[2] for s in stats]).mean(0), len(stats)
