"""Time of recomputing the BatchNorm statistics (optim.update_bn) on HISFCOS-R50 with every BatchNorm on batch statistics; prints one JSON line.

    python tools/time_update_bn.py [--reps 5] [--batches 8] [--batch 16] [--size 512]

The model is HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats(); the loader is a list of
--batches fixed batches of --batch x 3 x --size x --size already on the device.  Two sequences in ONE run and alternating, each on a model of its own:
  ours    optim.update_bn(loader, model): momentum = None on the HIP batch-statistics kernels (the `_cma` entry points read num_batches_tracked on the device)
  stock   the only route before update_bn existed: torch.optim.swa_utils.update_bn(loader, model) with every layer on stock PyTorch-ROCm ops -- the
          FD_TRAIN_STOCK_CONV=1 switch, set here through train_ops._STOCK (the variable that environment switch initialises) around the call, because with
          momentum = None the HIP batch-statistics nodes refused the layer or fell back to stock BatchNorm
update_bn_ms          median (min .. max) wall time of one call over --reps repetitions, host clock around a device synchronise
forward_enqueue_ms    median host time of enqueueing ONE train-mode no_grad forward with momentum = None on every BatchNorm, not followed by a synchronise
launches_per_batch    ours: C-ABI launches of one batch inside update_bn, and of an ordinary float-momentum train forward (the two are equal)
No figure here is a pass / fail bar.  One rank only; EfficientNet is not measured.
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.optim import swa_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import ops, optim  # noqa: E402
from pytorch_object_detection_amd import train_ops as T  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return dt


class stock_ops:
    """Every layer on stock PyTorch-ROCm ops inside the block (what FD_TRAIN_STOCK_CONV=1 selects for a whole process)."""

    def __enter__(self):
        self.was, T._STOCK = T._STOCK, True

    def __exit__(self, *exc):
        T._STOCK = self.was


def summary(v):
    return {"median": round(median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_update_bn.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)

    def build():
        torch.manual_seed(0)
        return HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=False).enable_stem_training().enable_trunk_batch_stats().to(dev)

    ours, stock = build(), build()
    g = torch.Generator(device=dev).manual_seed(7)
    loader = [torch.randn(a.batch, 3, a.size, a.size, generator=g, device=dev) for _ in range(a.batches)]

    def run_ours():
        optim.update_bn(loader, ours)

    def run_stock():
        with stock_ops():
            swa_utils.update_bn(loader, stock)

    def forward_none(model):
        """One train-mode forward with momentum = None everywhere, as inside either update_bn."""
        bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        keep = [m.momentum for m in bns]
        for m in bns:
            m.momentum = None
        model.train()
        try:
            with torch.no_grad():
                return host_ms(lambda: model(loader[0]))
        finally:
            for m, k in zip(bns, keep):
                m.momentum = k

    # launches of one batch inside update_bn against an ordinary train forward (ours)
    ours.train()
    with torch.no_grad():
        ours(loader[0])
        at = ops.LAUNCHES[0]
        ours(loader[0])
        plain_launches = ops.LAUNCHES[0] - at
    at = ops.LAUNCHES[0]
    run_ours()
    cma_launches = (ops.LAUNCHES[0] - at) / a.batches
    run_stock()                                                # warm-up of the stock sequence (MIOpen's algorithm search)
    t_ours, t_stock, e_ours, e_stock = [], [], [], []
    for _ in range(a.reps):
        t_ours.append(wall_ms(run_ours))
        t_stock.append(wall_ms(run_stock))
        e_ours.append(forward_none(ours))
        with stock_ops():
            e_stock.append(forward_none(stock))
    rm_o = [m.running_mean for m in ours.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    rm_s = [m.running_mean for m in stock.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    print(json.dumps({
        "tool": "time_update_bn", "device": torch.cuda.get_device_name(0), "model": "HISFCOS-R50 bn_freeze=False, stem + trunk on batch statistics",
        "batches": a.batches, "batch": a.batch, "size": a.size, "reps": a.reps, "batchnorms": len(rm_o),
        "update_bn_ms": {"ours": summary(t_ours), "stock": summary(t_stock)},
        "forward_enqueue_ms": {"ours": summary(e_ours), "stock": summary(e_stock)},
        "launches_per_batch": {"update_bn": cma_launches, "float_momentum_forward": plain_launches},
        "speedup_median": round(median(t_stock) / median(t_ours), 3),
        # (a sanity figure, not a test: the two routes' first-layer statistics after the same loader)
        "stem_running_mean_max_abs_diff": float((rm_o[0] - rm_s[0]).abs().max()),
        "not_measured": ["more than one rank", "EfficientNet"]}))


if __name__ == "__main__":
    main()
