"""The trainable 7x7 stem on the HIP path, measured: prints ONE JSON line.

  wgrad      fd_stem7x7_bwd_weight_nhwc4 alone (HIP events; with the ReLU mask and the folded scale, as the frozen-bn1 node calls it) at 16 x 512^2 and
             16 x 640^2: the bytes it must move (dy and y once, the [N][H][W][4] image once, the partial slabs written and read back), the fraction of the
             HBM peak (8.0 TB/s spec) that time corresponds to, and the EXECUTED MFMA FLOP/s (M = 64, N = 160 padded columns, K = the output pixels) against
             the 157.3 TFLOP/s fp32-MFMA peak
  segment    the whole stem segment, forward + backward -- conv1 + frozen bn1 + ReLU + max-pool and the gradient of conv1.weight for a given gradient of
             the pooled map -- on the HIP node (train_ops.stem_rows) against the same segment on stock PyTorch-ROCm ops, interleaved in one process
  step       the FCOS([2048, 1024, 512], 20, 256) training step (forward, targets, loss, backward, SGD) at 16 x 512^2 with enable_stem_training() and
             without it (the stock-op stem), interleaved

Method: warm-up, then `REPS` timed runs of a fixed number of launches / steps per variant, the variants alternating; median and spread (min .. max).

    python tools/time_stem_train.py [--reps 5] [--no-step]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd import train_ops as T  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import FCOS  # noqa: E402

DEV = "cuda:0"
HBM_PEAK, MFMA_F32_PEAK = 8.0e12, 157.3e12
B = 16


def _events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _stats(runs, unit="us"):
    return {unit: round(statistics.median(runs), 2), unit + "_min": round(min(runs), 2), unit + "_max": round(max(runs), 2)}


def time_wgrad(reps):
    res = []
    for S in (512, 640):
        rows = B * (S // 2) * (S // 2)
        x4 = torch.randn(B * S * S, 4, device=DEV)
        dy, y, scale = torch.randn(rows, 64, device=DEV), torch.randn(rows, 64, device=DEV), torch.rand(64, device=DEV) + 0.5
        ws = ops.stem7x7_wgrad_workspace(B, S, S, DEV)
        call = lambda: ops.stem7x7_wgrad(ops.Rows(x4), ops.Rows(dy), B, S, S, ops.Rows(y), scale, ws)       # noqa: E731
        plain = lambda: ops.stem7x7_wgrad(ops.Rows(x4), ops.Rows(dy), B, S, S, None, None, ws)             # noqa: E731
        for _ in range(10):
            call(), plain()
        runs, runs_p = [], []
        for _ in range(reps):
            runs.append(_events(call, 20))
            runs_p.append(_events(plain, 20))
        us = statistics.median(runs)
        nbytes = 2 * rows * 64 * 4 + x4.numel() * 4 + 2 * ws.numel() * 4
        flop = 2 * 64 * 160 * rows
        res.append({"input": S, "rows": rows, **_stats(runs), "no_mask": _stats(runs_p), "bytes": nbytes, "dy_bytes": rows * 64 * 4, "workspace_bytes": ws.numel() * 4,
                    "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), "executed_mfma_flop": flop,
                    "executed_tflops": round(flop / (us * 1e-6) / 1e12, 1), "mfma_f32_peak_fraction": round(flop / (us * 1e-6) / MFMA_F32_PEAK, 4)})
    return res


def time_segment(reps, S=512):
    torch.manual_seed(0)
    model = FCOS([2048, 1024, 512], 20, 256).to(DEV).train()
    trunk = model.backbone.trunk
    x = torch.randn(B, 3, S, S, device=DEV)
    gp = torch.randn(B, 64, S // 4, S // 4, device=DEV).contiguous(memory_format=torch.channels_last)

    def hip():
        trunk.conv1.weight.grad = None
        T.stem_rows(trunk, x).backward(gp)

    def stock():
        trunk.conv1.weight.grad = None
        F.max_pool2d(F.relu(trunk.bn1(trunk.conv1(x))), 3, 2, 1).backward(gp)

    for _ in range(5):
        hip(), stock()
    runs = {"hip": [], "stock": []}
    for _ in range(reps):
        runs["hip"].append(_events(hip, 10))
        runs["stock"].append(_events(stock, 10))
    return {"input": S, "hip": _stats(runs["hip"]), "stock": _stats(runs["stock"]),
            "hip_over_stock": round(statistics.median(runs["hip"]) / statistics.median(runs["stock"]), 3)}


def time_step(reps, S=512, steps=3):
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 3, S, S, device=DEV, generator=g)
    c = torch.rand(B, 8, 2, device=DEV, generator=g) * 400 + 50
    s = torch.rand(B, 8, 2, device=DEV, generator=g) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, S - 1)
    labels = torch.randint(1, 21, (B, 8), device=DEV, generator=g)
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 9999999]])
    crit = FCOSLoss("giou")
    torch.manual_seed(0)
    base = FCOS([2048, 1024, 512], 20, 256).to(DEV).train()
    variants = {}
    for name in ("hip_stem", "stock_stem"):
        m = copy.deepcopy(base)
        if name == "hip_stem":
            m.enable_stem_training()
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=1e-4)

        def step(m=m, opt=opt):
            opt.zero_grad(set_to_none=True)
            out = m(x)
            loss = crit([out, gen([out, gt, labels])])[-1]
            loss.backward()
            opt.step()
            return loss
        variants[name] = step
    strict, T.STRICT = T.STRICT, False              # (the stock-stem variant IS the documented fallback)
    try:
        for _ in range(3):
            for step in variants.values():
                step()
        torch.cuda.synchronize()
        runs = {k: [] for k in variants}
        for _ in range(reps):
            for k, step in variants.items():
                t = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                runs[k].append((time.perf_counter() - t) / steps * 1e3)
    finally:
        T.STRICT = strict
    return {"input": S, **{k: _stats(v, "ms") for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    _lib.lib()
    res = {"tool": "time_stem_train", "device": torch.cuda.get_device_name(0), "batch": B, "reps": args.reps}
    res["wgrad"] = time_wgrad(args.reps)
    res["segment"] = time_segment(args.reps)
    if not args.no_step:
        res["step"] = time_step(args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
