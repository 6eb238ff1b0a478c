"""DeformableConv2d on the HIP path, measured: prints ONE JSON line.

For 16 x 80 x 80 x 256 -> 256 (the stride-8 level of a 640 x 640 input) and the stride-16 level (40 x 40), 3 x 3, stride 1, padding 1:

  im2col     fd_deform_im2col_nhwc alone (HIP events): algorithmic bytes (x read once, the side-conv buffer, the columns written) and the fraction
             of the HBM peak (8.0 TB/s spec) that time corresponds to
  bwd        fd_deform_bwd_nhwc alone, with the d_x scatter and without it: algorithmic bytes (dcols and x read once, d_offset / d_mask / d_x written
             once), the bytes its atomics add (four corners per sample), and the HBM fraction
  cols_bytes the size of the columns buffer (9 x the input map): written and read once forward, and again backward
  layer      the whole layer (side convs, sampler, GEMM) forward under no_grad, and forward + backward, fp32
  conv3x3    the same for a plain 3 x 3 conv (conv_rows) of that shape, for scale

Method: 10 warm-up launches / 3 warm-up passes, then `--reps` timed runs of a fixed batch of launches / passes; median and spread (min .. max).

    python tools/time_deform.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd import ops, train_ops as T  # noqa: E402
from pytorch_object_detection_amd.model.modules.modules import DeformableConv2d  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
B, C, COUT, K = 16, 256, 256, 3
LEVELS = [("stride8", 80, 80), ("stride16", 40, 40)]


def events(fn, reps, n=20):
    for _ in range(10):
        fn()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / n)
    return runs


def launch_entry(runs, nbytes, **extra):
    us = statistics.median(runs)
    return {"us": round(us, 2), "us_min": round(min(runs), 2), "us_max": round(max(runs), 2), "algorithmic_bytes": nbytes,
            "bound_us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 2), "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), **extra}


def wall(fn, reps, n=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t) / n * 1e3)
    return {"ms": round(statistics.median(runs), 3), "ms_min": round(min(runs), 3), "ms_max": round(max(runs), 3)}


def time_level(H, W, reps):
    g = torch.Generator(device=DEV).manual_seed(3)
    M, KK = B * H * W, K * K
    x = torch.randn(M, C, device=DEV, generator=g)
    om = torch.randn(M, 32, device=DEV, generator=g)          # the merged side conv's buffer: 18 offsets (a pixel or so), 9 modulator logits, 5 pad
    cols, dcols = torch.empty(M, KK * C, device=DEV), torch.randn(M, KK * C, device=DEV, generator=g)
    d_om, d_x = torch.empty(M, 32, device=DEV), torch.zeros(M, C, device=DEV)
    xr, off, mask = ops.Rows(x), ops.Rows(om, 0, 2 * KK), ops.Rows(om, 2 * KK, KK)
    d_off, d_mask = ops.Rows(d_om, 0, 2 * KK), ops.Rows(d_om, 2 * KK, KK)
    side = M * 27 * 4
    res = {"H": H, "W": W, "rows": M, "cols_bytes": cols.numel() * 4}
    res["im2col"] = launch_entry(events(lambda: ops.deform_im2col(xr, off, mask, ops.Rows(cols), B, H, W, K, 1, 1, 1, True), reps),
                                 x.numel() * 4 + side + cols.numel() * 4)
    res["bwd"] = launch_entry(events(lambda: ops.deform_bwd(ops.Rows(dcols), xr, off, mask, d_off, d_mask, ops.Rows(d_x), B, H, W, K, 1, 1, 1, True), reps),
                              dcols.numel() * 4 + 2 * x.numel() * 4 + 2 * side, atomic_bytes=4 * dcols.numel() * 4)
    res["bwd_no_dx"] = launch_entry(events(lambda: ops.deform_bwd(ops.Rows(dcols), xr, off, mask, d_off, d_mask, None, B, H, W, K, 1, 1, 1, True), reps),
                                    dcols.numel() * 4 + x.numel() * 4 + 2 * side)
    del cols, dcols, d_x, om, d_om

    torch.manual_seed(0)
    layer = DeformableConv2d(C, COUT, K, padding=1, bias=True).to(DEV)
    with torch.no_grad():
        for m in (layer.offset_conv, layer.modulator_conv):
            m.weight.normal_(std=0.01)
    conv = nn.Conv2d(C, COUT, K, padding=1, bias=True).to(DEV)
    xi = torch.randn(B, C, H, W, device=DEV, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_()

    def fwd(m):
        with torch.no_grad():
            return m(xi)

    def fwd_bwd(m):
        for p in m.parameters():
            p.grad = None
        xi.grad = None
        m(xi).sum().backward()

    res["layer"] = {"fwd": wall(lambda: fwd(layer), reps), "fwd_bwd": wall(lambda: fwd_bwd(layer), reps)}
    plain = lambda t: T.conv_bn_act(conv, None, t)      # noqa: E731
    res["conv3x3"] = {"fwd": wall(lambda: fwd(plain), reps), "fwd_bwd": wall(lambda: (setattr(xi, "grad", None), conv.zero_grad(), plain(xi).sum().backward()), reps)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {"tool": "time_deform", "device": torch.cuda.get_device_name(0), "batch": B, "C": C, "Cout": COUT, "K": K, "reps": args.reps}
    for name, H, W in LEVELS:
        res[name] = time_level(H, W, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
