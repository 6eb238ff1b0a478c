"""MNFCOS training on the HIP path, measured: prints ONE JSON line.

  wgrad      fd_dwconv_dilated_bwd_weight_nhwc alone (HIP events) at MNFCOS's real shapes -- C = 256, batch 16, 512 x 512 input: the five FPN
             blocks' (k, dilation) on their own level and the head's pyramid-wide block -- with the read-once byte count (x and dy, fp32)
             and the fraction of the HBM peak (8.0 TB/s spec) that time corresponds to
  step       the whole training step (forward, targets, loss, backward, SGD) of MNFCOS([2048, 1024, 512], 20, 256).enable_training(),
             fp32 and under autocast(float16) + GradScaler, in the default train mode (backbone BatchNorm frozen, FPN / head on batch statistics)
  stock      the same step with the model run through stock PyTorch-ROCm ops: oracle.torch_ref.mnfcos_forward on the device under autograd
             (the same BatchNorm modes, the same target / loss kernels, the same optimizer; the stem conv frozen as enable_training() does)

Method: 10 warm-up launches / 3 warm-up steps, then `REPS` timed runs of a fixed batch of launches / steps; the median and the spread
(min .. max) of the runs are reported, with the clocks rocm-smi shows before and after (read-only query, when the tool is there).

    python tools/time_mn_train.py [--reps 5] [--no-stock]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import torch_ref as R  # noqa: E402
from pytorch_object_detection_amd import ops  # noqa: E402
from pytorch_object_detection_amd._lib import Segs  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import MNFCOS  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
B, S, C = 16, 512, 256
LEVELS = [(S // s, S // s) for s in (8, 16, 32, 64, 128)]
WGRAD_SHAPES = [("MNB3", 3, 1, [LEVELS[0]]), ("MNB4", 3, 2, [LEVELS[1]]), ("MNB5", 5, 2, [LEVELS[2]]), ("MNB6", 5, 1, [LEVELS[3]]),
                ("MNB7", 7, 1, [LEVELS[4]]), ("head.block", 3, 2, LEVELS)]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception:
        return []


def time_wgrad(reps):
    res = []
    for name, k, dil, hw in WGRAD_SHAPES:
        segs = Segs.make(B, hw)
        x = torch.randn(segs.rows, C, device=DEV)
        dy = torch.randn(segs.rows, C, device=DEV)
        xr, dr = ops.Rows(x), ops.Rows(dy)
        n = 50
        for _ in range(10):
            ops.dwconv_dilated_wgrad(xr, dr, segs, k, dil, torch_layout=True)
        runs = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                ops.dwconv_dilated_wgrad(xr, dr, segs, k, dil, torch_layout=True)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / n)
        us = statistics.median(runs)
        nbytes = 2 * segs.rows * C * 4
        res.append({"layer": name, "k": k, "dil": dil, "rows": segs.rows, "us": round(us, 2), "us_min": round(min(runs), 2), "us_max": round(max(runs), 2),
                    "read_once_bytes": nbytes, "bound_us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 2), "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)})
    return res


def batch():
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 3, S, S, device=DEV, generator=g)
    c = torch.rand(B, 8, 2, device=DEV, generator=g) * 400 + 50
    s = torch.rand(B, 8, 2, device=DEV, generator=g) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, S - 1)
    labels = torch.randint(1, 21, (B, 8), device=DEV, generator=g)
    return x, gt, labels


def time_step(forward, params, amp, reps, steps=5):
    x, gt, labels = batch()
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")
    opt = torch.optim.SGD(params, lr=1e-4, momentum=0.9, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=amp)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = forward(x)
            out = tuple([t.float() for t in grp] for grp in out)
            losses = crit([out, gen([out, gt, labels])])
        scaler.scale(losses[-1]).backward()
        scaler.step(opt)
        scaler.update()
        return losses[-1]

    for _ in range(3):
        loss = step()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t) / steps * 1e3)
    ms = statistics.median(runs)
    return {"ms": round(ms, 2), "ms_min": round(min(runs), 2), "ms_max": round(max(runs), 2), "img_per_s": round(B / ms * 1e3, 1), "loss": round(float(loss), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-stock", action="store_true")
    args = ap.parse_args()
    res = {"tool": "time_mn_train", "device": torch.cuda.get_device_name(0), "batch": B, "input": S, "C": C, "reps": args.reps, "clocks_before": clocks()}
    res["wgrad"] = time_wgrad(args.reps)
    for amp in (False, True):
        torch.manual_seed(0)
        model = MNFCOS([2048, 1024, 512], 20, 256).enable_training().to(DEV).train()
        res["step_hip_amp" if amp else "step_hip_fp32"] = time_step(model, [p for p in model.parameters() if p.requires_grad], amp, args.reps)
        del model
    if not args.no_stock:
        R.BN_TRAIN_PREFIXES = ("FeaturePyramidNetwork.", "head.")           # the default train mode of the HIP step above
        for amp in (False, True):
            torch.manual_seed(0)
            model = MNFCOS([2048, 1024, 512], 20, 256).enable_training()
            frozen = {n for n, p in model.named_parameters() if not p.requires_grad} | {"backbone.extract_feature.conv1.weight", "backbone.conv1.weight"}
            sd = {k: v.to(DEV).requires_grad_(v.is_floating_point() and "running" not in k and k not in frozen and ".bn" not in k and "downsample.1" not in k)
                  for k, v in model.state_dict().items()}
            del model
            res["step_stock_amp" if amp else "step_stock_fp32"] = time_step(lambda x: R.mnfcos_forward(sd, x), [v for v in sd.values() if v.requires_grad], amp, args.reps)
            del sd
        R.BN_TRAIN_PREFIXES = ()
    res["clocks_after"] = clocks()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
