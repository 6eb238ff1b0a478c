"""FCOS on EfficientNet-B3 (BASELINE Cfg5) training on the HIP path, measured: prints ONE JSON line.

  launches   fd_dwconv2d_bwd_data_nhwc and fd_dwconv2d_bwd_weight_nhwc alone (HIP events) at B3's real shapes for a 16 x 512 x 512 batch -- block 1
             (k3 s2 pad (0,1), 144 channels, 256^2 -> 128^2), the k5 s2 block at 816 channels (32^2 -> 16^2) and a k5 s1 block at 816 channels (32^2) --
             with the touch-once byte count (data gradient: dy read + dx written; weight gradient: x and dy read; fp32) and the fraction of the HBM
             peak (8.0 TB/s spec) that time corresponds to
  step       the whole training step (forward, targets, loss, backward, SGD) of FCOS([384, 136, 48], 20, 256, efficientnet=True,
             backbone_number=3).enable_training(), fp32 and under autocast(float16) + GradScaler
  stock      the same step in a child process started with FD_TRAIN_STOCK_CONV=1 (every layer on stock PyTorch-ROCm ops), for scale
  full       the launches and steps of enable_training(train_stem=True, batch_stats=True, drop_connect_rate=0.2) on a freeze_bn=False model:
             fd_batchnorm_train_fwd / _bwd on the 144-channel 256^2 map and on 816 x 32^2 (touch-once bytes: x read + y written; x and dy read + dx
             written -- the kernels read x, resp. x and dy, TWICE: statistics, then apply), fd_stem_conv_bwd_weight_nhwc4 at Cout 40 (x4 and dy read),
             fd_sample_scale_add_nhwc on a skip block's 48-channel 64^2 map held at 64 channels (branch and input read, output written); the whole
             fp32 / AMP step with the three switches on ("step_full_*"), HIP and stock (the stock trunk follows the same switches)
  sync       fd_batchnorm_train_sync_fwd / _bwd (SyncBatchNorm at these widths) on ONE device at the two BatchNorm shapes above: phase 1 then phase 2 back
             to back, no collective, timed in the same run as the unsynchronised launches and ALTERNATING with them ("launches_full_sync": per shape and
             direction an unsynchronised and a synchronised row, same warm-up, repetitions and median); --sync-only prints that section alone

Method: 10 warm-up launches / 3 warm-up steps, then `REPS` timed runs of a fixed batch of launches / steps; the median and the spread (min .. max) of
the runs are reported, with the clocks rocm-smi shows before and after (read-only query, when the tool is there).

    python tools/time_effnet_train.py [--reps 5] [--no-stock] [--sync-only]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

if "--steps-only" in sys.argv and "--stock" in sys.argv:
    os.environ["FD_TRAIN_STOCK_CONV"] = "1"          # read when the package is imported

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd import ops  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import FCOS  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
B, S = 16, 512
# (name, k, stride, (pad_before, pad_after), channels, input H = W)
SHAPES = [("blocks.2 k3 s2", 3, 2, (0, 1), 144, 256), ("blocks.18 k5 s2", 5, 2, (2, 2), 816, 32), ("blocks.14 k5 s1", 5, 1, (2, 2), 816, 32)]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception:
        return []


def _time(fn, reps, n=50):
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


def _time_alternating(fns, reps, n=50):
    """_time for several launches measured against each other: every repetition times one batch of n of each, in turn."""
    for fn in fns:
        for _ in range(10):
            fn()
    runs = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs[i].append(e0.elapsed_time(e1) * 1e3 / n)
    return runs


def time_launches(reps):
    res = []
    for name, k, s, pad, C, H in SHAPES:
        Ho = (H + pad[0] + pad[1] - k) // s + 1
        x = torch.randn(B * H * H, C, device=DEV)
        dy = torch.randn(B * Ho * Ho, C, device=DEV)
        dx = torch.empty_like(x)
        wkc = torch.randn(k * k, C, device=DEV)
        geo = (B, H, H, k, s, pad[0], pad[0], Ho, Ho)
        xr, gr, dr = ops.Rows(x), ops.Rows(dy), ops.Rows(dx)
        nbytes = (x.numel() + dy.numel()) * 4
        for what, fn in (("dgrad", lambda: ops.dwconv2d_dgrad(gr, wkc, dr, *geo)), ("wgrad", lambda: ops.dwconv2d_wgrad(xr, gr, *geo, torch_layout=True))):
            runs = _time(fn, reps)
            us = statistics.median(runs)
            res.append({"layer": name, "launch": what, "k": k, "stride": s, "pad": list(pad), "C": C, "in": H, "out": Ho, "us": round(us, 2),
                        "us_min": round(min(runs), 2), "us_max": round(max(runs), 2), "touch_once_bytes": nbytes,
                        "bound_us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 2), "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)})
    return res


def _row(name, launch, C, rows, runs, nbytes):
    us = statistics.median(runs)
    return {"layer": name, "launch": launch, "C": C, "rows": rows, "us": round(us, 2), "us_min": round(min(runs), 2), "us_max": round(max(runs), 2),
            "touch_once_bytes": nbytes, "bound_us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 2),
            "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}


def time_full_launches(reps):
    """The four launches the three switches add, at B3's real shapes for the 16 x 512 x 512 batch."""
    res = []
    for name, C, H in (("blocks.2 _bn0/_bn1 144 x 256^2", 144, 256), ("blocks.14 _bn0/_bn1 816 x 32^2", 816, 32)):
        rows, Cw = B * H * H, (C + 31) // 32 * 32
        x, dy = torch.randn(rows, Cw, device=DEV), torch.randn(rows, Cw, device=DEV)
        y, dx = torch.zeros_like(x), torch.zeros_like(x)
        gm, bt = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        xr, gr, yr, dr = (ops.Rows(t, 0, C) for t in (x, dy, y, dx))
        ws, ws2 = ops.batchnorm_train_workspace(rows, C, DEV), ops.batchnorm_train_workspace(rows, C, DEV)
        fwd = lambda: ops.batchnorm_train_fwd(xr, gm, bt, yr, 1e-3, ops.ACT_SILU, 0.01, rm, rv, ws)  # noqa: E731
        bwd = lambda: ops.batchnorm_train_bwd(xr, gr, gm, bt, dr, 1e-3, ops.ACT_SILU, ws, ws2)  # noqa: E731
        res.append(_row(name, "batchnorm_train_fwd", C, rows, _time(fwd, reps), 2 * rows * C * 4))
        res.append(_row(name, "batchnorm_train_bwd", C, rows, _time(bwd, reps), 3 * rows * C * 4))
    Ho, C0 = S // 2, 40
    x4 = torch.randn(B * S * S, 4, device=DEV)
    dy = torch.randn(B * Ho * Ho, 64, device=DEV)
    sc = torch.rand(C0, device=DEV) + 0.5
    gr = ops.Rows(dy, 0, C0)
    runs = _time(lambda: ops.stem_conv3_wgrad(x4, gr, B, S, S, 3, 2, 0, 0, Ho, Ho, sc), reps, n=20)
    res.append(_row("_conv_stem 3 -> 40, 512^2 -> 256^2", "stem_conv_bwd_weight", C0, B * Ho * Ho, runs, (x4.numel() + B * Ho * Ho * C0) * 4))
    HW, C = 64 * 64, 64
    a, r, y = (torch.randn(B * HW, C, device=DEV) for _ in range(3))
    s = torch.tensor([0.0, 1.25] * (B // 2), device=DEV)
    runs = _time(lambda: ops.sample_scale_add(ops.Rows(a), s, ops.Rows(r), ops.Rows(y), B, HW), reps)
    res.append(_row("blocks.6 skip 48 (held at 64) x 64^2", "sample_scale_add", C, B * HW, runs, 3 * B * HW * C * 4))
    return res


def time_sync_launches(reps):
    """The synchronised form of the batch-statistics BatchNorm on one device (phase 1, phase 2, no collective in between; the global count read from
    sums[2C] on the device as the autograd node does) against the unsynchronised launch at the same shape, alternating in one run."""
    res = []
    for name, C, H in (("blocks.2 _bn0/_bn1 144 x 256^2", 144, 256), ("blocks.14 _bn0/_bn1 816 x 32^2", 816, 32)):
        rows, Cw = B * H * H, (C + 31) // 32 * 32
        x, dy = torch.randn(rows, Cw, device=DEV), torch.randn(rows, Cw, device=DEV)
        y, dx = torch.zeros_like(x), torch.zeros_like(x)
        gm, bt = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        xr, gr, yr, dr = (ops.Rows(t, 0, C) for t in (x, dy, y, dx))
        ws, ws2 = ops.batchnorm_train_workspace(rows, C, DEV), ops.batchnorm_train_workspace(rows, C, DEV)
        sums, bsums = (torch.zeros(2 * C + 1, dtype=torch.float64, device=DEV) for _ in range(2))
        sums[2 * C], bsums[2 * C] = float(rows), float(rows)
        fwd = lambda: ops.batchnorm_train_fwd(xr, gm, bt, yr, 1e-3, ops.ACT_SILU, 0.01, rm, rv, ws)  # noqa: E731
        bwd = lambda: ops.batchnorm_train_bwd(xr, gr, gm, bt, dr, 1e-3, ops.ACT_SILU, ws, ws2)  # noqa: E731

        def sync_fwd():
            ops.batchnorm_train_sync_fwd(1, xr, sums, act_id=ops.ACT_SILU, ws=ws)
            ops.batchnorm_train_sync_fwd(2, xr, sums, gm, bt, yr, 1e-3, ops.ACT_SILU, -1.0, 0.01, rm, rv, ws=ws)

        def sync_bwd():
            ops.batchnorm_train_sync_bwd(1, xr, gr, gm, bt, bsums, ws, None, dg, db, 1e-3, ops.ACT_SILU, ws=ws2)
            ops.batchnorm_train_sync_bwd(2, xr, gr, gm, bt, bsums, ws, dr, None, None, 1e-3, ops.ACT_SILU, -1.0, ws=ws2)

        r_fwd, r_sfwd = _time_alternating((fwd, sync_fwd), reps)
        r_bwd, r_sbwd = _time_alternating((bwd, sync_bwd), reps)
        res.append(_row(name, "batchnorm_train_fwd", C, rows, r_fwd, 2 * rows * C * 4))
        res.append(_row(name, "batchnorm_train_sync_fwd (phase 1 + 2)", C, rows, r_sfwd, 2 * rows * C * 4))
        res.append(_row(name, "batchnorm_train_bwd", C, rows, r_bwd, 3 * rows * C * 4))
        res.append(_row(name, "batchnorm_train_sync_bwd (phase 1 + 2)", C, rows, r_sbwd, 3 * rows * C * 4))
    return res


def batch():
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 3, S, S, device=DEV, generator=g)
    c = torch.rand(B, 8, 2, device=DEV, generator=g) * 400 + 50
    s = torch.rand(B, 8, 2, device=DEV, generator=g) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, S - 1)
    labels = torch.randint(1, 21, (B, 8), device=DEV, generator=g)
    return x, gt, labels


def time_step(amp, reps, steps=5, full=False):
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = FCOS([384, 136, 48], 20, 256, freeze_bn=not full, efficientnet=True, backbone_number=3)
        model = (model.enable_training(train_stem=True, batch_stats=True, drop_connect_rate=0.2) if full else model.enable_training()).to(DEV).train()
    x, gt, labels = batch()
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=amp)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = model(x)
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
    ap.add_argument("--sync-only", action="store_true", help="time the synchronised BatchNorm launches against the unsynchronised ones only")
    ap.add_argument("--steps-only", action="store_true", help="(internal) time the two steps only and print them")
    ap.add_argument("--stock", action="store_true", help="(internal, with --steps-only) the child process that runs with FD_TRAIN_STOCK_CONV=1")
    args = ap.parse_args()
    if args.steps_only:
        print(json.dumps({"fp32": time_step(False, args.reps), "amp": time_step(True, args.reps),
                          "full_fp32": time_step(False, args.reps, full=True), "full_amp": time_step(True, args.reps, full=True)}))
        return
    res = {"tool": "time_effnet_train", "device": torch.cuda.get_device_name(0), "model": "FCOS EfficientNet-B3", "batch": B, "input": S, "reps": args.reps,
           "clocks_before": clocks()}
    if args.sync_only:
        res["launches_full_sync"] = time_sync_launches(args.reps)
        res["clocks_after"] = clocks()
        print(json.dumps(res))
        return
    res["launches"] = time_launches(args.reps)
    res["step_hip_fp32"] = time_step(False, args.reps)
    res["step_hip_amp"] = time_step(True, args.reps)
    res["launches_full"] = time_full_launches(args.reps)
    res["launches_full_sync"] = time_sync_launches(args.reps)
    res["step_full_hip_fp32"] = time_step(False, args.reps, full=True)
    res["step_full_hip_amp"] = time_step(True, args.reps, full=True)
    if not args.no_stock:
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps-only", "--stock", "--reps", str(args.reps)], capture_output=True, text=True)
        if out.returncode != 0:
            raise SystemExit(f"the FD_TRAIN_STOCK_CONV=1 child failed ({out.returncode}):\n{out.stderr[-2000:]}")
        stock = json.loads(out.stdout.strip().splitlines()[-1])
        res["step_stock_fp32"], res["step_stock_amp"] = stock["fp32"], stock["amp"]
        res["step_full_stock_fp32"], res["step_full_stock_amp"] = stock["full_fp32"], stock["full_amp"]
    res["clocks_after"] = clocks()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
