"""The ResNet-50 trunk on batch statistics (PlannedModule.enable_trunk_batch_stats), measured: prints ONE JSON line.

  launches   the bottleneck output relu(bn3(z) + identity) at the trunk's real block-output shapes for a 16 x 512 x 512 batch -- 16 * 128^2 x 256,
             16 * 64^2 x 512, 16 * 32^2 x 1024, 16 * 16^2 x 2048 -- two ways, ALTERNATING in the same process (every repetition times one batch of each):
               fused      fd_batchnorm_train_res_fwd_nhwc (statistics, then ONE apply pass that adds the residual and applies the ReLU)
               composed   ops.batchnorm_train_fwd with ACT_NONE, then ops.sample_scale_add with s = 1, then ops.act with ReLU
             with the bytes each moves over a [rows, C] fp32 map (fused: x twice, res, y = 4 passes; composed: 6 passes) and the fraction of the HBM peak
             (8.0 TB/s spec) its time corresponds to
  launches_f16   the f16-map forms against their fp32 twins at the same four shapes, again ALTERNATING in every repetition: the residual forward
             (fd_batchnorm_train_res_fwd_nhwc_h vs fd_batchnorm_train_res_fwd_nhwc: 4 map passes) and the backward (fd_batchnorm_train_bwd_nhwc_h vs
             fd_batchnorm_train_bwd_nhwc: x and dy twice, dx = 5 map passes), bytes at 2 resp. 4 per element, the HBM fraction of each and the ratio
  step       the whole HISFCOS-R50 training step (forward, targets, loss, backward, SGD) at 16 x 512 x 512, fp32 and under autocast(float16) + GradScaler:
               switch_on   bn_freeze=False, enable_stem_training().enable_trunk_batch_stats(): the trunk's BatchNorms on the HIP batch-statistics nodes
               switch_on_f16   the same with enable_trunk_batch_stats(f16_maps=True): f16 maps on those nodes (autocast only)
               switch_off  bn_freeze=False as it is without the switch: convs on HIP, stock nn.BatchNorm2d behind them, stock stem (strict mode off)
               frozen      the default model: frozen BatchNorm folded into the conv epilogues

Method: 10 warm-up launches / 3 warm-up steps, then `--reps` timed runs of a fixed batch of launches (HIP events) / steps (host clock around a device
synchronise); the median and the spread (min .. max) are reported, with the clocks rocm-smi shows before and after (read-only query, when the tool is there).

    python tools/time_resnet_bn_train.py [--reps 5] [--launches-only]
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
from pytorch_object_detection_amd import ops  # noqa: E402
from pytorch_object_detection_amd import train_ops  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
B, S = 16, 512
SHAPES = [("layer1 out 256 x 128^2", 256, 128), ("layer2 out 512 x 64^2", 512, 64), ("layer3 out 1024 x 32^2", 1024, 32), ("layer4 out 2048 x 16^2", 2048, 16)]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception:
        return []


def _time_alternating(fns, reps, n=50):
    """Several launches measured against each other: every repetition times one batch of n of each, in turn (HIP events)."""
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


def _row(name, form, C, rows, runs, passes, elt=4):
    us = statistics.median(runs)
    nbytes = passes * rows * C * elt
    return {"layer": name, "form": form, "C": C, "rows": rows, "us": round(us, 2), "us_min": round(min(runs), 2), "us_max": round(max(runs), 2),
            "map_passes": passes, "bytes": nbytes, "bound_us_at_hbm_peak": round(nbytes / HBM_PEAK * 1e6, 2),
            "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}


def time_launches(reps):
    res = []
    for name, C, H in SHAPES:
        rows = B * H * H
        x, r = torch.randn(rows, C, device=DEV), torch.randn(rows, C, device=DEV)
        y, t = torch.empty_like(x), torch.empty_like(x)
        gm, bt = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        one = torch.ones(B, device=DEV)
        xr, rr, yr, tr = (ops.Rows(v) for v in (x, r, y, t))
        ws = ops.batchnorm_train_workspace(rows, C, DEV)

        def fused():
            ops.batchnorm_train_res_fwd(xr, gm, bt, rr, yr, 1e-5, ops.ACT_RELU, 0.1, rm, rv, ws)

        def composed():
            ops.batchnorm_train_fwd(xr, gm, bt, tr, 1e-5, ops.ACT_NONE, 0.1, rm, rv, ws)
            ops.sample_scale_add(tr, one, rr, tr, B, H * H)
            ops.act(tr, yr, ops.ACT_RELU)

        fused()
        want = y.clone()
        composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(want, y))            # (one rounding of z + res either way: the two forms give the same bits)
        r_fused, r_comp = _time_alternating((fused, composed), reps)
        a, b = _row(name, "fused", C, rows, r_fused, 4), _row(name, "composed", C, rows, r_comp, 6)
        a["same_bits_as_composed"] = same
        res += [a, b]
    return res


def time_launches_f16(reps):
    """The `_h` residual forward and backward against the fp32 launches, alternating."""
    res = []
    for name, C, H in SHAPES:
        rows = B * H * H
        gm, bt = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        maps = {}
        for half in (False, True):
            dt = torch.float16 if half else torch.float32
            g = torch.Generator(device=DEV).manual_seed(C)
            x, r, dy = (torch.randn(rows, C, device=DEV, generator=g).to(dt) for _ in range(3))
            maps[half] = tuple(ops.Rows(v) for v in (x, r, dy, torch.empty_like(x), torch.empty_like(x)))
        ws = {half: (ops.batchnorm_train_workspace(rows, C, DEV), ops.batchnorm_train_workspace(rows, C, DEV)) for half in (False, True)}

        def fwd(half):
            xr, rr, _, yr, _ = maps[half]
            return lambda: ops.batchnorm_train_res_fwd(xr, gm, bt, rr, yr, 1e-5, ops.ACT_RELU, 0.1, rm, rv, ws[half][0])

        def bwd(half):
            xr, _, gr, _, dxr = maps[half]
            return lambda: ops.batchnorm_train_bwd(xr, gr, gm, bt, dxr, 1e-5, ops.ACT_NONE, ws[half][0], ws[half][1])

        for form, make, passes in (("res_fwd", fwd, 4), ("bwd", bwd, 5)):
            fns = (make(False), make(True))
            r32, r16 = _time_alternating(fns, reps)
            a, b = _row(name, form + " fp32", C, rows, r32, passes, 4), _row(name, form + " f16", C, rows, r16, passes, 2)
            b["fp32_over_f16"] = round(a["us"] / b["us"], 3)
            b["not_slower_than_fp32"] = b["us"] <= a["us"]
            res += [a, b]
    return res


def batch():
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 3, S, S, device=DEV, generator=g)
    c = torch.rand(B, 8, 2, device=DEV, generator=g) * 400 + 50
    s = torch.rand(B, 8, 2, device=DEV, generator=g) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, S - 1)
    labels = torch.randint(1, 21, (B, 8), device=DEV, generator=g)
    return x, gt, labels


def time_step(form, amp, reps, steps=3):
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256, bn_freeze=form == "frozen")
    if form in ("switch_on", "switch_on_f16"):
        model.enable_stem_training().enable_trunk_batch_stats(f16_maps=form == "switch_on_f16")
    model.to(DEV).train()
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

    train_ops.STATS["stock_fallbacks"] = 0
    for _ in range(3):
        loss = step()
    torch.cuda.synchronize()
    fallbacks_per_step = train_ops.STATS["stock_fallbacks"] // 3
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t) / steps * 1e3)
    ms = statistics.median(runs)
    return {"ms": round(ms, 2), "ms_min": round(min(runs), 2), "ms_max": round(max(runs), 2), "img_per_s": round(B / ms * 1e3, 1), "loss": round(float(loss.detach()), 4),
            "stock_fallbacks_per_step": fallbacks_per_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches-only", action="store_true")
    args = ap.parse_args()
    res = {"tool": "time_resnet_bn_train", "device": torch.cuda.get_device_name(0), "model": "HISFCOS-R50", "batch": B, "input": S, "reps": args.reps,
           "clocks_before": clocks()}
    res["launches"] = time_launches(args.reps)
    res["launches_f16"] = time_launches_f16(args.reps)
    if not args.launches_only:
        train_ops.STRICT = False        # the switch_off form runs stock BatchNorm behind the HIP convs: a counted fallback, an error under strict mode
        for form in ("switch_on", "switch_on_f16", "switch_off", "frozen"):
            for amp in (False, True):
                if form == "switch_on_f16" and not amp:
                    continue                # (without autocast the flag changes nothing: tests/test_resnet_bn_f16_gpu.py holds that bit for bit)
                res[f"step_{form}_{'amp' if amp else 'fp32'}"] = time_step(form, amp, args.reps)
                torch.cuda.empty_cache()
    res["clocks_after"] = clocks()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
