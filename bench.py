#!/usr/bin/env python3
"""bench.py — images/sec of HISFCOS-R50 640x640 inference on MI355X (BASELINE.json metric, configs[1]/[2]).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one batch of synthetic images already resident in HBM:
  model(x) [ResNet-50 trunk -> HIS FPN -> HIS head, all HIP kernels] -> FCOSHead (decode, top-1000, score >= 0.05,
  per-class NMS 0.6) -> ClipBoxes, plus (N > 1) one RCCL all-gather of the padded detections.
Per GPU: 16 images of 3x640x640 fp32 (weak scaling: the global batch is 16*N), 80 classes, random-init weights
with randomised BN statistics, seeded.  Rank 0 prints ONE JSON line (see DESIGN.md "Measurement").

A plain run sets up, warms up, times the K steps and prints the line.  --full adds every other measurement after the
timed region (per-kernel-family rooflines, parity against the CPU oracle, the f16x3 / mixed modes, the NMS and
post-process micro-benchmarks, the training-step diagnostic, the CPU baseline).  --dump-outputs DIR writes what the
last timed step returned as DIR/<name>.npy (float32 / float64), so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32, MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_HBM_GBS = 8000.0


def build_model(num_classes: int, seed: int, name: str = "HISFCOS"):
    from pytorch_object_detection_amd.model.od import FCOS, HalfInvertedStageFCOS
    torch.manual_seed(seed)
    if name == "FCOS":   # the baseline detector behind the same API; diagnostic, not the headline
        model = FCOS([2048, 1024, 512], num_classes, 256).eval()
    elif name == "MNFCOS":   # the detector the reference's config/main.yaml selects; diagnostic, not the headline
        from pytorch_object_detection_amd.model.od import MNFCOS
        model = MNFCOS([2048, 1024, 512], num_classes, 256).eval()
    elif name == "FCOS-B3":   # BASELINE configs[4]: EfficientNet-B3 trunk; diagnostic, not the headline
        model = FCOS([384, 136, 48], num_classes, 256, efficientnet=True, backbone_number=3).eval()
        gen = torch.Generator().manual_seed(seed + 2)
        for n, m in model.backbone.named_modules():   # variance-preserving init: torch's default drives 26 MBConv blocks to 1e-11
            if isinstance(m, torch.nn.Conv2d):
                fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                gain = 1.0 if "_se_" in n else (0.6 if "_project" in n else 3.2)
                with torch.no_grad():
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (gain / fan) ** 0.5)
    else:
        model = HalfInvertedStageFCOS([512, 1024, 2048], num_classes, 256).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.75)
    calibrate_head(model, seed)
    return model


def calibrate_head(model, seed: int) -> None:
    """Seeded scaling of the prediction layers so that the timed step does what a trained detector's step does.  At init the
    class logits are ~ -log(99) everywhere and the LTRB distances ~ exp(0) px: all 1000 candidates of an image pass the 0.05
    threshold with 2-pixel boxes and NMS suppresses nothing.  Here: class logits x 4 with a per-class bias spread (N(0, 2), seeded:
    a handful of classes dominate, as in a real image) and reg_pred.bias = 3.5 (LTRB distances ~ exp(1.2 * 3.5) = 67 px before the
    conv term), found with the CPU oracle on this model / these images: the NMS of the timed step then keeps ~ 25 % of its 1000
    candidates per image (`kept_mean` in the JSON line).  Conv work is unchanged (same shapes, dense weights)."""
    head = getattr(model, "head", None)
    if head is None or not hasattr(head, "cls_logits") or not hasattr(head, "reg_pred"):
        return
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        head.cls_logits.weight.mul_(4.0)
        head.cls_logits.bias.add_(torch.randn(head.cls_logits.bias.shape, generator=g) * 2.0)
        head.reg_pred.bias.fill_(3.5)


PMC_WORKLOAD = {"model": "HISFCOS", "batch": 16, "height": 640, "width": 640}     # what tools/pmc.sh runs (bench.py's defaults)


def pmc_traffic(workload: dict, kernel_hint: str = ""):
    """HBM bytes per launch of the roofline kernel from the separate rocprofv3 --pmc passes of this command
    (tools/pmc.sh -> tools/pmc_summary.py -> profiles/pmc_traffic.json): 2 x FETCH_SIZE (gfx950 reports half of a
    16-B/lane stream; calibrated on kernels of known byte count) + WRITE_SIZE.  (None, None) unless the recorded PMC run is THIS
    workload (model, batch, size: the passes are only ever made for bench.py's defaults) and the same kernel family: another model's
    or batch's traffic says nothing about this launch."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        rec = d.get("workload", PMC_WORKLOAD)
        if any(workload.get(k) != rec.get(k) for k in ("model", "batch", "height", "width")):
            return None, None
        if kernel_hint and kernel_hint not in d["head_tower_conv"]["kernel"]:
            return None, None
        return d["head_tower_conv"]["hbm_bytes_per_launch"], f"profiles/{d.get('tag', '?')}_pmc_summary.json"
    except Exception:
        return None, None


def tower_launch_share(plan) -> float:
    """Share of the head tower's work the TIMED launch does: 1.0, or -- when the plan runs the tower as whole rounds of workgroups + a tail launch
    (engine.TOWER_TAIL_SPLIT; the mark, and so the HIP events, cover the whole rounds) -- its share of the non-empty workgroups."""
    t = getattr(plan, "tail_of", {}).get(tower_mark_names(plan)[0])
    return float(t["main_share"]) if t else 1.0


def tower_mark_names(plan):
    """Names of the plan steps the 'head.tower3x3' mark covers (HISFCOS / MNFCOS: the fused cls_conv + reg_conv launch 'head.tower3x3'; FCOS: the fused first
    layer of its two 4-deep towers, 'head.tower0'): what the HIP events bracket, and so what the roofline object must describe."""
    lo, hi = plan.marks["head.tower3x3"]
    return [plan.names[i] for i in range(lo, hi)]


def tower_mark_flops(plan):
    """(algorithmic FLOPs, FLOPs executed on the matrix pipe) of the launches under the mark, from the plan's own per-step records."""
    lo, hi = plan.marks["head.tower3x3"]
    alg = sum(plan.step_flops.get(i, 0) for i in range(lo, hi))
    exe = sum(plan.step_flops.get(i, 0) / (plan.step_info[i].get("mfma_div", 1.0) if i in plan.step_info else 1.0) for i in range(lo, hi))
    return int(alg), int(exe)


def tower_roofline(plan, tower_ms: float, workload: dict, layer_ms=None) -> dict:
    """Roofline object of the dominant kernel: the launch(es) under the 'head.tower3x3' mark -- for HISFCOS the fused cls_conv + reg_conv 3x3 head tower (5 levels,
    one launch, HISFcos.py:196-204,224-225).  `achieved` / `frac` count the FLOPs the matrix pipe EXECUTES in the launch, over its HIP-event time, against the dense
    fp32-MFMA peak: on a Winograd kernel that is the direct convolution's count (2 * rows * Cout * Cin * 9) / 4 for F(4x4, 3x3) (36 multiplies per
    4x4 output tile and channel pair instead of 144) or / 2.25 for F(2x2, 3x3) -- so `frac` is a utilisation (<= 1, comparable with the PMC MFMA-busy counter).  The
    tile, the FLOP counts and the divisor are read from the plan records OF THE MARKED STEP (not from a fixed step name: FCOS names its launch head.tower0).  The
    algorithmic (direct-convolution) rate, which is what the layer delivers to the model, is `effective_tflops` / `effective_over_peak` (may exceed 1 on a Winograd
    kernel).  `layer_ms` / `layer_frac`: the WHOLE layer -- the marked launch plus its tail launch when the plan splits the grid (engine.TOWER_TAIL_SPLIT) -- timed on
    one stream with one batch in flight after the timed region (median of 5), full FLOPs: the figure comparable across rounds."""
    names = tower_mark_names(plan)
    lo, hi = plan.marks["head.tower3x3"]
    tile = plan.tiles.get(names[0], 0) & 0xFF
    wino, wino4 = tile == 14, tile == 16
    tower_flops, executed_flops = tower_mark_flops(plan)
    effective = tower_flops / (tower_ms * 1e-3) / 1e12
    achieved = executed_flops / (tower_ms * 1e-3) / 1e12
    info = plan.step_info.get(lo, {})
    what = f"{names[0]} ({info.get('Cin', '?')}>{info.get('Cout', '?')} 3x3, {plan.segs.nseg} levels" + (f", + {len(names) - 1} more launches under the mark" if len(names) > 1 else "") + ")"
    t = getattr(plan, "tail_of", {}).get(names[0])
    sk = getattr(plan, "sk_of", {}).get(names[0], 0)
    launch = None
    if t:
        what += f", workgroups [0, {t['main']}) of {t['workgroups']}"
        launch = (f"the layer runs as two launches of the same kernel: workgroups [0, {t['main']}) = {t['main'] // 256} whole rounds on 256 CUs (this launch: "
                  f"{100 * t['main_share']:.2f} % of the layer's {t['live']} non-empty workgroups, FLOPs counted pro rata) and a {t['workgroups'] - t['main']}-workgroup tail launch "
                  f"(plan step {names[0]}.tail, kernel instantiation TAG=0) beside which the other batch in flight runs (DESIGN 4.1k); layer_ms / layer_frac = both launches")
    elif sk:
        launch = (f"the whole layer in ONE launch of the persistent form: {sk} workgroups claim (tile block x 64 couts) items from a queue per XCD, the last partial "
                  "round of items is cut into pieces (fd_conv_params.sk_wgs, DESIGN 4.1m)")
    kern = ("conv3x3_wino4_kernel<TAG=1, SK>" if sk else "conv3x3_wino4_kernel<TAG=1>") if wino4 else ("conv3x3_wino_kernel<TAG=1>" if wino else "conv_igemm_kernel<...,TAG=1>")
    traffic, tsrc = pmc_traffic(workload, "wino4" if wino4 else ("wino_kernel" if wino else "igemm"))
    out = {"bound": "mfma", "launch": launch,
           "kernel": f"{kern} {what}: " + ("Winograd F(4x4,3x3), fp32" if wino4 else "Winograd F(2x2,3x3), fp32" if wino else f"direct implicit GEMM, tile id {tile}"),
           "instruction": "v_mfma_f32_32x32x2_f32", "achieved": round(achieved, 2),
           "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
           "traffic": traffic, "traffic_source": tsrc,
           "flops_basis": ("executed on the matrix pipe = direct-convolution FLOPs / 4 (Winograd F(4x4,3x3): 36 multiplies per 4x4 output tile "
                           "and channel pair instead of 144)" if wino4 else
                           "executed on the matrix pipe = direct-convolution FLOPs / 2.25 (Winograd F(2x2,3x3))" if wino
                           else "executed = algorithmic (direct convolution)"),
           "flops_per_launch": executed_flops, "algorithmic_flops_per_launch": tower_flops, "avg_launch_ms": round(tower_ms, 4),
           "effective_tflops": round(effective, 2), "effective_over_peak": round(effective / PEAK_F32_MFMA_TFLOPS, 4)}
    if layer_ms:
        div = tower_flops / executed_flops if executed_flops else 1.0
        full = tower_flops / t["main_share"] if t else tower_flops
        out["layer_ms"] = round(layer_ms, 4)
        out["layer_frac"] = round(full / div / (layer_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
        out["layer_note"] = ("whole layer (every launch of it), one stream, one batch in flight, median of 5 passes after the timed region; full FLOPs of the layer / the "
                             "same divisor: comparable with the one-launch `frac` of rounds 1-3")
    return out


def tower_layer_ms(plan, med) -> float:
    """One-stream time of the WHOLE marked layer from per-step HIP-event times `med`: the steps under the mark + the tail launch of a split grid."""
    lo, hi = plan.marks["head.tower3x3"]
    ms = sum(med[lo:hi])
    tail = plan.names[lo] + ".tail"
    for i in range(hi, min(hi + 2, len(plan.names))):
        if plan.names[i] == tail:
            ms += med[i]
    return ms


def family_rooflines(plan, x, reps: int = 5) -> dict:
    """Per kernel-family rooflines from the plan's own HIP-event step times (one batch in flight, one stream, median of `reps`
    passes, taken AFTER the timed region): family FLOPs / family time / peak.  `roofline_1x1` is the dominant family BY TIME
    (the GEMM-addressed 1x1 convs: bottleneck conv1 / conv3 / downsample, FPN laterals, head pointwise); executed = algorithmic
    there.  For the Winograd family the executed count is algorithmic / 4 (F(4x4, 3x3) launches) or / 2.25 (F(2x2, 3x3)), per launch."""
    plan.image_ref[0] = x
    for _ in range(2):
        plan.run()
    n = len(plan.steps)
    acc = [[] for _ in range(n)]
    for _ in range(reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        evs[0].record()
        for i, st in enumerate(plan.steps):
            st()
            evs[i + 1].record()
        torch.cuda.synchronize()
        for i in range(n):
            acc[i].append(evs[i].elapsed_time(evs[i + 1]))
    med = [sorted(a)[len(a) // 2] for a in acc]
    fam: dict = {}
    for i in range(n):
        info = plan.step_info.get(i)
        key = info["family"] if info else "other (HBM-bound passes, stem, post-process excluded)"
        f = fam.setdefault(key, {"ms": 0.0, "flops": 0, "executed": 0.0, "launches": 0})
        fl = plan.step_flops.get(i, 0) if info else 0
        f["ms"] += med[i]; f["flops"] += fl; f["executed"] += fl / (info.get("mfma_div", 1.0) if info else 1.0); f["launches"] += 1
    out = {"total_ms_one_batch_in_flight": round(sum(med), 3)}
    for key, f in fam.items():
        tf = f["executed"] / (f["ms"] * 1e-3) / 1e12 if f["ms"] > 0 else 0.0
        out[key] = {"ms": round(f["ms"], 3), "launches": f["launches"], "algorithmic_gflop": round(f["flops"] / 1e9, 1),
                    "executed_tflops": round(tf, 1), "frac_of_f32_mfma_peak": round(tf / PEAK_F32_MFMA_TFLOPS, 4)}
    out["_step_ms"] = med        # (popped by the caller: per-step medians, for the whole-layer figure of the roofline object)
    return out


def parity_vs_oracle(model, x, sd_cpu) -> dict:
    """Measured deviation of the TIMED plan (batch 16, default knobs) from the CPU oracle on image 0 of the timed batch, after the timed region:
    max over the 15 head outputs of |hip - oracle| / (1 + |oracle|).  (oracle/ is used here as the checker only.)"""
    from oracle import torch_ref as R
    out = model(x)
    dev_out = [[t[0:1].float().cpu() for t in grp] for grp in out]
    with torch.no_grad():
        ref = R.hisfcos_forward(sd_cpu, x[0:1].cpu())
    worst, worst_abs, where = 0.0, 0.0, ""
    for name, og, rg in zip(("cls", "cnt", "reg"), dev_out, ref):
        for i, (a, b) in enumerate(zip(og, rg)):
            d = (a - b).abs()
            e = float((d / (1 + b.abs())).max())
            if e > worst:
                worst, where = e, f"{name}{i}"
            worst_abs = max(worst_abs, float(d.max()))
    return {"value": float(f"{worst:.3g}"), "max_abs": float(f"{worst_abs:.3g}"), "where": where, "bar": 1e-4,
            "sample": "image 0 of the timed batch through the timed batch-16 plan vs oracle/torch_ref.hisfcos_forward (fp32 CPU), all 15 head outputs"}


def usable_cores() -> int:
    """CPU threads this process may really use: affinity mask, capped by the cgroup CPU quota (a GPU box exposes
    all host cores in os.cpu_count() but grants a 16-core share)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except Exception:
            pass
    return max(1, min(n, int(os.environ.get("FD_CPU_THREADS", "16"))))


def cpu_baseline(sd, num_classes: int, size: int, budget_s: float = 12.0):
    """The oracle (CPU restatement of the reference's torch path) timed on this host's cores on a bounded sample."""
    from oracle import torch_ref as R
    cores = usable_cores()
    torch.set_num_threads(cores)
    gen = torch.Generator().manual_seed(123)
    strides = [8, 16, 32, 64, 128]

    def one():
        x = torch.randn(1, 3, size, size, generator=gen)
        with torch.no_grad():
            outs = R.hisfcos_forward(sd, x)
        R.fcos_detect(outs, strides, 0.05, 0.6, 1000, (size, size))

    one()  # warm-up (oneDNN primitive creation)
    n, t0 = 0, time.perf_counter()
    while True:
        one()
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s or n >= 256:
            break
    res = {"value": round(n / el, 3), "unit": "images/sec", "cores": cores, "kind": "port",
           "sample": f"{n} single-image 640x640 forward+post-process passes of oracle/torch_ref.py "
                     f"(torch {torch.__version__} CPU, {cores} threads) in {el:.1f} s"}
    res["legs"] = cpu_baseline_legs(sd, num_classes, size, cores)
    return res


def cpu_baseline_legs(sd, num_classes: int, size: int, cores: int) -> dict:
    """SURVEY 8(d)'s other CPU legs, each a bounded sample on the same cores, timed AFTER the GPU measurement: the oracle's forward at the
    bench batch (B = 16), the GIoU loss forward + backward on the oracle's own head outputs, and the reference's greedy-torch NMS
    (DataEncoder._box_nms, utills.py:221-255, the form whose 104 ms at N = 1000 SURVEY quotes) next to its plain-C restatement."""
    import numpy as np
    from oracle import torch_ref as R
    legs = {}
    gen = torch.Generator().manual_seed(321)
    x = torch.randn(16, 3, size, size, generator=gen)
    with torch.no_grad():
        R.hisfcos_forward(sd, x[:2])
        t0 = time.perf_counter()
        outs = R.hisfcos_forward(sd, x)
        el = time.perf_counter() - t0
    legs["forward_b16"] = {"images_per_sec": round(16 / el, 2), "ms": round(el * 1e3, 1), "sample": f"one B=16 {size}x{size} forward of oracle/torch_ref.hisfcos_forward"}
    # GIoU loss forward + backward (loss.py:116-177) on [B, sum HW, 4] predictions with ~2 % positives: the arithmetic fd_ltrb_loss_fwd / _bwd replace
    B, L = 16, sum((size // s) ** 2 for s in (8, 16, 32, 64, 128))
    pred = (torch.rand(B, L, 4, generator=gen) * 64 + 1).requires_grad_(True)
    tgt = torch.rand(B, L, 4, generator=gen) * 64 + 1
    mask = torch.rand(B, L, generator=gen) < 0.02
    def giou_once():
        if pred.grad is not None:
            pred.grad = None
        tot = 0
        for b in range(B):              # the reference loops over the batch (loss.py:129-139)
            pos = mask[b]
            tot = tot + R.giou_loss(pred[b][pos], tgt[b][pos]) / pos.sum().clamp(min=1)
        (tot / B).backward()
    giou_once()
    reps, t0 = 0, time.perf_counter()
    while reps < 50 and time.perf_counter() - t0 < 2.0:
        giou_once(); reps += 1
    el = (time.perf_counter() - t0) / reps
    legs["giou_loss_fwd_bwd_b16"] = {"ms": round(el * 1e3, 3), "locations": B * L, "positives": int(mask.sum()),
                                     "sample": f"{reps} passes of oracle giou_loss + autograd over 16 images x {L} locations, per-image loop as loss.py:129-139"}
    # greedy-torch _box_nms at N = 1000 (class-agnostic, +1 areas, thr 0.5) and the C restatement of the same rule
    rng = np.random.default_rng(5)
    c = rng.uniform(0, size, (1000, 2)); sz = np.exp(rng.uniform(np.log(8), np.log(256), (1000, 2)))
    boxes = np.concatenate([c - sz / 2, c + sz / 2], -1).astype(np.float32)
    scores = rng.uniform(0, 1, 1000).astype(np.float32)
    tb, ts = torch.from_numpy(boxes), torch.from_numpy(scores)
    keep_t = R.box_nms_plus1_torch(tb, ts, 0.5)
    reps, t0 = 0, time.perf_counter()
    while reps < 20 and time.perf_counter() - t0 < 3.0:
        keep_t = R.box_nms_plus1_torch(tb, ts, 0.5); reps += 1
    el_t = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(20):
        keep_c = R.box_nms_plus1(boxes, scores, 0.5)
    el_c = (time.perf_counter() - t0) / 20
    legs["box_nms_greedy_torch_n1000"] = {"ms": round(el_t * 1e3, 2), "kept": int(len(keep_t)), "boxes_per_ms": round(1000 / (el_t * 1e3), 2),
                                          "c_restatement_ms": round(el_c * 1e3, 4), "same_kept_indices": bool(np.array_equal(keep_t.numpy(), keep_c)),
                                          "sample": f"{reps} passes of DataEncoder._box_nms's greedy torch loop (oracle box_nms_plus1_torch), 1000 boxes, thr 0.5"}
    return legs


def gpu_legs_beside_cpu(dev, size: int) -> dict:
    """The HIP side of cpu_baseline_legs' two op-level legs on the same shapes (device time, HIP events)."""
    import numpy as np
    from pytorch_object_detection_amd import ops
    from pytorch_object_detection_amd.model.loss import ltrb_reg_loss
    res = {}
    gen = torch.Generator().manual_seed(321)
    B, L = 16, sum((size // s) ** 2 for s in (8, 16, 32, 64, 128))
    pred = (torch.rand(B, L, 4, generator=gen) * 64 + 1).to(dev).requires_grad_(True)
    tgt = (torch.rand(B, L, 4, generator=gen) * 64 + 1).to(dev)
    mask = (torch.rand(B, L, generator=gen) < 0.02).to(dev)
    def giou_once():
        pred.grad = None
        ltrb_reg_loss(pred, tgt, mask, "giou").mean().backward()
    for _ in range(3):
        giou_once()
    g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g0.record()
    for _ in range(20):
        giou_once()
    g1.record(); g1.synchronize()
    res["giou_loss_fwd_bwd_b16"] = {"ms": round(g0.elapsed_time(g1) / 20, 4), "note": "fd_ltrb_iou_loss_fwd + _bwd through the autograd node, incl. its torch glue launches"}
    rng = np.random.default_rng(5)
    c = rng.uniform(0, size, (1000, 2)); sz = np.exp(rng.uniform(np.log(8), np.log(256), (1000, 2)))
    boxes = torch.from_numpy(np.concatenate([c - sz / 2, c + sz / 2], -1).astype(np.float32)).to(dev)
    scores = torch.from_numpy(rng.uniform(0, 1, 1000).astype(np.float32)).to(dev)
    boxes, scores = boxes[None].contiguous(), scores[None].contiguous()
    for _ in range(3):
        keep, cnt = ops.box_nms_plus1(boxes, scores, 0.5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        keep, cnt = ops.box_nms_plus1(boxes, scores, 0.5)
    e1.record(); e1.synchronize()
    res["box_nms_plus1_n1000"] = {"ms": round(e0.elapsed_time(e1) / 20, 4), "kept": int(cnt[0])}
    return res


def nms_micro(dev, batch: int, with_cpu: bool):
    """NMS micro-benchmark of SURVEY.md §8(d): per image 8 525 candidates (scores sqrt(U*U), 80 classes, box centres
    uniform in 640x640, log-uniform sizes 8-512 px, plus 200 clusters x 5 jittered copies) -> top-1000 -> score >= 0.05
    -> per-class NMS 0.6.  boxes/ms = batch * candidates entering NMS / device time of the NMS call."""
    import numpy as np
    from pytorch_object_detection_amd import ops
    rng = np.random.default_rng(0)
    L, K = 8525, 1000
    c = rng.uniform(0, 640, (batch, L, 2)); sz = np.exp(rng.uniform(np.log(8), np.log(512), (batch, L, 2)))
    cc = rng.uniform(40, 600, (batch, 200, 2)); cs = rng.uniform(24, 200, (batch, 200, 2))
    for b in range(batch):                                    # crowded subset: the first 1000 locations
        idx = np.repeat(np.arange(200), 5)
        c[b, :1000] = cc[b, idx] + rng.normal(0, 4, (1000, 2)); sz[b, :1000] = cs[b, idx] * rng.uniform(0.9, 1.1, (1000, 2))
    boxes = np.concatenate([c - sz / 2, c + sz / 2], -1).astype(np.float32)
    scores = np.sqrt(rng.uniform(0, 1, (batch, L)) * rng.uniform(0, 1, (batch, L))).astype(np.float32)
    scores[:, :1000] = np.maximum(scores[:, :1000], 0.6).astype(np.float32) + rng.uniform(0, 0.3, (batch, 1000)).astype(np.float32)
    classes = rng.integers(1, 81, (batch, L)).astype(np.int32)
    classes[:, :1000] = np.repeat(rng.integers(1, 81, (batch, 200)), 5, axis=1)
    ds, dc, db = (torch.from_numpy(a).to(dev) for a in (scores, classes, boxes))
    reps = 20
    for _ in range(3):
        ts, tc, tb = ops.fcos_topk(ds, dc, db, K)
        out = ops.batched_nms(ts, tc, tb, 0.05, 0.6)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_topk = t_nms = 0.0
    for _ in range(reps):
        e[0].record(); ts, tc, tb = ops.fcos_topk(ds, dc, db, K)
        e[1].record(); out = ops.batched_nms(ts, tc, tb, 0.05, 0.6)
        e[2].record(); e[2].synchronize()
        t_topk += e[0].elapsed_time(e[1]); t_nms += e[1].elapsed_time(e[2])
    t_topk /= reps; t_nms /= reps
    res = {"boxes_per_ms": round(batch * K / t_nms, 1), "nms_ms": round(t_nms, 4), "topk_ms": round(t_topk, 4),
           "kept_mean": round(float(out[4].float().mean()), 1), "candidates_per_image": K, "batch": batch,
           "candidate_set": "SURVEY 8(d)'s SYNTHETIC boxes (uniform centres, log-uniform sizes, 200 x 5 crowded clusters), not the timed model's "
                            "outputs: its kept_mean is a different quantity from the line's top-level kept_mean (the calibrated head's detections)"}
    if with_cpu:
        from oracle import torch_ref as R
        hs, hc, hb = ts.cpu().numpy(), tc.cpu().numpy(), tb.cpu().numpy()
        t0 = time.perf_counter()
        n_img = min(batch, 8)
        keeps = R.post_process(hs[:n_img], hc[:n_img], hb[:n_img], 0.05, 0.6)
        el = time.perf_counter() - t0
        res["cpu_boxes_per_ms"] = round(n_img * K / (el * 1e3), 2)
        res["cpu_sample"] = f"oracle/postproc_ref.c ref_post_process, 1 thread, {n_img} images"
        kd = out[3].cpu().numpy()
        res["matches_oracle"] = bool(all((kd[i, :len(k)] == k).all() and (kd[i, len(k):] == -1).all() for i, k in enumerate(keeps)))
    return res


def postproc_bench(dev, ncls: int = 80, size: int = 640):
    """Roofline evidence for the post-process kernels: decode is HBM-bound -- algorithmic bytes per location
    = (C + 1 + 4) * 4 read + 24 written (2.90 MB + 0.20 MB per 640^2 image) over its HIP-event time; top-k and NMS are
    on-chip / latency-bound (<= 1000 dependent steps): microseconds and boxes/ms, at batch 1 (the latency path) and 16."""
    from pytorch_object_detection_amd import ops
    from pytorch_object_detection_amd._lib import Segs
    strides = [8, 16, 32, 64, 128]
    res = {}
    for B in (1, 16):
        segs = Segs.make(B, [(size // s, size // s) for s in strides])
        g = torch.Generator().manual_seed(3)
        cls = ops.Rows((torch.randn(segs.rows, ncls, generator=g) * 2 - 3).to(dev))
        cnt = ops.Rows(torch.randn(segs.rows, 4, generator=g).to(dev), 0, 1)
        reg = ops.Rows((torch.rand(segs.rows, 4, generator=g) * 64).to(dev))
        L = segs.rows // B

        def timed(fn, reps=50):
            for _ in range(5):
                out = fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3, out            # microseconds

        sc, cl, bx = ops.fcos_decode(cls, cnt, reg, segs, strides)
        import ctypes as C
        from pytorch_object_detection_amd import _lib
        st = (C.c_int32 * 5)(*strides)
        fn, stream = _lib.lib().fd_fcos_decode, torch.cuda.current_stream().cuda_stream
        # the bare C-ABI call on preallocated outputs: the Python wrapper's allocations (~13 us of host time per call) would
        # hide a kernel this short behind the launch rate
        t_dec, _ = timed(lambda: fn(cls.ptr, cls.cs, cls.co, cnt.ptr, cnt.cs, cnt.co, reg.ptr, reg.cs, reg.co, ncls, C.byref(segs), st,
                                    sc.data_ptr(), cl.data_ptr(), bx.data_ptr(), stream), reps=200)
        t_top, (ts, tc, tb) = timed(lambda: ops.fcos_topk(sc, cl, bx, 1000))
        t_nms, out = timed(lambda: ops.batched_nms(ts, tc, tb, 0.05, 0.6))
        nbytes = B * L * ((ncls + 5) * 4 + 24)
        gbs = nbytes / (t_dec * 1e-6) / 1e9
        res[f"batch{B}"] = {"decode_us": round(t_dec, 2), "decode_GBps": round(gbs, 1), "decode_hbm_frac": round(gbs / PEAK_HBM_GBS, 4),
                            "decode_bytes": nbytes, "topk_us": round(t_top, 2), "nms_us": round(t_nms, 2),
                            "nms_boxes_per_ms": round(B * 1000 / (t_nms * 1e-3), 1), "kept_mean": round(float(out[4].float().mean()), 1)}
    res["note"] = ("decode: HBM-bound, peak 8000 GB/s; top-k / NMS: latency-bound on-chip passes (radix select + bitonic sort; "
                   "bitmask + <= 1000-step greedy scan), 24 KB out per image")
    return res


def fast_mode(model, head, clip, x, args, ref_res, precision="f16x3"):
    """Extra, NOT the headline: the same model with conv_precision='f16x3' (three f16 MFMAs per fp32 product, fp32
    accumulation; passes the same 1e-4 parity tests) -- or 'mixed': only the 1x1 layers on the split-f16 products, the 3x3
    stride-1 layers on the exact-fp32 Winograd kernel.  Reports its throughput, its head-tower rate and its deviation
    from the exact-fp32 path on this batch (one batch in flight)."""
    from pytorch_object_detection_amd import ops
    ref_out = [[t.clone() for t in grp] for grp in model(x)]
    model.conv_precision = precision
    try:
        plan = model.plan_for(x)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

        def step(i=None):
            out = model(x, events=None if i is None else {"head.tower3x3": ev[i]})
            s, c, b = head.decode_topk(out)
            os_, oc, ob, _, counts = ops.batched_nms(s, c, b, 0.05, 0.6)
            return out, os_, oc, clip(x, ob), counts

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out, os_, oc, ob, counts = step(i)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        dev_abs = max(float((a - b).abs().max()) for g1, g2 in zip(out, ref_out) for a, b in zip(g1, g2))
        dev_rel = max(float(((a - b).abs() / (b.abs() + 1.0)).max()) for g1, g2 in zip(out, ref_out) for a, b in zip(g1, g2))
        tower_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
        flops = tower_mark_flops(plan)[0]            # (algorithmic FLOPs of the launch the events bracket)
        r = {"conv_precision": ("f16x3 (x = hi + lo*2^-11, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulate)" if precision == "f16x3" else
                                "mixed: 1x1 layers f16x3, 3x3 stride-1 layers exact-fp32 Winograd F(2x2,3x3)"),
             "value": round(args.batch * args.steps / el, 2), "unit": "images/sec", "ms_per_step": round(el / args.steps * 1e3, 3), "batches_in_flight": 1,
             "head_tower_tflops_fp32_equivalent": round(flops / (tower_ms * 1e-3) / 1e12, 1),
             "max_abs_dev_vs_f32_path": dev_abs, "max_dev_over_1_plus_abs_vs_f32_path": dev_rel,
             "same_kept_counts_as_f32_path": bool(torch.equal(counts, ref_res[3][:args.batch]))}
        if precision == "f16x3":
            r["head_tower_f16_mfma_frac_of_2500TF"] = round(3 * flops / (tower_ms * 1e-3) / 1e12 / 2500.0, 3)
        if args.inflight == 2:      # the same schedule as the headline: two batches in flight, the tower exclusive
            from pytorch_object_detection_amd.pipeline import TwoLanePipeline

            def post(o, xx, tag):
                s, c, b = head.decode_topk(o)
                return ops.batched_nms(s, c, b, 0.05, 0.6)[4]
            pipe = TwoLanePipeline(model, post)
            pipe.calibrate(x)
            for _ in range(args.warmup):
                pipe.submit(x)
            pipe.drain()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                pipe.submit(x)
            pipe.drain()
            torch.cuda.synchronize()
            el2 = time.perf_counter() - t0
            r["value_two_batches_in_flight"] = round(args.batch * args.steps / el2, 2)
            r["ms_per_step_two_batches_in_flight"] = round(el2 / args.steps * 1e3, 3)
        return r
    finally:
        model.conv_precision = None


def train_step(dev, batch: int = 16, size: int = 512, steps: int = 5):
    """Diagnostic (SURVEY Cfg4): one HISFCOS-R50 training step (forward, FCOSGenTargets, FCOSLoss('giou'), backward, SGD)
    at the reference's VOC shape, with the HIP training kernels and with every layer routed to stock PyTorch-ROCm ops."""
    from pytorch_object_detection_amd import train_ops
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(dev).train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(batch, 3, size, size, device=dev)
    c = torch.rand(batch, 8, 2, device=dev) * (size - 112) + 50
    s = torch.rand(batch, 8, 2, device=dev) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, size - 1)
    labels = torch.randint(1, 21, (batch, 8), device=dev)
    gen = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")

    def one():
        opt.zero_grad(set_to_none=True)
        out = model(x)
        losses = crit([out, gen([out, gt, labels])])
        losses[-1].backward()
        opt.step()
        return float(losses[-1].detach())

    res = {"batch": batch, "size": size, "classes": 20, "gt_boxes_per_image": 8, "loss": "giou", "optimizer": "SGD",
           "batchnorm": "backbone frozen (eval), FPN BatchNorms on batch statistics as under the reference's model.train() (train.py:151)"}
    for name, stock, freeze_all in (("hip_ms", False, False), ("stock_ops_ms", True, False), ("hip_all_bn_frozen_ms", False, True)):
        train_ops._STOCK = stock
        model.freeze_all_bn = freeze_all
        model.train()
        try:
            for _ in range(2):
                one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one()
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) / steps * 1e3, 2)
        finally:
            train_ops._STOCK = False
            model.freeze_all_bn = False
    res["images_per_sec"] = round(batch / (res["hip_ms"] * 1e-3), 1)
    return res


def train_mode(args, rank, world, dev, use_dist, out=sys.stdout):
    """`--mode train` (SURVEY Cfg4): the reference's train.py step on N GPUs -- DistributedDataParallel around the model
    (gradient all-reduce over RCCL, bucketed and overlapped with backward by DDP), HIP forward / backward / target /
    loss kernels, SGD.  Weak scaling: --batch images of --size per GPU (defaults 16 x 512 x 512, 20 classes: voc.yaml)."""
    from pytorch_object_detection_amd.model.loss import FCOSLoss
    from pytorch_object_detection_amd.model.modules.head import FCOSGenTargets
    from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
    size, batch, ncls = args.size, args.batch, args.classes
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], ncls, 256).to(dev)
    ddp_kw = {"find": dict(find_unused_parameters=True),                                   # train.py:101 as written
              "static": dict(static_graph=True, gradient_as_bucket_view=True)}[os.environ.get("FD_BENCH_DDP", "static")]
    net = torch.nn.parallel.DistributedDataParallel(model, **ddp_kw) if use_dist else model
    if use_dist:
        # train.py:101-103: DDP wrap, then SyncBatchNorm.convert_sync_batchnorm -- the FPN's batch-statistic BatchNorms take their
        # statistics over all ranks, on the HIP kernels with one fp64 all-reduce per layer and direction (train_ops._SyncBatchNormTrainRows)
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
    net.train()
    # --amp: the fused SGD (torch.optim.SGD(fused=True): same update, one multi-tensor launch).  It takes GradScaler's found_inf tensor and skips the update ON THE DEVICE,
    # so scaler.step does not call .item(): with the plain optimizer every step ends in a host synchronisation, and the AMP step -- 21 ms of kernels behind ~20 ms of
    # Python / autograd enqueue work -- drains its pipeline once per step (tools/train_host_time.py: 25.1 ms synchronized = 25.1 ms on the host).  FD_BENCH_FUSED_OPT=0: plain.
    fused_opt = bool(getattr(args, "amp", False)) and os.environ.get("FD_BENCH_FUSED_OPT", "1") != "0"
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=1e-4, **({"fused": True} if fused_opt else {}))
    gen = torch.Generator().manual_seed(1000 + rank)
    x = torch.randn(batch, 3, size, size, generator=gen).to(dev)
    c = torch.rand(batch, 8, 2, generator=gen) * (size - 112) + 50
    s = torch.rand(batch, 8, 2, generator=gen) * 150 + 20
    gt = torch.cat([c - s / 2, c + s / 2], -1).clamp(0, size - 1).to(dev)
    labels = torch.randint(1, ncls + 1, (batch, 8), generator=gen).to(dev)
    gen_t = FCOSGenTargets([8, 16, 32, 64, 128], [[-1, 32], [32, 96], [96, 192], [192, 384], [384, 9999999]])
    crit = FCOSLoss("giou")

    amp = bool(getattr(args, "amp", False))
    scaler = torch.amp.GradScaler("cuda", enabled=amp)          # train.py:175-181: autocast forward + loss, scaled backward, scaler.step

    def one():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = net(x)
            losses = crit([out, gen_t([out, gt, labels])])
        scaler.scale(losses[-1]).backward()
        scaler.step(opt)
        scaler.update()
        return losses[-1]

    # One process, one GPU: the whole step (forward, loss, backward, optimizer, GradScaler) is captured once as a HIP graph and replayed (train_graph.GraphedStep):
    # under AMP the eager step is bound by the host (16 ms of kernels behind 15 - 20 ms of Python / autograd / ctypes enqueue work).  Each replay copies the batch
    # into the captured tensors and runs every launch of the step.  FD_BENCH_TRAIN_GRAPH=0 (and every multi-rank run): eager, as the reference's loop.
    step_mode = "eager"
    if not use_dist and os.environ.get("FD_BENCH_TRAIN_GRAPH", "1") != "0" and (not amp or fused_opt):
        from pytorch_object_detection_amd.train_graph import GraphedStep

        def one_g(x_, gt_, labels_):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp, cache_enabled=False):
                out = net(x_)
                losses = crit([out, gen_t([out, gt_, labels_])])
            scaler.scale(losses[-1]).backward()
            scaler.step(opt)
            scaler.update()
            return losses[-1].detach()
        try:
            graphed = GraphedStep(one_g, [x, gt, labels], warmup=max(3, args.warmup))
            xb, gtb, lb = x.clone(), gt.clone(), labels.clone()          # (the "loader's" batch: copied into the captured tensors by every step)
            one = lambda: graphed(xb, gtb, lb)  # noqa: E731
            step_mode = "hip graph (whole step captured once, replayed)"
        except Exception as e:  # noqa: BLE001
            print(f"bench: training step not captured as a graph ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
    for _ in range(args.warmup):
        one()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = one()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    el = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    if rank != 0:
        return
    if args.dump_outputs:       # the last step's loss and the weights it updated (a fixed, seeded sample of 4 Mi of them)
        import numpy as np
        flat = torch.cat([p.detach().reshape(-1).float() for p in model.parameters() if p.requires_grad])
        idx = np.sort(np.random.default_rng(0).choice(flat.numel(), min(flat.numel(), 1 << 22), replace=False))
        dump_outputs(args.dump_outputs, {"loss": loss.detach().double().reshape(1), "params": flat[torch.from_numpy(idx).to(dev)]})
    line = {
        "metric": f"images/sec HISFCOS-R50 {size}x{size} train step (GIoU loss, SGD)", "value": round(batch * world * args.steps / el, 2),
        "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(el / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f16 operands / f32 accumulate in every dense conv: forward, data gradient, weight gradient (torch.autocast + GradScaler, the reference's AMP arithmetic); norms, depthwise, losses f32" if amp else "f32",
        "data": "synthetic", "amp": amp,
        "config": {"workload": f"HISFCOS-R50 train.py step, {batch} x {size}x{size} images/GPU, {ncls} classes, 8 GT boxes/image, "
                               "HIP forward/backward/target/loss kernels" + (", DDP gradient all-reduce + SyncBatchNorm statistics all-reduces over RCCL" if use_dist else ""),
                   "batchnorm": "backbone frozen (eval); FPN BatchNorms on batch statistics" + (" over all ranks (SyncBatchNorm on the HIP statistics kernels)" if use_dist else ""),
                   "step_enqueue": step_mode,
                   "optimizer": "SGD momentum 0.9" + (", fused=True (GradScaler's found_inf handled on the device: no host synchronisation per step)" if fused_opt else ""),
                   "amp_activation_maps": ("f16 in HBM inside the ResNet bottlenecks (train_ops.AMP_F16_STORE), fp32 elsewhere" if amp else None),
                   "global_batch": batch * world, "parallelism": f"dp{world} (DistributedDataParallel)"},
        "final_loss": round(float(loss.detach()), 5)}
    if args.full:
        line.update(train_rooflines(args, dev, size, batch, amp))
    print(json.dumps(line), file=out, flush=True)


def train_rooflines(args, dev, size: int, batch: int, amp: bool) -> dict:
    """--full, `--mode train`: kernel rooflines timed on their own after the timed steps -- the head tower's weight gradient (`roofline`)
    and, under --amp, its f16 forward (`roofline_amp_f16`)."""
    from pytorch_object_detection_amd import ops
    from pytorch_object_detection_amd._lib import Segs
    # roofline of the dominant backward kernel: the weight gradient of the head tower 3x3 (256 -> 256, all five levels)
    lv = [(size // st, size // st) for st in (8, 16, 32, 64, 128)]
    segs = Segs.make(batch, lv)
    xr, dy = ops.Rows(torch.randn(segs.rows, 256, device=dev)), ops.Rows(torch.randn(segs.rows, 256, device=dev))
    wprec = 2 if bool(getattr(args, "amp", False)) else 0        # (--amp: the f16-operand weight gradient the AMP step runs)
    f = lambda: ops.conv_wgrad(xr, dy, segs, Cin=256, Cout=256, k=3, pad=1, oihw=True, precision=wprec)  # noqa: E731
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        f()
    e1.record()
    e1.synchronize()
    wms = e0.elapsed_time(e1) / 10
    wflops = 2 * segs.rows * 256 * 256 * 9
    ach = wflops / (wms * 1e-3) / 1e12
    amp_roof = None
    if amp:   # the f16 side of the AMP step: the head tower 3x3 forward (256 -> 512, five levels) on v_mfma_f32_32x32x16_f16, against the dense f16 peak
        from pytorch_object_detection_amd import _lib as L
        wt = torch.randn(512, 256, 3, 3, device=dev) / 48.0
        k64 = ops.F16K64 and ops.f16k64_ok(256, 512)        # the kernel the AMP step runs this layer on (FD_AMP_K64=0: round 3's K-tile-32 instantiation)
        wp16 = ops.pack_conv_weight_f16k64(wt) if k64 else ops.pack_conv_weight_hip(wt, f16=True)
        yt = ops.Rows(torch.empty(segs.rows, 512, device=dev))
        from pytorch_object_detection_amd import train_ops as TO
        z16 = bool(k64 and TO.AMP_F16_STORE)                  # the step stores the towers' input z as f16 (HISFCOSHead.train_forward_rows: conv_rows(pw2, ..., out_f16=True))
        xin = ops.Rows(xr.tensor().half().contiguous()) if z16 else xr
        ft = ops.conv_call(xin, segs, wp16, yt, Cin=256, Cout=512, k=3, pad=1, precision=L.PREC_F16, tile=L.F16K64_TILE if k64 else 0)
        for _ in range(3):
            ft()
        e0.record()
        for _ in range(10):
            ft()
        e1.record()
        e1.synchronize()
        tms = e0.elapsed_time(e1) / 10
        tfl = 2 * segs.rows * 512 * 256 * 9
        amp_roof = {"bound": "mfma", "kernel": ("conv_f16k64_kernel (FD_TILE_F16K64: K-tiles of 64 channels)" if k64 else "conv_igemm_kernel<..., H1>") +
                              " head tower 3x3 forward (cls_conv + reg_conv as one 256 -> 512 launch, 5 levels), f16 operands / fp32 accumulate, " +
                              ("f16 activation map in (the step stores the towers' input as f16), fp32 out" if z16 else "fp32 activation map in"),
                    "instruction": "v_mfma_f32_32x32x16_f16", "achieved": round(tfl / (tms * 1e-3) / 1e12, 1), "peak": 2500.0, "unit": "TFLOP/s",
                    "frac": round(tfl / (tms * 1e-3) / 1e12 / 2500.0, 4), "traffic": None, "flops_per_launch": tfl, "avg_launch_ms": round(tms, 4)}
    return {"roofline_amp_f16": amp_roof,
            "roofline": {"bound": "mfma", "kernel": ("conv_wgrad_f16_kernel" if wprec else "conv_wgrad_kernel") + " (head tower 3x3 weight gradient, 5 levels) + ordered slab reduce",
                         "instruction": "v_mfma_f32_32x32x16_f16" if wprec else "v_mfma_f32_32x32x2_f32", "achieved": round(ach, 2),
                         "peak": 2500.0 if wprec else PEAK_F32_MFMA_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(ach / (2500.0 if wprec else PEAK_F32_MFMA_TFLOPS), 4), "traffic": None,
                         "flops_per_launch": wflops, "avg_launch_ms": round(wms, 4)}}


def layer_times(plan, x, path, reps=5):
    """Diagnostic: HIP-event time of every plan step (median of `reps`), with conv TFLOP/s where applicable."""
    plan.image_ref[0] = x
    for _ in range(2):
        plan.run()
    n = len(plan.steps)
    acc = [[] for _ in range(n)]
    for _ in range(reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        evs[0].record()
        for i, st in enumerate(plan.steps):
            st()
            evs[i + 1].record()
        torch.cuda.synchronize()
        for i in range(n):
            acc[i].append(evs[i].elapsed_time(evs[i + 1]))
    tot = 0.0
    with open(path, "w") as f:
        f.write("step\tname\tms\tgflop\ttflops\n")
        for i, name in enumerate(plan.names):
            ms = sorted(acc[i])[len(acc[i]) // 2]
            tot += ms
            fl = plan.step_flops.get(i, 0)
            f.write(f"{i}\t{name}\t{ms:.4f}\t{fl / 1e9:.2f}\t{(fl / (ms * 1e-3) / 1e12) if fl else 0:.1f}\t{plan.tiles.get(name, '')}\n")
        f.write(f"#total_ms\t{tot:.3f}\n")


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path: str, arrays: dict, budget: int = DUMP_BUDGET_BYTES) -> None:
    """--dump-outputs: write every array as <path>/<name>.npy, float64 where it is float64 and float32 otherwise (class ids and
    counts are small integers, exact in float32).  The arrays together stay within `budget` bytes: smallest first, an array larger
    than an equal share of what is left of the budget is replaced by its elements at a fixed, seeded set of flat indices (the same
    set in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    out = {}
    for name, v in arrays.items():
        a = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        out[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    left = budget
    order = sorted(out, key=lambda n: out[n].nbytes)
    for k, name in enumerate(order):
        a = out[name]
        share = left // (len(order) - k)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        left -= a.nbytes
        np.save(os.path.join(path, name + ".npy"), a)


def _claim_stdout():
    """Rank 0 must print ONE JSON line on stdout; RCCL writes its version banner to file descriptor 1 when the first
    communicator comes up.  Keep a private handle on the real stdout for the JSON line and point fd 1 at stderr meanwhile."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    return real


def launch_ranks(n: int, out) -> int:
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start N rank processes of this same command -- fresh
    children with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, exactly what `python -m torch.distributed.run --nproc-per-node N`
    would start -- relay rank 0's single JSON line and fail if any rank fails.  This parent never touches the GPU (no HIP call
    before or after the children exist: a process that has initialised HIP must not fork / exec rank processes)."""
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # a rank that dies leaves the others waiting in a collective: watch all of them, stop the rest (exact PIDs) on the first failure
    failed = None
    while failed is None and any(p.poll() is None for p in procs[1:]) and procs[0].poll() is None:
        for r, p in enumerate(procs):
            if p.poll() not in (None, 0):
                failed = r
        time.sleep(0.2)
    if failed is None:
        # rank 0 (or every other rank) is done: the rest get a bounded time to leave their last collective / tear down, then count as failed
        deadline = time.time() + float(os.environ.get("FD_BENCH_RANK_EXIT_TIMEOUT", "120"))
        while time.time() < deadline and any(p.poll() is None for p in procs):
            time.sleep(0.2)
        stuck = next((r for r, p in enumerate(procs) if p.poll() is None), None)
        if stuck is not None:
            failed = stuck
        else:
            text = procs[0].stdout.read()
            failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    if failed is not None:
        for p in procs:
            if p.poll() is None:
                p.kill()
        print(f"bench.py: rank {failed} of {n} exited with code {procs[failed].poll()}", file=sys.stderr)
        return 1
    lines = [ln for ln in text.splitlines() if ln.strip()]
    if len(lines) != 1:
        print(f"bench.py: rank 0 printed {len(lines)} lines, expected ONE JSON line", file=sys.stderr)
        return 1
    if json.loads(lines[0]).get("n_gpus") != n:
        print(f"bench.py: the line reports n_gpus={json.loads(lines[0]).get('n_gpus')}, launched {n} ranks", file=sys.stderr)
        return 1
    out.write(lines[0] + "\n")
    out.flush()
    return 0


def main():
    out = _claim_stdout()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU")
    ap.add_argument("--size", default="640", help="input size: S (square) or HxW, multiples of 32 (Cfg5: 832x1344)")
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--model", default="HISFCOS", choices=["HISFCOS", "FCOS", "FCOS-B3", "MNFCOS"],
                    help="FCOS / FCOS-B3 = diagnostic runs of the baseline detector on ResNet-50 / EfficientNet-B3 (Cfg5)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train"], help="train = diagnostic: the Cfg4 training step (DDP over RCCL for N > 1)")
    ap.add_argument("--inflight", type=int, default=2, choices=[1, 2],
                    help="batches in flight per GPU: 2 = consecutive steps alternate between two plan instances on two HIP streams "
                         "(throughput), 1 = one stream, every step behind the previous one")
    ap.add_argument("--graph", action="store_true", help="inference: capture the plan's launches into a HIP graph and replay it (the latency path; implies --inflight 1)")
    ap.add_argument("--amp", action="store_true", help="--mode train: the step under torch.autocast(float16) + GradScaler (train.py:33,175-181): f16 MFMA operands, fp32 accumulation")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fast-mode", action="store_true", help="skip the extra opt-in f16x3 measurement")
    ap.add_argument("--save-tuning", action="store_true", help="write the conv tile table measured in this run back to tuned/gfx950_tiles.json")
    ap.add_argument("--no-train-step", action="store_true", help="skip the Cfg4 training-step diagnostic")
    ap.add_argument("--layer-times", default="", help="diagnostic: write per-plan-step timings (TSV) to this file and exit")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other measurement of the line (kernel-family rooflines, parity vs the CPU oracle, "
                         "f16x3 / mixed modes, NMS / post-process micro-benchmarks, training-step diagnostic, CPU baseline; --mode train: its rooflines)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step returned to DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    args = ap.parse_args()
    hw = [int(v) for v in str(args.size).lower().split("x")]
    args.height, args.width = (hw[0], hw[0]) if len(hw) == 1 else (hw[0], hw[1])
    args.size = args.height if args.height == args.width else f"{args.height}x{args.width}"

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus, out))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal of the N > 1 control flow on a ONE-GPU box (RCCL refuses two ranks on one device): FD_BENCH_BACKEND=gloo puts
    # every rank on cuda:0 and carries the collectives through gloo.  Never a measurement; the driver's runs use RCCL.
    backend = os.environ.get("FD_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = 0
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL (must precede HIP initialisation)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: the JSON line's n_gpus must be the number of ranks that ran")
    if os.environ.get("FD_BENCH_DRYRUN") == "1":
        # launcher / rendezvous rehearsal WITHOUT a GPU (tests/test_dist_cpu.py): every rank joins a gloo group, checks a collective,
        # rank 0 prints a line that carries no measurement.  Nothing of the product path runs.
        if world > 1:
            os.environ.setdefault("MASTER_PORT", "29511")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            t = torch.tensor([float(rank + 1)])
            dist.all_reduce(t)
            assert int(t.item()) == world * (world + 1) // 2
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            out.write(json.dumps({"metric": "dryrun (no measurement)", "value": None, "n_gpus": world, "mode": args.mode, "dryrun": True}) + "\n")
            out.flush()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or os.environ.get("FD_BENCH_FORCE_DIST") == "1"   # the env knob exercises the RCCL path with 1 rank
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    if args.mode == "train":
        if args.size == 640 and args.classes == 80:      # untouched defaults -> the reference's VOC training shape
            args.size, args.classes = 512, 20
        train_mode(args, rank, world, dev, use_dist, out)
        if use_dist:
            dist.destroy_process_group()
        return

    from pytorch_object_detection_amd import _lib
    from pytorch_object_detection_amd.dist import gather_detections
    from pytorch_object_detection_amd.model.modules.head import ClipBoxes, FCOSHead
    _lib.lib()

    model = build_model(args.classes, seed=0, name=args.model)
    if args.model != "HISFCOS":
        args.no_cpu_baseline = True   # the CPU-baseline leg restates HISFCOS only
    sd_cpu = {k: v.clone() for k, v in model.state_dict().items()} if (rank == 0 and world == 1 and args.full and not args.no_cpu_baseline) else None
    model.to(dev)
    if args.graph:
        model.use_graph, args.inflight = True, 1
    head = FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64, 128])
    clip = ClipBoxes()
    gen = torch.Generator().manual_seed(1000 + rank)
    x = torch.randn(args.batch, 3, args.height, args.width, generator=gen).to(dev)

    plan = model.plan_for(x)
    if args.layer_times:
        layer_times(plan, x, args.layer_times)
        return
    ev_pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    nms_pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

    from pytorch_object_detection_amd import ops

    def post(out, xx, i=None):
        """FCOSHead (decode, top-1000, score >= 0.05, per-class NMS 0.6) -> ClipBoxes -> (N > 1) the detection all-gather."""
        s, c, b = head.decode_topk(out)
        if i is not None:
            nms_pairs[i][0].record()
        os_, oc, ob, _, counts = ops.batched_nms(s, c, b, 0.05, 0.6)
        if i is not None:
            nms_pairs[i][1].record()
        ob = clip(xx, ob)
        return gather_detections(os_, oc, ob, counts, force=use_dist)

    def step(i=None):
        if args.graph:      # the latency path: model + FCOSHead + ClipBoxes as ONE plan, captured into one HIP graph (model.detect)
            os_, oc, ob, counts = model.detect(x, head)
            return gather_detections(os_, oc, ob, counts, force=use_dist)
        out = model(x, events=None if i is None else {"head.tower3x3": ev_pairs[i]})
        return post(out, x, i)

    pipe = None
    if args.inflight == 2:
        # two batches in flight on two HIP streams (pipeline.TwoLanePipeline): step i+1's trunk fills the launch tails of
        # step i; the head-tower launch of every step runs exclusively (its events below stay a clean kernel duration)
        from pytorch_object_detection_amd.pipeline import TwoLanePipeline
        pipe = TwoLanePipeline(model, post)
        pipe.calibrate(x)          # (untimed: picks the P1 | P2 cut of the interleaving from a few pipelined steps)

    def run_steps(n, timed):
        r = None
        if pipe is None:
            for i in range(n):
                r = step(i if timed else None)
            return r
        for i in range(n):
            pipe.submit(x, tower_events=ev_pairs[i] if timed else None, tag=i if timed else None)
        return pipe.drain()

    run_steps(args.warmup, False)
    if args.save_tuning and rank == 0:      # (after the warm-up: the two-lane plans and their "pair|" entries exist by now)
        ops.save_tune_table()
    if use_dist:
        dist.barrier(**({"device_ids": [local_rank]} if backend == "nccl" else {}))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run_steps(args.steps, True)
    if use_dist:
        dist.barrier(**({"device_ids": [local_rank]} if backend == "nccl" else {}))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())

    if rank == 0:
        if args.dump_outputs:   # (before anything else runs on the device: what the last timed step returned)
            dump_outputs(args.dump_outputs, dict(zip(("scores", "classes", "boxes", "counts"), res)))
        # the head-tower and NMS events were recorded inside the timed steps; a replayed graph has none: with --full its tower / NMS
        # times come from the same plans launched eagerly afterwards, a plain --graph run reports neither
        step_events = not args.graph
        if args.graph and args.full:
            for i in range(args.steps):
                post(model(x, events={"head.tower3x3": ev_pairs[i]}), x, i)
            torch.cuda.synchronize()
            step_events = True
        images = args.batch * world * args.steps
        ms_step = el / args.steps * 1e3
        fams = step_ms = None
        if args.full:
            fams = family_rooflines(plan, x)
            step_ms = fams.pop("_step_ms")
        workload = {"model": args.model, "batch": args.batch, "height": args.height, "width": args.width}
        line = {
            "metric": f"images/sec {args.model if '-' in args.model else args.model + '-R50'} {args.height}x{args.width} inference",
            "value": round(images / el, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic (randn images, seeded random-init weights, calibrated prediction layers)",
            "config": {"workload": f"{args.model if '-' in args.model else args.model + '-R50'} {args.height}x{args.width} batch={args.batch}/GPU inference on MI355X, "
                                   f"fused conv head + HIP NMS ({args.classes} classes, score>=0.05, IoU 0.6, top-1000)"
                                   + (", RCCL detection all-gather" if world > 1 else ""),
                       "global_batch": args.batch * world, "parallelism": f"dp{world} (image-sharded)",
                       "batches_in_flight": args.inflight, "hip_graph": bool(args.graph)},
            "model_conv_tflops": round(plan.flops / (ms_step * 1e-3) / 1e12, 2),
            "detections_kept_rank0": [int(v) for v in res[3][:args.batch].tolist()][:4],
            "kept_mean": round(float(res[3][:args.batch].float().mean()), 1),
            "parity_note": ("per-stage results on identical inputs are bit-exact vs the oracle (decode boxes, top-k order, NMS kept indices, "
                            "clip); END-TO-END detections are set-identical, not sequence-identical: device expf vs host libm differ by "
                            "1 ulp on ~2 % of scores, which can swap neighbours in the score order (tests/test_model_gpu.py).  Conv outputs: what the tests and "
                            "`max_err_over_1_plus_abs_vs_oracle` ASSERT is the RELATIVE bar |hip - oracle| <= 3e-5 * (1 + |oracle|) (tests/test_model_gpu.py:34-57), "
                            "not north_star's absolute 1e-4: the calibrated head's logits reach |x| ~ 100, where one fp32 ulp is 8e-6 and the reference's own CPU "
                            "runs differ by 4e-6 relative between thread counts (SURVEY section 7); `max_abs` is reported beside it, not asserted"),
        }
        line["head_calibrated"] = True      # bench.calibrate_head rescales the prediction layers (since round 3): lines of rounds 1-2 ran an NMS that kept all 1000 candidates
        if step_events:
            tower_ms = sum(a.elapsed_time(b) for a, b in ev_pairs) / args.steps
            nms_ms = sum(a.elapsed_time(b) for a, b in nms_pairs) / args.steps
            line["roofline"] = tower_roofline(plan, tower_ms, workload, layer_ms=tower_layer_ms(plan, step_ms) if step_ms is not None else None)
            line["nms_boxes_per_ms"], line["nms_ms"] = round(args.batch * 1000 / nms_ms, 1), round(nms_ms, 4)
        if args.full:
            if sd_cpu is not None:
                line["max_err_over_1_plus_abs_vs_oracle"] = parity_vs_oracle(model, x, sd_cpu)
            f1 = fams.get("1x1")
            if f1:
                line["roofline_1x1"] = {"bound": "mfma", "kernel": "conv_igemm_kernel / conv1x1 family: every GEMM-addressed 1x1 conv of the plan "
                                        f"({f1['launches']} launches)", "instruction": "v_mfma_f32_32x32x2_f32",
                                        "achieved": f1["executed_tflops"], "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                                        "frac": f1["frac_of_f32_mfma_peak"], "family_ms": f1["ms"], "family_gflop": f1["algorithmic_gflop"],
                                        "timing": "sum of per-launch HIP-event times, one batch in flight, median of 5 passes after the timed region"}
            line["kernel_families"] = fams
            if world == 1 and not args.no_fast_mode:
                line["fast_mode"] = fast_mode(model, head, clip, x, args, res)
                line["fast_mode_mixed"] = fast_mode(model, head, clip, x, args, res, "mixed")
            if world == 1:
                line["nms_micro"] = nms_micro(dev, args.batch, with_cpu=sd_cpu is not None)
                line["postproc"] = postproc_bench(dev, args.classes)
                line["note_end_to_end_nms"] = ("the bench head is calibrated (bench.calibrate_head, seeded): the timed end-to-end step's NMS suppresses "
                                               "most of its 1000 candidates per image (kept_mean); nms_micro / postproc are SURVEY 8d's synthetic workloads")
            if world == 1 and not args.no_train_step:
                line["train_step"] = train_step(dev)
            if sd_cpu is not None:
                line["cpu_baseline"] = cpu_baseline(sd_cpu, args.classes, args.height)
                line["cpu_baseline"]["hip_beside_legs"] = gpu_legs_beside_cpu(dev, args.height)
        out.write(json.dumps(line) + "\n")
        out.flush()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
