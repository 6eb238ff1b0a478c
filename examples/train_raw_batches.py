#!/usr/bin/env python3
"""The loop of examples/train_like_train_py.py fed from RAW images: decoded uint8 images and their boxes go through
data.augment.collate_train_raw -- the reference's flip + Transforms + preprocess_img_boxes + collate_fn, the pixel work in one
fused HIP launch -- and the triple it returns is what model / FCOSGenTargets / FCOSLoss take in train() mode.

    python examples/train_raw_batches.py [--steps 10] [--batch 8] [--amp] [--min-side 512 --max-side 512] [--assigner atss|simota]

The images here are synthetic (JPEG decoding stays on the host and is not part of this project); single GPU.
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd.data.augment import collate_train_raw  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import ATSSGenTargets, FCOSGenTargets, SimOTAGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402


def synthetic_sample(rng, dev):
    """One "decoded" VOC-shaped sample: uint8 [h, w, 3] on the device, fp32 boxes (x1, y1, x2, y2) and classes on the host."""
    h, w = [(375, 500), (500, 375), (333, 500), (480, 640)][int(rng.integers(0, 4))]
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev)
    n = int(rng.integers(1, 6))
    xy = rng.uniform(0, 0.6, (n, 2)) * [w, h]
    wh = rng.uniform(0.1, 0.35, (n, 2)) * [w, h]
    return img, np.concatenate([xy, xy + wh], 1).astype(np.float32), rng.integers(1, 21, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--min-side", type=int, default=512)
    ap.add_argument("--max-side", type=int, default=512)
    ap.add_argument("--assigner", choices=["fcos", "atss", "simota"], default="fcos",
                    help="target assignment: FCOSGenTargets, ATSSGenTargets or SimOTAGenTargets")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(dev)
    gen_target = FCOSGenTargets(strides=[8, 16, 32, 64, 128], limit_range=[[-1, 64], [64, 128], [128, 256], [256, 512], [512, 999999]])
    if args.assigner == "atss":
        gen_target = ATSSGenTargets(strides=[8, 16, 32, 64, 128])
    elif args.assigner == "simota":
        gen_target = SimOTAGenTargets(strides=[8, 16, 32, 64, 128])
    LR_INIT, WARMUP_STEPS = 1e-3, 501
    optimizer = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=LR_INIT, momentum=0.9, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=args.amp)
    criterion = FCOSLoss("giou")
    data_rng, aug_rng = np.random.default_rng(100), random.Random(100)
    model.train()
    t0 = None
    for step in range(1, args.steps + 1):
        samples = [synthetic_sample(data_rng, dev) for _ in range(args.batch)]
        imgs, targets, classes = collate_train_raw([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples],
                                                   (args.min_side, args.max_side), rng=aug_rng)
        if step < WARMUP_STEPS:
            for group in optimizer.param_groups:
                group["lr"] = float(step / WARMUP_STEPS * LR_INIT)
        optimizer.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16, enabled=args.amp):
            outputs = model(imgs)
            target = gen_target([outputs, targets, classes])
            losses = criterion([outputs, target])
            loss = losses[-1]
        scaler.scale(loss.mean()).backward()
        scaler.step(optimizer)
        scaler.update()
        if step == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if step % 5 == 0 or step == 1:
            print(f"step {step:4d}  canvas {tuple(imgs.shape[2:])}  cls {float(losses[0]):.4f}  cnt {float(losses[1]):.4f}  reg {float(losses[2]):.4f}  "
                  f"total {float(losses[3]):.4f}")
    torch.cuda.synchronize()
    if t0 is not None and args.steps > 3:
        dt = (time.perf_counter() - t0) / (args.steps - 3)
        print(f"{dt * 1e3:.1f} ms/step, {args.batch / dt:.1f} img/s (synthetic images generated inside the loop)")


if __name__ == "__main__":
    main()
