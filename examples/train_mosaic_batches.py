#!/usr/bin/env python3
"""The loop of examples/train_raw_batches.py fed with MOSAIC batches from JPEG bytes: decode, mosaic, targets, loss, step.

    python examples/train_mosaic_batches.py [FILE.jpg ...] [--steps 10] [--batch 8] [--side 512] [--amp] [--assigner atss]

Per step: data.JpegDecoder decodes the batch's JPEG streams into uint8 [h, w, 3] images on the device;
data.augment.collate_train_mosaic draws, per output, three partners, a centre, the reference's per-image transforms and a gain for
each of the four tiles, moves and clips the boxes on the host, and makes every pixel of the batch in one HIP launch;
the triple it returns is what model / FCOSGenTargets / FCOSLoss take in train() mode.  Nothing returns to the host inside a step but the progress line.

Without FILE arguments the example encodes synthetic images with Pillow first; their boxes are synthetic either way (a real
loader supplies the annotation of every file).  Single GPU.
"""
import argparse
import io
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd.data import JpegDecoder, collate_train_mosaic  # noqa: E402
from pytorch_object_detection_amd.model.loss import FCOSLoss  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import ATSSGenTargets, FCOSGenTargets  # noqa: E402
from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS  # noqa: E402


def synthetic_jpeg(rng):
    """One VOC-shaped JPEG stream."""
    from PIL import Image
    h, w = [(375, 500), (500, 375), (333, 500), (480, 640)][int(rng.integers(0, 4))]
    y, x = np.mgrid[0:h, 0:w]
    px = np.clip(np.stack([(x + 2 * y) % 256, (3 * x + y) % 256, (x * y // 64) % 256], -1) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(px, "RGB").save(buf, "JPEG", quality=90)
    return buf.getvalue()


def synthetic_boxes(rng, h, w):
    """fp32 boxes (x1, y1, x2, y2) and classes for an h x w image, on the host."""
    n = int(rng.integers(1, 6))
    xy = rng.uniform(0, 0.6, (n, 2)) * [w, h]
    wh = rng.uniform(0.1, 0.35, (n, 2)) * [w, h]
    return np.concatenate([xy, xy + wh], 1).astype(np.float32), rng.integers(1, 21, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--side", type=int, default=512, help="canvas side, a multiple of 32")
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--assigner", choices=["fcos", "atss"], default="fcos", help="target assignment: FCOSGenTargets or ATSSGenTargets")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = HalfInvertedStageFCOS([512, 1024, 2048], 20, 256).to(dev)
    gen_target = FCOSGenTargets(strides=[8, 16, 32, 64, 128], limit_range=[[-1, 64], [64, 128], [128, 256], [256, 512], [512, 999999]])
    if args.assigner == "atss":
        gen_target = ATSSGenTargets(strides=[8, 16, 32, 64, 128])
    LR_INIT, WARMUP_STEPS = 1e-3, 501
    optimizer = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=LR_INIT, momentum=0.9, weight_decay=1e-4)
    scaler = torch.amp.GradScaler("cuda", enabled=args.amp)
    criterion = FCOSLoss("giou")
    decoder = JpegDecoder(dev)
    data_rng, aug_rng = np.random.default_rng(100), random.Random(100)
    pool = list(args.files) or [synthetic_jpeg(data_rng) for _ in range(2 * args.batch)]          # paths or bytes: decode() takes both
    model.train()
    t0 = None
    for step in range(1, args.steps + 1):
        blobs = [pool[int(data_rng.integers(0, len(pool)))] for _ in range(args.batch)]
        images = decoder.decode(blobs)                                       # list of CUDA uint8 [h, w, 3]
        truth = [synthetic_boxes(data_rng, int(t.shape[0]), int(t.shape[1])) for t in images]
        imgs, targets, classes = collate_train_mosaic(images, [b for b, _ in truth], [c for _, c in truth], (args.side, args.side), rng=aug_rng,
                                                      fill=(114, 114, 114))
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
            print(f"step {step:4d}  canvas {tuple(imgs.shape[2:])}  boxes {int((classes >= 0).sum())}  cls {float(losses[0].detach()):.4f}  "
                  f"cnt {float(losses[1].detach()):.4f}  reg {float(losses[2].detach()):.4f}  total {float(losses[3].detach()):.4f}")
    torch.cuda.synchronize()
    if t0 is not None and args.steps > 3:
        dt = (time.perf_counter() - t0) / (args.steps - 3)
        print(f"{dt * 1e3:.1f} ms/step, {args.batch / dt:.1f} img/s (decoding and the synthetic boxes inside the loop)")


if __name__ == "__main__":
    main()
