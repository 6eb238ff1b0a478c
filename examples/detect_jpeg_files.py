#!/usr/bin/env python3
"""JPEG files in, detections in the files' own pixel coordinates out: detect_raw(decoder.decode(blobs), head).

    python examples/detect_jpeg_files.py [FILE.jpg ...] [--batch 4]

The reference opens every image with Image.open(path).convert('RGB') on the host (dataset/voc.py:69, Test_coco.py via
dataset/coco.py).  Here the host reads the bytes, parses the markers and undoes the Huffman coding (data.jpeg.JpegDecoder, a few
threads); dequantisation, inverse DCT, chroma upsampling and colour conversion run on the MI355X in two launches per batch, and the
decoded uint8 [h, w, 3] images go straight into detect_raw: size rule, resize, pad, normalise, model, FCOSHead, ClipBoxes,
boxes / scale -- nothing returns to the host before the detections do.  A progressive or CMYK file is decoded by Pillow on the host
and uploaded (fallback="pil"); a corrupt one raises FdError naming its index.

Without FILE arguments the example encodes a few synthetic images with Pillow first.
"""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402
from pytorch_object_detection_amd.data import JpegDecoder  # noqa: E402
from pytorch_object_detection_amd.model.modules.head import FCOSHead  # noqa: E402


def synthetic(n: int):
    from PIL import Image
    rng = np.random.default_rng(0)
    blobs = []
    for i in range(n):
        h, w = [(375, 500), (500, 375), (480, 640), (333, 500)][i % 4]
        y, x = np.mgrid[0:h, 0:w]
        px = np.clip(np.stack([(x + 2 * y) % 256, (3 * x + y) % 256, (x * y // 64) % 256], -1) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(px, "RGB").save(buf, "JPEG", quality=90, subsampling=[2, 1, 0][i % 3])
        blobs.append(buf.getvalue())
    return blobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = load_config()                      # COCO / HISFCOS, 80 classes
    model = Builder(cfg).model_build().eval().to(dev)
    head = FCOSHead(0.05, 0.6, 1000, cfg["HISFCOS"]["stride"])
    decoder = JpegDecoder(dev)               # fallback="pil": files the HIP path does not take are decoded by Pillow
    blobs = list(args.files) or synthetic(2 * args.batch)       # paths or bytes: decode() takes both
    for lo in range(0, len(blobs), args.batch):
        part = blobs[lo:lo + args.batch]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        images = decoder.decode(part)                            # list of CUDA uint8 [h, w, 3]
        scores, classes, boxes, counts, scales = model.detect_raw(images, head)
        counts = counts.tolist()                                 # the first host read of the batch
        dt = time.perf_counter() - t0
        for k, t in enumerate(images):
            name = part[k] if isinstance(part[k], str) else f"image {lo + k}"
            print(f"{name}: {t.shape[0]}x{t.shape[1]}, {counts[k]} detections, best score {float(scores[k, 0]) if counts[k] else 0.0:.3f}")
        print(f"batch of {len(part)}: {dt * 1e3:.1f} ms from bytes to detections")


if __name__ == "__main__":
    main()
