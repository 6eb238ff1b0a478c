"""Device time of the on-device training augmentations (ops.augment_resize_collate_u8, fd_jitter_l_sums, data.augment.collate_train_raw)
at detection sizes; prints one JSON line.

    python tools/time_augment.py [--reps 20] [--batch 16]

Cases: the two batches of tools/time_resize.py -- "landscape" = --batch raw 480 x 640 images, "mixed" = 480 x 640, 640 x 480,
375 x 500, 500 x 375 in turn -- resized to (800, 1333) by the reference's size rule.  Per case, warm device-event medians (ten
launches per event pair, records already on the device):
  fused_identity_ms        the fused launch with identity parameters (resize + pad + normalise only)
  fused_geometric_ms       flip + rotation + crop on every image
  fused_full_ms            flip + rotation + crop + a full colour chain (four operations, contrast mean already in the records)
  l_sums_ms                fd_jitter_l_sums for the batch (memset + reduction + mean), the chain prefix saturation, brightness, hue
  resize_collate_ms        the existing evaluation-side launch (fd_resize_collate_u8_nhwc4) on the same images, for scale
  collate_train_raw_ms     data.augment.collate_train_raw as a whole, seeded rng, records and boxes uploaded per call: device-event
                           median (and host wall-clock median with a synchronise at the end: it includes the host's sampling)
  bytes / GBps / hbm_frac  what the identity launch must move (12 * N * H * W written + the raw images read once), over its median,
                           and that rate over the 8000 GB/s HBM figure bench.py uses
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd.data.augment import collate_train_raw  # noqa: E402
from pytorch_object_detection_amd.utill.utills import pad32, resize_rule  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESIZE_SIZE = (800, 1333)
AMP_STEP_MS = 16.8          # the AMP training step for 16 images
FULL_CHAIN = [(ops.AUG_OP_SATURATION, 1.07), (ops.AUG_OP_BRIGHTNESS, 0.93), (ops.AUG_OP_HUE, 20), (ops.AUG_OP_CONTRAST, 1.09)]


def median_ms(fn, reps, inner=1):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        st.record()
        for _ in range(inner):
            fn()
        en.record()
        torch.cuda.synchronize()
        ms.append(st.elapsed_time(en) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def time_case(name, sizes, reps, dev):
    gen = torch.Generator().manual_seed(len(sizes) + sizes[0][0])
    raw_dev = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).to(dev) for h, w in sizes]
    N = len(raw_dev)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def params_for(geometric, chain):
        out = []
        for k, (h, w) in enumerate(sizes):
            crop = (w // 10, h // 8, w - w // 5, h - h // 4) if geometric else None
            ch, cw = (crop[3], crop[2]) if crop else (h, w)
            _, nh, nw = resize_rule(ch, cw, RESIZE_SIZE)
            out.append(dict(flip=geometric and k % 2 == 0, d=(7.5 if k % 2 else -9.0) if geometric else 0.0, crop=crop, chain=chain, nh=nh, nw=nw))
        return out

    variants = {"fused_identity": params_for(False, []), "fused_geometric": params_for(True, []), "fused_full": params_for(True, FULL_CHAIN)}
    H = max(pad32(p["nh"]) for ps in variants.values() for p in ps)
    W = max(pad32(p["nw"]) for ps in variants.values() for p in ps)
    out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    res = {"case": name, "images": N, "raw_hw": sorted(set(sizes)), "canvas_hw": [H, W]}
    for key, ps in variants.items():
        _, (tab, _, _) = ops.augment_resize_collate_u8(raw_dev, ps, H, W, MEAN, STD, out=out)      # records (and contrast means) now on the device
        ptrs, recs = tab[:2 * N].view(torch.int64), tab[2 * N:].view(N, ops.AUG_WORDS)
        med, mn = median_ms(lambda: _lib.check(lib.fd_augment_resize_collate_u8(ptrs.data_ptr(), recs.data_ptr(), out.data_ptr(), N, H, W, m3, s3, stream)),
                            reps, inner=10)
        res[key + "_ms"], res[key + "_ms_min"] = round(med, 4), round(mn, 4)
        if key == "fused_full":
            sums = torch.empty(N, dtype=torch.int64, device=dev)
            mp = max(h * w for h, w in sizes)
            l_med, _ = median_ms(lambda: _lib.check(lib.fd_jitter_l_sums(ptrs.data_ptr(), recs.data_ptr(), sums.data_ptr(), N, mp, stream)), reps, inner=10)
            res["l_sums_ms"] = round(l_med, 4)
    nbytes = 12 * N * H * W + sum(3 * h * w for h, w in sizes)
    gbps = nbytes / (res["fused_identity_ms"] * 1e-3) / 1e9
    res.update({"bytes": nbytes, "GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBS, 4)})
    # the existing evaluation-side launch on the same images and canvas, for scale (16 bytes per canvas pixel)
    dst = [(p["nh"], p["nw"]) for p in variants["fused_identity"]]
    out4 = torch.empty(N * H * W, 4, dtype=torch.float32, device=dev)
    _, (eptrs, ehw, _) = ops.resize_collate_u8(raw_dev, dst, H, W, MEAN, STD, out=out4)
    e_med, _ = median_ms(lambda: _lib.check(lib.fd_resize_collate_u8_nhwc4(eptrs.data_ptr(), ehw.data_ptr(), ehw.data_ptr() + 8 * N, out4.data_ptr(), N, H, W,
                                                                           m3, s3, stream)), reps, inner=10)
    res["resize_collate_ms"] = round(e_med, 4)
    # the whole entry point: sampling, records, uploads, launches
    brng = np.random.default_rng(3)
    boxes = []
    for h, w in sizes:
        xy = brng.uniform(0, 0.6, (4, 2)) * [w, h]
        boxes.append(np.concatenate([xy, xy + brng.uniform(0.1, 0.35, (4, 2)) * [w, h]], 1).astype(np.float32))
    classes = [np.arange(1, 5)] * N
    rng = random.Random(7)
    whole = lambda: collate_train_raw(raw_dev, boxes, classes, RESIZE_SIZE, rng=rng)      # noqa: E731
    w_med, _ = median_ms(whole, reps)
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    res.update({"collate_train_raw_ms": round(w_med, 4), "collate_train_raw_wall_ms": round(walls[len(walls) // 2], 4),
                "amp_step_ms": AMP_STEP_MS, "collate_over_amp_step": round(w_med / AMP_STEP_MS, 4),
                "collate_wall_over_amp_step": round(walls[len(walls) // 2] / AMP_STEP_MS, 4)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_augment.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    mixed = [(480, 640), (640, 480), (375, 500), (500, 375)]
    cases = [time_case("landscape", [(480, 640)] * a.batch, a.reps, dev),
             time_case("mixed", [mixed[i % 4] for i in range(a.batch)], a.reps, dev)]
    print(json.dumps({"tool": "time_augment", "device": torch.cuda.get_device_name(0), "resize_size": list(RESIZE_SIZE), "peak_hbm_GBps": PEAK_HBM_GBS,
                      "cases": cases}))


if __name__ == "__main__":
    main()
