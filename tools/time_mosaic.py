"""Device time of the mosaic launch (ops.mosaic_collate_u8 / fd_mosaic_collate_u8, data.augment.collate_train_mosaic)
at a detection size; prints one JSON line.

    python tools/time_mosaic.py [--reps 20] [--batch 16] [--side 640]

--batch outputs on a --side x --side canvas from --batch raw sources, 375 x 500 and 500 x 375 in turn; output n holds sources n,
n + 1, n + 2, n + 3 (mod batch), corners at a centre that moves with n, the long side of every tile resized to 0.75 * side.  Warm
device-event medians (ten launches per event pair, tables already on the device):
  mosaic_identity_ms       the launch with identity records (resize + place + fill + normalise only)
  mosaic_geometric_ms      flip + rotation + crop on every tile
  mosaic_full_ms           flip + rotation + crop + a full colour chain (four operations, contrast means already in the records)
  l_sums_ms                fd_jitter_l_sums over the 4 * batch records
  bytes_written            N * 3 * H * W * 4
  bytes_read_bound         an upper bound of the bytes read: four taps of three bytes per canvas pixel, but never more than the
                           4 * N sources as a whole, plus the tables
  GBps / hbm_frac          (bytes_written + bytes_read_bound) over the identity median, and that rate over the 8000 GB/s HBM figure
  collate_train_mosaic_ms  data.augment.collate_train_mosaic as a whole, seeded rng: device-event median, and host wall-clock median
                           with a synchronise at the end (it includes the host's sampling and box work)
  collate_train_raw_ms     data.augment.collate_train_raw on the same images with a size rule that yields the same canvas, likewise
  amp_step_ms              the AMP training step for 16 images, for scale
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
from pytorch_object_detection_amd.data.augment import collate_train_mosaic, collate_train_raw  # noqa: E402
from pytorch_object_detection_amd.utill.utills import resize_rule  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
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


def wall_ms(fn, reps):
    walls = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    return walls[len(walls) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=640)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mosaic.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    N, H, W = a.batch, a.side, a.side
    sizes = [[(375, 500), (500, 375)][i % 2] for i in range(N)]
    gen = torch.Generator().manual_seed(N)
    raw_dev = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen).to(dev) for h, w in sizes]
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L = int(0.75 * max(H, W))
    centres = [(W // 4 + (n * 37) % (W // 2), H // 4 + (n * 53) % (H // 2)) for n in range(N)]

    def tiles_for(geometric, chain):
        out = []
        for n in range(N):
            xc, yc = centres[n]
            quad = []
            for t in range(4):
                src = (n + t) % N
                h, w = sizes[src]
                crop = (w // 10, h // 8, w - w // 5, h - h // 4) if geometric else None
                ch, cw = (crop[3], crop[2]) if crop else (h, w)
                _, nh, nw = resize_rule(ch, cw, (L, L))
                quad.append(dict(src=src, px=xc if t & 1 else xc - nw, py=yc if t & 2 else yc - nh, nh=nh, nw=nw, flip=geometric and (n + t) % 2 == 0,
                                 d=(7.5 if t % 2 else -9.0) if geometric else 0.0, crop=crop, chain=chain))
            out.append(quad)
        return out

    variants = {"mosaic_identity": tiles_for(False, []), "mosaic_geometric": tiles_for(True, []), "mosaic_full": tiles_for(True, FULL_CHAIN)}
    out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    res = {"tool": "time_mosaic", "device": torch.cuda.get_device_name(0), "outputs": N, "canvas_hw": [H, W], "raw_hw": sorted(set(sizes)), "tile_long_side": L,
           "peak_hbm_GBps": PEAK_HBM_GBS}
    S = 4 * N
    for key, tiles in variants.items():
        _, (tab, _, _) = ops.mosaic_collate_u8(raw_dev, tiles, centres, H, W, MEAN, STD, out=out)      # tables (and contrast means) now on the device
        ptrs, recs, place = tab[:2 * S].view(torch.int64), tab[2 * S:S * (ops.AUG_WORDS + 2)], tab[S * (ops.AUG_WORDS + 2):]
        med, mn = median_ms(lambda: _lib.check(lib.fd_mosaic_collate_u8(ptrs.data_ptr(), recs.data_ptr(), place.data_ptr(), out.data_ptr(), N, H, W, m3, s3,
                                                                        stream)), a.reps, inner=10)
        res[key + "_ms"], res[key + "_ms_min"] = round(med, 4), round(mn, 4)
        if key == "mosaic_full":
            sums = torch.empty(S, dtype=torch.int64, device=dev)
            mp = max(h * w for h, w in sizes)
            l_med, _ = median_ms(lambda: _lib.check(lib.fd_jitter_l_sums(ptrs.data_ptr(), recs.data_ptr(), sums.data_ptr(), S, mp, stream)), a.reps, inner=10)
            res["l_sums_ms"] = round(l_med, 4)
    written = N * 3 * H * W * 4
    tables = S * (ops.AUG_WORDS + 2) * 4 + N * ops.MOSAIC_WORDS * 4
    read_bound = min(12 * N * H * W, sum(3 * sizes[(n + t) % N][0] * sizes[(n + t) % N][1] for n in range(N) for t in range(4))) + tables
    gbps = (written + read_bound) / (res["mosaic_identity_ms"] * 1e-3) / 1e9
    res.update({"bytes_written": written, "bytes_read_bound": read_bound, "GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBS, 4)})
    # the whole entry points: sampling, records, uploads, launches
    brng = np.random.default_rng(3)
    boxes = []
    for h, w in sizes:
        xy = brng.uniform(0, 0.6, (4, 2)) * [w, h]
        boxes.append(np.concatenate([xy, xy + brng.uniform(0.1, 0.35, (4, 2)) * [w, h]], 1).astype(np.float32))
    classes = [np.arange(1, 5)] * N
    rng = random.Random(7)
    mosaic = lambda: collate_train_mosaic(raw_dev, boxes, classes, (H, W), rng=rng)      # noqa: E731
    # short side to 0.7125 * side, long side capped at 0.95 * side: 375 x 500 -> 456 x 608 at 640, padded to the same side x side canvas
    raw_rule = (int(H * 0.7125), int(H * 0.95))
    raw = lambda: collate_train_raw(raw_dev, boxes, classes, raw_rule, rng=rng)          # noqa: E731
    res["collate_train_raw_canvas_hw"] = list(raw()[0].shape[2:])
    for key, fn in (("collate_train_mosaic", mosaic), ("collate_train_raw", raw)):
        med, _ = median_ms(fn, a.reps)
        wall = wall_ms(fn, a.reps)
        res.update({key + "_ms": round(med, 4), key + "_wall_ms": round(wall, 4), key + "_wall_over_amp_step": round(wall / AMP_STEP_MS, 4)})
    res["amp_step_ms"] = AMP_STEP_MS
    print(json.dumps(res))


if __name__ == "__main__":
    main()
