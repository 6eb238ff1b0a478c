"""Time of the cross-rank merge of sharded evaluation (VOCEvaluator.gather / COCOEvaluator.gather) over RCCL; prints one JSON line.

    python tools/time_eval_gather.py [--reps 5]

One process, world size 1, force=True: the real ncclAllGather runs, but nothing crosses a link, so the collective times are the
floor (launch + local copy), not an 8-GPU figure.  Sizes: a rank's share of VOC07-test over 8 ranks (619 images) and the whole
of it (4 952), K = 1 000 detections and G = 5 GT rows per image; a rank's share of COCO-val over 8 ranks (625 images, K = 1 000).
Per case, median of --reps after one warm-up, wall clock between device synchronisations:
  sizes_ms    collective 1, the ranks' sizes (a few int64)
  payload_ms  collective 2, the uint8 payload (payload_bytes per rank)
  merge_ms    the rest of gather(): padding and packing the payload, unpacking it, merge_order on the host, the row select
  total_ms    gather() as a whole
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd.Test_coco import COCOEvaluator  # noqa: E402
from pytorch_object_detection_amd.test import VOCEvaluator  # noqa: E402


def voc_evaluator(n, K, G, dev):
    g = torch.Generator().manual_seed(n)
    ev = VOCEvaluator(21, (0.5,), device=dev)
    ids = torch.randperm(n, generator=g).tolist()
    for i in range(0, n, 512):
        b = min(512, n - i)
        xy = torch.rand(b, K, 2, generator=g) * 400
        gxy = torch.rand(b, G, 2, generator=g) * 400
        ev.add(torch.rand(b, K, generator=g).to(dev), torch.randint(1, 21, (b, K), generator=g).to(dev),
               torch.cat([xy, xy + 50], 2).to(dev), None, torch.cat([gxy, gxy + 50], 2).to(dev),
               torch.randint(1, 21, (b, G), generator=g).to(dev), image_ids=ids[i:i + b])
    return ev


def coco_evaluator(n, K, dev):
    g = torch.Generator().manual_seed(n)
    ds = {"images": [{"id": i} for i in range(1, n + 1)], "categories": [{"id": c} for c in range(1, 81)],
          "annotations": [{"id": i, "image_id": i, "category_id": 1 + i % 80, "bbox": [10., 10., 50., 50.], "iscrowd": 0, "area": 2500.}
                          for i in range(1, n + 1)]}
    ev = COCOEvaluator(ds, device=dev)
    ids = (torch.randperm(n, generator=g) + 1).tolist()
    for i in range(0, n, 512):
        b = min(512, n - i)
        xy = torch.rand(b, K, 2, generator=g) * 400
        ev.add(ids[i:i + b], torch.rand(b, K, generator=g).to(dev), torch.randint(1, 81, (b, K), generator=g).to(dev),
               torch.cat([xy, xy * 0 + 50], 2).to(dev), None)
    return ev


def time_gather(ev, reps):
    real = dist.all_gather_into_tensor
    spans = []

    def timed(out, inp, group=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        real(out, inp, group=group)
        torch.cuda.synchronize()
        spans.append((time.perf_counter() - t0, inp.numel() * inp.element_size()))

    rows = []
    dist.all_gather_into_tensor = timed
    try:
        for rep in range(reps + 1):
            del spans[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merged = ev.gather(force=True)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            assert len(spans) == 2 and merged.num_images == ev.num_images
            if rep:     # the first pass warms RCCL and the allocator
                rows.append((spans[0][0], spans[1][0], total - spans[0][0] - spans[1][0], total))
            nbytes = spans[1][1]
            del merged
    finally:
        dist.all_gather_into_tensor = real
    med = [round(float(np.median([r[k] for r in rows])) * 1e3, 3) for k in range(4)]
    return {"sizes_ms": med[0], "payload_ms": med[1], "merge_ms": med[2], "total_ms": med[3], "payload_bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_gather.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("nccl", init_method=f"file://{os.path.join(tmp, 'rdzv')}", rank=0, world_size=1, device_id=dev)
        try:
            for n in (619, 4952):
                cases.append(dict({"evaluator": "voc", "rows": n, "K": 1000, "G": 5}, **time_gather(voc_evaluator(n, 1000, 5, dev), a.reps)))
            cases.append(dict({"evaluator": "coco", "rows": 625, "K": 1000}, **time_gather(coco_evaluator(625, 1000, dev), a.reps)))
        finally:
            dist.destroy_process_group()
    print(json.dumps({"tool": "time_eval_gather", "device": torch.cuda.get_device_name(0), "backend": "nccl", "world": 1, "reps": a.reps,
                      "cases": cases}))


if __name__ == "__main__":
    main()
