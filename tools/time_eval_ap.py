"""Device time of VOC AP evaluation (VOCEvaluator.compute, fd_eval_ap) at dataset sizes; prints one JSON line.

    python tools/time_eval_ap.py [--reps 5]

Sizes: 4 952 images (VOC07 test) x {100, 300, 1 000} detections x 20 classes at IoU 0.5, and 5 000 images x 1 000 detections x
80 classes x 10 thresholds (0.5 .. 0.95).  1-5 GT boxes per image (VOC) / 1-15 (80 classes); detections are jittered GT boxes and
random boxes with random scores.  compute_ms: warm device-event time of compute() (one fd_eval_ap call + the packed result copy),
median of --reps; add_us_per_batch: device-event time of add() per batch of 16 images.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd.test import VOCEvaluator  # noqa: E402


def synth(n_img, n_det, num_cls, max_gt, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    G = max_gt
    xy = torch.rand(n_img, G, 2, generator=g, device=dev) * 400
    wh = torch.rand(n_img, G, 2, generator=g, device=dev) * 110 + 10
    gt_boxes = torch.cat([xy, xy + wh], 2)
    gt_classes = torch.randint(1, num_cls, (n_img, G), generator=g, device=dev)
    n_gt = torch.randint(1, max_gt + 1, (n_img,), generator=g, device=dev)
    gt_classes = torch.where(torch.arange(G, device=dev)[None] < n_gt[:, None], gt_classes, torch.full_like(gt_classes, -1))
    src = torch.randint(0, G, (n_img, n_det), generator=g, device=dev) % n_gt[:, None]
    boxes = torch.gather(gt_boxes, 1, src[..., None].expand(-1, -1, 4)) + torch.randn(n_img, n_det, 4, generator=g, device=dev) * 8
    far = torch.rand(n_img, n_det, 1, generator=g, device=dev) < 0.5
    rxy = torch.rand(n_img, n_det, 2, generator=g, device=dev) * 400
    boxes = torch.where(far, torch.cat([rxy, rxy + torch.rand(n_img, n_det, 2, generator=g, device=dev) * 110 + 10], 2), boxes)
    classes = torch.where(torch.rand(n_img, n_det, generator=g, device=dev) < 0.7, torch.gather(gt_classes, 1, src),
                          torch.randint(1, num_cls, (n_img, n_det), generator=g, device=dev))
    scores = torch.sort(torch.rand(n_img, n_det, generator=g, device=dev) * 0.95 + 0.05, dim=1, descending=True)[0]
    return scores, classes, boxes.contiguous(), gt_boxes, gt_classes


def time_case(n_img, n_det, num_cls, thr, max_gt, reps, dev, batch=16):
    data = synth(n_img, n_det, num_cls, max_gt, n_img + n_det + num_cls, dev)
    ev = VOCEvaluator(num_cls, thr)
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    add_ms = []
    for i in range(0, n_img, batch):
        sl = slice(i, min(i + batch, n_img))
        st.record()
        ev.add(data[0][sl], data[1][sl], data[2][sl], None, data[3][sl], data[4][sl])
        en.record()
        if i < 20 * batch:
            torch.cuda.synchronize()
            add_ms.append(st.elapsed_time(en))
    ev.compute()                                  # warm-up (code objects, workspace)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        st.record()
        res = ev.compute()
        en.record()
        torch.cuda.synchronize()
        ms.append(st.elapsed_time(en))
    ms.sort()
    add_ms.sort()
    return {"images": n_img, "detections": n_det, "classes": num_cls - 1, "thresholds": len(thr),
            "compute_ms": round(ms[len(ms) // 2], 3), "compute_ms_min": round(ms[0], 3),
            "add_us_per_batch": round(1000 * add_ms[len(add_ms) // 2], 1), "mAP": float(res["mAP"][0]),
            "tp": int(res["n_tp"][0].sum()), "pred": int(res["n_pred"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_ap.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    cases = [time_case(4952, k, 21, (0.5,), 5, a.reps, dev) for k in (100, 300, 1000)]
    cases.append(time_case(5000, 1000, 81, tuple(0.5 + 0.05 * i for i in range(10)), 15, a.reps, dev))
    print(json.dumps({"tool": "time_eval_ap", "device": torch.cuda.get_device_name(0), "cases": cases}))


if __name__ == "__main__":
    main()
