"""Device time of the on-device input resize (ops.resize_collate_u8, fd_resize_collate_u8_nhwc4) at detection sizes; prints one JSON line.

    python tools/time_resize.py [--reps 20] [--batch 16] [--threads 16]

Cases: --batch synthetic raw uint8 images -> resize_size (800, 1333) by the reference's size rule (utill.utills.resize_rule):
"landscape" = all 480 x 640; "mixed" = 480 x 640, 640 x 480, 375 x 500 and 500 x 375 in turn.  Per case:
  resize_collate_ms   warm device-event median (and minimum) of the ONE launch that resizes, pads and normalises the batch
                      (ten launches per event pair, tables already on the device); op_with_table_upload_ms: ops.resize_collate_u8
                      as forward_raw calls it, pointer / size tables built and uploaded inside the timed window;
  bytes               what that launch must move: 16 * N * H * W written + the raw images (sum of 3 * h_n * w_n) read once;
  GBps / hbm_frac     bytes over the median, and that rate over the 8000 GB/s HBM figure bench.py uses (PEAK_HBM_GBS);
  host_path           for scale only -- the path the parent commit offers: bilinear resize on the host with torch
                      (F.interpolate on --threads CPU threads, rounded back to uint8: a STAND-IN for the absent cv2.resize, not
                      cv2 itself), the H2D copy of the RESIZED images, and forward_images' collate launch (ops.collate_u8).
                      host_resize_ms is a host clock, h2d_resized_ms a host clock around copies that end in a synchronise,
                      collate_ms a device-event median.  h2d_raw_ms: the same copy for the raw images, which is all the
                      device path needs.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd.utill.utills import pad32, resize_rule  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESIZE_SIZE = (800, 1333)


def median_ms(fn, reps, inner=1):
    """Median and minimum device-event time of fn() in ms; `inner` back-to-back calls share one event pair (a launch of tens of
    microseconds is otherwise measured together with the event records around it)."""
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


def host_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def time_case(name, sizes, reps, dev):
    gen = torch.Generator().manual_seed(len(sizes) + sizes[0][0])
    raw = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in sizes]
    rules = [resize_rule(h, w, RESIZE_SIZE) for h, w in sizes]
    dst = [(nh, nw) for _, nh, nw in rules]
    H, W = max(pad32(a) for a, _ in dst), max(pad32(b) for _, b in dst)
    N = len(raw)
    raw_dev = [t.to(dev) for t in raw]
    out = torch.empty(N * H * W, 4, dtype=torch.float32, device=dev)
    # the launch alone (tables already on the device), then the whole op (pointer / size tables rebuilt and uploaded per call)
    _, (ptrs, hw, _) = ops.resize_collate_u8(raw_dev, dst, H, W, MEAN, STD, out=out)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    m3, s3 = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def launch():
        _lib.check(lib.fd_resize_collate_u8_nhwc4(ptrs.data_ptr(), hw.data_ptr(), hw.data_ptr() + 8 * N, out.data_ptr(), N, H, W, m3, s3, stream))
    med, mn = median_ms(launch, reps, inner=10)
    op_med, _ = median_ms(lambda: ops.resize_collate_u8(raw_dev, dst, H, W, MEAN, STD, out=out), reps)
    nbytes = 16 * N * H * W + sum(3 * h * w for h, w in sizes)
    gbps = nbytes / (med * 1e-3) / 1e9

    # the parent commit's path, for scale: host resize (torch stand-in for cv2) + H2D of the resized images + the collate launch
    def host_resize():
        res = []
        for t, (nh, nw) in zip(raw, dst):
            x = t.permute(2, 0, 1)[None].float()
            y = torch.nn.functional.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False)
            res.append(y.add_(0.5).clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous())
        return res
    resized = host_resize()
    host_resize_ms = host_ms(host_resize, max(3, reps // 4))

    def h2d(imgs):
        def go():
            keep = [t.to(dev) for t in imgs]
            torch.cuda.synchronize()
            return keep
        return go
    h2d_resized_ms = host_ms(h2d(resized), max(3, reps // 2))
    h2d_raw_ms = host_ms(h2d(raw), max(3, reps // 2))
    resized_dev = [t.to(dev) for t in resized]
    _, (cptrs, chw, _) = ops.collate_u8(resized_dev, H, W, MEAN, STD, out=out)
    col_med, _ = median_ms(lambda: _lib.check(lib.fd_collate_u8_nhwc4(cptrs.data_ptr(), chw.data_ptr(), out.data_ptr(), N, H, W, m3, s3, stream)),
                           reps, inner=10)
    return {"case": name, "images": N, "raw_hw": sorted(set(sizes)), "canvas_hw": [H, W], "resize_collate_ms": round(med, 4),
            "resize_collate_ms_min": round(mn, 4), "op_with_table_upload_ms": round(op_med, 4), "bytes": nbytes, "GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBS, 4),
            "h2d_raw_ms": round(h2d_raw_ms, 3),
            "host_path": {"host_resize_ms": round(host_resize_ms, 3), "h2d_resized_ms": round(h2d_resized_ms, 3), "collate_ms": round(col_med, 4),
                          "total_ms": round(host_resize_ms + h2d_resized_ms + col_med, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_resize.py measures on the GPU; none found")
    torch.set_num_threads(a.threads)
    dev = torch.device("cuda", 0)
    mixed = [(480, 640), (640, 480), (375, 500), (500, 375)]
    cases = [time_case("landscape", [(480, 640)] * a.batch, a.reps, dev),
             time_case("mixed", [mixed[i % 4] for i in range(a.batch)], a.reps, dev)]
    print(json.dumps({"tool": "time_resize", "device": torch.cuda.get_device_name(0), "resize_size": list(RESIZE_SIZE), "peak_hbm_GBps": PEAK_HBM_GBS,
                      "host_threads": a.threads,
                      "host_path_note": "host resize = torch F.interpolate bilinear on the CPU, a stand-in for the absent cv2.resize",
                      "cases": cases}))


if __name__ == "__main__":
    main()
