"""Host and device time of JPEG decoding for the device (data.jpeg.JpegDecoder, csrc/fd_jpeg.hip) against the route the reference takes;
prints one JSON line.

    python tools/time_jpeg.py [--reps 20] [--batch 16] [--no-detect]

Workload: --batch images, 375 x 500 and 500 x 375 in turn, 4:2:0, quality 75 and quality 90, content from the fixture generator
(tests/golden/make_g16_jpeg.py: ramps plus noise; no data set is assumed).  Needs PIL (the encoder, and route (a)).  Per quality:
  a_pillow_ms_{1,16}thr     np.asarray(Image.open(...).convert('RGB')) of every image + its upload, on 1 thread and on 16: host wall clock, ends in a synchronise
  b_host_ms_{1,16}thr       fd_jpeg_parse + fd_jpeg_entropy_decode of every image on 1 thread and on 16: host wall clock, no device involved
  c_idct / c_color          each launch alone, warm device-event median (ten launches per event pair): ms, the bytes it must move (coefficients read + planes
                            written; planes read + images written), GB/s and that rate over the 8000 GB/s HBM figure bench.py uses
  d_decode_ms               JpegDecoder.decode as a whole: host wall clock with a synchronise at the end, and the device-event time of the same calls
  d_detect_*                decode + detect_raw against detect_raw on images already resident (HISFCOS-R50, 80 classes, the size rule's (800, 1333)); wall clock
All host figures are medians over --reps calls after three warm-up calls; per-image figures divide by the batch.
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from pytorch_object_detection_amd import ops  # noqa: E402
from pytorch_object_detection_amd.data.jpeg import JpegDecoder  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
DEV = "cuda:0"


def wall_ms(fn, reps, sync=True):
    for _ in range(3):
        fn()
    if sync:
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms[len(ms) // 2]


def event_ms(fn, reps, inner=1):
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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-detect", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_jpeg.py measures on the GPU; none is visible")
    from PIL import Image
    import make_g16_jpeg as M

    B = args.batch
    sizes = [(375, 500) if k % 2 == 0 else (500, 375) for k in range(B)]
    pool = ThreadPoolExecutor(16)
    res = {"tool": "time_jpeg", "device": torch.cuda.get_device_name(0), "batch": B, "sizes": "375x500 / 500x375 in turn", "sampling": "4:2:0", "reps": args.reps,
           "pillow": __import__("PIL").__version__, "qualities": {}}
    model = head = None
    if not args.no_detect:
        from pytorch_object_detection_amd.model.modules.head import FCOSHead
        from pytorch_object_detection_amd.model.od import HalfInvertedStageFCOS
        torch.manual_seed(0)
        model = HalfInvertedStageFCOS([512, 1024, 2048], 80, 256).eval().to(DEV)
        head = FCOSHead(0.05, 0.6, 1000, [8, 16, 32, 64, 128])
    for quality in (75, 90):
        blobs = [M.encode(M.image(h, w, 100 * quality + k), 2, quality, 0, False) for k, (h, w) in enumerate(sizes)]
        streams = [np.frombuffer(b, np.uint8) for b in blobs]
        r = {"stream_bytes_mean": int(np.mean([len(b) for b in blobs]))}

        def pil_one(b):
            return torch.from_numpy(np.asarray(Image.open(io.BytesIO(b)).convert("RGB")).copy()).to(DEV)

        def host_one(s):
            return ops.jpeg_entropy_decode(s, ops.jpeg_parse(s))

        r["a_pillow_ms_1thr"] = wall_ms(lambda: [pil_one(b) for b in blobs], args.reps)
        r["a_pillow_ms_16thr"] = wall_ms(lambda: list(pool.map(pil_one, blobs)), args.reps)
        r["a_pillow_decode_only_ms_1thr"] = wall_ms(lambda: [np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs], args.reps, sync=False)
        r["b_host_ms_1thr"] = wall_ms(lambda: [host_one(s) for s in streams], args.reps, sync=False)
        r["b_host_ms_16thr"] = wall_ms(lambda: list(pool.map(host_one, streams)), args.reps, sync=False)
        r["a_per_image_ms_1thr"] = r["a_pillow_decode_only_ms_1thr"] / B
        r["b_per_image_ms_1thr"] = r["b_host_ms_1thr"] / B
        r["b_over_a_1thr"] = r["b_host_ms_1thr"] / r["a_pillow_decode_only_ms_1thr"]

        dec = JpegDecoder(DEV, fallback="raise")
        dec.keep_last = True
        imgs = dec.decode(blobs)
        torch.cuda.synchronize()
        for t, b in zip(imgs[:2], blobs[:2]):            # the timed code computes Pillow's pixels
            assert np.array_equal(t.cpu().numpy(), np.asarray(Image.open(io.BytesIO(b)).convert("RGB")))
        L = dec.last
        qt = L["tab"][:L["q_bytes"]].view(torch.int16).view(L["n_jobs"], 64)
        ij, cj = L["tab"][L["q_bytes"]:L["q_bytes"] + L["ij_bytes"]], L["tab"][L["q_bytes"] + L["ij_bytes"]:]
        elems, out_bytes = L["coefs"].numel(), sum(t.numel() for t in L["out"])
        for name, fn, nbytes in (("c_idct", lambda: ops.jpeg_idct_u8(L["idct_jobs"], ij, L["coefs"], qt, L["planes"]), 3 * elems),
                                 ("c_color", lambda: ops.jpeg_color_u8(L["color_jobs"], cj, L["planes"]), elems + out_bytes)):
            ms = event_ms(fn, args.reps, inner=10)
            r[name] = {"ms": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6, "hbm_frac": nbytes / ms / 1e6 / PEAK_HBM_GBS}
        dec.keep_last, dec.last = False, None
        r["d_decode_ms"] = wall_ms(lambda: dec.decode(blobs), args.reps)
        r["d_decode_device_ms"] = event_ms(lambda: dec.decode(blobs), args.reps)
        if model is not None:
            resident = dec.decode(blobs)
            with torch.no_grad():
                r["d_detect_resident_ms"] = wall_ms(lambda: model.detect_raw(resident, head), args.reps)
                r["d_detect_with_decode_ms"] = wall_ms(lambda: model.detect_raw(dec.decode(blobs), head), args.reps)
                r["d_detect_with_pillow_1thr_ms"] = wall_ms(lambda: model.detect_raw([pil_one(b) for b in blobs], head), args.reps)
        res["qualities"][str(quality)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
