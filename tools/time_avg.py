"""Device and host time of averaging the weights (optim.AveragedModel) at HISFCOS-R50's real parameter and buffer list; prints one JSON line.

    python tools/time_avg.py [--reps 30] [--inner 10]

The model is Builder(cfg).model_build() with 20 classes; it is not trained here, the bytes an update moves do not depend on the values.  Four sequences in ONE
run and alternating, each one update_parameters(model) of an averaged copy of its own:
  ours_ema / ours_swa    optim.AveragedModel(model, decay=0.999) / (model): one begin launch, one update launch per 64 fp32 tensors, one copy launch per 64 buffers
  stock_ema / stock_swa  torch.optim.swa_utils.AveragedModel(model, device, multi_avg_fn=get_ema_multi_avg_fn(0.999)) / (model, device): two host reads of
                         n_averaged (on the device, as a checkpoint moved with .to(device) has it), the foreach lerp, one copy_ per buffer
step_ms          median device-event time of --inner back-to-back calls, per call
host_enqueue_ms  median host clock around one call that is NOT followed by a synchronise (the stock sequences synchronise inside: their reads of n_averaged)
graph_replay_ms  ours alone -- the stock sequence cannot be captured: the call captured once with torch.cuda.graph and replayed, --inner replays per event
                 pair; with the bytes moved (12 B per averaged element, 2 B per copied byte) that is a rate, given over the 8000 GB/s HBM figure bench.py uses
launches         ours: begin + update + copy launches of one call; the stock class's foreach kernels chunk inside torch and are not counted here
No figure here is a pass / fail bar.
"""
import argparse
import json
import os
import sys
import time

import torch
from torch.optim import swa_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import optim  # noqa: E402
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
DECAY = 0.999


def device_ms(fn, inner):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    st.record()
    for _ in range(inner):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / inner


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return dt


def graphed(fn):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_avg.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    cfg = load_config()
    cfg["model"]["name"] = "HISFCOS"
    cfg["dataset_setting"]["class_num"] = 20
    model = Builder(cfg).model_build().to(dev)
    n_params, n_buffers = len(list(model.parameters())), len(list(model.buffers()))
    elements = sum(p.numel() for p in model.parameters())
    buffer_bytes = sum(b.numel() * b.element_size() for b in model.buffers())
    moved = 12 * elements + 2 * buffer_bytes

    avgs = {"ours_ema": optim.AveragedModel(model, decay=DECAY), "ours_swa": optim.AveragedModel(model),
            "stock_ema": swa_utils.AveragedModel(model, dev, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(DECAY)),
            "stock_swa": swa_utils.AveragedModel(model, dev)}                                   # device=: n_averaged on the device, as ours keeps it
    seqs = {k: (lambda m=m: m.update_parameters(model)) for k, m in avgs.items()}
    for _ in range(5):
        for fn in seqs.values():
            fn()
    graphs = {k: graphed(fn) for k, fn in seqs.items() if k.startswith("ours")}
    dev_t, host_t, graph_t = {k: [] for k in seqs}, {k: [] for k in seqs}, {k: [] for k in graphs}
    for _ in range(a.reps):                                  # alternating, so a drift of the machine reaches all alike
        for k, fn in seqs.items():
            dev_t[k].append(device_ms(fn, a.inner))
            host_t[k].append(host_ms(fn))
            if k in graphs:
                graph_t[k].append(device_ms(graphs[k].replay, a.inner))
    out = {"tool": "time_avg", "device": torch.cuda.get_device_name(0), "model": "HISFCOS-R50, 20 classes", "parameters": n_params, "buffers": n_buffers,
           "elements": elements, "buffer_bytes": buffer_bytes, "bytes_moved": moved, "peak_hbm_GBps": PEAK_HBM_GBS, "decay": DECAY, "reps": a.reps,
           "inner": a.inner}
    for k in seqs:
        out[k] = {"step_ms": round(median(dev_t[k]), 4), "step_ms_min": round(min(dev_t[k]), 4), "step_ms_max": round(max(dev_t[k]), 4),
                  "host_enqueue_ms": round(median(host_t[k]), 4), "launches": avgs[k].launches if k in graphs else None}
        if k in graphs:
            ms = median(graph_t[k])
            gbps = moved / (ms * 1e-3) / 1e9
            out[k].update({"graph_replay_ms": round(ms, 4), "graph_replay_ms_min": round(min(graph_t[k]), 4), "graph_replay_ms_max": round(max(graph_t[k]), 4),
                           "GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBS, 4)})
    out["ours_over_stock"] = {m: round(out["ours_" + m]["step_ms"] / out["stock_" + m]["step_ms"], 4) for m in ("ema", "swa")}
    out["note"] = ("step_ms of back-to-back calls is bound by the slower of device work and host enqueue; where host_enqueue_ms exceeds the device time of the "
                   "bytes, step_ms measures the host (a replayed graph does not pay it)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
