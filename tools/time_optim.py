"""Device and host time of one optimizer step() at HISFCOS-R50's real trainable list; prints one JSON line.

    python tools/time_optim.py [--reps 30] [--inner 10]

The parameters are those of Builder(cfg).model_build() with 20 classes, gradients are N(0, 1) tensors of the same shapes (allocated once, so this measures the
update alone, not a backward).  For SGD (momentum 0.9, weight decay 1e-4) and Adam, in ONE run and alternating:
  ours    pytorch_object_detection_amd.optim.SGD / Adam: one fd_optim_begin launch and one update launch per 64 tensors
  torch   torch.optim.SGD(fused=True) / Adam(fused=True)
step_ms          median device-event time of --inner back-to-back step() calls, per call (the queue never drains inside the window)
host_enqueue_ms  median host clock around one step() call that is NOT followed by a synchronise: what Python and the launches cost the host
graph_replay_ms  the same step() captured once with torch.cuda.graph and replayed, --inner replays per event pair: the device time of the step's kernels without
                 the host (torch's Adam is built with capturable=True for this figure alone: its fused step refuses a capture otherwise)
bytes            what the rule must move: 20 B per element for SGD with momentum (p and buffer read and written, g read), 28 B for Adam
GBps / hbm_frac  bytes over step_ms, and that rate over the 8000 GB/s HBM figure bench.py uses
launches         kernel launches of one step() of ours (begin included); torch's fused step is not counted here, its launches are internal
No figure here is a pass / fail bar.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import optim  # noqa: E402
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure


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


def graphed(opt):
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
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
        raise SystemExit("time_optim.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    cfg = load_config()
    cfg["model"]["name"] = "HISFCOS"
    cfg["dataset_setting"]["class_num"] = 20
    model = Builder(cfg).model_build().to(dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)

    def twin():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
        return ps

    out = {"tool": "time_optim", "device": torch.cuda.get_device_name(0), "model": "HISFCOS-R50, 20 classes", "tensors": len(shapes), "elements": numel,
           "largest_tensor": max(int(torch.Size(s).numel()) for s in shapes), "peak_hbm_GBps": PEAK_HBM_GBS, "reps": a.reps, "inner": a.inner}
    rules = {"sgd": (20, lambda ps: optim.SGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4),
                     lambda ps, **kw: torch.optim.SGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4, fused=True)),
             "adam": (28, lambda ps: optim.Adam(ps, lr=1e-4, weight_decay=1e-4),
                      lambda ps, **kw: torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4, fused=True, **kw))}
    for name, (bpe, ours, stock) in rules.items():
        o_ours, o_stock, o_stock_graph = ours(twin()), stock(twin()), stock(twin(), capturable=True)
        for _ in range(5):
            o_ours.step()
            o_stock.step()
            o_stock_graph.step()
        graphs = {"ours": graphed(o_ours), "torch": graphed(o_stock_graph)}
        dev_t, host_t, graph_t = {"ours": [], "torch": []}, {"ours": [], "torch": []}, {"ours": [], "torch": []}
        for _ in range(a.reps):                              # alternating, so a drift of the machine reaches both alike
            for who, o in (("ours", o_ours), ("torch", o_stock)):
                dev_t[who].append(device_ms(o.step, a.inner))
                host_t[who].append(host_ms(o.step))
                graph_t[who].append(device_ms(graphs[who].replay, a.inner))
        nbytes = bpe * numel
        res = {"bytes": nbytes, "launches": o_ours.launches}
        for who in ("ours", "torch"):
            ms = median(dev_t[who])
            gbps = nbytes / (ms * 1e-3) / 1e9
            res[who] = {"step_ms": round(ms, 4), "step_ms_min": round(min(dev_t[who]), 4), "GBps": round(gbps, 1), "hbm_frac": round(gbps / PEAK_HBM_GBS, 4),
                        "host_enqueue_ms": round(median(host_t[who]), 4), "graph_replay_ms": round(median(graph_t[who]), 4),
                        "graph_replay_GBps": round(nbytes / (median(graph_t[who]) * 1e-3) / 1e9, 1),
                        "graph_replay_hbm_frac": round(nbytes / (median(graph_t[who]) * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
        out[name] = res
    out["note"] = ("step_ms of back-to-back calls is bound by the slower of device work and host enqueue; where host_enqueue_ms exceeds the device time of the "
                   "bytes, step_ms measures the host (a replayed graph does not pay it)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
