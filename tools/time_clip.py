"""Device and host time of gradient-norm clipping inside the HIP optimizer step at HISFCOS-R50's real trainable list; prints one JSON line.

    python tools/time_clip.py [--reps 30] [--inner 10]

The parameters are those of Builder(cfg).model_build() with 20 classes, gradients are N(0, 1) tensors of the same shapes, allocated once.  Three sequences over
optim.SGD (momentum 0.9, weight decay 1e-4), in ONE run and alternating, each with a GradScaler-style grad_scale / found_inf pair on the device:
  plain   step() of an optimizer built without max_grad_norm (no clipping at all: what the new launches are added to)
  ours    step() with max_grad_norm: one sum-of-squares launch per 64 gradients, the finish launch, then the same begin and update launches
  stock   what a user runs today for the same result: the unscale of scaler.unscale_ (torch._amp_foreach_non_finite_check_and_unscale_, the launch it makes),
          torch.nn.utils.clip_grad_norm_(foreach=True), then the same HIP step()
The scale is 1 and max_norm is far above the norm, so that the stock sequence, which rewrites the gradients in place, leaves their values as they are from one
repetition to the next; every launch of all three sequences still runs and moves the same bytes as with an active clip.
step_ms          median device-event time of --inner back-to-back calls, per call
host_enqueue_ms  median host clock around one call that is NOT followed by a synchronise
graph_replay_ms  the sequence captured once with torch.cuda.graph and replayed, --inner replays per event pair: the device time of its kernels without the host
norm             the sum-of-squares and finish launches alone (ops.grad_sumsq + ops.grad_clip_finish), replayed from a graph: 4 B per element, and that rate over
                 the 8000 GB/s HBM figure bench.py uses
added_ms         ours minus plain, eager and replayed
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

from pytorch_object_detection_amd import ops, optim  # noqa: E402
from pytorch_object_detection_amd.bulider import Builder, load_config  # noqa: E402

PEAK_HBM_GBS = 8000.0       # bench.py's figure
MAX_NORM = 1e9


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
        raise SystemExit("time_clip.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    cfg = load_config()
    cfg["model"]["name"] = "HISFCOS"
    cfg["dataset_setting"]["class_num"] = 20
    model = Builder(cfg).model_build().to(dev)
    shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
    del model
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)

    def twin(**kw):
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
        opt = optim.SGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4, **kw)
        opt.grad_scale, opt.found_inf = torch.ones((), device=dev), torch.zeros((), device=dev)
        return ps, opt

    (_, o_plain), (_, o_ours), (p_stock, o_stock) = twin(), twin(max_grad_norm=MAX_NORM), twin()
    g_stock = [p.grad for p in p_stock]
    inv_scale, scale, found = torch.ones((), device=dev), o_stock.grad_scale, o_stock.found_inf
    o_stock.grad_scale = None                                # the gradients reach the step unscaled, as after scaler.unscale_

    def stock():
        torch._amp_foreach_non_finite_check_and_unscale_(g_stock, found, inv_scale)
        torch.nn.utils.clip_grad_norm_(p_stock, MAX_NORM, foreach=True)
        o_stock.step()

    g_ours = sorted((p.grad for g in o_ours.param_groups for p in g["params"]), key=lambda g: -g.numel())     # largest first, as step() orders them
    ptrs, numels = [g.data_ptr() for g in g_ours], [g.numel() for g in g_ours]

    def norm_only():
        _, slots = ops.grad_sumsq(ptrs, numels, o_ours._fd_partials)
        ops.grad_clip_finish(o_ours._fd_partials, slots, scale, None, MAX_NORM, o_ours._fd_clip)

    seqs = {"plain": o_plain.step, "ours": o_ours.step, "stock": stock}
    for _ in range(5):
        for fn in seqs.values():
            fn()
        norm_only()
    graphs = {k: graphed(fn) for k, fn in seqs.items()}
    norm_graph = graphed(norm_only)
    dev_t, host_t, graph_t, norm_t = {k: [] for k in seqs}, {k: [] for k in seqs}, {k: [] for k in seqs}, []
    for _ in range(a.reps):                                  # alternating, so a drift of the machine reaches all alike
        for k, fn in seqs.items():
            dev_t[k].append(device_ms(fn, a.inner))
            host_t[k].append(host_ms(fn))
            graph_t[k].append(device_ms(graphs[k].replay, a.inner))
        norm_t.append(device_ms(norm_graph.replay, a.inner))
    out = {"tool": "time_clip", "device": torch.cuda.get_device_name(0), "model": "HISFCOS-R50, 20 classes", "tensors": len(shapes), "elements": numel,
           "peak_hbm_GBps": PEAK_HBM_GBS, "reps": a.reps, "inner": a.inner,
           "launches": {"plain": o_plain.launches, "ours": o_ours.launches, "norm": o_ours.launches - o_plain.launches}}
    for k in seqs:
        out[k] = {"step_ms": round(median(dev_t[k]), 4), "step_ms_min": round(min(dev_t[k]), 4), "host_enqueue_ms": round(median(host_t[k]), 4),
                  "graph_replay_ms": round(median(graph_t[k]), 4), "graph_replay_ms_min": round(min(graph_t[k]), 4)}
    ms = median(norm_t)
    gbps = 4 * numel / (ms * 1e-3) / 1e9
    out["norm"] = {"bytes": 4 * numel, "graph_replay_ms": round(ms, 4), "graph_replay_ms_min": round(min(norm_t), 4), "GBps": round(gbps, 1),
                   "hbm_frac": round(gbps / PEAK_HBM_GBS, 4)}
    out["added_ms"] = {"step": round(out["ours"]["step_ms"] - out["plain"]["step_ms"], 4),
                       "graph_replay": round(out["ours"]["graph_replay_ms"] - out["plain"]["graph_replay_ms"], 4)}
    out["ours_over_stock"] = {"step": round(out["ours"]["step_ms"] / out["stock"]["step_ms"], 4),
                              "graph_replay": round(out["ours"]["graph_replay_ms"] / out["stock"]["graph_replay_ms"], 4)}
    out["note"] = ("step_ms of back-to-back calls is bound by the slower of device work and host enqueue; where host_enqueue_ms exceeds the device time of the "
                   "bytes, step_ms measures the host (a replayed graph does not pay it)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
