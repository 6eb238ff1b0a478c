"""Device time of ATSS target assignment (fd_atss_gen_targets) beside fd_fcos_gen_targets at a training shape;
prints one JSON line.

    python tools/time_atss.py [--reps 20] [--batch 16] [--size 640] [--boxes 8 64] [--classes 80]

Per --boxes value M: --batch images of --size x --size (five levels of strides 8 .. 128: L = 8 525 at 640) with M ground-truth
rows each, all valid.  The two assigners are timed alternately, rep by rep, on the same boxes: atss_ms is the whole call (the
workspace memset, the selection launch with one workgroup per (image, row), the output launch), fcos_ms the one launch of
fd_fcos_gen_targets.  median and minimum of device-event times, `inner` back-to-back calls per event pair: these include what
the host needs to enqueue a call (the wrapper allocates its outputs).  *_graph_ms is the same `inner` calls captured once in a
torch.cuda.graph and replayed -- the device side alone, as the call runs inside a captured training step.
launches           what one call enqueues (the wrapper's output allocations are not launches)
workspace_bytes    fd_atss_workspace_bytes(B, L): one 64-bit claim word per (image, location)
positives          locations with cls > 0 under each rule, for scale
No figure here is a pass / fail bar.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_object_detection_amd import _lib, ops  # noqa: E402

STRIDES = [8, 16, 32, 64, 128]
RANGES = [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 999999]]


def alternate_ms(fns, reps, inner):
    """Median and minimum device-event time in ms of each fn, the fns taking turns inside every rep."""
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns:
        for _ in range(3):
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            st.record()
            for _ in range(inner):
                fn()
            en.record()
            torch.cuda.synchronize()
            ms[k].append(st.elapsed_time(en) / inner)
    for m in ms:
        m.sort()
    return [(m[len(m) // 2], m[0]) for m in ms]


def captured(fn, inner):
    """`inner` calls of fn recorded in one graph -> a callable that replays it."""
    fn()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep = [fn() for _ in range(inner)]
    torch.cuda.current_stream().wait_stream(side)
    graph.keep = keep
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--boxes", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--topk", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_atss.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    level_hw = [(-(-S // s), -(-S // s)) for s in STRIDES]
    L = sum(h * w for h, w in level_hw)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "L": L, "topk": a.topk,
           "workspace_bytes": int(_lib.lib().fd_atss_workspace_bytes(B, L)),
           "launches": {"atss": {"memsets": 1, "kernels": 2}, "fcos": {"memsets": 0, "kernels": 1}}, "cases": []}
    for M in a.boxes:
        gen = torch.Generator().manual_seed(S + M)
        xy = torch.rand(B, M, 2, generator=gen) * 0.6 * S
        wh = (torch.rand(B, M, 2, generator=gen) * 0.35 + 0.05) * S
        gt = torch.cat([xy, xy + wh], 2).contiguous().to(dev)
        labels = torch.randint(1, a.classes + 1, (B, M), generator=gen).to(dev)
        n0 = ops.LAUNCHES[0]
        cls_a = ops.atss_gen_targets(gt, labels, level_hw, STRIDES, a.topk)[0]
        calls_atss = ops.LAUNCHES[0] - n0
        cls_f = ops.fcos_gen_targets(gt, labels, level_hw, STRIDES, RANGES)[0]
        fa = lambda: ops.atss_gen_targets(gt, labels, level_hw, STRIDES, a.topk)  # noqa: E731
        ff = lambda: ops.fcos_gen_targets(gt, labels, level_hw, STRIDES, RANGES)  # noqa: E731
        (am, amin), (fm, fmin) = alternate_ms([fa, ff], a.reps, a.inner)
        (gam, gamin), (gfm, gfmin) = alternate_ms([captured(fa, a.inner), captured(ff, a.inner)], a.reps, 1)
        out["cases"].append({"M": M, "atss_ms": round(am, 4), "atss_min_ms": round(amin, 4), "fcos_ms": round(fm, 4), "fcos_min_ms": round(fmin, 4),
                             "atss_graph_ms": round(gam / a.inner, 4), "atss_graph_min_ms": round(gamin / a.inner, 4),
                             "fcos_graph_ms": round(gfm / a.inner, 4), "fcos_graph_min_ms": round(gfmin / a.inner, 4),
                             "abi_calls_per_atss_call": calls_atss, "selection_workgroups": B * M,
                             "positives": {"atss": int((cls_a > 0).sum()), "fcos": int((cls_f > 0).sum())}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
