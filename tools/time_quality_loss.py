"""Device time of the IoU-aware classification losses (fd_ltrb_quality, fd_quality_loss_fwd / _bwd) beside the
hard-label focal loss (fd_focal_loss_fwd / _bwd) at a training shape; prints one JSON line.

    python tools/time_quality_loss.py [--reps 20] [--inner 10] [--batch 16] [--size 640] [--classes 80]

--batch images of --size x --size (five levels of strides 8 .. 128: L = 8 525 at 640), --classes classes; logits ~ N(-2, 1.5) as a
head under training emits them, 3 % of the locations positive with a box prediction under log-normal noise.  Seven launches are
timed alternately, rep by rep, on the same tensors: the quality launch, the forward (two kernels: the sum and its final pass) and
the backward of QFL and of VFL, and the focal forward and backward.  median and minimum of device-event times, `inner`
back-to-back calls per event pair: *_ms includes what the host needs to enqueue a call (the wrapper allocates its outputs and the
workspace); *_graph_ms is the same `inner` calls captured once in a torch.cuda.graph and replayed -- the device side alone, as the
call runs inside a captured training step.
bytes       what a launch must move: the logits once in a forward, once read and once written in a backward, plus labels and q
            (the focal launches: labels only); quality: two boxes and a label read, one float written per location
hbm_frac    bytes / graph time over --hbm-gbs (8 000 GB/s, the MI355X's specified peak): a bound on what the time could be,
            not a measurement of traffic -- at this size the tensors fit the 256 MiB last-level cache
No figure here is a pass / fail bar.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from time_atss import STRIDES, alternate_ms, captured  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_quality_loss.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    B, S, C = a.batch, a.size, a.classes
    L = sum((-(-S // s)) ** 2 for s in STRIDES)
    gen = torch.Generator().manual_seed(S + C)
    logits = (torch.randn(B, L, C, generator=gen) * 1.5 - 2.0).to(dev)
    labels = torch.where(torch.rand(B, L, generator=gen) < 0.03, torch.randint(1, C + 1, (B, L), generator=gen), torch.zeros(B, L, dtype=torch.int64)).to(dev)
    tgt = torch.rand(B, L, 4, generator=gen) * 56 + 4
    pred = (tgt * torch.exp(0.25 * torch.randn(B, L, 4, generator=gen))).to(dev)
    tgt = tgt.to(dev)
    gscale = torch.full((B,), 1.0 / 256, device=dev)
    q = ops.ltrb_quality(pred, tgt, labels)
    fns = {"quality": lambda: ops.ltrb_quality(pred, tgt, labels),
           "qfl_fwd": lambda: ops.quality_loss_fwd(logits, labels, q, "qfl"),
           "qfl_bwd": lambda: ops.quality_loss_bwd(logits, labels, q, gscale, "qfl"),
           "vfl_fwd": lambda: ops.quality_loss_fwd(logits, labels, q, "vfl"),
           "vfl_bwd": lambda: ops.quality_loss_bwd(logits, labels, q, gscale, "vfl"),
           "focal_fwd": lambda: ops.focal_loss_fwd(logits, labels),
           "focal_bwd": lambda: ops.focal_loss_bwd(logits, labels, gscale)}
    x_bytes, loc = B * L * C * 4, B * L
    nbytes = {"quality": loc * (32 + 8 + 4), "qfl_fwd": x_bytes + loc * 12, "qfl_bwd": 2 * x_bytes + loc * 12, "vfl_fwd": x_bytes + loc * 12,
              "vfl_bwd": 2 * x_bytes + loc * 12, "focal_fwd": x_bytes + loc * 8, "focal_bwd": 2 * x_bytes + loc * 8}
    names = list(fns)
    eager = alternate_ms([fns[n] for n in names], a.reps, a.inner)
    graph = alternate_ms([captured(fns[n], a.inner) for n in names], a.reps, 1)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "L": L, "classes": C, "positives": int((labels > 0).sum()),
           "q_mean_on_positives": round(float(q[labels > 0].mean()), 4), "hbm_gbs": a.hbm_gbs,
           "workspace_bytes": int(_lib.lib().fd_quality_loss_workspace_bytes(B)),
           "launches": {"quality": 1, "quality_loss_fwd": 2, "quality_loss_bwd": 1, "focal_fwd": 2, "focal_bwd": 1}, "cases": {}}
    for n, (em, emin), (gm, gmin) in zip(names, eager, graph):
        g = gm / a.inner
        out["cases"][n] = {"ms": round(em, 4), "min_ms": round(emin, 4), "graph_ms": round(g, 4), "graph_min_ms": round(gmin / a.inner, 4),
                           "bytes": nbytes[n], "hbm_frac": round(nbytes[n] / (g * 1e-3) / (a.hbm_gbs * 1e9), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
