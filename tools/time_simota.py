"""Device time of SimOTA target assignment (fd_simota_gen_targets) beside fd_atss_gen_targets at a training shape;
prints one JSON line.

    python tools/time_simota.py [--reps 20] [--batch 16] [--size 640] [--boxes 8 64] [--classes 80] [--top-q 10]

Per --boxes value M: --batch images of --size x --size (five levels of strides 8 .. 128: L = 8 525 at 640) with M ground-truth
rows each, all valid, and predictions as a head under training emits them: cls logits ~ N(-2, 1.5), cnt logits ~ N(0, 1), and at
every location inside a box that box's distances under log-normal noise (random distances elsewhere).  The two assigners are
timed alternately, rep by rep, on the same boxes: simota_ms is the whole call (the pair-matrix launch, the selection launch with
one workgroup per (image, row), the output launch), atss_ms the whole call of fd_atss_gen_targets.  median and minimum of
device-event times, `inner` back-to-back calls per event pair: these include what the host needs to enqueue a call
(the wrapper allocates its outputs and the workspace).  *_graph_ms is the same `inner` calls captured once in a torch.cuda.graph
and replayed -- the device side alone, as the call runs inside a captured training step.
launches           what one call enqueues (the wrapper's allocations are not launches)
workspace_bytes    fd_simota_workspace_bytes(B, M, L): one 64-bit claim word per (image, location) and two 32-bit words per pair
positives          locations with cls > 0 under each rule, for scale; k_mean the mean dynamic k of the rows
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


def predictions(gt, level_hw, classes, gen):
    """cls [B,L,C], cnt [B,L], reg [B,L,4] on the CPU: every location predicts, under log-normal noise, the first box that holds it."""
    B, M, _ = gt.shape
    cx, cy, st = [], [], []
    for (h, w), s in zip(level_hw, STRIDES):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        cx.append((xs.reshape(-1) * s + s // 2).float())
        cy.append((ys.reshape(-1) * s + s // 2).float())
        st.append(torch.full((h * w,), float(s)))
    cx, cy, st = torch.cat(cx), torch.cat(cy), torch.cat(st)
    L = cx.numel()
    off = torch.stack([cx[None, None] - gt[..., 0:1], cy[None, None] - gt[..., 1:2], gt[..., 2:3] - cx[None, None], gt[..., 3:4] - cy[None, None]], 3)
    inside = off.min(3).values > 0                                                           # [B, M, L]
    first = inside.float().argmax(1)                                                         # [B, L]
    held = inside.any(1)
    target = off.gather(1, first[:, None, :, None].expand(B, 1, L, 4))[:, 0]
    rand = st[None, :, None] * (0.5 + 3.5 * torch.rand(B, L, 4, generator=gen))
    reg = torch.where(held[..., None], target * torch.exp(0.25 * torch.randn(B, L, 4, generator=gen)), rand)
    return torch.randn(B, L, classes, generator=gen) * 1.5 - 2.0, torch.randn(B, L, generator=gen), reg.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--boxes", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--top-q", type=int, default=10)
    ap.add_argument("--atss-topk", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_simota.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    level_hw = [(-(-S // s), -(-S // s)) for s in STRIDES]
    L = sum(h * w for h, w in level_hw)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "L": L, "classes": a.classes, "top_q": a.top_q,
           "launches": {"simota": {"memsets": 0, "kernels": 3}, "atss": {"memsets": 1, "kernels": 2}}, "cases": []}
    for M in a.boxes:
        gen = torch.Generator().manual_seed(S + M)
        xy = torch.rand(B, M, 2, generator=gen) * 0.6 * S
        wh = (torch.rand(B, M, 2, generator=gen) * 0.35 + 0.05) * S
        gt_cpu = torch.cat([xy, xy + wh], 2).contiguous()
        labels = torch.randint(1, a.classes + 1, (B, M), generator=gen).to(dev)
        cl, cn, rp = (t.to(dev) for t in predictions(gt_cpu, level_hw, a.classes, gen))
        gt = gt_cpu.to(dev)
        n0 = ops.LAUNCHES[0]
        cls_s, _, _, _, _, k, _ = ops.simota_gen_targets(cl, cn, rp, gt, labels, level_hw, STRIDES, a.top_q, return_stats=True)
        calls = ops.LAUNCHES[0] - n0
        cls_a = ops.atss_gen_targets(gt, labels, level_hw, STRIDES, a.atss_topk)[0]
        fs = lambda: ops.simota_gen_targets(cl, cn, rp, gt, labels, level_hw, STRIDES, a.top_q)  # noqa: E731
        fa = lambda: ops.atss_gen_targets(gt, labels, level_hw, STRIDES, a.atss_topk)  # noqa: E731
        (sm, smin), (am, amin) = alternate_ms([fs, fa], a.reps, a.inner)
        (gsm, gsmin), (gam, gamin) = alternate_ms([captured(fs, a.inner), captured(fa, a.inner)], a.reps, 1)
        out["cases"].append({"M": M, "simota_ms": round(sm, 4), "simota_min_ms": round(smin, 4), "atss_ms": round(am, 4), "atss_min_ms": round(amin, 4),
                             "simota_graph_ms": round(gsm / a.inner, 4), "simota_graph_min_ms": round(gsmin / a.inner, 4),
                             "atss_graph_ms": round(gam / a.inner, 4), "atss_graph_min_ms": round(gamin / a.inner, 4),
                             "abi_calls_per_simota_call": calls, "selection_workgroups": B * M,
                             "workspace_bytes": int(_lib.lib().fd_simota_workspace_bytes(B, M, L)), "k_mean": round(float(k.float().mean()), 2),
                             "positives": {"simota": int((cls_s > 0).sum()), "atss": int((cls_a > 0).sum())}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
