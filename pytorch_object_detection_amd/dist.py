"""Image-sharded multi-GPU inference: one process per GPU (torch.distributed, backend 'nccl' = RCCL over xGMI),
batch split in contiguous slices, weights replicated, and ONE collective — an all-gather of the fixed-size padded
detections.  The network itself exchanges nothing (frozen BN, per-sample GN / SE).

Sharded evaluation adds a ragged row gather, `gather_rows` (two collectives: the ranks' sizes, then one
uint8 payload), and `merge_order`, the row order of the union of what the ranks evaluated."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from ._lib import FdError


def shard_batch(global_batch: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous slice [lo, hi) of the global batch owned by `rank` (sizes differ by at most one)."""
    base, rem = divmod(global_batch, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def pack_detections(scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """[B,K] f32, [B,K] i64, [B,K,4] f32, [B] i32 -> ONE message [B, K+1, 6] f32: row 0 of an image carries its count, rows
    1..K are (x1, y1, x2, y2, score, class); class ids and counts are < 2^24, exact in fp32.  One HIP launch on CUDA
    tensors (fd_pack_detections); CPU tensors (the gloo rehearsal of the protocol in tests/test_dist_cpu.py) take the
    equivalent torch ops."""
    if scores.is_cuda:
        from . import ops
        return ops.pack_detections(scores, classes, boxes, counts)
    B, K = scores.shape
    rec = torch.zeros(B, K + 1, 6, dtype=torch.float32)
    rec[:, 0, 0] = counts.to(torch.float32)
    rec[:, 1:, :4], rec[:, 1:, 4], rec[:, 1:, 5] = boxes, scores, classes.to(torch.float32)
    return rec


def unpack_detections(rec: torch.Tensor):
    """Inverse of pack_detections: -> (scores [B,K], classes [B,K] int64, boxes [B,K,4], counts [B] int32)."""
    if rec.is_cuda:
        from . import ops
        return ops.unpack_detections(rec)
    return (rec[:, 1:, 4].contiguous(), rec[:, 1:, 5].to(torch.int64), rec[:, 1:, :4].contiguous(), rec[:, 0, 0].to(torch.int32))


def gather_detections(scores, classes, boxes, counts, group=None, force: bool = False, pad_to: int = 0):
    """All-gather padded detections from every rank: returns (scores [W*B,K], classes, boxes [W*B,K,4], counts [W*B]).
    ONE collective: a single all_gather_into_tensor of the [B, K+1, 6] fp32 records (385 KB at B=16, K=1000; latency-bound on xGMI),
    one pack launch before it and one unpack launch after it.  Every rank must contribute the same number of records: with equal
    shards (the bench: 16 images per GPU) that is the local batch; for a global batch that does not divide (shard_batch hands the
    first ranks one image more) pass pad_to = the LARGEST local batch -- shorter shards are padded with empty records (count 0) and
    the caller drops them with `unpad_gathered` (the shard sizes are known analytically: no second collective)."""
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
        return scores, classes, boxes, counts
    world = dist.get_world_size(group)
    rec = pack_detections(scores, classes, boxes, counts)
    if pad_to and pad_to > rec.shape[0]:
        rec = torch.cat([rec, torch.zeros((pad_to - rec.shape[0],) + tuple(rec.shape[1:]), dtype=rec.dtype, device=rec.device)], 0)
    out = torch.empty((world * rec.shape[0],) + tuple(rec.shape[1:]), dtype=rec.dtype, device=rec.device)
    dist.all_gather_into_tensor(out, rec, group=group)
    return unpack_detections(out)


def unpad_gathered(gathered, global_batch: int, world: int):
    """Drop the padding records gather_detections(pad_to=...) added: rank r contributed shard_batch(global_batch, r, world) images."""
    sizes = [hi - lo for lo, hi in (shard_batch(global_batch, r, world) for r in range(world))]
    pad = max(sizes)
    idx = torch.cat([torch.arange(r * pad, r * pad + n) for r, n in enumerate(sizes)]).to(gathered[0].device)
    return tuple(t.index_select(0, idx) for t in gathered)


# ---------------------------------------------------------------------------------------------- sharded evaluation
def _no_group(group, force: bool) -> bool:
    return not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force)


def _pad_block(t: torch.Tensor, n: int, rows: int, width: int, fill) -> torch.Tensor:
    """The first n rows of t in a [rows, width, ...] block (a [rows] block for a 1-D tensor), the rest holding `fill`."""
    if t.dim() == 1:
        out = torch.full((rows,), fill, dtype=t.dtype, device=t.device)
        out[:n] = t[:n]
        return out
    out = torch.full((rows, width) + tuple(t.shape[2:]), fill, dtype=t.dtype, device=t.device)
    out[:n, :t.shape[1]] = t[:n]
    return out


def _gather_rows(tensors: Sequence[torch.Tensor], n: int, group, fills: Optional[Sequence], header: Sequence[int]):
    """gather_rows' protocol, which also hands back every rank's header: -> (tensors, rows_per_rank, headers [W, len(header)])."""
    world = dist.get_world_size(group)
    tensors = list(tensors)
    fills = [0] * len(tensors) if fills is None else list(fills)
    n = int(n)
    if not tensors or len(fills) != len(tensors):
        raise FdError("gather_rows: needs at least one tensor and one fill value per tensor")
    dev = tensors[0].device
    for t in tensors:
        if t.dtype not in (torch.float32, torch.int32, torch.int64) or t.dim() < 1 or t.shape[0] < n or t.device != dev:
            raise FdError("gather_rows: f32 / i32 / i64 tensors on one device with at least n rows each")
    # collective 1: n, the dimension-1 widths, the header -- a fixed-size message
    msg = torch.tensor([n] + [t.shape[1] if t.dim() > 1 else 0 for t in tensors] + [int(h) for h in header], dtype=torch.int64, device=dev)
    sizes = torch.empty(world * msg.numel(), dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(sizes, msg, group=group)
    sizes = sizes.cpu().view(world, msg.numel())
    rows = [int(v) for v in sizes[:, 0]]
    headers = sizes[:, 1 + len(tensors):]
    for k in range(headers.shape[1]):           # every rank sees the same table: all of them raise, none waits in collective 2
        vals = sorted({int(v) for v in headers[:, k] if int(v) >= 0})
        if len(vals) > 1:
            raise FdError(f"gather_rows: the ranks disagree on header value {k}: {[int(v) for v in headers[:, k]]}")
    widths = [int(v) for v in sizes[:, 1:1 + len(tensors)].max(dim=0).values]
    pad = max(rows)
    if pad == 0:                                # no rank has a row, and every rank knows: nothing to send
        return [_pad_block(t, 0, 0, w, f) for t, w, f in zip(tensors, widths, fills)], rows, headers
    # collective 2: every tensor padded to [pad, width, ...], as bytes, each block on an 8-byte boundary
    blocks = [_pad_block(t, n, pad, w, f) for t, w, f in zip(tensors, widths, fills)]
    nbytes = [(b.numel() * b.element_size() + 7) // 8 * 8 for b in blocks]
    send = torch.zeros(sum(nbytes), dtype=torch.uint8, device=dev)
    off = 0
    for b, nb in zip(blocks, nbytes):
        send[off:off + b.numel() * b.element_size()] = b.view(-1).view(torch.uint8)
        off += nb
    recv = torch.empty(world * send.numel(), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    recv = recv.view(world, send.numel())
    out, off = [], 0
    for b, nb in zip(blocks, nbytes):
        live = b.numel() * b.element_size()
        parts = [recv[r, off:off + live].view(b.dtype).view(b.shape)[:rows[r]] for r in range(world)]
        out.append(torch.cat(parts, 0))
        off += nb
    return out, rows, headers


def gather_rows(tensors: Sequence[torch.Tensor], n: int, group=None, force: bool = False, fills: Optional[Sequence] = None,
                header: Sequence[int] = ()) -> Tuple[List[torch.Tensor], List[int]]:
    """Ragged all-gather of rows: every rank contributes the first `n` rows of each of `tensors` (f32 / i32 / i64, one device,
    the same trailing shapes on every rank except dimension 1 -- a K or G width -- which may differ from rank to rank).
    -> ([rank 0's rows, then rank 1's, ...] per tensor, rows_per_rank); dimension 1 is the widest rank's, the columns a
    narrower rank did not have hold that tensor's `fills` value (default 0).

    TWO collectives: an all_gather_into_tensor of the sizes (n, the widths and `header`), then one of a uint8 payload in which
    every rank has padded its columns to the widest and its rows to the largest n (the padding rows are dropped on arrival).
    When no rank has a row the sizes say so on every rank and the payload is skipped.  `header`: ints that must be equal on
    every rank (a negative value agrees with anything); a disagreement raises FdError on every rank before the payload, so no
    rank is left waiting.  CUDA tensors travel as they are (RCCL); CPU tensors take the same protocol over gloo.
    No initialised process group, or world size 1 without `force`: the inputs' first n rows (views) and no collective."""
    if _no_group(group, force):
        return [t[:int(n)] for t in tensors], [int(n)]
    out, rows, _ = _gather_rows(tensors, n, group, fills, header)
    return out, rows


def merge_order(ids_per_rank) -> torch.Tensor:
    """Row order of a merged evaluation.  `ids_per_rank`: the image id of every gathered row, rank 0's rows first, as one flat
    sequence or as one sequence per rank.  -> int64 index that visits each distinct id once, ids ascending; of equal ids it
    keeps the first row, i.e. the lowest rank's earliest arrival.  Host arithmetic only."""
    flat: List[int] = []
    for x in (ids_per_rank.tolist() if torch.is_tensor(ids_per_rank) else ids_per_rank):
        if isinstance(x, (list, tuple)) or torch.is_tensor(x) or hasattr(x, "tolist"):
            flat.extend(int(i) for i in (x.tolist() if hasattr(x, "tolist") else x))
        else:
            flat.append(int(x))
    ids = torch.tensor(flat, dtype=torch.int64)
    if ids.numel() == 0:
        return ids
    srt, order = torch.sort(ids, stable=True)
    keep = torch.ones(ids.numel(), dtype=torch.bool)
    keep[1:] = srt[1:] != srt[:-1]
    return order[keep]
