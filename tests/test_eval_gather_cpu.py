"""Sharded evaluation, host side: merge_order on hand-written id lists, and gather_rows over gloo on CPU tensors (the protocol
the device path takes: one collective for the sizes, one for a uint8 payload)."""
import os
import socket
import tempfile
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pytorch_object_detection_amd._lib import FdError
from pytorch_object_detection_amd.dist import gather_rows, merge_order

ROWS = (4, 0, 3)            # rows per rank (rank 1 has none)
WIDTHS = (5, 1, 7)          # dimension-1 width per rank
FILLS = (0.5, -1, 7, 0)     # per tensor: f32 [n, K], i64 [n, K], i32 [n, K, 4], i64 [n]


# ---------------------------------------------------------------------------------------------------------------- merge_order
def test_merge_order_duplicates_within_and_across_ranks():
    # rows:          0  1  2   3  4   5  6
    per_rank = [[7, 3, 7], [3, 9], [1, 7]]
    idx = merge_order(per_rank)
    assert idx.dtype == torch.int64 and idx.tolist() == [5, 1, 0, 4]         # ids 1, 3, 7, 9: the first row that holds each
    assert merge_order([7, 3, 7, 3, 9, 1, 7]).tolist() == [5, 1, 0, 4]       # the concatenated list says the same
    assert merge_order(torch.tensor([7, 3, 7, 3, 9, 1, 7])).tolist() == [5, 1, 0, 4]


def test_merge_order_empty_rank_and_empty_input():
    assert merge_order([[4, 2], [], [2, 0]]).tolist() == [3, 1, 0]
    assert merge_order([]).tolist() == [] and merge_order([[], []]).tolist() == []


def test_merge_order_sorted_and_reversed_input():
    assert merge_order([[0, 1, 2], [3, 4]]).tolist() == [0, 1, 2, 3, 4]
    assert merge_order([[9, 7, 5], [3, 1]]).tolist() == [4, 3, 2, 1, 0]
    assert merge_order([[-2, 5], [5, -2]]).tolist() == [0, 1]                # equal ids: the lower rank's row


# ---------------------------------------------------------------------------------------------------------------- gather_rows
def _rank_tensors(r):
    """Rank r's buffers: more rows than it contributes (a growable buffer's spare capacity), values that name (rank, position)."""
    g = torch.Generator().manual_seed(50 + r)
    cap, K = ROWS[r] + 2, WIDTHS[r]
    return [torch.rand(cap, K, generator=g) + r, torch.randint(0, 1 << 40, (cap, K), generator=g),
            torch.randint(-100, 100, (cap, K, 4), generator=g).to(torch.int32), torch.arange(cap, dtype=torch.int64) + 1000 * r]


def _expected(world):
    K = max(WIDTHS[:world])
    out = [[], [], [], []]
    for r in range(world):
        n, k = ROWS[r], WIDTHS[r]
        for j, (t, fill) in enumerate(zip(_rank_tensors(r), FILLS)):
            if t.dim() == 1:
                out[j].append(t[:n])
                continue
            e = torch.full((n, K) + tuple(t.shape[2:]), fill, dtype=t.dtype)
            e[:, :k] = t[:n]
            out[j].append(e)
    return [torch.cat(x) for x in out]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        calls = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, inp, group=None: (calls.append((inp.dtype, tuple(inp.shape))), real(out, inp, group=group))[1]
        try:
            got, rows = gather_rows(_rank_tensors(rank), ROWS[rank], fills=FILLS)
        finally:
            dist.all_gather_into_tensor = real
        assert [c[0] for c in calls] == [torch.int64, torch.uint8], calls        # the sizes, then ONE payload
        # a header every rank agrees on passes (a negative value agrees with anything); one they do not raises on EVERY rank
        gather_rows(_rank_tensors(rank), ROWS[rank], header=(21, -1 if rank else 3))
        with pytest.raises(FdError, match="disagree"):
            gather_rows(_rank_tensors(rank), ROWS[rank], header=(21, rank))
        # no rank has a row: the sizes say so and nothing else is sent
        empty, none = gather_rows(_rank_tensors(rank), 0)
        assert none == [0] * world and [tuple(t.shape) for t in empty] == [(0, max(WIDTHS[:world])), (0, max(WIDTHS[:world])),
                                                                          (0, max(WIDTHS[:world]), 4), (0,)]
        torch.save({"tensors": got, "rows": rows}, os.path.join(out_dir, f"rank{rank}.pt"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_rows_gloo(world):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, port, tmp), nprocs=world, join=True)
        res = [torch.load(os.path.join(tmp, f"rank{r}.pt")) for r in range(world)]
    want = _expected(world)
    for r in range(world):
        assert res[r]["rows"] == list(ROWS[:world])
        for got, exp in zip(res[r]["tensors"], want):       # every rank: the real rows in rank order, the fill in the padding columns
            assert got.dtype == exp.dtype and got.shape == exp.shape and torch.equal(got, exp)
    if world == 3:      # rank 2 is the widest: ranks 0 and 1 were padded, each tensor with its own fill
        s, c, b, _ = res[0]["tensors"]
        assert (s[:4, 5:] == 0.5).all() and (c[:4, 5:] == -1).all() and (b[:4, 5:] == 7).all() and s.shape == (7, 7)


def test_gather_rows_is_two_collectives(monkeypatch):
    """Count the collectives as test_dist_cpu.py does for gather_detections: a faked world of 2 whose other rank is a copy."""
    calls = []
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "all_gather_into_tensor",
                        lambda out, inp, group=None: (calls.append((inp.dtype, inp.numel())), out.copy_(torch.cat([inp, inp])))[0])
    s, c, i = torch.rand(6, 3), torch.randint(0, 9, (6, 3, 4)).to(torch.int32), torch.arange(6)
    (gs, gc, gi), rows = gather_rows([s, c, i], 5)
    # message 1: n + one width per tensor; message 2: 5 x (3 f32 + 12 i32 + 1 i64) bytes, each block on an 8-byte boundary
    assert calls == [(torch.int64, 4), (torch.uint8, 64 + 240 + 40)] and rows == [5, 5]
    assert torch.equal(gs, torch.cat([s[:5], s[:5]])) and torch.equal(gc, torch.cat([c[:5], c[:5]])) and gi.tolist() == [0, 1, 2, 3, 4] * 2


def test_gather_rows_without_a_group_is_no_collective(monkeypatch):
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda *a, **k: pytest.fail("a collective without a process group"))
    s, i = torch.rand(6, 3), torch.arange(6)
    (gs, gi), rows = gather_rows([s, i], 4)
    assert rows == [4] and torch.equal(gs, s[:4]) and gs.data_ptr() == s.data_ptr() and gi.tolist() == [0, 1, 2, 3]


def test_gather_rows_refuses_what_it_cannot_carry(monkeypatch):
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda *a, **k: pytest.fail("refused before any collective"))
    with pytest.raises(FdError):
        gather_rows([torch.zeros(3, 2, dtype=torch.float64)], 3)         # f32 / i32 / i64 only
    with pytest.raises(FdError):
        gather_rows([torch.zeros(3, 2)], 4)                              # fewer rows than n
    with pytest.raises(FdError):
        gather_rows([torch.zeros(3, 2)], 3, fills=(0, 1))                # one fill per tensor
