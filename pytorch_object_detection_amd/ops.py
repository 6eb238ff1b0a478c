"""Tensor-level wrappers over the C-ABI (include/fcosdet.h).  Every function enqueues HIP kernels on torch's
current stream and returns immediately; tensors must be CUDA (ROCm) fp32 and are never copied to the host.

`Rows` describes an NHWC activation as rows x channels with a channel stride / offset, so concatenations are
written in place (torch.cat in HISFcos.py:107,111 disappears) and slices are read without copies.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import math
import os
import re
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ACT_EXP, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ConvParams, FdError, Segs, check  # noqa: F401


CONV_LOG = None     # a list: conv_call appends (closure, description) of every launch it builds (tools/time_train_convs.py replays them); None = off
LAUNCHES = [0]      # C-ABI launches enqueued by this process (every wrapper asks for the stream once per launch): train_ops.SYNC_TRACE differences it


def _stream() -> int:
    LAUNCHES[0] += 1
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise FdError("pytorch_object_detection_amd runs on the GPU only (got a CPU tensor); there is no CPU "
                          "fallback — use the reference or oracle/ for CPU runs")


class Rows:
    """Channel view [rows, C] of a [rows, cs] buffer starting at channel `co`: fp32, or f16 (AMP activations stored as f16: the FD_PREC_F16 conv
    launches and the f16 forms of the elementwise kernels read / write them directly; cs / co stay in elements)."""
    __slots__ = ("buf", "cs", "co", "C")

    def __init__(self, buf: torch.Tensor, co: int = 0, C_: Optional[int] = None):
        assert buf.dim() == 2 and buf.dtype in (torch.float32, torch.float16) and buf.is_contiguous()
        _need_gpu(buf)
        self.buf, self.cs, self.co = buf, buf.shape[1], co
        self.C = buf.shape[1] - co if C_ is None else C_
        assert 0 <= co and co + self.C <= self.cs

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr()

    @property
    def rows(self) -> int:
        return self.buf.shape[0]

    @property
    def f16(self) -> bool:
        return self.buf.dtype == torch.float16

    def slice(self, co: int, C_: int) -> "Rows":
        return Rows(self.buf, self.co + co, C_)

    def tensor(self) -> torch.Tensor:
        return self.buf[:, self.co:self.co + self.C]


def new_rows(rows: int, C_: int, device) -> Rows:
    return Rows(torch.empty(rows, C_, dtype=torch.float32, device=device))


# ---------------------------------------------------------------------------------------------------- weights
def _pad_cin32(w: torch.Tensor) -> torch.Tensor:
    """Zero input channels up to the next multiple of 32 (the kernel masks the matching activation reads: Cin % 4 == 0)."""
    i = w.shape[1]
    if i % 4:
        raise FdError(f"conv weights need Cin % 4 == 0 (got {i})")
    return torch.nn.functional.pad(w.detach(), (0, 0, 0, 0, 0, (-i) % 32)) if i % 32 else w


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW -> [Cout][Cin/32][KH][KW][32] contiguous: K runs (32-channel chunk, tap, channel-in-chunk), the order the
    conv kernel walks its K-tiles in (taps of one chunk adjacent -> shifted input re-reads stay in L1/L2)."""
    w = _pad_cin32(w)
    o, i, kh, kw = w.shape
    return w.detach().float().reshape(o, i // 32, 32, kh, kw).permute(0, 1, 3, 4, 2).contiguous()


def pack_conv_weight_f16x3(w: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 -> [Cout][Cin/32][KH][KW][2][32] f16: per K-tile of 32 the hi plane then the lo plane, where
    w = hi + lo * 2^-11 (hi = fp16(w) round-to-nearest, lo = fp16((w - hi) * 2^11)): FD_PREC_F16X3 operand format."""
    w = _pad_cin32(w)
    o, i, kh, kw = w.shape
    t = w.detach().float().reshape(o, i // 32, 32, kh, kw).permute(0, 1, 3, 4, 2)      # [O, I/32, KH, KW, 32]
    hi = t.half()
    lo = ((t - hi.float()) * 2048.0).half()
    return torch.stack([hi, lo], dim=-2).contiguous()                                   # [O, I/32, KH, KW, 2, 32]


def wave_ok(Cin: int, Cout: int, k: int, stride: int, pad: int) -> bool:
    """Layers FD_TILE_WAVE64 (fd_conv_wave.hip: wave-autonomous 64 x 64 tiles) covers: GEMM-addressed, Cin and Cout multiples of 32."""
    return k == 1 and stride == 1 and pad == 0 and Cin % 32 == 0 and Cout % 32 == 0


def pack_conv_weight_wave(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 1, 1] fp32 -> the MFMA-fragment-order operand of FD_TILE_WAVE64 (fd_pack_conv_weight_wave_f32), one HIP launch."""
    w = w.detach().float().contiguous()
    _need_gpu(w)
    co, ci = w.shape[0], w.shape[1]
    nb = _lib.lib().fd_conv_weight_wave_bytes(co, ci)
    if nb < 0 or w.numel() != co * ci:
        raise FdError(f"pack_conv_weight_wave: needs a 1x1 filter bank with Cin % 32 == 0 (got {tuple(w.shape)})")
    out = torch.empty(nb // 4, dtype=torch.float32, device=w.device)
    check(_lib.lib().fd_pack_conv_weight_wave_f32(w.data_ptr(), out.data_ptr(), co, ci, _stream()), "fd_pack_conv_weight_wave_f32")
    return out


def pack_stem_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout,3,7,7] -> [Cout][7][8][4], zero at kw=7 and c=3 (FD_CONV_STEM)."""
    co = w.shape[0]
    p = torch.zeros(co, 7, 8, 4, dtype=torch.float32, device=w.device)
    p[:, :, :7, :3] = w.detach().permute(0, 2, 3, 1).float()
    return p.contiguous()


def pack_stem7_weight(w: torch.Tensor) -> torch.Tensor:
    """[64,3,7,7] -> [7 filter rows][22][64]: k = 3 * column + channel, k = 21 zero (fd_stem7x7_nhwc4)."""
    if tuple(w.shape) != (64, 3, 7, 7):
        raise FdError(f"the stem kernel takes a [64, 3, 7, 7] filter bank (got {tuple(w.shape)})")
    p = torch.zeros(7, 22, 64, dtype=torch.float32, device=w.device)
    p[:, :21, :] = w.detach().float().permute(2, 3, 1, 0).reshape(7, 21, 64)
    return p.contiguous()


def stem7x7(x4: Rows, w722: torch.Tensor, y: Rows, N: int, H: int, W: int, scale=None, shift=None, act: int = ACT_NONE) -> None:
    """ResNet stem 7x7 s2 p3 (3 -> 64) + scale / shift + act on the [N][H][W][4] image rows: its own LDS-staged MFMA kernel."""
    _need_gpu(w722, scale, shift)
    if x4.cs != 4 or x4.co != 0 or y.C != 64:
        raise FdError("stem7x7: input must be the [rows][4] image buffer, output a 64-channel view")
    check(_lib.lib().fd_stem7x7_nhwc4(x4.ptr, w722.data_ptr(), scale.data_ptr() if scale is not None else None,
                                      shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, N, H, W, act, _stream()),
          "fd_stem7x7_nhwc4")


def stem7x7_pool(x4: Rows, w722: torch.Tensor, y: Rows, N: int, H: int, W: int, scale=None, shift=None) -> None:
    """ResNet stem 7x7 s2 p3 (3 -> 64) + scale / shift + ReLU + max-pool 3x3 s2 p1 in one call (fd_stem7x7_pool_nhwc4): y = the pooled map; the
    64-channel stride-2 map is never written."""
    _need_gpu(w722, scale, shift)
    if x4.cs != 4 or x4.co != 0 or y.C != 64:
        raise FdError("stem7x7_pool: input must be the [rows][4] image buffer, output a 64-channel view")
    check(_lib.lib().fd_stem7x7_pool_nhwc4(x4.ptr, w722.data_ptr(), scale.data_ptr() if scale is not None else None,
                                           shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, N, H, W, _stream()),
          "fd_stem7x7_pool_nhwc4")


def stem7x7_nchw(x: torch.Tensor, w722: torch.Tensor, y: Rows, scale=None, shift=None, act: int = ACT_NONE, pool: bool = False) -> None:
    """The stem (pool: + ReLU + max-pool 3x3 s2 p1) straight from the reference's fp32 [N, 3, H, W] input tensor (fd_stem7x7_nchw3): the planes are
    read by the patch loader, no [N][H][W][4] copy of the batch is made."""
    _need_gpu(x, w722, scale, shift)
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous() or y.C != 64:
        raise FdError("stem7x7_nchw: input must be a contiguous fp32 [N, 3, H, W] tensor, output a 64-channel view")
    N, _, H, W = x.shape
    check(_lib.lib().fd_stem7x7_nchw3(x.data_ptr(), w722.data_ptr(), scale.data_ptr() if scale is not None else None,
                                      shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, N, H, W, act, 1 if pool else 0, _stream()),
          "fd_stem7x7_nchw3")


def pack_dw_weight(w: torch.Tensor) -> torch.Tensor:
    """[C,1,3,3] -> [9][C]."""
    return w.detach().reshape(w.shape[0], 9).t().contiguous().float()


def pack_dwk_weight(w: torch.Tensor) -> torch.Tensor:
    """[C,1,K,K] -> [K*K][C] (fd_dwconv2d_nhwc)."""
    return w.detach().reshape(w.shape[0], -1).t().contiguous().float()


def stem7x7_wgrad_workspace(N: int, H: int, W: int, device) -> torch.Tensor:
    """The workspace of stem7x7_wgrad for an [N, 3, H, W] batch (fd_stem7x7_wgrad_workspace_bytes: the fp32 partial slabs of the fixed pixel partition)."""
    nb = _lib.lib().fd_stem7x7_wgrad_workspace_bytes(N, H, W)
    if nb < 0:
        raise FdError(f"fd_stem7x7_wgrad_workspace_bytes: N >= 1 and even H, W >= 2 (got N={N}, H={H}, W={W})")
    return torch.empty(nb // 4, dtype=torch.float32, device=device)


def stem7x7_wgrad(x4: Rows, dy: Rows, N: int, H: int, W: int, y: Optional[Rows] = None, scale: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient [64, 3, 7, 7] of the ResNet stem 7x7 s2 p3 given dy on the [N][H/2][W/2] rows (fd_stem7x7_bwd_weight_nhwc4).  `y`: the forward output
    after ReLU -- the mask dy * [y > 0] is applied in the kernel's loader; `scale` multiplies the result per output channel (a frozen BatchNorm folded into
    the forward).  dy / y may be 64-channel views.  Deterministic; two launches, no host sync."""
    _need_gpu(x4.buf, dy.buf, y.buf if y is not None else None, scale, ws)
    if x4.cs != 4 or x4.co != 0 or dy.C != 64 or (y is not None and y.C != 64) or dy.f16 or x4.f16 or (y is not None and y.f16):
        raise FdError("stem7x7_wgrad: input must be the fp32 [rows][4] image buffer, dy (and y) fp32 64-channel views")
    if x4.rows != N * H * W or dy.rows * 4 != N * H * W or (y is not None and y.rows != dy.rows):
        raise FdError(f"stem7x7_wgrad: {x4.rows} image rows / {dy.rows} gradient rows do not match N={N}, H={H}, W={W}")
    if ws is None:
        ws = stem7x7_wgrad_workspace(N, H, W, dy.buf.device)
    dw = torch.empty(64, 3, 7, 7, dtype=torch.float32, device=dy.buf.device)
    check(_lib.lib().fd_stem7x7_bwd_weight_nhwc4(x4.ptr, dy.ptr, dy.cs, dy.co, y.ptr if y is not None else None, y.cs if y is not None else 0,
                                                 y.co if y is not None else 0, scale.data_ptr() if scale is not None else None, dw.data_ptr(),
                                                 ws.data_ptr(), ws.numel() * ws.element_size(), N, H, W, _stream()), "fd_stem7x7_bwd_weight_nhwc4")
    return dw


def pack_stem3_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout,3,K,K] -> [K*K][4][Cout] (fd_stem_conv_nhwc4); input channel 3 is zero."""
    co, ci, kh, kw = w.shape
    p = torch.zeros(kh * kw, 4, co, dtype=torch.float32, device=w.device)
    p[:, :ci, :] = w.detach().float().permute(2, 3, 1, 0).reshape(kh * kw, ci, co)
    return p.contiguous()


def fold_bn(weight, bias, mean, var, eps: float = 1e-5, conv_bias: Optional[torch.Tensor] = None):
    """Frozen BatchNorm2d -> per-channel (scale, shift); a preceding conv bias is absorbed into the shift."""
    scale = (weight.detach().double() / torch.sqrt(var.detach().double() + eps))
    shift = bias.detach().double() - mean.detach().double() * scale
    if conv_bias is not None:
        shift = shift + conv_bias.detach().double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


# ---------------------------------------------------------------------------------------------------- conv
def conv_call(x: Rows, segs: Segs, w_packed: torch.Tensor, y: Rows, *, Cin: int, Cout: int, k: int, stride: int = 1,
              pad: int = 0, dil: int = 1, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
              res: Optional[Rows] = None, act: int = ACT_NONE, act_c0: int = 0,
              seg_param: Optional[Sequence[float]] = None, stem: bool = False, tile: int = 0,
              tag: int = 0, precision: int = 0, ksplit: int = 1,
              workspace: Optional[torch.Tensor] = None, res_mask: bool = False, kw: Optional[int] = None,
              out_hw: Optional[Tuple[int, int]] = None, scatter: Optional[Tuple[int, int, int, int, int, int]] = None,
              gate: Optional[torch.Tensor] = None, w_frag: Optional[torch.Tensor] = None, gn_stats: Optional[torch.Tensor] = None,
              gn_groups: int = 0, gate_b: Optional[torch.Tensor] = None, gate_act: int = ACT_NONE,
              x2: Optional[Rows] = None, x2_stride: int = 1, x2_hw: Optional[Tuple[int, int]] = None, res_up: bool = False,
              sk_wgs: int = 0) -> Callable[[], None]:
    """Build the argument block once; the returned closure launches fd_conv2d_nhwc_f32 on the current stream.
    w_frag: the same weights in FD_TILE_WAVE64's fragment order (pack_conv_weight_wave), which makes that tile selectable."""
    _need_gpu(w_packed, scale, shift)
    p = ConvParams()
    p.x, p.w, p.y = x.ptr, w_packed.data_ptr(), y.ptr
    p.scale = scale.data_ptr() if scale is not None else None
    p.shift = shift.data_ptr() if shift is not None else None
    p.res = res.ptr if res is not None else None
    p.x_cs, p.x_co, p.y_cs, p.y_co = x.cs, x.co, y.cs, y.co
    if res is not None:
        p.res_cs, p.res_co = res.cs, res.co
    p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.dil = Cin, Cout, k, (k if kw is None else kw), stride, pad, dil
    if out_hw is not None:
        p.out_H, p.out_W = out_hw
    if scatter is not None:           # (sy, sx, oy, ox, H, W): output pixel (i, j) -> (sy*i + oy, sx*j + ox) of an [N, H, W] map
        p.sc_sy, p.sc_sx, p.sc_oy, p.sc_ox, p.sc_H, p.sc_W = scatter
    p.act, p.act_c0, p.mode = act, act_c0, (_lib.CONV_STEM if stem else _lib.CONV_GENERIC)
    p.tile, p.tag, p.precision, p.ksplit = tile, tag, precision, ksplit
    p.res_mode = 1 if (res_mask and res is not None) else 0
    if res_up:        # `res` = the coarser level [batch, H / 2, W / 2]: added after the activation at (i / 2, j / 2) (fd_conv_params.res_mode 2)
        if res is None or res_mask or segs.nseg != 1 or res.rows != segs.batch * (segs.H[0] // 2) * (segs.W[0] // 2):
            raise FdError("conv_call: res_up needs a single-level conv and a residual of batch * (H / 2) * (W / 2) rows, no mask")
        p.res_mode = 2
    if gate is not None:             # [levels * batch, >= Cin] fp32: per-(level, image, input channel) gate applied in the loader (1x1 convs)
        _need_gpu(gate, gate_b)
        if gate.dim() != 2 or gate.shape[0] != segs.batch * segs.nseg or gate.stride(1) != 1 or gate.dtype != torch.float32:
            raise FdError("conv gate must be a [levels * batch, C] fp32 tensor with unit channel stride")
        p.gate, p.gate_cs = gate.data_ptr(), gate.stride(0)
        if gate_b is not None:       # x' = gate_act(x * gate + gate_b): the preceding GroupNorm's affine + activation (groupnorm_from_rowstats coef)
            if gate_b.shape != gate.shape or gate_b.stride() != gate.stride() or gate_b.dtype != torch.float32:
                raise FdError("conv gate_b must have gate's shape and strides")
            p.gate_b, p.gate_act = gate_b.data_ptr(), gate_act
    if gn_stats is not None:         # [rows, gn_groups, 2] fp32: row-group (sum, sum of squares) of the stored output (GroupNorm fused into the producer)
        _need_gpu(gn_stats)
        if gn_stats.dtype != torch.float32 or not gn_stats.is_contiguous() or gn_stats.numel() < y.rows * gn_groups * 2:
            raise FdError("conv gn_stats must be a contiguous fp32 buffer of rows x gn_groups x 2")
        p.gn_stats, p.gn_groups = gn_stats.data_ptr(), gn_groups
    if w_frag is not None:
        _need_gpu(w_frag)
        p.w_frag = w_frag.data_ptr()
    if x2 is not None:               # K-concatenated second source (1x1 layers): x2 [batch, x2_hw[0], x2_hw[1]] sampled with x2_stride; w covers Cin + x2.C channels
        p.x2, p.x2_cs, p.x2_co, p.x2_Cin, p.x2_stride = x2.ptr, x2.cs, x2.co, x2.C, x2_stride
        p.x2_H, p.x2_W = x2_hw
    if workspace is not None:
        _need_gpu(workspace)
        p.workspace, p.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    io = (1 if x.f16 else 0) | (2 if y.f16 else 0) | (4 if (res is not None and res.f16) else 0)
    if io:                           # f16 activation maps (AMP): the FD_PREC_F16 kernels read / write them directly (fd_conv_params.io_f16)
        if precision != _lib.PREC_F16:
            raise FdError("conv_call: f16 input / output / residual maps need precision = FD_PREC_F16")
        p.io_f16 = io
    if sk_wgs:                       # FD_TILE_WINOGRAD4 as a persistent stream-K grid of sk_wgs workgroups; workspace = sk_workspace(sk_wgs) (zeroed flags)
        p.sk_wgs = sk_wgs
    if seg_param is not None:
        for i, v in enumerate(seg_param):
            p.seg_param[i] = float(v)
    p.segs = segs
    fn = _lib.lib().fd_conv2d_nhwc_f32
    ref = C.byref(p)
    keep = (x, w_packed, y, scale, shift, res, p, workspace, gate, w_frag, gn_stats, gate_b, x2)

    def run(_keep=keep):
        check(fn(ref, _stream()), "fd_conv2d_nhwc_f32")

    run.params = p  # type: ignore[attr-defined]   (autotuning rewrites p.tile in place)
    if CONV_LOG is not None:
        eb = lambda r: 2 if r.f16 else 4
        rows_in = sum(segs.batch * segs.H[i] * segs.W[i] for i in range(segs.nseg))
        CONV_LOG.append((run, dict(Cin=Cin, Cout=Cout, k=k, stride=stride, dil=dil, rows_in=rows_in, rows_out=y.rows, io=io, precision=precision, res=res is not None,
                                   bytes=rows_in * Cin * eb(x) + y.rows * Cout * eb(y) + (y.rows * Cout * eb(res) if res is not None and not res_up else 0)
                                   + w_packed.numel() * w_packed.element_size(), flops=2 * y.rows * Cout * Cin * k * (k if kw is None else kw))))
    return run


def sk_workspace(sk_wgs: int, device) -> torch.Tensor:
    """Workspace of the persistent stream-K form of an F(4x4) launch (fd_conv_params.sk_wgs): flags (zero, and left zero by every launch) + one 128 KB slot per
    workgroup.  One per concurrently running launch; launches on one stream may share it."""
    n = _lib.lib().fd_conv_sk_workspace_bytes(sk_wgs)
    if n < 0:
        raise FdError(f"fd_conv_sk_workspace_bytes({sk_wgs}): sk_wgs must be a multiple of 8 in 8 .. 1024")
    ws = torch.empty((n + 3) // 4, dtype=torch.float32, device=device)
    ws[:2048].zero_()            # the fixed 8 KB header
    return ws


# F(4x4) launches as a persistent grid with a work queue per XCD (fd_conv_params.sk_wgs): FD_W4_SK=0 keeps every layer on the plain launch
W4_SK = os.environ.get("FD_W4_SK", "1") != "0"


def conv_sk(run, sk_wgs: int, ws: torch.Tensor) -> Callable[[], None]:
    """conv_call()'s F(4x4) launch in its persistent form: sk_wgs workgroups, workspace ws = sk_workspace(>= sk_wgs)."""
    q = _lib.ConvParams()
    C.memmove(C.byref(q), C.byref(run.params), C.sizeof(q))
    q.sk_wgs, q.wg_first, q.wg_count = sk_wgs, 0, 0
    q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    fn = _lib.lib().fd_conv2d_nhwc_f32
    ref = C.byref(q)

    def run_sk(_keep=(run, q, ws)):
        check(fn(ref, _stream()), "fd_conv2d_nhwc_f32")

    run_sk.params = q  # type: ignore[attr-defined]
    return run_sk


def wino4_sk_choice(run, key: str, ws: torch.Tensor, reps: int = 5) -> int:
    """Plain launch (0) or the persistent form with 240 / 256 workgroups for one F(4x4) layer: the committed table first (key = tune_key(..., pre="w4sk")
    of tuned/gfx950_tiles.json, measured on MI355X); a miss is timed on the spot under FD_AUTOTUNE, else stays plain.  The persistent form wins where the
    plain grid ends in a mostly idle round of workgroups and the chunk loop is long enough to carry the pieces' fixed cost (cls_logits, the dilated
    HisBlock conv4, the head tower); elsewhere it costs ~2 % (an extra barrier and a queue claim per item)."""
    if not W4_SK:
        return 0
    table = _tune_table()
    if _TUNE_MODE != "force" and key in table:
        return int(table[key])
    if _TUNE_MODE == "0":
        return 0
    best, best_t = 0, float("inf")
    for wgs in (0, 256, 240):
        call = conv_sk(run, wgs, ws) if wgs else run
        try:
            call()
        except FdError as e:
            if e.rc != _lib.E_UNSUPPORTED:
                raise
            continue
        t = min(_time_launches(call, reps, False) for _ in range(3))
        if t < best_t * 0.98:
            best, best_t = wgs, t
    table[key] = best
    return best


def conv_workgroups(run) -> Tuple[int, int]:
    """(workgroups, non-empty workgroups) of the launch a conv_call() callable describes -- or of its slice, if it is one (FD_TILE_WINOGRAD4 only)."""
    n = _lib.lib().fd_conv_workgroups(C.byref(run.params))
    live = _lib.lib().fd_conv_workgroups_live(C.byref(run.params))
    if n < 0 or live < 0:
        raise FdError("fd_conv_workgroups: " + _lib.lib().fd_last_error().decode(errors="replace"), int(min(n, live)))
    return (run.params.wg_count or n), live


def conv_wg_slice(run, first: int, count: int, tag: Optional[int] = None) -> Callable[[], None]:
    """The workgroups [first, first + count) of conv_call()'s launch as a launch of their own (fd_conv_params.wg_first / wg_count; FD_TILE_WINOGRAD4, first % 8 == 0).
    The slices of a partition of the grid together compute the layer; `tag` overrides the kernel tag (1 = the instantiation rocprof lists as the head tower)."""
    q = _lib.ConvParams()
    C.memmove(C.byref(q), C.byref(run.params), C.sizeof(q))
    q.wg_first, q.wg_count = first, count
    if tag is not None:
        q.tag = tag
    fn = _lib.lib().fd_conv2d_nhwc_f32
    ref = C.byref(q)

    def run_slice(_keep=(run, q)):
        check(fn(ref, _stream()), "fd_conv2d_nhwc_f32")

    run_slice.params = q  # type: ignore[attr-defined]
    return run_slice


def b2b_ok(K1: int, N1: int, N2: int) -> bool:
    """Shapes fd_conv1x1_b2b_f32 covers (two 1x1 stride-1 convs back to back: a bottleneck's conv3 and the next block's conv1)."""
    return K1 % 32 == 0 and N1 % 64 == 0 and N2 in (64, 128)


def conv_b2b_call(x: Rows, w1_frag: torch.Tensor, y: Rows, w2_frag: torch.Tensor, z: Rows, *, K1: int, N1: int, N2: int,
                  scale1: Optional[torch.Tensor] = None, shift1: Optional[torch.Tensor] = None, res: Optional[Rows] = None, act1: int = ACT_NONE,
                  scale2: Optional[torch.Tensor] = None, shift2: Optional[torch.Tensor] = None, act2: int = ACT_NONE) -> Callable[[], None]:
    """y = act1(x . W1^T * scale1 + shift1 + res); z = act2(y . W2^T * scale2 + shift2) in ONE launch (fd_conv1x1_b2b_f32): y is written (it is the next
    residual) but never read back.  w1_frag / w2_frag = pack_conv_weight_wave of the [N1, K1] / [N2, N1] filter banks."""
    _need_gpu(w1_frag, w2_frag, scale1, shift1, scale2, shift2)
    p = _lib.B2BParams()
    p.x, p.w1_frag, p.y, p.w2_frag, p.z = x.ptr, w1_frag.data_ptr(), y.ptr, w2_frag.data_ptr(), z.ptr
    p.scale1 = scale1.data_ptr() if scale1 is not None else None
    p.shift1 = shift1.data_ptr() if shift1 is not None else None
    p.scale2 = scale2.data_ptr() if scale2 is not None else None
    p.shift2 = shift2.data_ptr() if shift2 is not None else None
    p.res = res.ptr if res is not None else None
    p.x_cs, p.x_co, p.y_cs, p.y_co, p.z_cs, p.z_co = x.cs, x.co, y.cs, y.co, z.cs, z.co
    if res is not None:
        p.res_cs, p.res_co = res.cs, res.co
    p.K1, p.N1, p.N2, p.act1, p.act2, p.rows = K1, N1, N2, act1, act2, y.rows
    fn = _lib.lib().fd_conv1x1_b2b_f32
    ref = C.byref(p)
    keep = (x, w1_frag, y, w2_frag, z, scale1, shift1, scale2, shift2, res, p)

    def run(_keep=keep):
        check(fn(ref, _stream()), "fd_conv1x1_b2b_f32")

    run.params = p  # type: ignore[attr-defined]
    return run


_TUNE_CACHE: dict = {}
_TUNE_FILE = os.environ.get("FD_TILE_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gfx950_tiles.json")   # (FD_TILE_TABLE: A/B of two tables)
# FD_AUTOTUNE: "0" (default) = committed table, misses use the shape heuristic (no first-call latency);
#              "1" = time the misses on the spot; "force" = re-time everything (bench.py --save-tuning writes the table)
_TUNE_MODE = os.environ.get("FD_AUTOTUNE", "0")
_TUNE_LOADED = False


def _tune_table() -> dict:
    global _TUNE_LOADED
    if not _TUNE_LOADED:
        _TUNE_LOADED = True
        try:
            with open(_TUNE_FILE) as f:
                _TUNE_CACHE.update(json.load(f))
        except Exception:
            pass
    return _TUNE_CACHE


def save_tune_table() -> None:
    os.makedirs(os.path.dirname(_TUNE_FILE), exist_ok=True)
    with open(_TUNE_FILE, "w") as f:
        json.dump(dict(sorted(_TUNE_CACHE.items())), f, indent=0)


KSPLIT_MAX = 8
_BKEY = re.compile(r"^(f16x3\|)?B(\d+)(\|.*)$")


def tile_code(tile: int, ksplit: int = 1) -> int:
    """The integer a tile table entry / plan.tiles holds for a launch: tile | ksplit << 8 (no split: the upper bits are zero)."""
    return tile | ((ksplit if ksplit > 1 else 0) << 8)


def tile_split(code: int) -> Tuple[int, int]:
    """tile_code's inverse: (tile, ksplit >= 1)."""
    return code & 0xFF, max(1, code >> 8)


def tune_key(segs: Segs, Cin: int, Cout: int, k: int = 3, stride: int = 1, pad: int = 1, dil: int = 1, *, res: bool = False, xcs: int = 0,
             ycs: int = 0, pre: str = "", x2: Optional[Tuple[int, int]] = None, rup: bool = False) -> str:
    """Key of one conv launch in the tile table (tuned/gfx950_tiles.json): "[pre|]B<batch>|<HxW levels>|<Cin>><Cout>|k s p d|res|xcs|ycs" plus
    "|x2s<stride>c<C>" for a K-concatenated second source and "|rup" for a res_up layer's own timing.  pre: "" (fp32), "f16x3" (split-f16 products),
    "f16" (AMP), "pair" (autotune_conv(pair=True)); "w4sk" keys the persistent-F(4x4) choice by "B|levels|Cin>Cout|d|res" alone."""
    hw = "+".join(f"{h}x{w}" for h, w in segs.level_hw())
    if pre == "w4sk":
        return f"w4sk|B{segs.batch}|{hw}|{Cin}>{Cout}|d{dil}|res{int(res)}"
    key = f"B{segs.batch}|{hw}|{Cin}>{Cout}|k{k}s{stride}p{pad}d{dil}|res{int(res)}|xcs{xcs}|ycs{ycs}"
    if pre:
        key = f"{pre}|{key}"
    if x2 is not None:
        key += f"|x2s{x2[0]}c{x2[1]}"
    return key + "|rup" if rup else key


def heuristic_conv(M: int, Cout: int, KT: int, have_ws: bool) -> int:
    """Tile | ksplit << 8 for a shape that is not in the tuned table, distilled from the table: single-LDS-buffer
    tiles (3-4 blocks/CU) whenever they still give >= 2 workgroups per CU, otherwise 64x64 tiles with the K loop
    split so that about 2-4 workgroups per CU exist."""
    if Cout <= 32:
        return 5
    if Cout <= 64:
        tiles, bm, bn = 4, 64, 64
    elif Cout <= 96:
        return 12
    else:
        def nblk(bm_, bn_):
            return -(-M // bm_) * -(-Cout // bn_)
        if nblk(128, 128) >= 768:
            return 7
        if nblk(64, 128) >= 512:
            return 9
        tiles, bm, bn = 4, 64, 64
    n = -(-M // bm) * -(-Cout // bn)
    ks = 1
    if have_ws:
        while ks < KSPLIT_MAX and n * ks < 512 and KT >= 8 * ks:
            ks *= 2
    return tile_code(tiles, ks)


_PAIR_STREAMS: list = []


def _time_launches(run: Callable[[], None], reps: int, pair: bool) -> float:
    """Device milliseconds per launch.  pair=True: the launch runs beside a twin of itself on a second stream (what a layer
    meets under pipeline.TwoLanePipeline, where the other batch's kernels fill its tail): per-launch share of the pair."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not pair:
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    if not _PAIR_STREAMS:
        _PAIR_STREAMS.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    cur = torch.cuda.current_stream()
    e0.record()
    for st in _PAIR_STREAMS:
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            for _ in range(reps):
                run()
    for st in _PAIR_STREAMS:
        cur.wait_stream(st)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (2 * reps)


def autotune_conv(run: Callable[[], None], key: str, M: int, Cout: int, KT: int, reps: int = 3, pair: bool = False) -> int:
    """Block-tile (+ split-K factor) choice for one conv launch.  Looked up in the committed table
    (tuned/gfx950_tiles.json, measured on MI355X) first; a miss is timed on the spot under every sensible tile — and,
    for maps with few tiles, K split 2/4/8 ways — (best of 3 batches of `reps` launches) and remembered for the
    process (bench.py --save-tuning writes the table back).  Returns tile | ksplit << 8 (tile 0 = heuristic)."""
    p = run.params  # type: ignore[attr-defined]
    table = _tune_table()

    def apply(code: int) -> int:
        """Install a table / heuristic / timed code on the launch and return the code ACTUALLY applied (what plan.tiles records)."""
        tile, ks = tile_split(code)
        if tile == _lib.WAVE_TILE and not p.w_frag:
            # the key does not say whether the caller packed the weights in MFMA fragment order (train_ops._conv_launch never does, nor
            # does add_conv for a layer whose shape or epilogue rules the tile out): the wave-autonomous tile is then not available -- fall back to the library's heuristic tile
            tile, ks = 0, 1
        if ks > 1 and (not p.workspace or p.gn_stats):        # (split-K needs the scratch; a row-statistics epilogue has no combine launch)
            ks = 1
        p.tile, p.ksplit = tile, ks
        return tile_code(tile, ks)

    base = key
    if pair:                         # tiles chosen for throughput beside another batch: own table entries, serial ones as fallback
        key = "pair|" + key
    if _TUNE_MODE != "force" and key in table:
        return apply(int(table[key]))
    if _TUNE_MODE == "0":
        if base in table:
            return apply(int(table[base]))
        # the table is keyed by exact shape incl. batch: for another batch size take the measured choice of the nearest larger
        # (else nearest smaller) batch of the same layer geometry, when its tile count says the same regime; else the heuristic
        m = _BKEY.match(base)
        if m:
            pre, b0, rest = m.group(1) or "", int(m.group(2)), m.group(3)
            near = []
            for k2 in table:
                m2 = _BKEY.match(k2)
                if m2 and (m2.group(1) or "") == pre and m2.group(3) == rest:
                    b2 = int(m2.group(2))
                    near.append((abs(b2 - b0) + (0.5 if b2 < b0 else 0.0), b2, k2))
            if near:
                _, b2, k2 = min(near)
                code = int(table[k2])
                if 0.5 <= b0 / b2 <= 2.0 and tile_split(code)[1] == 1:        # (split-K factors depend on the tile count: not transferred)
                    return apply(code)
        return apply(heuristic_conv(M, Cout, KT, bool(p.workspace)))
    cands = [(0, 1)]
    # FD_TILE_128x128_PATCH only exists for 3x3 stride-1 'same' convs whose (128-row tile + halo) patch fits its LDS budget, without split-K
    wmax = max(p.segs.W[i] for i in range(p.segs.nseg))
    patch_ok = (p.KH == 3 and p.KW == 3 and p.stride == 1 and p.pad == p.dil and p.out_H <= 0 and p.sc_H <= 0
                and 128 + 2 * p.dil * (wmax + 1) <= 320)
    wave_tile_ok = bool(p.w_frag) and wave_ok(p.Cin, p.Cout, p.KH, p.stride, p.pad) and p.KW == 1 and p.act_c0 % 32 == 0
    for tid, (bm, bn) in _lib.TILES.items():
        if (tid == _lib.PATCH_TILE and not patch_ok) or (tid == _lib.WAVE_TILE and not wave_tile_ok):
            continue
        padded = -(-Cout // bn) * bn
        if padded <= max(32, int(Cout * 1.34)) and not (bn == 32 and Cout > 32):
            cands.append((tid, 1))
            ntile = -(-M // bm) * -(-Cout // bn)
            if p.workspace and tid not in (_lib.PATCH_TILE, _lib.WAVE_TILE):
                for ks in (2, 4, 8):
                    if ks <= KSPLIT_MAX and KT >= 4 * ks and ntile * ks <= 2048 and ntile < 1024:
                        cands.append((tid, ks))
    best, best_t = 0, float("inf")
    for tid, ks in cands:
        apply(tile_code(tid, ks))
        try:
            run()  # warm
        except FdError as e:          # a tile the library has no kernel for on this layer (FD_E_UNSUPPORTED): not a candidate
            if e.rc != _lib.E_UNSUPPORTED:
                raise
            continue
        t = float("inf")
        for _ in range(3):
            t = min(t, _time_launches(run, reps, pair))
        if t < best_t * 0.985:  # an earlier (simpler) candidate wins near-ties
            best, best_t = tile_code(tid, ks), t
    table[key] = best
    return apply(best)


def conv_wgrad(x: Rows, dy: Rows, segs_in: Segs, *, Cin: int, Cout: int, k: int, stride: int = 1, pad: int = 0,
               dil: int = 1, nsplit: int = 0, scale: Optional[torch.Tensor] = None, oihw: bool = False, precision: int = 0) -> torch.Tensor:
    """Weight gradient of conv(x) w.r.t. its weights given dy (rows in output geometry): [Cout, k, k, Cin] (OHWI), or
    torch's [Cout, Cin, k, k] with oihw=True; `scale` [Cout] multiplies it per output channel (folded frozen BN).
    precision = FD_PREC_F16 (AMP): operands rounded to f16, fp32 accumulation (fd_conv_wgrad_params.precision)."""
    out_rows = conv_out_segs(segs_in, k, stride, pad, dil).rows
    dev = x.buf.device
    dw = torch.empty((Cout, Cin, k, k) if oihw else (Cout, k, k, Cin), dtype=torch.float32, device=dev)
    nb = _lib.lib().fd_conv_wgrad_workspace_bytes(out_rows, Cin, Cout, k, k) if nsplit <= 0 else (nsplit + 8) * dw.numel() * 4
    ws = torch.empty(max(nb // 4, 4), dtype=torch.float32, device=dev)
    p = _lib.WgradParams()
    p.nsplit = max(nsplit, 0)
    p.layout = 1 if oihw else 0
    p.scale = scale.data_ptr() if scale is not None else None
    p.x, p.dy, p.dw = x.ptr, dy.ptr, dw.data_ptr()
    p.x_cs, p.x_co, p.dy_cs, p.dy_co = x.cs, x.co, dy.cs, dy.co
    p.Cin, p.Cout, p.KH, p.KW, p.stride, p.pad, p.dil = Cin, Cout, k, k, stride, pad, dil
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    p.segs = segs_in
    p.precision = precision
    p.io_f16 = (1 if x.f16 else 0) | (2 if dy.f16 else 0)       # (f16 operand maps: FD_PREC_F16 -- the library rejects anything else)
    check(_lib.lib().fd_conv2d_bwd_weight_f32(C.byref(p), _stream()), "fd_conv2d_bwd_weight_f32")
    if CONV_LOG is not None:
        def rerun(_keep=(x, dy, dw, ws, scale, p)):
            check(_lib.lib().fd_conv2d_bwd_weight_f32(C.byref(p), _stream()), "fd_conv2d_bwd_weight_f32")
        rerun.params = p  # type: ignore[attr-defined]
        CONV_LOG.append((rerun, dict(kind="wgrad", Cin=Cin, Cout=Cout, k=k, stride=stride, dil=dil, rows_in=segs_in.rows, rows_out=out_rows, io=p.io_f16, precision=precision,
                                     res=False, bytes=segs_in.rows * Cin * (2 if x.f16 else 4) + out_rows * Cout * (2 if dy.f16 else 4) + dw.numel() * 4,
                                     flops=2 * out_rows * Cout * Cin * k * k)))
    return dw


class WFormat(enum.Enum):
    """Weight formats of the conv kernels: the fd_pack_job.mode bits of the HIP packer that writes the format (| 1 for the flipped / transposed / per-Cout
    scaled weights of the stride-1 data-gradient conv), the tile it implies (0: the direct kernel picks one) and the arithmetic it is packed for.  A conv
    with dgrad=False outputs w.shape[0] channels, one with dgrad=True w.shape[1] (cout()).  NARROW is packed on the torch side (pack_conv_weight_narrow);
    the plans pack DIRECT / DIRECT_F16 on the torch side too (pack_conv_weight / pack_conv_weight_f16x3)."""
    DIRECT = (0, 0, _lib.PREC_F32)                       # [N][K/32][KH][KW][32] fp32
    DIRECT_F16 = (4, 0, _lib.PREC_F16)                   # the (hi, lo) f16 pair [N][K/32][KH][KW][2][32] of FD_PREC_F16 (the plans: FD_PREC_F16X3)
    F16K64 = (16, _lib.F16K64_TILE, _lib.PREC_F16)       # f16 [N][K/64][KH][KW][64]
    WINO = (2, _lib.WINO_TILE, _lib.PREC_F32)            # Winograd F(2x2, 3x3): U = G g G^T (fd_wino_pack_weights_f32)
    WINO4 = (8, _lib.WINO4_TILE, _lib.PREC_F32)          # Winograd F(4x4, 3x3) (fd_wino4_pack_weights_f32)
    NARROW = (None, _lib.NARROW_TILE, _lib.PREC_F32)     # the vector-unit kernel of <= 8 output channels

    def __init__(self, mode, tile, prec):
        self.mode, self.tile, self.prec = mode, tile, prec

    @staticmethod
    def cout(shape, dgrad: bool) -> int:          # (the same rule for every format)
        return shape[1] if dgrad else shape[0]

    def pack(self, w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """OIHW fp32 weights -> this format, one HIP launch; dgrad=True: the data-gradient conv's weights (N = Cin, K = Cout) times the optional per-Cout
        `scale`.  out: re-pack in place into an earlier result of the same call."""
        wino = self in (WFormat.WINO, WFormat.WINO4)
        w = w.detach().float().contiguous() if wino else w.detach().contiguous()
        co, ci, kh, kw = w.shape
        if out is None:
            if wino:
                _need_gpu(w, scale)
                if kh != 3 or kw != 3:
                    raise FdError("Winograd weights need a 3x3 filter")
                n, k = (ci, co) if dgrad else (co, ci)
                nbytes = (_lib.lib().fd_wino4_weight_bytes if self is WFormat.WINO4 else _lib.lib().fd_wino_weight_bytes)(n, k)
                if nbytes < 0:
                    raise FdError(f"Winograd weights need a reduction width that is a multiple of 8 (got {k})")
                out = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            elif self is WFormat.F16K64:         # (half the byte size of the fp32 packing, as an fp32-typed buffer)
                out = torch.empty(co * ci * kh * kw // 2, dtype=torch.float32, device=w.device)
            elif self.mode is not None:
                out = torch.empty((ci, co // 32, kh, kw, 32) if dgrad else (co, ci // 32, kh, kw, 32), dtype=torch.float32, device=w.device)
            else:
                raise FdError(f"{self.name} weights have no HIP packer")
        sp = scale.data_ptr() if (scale is not None and dgrad) else None
        if wino:
            name = "fd_wino4_pack_weights_f32" if self is WFormat.WINO4 else "fd_wino_pack_weights_f32"
            check(getattr(_lib.lib(), name)(w.data_ptr(), sp, out.data_ptr(), co, ci, int(dgrad), _stream()), name)
        else:
            check(_lib.lib().fd_pack_conv_weight_f32(w.data_ptr(), sp, out.data_ptr(), co, ci, kh, kw, self.mode | int(dgrad), _stream()),
                  "fd_pack_conv_weight_f32")
        return out


def pack_conv_weight_hip(w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False, f16: bool = False) -> torch.Tensor:
    """pack_conv_weight (dgrad=False) or dgrad_weight with a per-output-channel scale (dgrad=True) as one HIP launch; f16=True: the
    (hi, lo) f16 operand format of FD_PREC_F16 / FD_PREC_F16X3 (same byte size, returned as an fp32-typed buffer)."""
    return (WFormat.DIRECT_F16 if f16 else WFormat.DIRECT).pack(w, scale, dgrad)


F16K64 = os.environ.get("FD_AMP_K64", "1") != "0"       # "0": AMP convs stay on the K-tile-32 f16 instantiations of the fp32 kernel


def f16k64_ok(Cin: int, Cout: int) -> bool:
    """Shapes FD_TILE_F16K64 covers (reduction width a multiple of 64, 4-channel aligned output)."""
    return Cin % 64 == 0 and Cout % 4 == 0


def amp_format(K: int, N: int) -> WFormat:
    """Weight format of a dense AMP (FD_PREC_F16) conv of reduction width K and N outputs: FD_TILE_F16K64 wherever the widths allow."""
    return WFormat.F16K64 if F16K64 and f16k64_ok(K, N) else WFormat.DIRECT_F16


def pack_conv_weight_f16k64(w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False) -> torch.Tensor:
    """OIHW fp32 -> FD_TILE_F16K64's operand (WFormat.F16K64)."""
    return WFormat.F16K64.pack(w, scale, dgrad)


def pack_conv_weight_wino(w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False) -> torch.Tensor:
    """OIHW [Cout, Cin, 3, 3] -> the Winograd F(2x2, 3x3) operand of FD_TILE_WINOGRAD: U = G g G^T per (cout, cin), packed
    [ceil(N/32)][K/8][16][32][8] (N = Cout, K = Cin; dgrad=True: N = Cin, K = Cout)."""
    return WFormat.WINO.pack(w, scale, dgrad)


def pack_conv_weight_wino4(w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False) -> torch.Tensor:
    """OIHW [Cout, Cin, 3, 3] -> the Winograd F(4x4, 3x3) operand of FD_TILE_WINOGRAD4."""
    return WFormat.WINO4.pack(w, scale, dgrad)


NARROW_MIN_TILES = 128     # below this many 16 x 16 tiles (batch-1 plans) the MFMA kernels' split-K forms are the lower-latency choice


def narrow_ok(Cin: int, Cout: int, k: int, stride: int, pad: int, dil: int) -> bool:
    """Shapes FD_TILE_NARROW covers (fd_conv_narrow.hip: the vector-unit kernel for 3x3 convs of <= 8 output channels)."""
    return k == 3 and stride == 1 and pad == 1 and dil == 1 and 1 <= Cout <= 8 and Cin % 16 == 0


def narrow_tiles(segs: Segs) -> int:
    return sum(segs.batch * -(-h // 16) * -(-w // 16) for h, w in segs.level_hw())


def pack_conv_weight_narrow(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout <= 8, Cin, 3, 3] -> [Cin / 16][3 r][4 quads][3 q][4 k][8 couts] (FD_TILE_NARROW; zero filters past Cout): one (chunk, filter row,
    channel quad, filter column) step is a [4 channels][8 couts] block that the kernel keeps in LDS and reads one row of per lane."""
    w = w.detach().float()
    co, ci, kh, kw = w.shape
    if kh != 3 or kw != 3 or not 1 <= co <= 8 or ci % 16:
        raise FdError(f"narrow-conv weights need a 3x3 filter bank with Cout <= 8 and Cin % 16 == 0 (got {tuple(w.shape)})")
    if co < 8:
        w = torch.cat([w, torch.zeros(8 - co, ci, 3, 3, dtype=w.dtype, device=w.device)], 0)
    # (co, ch, c4, k, r, q) -> (ch, r, c4, q, k, co)
    return w.reshape(8, ci // 16, 4, 4, 3, 3).permute(1, 4, 2, 5, 3, 0).contiguous()


def wino4_ok(Cin: int, Cout: int, k: int, stride: int, pad: int, dil: int) -> bool:
    """Shapes FD_TILE_WINOGRAD4 covers: those of FD_TILE_WINOGRAD."""
    return wino_ok(Cin, Cout, k, stride, pad, dil)


# FD_WINOGRAD4: "1" (default) = layers the F(4x4, 3x3) kernel covers run on it where wino4_choice's cost model says it beats F(2x2, 3x3);
# "0" = never (the round-2 plans); "force" = wherever it applies (tests exercise the kernel inside whole models this way)
WINO4_MODE = os.environ.get("FD_WINOGRAD4", "1")
_W4_FIXED_US = 12.0       # the cost model's per-workgroup prologue + epilogue term, microseconds (fitted; 8 moved more layers onto F(4x4) and lost: profiles/r03y_layer_times_w4_fixed8.tsv)


def wino4_tiles(segs: Segs, dil: int = 1) -> int:
    """4x4 output tiles FD_TILE_WINOGRAD4 enumerates: per level, image and dilation parity class ceil(ceil(H/dil)/4) x ceil(ceil(W/dil)/4)."""
    return sum(segs.batch * dil * dil * (-(-(-(-h // dil)) // 4)) * (-(-(-(-w // dil)) // 4)) for h, w in segs.level_hw())


def wino4_choice(segs: Segs, Cin: int, Cout: int, dil: int = 1, allow_split: bool = True) -> Tuple[bool, int]:
    """(F(4x4, 3x3) instead of F(2x2, 3x3) / the direct kernel?, its split-K factor).  One F(4x4) workgroup owns 32 tiles x 64 couts and a whole CU
    (146 KB of LDS, 2 x 256-register waves per SIMD), so its time goes in ROUNDS of 256 workgroups:
      t_w4(ks) = ceil(ks * workgroups / 256) * ((1.0 + 2.0 * live) us * Cin / 8 / ks + 12 us)  [+ 10 us for the combine launch, ks > 1]
    live = the fraction of the workgroups' 32-cout blocks below Cout (the waves of a dead block skip their MFMAs).  Fitted to the in-plan step
    times of profiles/r03y_layer_times_w4*.tsv at batch 16: head tower 0.94 ms in 9 rounds, layer3.conv2 0.118 in 1, layer2.conv2 0.150 in 2,
    layer1.conv2 0.179 in 4 -- against 0.182 on F(2x2): the break-even case.  Split-K (layer4's 20 x 20 maps: 104 workgroups for 256 CUs) halves
    the chunk loop per workgroup where that fills the chip; there is no row-statistics epilogue (add_conv keeps those launches on F(2x2))."""
    if WINO4_MODE == "0":
        return False, 1
    if WINO4_MODE == "force":
        return True, 1
    wgs = -(-wino4_tiles(segs, dil) // 32) * -(-Cout // 64)
    live = -(-Cout // 32) / (2.0 * -(-Cout // 64))
    nc = Cin // 8
    best_t, best_ks = None, 1
    for ks in ((1, 2, 4) if allow_split else (1,)):
        if ks > 1 and nc < 8 * ks:
            break
        t = -(-wgs * ks // 256) * ((1.0 + 2.0 * live) * nc / ks + _W4_FIXED_US) + (10.0 if ks > 1 else 0.0)
        if best_t is None or t < best_t * 0.9:
            best_t, best_ks = t, ks
    return best_t < 0.95 * _wino_times(segs, Cin, Cout, dil, allow_split)[0], best_ks


def wino_ok(Cin: int, Cout: int, k: int, stride: int, pad: int, dil: int) -> bool:
    """Shapes FD_TILE_WINOGRAD covers (the output / residual views must also be 16-byte addressable)."""
    return k == 3 and stride == 1 and pad == dil and dil in (1, 2) and Cin % 8 == 0 and Cout % 4 == 0


def wino_tiles(segs: Segs, dil: int) -> int:
    """2x2 output tiles the Winograd kernel enumerates: per level, image and dilation parity class ceil(ceil(H/dil)/2) x ceil(ceil(W/dil)/2)."""
    return sum(segs.batch * dil * dil * ((-(-h // dil) + 1) // 2) * ((-(-w // dil) + 1) // 2) for h, w in segs.level_hw())


# FD_WINOGRAD: "1" (default) = 3x3 stride-1 'same' convs (dilation 1 / 2, Cin % 8 == 0) of exact-fp32 arithmetic run on the Winograd F(2x2, 3x3) kernel
# (fd_conv_wino.hip: 2.25x fewer MFMAs, still fp32 arithmetic) where wino_choice says it wins; "force" = wherever it applies, whatever the map size (tests exercise
# the kernel on small maps this way); "0" = every conv on the direct implicit-GEMM kernel (and never on F(4x4) either)
WINO_MODE = os.environ.get("FD_WINOGRAD", "1")


def wino_choice(segs: Segs, Cin: int, Cout: int, dil: int, allow_split: bool = True) -> Tuple[bool, int]:
    """(use the Winograd kernel?, its split-K factor) for a 3x3 stride-1 layer both kernels cover.  Without split-K one Winograd
    workgroup walks all Cin (1.5 us per 8 channels), so a map with few tiles is latency-bound on it while the direct kernel splits K over
    workgroups (floor ~21 us, two launches); wide maps are throughput-bound and Winograd's 2.25x fewer MFMAs win.  A small cost model
    fitted to MI355X measurements (batch 1 .. 16 at 512^2 / 640^2: profiles/r02z_layer_times.tsv, r02z_bench_latency_b*.json):
      t_wino(ks) = (1.5 * Cin / 8 / ks + 3) us * max(1, ks * workgroups / (0.55 * resident slots))  [+ 7 us for the combine launch, ks > 1]
      t_direct   = max(21 us [narrow Cout <= 96: no split-K there, 1.9 us per K-tile], FLOPs / 95 TFLOP/s)"""
    if WINO_MODE == "force":
        return True, 1
    best_t, best_ks, t_d = _wino_times(segs, Cin, Cout, dil, allow_split)[1:]
    return best_t < t_d, best_ks


def _wino_times(segs: Segs, Cin: int, Cout: int, dil: int, allow_split: bool):
    """The cost model of wino_choice: (min(t_wino, t_direct), t_wino at its best split, that split, t_direct), microseconds."""
    T = wino_tiles(segs, dil)
    mt = -(-T // 32)
    nch = 4 if (Cout % 128 == 0 and Cout >= 256 and mt * (Cout // 128) >= 192) else 2      # as fd_launch_conv_wino chooses
    wgs = mt * -(-Cout // (32 * nch))
    slots = 256 * (2 if nch == 2 else 1)
    nc = Cin // 8
    best_t, best_ks = None, 1
    for ks in ((1, 2, 4, 8) if allow_split else (1,)):
        if ks > 1 and nc < 4 * ks:
            break
        t = (1.5 * nc / ks + 3.0) * max(1.0, ks * wgs / (0.55 * slots)) + (7.0 if ks > 1 else 0.0)
        if best_t is None or t < best_t * 0.9:          # (a split has to pay for its workspace traffic)
            best_t, best_ks = t, ks
    flops = 2.0 * segs.rows * max(Cout, 32) * Cin * 9
    floor = 1.9 * (-(-Cin // 32) * 9) if Cout <= 96 else 21.0
    t_d = max(floor, flops / 95e12 * 1e6)
    return min(best_t, t_d), best_t, best_ks, t_d


def wino_preferred(segs: Segs, Cin: int, Cout: int, dil: int) -> bool:
    """wino_choice without split-K (callers that have no workspace: the training nodes)."""
    return wino_choice(segs, Cin, Cout, dil, allow_split=False)[0]


class ConvChoice(NamedTuple):
    fmt: WFormat        # the weight format, which names the kernel family: NARROW / WINO / WINO4, or the direct kernel (DIRECT / DIRECT_F16 / F16K64)
    ksplit: int         # the Winograd kernels' split-K factor (1 elsewhere: the direct kernel's split comes with its tile)
    prec: int           # fd_conv_params.precision


def choose_conv(segs: Segs, Cin: int, Cout: int, k: int, stride: int, pad: int, dil: int, arith: str = "f32", *, split_k: bool = True,
                narrow: bool = True, wino4: bool = True, res: bool = False, gate: bool = False, gate_b: bool = False, gn_stats: bool = False, aligned: bool = True,
                force_wino: bool = False) -> ConvChoice:
    """Kernel family, weight format and Winograd split of one conv layer: the one rule of the inference plans (engine.add_conv and the pre-decisions of
    its callers) and of the training nodes (train_ops).  Touches no tensor and no GPU.
      arith: "f32" (exact fp32), "mixed" (the GEMM-addressed 1x1 layers on split-f16 products), "f16x3" (split-f16 products everywhere),
             "amp" (FD_PREC_F16 operands: the AMP training step -- always the direct kernel)
      what the caller offers: split_k (a split-K workspace), narrow (the vector-unit kernel), wino4 (the F(4x4) kernel), the epilogues it asks for (res, gate, gate_b: the gate is
      a GroupNorm's affine, gn_stats), aligned (16-byte addressable output and residual views: the Winograd kernels' stores), force_wino (the head
      tower, the roofline launch: Winograd whatever its cost model says)."""
    if arith == "amp":
        return ConvChoice(amp_format(Cin, Cout), 1, _lib.PREC_F16)
    exact = arith in ("f32", "mixed")
    # <= 8 output channels (the centre-ness / box predictor): the vector-unit kernel where the map has enough tiles to fill the chip
    if (exact and narrow and not res and (not gate or gate_b) and not gn_stats and narrow_ok(Cin, Cout, k, stride, pad, dil)
            and narrow_tiles(segs) >= NARROW_MIN_TILES):
        return ConvChoice(WFormat.NARROW, 1, _lib.PREC_F32)
    if exact and WINO_MODE != "0" and aligned and wino_ok(Cin, Cout, k, stride, pad, dil):
        if wino4 and not gate and not gn_stats:        # F(4x4) where its cost model beats F(2x2) / the direct kernel: no gate / statistics epilogue
            use4, ks4 = wino4_choice(segs, Cin, Cout, dil, split_k)
            if use4:
                return ConvChoice(WFormat.WINO4, ks4, _lib.PREC_F32)
        use, ks = wino_choice(segs, Cin, Cout, dil, split_k)
        if use or force_wino:
            return ConvChoice(WFormat.WINO, ks, _lib.PREC_F32)
    if arith == "f16x3" or (arith == "mixed" and k == 1 and stride == 1 and not gate and not gn_stats and Cin % 32 == 0):
        return ConvChoice(WFormat.DIRECT_F16, 1, _lib.PREC_F16X3)
    return ConvChoice(WFormat.DIRECT, 1, _lib.PREC_F32)


def strided_dgrad_classes(k: int, stride: int, pad: int):
    """Parity classes of the data gradient of a k x k conv with `stride`: for input rows h = stride*i + a only the taps
    r = r0 + stride*t contribute, and dY row = i + c - t.  Returns per class a: (r0, T taps, c) with r0 = (a + pad) % stride,
    T = number of taps, c = (a + pad - r0) // stride; T == 0: the class is identically zero."""
    out = []
    for a in range(stride):
        r0 = (a + pad) % stride
        T = len(range(r0, k, stride))
        out.append((r0, T, (a + pad - r0) // stride))
    return out


def conv_dgrad_strided(dy: Rows, w: torch.Tensor, scale: Optional[torch.Tensor], dx: Rows, N: int, H: int, W: int, k: int,
                       stride: int, pad: int, res: Optional[Rows] = None, res_mask: bool = False, precision: int = 0) -> bool:
    """dX of y = conv(x, w, stride >= 2, pad, dilation 1) on the MFMA conv kernel, exact FLOPs: one stride-1 launch per parity
    class (h % stride, w % stride) over dY with that class's taps, outputs interleaved straight into dX (fd_conv_params out_H /
    sc_*).  dx must be zero-initialised when some class has no tap (1x1 stride 2).  `scale` [Cout]: a folded frozen BatchNorm;
    res / res_mask as in conv_call (dX geometry).  Returns False (nothing launched) for a geometry it does not cover."""
    Cout, Cin = w.shape[0], w.shape[1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cls = strided_dgrad_classes(k, stride, pad)
    if Cout % 32 or Cin % 4 or any(T and (T - 1 - c) != 0 for _, T, c in cls):
        return False                      # (the class convs of k = 3 / pad 1, k = 1 / pad 0 and k = stride / pad 0 need no padding; others are not built)
    segs = Segs.make(N, [(Ho, Wo)])
    wd = w.detach()
    fmt = amp_format(Cout, Cin) if precision else WFormat.DIRECT       # AMP: the class convs on FD_TILE_F16K64 where the widths allow
    for a, (r0, Ta, _) in enumerate(cls):
        Ia = len(range(a, H, stride))
        for b, (q0, Tb, _) in enumerate(cls):
            Jb = len(range(b, W, stride))
            if Ta == 0 or Tb == 0 or Ia == 0 or Jb == 0:
                continue
            sub = wd[:, :, r0::stride, q0::stride].contiguous()                      # [Cout, Cin, Ta, Tb]
            conv_call(dy, segs, fmt.pack(sub, scale, dgrad=True), dx, Cin=Cout, Cout=Cin, k=Ta, kw=Tb, stride=1, pad=0, res=res, res_mask=res_mask,
                      out_hw=(Ia, Jb), scatter=(stride, stride, a, b, H, W), precision=precision, tile=fmt.tile)()
    return True


def dgrad_weight(w: torch.Tensor) -> torch.Tensor:
    """Packed weights of the stride-1 data-gradient conv: w'[ci][co][r][q] = w[co][ci][K-1-r][K-1-q]."""
    return pack_conv_weight(w.detach().flip(2, 3).transpose(0, 1).contiguous())


def conv_pad(m) -> Optional[int]:
    """The one symmetric zero padding the conv kernels take, read off a square nn.Conv2d-like `m` (kernel_size, dilation, padding): an int / tuple padding
    as it stands, 'valid' = 0, 'same' = dil * (k - 1) / 2.  None where 'same' has no such padding: with dil * (k - 1) odd (an even kernel at an odd dilation)
    torch pads one more row / column at the end than at the start, which the kernels do not take -- callers decline that module."""
    if isinstance(m.padding, str):
        if m.padding == "valid":
            return 0
        total = m.dilation[0] * (m.kernel_size[0] - 1)
        return None if (m.padding != "same" or total % 2) else total // 2
    return m.padding[0]


def conv_out_segs(segs: Segs, k: int, stride: int, pad: int, dil: int) -> Segs:
    hw = [((h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1)
          for h, w in segs.level_hw()]
    return Segs.make(segs.batch, hw)


# ---------------------------------------------------------------------------------------------------- layer ops
def nchw3_to_nhwc4(x: torch.Tensor, y: torch.Tensor) -> None:
    _need_gpu(x, y)
    N, c, H, W = x.shape
    assert c == 3 and x.is_contiguous() and x.dtype == torch.float32
    check(_lib.lib().fd_nchw3_to_nhwc4(x.data_ptr(), y.data_ptr(), N, H, W, _stream()), "fd_nchw3_to_nhwc4")


def preprocess_u8(x: torch.Tensor, y: torch.Tensor, mean, std) -> None:
    """uint8 [N,H,W,3] (resized + zero padded) -> normalised fp32 [N*H*W, 4] (stem input)."""
    _need_gpu(x, y)
    N, H, W, c = x.shape
    assert c == 3 and x.dtype == torch.uint8 and x.is_contiguous()
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().fd_preprocess_u8_nhwc4(x.data_ptr(), y.data_ptr(), N, H, W, m, s_, _stream()), "fd_preprocess_u8_nhwc4")


def boxes_rescale_xywh_(boxes: torch.Tensor, scale: float) -> torch.Tensor:
    """In place: boxes /= scale; (x1, y1, x2, y2) -> (x, y, w, h)  (Test_coco.py:147-151)."""
    _need_gpu(boxes)
    assert boxes.is_contiguous() and boxes.shape[-1] == 4 and boxes.dtype == torch.float32
    check(_lib.lib().fd_boxes_rescale_xywh(boxes.data_ptr(), boxes.numel() // 4, float(scale), _stream()), "fd_boxes_rescale_xywh")
    return boxes


def nhwc_to_nchw(x: Rows, N: int, HW: int, out: torch.Tensor) -> None:
    check(_lib.lib().fd_nhwc_to_nchw(x.ptr, x.cs, x.co, out.data_ptr(), N, HW, x.C, _stream()), "fd_nhwc_to_nchw")


def maxpool(x: Rows, y: Rows, N: int, H: int, W: int, k: int, s: int, pad: int, add: Optional[Rows] = None) -> None:
    a = (add.ptr, add.cs, add.co) if add is not None else (None, 0, 0)
    check(_lib.lib().fd_maxpool_nhwc(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, a[0], a[1], a[2], N, H, W, x.C, k, s, pad,
                                     _stream()), "fd_maxpool_nhwc")


def upsample2x_add(x: Rows, lat: Rows, y: Rows, N: int, H: int, W: int) -> None:
    check(_lib.lib().fd_upsample2x_add_nhwc(x.ptr, x.cs, x.co, lat.ptr, lat.cs, lat.co, y.ptr, y.cs, y.co, N, H, W, x.C,
                                            _stream()), "fd_upsample2x_add_nhwc")


def dwconv3x3(x: Rows, w9c: torch.Tensor, y: Rows, segs: Segs, scale=None, shift=None, act: int = ACT_NONE) -> None:
    check(_lib.lib().fd_dwconv3x3_nhwc(x.ptr, x.cs, x.co, w9c.data_ptr(),
                                       scale.data_ptr() if scale is not None else None,
                                       shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, x.C, act,
                                       C.byref(segs), _stream()), "fd_dwconv3x3_nhwc")


def dwconv2d(x: Rows, wkc: torch.Tensor, y: Rows, N: int, H: int, W: int, K: int, stride: int, pad_top: int, pad_left: int,
             Ho: int, Wo: int, scale=None, shift=None, act: int = ACT_NONE) -> None:
    """Depthwise K x K, stride 1 / 2, asymmetric zero padding (EfficientNet MBConv), + scale / shift + act."""
    check(_lib.lib().fd_dwconv2d_nhwc(x.ptr, x.cs, x.co, wkc.data_ptr(), scale.data_ptr() if scale is not None else None,
                                      shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, N, H, W, x.C, K, stride,
                                      pad_top, pad_left, Ho, Wo, act, _stream()), "fd_dwconv2d_nhwc")


def dwconv2d_dgrad(dy: Rows, wkc: torch.Tensor, dx: Rows, N: int, H: int, W: int, K: int, stride: int, pad_top: int, pad_left: int,
                   Ho: int, Wo: int, scale: Optional[torch.Tensor] = None) -> None:
    """Data gradient of dwconv2d (K in {3, 5}, stride 1 / 2, the forward's padding and sizes): dx = scale * sum of dy * w over the taps that meet each input
    pixel; wkc is the forward's [K*K][C].  Every pixel of dx is written (unreached rows / columns as 0)."""
    _need_gpu(dy.buf, dx.buf, wkc, scale)
    if dy.C != dx.C or dy.rows != N * Ho * Wo or dx.rows != N * H * W or dy.f16 or dx.f16 or tuple(wkc.shape) != (K * K, dx.C):
        raise FdError(f"dwconv2d_dgrad: fp32 dy [{N}*{Ho}*{Wo}, C] / dx [{N}*{H}*{W}, C] views and w [{K * K}, C] expected "
                      f"(got {dy.rows} x {dy.C}, {dx.rows} x {dx.C}, {tuple(wkc.shape)})")
    check(_lib.lib().fd_dwconv2d_bwd_data_nhwc(dy.ptr, dy.cs, dy.co, wkc.data_ptr(), scale.data_ptr() if scale is not None else None, dx.ptr, dx.cs, dx.co,
                                               N, H, W, dx.C, K, stride, pad_top, pad_left, Ho, Wo, _stream()), "fd_dwconv2d_bwd_data_nhwc")


def dwconv2d_wgrad(x: Rows, dy: Rows, N: int, H: int, W: int, K: int, stride: int, pad_top: int, pad_left: int, Ho: int, Wo: int,
                   scale: Optional[torch.Tensor] = None, torch_layout: bool = False) -> torch.Tensor:
    """Weight gradient of dwconv2d given dy: [K*K][C], or [C][1][K][K] with torch_layout; `scale` multiplies it per channel (a frozen BatchNorm folded
    into the forward).  Deterministic; two launches, no host sync."""
    dev = x.buf.device
    _need_gpu(x.buf, dy.buf, scale)
    if dy.C != x.C or dy.rows != N * Ho * Wo or x.rows != N * H * W or dy.f16 or x.f16:
        raise FdError(f"dwconv2d_wgrad: fp32 x [{N}*{H}*{W}, C] / dy [{N}*{Ho}*{Wo}, C] views expected (got {x.rows} x {x.C}, {dy.rows} x {dy.C})")
    nb = _lib.lib().fd_dwconv2d_wgrad_workspace_bytes(N, Ho, Wo, x.C, K)
    if nb < 0:
        raise FdError(f"fd_dwconv2d_wgrad_workspace_bytes: bad arguments (N={N}, Ho={Ho}, Wo={Wo}, C={x.C}, K={K})")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
    dw = torch.empty((x.C, 1, K, K) if torch_layout else (K * K, x.C), dtype=torch.float32, device=dev)
    check(_lib.lib().fd_dwconv2d_bwd_weight_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dw.data_ptr(), x.C, K, stride, pad_top, pad_left, N, H, W, Ho, Wo,
                                                 scale.data_ptr() if scale is not None else None, 1 if torch_layout else 0, ws.data_ptr(), _stream()),
          "fd_dwconv2d_bwd_weight_nhwc")
    return dw


def mbconv_fused_ok(Cin: int, mid: int, K: int, stride: int) -> bool:
    """Shapes fd_mbconv_expand_dw_nhwc covers (the input patch of a tile and two expanded tiles must fit LDS: Cin <= 48)."""
    return K in (3, 5) and stride in (1, 2) and 8 <= Cin <= 48 and Cin % 8 == 0 and mid % 4 == 0


def pack_mbconv_expand_weight(w: torch.Tensor) -> torch.Tensor:
    """[mid, Cin, 1, 1] expand weights -> fd_mbconv_expand_dw_nhwc's fragment order [ceil(mid / 32)][Cin / 8][2][32][4]: element (cb, g, h, l, jj) =
    w[32 cb + l][h * Cin / 2 + 4 g + jj] (a lane's four consecutive K steps are one 16-byte LDS read)."""
    mid, cin = w.shape[0], w.shape[1]
    wp = torch.nn.functional.pad(w.detach().float().reshape(mid, cin), (0, 0, 0, (-mid) % 32))
    return wp.view(-1, 32, 2, cin // 8, 4).permute(0, 3, 2, 1, 4).contiguous()


def mbconv_pool_buffer(N: int, Ho: int, Wo: int, mid: int, K: int, stride: int, device) -> Tuple[torch.Tensor, int]:
    """(per-tile pooling partials buffer, tiles per image) of mbconv_expand_dw."""
    nb = _lib.lib().fd_mbconv_pool_bytes(N, Ho, Wo, mid, K, stride)
    if nb < 0:
        raise FdError("fd_mbconv_pool_bytes: bad arguments")
    return torch.empty(nb // 4, dtype=torch.float32, device=device), nb // 4 // (N * mid)


def mbconv_expand_dw(x: Rows, we_frag: torch.Tensor, sc0, sf0, wkc: torch.Tensor, sc1, sf1, y: Rows, pool: torch.Tensor, N: int, H: int, W: int, K: int, stride: int,
                     pad_top: int, pad_left: int, Ho: int, Wo: int) -> None:
    """MBConv expand 1x1 + BN + swish -> depthwise K x K + BN + swish in one launch (the expanded map stays on chip) + the SE pooling's per-tile partial sums."""
    check(_lib.lib().fd_mbconv_expand_dw_nhwc(x.ptr, x.cs, x.co, we_frag.data_ptr(), sc0.data_ptr(), sf0.data_ptr(), wkc.data_ptr(), sc1.data_ptr(), sf1.data_ptr(),
                                              y.ptr, y.cs, y.co, pool.data_ptr(), N, H, W, x.C, y.C, K, stride, pad_top, pad_left, Ho, Wo, _stream()),
          "fd_mbconv_expand_dw_nhwc")


def se_gate_from_pool(pool: torch.Tensor, T: int, w1, b1, w2, b2, N: int, HW: int, C_: int, Cr: int, ws: torch.Tensor) -> torch.Tensor:
    """The SE gates from mbconv_expand_dw's per-tile partial sums (no pass over the map); returns the [N, C] gate view into `ws` like se_gate."""
    check(_lib.lib().fd_se_gate_from_pool(pool.data_ptr(), T, w1.data_ptr(), b1.data_ptr() if b1 is not None else None, w2.data_ptr(),
                                          b2.data_ptr() if b2 is not None else None, N, HW, C_, Cr, ws.data_ptr(), _stream()), "fd_se_gate_from_pool")
    return se_gate_view(ws, N, HW, C_)


def dwconv_dilated(x: Rows, wkc: torch.Tensor, y: Rows, segs: Segs, K: int, dil: int, scale=None, shift=None, act: int = ACT_NONE) -> None:
    """Dilated depthwise K x K, stride 1, 'same' padding, over a pyramid (MNBlock.DilatedDepthWiseConv + folded BN); w [K*K][C]."""
    _need_gpu(wkc, scale, shift)
    check(_lib.lib().fd_dwconv_dilated_nhwc(x.ptr, x.cs, x.co, wkc.data_ptr(), scale.data_ptr() if scale is not None else None,
                                            shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, x.C, K, dil, act,
                                            C.byref(segs), _stream()), "fd_dwconv_dilated_nhwc")


def stem_conv3(x4: torch.Tensor, w: torch.Tensor, y: Rows, N: int, H: int, W: int, K: int, stride: int, pad_top: int,
               pad_left: int, Ho: int, Wo: int, scale=None, shift=None, act: int = ACT_NONE) -> None:
    """3-channel stem conv on the [N*H*W, 4] image layout (w from pack_stem3_weight)."""
    check(_lib.lib().fd_stem_conv_nhwc4(x4.data_ptr(), w.data_ptr(), scale.data_ptr() if scale is not None else None,
                                        shift.data_ptr() if shift is not None else None, y.ptr, y.cs, y.co, N, H, W, y.C, K, stride,
                                        pad_top, pad_left, Ho, Wo, act, _stream()), "fd_stem_conv_nhwc4")


def collate_u8(images: Sequence[torch.Tensor], H: int, W: int, mean, std, out: Optional[torch.Tensor] = None):
    """Resized uint8 [h_n, w_n, 3] CUDA images of different sizes -> one normalised [N*H*W, 4] fp32 batch
    (dataset/voc.py:128-132,141-156 on the device).  Returns (batch rows tensor, keep-alive tuple)."""
    N = len(images)
    dev = images[0].device
    for t in images:
        _need_gpu(t)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous() or t.shape[0] > H or t.shape[1] > W:
            raise FdError("collate_u8: images must be contiguous CUDA uint8 [h, w, 3] with h <= H and w <= W")
    ptrs = torch.tensor([t.data_ptr() for t in images], dtype=torch.int64).to(dev)
    hw = torch.tensor([[t.shape[0], t.shape[1]] for t in images], dtype=torch.int32).to(dev)
    if out is None:
        out = torch.empty(N * H * W, 4, dtype=torch.float32, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().fd_collate_u8_nhwc4(ptrs.data_ptr(), hw.data_ptr(), out.data_ptr(), N, H, W, m, s_, _stream()),
          "fd_collate_u8_nhwc4")
    return out, (ptrs, hw, tuple(images))


def _check_raw_image(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise FdError(f"{what}: expected a CUDA tensor (the HIP path runs on the GPU only; there is no CPU fallback)")
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous() or t.shape[0] < 1 or t.shape[1] < 1:
        raise FdError(f"{what}: images must be contiguous CUDA uint8 [h, w, 3] with h, w >= 1")


def resize_u8(img: torch.Tensor, nh: int, nw: int) -> torch.Tensor:
    """Raw uint8 [h, w, 3] CUDA image -> uint8 [nh, nw, 3]: the cv2.resize call of preprocess_img_boxes (dataset/voc.py:126,
    Test_coco.py:92) on the device.  Bilinear, half-pixel geometry, integer blending; unpinned against cv2."""
    _check_raw_image(img, "resize_u8")
    nh, nw = int(nh), int(nw)
    if nh < 1 or nw < 1:
        raise FdError(f"resize_u8: destination size must be >= 1 x 1 (got {nh} x {nw})")
    out = torch.empty(nh, nw, 3, dtype=torch.uint8, device=img.device)
    check(_lib.lib().fd_resize_u8(img.data_ptr(), img.shape[0], img.shape[1], out.data_ptr(), nh, nw, _stream()), "fd_resize_u8")
    return out


def resize_collate_u8(images: Sequence[torch.Tensor], dst_hw, H: int, W: int, mean, std, out: Optional[torch.Tensor] = None):
    """RAW uint8 [h_n, w_n, 3] CUDA images -> resized to dst_hw[n] = (nh_n, nw_n), padded to the H x W canvas and normalised:
    one [N*H*W, 4] fp32 batch in ONE launch (preprocess_img_boxes + collate_fn + Normalize, dataset/voc.py:110-156, on the
    device).  Bit-identical to collate_u8 on the images resize_u8 produces.  Returns (batch rows tensor, keep-alive tuple)."""
    images = list(images)
    N = len(images)
    if N < 1:
        raise FdError("resize_collate_u8: empty image list")
    for t in images:
        _check_raw_image(t, "resize_collate_u8")
    dst = [(int(a), int(b)) for a, b in dst_hw]
    if len(dst) != N or any(a < 1 or b < 1 or a > H or b > W for a, b in dst):
        raise FdError("resize_collate_u8: dst_hw must hold one (nh, nw) per image with 1 <= nh <= H and 1 <= nw <= W")
    dev = images[0].device
    if out is None:
        out = torch.empty(N * H * W, 4, dtype=torch.float32, device=dev)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != N * H * W * 4:
        raise FdError("resize_collate_u8: out must be a contiguous CUDA fp32 tensor of N * H * W * 4 elements")
    ptrs = torch.tensor([t.data_ptr() for t in images], dtype=torch.int64).to(dev)
    # one table, one copy: rows 0..N-1 = source sizes, rows N..2N-1 = resized sizes
    hw = torch.tensor([[t.shape[0], t.shape[1]] for t in images] + [list(d) for d in dst], dtype=torch.int32).to(dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().fd_resize_collate_u8_nhwc4(ptrs.data_ptr(), hw.data_ptr(), hw.data_ptr() + 8 * N, out.data_ptr(), N, H, W, m, s_, _stream()),
          "fd_resize_collate_u8_nhwc4")
    return out, (ptrs, hw, tuple(images))


def boxes_scale_batch_(boxes: torch.Tensor, scales: torch.Tensor, counts: Optional[torch.Tensor] = None, invert: bool = True,
                       xywh: bool = False) -> torch.Tensor:
    """In place on padded [B, K, 4] boxes, image b by scales[b] (CUDA fp32 [B]): invert -> boxes / scale (detections back to the
    source image, Test_coco.py:147), else boxes * scale (ground truth onto the resized image, dataset/voc.py:137-138); xywh ->
    then (x1, y1, x2, y2) -> (x, y, w, h) (Test_coco.py:150-151).  Rows at or beyond counts[b] (CUDA int32 [B]) stay untouched."""
    for t, what in ((boxes, "boxes"), (scales, "scales"), (counts, "counts")):
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise FdError(f"boxes_scale_batch_: {what} must be a CUDA tensor (there is no CPU fallback)")
    if boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[2] != 4 or not boxes.is_contiguous():
        raise FdError("boxes_scale_batch_: boxes must be contiguous fp32 [B, K, 4]")
    B, K = int(boxes.shape[0]), int(boxes.shape[1])
    if scales.dtype != torch.float32 or scales.dim() != 1 or scales.shape[0] != B or not scales.is_contiguous():
        raise FdError(f"boxes_scale_batch_: scales must be contiguous fp32 [{B}] (one per image)")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != B or not counts.is_contiguous()):
        raise FdError(f"boxes_scale_batch_: counts must be contiguous int32 [{B}]")
    check(_lib.lib().fd_boxes_scale_batch(boxes.data_ptr(), counts.data_ptr() if counts is not None else None, scales.data_ptr(), B, K,
                                          1 if invert else 0, 1 if xywh else 0, _stream()), "fd_boxes_scale_batch")
    return boxes


# ---------------------------------------------------------------------------------------------- training augmentations
AUG_WORDS = 32                                   # include/fcosdet.h FD_AUG_*: the per-image parameter record
AUG_OP_BRIGHTNESS, AUG_OP_CONTRAST, AUG_OP_SATURATION, AUG_OP_HUE = 1, 2, 3, 4
AUG_MAX_OPS = 4
AUG_MAX_ROT_SIDE = 16384
_AUG_H, _AUG_W, _AUG_FLIP, _AUG_ROT_ON, _AUG_ROT0, _AUG_CROP, _AUG_NH, _AUG_NW, _AUG_NOPS, _AUG_OP0, _AUG_ARG0, _AUG_MEAN_L = 0, 1, 2, 3, 4, 10, 14, 15, 16, 17, 21, 25


def _fix16(v: float) -> int:
    return int(v * 65536.0 + (-0.5 if v < 0 else 0.5))


def rotation_fixed(d: float, h: int, w: int) -> Tuple[int, int, int, int, int, int]:
    """The six 16.16 integers (A0, A1, X0, A3, A4, Y0) of PIL's img.rotate(d) (NEAREST, no expand, centre (w/2, h/2)) on an
    h x w image: destination (x, y) takes source pixel ((X0 + A0*x + A1*y) >> 16, (Y0 + A3*x + A4*y) >> 16).  Doubles in PIL's
    order of operations.  |d| < 90 and sides <= 16384: every |coordinate| stays below (side / 2) * (1 + sqrt 2) * 65536 < 2^31
    (checked here on the four corners), the device adds in 64-bit integers."""
    d, h, w = float(d), int(h), int(w)
    if not abs(d) < 90.0:
        raise FdError(f"rotation_fixed: |d| must be below 90 degrees (got {d})")
    if h < 1 or w < 1 or h > AUG_MAX_ROT_SIDE or w > AUG_MAX_ROT_SIDE:
        raise FdError(f"rotation_fixed: sides must be in 1 .. {AUG_MAX_ROT_SIDE} on the rotation path (got {h} x {w})")
    angle = -math.radians(d % 360.0)
    a0, a1 = round(math.cos(angle), 15), round(math.sin(angle), 15)
    a3, a4 = round(-math.sin(angle), 15), round(math.cos(angle), 15)
    cx, cy = w / 2.0, h / 2.0
    a2 = a0 * -cx + a1 * -cy + 0.0
    a5 = a3 * -cx + a4 * -cy + 0.0
    a2 += cx
    a5 += cy
    fx = (_fix16(a0), _fix16(a1), _fix16(a2 + a0 * 0.5 + a1 * 0.5), _fix16(a3), _fix16(a4), _fix16(a5 + a3 * 0.5 + a4 * 0.5))
    for x in (0, w - 1):
        for y in (0, h - 1):
            if abs(fx[2] + fx[0] * x + fx[1] * y) >= 2 ** 31 or abs(fx[5] + fx[3] * x + fx[4] * y) >= 2 ** 31:
                raise FdError("rotation_fixed: fixed-point coordinate beyond 31 bits")      # unreachable within the limits above
    return fx


def hue_shift(hue: float) -> int:
    """The uint8 added to H (with wrap) for a hue factor in [-0.5, 0.5]: truncation toward zero, modulo 256."""
    hue = float(hue)
    if not -0.5 <= hue <= 0.5:
        raise FdError(f"hue factor must be in [-0.5, 0.5] (got {hue})")
    return int(hue * 255) & 255


def _f32_bits(f: float) -> int:
    return int(np.array([f], np.float32).view(np.int32)[0])


def _check_chain(chain, what: str):
    chain = [(int(op), arg) for op, arg in chain]
    if len(chain) > AUG_MAX_OPS:
        raise FdError(f"{what}: a colour chain holds at most {AUG_MAX_OPS} operations (got {len(chain)})")
    ids = [op for op, _ in chain]
    if any(op not in (AUG_OP_BRIGHTNESS, AUG_OP_CONTRAST, AUG_OP_SATURATION, AUG_OP_HUE) for op in ids) or len(set(ids)) != len(ids):
        raise FdError(f"{what}: chain operations must be distinct AUG_OP_* ids (got {ids})")
    out = []
    for op, arg in chain:
        if op == AUG_OP_HUE:
            arg = int(arg)
            if not 0 <= arg <= 255:
                raise FdError(f"{what}: the hue argument is the uint8 shift 0 .. 255 (ops.hue_shift(factor)); got {arg}")
            out.append((op, arg))
        else:
            f = float(arg)
            if not (math.isfinite(f) and f >= 0.0):
                raise FdError(f"{what}: factor must be finite and >= 0 (got {f})")
            out.append((op, _f32_bits(f)))
    return out


def augment_record(h: int, w: int, *, flip: bool = False, chain=(), d: float = 0.0, crop=None, nh: Optional[int] = None, nw: Optional[int] = None,
                   what: str = "augment_record") -> List[int]:
    """One validated parameter record (include/fcosdet.h FD_AUG_*) as a list of AUG_WORDS ints.  chain: [(AUG_OP_*, factor or
    uint8 hue shift)] in application order; d: rotation in degrees (0: off); crop: (x, y, cw, ch) inside the image or None;
    nh, nw: resized size of the crop (default: the crop's own size)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h > 65536 or w > 65536:
        raise FdError(f"{what}: image sides must be in 1 .. 65536 (got {h} x {w})")
    x, y, cw, ch = (0, 0, w, h) if crop is None else (int(v) for v in crop)
    if cw < 1 or ch < 1 or x < 0 or y < 0 or x + cw > w or y + ch > h:
        raise FdError(f"{what}: crop {(x, y, cw, ch)} (x, y, w, h) is not inside the {h} x {w} image")
    nh, nw = ch if nh is None else int(nh), cw if nw is None else int(nw)
    if nh < 1 or nw < 1:
        raise FdError(f"{what}: resized size must be >= 1 x 1 (got {nh} x {nw})")
    ops_ = _check_chain(chain, what)
    rec = [0] * AUG_WORDS
    rec[_AUG_H], rec[_AUG_W], rec[_AUG_FLIP] = h, w, 1 if flip else 0
    if float(d) != 0.0:
        rec[_AUG_ROT_ON] = 1
        rec[_AUG_ROT0:_AUG_ROT0 + 6] = rotation_fixed(d, h, w)
    rec[_AUG_CROP:_AUG_CROP + 4] = [x, y, cw, ch]
    rec[_AUG_NH], rec[_AUG_NW], rec[_AUG_NOPS] = nh, nw, len(ops_)
    for k, (op, bits) in enumerate(ops_):
        rec[_AUG_OP0 + k], rec[_AUG_ARG0 + k] = op, bits
    return rec


def _has_contrast(rec) -> bool:
    return AUG_OP_CONTRAST in rec[_AUG_OP0:_AUG_OP0 + rec[_AUG_NOPS]]


def jitter_l_sums(images: Sequence[torch.Tensor], recs_dev: torch.Tensor, ptrs: torch.Tensor, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fd_jitter_l_sums: per image with contrast in its chain, the integer sum of L in front of the contrast operation
    (int64 CUDA [N]) and the contrast mean into the records (recs_dev: int32 CUDA [N, AUG_WORDS], ptrs: int64 CUDA [N])."""
    N = len(images)
    _need_gpu(recs_dev, ptrs, *images)
    if recs_dev.dtype != torch.int32 or tuple(recs_dev.shape) != (N, AUG_WORDS) or not recs_dev.is_contiguous() or ptrs.dtype != torch.int64 or ptrs.numel() != N:
        raise FdError("jitter_l_sums: recs_dev must be contiguous int32 [N, AUG_WORDS] and ptrs int64 [N]")
    if sums is None:
        sums = torch.empty(N, dtype=torch.int64, device=recs_dev.device)
    elif not sums.is_cuda or sums.dtype != torch.int64 or sums.numel() != N or not sums.is_contiguous():
        raise FdError("jitter_l_sums: sums must be a contiguous CUDA int64 tensor of N elements")
    mp = max(int(t.shape[0]) * int(t.shape[1]) for t in images)
    check(_lib.lib().fd_jitter_l_sums(ptrs.data_ptr(), recs_dev.data_ptr(), sums.data_ptr(), N, mp, _stream()), "fd_jitter_l_sums")
    return sums


def augment_resize_collate_u8(images: Sequence[torch.Tensor], params, H: int, W: int, mean, std, out: Optional[torch.Tensor] = None):
    """RAW uint8 [h_n, w_n, 3] CUDA images -> flipped / colour-jittered / rotated / cropped as params[n] says, resized, padded to
    the H x W canvas and normalised: the planar fp32 [N, 3, H, W] batch of the reference's collate_fn in ONE launch (plus the
    L-sum launch when a chain holds contrast).  params[n]: dict(flip=, chain=, d=, crop=, nh=, nw=), the keywords of
    augment_record.  Returns (batch, keep-alive tuple).  Does not synchronise."""
    images = list(images)
    N = len(images)
    if N < 1:
        raise FdError("augment_resize_collate_u8: empty image list")
    for t in images:
        _check_raw_image(t, "augment_resize_collate_u8")
    params = list(params)
    if len(params) != N:
        raise FdError("augment_resize_collate_u8: one parameter set per image")
    H, W = int(H), int(W)
    recs = []
    for t, p in zip(images, params):
        rec = augment_record(int(t.shape[0]), int(t.shape[1]), what="augment_resize_collate_u8", **p)
        if rec[_AUG_NH] > H or rec[_AUG_NW] > W:
            raise FdError(f"augment_resize_collate_u8: resized size {rec[_AUG_NH]} x {rec[_AUG_NW]} exceeds the {H} x {W} canvas")
        recs.append(rec)
    dev = images[0].device
    if out is None:
        out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != N * 3 * H * W:
        raise FdError("augment_resize_collate_u8: out must be a contiguous CUDA fp32 tensor of N * 3 * H * W elements")
    # one table, one copy: the N image pointers (two int32 words each) in front, then the N records
    table = np.empty(N * (AUG_WORDS + 2), np.int32)
    table[:2 * N] = np.array([t.data_ptr() for t in images], np.int64).view(np.int32)
    table[2 * N:] = np.array(recs, np.int64).astype(np.int32).reshape(-1)
    tab = torch.from_numpy(table).to(dev, non_blocking=True)
    ptrs, recs_dev = tab[:2 * N].view(torch.int64), tab[2 * N:].view(N, AUG_WORDS)
    sums = None
    if any(_has_contrast(r) for r in recs):
        sums = jitter_l_sums(images, recs_dev, ptrs)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().fd_augment_resize_collate_u8(ptrs.data_ptr(), recs_dev.data_ptr(), out.data_ptr(), N, H, W, m, s_, _stream()),
          "fd_augment_resize_collate_u8")
    return out.view(N, 3, H, W), (tab, sums, tuple(images))


# mosaic: include/fcosdet.h FD_MOSAIC_*, the per-output placement record
MOSAIC_WORDS = 12
_MOSAIC_XC, _MOSAIC_YC, _MOSAIC_FILL, _MOSAIC_PX0 = 0, 1, 2, 3
MOSAIC_MAX_N = 16383                             # 4 * N records must fit fd_jitter_l_sums
MOSAIC_MAX_OFFSET = 65536


def _pack_fill(fill, what: str) -> int:
    try:
        r, g, b = (int(v) for v in fill)
    except (TypeError, ValueError):
        raise FdError(f"{what}: fill must be three levels 0 .. 255 (got {fill!r})") from None
    if not all(0 <= v <= 255 for v in (r, g, b)) or any(float(v) != int(v) for v in fill):
        raise FdError(f"{what}: fill must be three levels 0 .. 255 (got {fill!r})")
    return r | (g << 8) | (b << 16)


def mosaic_collate_u8(images: Sequence[torch.Tensor], tiles, centres, H: int, W: int, mean, std, fill=(0, 0, 0), out: Optional[torch.Tensor] = None):
    """Mosaic of RAW uint8 [h, w, 3] CUDA images: output n is an H x W canvas split at centres[n] = (xc, yc) into four quadrants
    (tile 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right); tiles[n][t] = dict(src=index into images, px=, py=, plus the
    keywords of augment_record: flip=, chain=, d=, crop=, nh=, nw=) puts the augmented, nh x nw resized source with its pixel
    (0, 0) at canvas (py, px), clipped to quadrant t; what no tile covers is `fill` (R, G, B).  Pixels inside a tile are exactly
    those of augment_resize_collate_u8 for that record; then Normalize: the planar fp32 [N, 3, H, W] batch in ONE launch (plus the
    L-sum launch over the 4 * N records when a chain holds contrast) after one table upload.  A source may be used in any number
    of tiles and outputs.  Returns (batch, keep-alive tuple).  Does not synchronise."""
    what = "mosaic_collate_u8"
    images = list(images)
    if len(images) < 1:
        raise FdError(f"{what}: empty image list")
    for t in images:
        _check_raw_image(t, what)
    tiles, centres = [list(q) for q in tiles], [tuple(c) for c in centres]
    N = len(tiles)
    if N < 1 or N > MOSAIC_MAX_N or len(centres) != N:
        raise FdError(f"{what}: 1 .. {MOSAIC_MAX_N} outputs, one centre and four tiles each (got {N} tile sets, {len(centres)} centres)")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > 65536 or W > 65536 or H * W >= 2 ** 31:
        raise FdError(f"{what}: bad canvas {H} x {W}")
    if any(float(v) == 0.0 for v in std):
        raise FdError(f"{what}: zero std")
    packed_fill = _pack_fill(fill, what)
    recs, slots, place = [], [], []
    for n, (quad, c) in enumerate(zip(tiles, centres)):
        if len(quad) != 4 or len(c) != 2:
            raise FdError(f"{what}: output {n} needs four tiles and a centre (xc, yc)")
        xc, yc = int(c[0]), int(c[1])
        if not (0 <= xc <= W and 0 <= yc <= H):
            raise FdError(f"{what}: centre {(xc, yc)} of output {n} is outside 0 .. {W} / 0 .. {H}")
        row = [xc, yc, packed_fill]
        for tile in quad:
            kw = dict(tile)
            try:
                src, px, py = int(kw.pop("src")), int(kw.pop("px")), int(kw.pop("py"))
            except KeyError as e:
                raise FdError(f"{what}: a tile needs src=, px= and py= (missing {e})") from None
            if not 0 <= src < len(images):
                raise FdError(f"{what}: tile source {src} is not an index into the {len(images)} images")
            if abs(px) > MOSAIC_MAX_OFFSET or abs(py) > MOSAIC_MAX_OFFSET:
                raise FdError(f"{what}: tile offset {(px, py)} beyond +-{MOSAIC_MAX_OFFSET}")
            img = images[src]
            rec = augment_record(int(img.shape[0]), int(img.shape[1]), what=what, **kw)
            if rec[_AUG_NH] > 65536 or rec[_AUG_NW] > 65536:
                raise FdError(f"{what}: resized tile {rec[_AUG_NH]} x {rec[_AUG_NW]} has a side above 65536")
            recs.append(rec)
            slots.append(img)
            row += [px, py]
        place.append(row + [0])
    dev = images[0].device
    if out is None:
        out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != N * 3 * H * W:
        raise FdError(f"{what}: out must be a contiguous CUDA fp32 tensor of N * 3 * H * W elements")
    # one table, one copy: the 4N tile pointers (two int32 words each) in front, then the 4N records, then the N placements
    S = 4 * N
    table = np.empty(S * (AUG_WORDS + 2) + N * MOSAIC_WORDS, np.int32)
    table[:2 * S] = np.array([t.data_ptr() for t in slots], np.int64).view(np.int32)
    table[2 * S:S * (AUG_WORDS + 2)] = np.array(recs, np.int64).astype(np.int32).reshape(-1)
    table[S * (AUG_WORDS + 2):] = np.array(place, np.int64).astype(np.int32).reshape(-1)
    tab = torch.from_numpy(table).to(dev, non_blocking=True)
    ptrs, recs_dev, place_dev = tab[:2 * S].view(torch.int64), tab[2 * S:S * (AUG_WORDS + 2)].view(S, AUG_WORDS), tab[S * (AUG_WORDS + 2):]
    sums = None
    if any(_has_contrast(r) for r in recs):
        sums = jitter_l_sums(slots, recs_dev, ptrs)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().fd_mosaic_collate_u8(ptrs.data_ptr(), recs_dev.data_ptr(), place_dev.data_ptr(), out.data_ptr(), N, H, W, m, s_, _stream()),
          "fd_mosaic_collate_u8")
    return out.view(N, 3, H, W), (tab, sums, tuple(images))


def rotate_u8(img: torch.Tensor, d: float) -> torch.Tensor:
    """PIL's img.rotate(d) (NEAREST, no expand) of a raw uint8 [h, w, 3] CUDA image, exact: 16.16 fixed-point integer
    arithmetic on the device (random_rotation, data/augment.py:26-30).  d == 0 is the identity; |d| >= 90 is refused."""
    _check_raw_image(img, "rotate_u8")
    d = float(d)
    if not abs(d) < 90.0:
        raise FdError(f"rotate_u8: |d| must be below 90 degrees (got {d})")
    h, w = int(img.shape[0]), int(img.shape[1])
    if d == 0.0:
        return img.clone()
    fx = (C.c_int32 * 6)(*rotation_fixed(d, h, w))
    out = torch.empty_like(img)
    check(_lib.lib().fd_rotate_u8(img.data_ptr(), h, w, out.data_ptr(), fx, _stream()), "fd_rotate_u8")
    return out


def color_jitter_u8(img: torch.Tensor, chain) -> torch.Tensor:
    """One raw uint8 [h, w, 3] CUDA image through a colour chain [(AUG_OP_*, factor or uint8 hue shift), ...] -> uint8:
    PIL's ImageEnhance Brightness / Contrast / Color and the HSV hue shift, exact."""
    _check_raw_image(img, "color_jitter_u8")
    h, w = int(img.shape[0]), int(img.shape[1])
    rec = augment_record(h, w, chain=chain, what="color_jitter_u8")
    table = np.empty(AUG_WORDS + 2, np.int32)
    table[:2] = np.array([img.data_ptr()], np.int64).view(np.int32)
    table[2:] = np.array(rec, np.int64).astype(np.int32)
    tab = torch.from_numpy(table).to(img.device, non_blocking=True)
    ptrs, rec_dev = tab[:2].view(torch.int64), tab[2:].view(1, AUG_WORDS)
    if _has_contrast(rec):
        jitter_l_sums([img], rec_dev, ptrs)
    out = torch.empty_like(img)
    check(_lib.lib().fd_color_jitter_u8(img.data_ptr(), h, w, out.data_ptr(), rec_dev.data_ptr(), _stream()), "fd_color_jitter_u8")
    return out


def dwconv3x3_wgrad(x: Rows, dy: Rows, segs: Segs, scale: Optional[torch.Tensor] = None, torch_layout: bool = False) -> torch.Tensor:
    """Weight gradient of the depthwise 3x3 conv (stride 1, pad 1) given dy: [9][C], or [C][1][3][3] with torch_layout."""
    dev = x.buf.device
    nb = _lib.lib().fd_dwconv3x3_wgrad_workspace_bytes(C.byref(segs), x.C)
    if nb < 0:
        raise FdError("fd_dwconv3x3_wgrad_workspace_bytes: bad arguments")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
    dw = torch.empty((x.C, 1, 3, 3) if torch_layout else (9, x.C), dtype=torch.float32, device=dev)
    check(_lib.lib().fd_dwconv3x3_bwd_weight_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dw.data_ptr(), x.C,
                                                  scale.data_ptr() if scale is not None else None, 1 if torch_layout else 0,
                                                  C.byref(segs), ws.data_ptr(), _stream()), "fd_dwconv3x3_bwd_weight_nhwc")
    return dw


def pack_dwk_weight_reversed(w: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[C,1,K,K] -> [K*K][C] with the taps reversed (and scaled per channel): the weights with which a stride-1 'same' depthwise conv -- odd K, symmetric
    padding -- computes its own data gradient (dx = dw(dy, w'), w'[t] = w[K*K-1-t] * scale)."""
    w = w.detach().float()
    if scale is not None:
        w = w * scale.view(-1, 1, 1, 1)
    return w.flip(2, 3).reshape(w.shape[0], -1).t().contiguous()


def dwconv_dilated_wgrad(x: Rows, dy: Rows, segs: Segs, K: int, dil: int, scale: Optional[torch.Tensor] = None,
                         torch_layout: bool = False) -> torch.Tensor:
    """Weight gradient of the dilated depthwise K x K conv (stride 1, 'same' padding, over a pyramid) given dy: [K*K][C], or [C][1][K][K] with
    torch_layout; `scale` multiplies it per channel (a frozen BatchNorm folded into the forward).  Deterministic; two launches, no host sync."""
    dev = x.buf.device
    _need_gpu(x.buf, dy.buf, scale)
    nb = _lib.lib().fd_dwconv_dilated_wgrad_workspace_bytes(C.byref(segs), x.C, K)
    if nb < 0:
        raise FdError(f"fd_dwconv_dilated_wgrad_workspace_bytes: bad arguments (C={x.C}, K={K})")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
    dw = torch.empty((x.C, 1, K, K) if torch_layout else (K * K, x.C), dtype=torch.float32, device=dev)
    check(_lib.lib().fd_dwconv_dilated_bwd_weight_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dw.data_ptr(), x.C, K, dil,
                                                       scale.data_ptr() if scale is not None else None, 1 if torch_layout else 0,
                                                       C.byref(segs), ws.data_ptr(), _stream()), "fd_dwconv_dilated_bwd_weight_nhwc")
    return dw


def deform_out_hw(H: int, W: int, K: int, stride: int, pad: int, dil: int) -> Tuple[int, int]:
    return (H + 2 * pad - dil * (K - 1) - 1) // stride + 1, (W + 2 * pad - dil * (K - 1) - 1) // stride + 1


def _deform_check(what: str, x: Rows, offset: Rows, mask: Optional[Rows], B: int, H: int, W: int, K: int, stride: int, pad: int, dil: int) -> int:
    """The argument checks the two deformable-conv launches share (the library repeats the geometry ones); returns the output row count."""
    _need_gpu(x.buf, offset.buf, mask.buf if mask is not None else None)
    if not (1 <= K <= 7 and 1 <= stride <= 4 and 0 <= pad <= 7 and 1 <= dil <= 4):
        raise FdError(f"{what}: 1 <= K <= 7, 1 <= stride <= 4, 0 <= pad <= 7, 1 <= dil <= 4 expected (K={K} stride={stride} pad={pad} dil={dil})")
    Ho, Wo = deform_out_hw(H, W, K, stride, pad, dil)
    if B < 1 or H < 1 or W < 1 or Ho < 1 or Wo < 1:
        raise FdError(f"{what}: empty map (B={B} H={H} W={W} -> {Ho} x {Wo})")
    if x.C % 4:
        raise FdError(f"{what}: C % 4 == 0 expected (C={x.C})")
    if x.f16 or offset.f16 or (mask is not None and mask.f16):
        raise FdError(f"{what}: fp32 maps expected")
    if x.rows != B * H * W:
        raise FdError(f"{what}: x has {x.rows} rows, B*H*W = {B * H * W}")
    if offset.C != 2 * K * K or offset.rows != B * Ho * Wo:
        raise FdError(f"{what}: offset must be [B*Ho*Wo = {B * Ho * Wo}, 2*K*K = {2 * K * K}] (got [{offset.rows}, {offset.C}])")
    if mask is not None and (mask.C != K * K or mask.rows != B * Ho * Wo):
        raise FdError(f"{what}: mask must be [B*Ho*Wo = {B * Ho * Wo}, K*K = {K * K}] (got [{mask.rows}, {mask.C}])")
    return B * Ho * Wo


def _view3(r: Optional[Rows]):
    return (r.ptr, r.cs, r.co) if r is not None else (None, 0, 0)


def deform_im2col(x: Rows, offset: Rows, mask: Optional[Rows], cols: Rows, B: int, H: int, W: int, K: int, stride: int = 1, pad: int = 0, dil: int = 1,
                  mask_act: bool = False) -> None:
    """The sampler of modulated deformable convolution (include/fcosdet.h fd_deform_im2col_nhwc): cols[m, t*C + c] = mask[m, t] * bilinear(x_c at the
    offset position of tap t), [B*Ho*Wo, K*K*C].  mask=None: no modulation; mask_act: `mask` holds logits and the kernel applies 2 * sigmoid."""
    M = _deform_check("deform_im2col", x, offset, mask, B, H, W, K, stride, pad, dil)
    _need_gpu(cols.buf)
    if cols.f16 or cols.C != K * K * x.C or cols.rows != M:
        raise FdError(f"deform_im2col: cols must be fp32 [{M}, K*K*C = {K * K * x.C}] (got [{cols.rows}, {cols.C}])")
    check(_lib.lib().fd_deform_im2col_nhwc(x.ptr, x.cs, x.co, offset.ptr, offset.cs, offset.co, *_view3(mask), 1 if mask_act else 0, cols.ptr, cols.cs, cols.co,
                                           B, H, W, x.C, K, stride, pad, dil, _stream()), "fd_deform_im2col_nhwc")


def deform_bwd(dcols: Rows, x: Rows, offset: Rows, mask: Optional[Rows], d_offset: Rows, d_mask: Optional[Rows], d_x: Optional[Rows], B: int, H: int, W: int,
               K: int, stride: int = 1, pad: int = 0, dil: int = 1, mask_act: bool = False) -> None:
    """Backward of deform_im2col from the gradient of the columns (fd_deform_bwd_nhwc): writes d_offset and d_mask (with mask_act: of the logits) --
    deterministic -- and, when d_x is given, ADDS the input gradient into it with fp32 atomics (the caller zeroes it; not bit-reproducible)."""
    M = _deform_check("deform_bwd", x, offset, mask, B, H, W, K, stride, pad, dil)
    _need_gpu(dcols.buf, d_offset.buf, d_mask.buf if d_mask is not None else None, d_x.buf if d_x is not None else None)
    if dcols.f16 or dcols.C != K * K * x.C or dcols.rows != M:
        raise FdError(f"deform_bwd: dcols must be fp32 [{M}, K*K*C = {K * K * x.C}] (got [{dcols.rows}, {dcols.C}])")
    if d_offset.f16 or d_offset.C != offset.C or d_offset.rows != M:
        raise FdError(f"deform_bwd: d_offset must be fp32 [{M}, {offset.C}]")
    if (mask is None) != (d_mask is None) or (d_mask is not None and (d_mask.f16 or d_mask.C != K * K or d_mask.rows != M)):
        raise FdError(f"deform_bwd: d_mask (fp32 [{M}, {K * K}]) comes with mask, and only with it")
    if d_x is not None and (d_x.f16 or d_x.C != x.C or d_x.rows != x.rows):
        raise FdError(f"deform_bwd: d_x must be fp32 [{x.rows}, {x.C}]")
    check(_lib.lib().fd_deform_bwd_nhwc(dcols.ptr, dcols.cs, dcols.co, x.ptr, x.cs, x.co, offset.ptr, offset.cs, offset.co, *_view3(mask), 1 if mask_act else 0,
                                        d_offset.ptr, d_offset.cs, d_offset.co, *_view3(d_mask), *_view3(d_x), B, H, W, x.C, K, stride, pad, dil, _stream()),
          "fd_deform_bwd_nhwc")


def groupnorm_workspace(segs: Segs, G: int, device) -> torch.Tensor:
    n = _lib.lib().fd_groupnorm_workspace_bytes(C.byref(segs), G)
    if n < 0:
        raise FdError("fd_groupnorm_workspace_bytes: bad arguments")
    return torch.empty(n // 8, dtype=torch.float64, device=device)


def groupnorm_act(x: Rows, gamma: torch.Tensor, beta: torch.Tensor, y: Rows, segs: Segs, G: int, act: int,
                  ws: torch.Tensor, eps: float = 1e-5) -> None:
    check(_lib.lib().fd_groupnorm_act_nhwc(x.ptr, x.cs, x.co, gamma.data_ptr(), beta.data_ptr(), y.ptr, y.cs, y.co, x.C,
                                           G, eps, act, C.byref(segs), ws.data_ptr(), _stream()), "fd_groupnorm_act_nhwc")


def groupnorm_from_rowstats(rowstats: torch.Tensor, Cc: int, G: int, eps: float, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                            segs: Segs, ws: torch.Tensor, coef: Optional[torch.Tensor] = None) -> None:
    """Row-group sums left by a producer (conv_call(gn_stats=...), dwconv3x3_gn) -> GroupNorm statistics per (level, image, group) in `ws`
    (groupnorm_workspace layout) and, with `coef` [levels * batch, 2, C], the affine (rstd * gamma, beta - mean * rstd * gamma) a consumer
    applies in its loader."""
    _need_gpu(rowstats, ws, coef, gamma, beta)
    check(_lib.lib().fd_groupnorm_from_rowstats(rowstats.data_ptr(), Cc, G, eps, gamma.data_ptr() if gamma is not None else None,
                                                beta.data_ptr() if beta is not None else None, C.byref(segs), ws.data_ptr(),
                                                coef.data_ptr() if coef is not None else None, _stream()), "fd_groupnorm_from_rowstats")


def groupnorm_apply(x: Rows, gamma: torch.Tensor, beta: torch.Tensor, y: Rows, segs: Segs, G: int, act: int, ws: torch.Tensor, eps: float = 1e-5) -> None:
    """y = act(GroupNorm(x)) from statistics already in `ws` (groupnorm_from_rowstats / an earlier groupnorm_act): one pass over the map."""
    check(_lib.lib().fd_groupnorm_apply_nhwc(x.ptr, x.cs, x.co, gamma.data_ptr(), beta.data_ptr(), y.ptr, y.cs, y.co, x.C, G, eps, act,
                                             C.byref(segs), ws.data_ptr(), _stream()), "fd_groupnorm_apply_nhwc")


def groupnorm_stats(x: Rows, gamma: torch.Tensor, beta: torch.Tensor, segs: Segs, G: int, ws: torch.Tensor, eps: float = 1e-5,
                    coef: Optional[torch.Tensor] = None) -> None:
    """GroupNorm statistics of x per (level, image, group) into `ws` (groupnorm_workspace layout) and, with `coef` [levels * batch, 2, C], the
    affine (rstd * gamma, beta - mean * rstd * gamma) for consumers that normalise themselves (conv_call(gate_b=...), coef_apply)."""
    _need_gpu(ws, coef, gamma, beta)
    check(_lib.lib().fd_groupnorm_stats_nhwc(x.ptr, x.cs, x.co, x.C, G, eps, gamma.data_ptr(), beta.data_ptr(), C.byref(segs), ws.data_ptr(),
                                             coef.data_ptr() if coef is not None else None, _stream()), "fd_groupnorm_stats_nhwc")


def coef_apply(x: Rows, coef_a: torch.Tensor, coef_b: torch.Tensor, y: Rows, segs: Segs, act: int) -> None:
    """y = act(x * coef_a[img] + coef_b[img]) over x's channel view: coef_a / coef_b are [levels * batch, x.C] views (unit channel stride, same row
    stride) into groupnorm_from_rowstats' coef -- the normalise pass of a channel SLICE of a jointly reduced map."""
    _need_gpu(coef_a, coef_b)
    if (coef_a.dim() != 2 or coef_a.shape != (segs.batch * segs.nseg, x.C) or coef_b.shape != coef_a.shape or coef_a.stride() != coef_b.stride()
            or coef_a.stride(1) != 1 or coef_a.dtype != torch.float32 or coef_b.dtype != torch.float32):
        raise FdError("coef_apply: coef_a / coef_b must be [levels * batch, C] fp32 views with unit channel stride and equal row strides")
    check(_lib.lib().fd_coef_apply_nhwc(x.ptr, x.cs, x.co, coef_a.data_ptr(), coef_b.data_ptr(), coef_a.stride(0), y.ptr, y.cs, y.co, x.C, act,
                                        C.byref(segs), _stream()), "fd_coef_apply_nhwc")


def dwconv3x3_gn(x: Rows, w9c: torch.Tensor, y: Rows, segs: Segs, in_coef: Optional[torch.Tensor], in_act: int,
                 gn_stats: Optional[torch.Tensor], gn_groups: int) -> None:
    """Depthwise 3x3 (stride 1, pad 1, no bias) that reads its input as in_act(x * a + b) (in_coef [levels * batch, 2, C] from
    groupnorm_from_rowstats; the zero padding applies to the normalised map) and leaves the row-group sums of its output in gn_stats."""
    _need_gpu(w9c, in_coef, gn_stats)
    check(_lib.lib().fd_dwconv3x3_gn_nhwc(x.ptr, x.cs, x.co, w9c.data_ptr(), in_coef.data_ptr() if in_coef is not None else None, in_act,
                                          y.ptr, y.cs, y.co, x.C, gn_stats.data_ptr() if gn_stats is not None else None, gn_groups,
                                          C.byref(segs), _stream()), "fd_dwconv3x3_gn_nhwc")


def groupnorm_act_bwd(x: Rows, dy: Rows, gamma: torch.Tensor, beta: torch.Tensor, dx: Rows, segs: Segs, G: int, act: int,
                      fwd_ws: torch.Tensor, eps: float = 1e-5):
    """Backward of groupnorm_act (fwd_ws = the forward call's workspace, untouched since).  Returns (dgamma, dbeta)."""
    dev = x.buf.device
    n = _lib.lib().fd_groupnorm_bwd_workspace_bytes(C.byref(segs), x.C)
    if n < 0:
        raise FdError("fd_groupnorm_bwd_workspace_bytes: bad arguments")
    ws = torch.empty(n // 8, dtype=torch.float64, device=dev)
    dgamma = torch.empty(x.C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(x.C, dtype=torch.float32, device=dev)
    check(_lib.lib().fd_groupnorm_act_bwd_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, gamma.data_ptr(), beta.data_ptr(),
                                               dx.ptr, dx.cs, dx.co, dgamma.data_ptr(), dbeta.data_ptr(), x.C, G, eps, act,
                                               C.byref(segs), fwd_ws.data_ptr(), ws.data_ptr(), _stream()),
          "fd_groupnorm_act_bwd_nhwc")
    return dgamma, dbeta


def se_workspace(N: int, HW: int, C_: int, device) -> torch.Tensor:
    n = _lib.lib().fd_se_workspace_bytes(N, HW, C_)
    return torch.empty((n + 7) // 8, dtype=torch.float64, device=device)


def se_scale(x: Rows, w1, b1, w2, b2, y: Rows, N: int, HW: int, Cr: int, ws: torch.Tensor) -> None:
    check(_lib.lib().fd_se_scale_nhwc(x.ptr, x.cs, x.co, w1.data_ptr(), b1.data_ptr() if b1 is not None else None,
                                      w2.data_ptr(), b2.data_ptr() if b2 is not None else None, y.ptr, y.cs, y.co, N, HW,
                                      x.C, Cr, ws.data_ptr(), _stream()), "fd_se_scale_nhwc")


def se_gate(x: Rows, w1, b1, w2, b2, N: int, HW: int, Cr: int, ws: torch.Tensor) -> torch.Tensor:
    """Squeeze-excitation gates only: sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2) as an [N, C] fp32 view into `ws` (se_workspace), for a
    consumer that applies them itself (conv_call(..., gate=...): the MBConv project conv multiplies them in on its way to LDS)."""
    check(_lib.lib().fd_se_scale_nhwc(x.ptr, x.cs, x.co, w1.data_ptr(), b1.data_ptr() if b1 is not None else None,
                                      w2.data_ptr(), b2.data_ptr() if b2 is not None else None, None, 0, 0, N, HW,
                                      x.C, Cr, ws.data_ptr(), _stream()), "fd_se_scale_nhwc")
    return se_gate_view(ws, N, HW, x.C)


def se_gate_view(ws: torch.Tensor, N: int, HW: int, C_: int) -> torch.Tensor:
    """The [N, C] gate array inside an se_workspace buffer (the last N * C floats of its fd_se_workspace_bytes)."""
    nbytes = _lib.lib().fd_se_workspace_bytes(N, HW, C_)
    return ws.view(torch.float32)[nbytes // 4 - N * C_: nbytes // 4].view(N, C_)


def se_scale_bwd(x: Rows, dy: Rows, w1, b1, w2, b2, dx: Rows, N: int, HW: int, Cr: int, fwd_ws: torch.Tensor):
    """Backward of se_scale: writes dx, returns (dw1 [Cr,C], db1 [Cr], dw2 [C,Cr], db2 [C])."""
    dev = x.buf.device
    Cc = x.C
    n = _lib.lib().fd_se_bwd_workspace_bytes(N, HW, Cc)
    ws = torch.empty((n + 7) // 8, dtype=torch.float64, device=dev)
    dw1 = torch.empty(Cr, Cc, dtype=torch.float32, device=dev)
    db1 = torch.empty(Cr, dtype=torch.float32, device=dev)
    dw2 = torch.empty(Cc, Cr, dtype=torch.float32, device=dev)
    db2 = torch.empty(Cc, dtype=torch.float32, device=dev)
    check(_lib.lib().fd_se_scale_bwd_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, w1.data_ptr(), b1.data_ptr() if b1 is not None else None,
                                          w2.data_ptr(), b2.data_ptr() if b2 is not None else None, dx.ptr, dx.cs, dx.co, dw1.data_ptr(),
                                          db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), N, HW, Cc, Cr, fwd_ws.data_ptr(), ws.data_ptr(),
                                          _stream()), "fd_se_scale_bwd_nhwc")
    return dw1, db1, dw2, db2


def act(x: Rows, y: Rows, act_id: int, param: float = 0.0) -> None:
    check(_lib.lib().fd_act_nhwc(x.ptr, x.cs, x.co, y.ptr, y.cs, y.co, x.rows, x.C, act_id, float(param), _stream()), "fd_act_nhwc")


def act_bwd(x: Rows, dy: Rows, dx: Rows, act_id: int, param: float = 0.0) -> None:
    if x.f16 or dy.f16 or dx.f16:          # f16 maps (AMP): all three, or none
        if not (x.f16 and dy.f16 and dx.f16):
            raise FdError("act_bwd: x, dy and dx must all be f16 maps or all fp32")
        check(_lib.lib().fd_act_bwd_nhwc_h(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, x.rows, x.C, act_id, float(param),
                                           _stream()), "fd_act_bwd_nhwc_h")
        return
    check(_lib.lib().fd_act_bwd_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, x.rows, x.C, act_id, float(param),
                                     _stream()), "fd_act_bwd_nhwc")


def maxpool_bwd(x: Rows, dy: Rows, dx: Rows, N: int, H: int, W: int, k: int, s: int, pad: int) -> None:
    check(_lib.lib().fd_maxpool_bwd_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, N, H, W, x.C, k, s, pad,
                                         _stream()), "fd_maxpool_bwd_nhwc")


def upsample2x_bwd(dy: Rows, dx: Rows, N: int, H: int, W: int) -> None:
    """dx [N,H,W] = 2x2 block sums of dy [N,2H,2W]."""
    check(_lib.lib().fd_upsample2x_bwd_nhwc(dy.ptr, dy.cs, dy.co, dx.ptr, dx.cs, dx.co, N, H, W, dx.C, _stream()), "fd_upsample2x_bwd_nhwc")


def _bn_counter(momentum) -> bool:
    """`momentum` is the layer's live num_batches_tracked tensor (nn.BatchNorm2d(momentum=None), the cumulative moving average): the `_cma` entry points
    read it on the device and blend with (float)(1 / n).  One int64 element on the device, already incremented for this batch."""
    if not isinstance(momentum, torch.Tensor):
        return False
    if momentum.dtype != torch.int64 or momentum.numel() != 1 or not momentum.is_cuda:
        raise FdError("a BatchNorm momentum given as a tensor must be num_batches_tracked: one int64 element on the device")
    return True


def batchnorm_update_running(gn_ws: torch.Tensor, rows: int, Cc: int, momentum, eps: float, running_mean: torch.Tensor,
                             running_var: torch.Tensor) -> None:
    """momentum: a float, or the layer's num_batches_tracked tensor (fd_batchnorm_update_running_cma: momentum = 1 / n, read on the device)."""
    _need_gpu(gn_ws, running_mean, running_var)
    if _bn_counter(momentum):
        check(_lib.lib().fd_batchnorm_update_running_cma(gn_ws.data_ptr(), rows, Cc, momentum.data_ptr(), float(eps), running_mean.data_ptr(),
                                                         running_var.data_ptr(), _stream()), "fd_batchnorm_update_running_cma")
        return
    check(_lib.lib().fd_batchnorm_update_running(gn_ws.data_ptr(), rows, Cc, float(momentum), float(eps), running_mean.data_ptr(),
                                                 running_var.data_ptr(), _stream()), "fd_batchnorm_update_running")


def batchnorm_update_running_dev(gn_ws: torch.Tensor, count: torch.Tensor, Cc: int, momentum, eps: float, running_mean: torch.Tensor,
                                 running_var: torch.Tensor) -> None:
    """As batchnorm_update_running with the row count in device memory (`count`: one float64 element, e.g. the tail of SyncBatchNorm's
    all-reduced buffer): no host round trip."""
    _need_gpu(gn_ws, count, running_mean, running_var)
    assert count.dtype == torch.float64 and count.numel() == 1
    if _bn_counter(momentum):
        check(_lib.lib().fd_batchnorm_update_running_dev_cma(gn_ws.data_ptr(), count.data_ptr(), Cc, momentum.data_ptr(), float(eps),
                                                             running_mean.data_ptr(), running_var.data_ptr(), _stream()),
              "fd_batchnorm_update_running_dev_cma")
        return
    check(_lib.lib().fd_batchnorm_update_running_dev(gn_ws.data_ptr(), count.data_ptr(), Cc, float(momentum), float(eps), running_mean.data_ptr(),
                                                     running_var.data_ptr(), _stream()), "fd_batchnorm_update_running_dev")


def batchnorm_train_workspace(rows: int, Cc: int, device) -> torch.Tensor:
    """A workspace of batchnorm_train_fwd / _bwd (fd_batchnorm_train_workspace_bytes) as float64 elements: the forward leaves mean[C], rstd[C] at its start."""
    nb = _lib.lib().fd_batchnorm_train_workspace_bytes(rows, Cc)
    if nb < 0:
        raise FdError(f"batch-statistics BatchNorm over {rows} rows of {Cc} channels: the HIP kernels cover C % 4 == 0, 4 <= C <= 4096, 2 <= rows < 2^31",
                      rc=_lib.E_UNSUPPORTED)
    return torch.empty(nb // 8, dtype=torch.float64, device=device)


def _bn_res_check(who: str, x: Rows, res: Optional[Rows], act_id: int) -> None:
    """The residual forms' own contract: act in {NONE, RELU} (the backward takes its mask from y) and a residual view of x's shape (and element type:
    _bn_maps_f16)."""
    if act_id not in (ACT_NONE, ACT_RELU):
        raise FdError(f"{who}: act must be ACT_NONE or ACT_RELU (the backward takes its mask from the output)", rc=_lib.E_UNSUPPORTED)
    if res is not None and (res.C != x.C or res.rows != x.rows):
        raise FdError(f"{who}: the residual must be a view of x's shape")


def _bn_maps_f16(who: str, x: Rows, **maps: Optional[Rows]) -> bool:
    """The element type of one call's map operands: all fp32 (False) or all f16 (True: the `_h` entry point), x deciding.  A map of the other type is
    refused by name -- the kernels convert nothing between maps."""
    for name, m in maps.items():
        if m is not None and m.f16 != x.f16:
            raise FdError(f"{who}: {name} is {'an f16' if m.f16 else 'an fp32'} map but x is {'f16' if x.f16 else 'fp32'}: the map operands of one call "
                          "share one element type")
    return x.f16


def _bn_sums_check(who: str, sums: torch.Tensor, Cc: int) -> None:
    if sums.dtype != torch.float64 or sums.numel() != 2 * Cc + 1 or not sums.is_contiguous():
        raise FdError(f"{who}: sums must be {2 * Cc + 1} contiguous float64 elements")


def _bn_running(momentum, running_mean, running_var) -> bool:
    """The running statistics move when the momentum and both tensors are given."""
    return momentum is not None and running_mean is not None and running_var is not None


def _bn_running_args(momentum, running_mean, running_var):
    """(`_cma` entry point?, the three operands).  A tensor momentum is the layer's num_batches_tracked: its address goes where the float would, read from
    the live tensor in every call (nothing cached: a captured forward follows the counter)."""
    if not _bn_running(momentum, running_mean, running_var):
        return False, (0.0, None, None)
    if _bn_counter(momentum):
        return True, (momentum.data_ptr(), running_mean.data_ptr(), running_var.data_ptr())
    return False, (float(momentum), running_mean.data_ptr(), running_var.data_ptr())


def _dptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _bn_train_fwd(who: str, res_form: bool, phase: Optional[int], x, sums, gamma, beta, res, y, eps, act_id, total_rows, momentum, running_mean, running_var,
                  ws) -> torch.Tensor:
    """The one body of the four any-width forward wrappers, fd_<who>_nhwc: phase None = the unsynchronised entry point (no phase, sums, total_rows
    operands), res_form = the entry point that takes a residual view behind beta."""
    _need_gpu(x.buf, sums, gamma, beta, res.buf if res is not None else None, y.buf if y is not None else None, running_mean, running_var, ws)
    if (y is not None and (y.C != x.C or y.rows != x.rows)) or any(t is not None and t.numel() != x.C for t in (gamma, beta)):
        raise FdError(f"{who}: views of the same shape and C-element gamma / beta expected")
    half = _bn_maps_f16(who, x, res=res, y=y)
    if res_form:
        _bn_res_check(who, x, res, act_id)
    cma, running = _bn_running_args(momentum, running_mean, running_var)
    if cma and half:
        raise FdError(f"{who}: the cumulative moving average (momentum=None) has no f16-map form; hand it fp32 maps", rc=_lib.E_UNSUPPORTED)
    name = f"fd_{who}_cma_nhwc" if cma else f"fd_{who}_nhwc_h" if half else f"fd_{who}_nhwc"
    if phase is None:
        sync, sym = (), name
    else:
        _bn_sums_check(who, sums, x.C)
        sync, sym = (phase, sums.data_ptr(), float(total_rows)), f"{name} (phase {phase})"
    if ws is None:
        ws = (batchnorm_train_workspace if phase is None else batchnorm_train_sync_workspace)(x.rows, x.C, x.buf.device)
    check(getattr(_lib.lib(), name)(x.ptr, x.cs, x.co, _dptr(gamma), _dptr(beta), *(_view3(res) if res_form else ()), *_view3(y), x.rows, x.C, float(eps),
                                    act_id, *sync, *running, ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), sym)
    return ws


def batchnorm_train_fwd(x: Rows, gamma: torch.Tensor, beta: torch.Tensor, y: Rows, eps: float, act_id: int = ACT_NONE, momentum: Optional[float] = None,
                        running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(BatchNorm(x)) on the batch statistics of the channel view x (fd_batchnorm_train_fwd_nhwc: any C % 4 == 0 up to 4096).  x and y -- in this and
    the wrappers below every MAP operand: x, res, y, dy, dx -- are all fp32 or all f16 Rows; f16 maps go to the `_h` entry point, whose y / dx are the fp32
    kernel's rounded to f16 once and whose statistics, running tensors, dgamma / dbeta and sums are the fp32 kernel's bits (float momentum only).  With `momentum`
    and the running tensors given they are updated in place like nn.BatchNorm2d's.  `momentum` in this and the three wrappers below: a float, or the
    layer's live num_batches_tracked tensor for nn.BatchNorm2d(momentum=None) -- the `_cma` entry point then reads it on the device and blends with 1 / n,
    bit for bit the float form at float32(1 / n).  Returns the workspace batchnorm_train_bwd needs."""
    return _bn_train_fwd("batchnorm_train_fwd", False, None, x, None, gamma, beta, None, y, eps, act_id, 0.0, momentum, running_mean, running_var, ws)


def batchnorm_train_res_fwd(x: Rows, gamma: torch.Tensor, beta: torch.Tensor, res: Rows, y: Rows, eps: float, act_id: int = ACT_NONE,
                            momentum: Optional[float] = None, running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                            ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(BatchNorm(x) + res) on the batch statistics of x (fd_batchnorm_train_res_fwd_nhwc), act in {NONE, RELU}: batchnorm_train_fwd with the residual
    added in the apply pass.  y must not alias x or res.  Returns the workspace: batchnorm_train_bwd with ACT_NONE on the (ReLU-masked) gradient needs it."""
    return _bn_train_fwd("batchnorm_train_res_fwd", True, None, x, None, gamma, beta, res, y, eps, act_id, 0.0, momentum, running_mean, running_var, ws)


def batchnorm_train_sync_workspace(rows: int, Cc: int, device) -> torch.Tensor:
    """A workspace of batchnorm_train_sync_fwd / _bwd (fd_batchnorm_train_sync_workspace_bytes: batchnorm_train_workspace's layout, from ONE row up)."""
    nb = _lib.lib().fd_batchnorm_train_sync_workspace_bytes(rows, Cc)
    if nb < 0:
        raise FdError(f"synchronised batch-statistics BatchNorm over {rows} rows of {Cc} channels: the HIP kernels cover C % 4 == 0, 4 <= C <= 4096, "
                      "1 <= rows < 2^31", rc=_lib.E_UNSUPPORTED)
    return torch.empty(nb // 8, dtype=torch.float64, device=device)

def batchnorm_train_sync_fwd(phase: int, x: Rows, sums: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                             y: Optional[Rows] = None, eps: float = 1e-5, act_id: int = ACT_NONE, total_rows: float = -1.0, momentum: Optional[float] = None,
                             running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                             ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One phase of SyncBatchNorm's forward at any width (fd_batchnorm_train_sync_fwd_nhwc).  Phase 1 writes this rank's sum x, sum x^2 to sums[:2C] (`sums`:
    [2C + 1] float64; the caller puts its row count in sums[2C] and all-reduces); phase 2 normalises x into y with the global statistics, `total_rows` the
    global count or -1 = sums[2C] on the device, and updates the running tensors when `momentum` and both are given.  Returns the workspace: hand phase 1's
    to phase 2, and phase 2's to batchnorm_train_sync_bwd."""
    return _bn_train_fwd("batchnorm_train_sync_fwd", False, phase, x, sums, gamma, beta, None, y, eps, act_id, total_rows, momentum, running_mean, running_var,
                         ws)


def batchnorm_train_sync_res_fwd(phase: int, x: Rows, sums: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                                 res: Optional[Rows] = None, y: Optional[Rows] = None, eps: float = 1e-5, act_id: int = ACT_NONE, total_rows: float = -1.0,
                                 momentum: Optional[float] = None, running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                                 ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One phase of batchnorm_train_sync_fwd's residual form (fd_batchnorm_train_sync_res_fwd_nhwc): phase 2 gives y = act(BatchNorm(x) + res), act in
    {NONE, RELU}; phase 1 is the plain phase 1 and needs no `res`.  Everything else as batchnorm_train_sync_fwd."""
    return _bn_train_fwd("batchnorm_train_sync_res_fwd", True, phase, x, sums, gamma, beta, res, y, eps, act_id, total_rows, momentum, running_mean,
                         running_var, ws)


def _bn_train_bwd(who: str, phase: Optional[int], x, dy, gamma, beta, sums, fwd_ws, dx, dgamma, dbeta, eps, act_id, total_rows, ws) -> torch.Tensor:
    """The one body of the two any-width backward wrappers, fd_<who>_nhwc (phase None: the unsynchronised entry point)."""
    _need_gpu(x.buf, dy.buf, dx.buf if dx is not None else None, gamma, beta, sums, fwd_ws, dgamma, dbeta, ws)
    if x.C != dy.C or x.rows != dy.rows or (dx is not None and (dx.C != x.C or dx.rows != x.rows)):
        raise FdError(f"{who}: views of the same shape expected")
    name = f"fd_{who}_nhwc_h" if _bn_maps_f16(who, x, dy=dy, dx=dx) else f"fd_{who}_nhwc"
    if phase is None:
        sync, sym = (), name
    else:
        _bn_sums_check(who, sums, x.C)
        sync, sym = (phase, sums.data_ptr(), float(total_rows)), f"{name} (phase {phase})"
    if ws is None:
        ws = (batchnorm_train_workspace if phase is None else batchnorm_train_sync_workspace)(x.rows, x.C, x.buf.device)
    check(getattr(_lib.lib(), name)(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, gamma.data_ptr(), beta.data_ptr(), *_view3(dx), _dptr(dgamma),
                                                _dptr(dbeta), x.rows, x.C, float(eps), act_id, *sync, fwd_ws.data_ptr(), ws.data_ptr(),
                                                ws.numel() * ws.element_size(), _stream()), sym)
    return ws


def batchnorm_train_bwd(x: Rows, dy: Rows, gamma: torch.Tensor, beta: torch.Tensor, dx: Rows, eps: float, act_id: int, fwd_ws: torch.Tensor,
                        ws: Optional[torch.Tensor] = None):
    """The backward of batchnorm_train_fwd (fd_batchnorm_train_bwd_nhwc): writes dx, returns (dgamma, dbeta)."""
    dgamma = torch.empty(x.C, dtype=torch.float32, device=x.buf.device)
    dbeta = torch.empty(x.C, dtype=torch.float32, device=x.buf.device)
    _bn_train_bwd("batchnorm_train_bwd", None, x, dy, gamma, beta, None, fwd_ws, dx, dgamma, dbeta, eps, act_id, 0.0, ws)
    return dgamma, dbeta


def batchnorm_train_sync_bwd(phase: int, x: Rows, dy: Rows, gamma: torch.Tensor, beta: torch.Tensor, sums: torch.Tensor, fwd_ws: torch.Tensor,
                             dx: Optional[Rows] = None, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None, eps: float = 1e-5,
                             act_id: int = ACT_NONE, total_rows: float = -1.0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One phase of SyncBatchNorm's backward at any width (fd_batchnorm_train_sync_bwd_nhwc).  Phase 1 writes this rank's sum dz, sum dz * xhat to sums[:2C]
    and dgamma / dbeta (from those local sums); the caller all-reduces sums[:2C]; phase 2 writes dx, `total_rows` as in the forward.  fwd_ws: the forward's
    phase-2 workspace.  Returns the workspace: hand phase 1's to phase 2."""
    return _bn_train_bwd("batchnorm_train_sync_bwd", phase, x, dy, gamma, beta, sums, fwd_ws, dx, dgamma, dbeta, eps, act_id, total_rows, ws)


def batchnorm_sync_fwd(phase: int, x: Rows, sums: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                       y: Optional[Rows] = None, eps: float = 1e-5, act_id: int = ACT_NONE, total_rows: float = -1.0, momentum: Optional[float] = None,
                       running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """batchnorm_train_sync_fwd on the narrow kernel family (fd_batchnorm_sync_fwd_nhwc, the GroupNorm route: C / 4 divides 256, C <= 1024), same parameters
    and protocol.  `sums` is [2C + 1] float64 and OPAQUE to the caller, who only fills sums[2C] with the row count and all-reduces: the forward's sums lie
    interleaved here (sum x, sum x^2 per channel) and planar in the any-width family.  The workspace is a groupnorm_workspace of one image of rows x 1 pixels
    with G = C; phase 2 with `momentum` and both running tensors enqueues fd_batchnorm_update_running_dev on sums[2C:] behind the apply launch."""
    _need_gpu(x.buf, sums, gamma, beta, y.buf if y is not None else None, running_mean, running_var, ws)
    if x.f16 or (y is not None and (y.f16 or y.C != x.C or y.rows != x.rows)) or any(t is not None and t.numel() != x.C for t in (gamma, beta)):
        raise FdError("batchnorm_sync_fwd: fp32 views of the same shape and C-element gamma / beta expected")
    _bn_sums_check("batchnorm_sync_fwd", sums, x.C)
    if ws is None:
        ws = groupnorm_workspace(Segs.make(1, [(x.rows, 1)]), x.C, x.buf.device)
    check(_lib.lib().fd_batchnorm_sync_fwd_nhwc(x.ptr, x.cs, x.co, _dptr(gamma), _dptr(beta), *_view3(y), x.rows, x.C, float(eps), act_id, phase,
                                                sums.data_ptr(), float(total_rows), ws.data_ptr(), _stream()), f"fd_batchnorm_sync_fwd_nhwc (phase {phase})")
    if phase == 2 and _bn_running(momentum, running_mean, running_var):
        batchnorm_update_running_dev(ws, sums[2 * x.C:], x.C, momentum, eps, running_mean, running_var)
    return ws


def batchnorm_sync_bwd(phase: int, x: Rows, dy: Rows, gamma: torch.Tensor, beta: torch.Tensor, sums: torch.Tensor, fwd_ws: torch.Tensor,
                       dx: Optional[Rows] = None, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None, eps: float = 1e-5,
                       act_id: int = ACT_NONE, total_rows: float = -1.0, ws: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """batchnorm_train_sync_bwd on the narrow kernel family (fd_batchnorm_sync_bwd_nhwc), same parameters and protocol; `sums` as in batchnorm_sync_fwd.
    The workspace is fd_groupnorm_bwd_workspace_bytes of the forward's segment table: phase 1 allocates it when none is given, phase 2 reads none."""
    _need_gpu(x.buf, dy.buf, dx.buf if dx is not None else None, gamma, beta, sums, fwd_ws, dgamma, dbeta, ws)
    if x.f16 or dy.f16 or x.C != dy.C or x.rows != dy.rows or (dx is not None and (dx.f16 or dx.C != x.C or dx.rows != x.rows)):
        raise FdError("batchnorm_sync_bwd: fp32 views of the same shape expected")
    _bn_sums_check("batchnorm_sync_bwd", sums, x.C)
    if ws is None and phase == 1:
        nb = _lib.lib().fd_groupnorm_bwd_workspace_bytes(C.byref(Segs.make(1, [(x.rows, 1)])), x.C)
        if nb < 0:
            raise FdError("fd_groupnorm_bwd_workspace_bytes: bad arguments")
        ws = torch.empty(nb // 8, dtype=torch.float64, device=x.buf.device)
    check(_lib.lib().fd_batchnorm_sync_bwd_nhwc(x.ptr, x.cs, x.co, dy.ptr, dy.cs, dy.co, gamma.data_ptr(), beta.data_ptr(), *_view3(dx), _dptr(dgamma),
                                                _dptr(dbeta), x.rows, x.C, float(eps), act_id, phase, sums.data_ptr(), float(total_rows), fwd_ws.data_ptr(),
                                                _dptr(ws), _stream()), f"fd_batchnorm_sync_bwd_nhwc (phase {phase})")
    return ws


def sample_scale_add(a: Rows, s: torch.Tensor, r: Optional[Rows], y: Rows, N: int, HW: int) -> None:
    """y = a * s[n] + r on [N * HW, C] fp32 channel views (fd_sample_scale_add_nhwc: drop-connect); s = N fp32 on the device, r may be None, y may alias a."""
    _need_gpu(a.buf, s, r.buf if r is not None else None, y.buf)
    if a.f16 or y.f16 or (r is not None and r.f16) or s.dtype != torch.float32 or s.numel() != N or not s.is_contiguous():
        raise FdError("sample_scale_add: fp32 views and N contiguous fp32 scales expected")
    if a.rows != N * HW or y.rows != N * HW or a.C != y.C or (r is not None and (r.rows != N * HW or r.C != a.C)):
        raise FdError(f"sample_scale_add: views do not match N={N}, HW={HW}")
    check(_lib.lib().fd_sample_scale_add_nhwc(a.ptr, a.cs, a.co, s.data_ptr(), r.ptr if r is not None else None, r.cs if r is not None else 0,
                                              r.co if r is not None else 0, y.ptr, y.cs, y.co, N, HW, a.C, _stream()), "fd_sample_scale_add_nhwc")


def stem_conv3_wgrad(x4: torch.Tensor, dy: Rows, N: int, H: int, W: int, K: int, stride: int, pad_top: int, pad_left: int, Ho: int, Wo: int,
                     scale: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient [Cout, 3, 3, 3] of stem_conv3 given dy, a Cout-channel view of the [N * Ho * Wo] output rows (fd_stem_conv_bwd_weight_nhwc4); `scale`
    multiplies the result per output channel (a frozen BatchNorm folded into the forward).  Deterministic; two launches, no host sync."""
    _need_gpu(x4, dy.buf, scale, ws)
    if x4.dtype != torch.float32 or x4.dim() != 2 or x4.shape != (N * H * W, 4) or not x4.is_contiguous() or dy.f16 or dy.rows != N * Ho * Wo:
        raise FdError(f"stem_conv3_wgrad: the fp32 [N*H*W, 4] image buffer and fp32 gradient rows [N*Ho*Wo] expected (N={N}, H={H}, W={W}, Ho={Ho}, Wo={Wo})")
    if ws is None:
        nb = _lib.lib().fd_stem_conv_wgrad_workspace_bytes(N, H, W, dy.C, Ho, Wo)
        if nb < 0:
            raise FdError(f"stem_conv3_wgrad: Cout % 4 == 0, Cout <= 64 and a non-empty geometry expected (Cout={dy.C})", rc=_lib.E_UNSUPPORTED)
        ws = torch.empty(nb // 4, dtype=torch.float32, device=dy.buf.device)
    dw = torch.empty(dy.C, 3, K, K, dtype=torch.float32, device=dy.buf.device)
    check(_lib.lib().fd_stem_conv_bwd_weight_nhwc4(x4.data_ptr(), dy.ptr, dy.cs, dy.co, scale.data_ptr() if scale is not None else None, dw.data_ptr(),
                                                   ws.data_ptr(), ws.numel() * ws.element_size(), N, H, W, dy.C, K, stride, pad_top, pad_left, Ho, Wo,
                                                   _stream()), "fd_stem_conv_bwd_weight_nhwc4")
    return dw


# ---------------------------------------------------------------------------------------------------- post-process
def fcos_decode(cls: Rows, cnt: Rows, reg: Rows, segs: Segs, strides: Sequence[int]):
    """-> scores [N,L] f32, classes [N,L] i32, boxes [N,L,4] f32 (levels concatenated per image)."""
    N = segs.batch
    L = sum(h * w for h, w in segs.level_hw())
    dev = cls.buf.device
    scores = torch.empty(N, L, dtype=torch.float32, device=dev)
    classes = torch.empty(N, L, dtype=torch.int32, device=dev)
    boxes = torch.empty(N, L, 4, dtype=torch.float32, device=dev)
    st = (C.c_int32 * len(strides))(*strides)
    check(_lib.lib().fd_fcos_decode(cls.ptr, cls.cs, cls.co, cnt.ptr, cnt.cs, cnt.co, reg.ptr, reg.cs, reg.co, cls.C,
                                    C.byref(segs), st, scores.data_ptr(), classes.data_ptr(), boxes.data_ptr(), _stream()),
          "fd_fcos_decode")
    return scores, classes, boxes


def fcos_topk(scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, K: int, want_idx: bool = False):
    _need_gpu(scores, classes, boxes)
    N, L = scores.shape
    dev = scores.device
    ts = torch.empty(N, K, dtype=torch.float32, device=dev)
    tc = torch.empty(N, K, dtype=torch.int64, device=dev)
    tb = torch.empty(N, K, 4, dtype=torch.float32, device=dev)
    ti = torch.empty(N, K, dtype=torch.int32, device=dev) if want_idx else None
    ws = None
    if K > 1024:        # (FCOSHead(max_detection_box > 1024): the candidate list is sorted in a global scratch)
        nb = _lib.lib().fd_topk_workspace_bytes(N, L, K)
        if nb < 0:
            raise FdError(f"fd_topk_workspace_bytes: bad arguments N={N} L={L} K={K}")
        ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
    check(_lib.lib().fd_fcos_topk(scores.data_ptr(), classes.data_ptr(), boxes.data_ptr(), N, L, K, ts.data_ptr(),
                                  tc.data_ptr(), tb.data_ptr(), ti.data_ptr() if want_idx else None,
                                  ws.data_ptr() if ws is not None else None, _stream()),
          "fd_fcos_topk")
    return (ts, tc, tb, ti) if want_idx else (ts, tc, tb)


_NMS_WS: dict = {}


def _nms_workspace(N: int, K: int, dev) -> torch.Tensor:
    """Per-(device, stream) cached scratch for the suppression bitmask (stream order makes reuse safe)."""
    key = (str(dev), _stream())
    need = _lib.lib().fd_nms_workspace_bytes(N, K)
    if need < 0:
        raise FdError(f"fd_nms_workspace_bytes: unsupported N={N} K={K} (K <= 262144)")
    ws = _NMS_WS.get(key)
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
        _NMS_WS[key] = ws
    return ws


def batched_nms(scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, score_thr: float, iou_thr: float):
    """Padded outputs [N,K] + keep_idx [N,K] (int32, -1 padded) + counts [N] (int32)."""
    _need_gpu(scores, classes, boxes)
    N, K = scores.shape
    assert classes.dtype == torch.int64 and scores.is_contiguous() and classes.is_contiguous() and boxes.is_contiguous()
    dev = scores.device
    os_ = torch.empty(N, K, dtype=torch.float32, device=dev)
    oc = torch.empty(N, K, dtype=torch.int64, device=dev)
    ob = torch.empty(N, K, 4, dtype=torch.float32, device=dev)
    keep = torch.empty(N, K, dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _nms_workspace(N, K, dev)
    check(_lib.lib().fd_batched_nms(scores.data_ptr(), classes.data_ptr(), boxes.data_ptr(), N, K, score_thr, iou_thr,
                                    os_.data_ptr(), oc.data_ptr(), ob.data_ptr(), keep.data_ptr(), counts.data_ptr(),
                                    ws.data_ptr(), _stream()), "fd_batched_nms")
    return os_, oc, ob, keep, counts


def box_nms_plus1(boxes: torch.Tensor, scores: torch.Tensor, thr: float = 0.5, mode: str = "union",
                  n_valid: Optional[torch.Tensor] = None):
    _need_gpu(boxes, scores)
    N, K = scores.shape
    keep = torch.empty(N, K, dtype=torch.int32, device=scores.device)
    counts = torch.empty(N, dtype=torch.int32, device=scores.device)
    check(_lib.lib().fd_box_nms_plus1(boxes.data_ptr(), scores.data_ptr(), n_valid.data_ptr() if n_valid is not None else None,
                                      N, K, thr, {"union": 0, "min": 1}[mode], keep.data_ptr(), counts.data_ptr(), _stream()),
          "fd_box_nms_plus1")
    return keep, counts


def pairwise_iou(a: torch.Tensor, b: torch.Tensor, plus_one: bool) -> torch.Tensor:
    _need_gpu(a, b)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    check(_lib.lib().fd_pairwise_iou(a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], int(plus_one), out.data_ptr(),
                                     _stream()), "fd_pairwise_iou")
    return out


def clip_boxes_(boxes: torch.Tensor, img_h: int, img_w: int) -> torch.Tensor:
    _need_gpu(boxes)
    assert boxes.is_contiguous() and boxes.shape[-1] == 4 and boxes.dtype == torch.float32
    check(_lib.lib().fd_clip_boxes(boxes.data_ptr(), boxes.numel() // 4, img_h, img_w, _stream()), "fd_clip_boxes")
    return boxes


def pack_detections(scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """Padded detections of B images -> one [B, K+1, 6] fp32 message (row 0 = count; then x1, y1, x2, y2, score, class)."""
    _need_gpu(scores, classes, boxes, counts)
    B, K = scores.shape
    assert classes.dtype == torch.int64 and counts.dtype == torch.int32
    rec = torch.empty(B, K + 1, 6, dtype=torch.float32, device=scores.device)
    check(_lib.lib().fd_pack_detections(scores.contiguous().data_ptr(), classes.contiguous().data_ptr(), boxes.contiguous().data_ptr(),
                                        counts.contiguous().data_ptr(), B, K, rec.data_ptr(), _stream()), "fd_pack_detections")
    return rec


def unpack_detections(rec: torch.Tensor):
    """Inverse of pack_detections on [B, K+1, 6] records -> (scores [B,K], classes [B,K] int64, boxes [B,K,4], counts [B] int32)."""
    _need_gpu(rec)
    B, K1, six = rec.shape
    assert six == 6 and rec.is_contiguous() and rec.dtype == torch.float32
    K, dev = K1 - 1, rec.device
    s = torch.empty(B, K, dtype=torch.float32, device=dev)
    c = torch.empty(B, K, dtype=torch.int64, device=dev)
    b = torch.empty(B, K, 4, dtype=torch.float32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.lib().fd_unpack_detections(rec.data_ptr(), B, K, s.data_ptr(), c.data_ptr(), b.data_ptr(), n.data_ptr(), _stream()),
          "fd_unpack_detections")
    return s, c, b, n


# ---------------------------------------------------------------------------------------------------- loss
def ltrb_loss_fwd(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, mode: int):
    _need_gpu(pred, target, mask)
    B, L, _ = pred.shape
    loss = torch.empty(B, dtype=torch.float32, device=pred.device)
    npos = torch.empty(B, dtype=torch.int32, device=pred.device)
    check(_lib.lib().fd_ltrb_iou_loss_fwd(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), B, L, mode, loss.data_ptr(),
                                          npos.data_ptr(), _stream()), "fd_ltrb_iou_loss_fwd")
    return loss, npos


def ltrb_loss_bwd(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, gscale: torch.Tensor, mode: int):
    B, L, _ = pred.shape
    grad = torch.empty_like(pred)
    check(_lib.lib().fd_ltrb_iou_loss_bwd(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), gscale.data_ptr(), B, L, mode,
                                          grad.data_ptr(), _stream()), "fd_ltrb_iou_loss_bwd")
    return grad


def focal_loss_fwd(logits: torch.Tensor, labels: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0) -> torch.Tensor:
    """logits [B,L,C] f32, labels [B,L] int64 -> per-image summed focal loss [B]."""
    _need_gpu(logits, labels)
    B, L, Cn = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = torch.empty(_lib.lib().fd_focal_workspace_bytes(B) // 8, dtype=torch.float64, device=logits.device)
    check(_lib.lib().fd_focal_loss_fwd(logits.data_ptr(), labels.data_ptr(), B, L, Cn, alpha, gamma, loss.data_ptr(),
                                       ws.data_ptr(), _stream()), "fd_focal_loss_fwd")
    return loss


def focal_loss_bwd(logits, labels, gscale, alpha: float = 0.25, gamma: float = 2.0) -> torch.Tensor:
    B, L, Cn = logits.shape
    grad = torch.empty_like(logits)
    check(_lib.lib().fd_focal_loss_bwd(logits.data_ptr(), labels.data_ptr(), gscale.data_ptr(), B, L, Cn, alpha, gamma,
                                       grad.data_ptr(), _stream()), "fd_focal_loss_bwd")
    return grad


QUALITY_KIND = {"qfl": 0, "vfl": 1}      # include/fcosdet.h fd_quality_loss_fwd `kind`


def _quality_kind(kind, who: str) -> int:
    if kind in QUALITY_KIND:
        return QUALITY_KIND[kind]
    if kind in (0, 1) and not isinstance(kind, bool):
        return int(kind)
    raise FdError(f"{who}: kind must be one of {sorted(QUALITY_KIND)} (got {kind!r})")


def _quality_check(who: str, logits, labels, q) -> None:
    if logits.dim() != 3 or tuple(labels.shape) != tuple(logits.shape[:2]) or tuple(q.shape) != tuple(logits.shape[:2]):
        raise FdError(f"{who}: logits {tuple(logits.shape)}, labels {tuple(labels.shape)}, q {tuple(q.shape)}: expected [B,L,C], [B,L], [B,L]")
    if logits.dtype != torch.float32 or q.dtype != torch.float32 or labels.dtype != torch.int64:
        raise FdError(f"{who}: logits and q must be float32 and labels int64 (got {logits.dtype}, {q.dtype}, {labels.dtype})")
    if not (logits.is_contiguous() and labels.is_contiguous() and q.is_contiguous()):
        raise FdError(f"{who}: logits, labels and q must be contiguous")


def ltrb_quality(reg_pred: torch.Tensor, reg_target: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """The soft classification target (fd_ltrb_quality): reg_pred / reg_target [B,L,4] f32 LTRB distances, labels
    [B,L] or [B,L,1] int64 -> q [B,L] f32: 0 where labels <= 0, else the pair's IoU as the LTRB loss computes it, in [0, 1]
    (NaN gives 0).  No gradient: q is a target."""
    _need_gpu(reg_pred, reg_target, labels)
    if reg_pred.dim() != 3 or reg_pred.shape[2] != 4 or reg_target.shape != reg_pred.shape or labels.numel() != reg_pred.shape[0] * reg_pred.shape[1]:
        raise FdError(f"ltrb_quality: reg_pred {tuple(reg_pred.shape)}, reg_target {tuple(reg_target.shape)}, labels {tuple(labels.shape)}: "
                      "expected [B,L,4], [B,L,4], [B,L]")
    if reg_pred.dtype != torch.float32 or reg_target.dtype != torch.float32 or labels.dtype != torch.int64:
        raise FdError(f"ltrb_quality: boxes must be float32 and labels int64 (got {reg_pred.dtype}, {reg_target.dtype}, {labels.dtype})")
    B, L, _ = reg_pred.shape
    rp, rt, lb = reg_pred.detach().contiguous(), reg_target.detach().contiguous(), labels.contiguous()
    q = torch.empty(B, L, dtype=torch.float32, device=reg_pred.device)
    check(_lib.lib().fd_ltrb_quality(rp.data_ptr(), rt.data_ptr(), lb.data_ptr(), B, L, q.data_ptr(), _stream()), "fd_ltrb_quality")
    return q


def quality_loss_fwd(logits: torch.Tensor, labels: torch.Tensor, q: torch.Tensor, kind, alpha: float = 0.75, gamma: float = 2.0):
    """QFL (kind "qfl") or VFL ("vfl") summed per image (fd_quality_loss_fwd): logits [B,L,C] f32, labels [B,L] int64,
    q [B,L] f32, all contiguous -> (loss [B] f32, qsum [B] f32 = sum of q), both summed in doubles in a fixed order."""
    _need_gpu(logits, labels, q)
    k = _quality_kind(kind, "quality_loss_fwd")
    _quality_check("quality_loss_fwd", logits, labels, q)
    B, L, Cn = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    qsum = torch.empty(B, dtype=torch.float32, device=logits.device)
    ws = torch.empty(max(_lib.lib().fd_quality_loss_workspace_bytes(B), 8) // 8, dtype=torch.float64, device=logits.device)
    check(_lib.lib().fd_quality_loss_fwd(logits.data_ptr(), labels.data_ptr(), q.data_ptr(), B, L, Cn, k, float(alpha), float(gamma),
                                         loss.data_ptr(), qsum.data_ptr(), ws.data_ptr(), _stream()), "fd_quality_loss_fwd")
    return loss, qsum


def quality_loss_bwd(logits: torch.Tensor, labels: torch.Tensor, q: torch.Tensor, gscale: torch.Tensor, kind, alpha: float = 0.75,
                     gamma: float = 2.0) -> torch.Tensor:
    """grad [B,L,C] = d loss_b / d logits * gscale[b] of quality_loss_fwd (fd_quality_loss_bwd); gscale [B] f32."""
    _need_gpu(logits, labels, q, gscale)
    k = _quality_kind(kind, "quality_loss_bwd")
    _quality_check("quality_loss_bwd", logits, labels, q)
    B, L, Cn = logits.shape
    if tuple(gscale.shape) != (B,) or gscale.dtype != torch.float32 or not gscale.is_contiguous():
        raise FdError(f"quality_loss_bwd: gscale must be contiguous float32 [{B}] (got {gscale.dtype} {tuple(gscale.shape)})")
    grad = torch.empty_like(logits)
    check(_lib.lib().fd_quality_loss_bwd(logits.data_ptr(), labels.data_ptr(), q.data_ptr(), gscale.data_ptr(), B, L, Cn, k, float(alpha),
                                         float(gamma), grad.data_ptr(), _stream()), "fd_quality_loss_bwd")
    return grad


def bce_loss_fwd(x: torch.Tensor, target: torch.Tensor, mask: torch.Tensor):
    _need_gpu(x, target, mask)
    B, L = x.shape
    loss = torch.empty(B, dtype=torch.float32, device=x.device)
    npos = torch.empty(B, dtype=torch.int32, device=x.device)
    check(_lib.lib().fd_bce_logits_loss_fwd(x.data_ptr(), target.data_ptr(), mask.data_ptr(), B, L, loss.data_ptr(),
                                            npos.data_ptr(), _stream()), "fd_bce_logits_loss_fwd")
    return loss, npos


def bce_loss_bwd(x, target, mask, gscale) -> torch.Tensor:
    B, L = x.shape
    grad = torch.empty_like(x)
    check(_lib.lib().fd_bce_logits_loss_bwd(x.data_ptr(), target.data_ptr(), mask.data_ptr(), gscale.data_ptr(), B, L,
                                            grad.data_ptr(), _stream()), "fd_bce_logits_loss_bwd")
    return grad


def fcos_gen_targets(gt_boxes: torch.Tensor, labels: torch.Tensor, level_hw, strides, ranges, radius: float = 1.5):
    """gt_boxes [B,M,4] f32, labels [B,M] int64 -> (cls [B,L,1] int64, cnt [B,L,1] f32, reg [B,L,4] f32)."""
    _need_gpu(gt_boxes, labels)
    B, M = labels.shape
    segs = Segs.make(B, list(level_hw))
    L = sum(h * w for h, w in level_hw)
    dev = gt_boxes.device
    cls = torch.empty(B, L, 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(B, L, 1, dtype=torch.float32, device=dev)
    reg = torch.empty(B, L, 4, dtype=torch.float32, device=dev)
    n = len(level_hw)
    st = (C.c_int32 * n)(*[int(s) for s in strides])
    lo = (C.c_int32 * n)(*[int(r[0]) for r in ranges])
    hi = (C.c_int32 * n)(*[int(r[1]) for r in ranges])
    gb = gt_boxes.contiguous().float()
    lb = labels.contiguous().to(torch.int64)
    check(_lib.lib().fd_fcos_gen_targets(gb.data_ptr(), lb.data_ptr(), M, C.byref(segs), st, lo, hi, radius, cls.data_ptr(),
                                         cnt.data_ptr(), reg.data_ptr(), _stream()), "fd_fcos_gen_targets")
    return cls, cnt, reg


ATSS_MAX_TOPK = 16      # include/fcosdet.h FD_ATSS_MAX_TOPK


def atss_gen_targets(gt_boxes: torch.Tensor, labels: torch.Tensor, level_hw, strides, topk: int = 9, anchor_scale: float = 8.0,
                     inside_eps: float = 0.01, return_stats: bool = False):
    """ATSS assignment (fd_atss_gen_targets) on the contract of fcos_gen_targets: gt_boxes [B,M,4] f32, labels [B,M]
    int64 (M may be 0) -> (cls [B,L,1] int64, cnt [B,L,1] f32, reg [B,L,4] f32); with return_stats also thr [B,M] f64 (mean + std
    of a row's candidate IoUs, NaN for padding) and npos [B,M] int32 (its positives before locations are contested)."""
    _need_gpu(gt_boxes, labels)
    B, M = labels.shape
    if len(strides) != len(level_hw) or tuple(gt_boxes.shape) != (B, M, 4):
        raise FdError(f"atss_gen_targets: {len(level_hw)} levels, {len(strides)} strides, gt_boxes {tuple(gt_boxes.shape)}, labels {tuple(labels.shape)}")
    segs = Segs.make(B, list(level_hw))
    L = sum(h * w for h, w in level_hw)
    dev = gt_boxes.device
    cls = torch.empty(B, L, 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(B, L, 1, dtype=torch.float32, device=dev)
    reg = torch.empty(B, L, 4, dtype=torch.float32, device=dev)
    thr =torch.empty(B, M, dtype=torch.float64, device=dev) if return_stats else None
    npos = torch.empty(B, M, dtype=torch.int32, device=dev) if return_stats else None
    ws = torch.empty(max(_lib.lib().fd_atss_workspace_bytes(B, L), 0) // 8, dtype=torch.int64, device=dev)
    n = len(level_hw)
    st = (C.c_int32 * n)(*[int(s) for s in strides])
    gb = gt_boxes.contiguous().float()
    lb = labels.contiguous().to(torch.int64)
    check(_lib.lib().fd_atss_gen_targets(gb.data_ptr() if M else None, lb.data_ptr() if M else None, M, C.byref(segs), st, int(topk),
                                         float(anchor_scale), float(inside_eps), cls.data_ptr(), cnt.data_ptr(), reg.data_ptr(),
                                         thr.data_ptr() if return_stats and M else None, npos.data_ptr() if return_stats and M else None,
                                         ws.data_ptr(), _stream()), "fd_atss_gen_targets")
    return (cls, cnt, reg, thr, npos) if return_stats else (cls, cnt, reg)


SIMOTA_MAX_TOPQ, SIMOTA_MAX_GT = 16, 256      # include/fcosdet.h FD_SIMOTA_MAX_TOPQ, FD_SIMOTA_MAX_GT
SIMOTA_QUALITY = {"centerness": 0, "iou": 1}


def simota_gen_targets(cls_logits: torch.Tensor, cnt_logits: torch.Tensor, reg_pred: torch.Tensor, gt_boxes: torch.Tensor,
                       labels: torch.Tensor, level_hw, strides, top_q: int = 10, centre_radius: float = 2.5, iou_weight: float = 3.0,
                       inside_eps: float = 0.01, quality: str = "centerness", return_stats: bool = False):
    """SimOTA assignment (fd_simota_gen_targets) on the contract of fcos_gen_targets, ranked by the current
    predictions: cls_logits [B,L,C], cnt_logits [B,L] or [B,L,1], reg_pred [B,L,4] (l, t, r, b in pixels), all f32 in the location
    order of level_hw; gt_boxes [B,M,4] f32, labels [B,M] int64 in 1..C (M may be 0) -> (cls [B,L,1] int64, cnt [B,L,1] f32,
    reg [B,L,4] f32).  quality: "centerness" (cnt as fcos_gen_targets) or "iou" (cnt = the predicted box's IoU).  With
    return_stats also pair_iou, pair_cost [B,M,L] f32 (0 / +inf for non-candidates), k and ncand [B,M] int32."""
    _need_gpu(cls_logits, cnt_logits, reg_pred, gt_boxes, labels)
    B, M = labels.shape
    L = sum(h * w for h, w in level_hw)
    if quality not in SIMOTA_QUALITY:
        raise FdError(f"simota_gen_targets: quality must be one of {sorted(SIMOTA_QUALITY)} (got {quality!r})")
    if (len(strides) != len(level_hw) or tuple(gt_boxes.shape) != (B, M, 4) or cls_logits.dim() != 3 or tuple(cls_logits.shape[:2]) != (B, L)
            or cnt_logits.numel() != B * L or tuple(reg_pred.shape) != (B, L, 4)):
        raise FdError(f"simota_gen_targets: {len(level_hw)} levels of {L} locations, {len(strides)} strides, cls_logits {tuple(cls_logits.shape)}, "
                      f"cnt_logits {tuple(cnt_logits.shape)}, reg_pred {tuple(reg_pred.shape)}, gt_boxes {tuple(gt_boxes.shape)}, labels {tuple(labels.shape)}")
    for t in (cls_logits, cnt_logits, reg_pred):
        if t.dtype != torch.float32:
            raise FdError(f"simota_gen_targets: predictions must be float32 (got {t.dtype})")
    Cn = int(cls_logits.shape[2])
    segs = Segs.make(B, list(level_hw))
    dev = gt_boxes.device
    cls = torch.empty(B, L, 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(B, L, 1, dtype=torch.float32, device=dev)
    reg = torch.empty(B, L, 4, dtype=torch.float32, device=dev)
    stats = None
    if return_stats:
        stats = (torch.empty(B, M, L, dtype=torch.float32, device=dev), torch.empty(B, M, L, dtype=torch.float32, device=dev),
                 torch.empty(B, M, dtype=torch.int32, device=dev), torch.empty(B, M, dtype=torch.int32, device=dev))
    ws = torch.empty(max(_lib.lib().fd_simota_workspace_bytes(B, M, L), 8) // 8, dtype=torch.int64, device=dev)
    n = len(level_hw)
    st = (C.c_int32 * n)(*[int(s) for s in strides])
    cl, cn, rp = cls_logits.detach().contiguous(), cnt_logits.detach().contiguous(), reg_pred.detach().contiguous()
    gb = gt_boxes.contiguous().float()
    lb = labels.contiguous().to(torch.int64)
    sp = [t.data_ptr() if M else None for t in stats] if return_stats else [None] * 4
    check(_lib.lib().fd_simota_gen_targets(cl.data_ptr(), cn.data_ptr(), rp.data_ptr(), Cn, gb.data_ptr() if M else None,
                                           lb.data_ptr() if M else None, M, C.byref(segs), st, int(top_q), float(centre_radius),
                                           float(iou_weight), float(inside_eps), SIMOTA_QUALITY[quality], cls.data_ptr(), cnt.data_ptr(),
                                           reg.data_ptr(), sp[0], sp[1], sp[2], sp[3], ws.data_ptr(), _stream()), "fd_simota_gen_targets")
    return (cls, cnt, reg) + stats if return_stats else (cls, cnt, reg)


# ---------------------------------------------------------------------------------------------------- anchors (DataEncoder)
ANCHOR_LEVELS, ANCHOR_PER_CELL = 5, 9


def anchor_params(input_size, anchor_wh) -> _lib.AnchorParams:
    """fd_anchor_params of one input size: `input_size` an int or (w, h); `anchor_wh` [5, 9, 2] (w, h) pairs, rounded here to
    fp32.  fm = ceil(input / 2^(level + 3)) and grid = input / fm in fp32, the reference's tensors (utills.py:121-130)."""
    wh = np.asarray(anchor_wh.detach().cpu().numpy() if isinstance(anchor_wh, torch.Tensor) else anchor_wh, dtype=np.float64).astype(np.float32)
    if wh.shape != (ANCHOR_LEVELS, ANCHOR_PER_CELL, 2) or not np.isfinite(wh).all() or not (wh > 0).all():
        raise FdError(f"anchor_params: anchor_wh must be [5, 9, 2], finite and > 0 (got shape {wh.shape})")
    if isinstance(input_size, torch.Tensor):
        input_size = input_size.tolist()
    size = np.array([input_size, input_size] if isinstance(input_size, (int, float)) else list(input_size), dtype=np.float32)
    if size.shape != (2,) or not np.isfinite(size).all() or not (size >= 1).all():
        raise FdError(f"anchor_params: input_size must be an int or (w, h) with sides >= 1 (got {input_size!r})")
    p = _lib.AnchorParams()
    total = 0
    for i in range(ANCHOR_LEVELS):
        fm = np.ceil(size / np.float32(2.0 ** (i + 3)))
        grid = size / fm
        p.fm_w[i], p.fm_h[i] = int(fm[0]), int(fm[1])
        p.grid_w[i], p.grid_h[i] = float(grid[0]), float(grid[1])
        for k in range(ANCHOR_PER_CELL):
            p.wh[i][k][0], p.wh[i][k][1] = float(wh[i, k, 0]), float(wh[i, k, 1])
        total += ANCHOR_PER_CELL * int(fm[0]) * int(fm[1])
    if total >= 1 << 28:
        raise FdError(f"anchor_params: {total} anchors (limit 2^28)")
    p.num_anchors = total
    return p


def _need_f32(what: str, **ts) -> None:
    for name, t in ts.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
            raise FdError(f"{what}: {name} must be a contiguous fp32 tensor")


def anchor_boxes(params: _lib.AnchorParams, device) -> torch.Tensor:
    """-> anchors [A, 4] fp32 (cx, cy, w, h), DataEncoder._get_anchor_boxes bit for bit."""
    device = torch.device(device)
    if device.type != "cuda":
        raise FdError("anchor_boxes runs on the GPU only; there is no CPU fallback")
    out = torch.empty(params.num_anchors, 4, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(_lib.lib().fd_anchor_boxes(C.byref(params), out.data_ptr(), params.num_anchors, _stream()), "fd_anchor_boxes")
    return out


def anchor_encode(params: _lib.AnchorParams, gt_boxes: torch.Tensor, labels: torch.Tensor):
    """gt_boxes [B, M, 4] fp32 xyxy, labels [B, M] int64 (< 0 = padding) -> (loc [B, A, 4] fp32, cls [B, A] int64): fd_anchor_encode."""
    _need_gpu(gt_boxes, labels)
    _need_f32("anchor_encode", gt_boxes=gt_boxes)
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or not labels.is_contiguous():
        raise FdError("anchor_encode: labels must be a contiguous int64 tensor")
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or tuple(labels.shape) != tuple(gt_boxes.shape[:2]) or gt_boxes.shape[0] < 1:
        raise FdError(f"anchor_encode: gt_boxes {tuple(gt_boxes.shape)} / labels {tuple(labels.shape)} must be [B, M, 4] / [B, M] with B >= 1")
    B, M = labels.shape
    A = params.num_anchors
    loc = torch.empty(B, A, 4, dtype=torch.float32, device=gt_boxes.device)
    cls = torch.empty(B, A, dtype=torch.int64, device=gt_boxes.device)
    check(_lib.lib().fd_anchor_encode(C.byref(params), gt_boxes.data_ptr() if M else None, labels.data_ptr() if M else None, B, M, A,
                                      loc.data_ptr(), cls.data_ptr(), _stream()), "fd_anchor_encode")
    return loc, cls


def anchor_decode(params: _lib.AnchorParams, loc: torch.Tensor, cls: torch.Tensor, cls_thresh: float = 0.5, nms_thresh: float = 0.5,
                  max_candidates: int = 1000):
    """loc [B, A, 4] fp32, cls [B, A, C] fp32 logits -> (boxes [B, K, 4], labels [B, K] int64 (-1 = padding), scores [B, K], counts [B] int32,
    n_candidates [B] int32), K = min(max_candidates, A): fd_anchor_decode.  n_candidates[b] > K: image b was cut to its K best candidates."""
    _need_gpu(loc, cls)
    _need_f32("anchor_decode", loc=loc, cls=cls)
    A = params.num_anchors
    if loc.dim() != 3 or cls.dim() != 3 or tuple(loc.shape[1:]) != (A, 4) or tuple(cls.shape[:2]) != tuple(loc.shape[:2]) or loc.shape[0] < 1:
        raise FdError(f"anchor_decode: loc {tuple(loc.shape)} / cls {tuple(cls.shape)} must be [B, {A}, 4] / [B, {A}, C] with B >= 1")
    B, _, Cn = cls.shape
    need = _lib.lib().fd_anchor_decode_workspace_bytes(B, A, int(max_candidates))
    if need < 0:
        raise FdError(f"anchor_decode: unsupported B={B} A={A} max_candidates={max_candidates} (1 <= max_candidates <= {_lib.ANCHOR_MAX_CAND})",
                      rc=_lib.E_UNSUPPORTED)
    K = min(int(max_candidates), A)
    dev = loc.device
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    boxes = torch.empty(B, K, 4, dtype=torch.float32, device=dev)
    labels = torch.empty(B, K, dtype=torch.int64, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    n_cand = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.lib().fd_anchor_decode(C.byref(params), loc.data_ptr(), cls.data_ptr(), B, A, Cn, float(cls_thresh), float(nms_thresh),
                                      int(max_candidates), boxes.data_ptr(), labels.data_ptr(), scores.data_ptr(), counts.data_ptr(),
                                      n_cand.data_ptr(), ws.data_ptr(), _stream()), "fd_anchor_decode")
    return boxes, labels, scores, counts, n_cand


EVAL_INPUT_ORDER = 1    # include/fcosdet.h FD_EVAL_INPUT_ORDER: match each image's detections in row order (eval_ap_2d) instead of score order


def eval_ap_bytes(n_thr: int, num_cls: int) -> int:
    """Size of the packed result buffer of eval_ap: ap [T, C] f64, n_gt [C], n_pred [C], n_tp [T, C] int32."""
    return n_thr * num_cls * 8 + 2 * num_cls * 4 + n_thr * num_cls * 4


def eval_ap_views(buf: torch.Tensor, n_thr: int, num_cls: int):
    """(ap, n_gt, n_pred, n_tp) views of a packed uint8 result buffer (device or host copy alike)."""
    T, Cn = n_thr, num_cls
    a = T * Cn * 8
    ap = buf[:a].view(torch.float64).view(T, Cn)
    n_gt = buf[a:a + 4 * Cn].view(torch.int32)
    n_pred = buf[a + 4 * Cn:a + 8 * Cn].view(torch.int32)
    n_tp = buf[a + 8 * Cn:a + 8 * Cn + 4 * T * Cn].view(torch.int32).view(T, Cn)
    return ap, n_gt, n_pred, n_tp


def eval_ap(scores: torch.Tensor, classes: torch.Tensor, boxes: torch.Tensor, det_counts: Optional[torch.Tensor],
            gt_boxes: torch.Tensor, gt_classes: torch.Tensor, gt_counts: Optional[torch.Tensor], num_cls: int,
            thresholds: Sequence[float], flags: int = 0, out: Optional[torch.Tensor] = None):
    """VOC AP of the reference's eval_ap_2d (fd_eval_ap, include/fcosdet.h) on the current stream.
    scores [N,K] f32, classes [N,K] int64, boxes [N,K,4] f32, det_counts [N] int32 or None; gt_boxes [N,G,4] f32, gt_classes [N,G]
    int64, gt_counts [N] int32 or None.  -> (ap [T, num_cls] f64, n_gt [num_cls], n_pred [num_cls], n_tp [T, num_cls] int32), views of
    `out` (uint8, eval_ap_bytes(T, num_cls), allocated when None); column 0 (background) is 0."""
    _need_gpu(scores, classes, boxes, det_counts, gt_boxes, gt_classes, gt_counts)
    N, K = scores.shape
    G = gt_classes.shape[1]
    if tuple(classes.shape) != (N, K) or tuple(boxes.shape) != (N, K, 4) or tuple(gt_boxes.shape) != (N, G, 4) or gt_classes.shape[0] != N:
        raise FdError(f"eval_ap: shapes scores {tuple(scores.shape)} classes {tuple(classes.shape)} boxes {tuple(boxes.shape)} "
                      f"gt_boxes {tuple(gt_boxes.shape)} gt_classes {tuple(gt_classes.shape)} do not agree")
    if (scores.dtype != torch.float32 or classes.dtype != torch.int64 or boxes.dtype != torch.float32 or gt_boxes.dtype != torch.float32
            or gt_classes.dtype != torch.int64):
        raise FdError("eval_ap: scores / boxes must be fp32, classes int64")
    for t in (scores, classes, boxes, gt_boxes, gt_classes, det_counts, gt_counts):
        if t is not None and not t.is_contiguous():
            raise FdError("eval_ap: inputs must be contiguous")
    for t in (det_counts, gt_counts):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (N,)):
            raise FdError("eval_ap: counts must be int32 [N]")
    T = len(thresholds)
    dev = scores.device
    need = _lib.lib().fd_eval_ap_workspace_bytes(N, K, G, num_cls, T)
    if need < 0:
        check(_lib.lib().fd_eval_ap(None, None, None, None, N, K, None, None, None, G, num_cls, None, T, flags, None, None, None, None,
                                    None, None), "fd_eval_ap")
    # workspace per call (~25 bytes per detection row): evaluation runs once per epoch, so it is not kept in a module cache; it goes
    # back to torch's caching allocator when the call's kernels are enqueued (torch.cuda.empty_cache() can then release it)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    if out is None:
        out = torch.empty(eval_ap_bytes(T, num_cls), dtype=torch.uint8, device=dev)
    ap, n_gt, n_pred, n_tp = eval_ap_views(out, T, num_cls)
    thr = (C.c_float * T)(*[float(t) for t in thresholds])
    check(_lib.lib().fd_eval_ap(scores.data_ptr(), classes.data_ptr(), boxes.data_ptr(),
                                det_counts.data_ptr() if det_counts is not None else None, N, K, gt_boxes.data_ptr(), gt_classes.data_ptr(),
                                gt_counts.data_ptr() if gt_counts is not None else None, G, num_cls, thr, T, int(flags), ap.data_ptr(),
                                n_gt.data_ptr(), n_pred.data_ptr(), n_tp.data_ptr(), ws.data_ptr(), _stream()), "fd_eval_ap")
    return ap, n_gt, n_pred, n_tp


COCO_IOU_THRS = tuple(float(t) for t in np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True))    # COCOeval Params
COCO_REC_THRS = tuple(float(r) for r in np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True))
COCO_AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
COCO_MAX_DETS = (1, 10, 100)


def eval_coco(scores: torch.Tensor, labels: torch.Tensor, boxes: torch.Tensor, det_counts: Optional[torch.Tensor], gt_boxes: torch.Tensor,
              gt_area: torch.Tensor, gt_crowd: torch.Tensor, gt_labels: torch.Tensor, num_cats: int, image_order: Optional[torch.Tensor] = None,
              iou_thrs: Sequence[float] = COCO_IOU_THRS, rec_thrs: Sequence[float] = COCO_REC_THRS,
              area_rng: Sequence[Sequence[float]] = COCO_AREA_RNG, max_dets: Sequence[int] = COCO_MAX_DETS):
    """COCOeval bbox evaluate + accumulate (fd_eval_coco, include/fcosdet.h) on the current stream.
    scores [N,K] f32, labels [N,K] int64 (1 .. num_cats), boxes [N,K,4] f32 xywh, det_counts [N] int32 or None; gt_boxes [N,G,4] f64 xywh,
    gt_area [N,G] f64, gt_crowd [N,G] uint8, gt_labels [N,G] int64 (-1 = padding); image_order [N] int32 or None.
    -> (precision [T,R,num_cats,A,M] f64, recall [T,num_cats,A,M] f64, n_gt [num_cats,A] int32), device tensors."""
    _need_gpu(scores, labels, boxes, det_counts, gt_boxes, gt_area, gt_crowd, gt_labels, image_order)
    N, K = scores.shape
    G = gt_labels.shape[1]
    if (tuple(labels.shape) != (N, K) or tuple(boxes.shape) != (N, K, 4) or tuple(gt_boxes.shape) != (N, G, 4)
            or tuple(gt_area.shape) != (N, G) or tuple(gt_crowd.shape) != (N, G) or gt_labels.shape[0] != N):
        raise FdError("eval_coco: shapes of the detection / GT tensors do not agree")
    if (scores.dtype != torch.float32 or labels.dtype != torch.int64 or boxes.dtype != torch.float32 or gt_boxes.dtype != torch.float64
            or gt_area.dtype != torch.float64 or gt_crowd.dtype != torch.uint8 or gt_labels.dtype != torch.int64):
        raise FdError("eval_coco: scores / boxes f32, GT boxes / area f64, iscrowd uint8, labels int64")
    for t in (scores, labels, boxes, det_counts, gt_boxes, gt_area, gt_crowd, gt_labels, image_order):
        if t is not None and not t.is_contiguous():
            raise FdError("eval_coco: inputs must be contiguous")
    for t in (det_counts, image_order):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (N,)):
            raise FdError("eval_coco: det_counts / image_order must be int32 [N]")
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rng), len(max_dets)
    dev = scores.device
    L = _lib.lib()
    need = L.fd_eval_coco_workspace_bytes(N, K, G, int(num_cats))
    if need < 0:
        check(L.fd_eval_coco(None, None, None, None, N, K, None, None, None, None, G, None, int(num_cats), None, T, None, R, None, A, None, M,
                             None, None, None, None, None), "fd_eval_coco")
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)      # per call, as eval_ap's
    precision = torch.empty((T, R, int(num_cats), A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, int(num_cats), A, M), dtype=torch.float64, device=dev)
    n_gt = torch.empty((int(num_cats), A), dtype=torch.int32, device=dev)
    thr = (C.c_double * T)(*[float(t) for t in iou_thrs])
    rec = (C.c_double * R)(*[float(r) for r in rec_thrs])
    ar = (C.c_double * (2 * A))(*[float(v) for rng in area_rng for v in rng])
    md = (C.c_int32 * M)(*[int(m) for m in max_dets])
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    check(L.fd_eval_coco(ptr(scores), ptr(labels), ptr(boxes), ptr(det_counts), N, K, ptr(gt_boxes), ptr(gt_area), ptr(gt_crowd), ptr(gt_labels),
                         G, ptr(image_order), int(num_cats), thr, T, rec, R, ar, A, md, M, precision.data_ptr(), recall.data_ptr(),
                         n_gt.data_ptr(), ws.data_ptr(), _stream()), "fd_eval_coco")
    return precision, recall, n_gt


def optim_begin(state: torch.Tensor, found_inf: Optional[torch.Tensor], params: _lib.OptimBeginParams) -> None:
    """fd_optim_begin on the optimizer's state block (optim.py): counters, skip flag, the step's rates, Adam's bias corrections.  One launch."""
    _need_gpu(state, found_inf)
    if state.dtype != torch.float64 or not state.is_contiguous() or state.numel() * 8 < C.sizeof(_lib.OptimState):
        raise FdError("optim_begin: state must be the optimizer's contiguous float64 block")
    if found_inf is not None and (found_inf.dtype != torch.float32 or found_inf.numel() != 1 or found_inf.device != state.device):
        raise FdError("optim_begin: found_inf must be one fp32 element on the optimizer's device")
    check(_lib.lib().fd_optim_begin(state.data_ptr(), _dptr(found_inf), C.byref(params), _stream()), "fd_optim_begin")


def optim_update(adam: bool, p: Sequence[int], g: Sequence[int], s0: Optional[Sequence[int]], s1: Optional[Sequence[int]], numel: Sequence[int],
                 hyper: _lib.OptimHyper, state: torch.Tensor, grad_scale: Optional[torch.Tensor]) -> int:
    """fd_optim_sgd_f32 / fd_optim_adam_f32 over a list of tensors given as device addresses (s0 / s1: None when the rule has no such state), in chunks of
    _lib.OPTIM_MAX_TENSORS whose pointers travel by value in the kernel arguments.  The caller read every address from the live tensors just now: nothing
    here is kept across calls.  -> launches enqueued."""
    _need_gpu(state, grad_scale)
    if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != state.device):
        raise FdError("optim_update: grad_scale must be one fp32 element on the optimizer's device")
    fn = _lib.lib().fd_optim_adam_f32 if adam else _lib.lib().fd_optim_sgd_f32
    what = "fd_optim_adam_f32" if adam else "fd_optim_sgd_f32"
    cap, total, launches = _lib.OPTIM_MAX_TENSORS, len(p), 0
    st, gs = state.data_ptr(), _dptr(grad_scale)
    for lo in range(0, total, cap):
        n = min(cap, total - lo)
        c = _lib.OptimChunk()
        c.n = n
        c.p[:n], c.g[:n], c.numel[:n] = p[lo:lo + n], g[lo:lo + n], numel[lo:lo + n]
        if s0 is not None:
            c.s0[:n] = s0[lo:lo + n]
        if s1 is not None:
            c.s1[:n] = s1[lo:lo + n]
        check(fn(C.byref(c), C.byref(hyper), st, gs, _stream()), what)
        launches += 1
    return launches


def grad_sumsq(g: Sequence[int], numel: Sequence[int], partials: torch.Tensor) -> Tuple[int, int]:
    """fd_grad_sumsq_f32 over a list of gradients given as device addresses, in chunks of _lib.OPTIM_MAX_TENSORS whose pointers travel by value in the kernel
    arguments: every block stores one fp64 partial into its own slot of `partials` (the optimizer's workspace, fd_grad_norm_workspace_bytes), the chunks'
    slots one after the other from slot 0.  Nothing is kept across calls.  -> (launches enqueued, slots written)."""
    _need_gpu(partials)
    if partials.dtype != torch.float64 or not partials.is_contiguous():
        raise FdError("grad_sumsq: partials must be the optimizer's contiguous float64 workspace")
    L = _lib.lib()
    cap, total, launches, slot = _lib.OPTIM_MAX_TENSORS, len(g), 0, 0
    ws = partials.data_ptr()
    for lo in range(0, total, cap):
        n = min(cap, total - lo)
        c = _lib.GradChunk()
        c.n = n
        c.g[:n], c.numel[:n] = g[lo:lo + n], numel[lo:lo + n]
        slots = L.fd_grad_sumsq_slots(C.byref(c))
        if slots >= 0 and slot + slots > partials.numel():
            raise FdError(f"grad_sumsq: the workspace holds {partials.numel()} slots, the launches need at least {slot + slots}")
        check(L.fd_grad_sumsq_f32(C.byref(c), ws, slot, _stream()), "fd_grad_sumsq_f32")         # (slots < 0: the same check refuses the chunk here, with its message)
        launches += 1
        slot += slots
    return launches, slot


def grad_clip_finish(partials: torch.Tensor, n_slots: int, grad_scale: Optional[torch.Tensor], found_inf: Optional[torch.Tensor], max_norm: float,
                     clip: torch.Tensor) -> None:
    """fd_grad_clip_finish: the slots partials[:n_slots] added in index order, then norm, clip coefficient, effective scale and found flag into the
    optimizer's clip block (fd_grad_clip, a contiguous float64 tensor of its size).  One launch."""
    _need_gpu(partials, clip, grad_scale, found_inf)
    if partials.dtype != torch.float64 or not partials.is_contiguous() or not 0 <= int(n_slots) <= partials.numel():
        raise FdError(f"grad_clip_finish: n_slots = {n_slots} slots of the optimizer's contiguous float64 workspace ({partials.numel()} slots)")
    if clip.dtype != torch.float64 or not clip.is_contiguous() or clip.numel() * 8 < C.sizeof(_lib.GradClip) or clip.device != partials.device:
        raise FdError("grad_clip_finish: clip must be the optimizer's contiguous float64 clip block")
    for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != clip.device):
            raise FdError(f"grad_clip_finish: {name} must be one fp32 element on the optimizer's device")
    check(_lib.lib().fd_grad_clip_finish(partials.data_ptr(), int(n_slots), _dptr(grad_scale), _dptr(found_inf), float(max_norm), clip.data_ptr(), _stream()),
          "fd_grad_clip_finish")


def avg_begin(state: torch.Tensor, n_averaged: torch.Tensor, skip: Optional[torch.Tensor], global_step: Optional[torch.Tensor],
              params: _lib.AvgBeginParams) -> None:
    """fd_avg_begin on the averager's state block (optim.AveragedModel): the gate (skip / global_step: 0-dim int64 views of an optimizer's state block, or
    None), this call's blend factor, n_averaged += 1 when it applies.  One launch."""
    _need_gpu(state, n_averaged, skip, global_step)
    if state.dtype != torch.float64 or not state.is_contiguous() or state.numel() * 8 < C.sizeof(_lib.AvgState):
        raise FdError("avg_begin: state must be the averager's contiguous float64 block")
    for name, t in (("n_averaged", n_averaged), ("skip", skip), ("global_step", global_step)):
        if t is not None and (t.dtype != torch.int64 or t.numel() != 1 or t.device != state.device):
            raise FdError(f"avg_begin: {name} must be one int64 element on the averager's device ({state.device})")
    check(_lib.lib().fd_avg_begin(state.data_ptr(), n_averaged.data_ptr(), _dptr(skip), _dptr(global_step), C.byref(params), _stream()), "fd_avg_begin")


def avg_update(avg: Sequence[int], p: Sequence[int], numel: Sequence[int], state: torch.Tensor) -> int:
    """fd_avg_update_f32 over a list of (averaged copy, model tensor) pairs given as device addresses, in chunks of _lib.OPTIM_MAX_TENSORS whose pointers
    travel by value in the kernel arguments.  Nothing is kept across calls.  -> launches enqueued."""
    _need_gpu(state)
    fn, st = _lib.lib().fd_avg_update_f32, state.data_ptr()
    cap, total, launches = _lib.OPTIM_MAX_TENSORS, len(avg), 0
    for lo in range(0, total, cap):
        n = min(cap, total - lo)
        c = _lib.AvgChunk()
        c.n = n
        c.avg[:n], c.p[:n], c.numel[:n] = avg[lo:lo + n], p[lo:lo + n], numel[lo:lo + n]
        check(fn(C.byref(c), st, _stream()), "fd_avg_update_f32")
        launches += 1
    return launches


def avg_copy(dst: Sequence[int], src: Sequence[int], nbytes: Sequence[int], state: torch.Tensor) -> int:
    """fd_avg_copy_bytes over a list of (destination, source) buffers given as device addresses and byte counts, chunked like avg_update and gated by the
    same state block.  -> launches enqueued."""
    _need_gpu(state)
    fn, st = _lib.lib().fd_avg_copy_bytes, state.data_ptr()
    cap, total, launches = _lib.OPTIM_MAX_TENSORS, len(dst), 0
    for lo in range(0, total, cap):
        n = min(cap, total - lo)
        c = _lib.AvgCopyChunk()
        c.n = n
        c.dst[:n], c.src[:n], c.nbytes[:n] = dst[lo:lo + n], src[lo:lo + n], nbytes[lo:lo + n]
        check(fn(C.byref(c), st, _stream()), "fd_avg_copy_bytes")
        launches += 1
    return launches


# ------------------------------------------------------------------------------ baseline JPEG decoding
def _jpeg_stream(data) -> np.ndarray:
    """bytes / bytearray / memoryview / uint8 array -> contiguous uint8 array over the same memory where possible."""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise FdError("jpeg: a stream given as an array must be one-dimensional uint8")
        return np.ascontiguousarray(data)
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    raise FdError(f"jpeg: a stream must be bytes or a uint8 array, not {type(data).__name__}")


def jpeg_error(rc: int, what: str) -> FdError:
    return FdError(f"{what} failed ({rc}): {_lib.JPEG_ERRORS.get(int(rc), 'unknown error')}", rc=int(rc))


def jpeg_parse(data) -> _lib.JpegInfo:
    """fd_jpeg_parse: the headers of one JPEG stream up to SOS (host only).  -> JpegInfo; info.supported == 0 with info.reason (_lib.JPEG_R_*) for a
    well-formed stream the decoder does not take.  A stream that is not well formed raises FdError with rc = _lib.JPEG_E_*."""
    buf = _jpeg_stream(data)
    info = _lib.JpegInfo()
    rc = _lib.lib().fd_jpeg_parse(buf.ctypes.data, buf.size, C.byref(info))
    if rc != 0:
        raise jpeg_error(rc, "fd_jpeg_parse")
    return info


def jpeg_entropy_decode(data, info: _lib.JpegInfo, out: Optional[np.ndarray] = None) -> np.ndarray:
    """fd_jpeg_entropy_decode: the scan of a parsed, supported stream -> dense quantised coefficients, int16 [info.coef_bytes / 2] (component after component,
    [bh][bw][64] in natural order).  out: a writable contiguous int16 array of at least that many elements (a slice of a staging buffer); the ctypes call
    releases the GIL, so several threads may decode different streams at once.  Host only."""
    buf = _jpeg_stream(data)
    elems = int(info.coef_bytes) // 2
    if out is None:
        out = np.empty(elems, np.int16)
    elif not isinstance(out, np.ndarray) or out.dtype != np.int16 or out.ndim != 1 or not out.flags.c_contiguous or not out.flags.writeable or out.size < elems:
        raise FdError("jpeg_entropy_decode: out must be a writable contiguous int16 array of at least info.coef_bytes / 2 elements")
    rc = _lib.lib().fd_jpeg_entropy_decode(buf.ctypes.data, buf.size, C.byref(info), out.ctypes.data, out.size * 2)
    if rc != 0:
        raise jpeg_error(rc, "fd_jpeg_entropy_decode")
    return out[:elems]


def _jpeg_jobs(who: str, jobs_host, cls, jobs_dev: torch.Tensor) -> int:
    if not isinstance(jobs_host, C.Array) or jobs_host._type_ is not cls or len(jobs_host) < 1:
        raise FdError(f"{who}: jobs_host must be a non-empty ctypes array of {cls.__name__}")
    n = len(jobs_host)
    if jobs_dev.dtype != torch.uint8 or not jobs_dev.is_contiguous() or jobs_dev.numel() < n * C.sizeof(cls):
        raise FdError(f"{who}: jobs_dev must be a contiguous CUDA uint8 tensor holding the {n} job records")
    return n


def jpeg_idct_u8(jobs_host, jobs_dev: torch.Tensor, coefs: torch.Tensor, qtabs: torch.Tensor, planes: torch.Tensor) -> None:
    """fd_jpeg_idct_u8: dequantise + jpeg_idct_islow for every (image, component) job in ONE launch.  jobs_host: ctypes array of _lib.JpegIdctJob (validated
    before the launch); jobs_dev: the same bytes on the device (uint8); coefs: CUDA int16 [elements]; qtabs: CUDA int16 [n, 64] (the uint16 tables' bits);
    planes: CUDA uint8 [bytes], written at each job's plane_off as [8 * bh][8 * bw].  Does not synchronise."""
    _need_gpu(jobs_dev, coefs, qtabs, planes)
    n = _jpeg_jobs("jpeg_idct_u8", jobs_host, _lib.JpegIdctJob, jobs_dev)
    if coefs.dtype != torch.int16 or not coefs.is_contiguous() or qtabs.dtype != torch.int16 or not qtabs.is_contiguous() or qtabs.dim() != 2 or qtabs.shape[1] != 64:
        raise FdError("jpeg_idct_u8: coefs must be contiguous int16 and qtabs contiguous int16 [n, 64]")
    if planes.dtype != torch.uint8 or not planes.is_contiguous():
        raise FdError("jpeg_idct_u8: planes must be a contiguous uint8 tensor")
    check(_lib.lib().fd_jpeg_idct_u8(C.addressof(jobs_host), jobs_dev.data_ptr(), n, coefs.data_ptr(), coefs.numel(), qtabs.data_ptr(), int(qtabs.shape[0]),
                                     planes.data_ptr(), planes.numel(), _stream()), "fd_jpeg_idct_u8")


def jpeg_color_u8(jobs_host, jobs_dev: torch.Tensor, planes: torch.Tensor) -> None:
    """fd_jpeg_color_u8: chroma upsampling + YCbCr -> RGB for every image job in ONE launch, each into its job's `out` (CUDA uint8 [h, w, 3], kept alive by the
    caller).  jobs_host: ctypes array of _lib.JpegColorJob; jobs_dev: the same bytes on the device; planes: what jpeg_idct_u8 wrote.  Does not synchronise."""
    _need_gpu(jobs_dev, planes)
    n = _jpeg_jobs("jpeg_color_u8", jobs_host, _lib.JpegColorJob, jobs_dev)
    if planes.dtype != torch.uint8 or not planes.is_contiguous():
        raise FdError("jpeg_color_u8: planes must be a contiguous uint8 tensor")
    check(_lib.lib().fd_jpeg_color_u8(C.addressof(jobs_host), jobs_dev.data_ptr(), n, planes.data_ptr(), planes.numel(), _stream()), "fd_jpeg_color_u8")
