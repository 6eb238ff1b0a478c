"""Autograd bindings of the HIP kernels for the training forward (reference train.py:175-181).

Everything here works on the library's own layout: NHWC rows, i.e. 2-D tensors [rows, C] described by a segment table
(`Segs`: one segment per pyramid level).  An NCHW-shaped channels-last tensor IS such a buffer (zero-copy view), and the
five FCOS levels concatenated along the row axis are one buffer too, so a shared-weight head runs one launch per layer
over the whole pyramid exactly as at inference.

  conv_rows / conv_bn_act   Conv2d -> frozen BatchNorm2d -> (+ residual) -> ReLU as ONE launch of fd_conv2d_nhwc_f32
                            (BN folded into the epilogue).  Backward: ReLU mask on the incoming gradient (one
                            elementwise pass from the saved output), data gradient = the same conv kernel on dY with
                            flipped / transposed weights (stride-1 layers), weight gradient = fd_conv2d_bwd_weight_f32.
  dw_rows                   depthwise 3x3: fd_dwconv3x3_nhwc forward and data gradient, fd_dwconv3x3_bwd_weight_nhwc.
  dw_kxk_rows               strided depthwise k x k with asymmetric padding (MBConv): fd_dwconv2d_nhwc forward, fd_dwconv2d_bwd_data_nhwc /
                            fd_dwconv2d_bwd_weight_nhwc backward; mbconv_rows = the whole MBConv block on maps held at widths rounded up to 32.
  dw_dilated_rows           dilated depthwise k x k (MNBlock): fd_dwconv_dilated_nhwc forward and data gradient, fd_dwconv_dilated_bwd_weight_nhwc;
                            mn_block_rows = the whole MNBlock (depthwise, BatchNorm frozen or on batch statistics, PW1 + SiLU, PW2 + residual).
  deform_conv_rows          modulated deformable conv (DeformableConv2d): the sampler node fd_deform_im2col_nhwc / fd_deform_bwd_nhwc writes the columns,
                            conv_rows' node is the GEMM over them; deformable_conv2d = the layer with its two side convs as one launch.
  groupnorm_rows            GroupNorm + ReLU / SiLU: fd_groupnorm_act_nhwc / fd_groupnorm_act_bwd_nhwc.
  stem_rows                 the trainable 7x7 stem (Cin = 3), opt-in (trunk.hip_stem_train): fd_stem7x7_nhwc4 forward, fd_stem7x7_bwd_weight_nhwc4 backward.
  batchnorm_train_res_rows  act(bn(x) + res) on batch statistics, the output of a ResNet bottleneck: fd_batchnorm_train_res_fwd_nhwc forward (the add and the ReLU in the
                            apply pass), ReLU-mask pass + fd_batchnorm_train_bwd_nhwc backward; bottleneck(blk, x, batch_stats=True) = the whole block with its
                            BatchNorms in training mode, opt-in (trunk.hip_bn_train), nn.SyncBatchNorm across ranks included.  With f16_maps=True
                            (trunk.hip_bn_f16_maps) under torch.autocast(float16) those nodes keep f16 maps: _BatchNormWideRowsH, _BatchNormResRowsH,
                            _SyncBatchNormApplyH on fd_batchnorm_train_*_nhwc_h, the raw conv outputs stored as f16.

What the kernels do not cover falls back to stock PyTorch-ROCm ops on the GPU: the data gradient of strided layers other than the
parity-class geometries and of layers padded by more than dil * (k - 1) (the rungs of _dense_dgrad), a padding='same' that torch pads asymmetrically,
dense layers with Cin % 32 != 0 (the 7x7 stem when it is trainable and its node is not switched on), BatchNorm in training mode or with trainable
affine parameters behind a conv of the ResNet trunk while trunk.hip_bn_train is off (conv_bn_act: the conv on HIP, the statistics stock), and SiLU after a BatchNorm (its derivative needs the pre-activation, which the fused epilogue does
not keep).  Narrow outputs (class / centre-ness / box logits) are padded to 32 channels by `conv_rows(pad_out=True)`.
"""
from __future__ import annotations

import collections
import functools
import os
import weakref
from typing import List, NamedTuple, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from ._lib import FdError, Segs
from .ops import ACT_NONE, ACT_RELU, ACT_SILU, Rows

# Under torch.autocast (the reference trains with AMP when cfg['model']['amp'] is set, train.py:175) the HIP nodes keep
# computing in fp32: inputs are cast up on entry, autocast is off inside, gradients come back in fp32.
def _fwd32(fwd):
    """torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32) without its recursive argument walk: under autocast the top-level floating-point CUDA
    tensors are cast to fp32 and the forward runs with autocast off (custom_bwd then runs the backward the same way); otherwise the forward runs as it is.  The nodes'
    arguments are flat (tensors, Segs tables, ints, tuples of fp32 constants), and torch's generic walk over them -- ~1 100 _cast calls per training step -- was 2 ms of
    the 20 ms of host work that bound the AMP step (tools/train_host_time.py)."""
    @functools.wraps(fwd)
    def wrapper(ctx, *args):
        ctx._dtype = torch.get_autocast_dtype("cuda")
        ctx._fwd_used_autocast = False
        if torch.is_autocast_enabled("cuda"):
            args = tuple(a.float() if (isinstance(a, torch.Tensor) and a.is_cuda and a.is_floating_point() and a.dtype is not torch.float32) else a for a in args)
            with torch.autocast("cuda", enabled=False):
                return fwd(ctx, *args)
        return fwd(ctx, *args)
    return wrapper


_bwd = torch.amp.custom_bwd(device_type="cuda")
_fwd_keep = torch.amp.custom_fwd(device_type="cuda")      # nodes that handle f16 / fp32 inputs themselves (AMP_F16_STORE): no cast on entry

AMP_F16 = os.environ.get("FD_AMP_F16", "1") != "0"      # "0": the HIP nodes compute in fp32 under torch.autocast too (wider than the reference)
# Under autocast the reference's convolutions read and write fp16 TENSORS (train.py:175-181): with FD_AMP_F16_STORE (default on) the nodes that are built for it keep
# their activations -- and the gradients flowing back through them -- in HBM as f16 (fd_conv_params.io_f16: the FD_PREC_F16 kernels fetch / store f16 without a
# conversion pass; GradScaler keeps the gradients in f16's range exactly as it does for the reference).  Today: the ResNet bottlenecks (_BottleneckRows); the other
# nodes take fp32 and torch.amp's cast on entry converts at the boundary.  "0": fp32 maps everywhere (round 3's AMP step).
AMP_F16_STORE = os.environ.get("FD_AMP_F16_STORE", "1") != "0"


def amp_prec() -> int:
    """Conv arithmetic of the HIP nodes for the current autocast state: under torch.autocast(float16) -- how the reference trains
    (train.py:33 amp_enabled, :175-181 autocast + GradScaler) -- dense convolutions (forward, data gradient, weight gradient) run with
    f16 operands and fp32 accumulation (FD_PREC_F16: what autocast's fp16 convolution computes); GroupNorm / BatchNorm statistics,
    depthwise convs, SE, activations and the losses stay fp32, as autocast keeps normalisation and loss ops.  Otherwise exact fp32."""
    if AMP_F16 and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.float16:
        return _lib.PREC_F16
    return _lib.PREC_F32


_STOCK = os.environ.get("FD_TRAIN_STOCK_CONV") == "1"   # diagnostic: route every layer to the stock ops (timing comparisons)
STATS = {"cl_copies": 0, "stock_fallbacks": 0}           # activation-sized layout copies made on entry / stock-op fallbacks taken (both should stay 0)
# FD_STRICT=1 (the test suite's default, tests/conftest.py): a layer of the TRAINING forward / backward that the HIP kernels do not cover
# raises FdError instead of silently running on stock PyTorch-ROCm ops (MIOpen convolutions, native batch / group norm).  Off by
# default so that exotic user configurations (a trainable 7x7 stem, odd widths) still train; the explicit diagnostic mode
# FD_TRAIN_STOCK_CONV=1 is exempt.
STRICT = os.environ.get("FD_STRICT", "0") == "1"


def stock_fallback(what: str) -> None:
    """Called on every path that is about to run a conv / norm of the training step on stock ops."""
    STATS["stock_fallbacks"] = STATS.get("stock_fallbacks", 0) + 1
    if STRICT and not _STOCK:
        raise FdError(f"FD_STRICT=1: {what} is not covered by the HIP kernels and would run on stock PyTorch-ROCm ops")


# ----------------------------------------------------------------------------------------------- layout helpers
def to_rows(t: torch.Tensor) -> torch.Tensor:
    """NCHW-shaped tensor -> [B*H*W, C] rows (a view when `t` is channels-last; autograd-tracked either way)."""
    if not t.is_contiguous(memory_format=torch.channels_last):
        STATS["cl_copies"] += 1
        t = t.contiguous(memory_format=torch.channels_last)
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, Cc)


def from_rows(r: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """[B*H*W, C] rows -> NCHW-shaped channels-last view."""
    return r.view(B, H, W, r.shape[1]).permute(0, 3, 1, 2)


def pyramid_rows(maps: Sequence[torch.Tensor]):
    """Five NCHW maps -> one [sum B*H*W, C] rows buffer (level-major, the inference layout) + its segment table."""
    B = maps[0].shape[0]
    segs = Segs.make(B, [(t.shape[2], t.shape[3]) for t in maps])
    return torch.cat([to_rows(t) for t in maps], 0), segs


def pyramid_split(r: torch.Tensor, segs: Segs) -> List[torch.Tensor]:
    """Rows buffer -> list of NCHW-shaped channels-last views, one per level."""
    out = []
    for i, (h, w) in enumerate(segs.level_hw()):
        out.append(from_rows(r[segs.m_start[i]:segs.m_start[i + 1]], segs.batch, h, w))
    return out


def _r(t: torch.Tensor) -> Rows:
    return Rows(t)


def _rv(t: torch.Tensor) -> Optional[Rows]:
    """Rows of a 2-D tensor that may be a channel-slice VIEW of a contiguous rows buffer (x[:, a:b]); None if it is neither."""
    if t.is_contiguous():
        return Rows(t)
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        cs = t.stride(0)
        co = t.storage_offset() % cs
        if co + t.shape[1] <= cs and t.storage_offset() - co + t.shape[0] * cs <= t.untyped_storage().nbytes() // 4:
            base = t.as_strided((t.shape[0], cs), (cs, 1), t.storage_offset() - co)
            return Rows(base, co, t.shape[1])
    return None


def _pad_of(m: nn.Conv2d) -> Optional[int]:
    """The kernels' symmetric padding of a square conv (ops.conv_pad): 'valid' is 0, 'same' is dil * (k - 1) / 2, None for a 'same' that torch pads
    asymmetrically (dil * (k - 1) odd).  _square declines the None case, so behind a coverage predicate this is an int."""
    return ops.conv_pad(m)


def _square(m: nn.Conv2d) -> bool:
    return (m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.dilation[0] == m.dilation[1]
            and (_pad_of(m) is not None if isinstance(m.padding, str) else m.padding[0] == m.padding[1]) and m.padding_mode == "zeros")


def _f32(x: torch.Tensor) -> bool:
    """fp32 data, or any float data while autocast is on (the nodes cast their inputs up to fp32 then)."""
    return x.dtype == torch.float32 or (x.is_floating_point() and torch.is_autocast_enabled())


def _dense_ok(m: nn.Conv2d, x: torch.Tensor, pad_out: bool = False) -> bool:
    """Dense convs the HIP node takes: groups 1, Cin % 32 == 0, Cout % 4 == 0 (any Cout with pad_out), fp32, a square kernel / stride / dilation and a
    SYMMETRIC zero padding -- an int or (p, p) tuple of any size, 'valid' (= 0), or 'same' with dil * (k - 1) even.  A 'same' that torch pads asymmetrically
    (an even kernel at an odd dilation) is declined: conv_bn_act then takes the counted stock fallback, the layers raise FdError.  The forward and the weight
    gradient run on the HIP kernels for every admitted geometry; the data gradient's rungs, stock ones included, are listed in _dense_dgrad."""
    return (m.groups == 1 and m.in_channels % 32 == 0 and (pad_out or m.out_channels % 4 == 0) and _square(m)
            and _f32(x) and m.weight.dtype == torch.float32)


def _dw_ok(m: nn.Conv2d, x: torch.Tensor) -> bool:
    c4 = m.in_channels // 4
    return (m.groups == m.in_channels == m.out_channels and m.in_channels % 4 == 0 and m.kernel_size == (3, 3)
            and m.stride == (1, 1) and m.dilation == (1, 1) and _square(m) and _pad_of(m) == 1      # (_square: padding (1, 1), not (1, q))
            and m.bias is None and ((c4 < 256 and 256 % c4 == 0) or c4 % 256 == 0) and _f32(x))


def _gn_ok(gn: nn.Module, x: torch.Tensor) -> bool:
    if not isinstance(gn, nn.GroupNorm) or not gn.affine or not _f32(x):
        return False
    Cc = gn.num_channels
    return Cc % 4 == 0 and Cc <= 1024 and 256 % (Cc // 4) == 0 and Cc % gn.num_groups == 0


BN_TYPES = (nn.BatchNorm2d, nn.SyncBatchNorm)     # SyncBatchNorm.convert_sync_batchnorm(model) (train.py:103) swaps the class, not the tensors


def bn_is_frozen(bn: Optional[nn.Module]) -> bool:
    return (isinstance(bn, BN_TYPES) and not bn.training and bn.track_running_stats and bn.affine
            and not bn.weight.requires_grad and not bn.bias.requires_grad)


def _bn_fold(bn: nn.BatchNorm2d):
    """(scale, shift) of a frozen BatchNorm2d, cached on the module until any of its tensors is written to."""
    key = (bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version,
           bn.weight.data_ptr(), bn.running_mean.data_ptr())
    hit = getattr(bn, "_fd_fold", None)
    if hit is None or hit[0] != key:
        hit = (key, ops.fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps))
        bn._fd_fold = hit
    return hit[1]


def _act_id(act) -> int:
    if act is None or isinstance(act, nn.Identity):
        return ACT_NONE
    if isinstance(act, nn.ReLU):
        return ACT_RELU
    if isinstance(act, nn.SiLU):
        return ACT_SILU
    if isinstance(act, int):
        return act
    raise FdError(f"unsupported activation module {type(act).__name__}")


# ------------------------------------------------------------------------------------------- dense convolution
class Packed(NamedTuple):
    w: torch.Tensor          # the packed weights
    fmt: ops.WFormat         # their format (names the kernel and the arithmetic)
    cout: int                # output channels of the conv they feed


class _PackCache:
    """Packed conv weights of the model's PARAMETERS, kept across steps and refreshed by ONE launch per step.

    A train step needs every weight in the conv kernel's layout twice (forward, and flipped / transposed / BN-scaled for the
    data gradient) and the optimizer changes them all every step: ~150 small packing launches.  Entries are keyed by the
    parameter's storage (data_ptr, shape) and guarded by its version counter, so a stale entry is never used: a miss or a
    version mismatch packs on the spot (always correct), `refresh()` -- called at the top of every training forward --
    re-packs every known entry with fd_pack_conv_weights_batch_f32 (unconditionally: updates made through `.data` do not
    move the version counter) and records the versions it packed.  Code that calls the layer functions of this module
    directly AND updates weights through `.data` must call PACKS.refresh() itself before the next forward."""

    def __init__(self):
        self.entries: dict = {}     # key -> [weakref(param), scale, dgrad, Packed, version]
        self.params: dict = {}      # data_ptr -> weakref(param)
        self.table = None           # (signature, device tensor of fd_pack_job, max_elems)

    @staticmethod
    def _key(w, scale, dgrad, fmt):
        return (w.data_ptr(), tuple(w.shape), bool(dgrad), scale.data_ptr() if (scale is not None and dgrad) else 0, fmt)

    @staticmethod
    def _pack_now(w, scale, dgrad, fmt) -> Packed:
        return Packed(fmt.pack(w, scale, dgrad), fmt, fmt.cout(w.shape, dgrad))

    def get(self, w: torch.Tensor, scale: Optional[torch.Tensor] = None, dgrad: bool = False, fmt: ops.WFormat = ops.WFormat.DIRECT) -> Packed:
        """Weights packed in `fmt` (conv_format's choice); dgrad=True = the flipped / transposed / BN-scaled weights of the data gradient."""
        if isinstance(w, nn.Parameter) and w.is_contiguous():
            self.params[w.data_ptr()] = weakref.ref(w)
        ref = self.params.get(w.data_ptr())
        owner = ref() if ref is not None else None
        if owner is None or owner.data_ptr() != w.data_ptr() or owner.shape != w.shape or not w.is_contiguous():
            return self._pack_now(w, scale, dgrad, fmt)                   # a temporary (merged / padded weights): pack now
        key = self._key(w, scale, dgrad, fmt)
        e = self.entries.get(key)
        if e is not None and e[0]() is not owner:       # the address was recycled by another parameter: drop the old entry
            e = None
        if e is None:
            out = self._pack_now(w, scale, dgrad, fmt)
            self.entries[key] = [ref, scale, dgrad, out, w._version]
            self.table = None
            return out
        if e[4] != w._version:                                            # changed since the last refresh: re-pack in place
            fmt.pack(w, scale, dgrad, out=e[3].w)
            e[4] = w._version
        return e[3]

    def refresh(self) -> None:
        live = {}
        newest: dict = {}        # (param address, shape, format) -> newest data-gradient entry: a re-folded frozen BN (load_state_dict) makes
        for key, e in self.entries.items():      # a new scale tensor and a new entry; the superseded one is dropped here
            if key[2]:
                newest[(key[0], key[1], key[4])] = key
        for key, e in self.entries.items():
            p = e[0]()
            if p is not None and p.data_ptr() == key[0] and tuple(p.shape) == key[1] and (not key[2] or newest[(key[0], key[1], key[4])] == key):
                live[key] = e
        self.params = {a: r for a, r in self.params.items() if r() is not None}
        if len(live) != len(self.entries):
            self.entries, self.table = live, None
        if not live:
            return
        # unconditional: an update made through `.data` does not move the version counter, a re-pack is one short launch
        if self.table is None:
            jobs = (_lib.PackJob * len(live))()
            mx = 0
            for j, (key, e) in zip(jobs, live.items()):
                co, ci, kh, kw = key[1]
                j.w, j.scale, j.out = key[0], (e[1].data_ptr() if (e[1] is not None and e[2]) else None), e[3].w.data_ptr()
                j.Cout, j.Cin, j.KH, j.KW, j.mode = co, ci, kh, kw, key[4].mode | int(e[2])
                mx = max(mx, co * ci * kh * kw)
            raw = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).clone()
            dev = next(iter(live.values()))[3].w.device
            self.table = (raw.to(dev), len(live), mx)
        tab, n, mx = self.table
        ops.check(_lib.lib().fd_pack_conv_weights_batch_f32(tab.data_ptr(), n, mx, ops._stream()), "fd_pack_conv_weights_batch_f32")
        for e in live.values():
            e[4] = e[0]()._version


PACKS = _PackCache()


def conv_format(Cin: int, Cout: int, k: int, stride: int, pad: int, dil: int, segs: Segs, prec: int = 0) -> ops.WFormat:
    """PACKS.get's `fmt` for a dense conv (forward Cin -> Cout, or a data gradient with the channel roles swapped) under the node's arithmetic: ops.choose_conv
    with what the training nodes offer -- no split-K workspace, no vector-unit kernel.  3x3 stride-1 'same' fp32 layers go to a Winograd kernel as in the plans,
    AMP (FD_PREC_F16) layers stay on the direct kernel (F16K64 where the widths allow)."""
    return ops.choose_conv(segs, Cin, Cout, k, stride, pad, dil, "amp" if prec else "f32", split_k=False, narrow=False).fmt


_TILE_CACHE: dict = {}


def _conv_launch(x: torch.Tensor, segs: Segs, packed: Packed, y: torch.Tensor, *, k, stride, pad, dil, scale=None,
                 shift=None, res: Optional[torch.Tensor] = None, act=ACT_NONE, res_mask: bool = False) -> None:
    """y = act(conv(x, w) * scale + shift + res) on contiguous rows buffers; `packed` from PACKS.get.  Winograd / F16K64 formats name their kernel (the
    library picks the block tile).  The direct kernel's tile comes from the same table as the inference plans', remembered per key for the process: fp32
    launches take ops.autotune_conv's choice (table / shape heuristic / FD_AUTOTUNE timing); f16 launches (AMP) have own table entries ("f16|" keys, timed by
    `FD_AUTOTUNE=1 FD_AMP=1 python tools/tune_train.py`), and a miss takes the library's tile -- the fp32 heuristic would name single-buffer tiles the f16
    kernel is not built for -- unless FD_AUTOTUNE times it."""
    w, fmt, Cout = packed
    Cin = x.shape[1]
    rx, ry, rr = _r(x), _r(y), (_r(res) if res is not None else None)
    if fmt.tile:
        ops.conv_call(rx, segs, w, ry, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, scale=scale, shift=shift, res=rr, act=act,
                      res_mask=res_mask, precision=fmt.prec, tile=fmt.tile)()
        return
    f16 = fmt.prec == _lib.PREC_F16
    out_rows = y.shape[0]
    key = ops.tune_key(segs, Cin, Cout, k, stride, pad, dil, res=res is not None, xcs=Cin, ycs=Cout, pre="f16" if f16 else "")   # (mask / add: same cost)
    code = _TILE_CACHE.get(key)
    if code is None and f16:
        code = ops._tune_table().get(key, 0 if ops._TUNE_MODE == "0" else None)
        if code is not None:
            code = _TILE_CACHE[key] = int(code)
    ks = ops.tile_split(code)[1] if code is not None else 0
    # split-K scratch: an f16 code's own split; else (fp32, or a code still to be tuned) the widest split, up to 256 MB
    ws = None
    if f16 and ks > 1:
        ws = torch.empty(_lib.lib().fd_conv_workspace_bytes(out_rows, Cout, ks) // 4, dtype=torch.float32, device=x.device)
    elif code is None or ks > 1:
        nb = _lib.lib().fd_conv_workspace_bytes(out_rows, Cout, ops.KSPLIT_MAX)
        if 0 < nb <= 256 * 1024 * 1024:
            ws = torch.empty(nb // 4, dtype=torch.float32, device=x.device)
    call = ops.conv_call(rx, segs, w, ry, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, scale=scale, shift=shift, res=rr, act=act,
                         workspace=ws, res_mask=res_mask, precision=fmt.prec)
    if code is None:              # (autotune_conv installs the code it returns on the launch)
        code = _TILE_CACHE[key] = ops.autotune_conv(call, key, out_rows, Cout, (Cin // 32) * k * k)
    else:
        p = call.params
        p.tile, p.ksplit = ops.tile_split(code)
        if p.ksplit > 1 and ws is None:
            p.ksplit = 1
    call()


def _strided_dgrad(g: torch.Tensor, weight: torch.Tensor, scale: Optional[torch.Tensor], segs: Segs, k: int, stride: int, pad: int,
                   res: Optional[torch.Tensor] = None, res_mask: bool = False, prec: int = 0) -> Optional[torch.Tensor]:
    """dX rows of a strided single-level conv from dY rows `g` on the HIP conv kernel (None: geometry not covered)."""
    if _STOCK or segs.nseg != 1:
        return None
    B, (H, W) = segs.batch, segs.level_hw()[0]
    Cin = weight.shape[1]
    empty_class = any(T == 0 for _, T, _ in ops.strided_dgrad_classes(k, stride, pad))
    gx = (torch.zeros if empty_class else torch.empty)(B * H * W, Cin, dtype=g.dtype, device=g.device)      # (f16 maps under AMP_F16_STORE: the gradient's own type)
    ok = ops.conv_dgrad_strided(_r(g), weight, scale, _r(gx), B, H, W, k, stride, pad, res=_r(res) if res is not None else None,
                                res_mask=res_mask, precision=prec)
    if not ok:
        return None
    if res_mask and empty_class and res is not None:
        raise FdError("strided dgrad: a ReLU mask over a class-sparse gradient is not built")
    return gx


def _dense_launch(x: torch.Tensor, segs: Segs, w: torch.Tensor, y: torch.Tensor, k: int, stride: int, pad: int, dil: int, prec: int, scale=None, shift=None,
                  res: Optional[torch.Tensor] = None, act=ACT_NONE) -> None:
    """The forward launch of a dense conv layer from its OIHW weight `w` and its geometry (k, stride, pad, dil), stated once: the weight format, the packed
    weights (PACKS) and the launch.  y = act(conv(x, w) * scale + shift + res); `segs` is the table of x.  (Its data gradient: _dense_dgrad.)"""
    _conv_launch(x, segs, PACKS.get(w, fmt=conv_format(w.shape[1], w.shape[0], k, stride, pad, dil, segs, prec)), y, k=k, stride=stride, pad=pad, dil=dil,
                 scale=scale, shift=shift, res=res, act=act)


def _dense_dgrad(g: torch.Tensor, x: torch.Tensor, w: torch.Tensor, scale: Optional[torch.Tensor], segs: Segs, so: Segs, k: int, stride: int, pad: int,
                 dil: int, prec: int, res: Optional[torch.Tensor] = None, res_mask: bool = False) -> torch.Tensor:
    """dX rows of a dense conv layer from dY rows `g`, given the layer as its forward saw it: input map x on `segs`, output on `so` (both tables were made by
    the forward: none is built here), OIHW weight `w`, folded-BN `scale`, geometry k / stride / pad / dil.  `res` is a gradient added to dX, or with res_mask
    the ReLU output of the layer dX flows into (dX is masked by it).  The rungs:
      stride 1, Cout % 32 == 0      the conv kernel on dY over `so` with the channel roles swapped, the flipped / transposed / scaled weights and
      and pad <= dil * (k - 1)      pad' = dil * (k - 1) - pad; `res` rides in its epilogue
      strided, one level, dil 1     one exact-FLOP launch per parity class (ops.conv_dgrad_strided: the classes that need no padding -- k = 3 / pad 1,
                                    k = 1 / pad 0, k = stride / pad 0), `res` in their epilogues
      what is left on one level     (narrow Cout, dilated + strided, the other strided geometries, pad > dil * (k - 1): pad' would be negative, a crop the
                                    kernel does not take) the stock op, then one relu_mask launch or the add; counted by stock_fallback
      what is left over a pyramid   an error
    _BottleneckRows never reaches the last two: bottleneck() admits only widths with Cout % 32 == 0 and dilation 1 to the node."""
    Cout = w.shape[0]
    if stride == 1 and Cout % 32 == 0 and pad <= dil * (k - 1):
        gx = torch.empty_like(x)
        pad = dil * (k - 1) - pad
        _conv_launch(g, so, PACKS.get(w, scale, dgrad=True, fmt=conv_format(Cout, w.shape[1], k, 1, pad, dil, so, prec)), gx, k=k, stride=1, pad=pad, dil=dil,
                     res=res, res_mask=res_mask)
        return gx
    if segs.nseg != 1:
        if stride == 1 and Cout % 32 == 0:
            raise FdError(f"data gradient of a {k}x{k} conv padded by {pad} > dilation * (k - 1) = {dil * (k - 1)} over a pyramid is not supported: the HIP "
                          "kernel takes no negative padding and the stock rung is single-level (run the levels one by one, or pad by at most dilation * (k - 1))")
        raise FdError("data gradient of a strided / narrow conv over a pyramid is not supported (pad Cout to 32)")
    if stride > 1 and dil == 1 and (gx := _strided_dgrad(g, w, scale, segs, k, stride, pad, res=res, res_mask=res_mask, prec=prec)) is not None:
        return gx
    stock_fallback(f"the data gradient of a {k}x{k} stride-{stride} pad-{pad} dilation-{dil} conv with Cout={Cout}")
    weff = w.detach() if scale is None else w.detach() * scale.view(-1, 1, 1, 1)
    B, (H, W), (Ho, Wo) = segs.batch, segs.level_hw()[0], so.level_hw()[0]
    gx = to_rows(torch.ops.aten.convolution_backward(from_rows(g, B, Ho, Wo), from_rows(x, B, H, W), weff, None, [stride, stride], [pad, pad], [dil, dil],
                                                     False, [0, 0], 1, [True, False, False])[0])
    if res_mask:
        return relu_mask(gx.contiguous(), res)
    return gx if res is None else gx + res


class _ConvRows(torch.autograd.Function):
    """y = act(conv(x, w) * scale + shift + residual) on rows; scale is a constant (frozen BN), shift may need a gradient."""

    @staticmethod
    @_fwd_keep
    def forward(ctx, x, weight, scale, shift, residual, segs, stride, pad, dil, act, prec=0, out_f16=False):
        # (no cast on entry: under AMP with AMP_F16_STORE the FD_PREC_F16 kernels read an f16 or an fp32 map as it is; out_f16 -- set by the caller for an edge whose
        # consumers are conv nodes too -- stores the output as f16.  Otherwise everything is fp32, as with torch.amp's cast_inputs.)
        if act not in (ACT_NONE, ACT_RELU):
            raise FdError("_ConvRows differentiates ACT_NONE / ACT_RELU epilogues only (use act_rows for SiLU: it keeps the pre-activation)")
        f16_io = bool(prec) and AMP_F16_STORE
        if not f16_io or x.dtype not in (torch.float16, torch.float32):
            x = x.float()
            residual = residual.float() if residual is not None else None
        x = x.contiguous()
        Cout, _, k, _ = weight.shape
        so = ops.conv_out_segs(segs, k, stride, pad, dil)
        y = torch.empty(so.rows, Cout, dtype=torch.float16 if (f16_io and out_f16) else torch.float32, device=x.device)
        _dense_launch(x, segs, weight, y, k, stride, pad, dil, prec, scale=scale.float() if scale is not None else None,
                      shift=shift.detach().float().contiguous() if shift is not None else None, res=residual.contiguous() if residual is not None else None, act=act)
        ctx.res_dtype = residual.dtype if residual is not None else None
        ctx.save_for_backward(x, weight, scale, y if act == ACT_RELU else None)
        ctx.geom = (segs, so, stride, pad, dil, act, prec)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, weight, scale, y = ctx.saved_tensors
        segs, so, stride, pad, dil, act, prec = ctx.geom
        g = resolve_pending(gy).contiguous()
        if act == ACT_RELU:
            g = relu_mask(g if g.dtype == y.dtype else g.to(y.dtype), y)
        Cin = x.shape[1]
        Cout, _, k, _ = weight.shape
        gx = gw = gshift = gres = None
        if ctx.needs_input_grad[4]:
            gres = g if g.dtype == ctx.res_dtype else g.to(ctx.res_dtype)
        if ctx.needs_input_grad[0]:
            gx = _dense_dgrad(g, x, weight, scale, segs, so, k, stride, pad, dil, prec)
        if ctx.needs_input_grad[1]:
            gw = ops.conv_wgrad(_r(x), _r(g), segs, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, scale=scale,
                                oihw=True, precision=prec)
        if ctx.needs_input_grad[3]:
            gshift = g.sum(dim=0, dtype=torch.float32)
        return gx, gw, None, gshift, gres, None, None, None, None, None, None, None


def conv_rows(m: nn.Conv2d, x: torch.Tensor, segs: Segs, bn: Optional[nn.Module] = None, act: int = ACT_NONE,
              residual: Optional[torch.Tensor] = None, pad_out: bool = False, out_f16: bool = False) -> torch.Tensor:
    """HIP conv layer on a rows buffer (must be covered: check with `covered(m, bn, x)`).  With pad_out the output
    channels are zero-padded to a multiple of 32 inside (so the data gradient runs on the HIP kernel) and sliced back.
    out_f16: under AMP (and AMP_F16_STORE) the output map is stored as f16 -- for edges whose consumers are conv nodes (they read f16 maps directly)."""
    scale = shift = None
    if bn is not None:
        scale, shift = _bn_fold(bn)
    w, b = m.weight, m.bias
    Cout = w.shape[0]
    padn = (-Cout) % 32 if pad_out else 0
    if padn:
        w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, padn))
        b = F.pad(b, (0, padn)) if b is not None else None
        if scale is not None:
            scale, shift = F.pad(scale, (0, padn), value=1.0), F.pad(shift, (0, padn))
    if b is not None:
        shift = b if scale is None else b * scale + shift
    y = _ConvRows.apply(x, w, scale, shift, residual, segs, m.stride[0], _pad_of(m), m.dilation[0], act, amp_prec(), out_f16)
    return y[:, :Cout] if padn else y


class MergedConv:
    """Two convs with the same geometry and input (reg_pred 4 + cnt_logits 1) presented to conv_rows as one layer."""

    def __init__(self, a: nn.Conv2d, b: nn.Conv2d):
        self.weight = torch.cat((a.weight, b.weight), 0)
        self.bias = torch.cat((a.bias, b.bias), 0) if a.bias is not None else None
        self.stride, self.padding, self.dilation, self.kernel_size = a.stride, a.padding, a.dilation, a.kernel_size


def predictor_rows(cls_logits: nn.Conv2d, reg_pred: nn.Conv2d, cnt_logits: nn.Conv2d, c: torch.Tensor, r: torch.Tensor, segs: Segs, scale_exp):
    """The predictor tail of an FCOS head over the whole pyramid: class logits from the class tower `c`; box regression and centre-ness from the
    regression tower `r` in one launch; exp(reg * scale_i) per level.  Returns (cls_l, cnt_l, reg_l), each a list of per-level NCHW-shaped views."""
    cls = conv_rows(cls_logits, c, segs, pad_out=True)
    rc = conv_rows(MergedConv(reg_pred, cnt_logits), r, segs, pad_out=True)     # [:, :4] boxes, [:, 4] centre-ness
    cls_l = pyramid_split(cls, segs)
    cnt_l = pyramid_split(rc[:, 4:5], segs)
    reg_l = [torch.exp(t * scale_exp[i].scale) for i, t in enumerate(pyramid_split(rc[:, :4], segs))]
    return cls_l, cnt_l, reg_l


class _BottleneckRows(torch.autograd.Function):
    """A whole ResNet bottleneck with frozen BatchNorm as one autograd node (torchvision Bottleneck.forward):
         y1 = relu(bn1(conv1 x));  y2 = relu(bn2(conv2 y1));  out = relu(bn3(conv3 y2) + (downsample(x) | x))
    Forward: the same 3-4 fused conv launches as separate nodes would issue.  Backward, written out by hand so that the
    elementwise work rides in the conv epilogues: one mask pass for the block output, then every data gradient is masked
    by the ReLU of the layer it flows into INSIDE the conv that produces it (res_mode 1) and the identity gradient is added
    in conv1's data-gradient epilogue (res_mode 0): per block 1 elementwise pass instead of 3 masks + 1 add."""

    @staticmethod
    @_fwd_keep
    def forward(ctx, x, w1, w2, w3, wd, c1, c2, c3, cd, segs, stride, prec=0):
        # (no cast on entry: under AMP the node takes an f16 map as it is -- the previous bottleneck's output -- or an fp32 one, and keeps its own maps in f16)
        h = bool(prec)
        st = torch.float16 if (h and AMP_F16_STORE) else torch.float32          # storage type of this node's activations and gradients
        x = x.contiguous() if (x.dtype == st or (h and AMP_F16_STORE and x.dtype == torch.float32)) else x.to(st).contiguous()
        dev = x.device
        so = ops.conv_out_segs(segs, 3, stride, 1, 1)
        P, C4 = w1.shape[0], w3.shape[0]
        y1 = torch.empty(segs.rows, P, dtype=st, device=dev)
        y2 = torch.empty(so.rows, P, dtype=st, device=dev)
        out = torch.empty(so.rows, C4, dtype=st, device=dev)
        _dense_launch(x, segs, w1, y1, 1, 1, 0, 1, prec, scale=c1[0], shift=c1[1], act=ACT_RELU)
        _dense_launch(y1, segs, w2, y2, 3, stride, 1, 1, prec, scale=c2[0], shift=c2[1], act=ACT_RELU)
        if wd is not None:
            idt = torch.empty(so.rows, C4, dtype=st, device=dev)
            _dense_launch(x, segs, wd, idt, 1, stride, 0, 1, prec, scale=cd[0], shift=cd[1])
        else:
            idt = x
        _dense_launch(y2, so, w3, out, 1, 1, 0, 1, prec, scale=c3[0], shift=c3[1], res=idt, act=ACT_RELU)
        ctx.save_for_backward(x, y1, y2, out, w1, w2, w3, wd, c1[0], c2[0], c3[0], cd[0] if wd is not None else None)
        ctx.geom = (segs, so, stride, prec)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, gout):
        x, y1, y2, out, w1, w2, w3, wd, s1, s2, s3, sd = ctx.saved_tensors
        segs, so, stride, prec = ctx.geom
        h = bool(prec)
        need_x = ctx.needs_input_grad[0]
        P, Cin, C4 = w1.shape[0], w1.shape[1], w3.shape[0]
        g = relu_mask(gout.contiguous() if gout.dtype == out.dtype else gout.to(out.dtype), out)      # the one elementwise pass of the block
        gw1 = gw2 = gw3 = gwd = gx = None
        wg = lambda xx, gg, sg, Ci, Co, k, st, pad, sc: ops.conv_wgrad(_r(xx), _r(gg), sg, Cin=Ci, Cout=Co, k=k, stride=st,  # noqa: E731
                                                                     pad=pad, dil=1, scale=sc, oihw=True, precision=prec)
        if ctx.needs_input_grad[3]:
            gw3 = wg(y2, g, so, P, C4, 1, 1, 0, s3)
        g2 = _dense_dgrad(g, y2, w3, s3, so, so, 1, 1, 0, 1, prec, res=y2, res_mask=True)     # d/d(conv2 output), ReLU-masked in the epilogue
        if ctx.needs_input_grad[2]:
            gw2 = wg(y1, g2, segs, P, P, 3, stride, 1, s2)
        # conv2's data gradient, the ReLU mask of y1 in the epilogue (strided: four parity-class launches on the conv kernel)
        g1 = _dense_dgrad(g2, y1, w2, s2, segs, so, 3, stride, 1, 1, prec, res=y1, res_mask=True)
        if ctx.needs_input_grad[1]:
            gw1 = wg(x, g1, segs, Cin, P, 1, 1, 0, s1)
        if wd is not None and ctx.needs_input_grad[4]:
            gwd = wg(x, g, segs, Cin, C4, 1, stride, 0, sd)
        if need_x:
            # identity path, or the downsample's data gradient (1x1 stride 2: the (0, 0) parity class is a plain GEMM scattered into a zeroed dX)
            gid = g if wd is None else _dense_dgrad(g, x, wd, sd, segs, so, 1, stride, 0, 1, prec)
            gx = _dense_dgrad(g1, x, w1, s1, segs, segs, 1, 1, 0, 1, prec, res=gid)       # conv1's data gradient + the identity gradient
        return gx, gw1, gw2, gw3, gwd, None, None, None, None, None, None, None


def _bottleneck_bn_rows(blk: nn.Module, x: torch.Tensor, f16_maps: bool = False) -> torch.Tensor:
    """A bottleneck whose BatchNorms run on batch statistics (any of them may also be frozen), every layer a HIP node on rows: conv1/bn1/ReLU, conv2/bn2/ReLU
    and the downsample conv/BN through conv_norm_act_rows' dispatch, then the raw conv3 and act(bn3(.) + identity) as one node (batchnorm_train_res_rows).
    Across ranks the downsample BatchNorm's statistics all-reduce is issued before conv1 and waited for where the residual is needed.
    f16_maps (the trunk's opt-in hip_bn_f16_maps) under torch.autocast(float16) with AMP_F16_STORE; otherwise the graph is the one above, unchanged.  The
    f16 maps are then: the raw output of every conv that feeds a BatchNorm in training mode with a float momentum, and that BatchNorm's output (the
    any-width `_h` kernels at every width, narrow ones included); the output of every conv with a frozen BatchNorm folded in, the downsample's and conv3's
    included; hence y1, y2, the identity and the block's output whenever their BatchNorm is one of those two kinds -- what _BottleneckRows keeps in f16.  A
    BatchNorm with momentum=None keeps the fp32 node behind a raw fp32 conv output, so its own output map (and, for bn3, the block's) is fp32; its
    neighbours take either type as it comes, and an fp32 identity reaching an f16 bn3 node is converted once on entry."""
    B, _, H, W = x.shape
    ds, s = blk.downsample, blk.conv2.stride[0]
    segs = Segs.make(B, [(H, W)])
    so = ops.conv_out_segs(segs, 3, s, 1, 1)
    xr = to_rows(x)
    hd = conv_norm_begin(ds[0], ds[1], xr, segs, ACT_NONE, f16_maps) if ds is not None else None
    y = conv_norm_act_rows(blk.conv1, blk.bn1, xr, segs, ACT_RELU, f16_maps)
    y = conv_norm_act_rows(blk.conv2, blk.bn2, y, segs, ACT_RELU, f16_maps)
    idt = xr if ds is None else conv_norm_finish(hd)
    f16_maps = _f16_maps_on(f16_maps)
    if bn_is_frozen(blk.bn3):
        if f16_maps:
            out = conv_rows(blk.conv3, y, so, blk.bn3, ACT_RELU, residual=idt, out_f16=True)
        else:
            out = conv_rows(blk.conv3, y, so, blk.bn3, ACT_RELU, residual=idt.float())      # (fp32 maps on this path, whatever the block before stored)
    else:
        f16 = _bn_f16_ok(blk.bn3, f16_maps)
        out = batchnorm_train_res_rows(blk.bn3, conv_rows(blk.conv3, y, so, None, ACT_NONE, out_f16=f16), idt, ACT_RELU, f16=f16)
    return from_rows(out, B, so.H[0], so.W[0])


def bottleneck(blk: nn.Module, x: torch.Tensor, batch_stats: bool = False, f16_maps: bool = False) -> torch.Tensor:
    """torchvision-style Bottleneck (conv1/bn1, conv2/bn2, conv3/bn3, optional downsample) on an NCHW-shaped tensor: one
    fused autograd node when every BatchNorm is frozen and the shapes are covered, else layer by layer (conv_bn_act).  batch_stats (the trunk's opt-in
    hip_bn_train): a covered block with BatchNorms in training mode runs on the batch-statistics nodes instead (_bottleneck_bn_rows); f16_maps (the trunk's
    hip_bn_f16_maps, read with batch_stats only): those nodes keep f16 maps under torch.autocast(float16)."""
    _need_cuda(x)
    ds = blk.downsample
    bns = [blk.bn1, blk.bn2, blk.bn3] + ([ds[1]] if ds is not None else [])
    convs = [blk.conv1, blk.conv2, blk.conv3] + ([ds[0]] if ds is not None else [])
    shapes_ok = (not _STOCK and all(c.bias is None and _dense_ok(c, x) and c.out_channels % 32 == 0 for c in convs)
                 and blk.conv1.kernel_size == (1, 1) and blk.conv3.kernel_size == (1, 1) and blk.conv2.kernel_size == (3, 3)
                 and blk.conv2.padding == (1, 1) and blk.conv2.dilation == (1, 1) and blk.conv1.stride == (1, 1) and blk.conv3.stride == (1, 1)
                 and (ds is None or (ds[0].kernel_size == (1, 1) and ds[0].stride == blk.conv2.stride)))
    ok = shapes_ok and all(bn_is_frozen(b) for b in bns)
    if batch_stats and shapes_ok and not ok and all(bn_is_frozen(b) or _bn_family(b, x) is not None for b in bns):
        return _bottleneck_bn_rows(blk, x, f16_maps)
    if not ok:
        idt = x if ds is None else conv_bn_act(ds[0], ds[1], x, ACT_NONE)
        y = conv_bn_act(blk.conv1, blk.bn1, x, ACT_RELU)
        y = conv_bn_act(blk.conv2, blk.bn2, y, ACT_RELU)
        return conv_bn_act(blk.conv3, blk.bn3, y, ACT_RELU, residual=idt)
    B, _, H, W = x.shape
    s = blk.conv2.stride[0]
    out = _BottleneckRows.apply(to_rows(x), blk.conv1.weight, blk.conv2.weight, blk.conv3.weight, ds[0].weight if ds is not None else None,
                                _bn_fold(blk.bn1), _bn_fold(blk.bn2), _bn_fold(blk.bn3), _bn_fold(ds[1]) if ds is not None else (None, None),
                                Segs.make(B, [(H, W)]), s, amp_prec())
    return from_rows(out, B, (H - 1) // s + 1, (W - 1) // s + 1)


# --------------------------------------------------------------------------------------------- depthwise 3x3
class _DwRows(torch.autograd.Function):
    """Depthwise 3x3 (stride 1, pad 1, no bias): y = act(dw(x, w) * scale + shift), scale / shift constants."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, weight, scale, shift, segs, act):
        if act not in (ACT_NONE, ACT_RELU):
            raise FdError("_DwRows differentiates ACT_NONE / ACT_RELU epilogues only (use act_rows for SiLU)")
        x = x.contiguous()
        y = torch.empty_like(x)
        ops.dwconv3x3(_r(x), ops.pack_dw_weight(weight), _r(y), segs, scale, shift, act)
        ctx.save_for_backward(x, weight, scale, y if act == ACT_RELU else None)
        ctx.geom = (segs, act)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, weight, scale, y = ctx.saved_tensors
        segs, act = ctx.geom
        g = resolve_pending(gy).contiguous()
        if act == ACT_RELU:
            g = relu_mask(g, y)
        Cc = x.shape[1]
        gx = gw = None
        if ctx.needs_input_grad[0]:
            weff = weight.detach() if scale is None else weight.detach() * scale.view(-1, 1, 1, 1)
            gx = torch.empty_like(x)
            ops.dwconv3x3(_r(g), ops.pack_dw_weight(weff.flip(2, 3)), _r(gx), segs)
        if ctx.needs_input_grad[1]:
            gw = ops.dwconv3x3_wgrad(_r(x), _r(g), segs, scale, torch_layout=True)
        return gx, gw, None, None, None, None


def dw_rows(m: nn.Conv2d, x: torch.Tensor, segs: Segs, bn: Optional[nn.Module] = None, act: int = ACT_NONE) -> torch.Tensor:
    scale = shift = None
    if bn is not None:
        scale, shift = _bn_fold(bn)
    return _DwRows.apply(x, m.weight, scale, shift, segs, act)


# ------------------------------------------------------------------------- dilated depthwise k x k (MNBlock)
def _dw_dilated_ok(m: nn.Conv2d, x: torch.Tensor) -> bool:
    k, d = m.kernel_size[0], m.dilation[0]
    return (m.groups == m.in_channels == m.out_channels and m.in_channels % 4 == 0 and _square(m) and k in (3, 5, 7) and 1 <= d <= 8
            and m.stride == (1, 1) and _pad_of(m) == d * (k - 1) // 2 and m.bias is None and _f32(x) and m.weight.dtype == torch.float32)


class _DwDilatedRows(torch.autograd.Function):
    """Dilated depthwise k x k (k in {3, 5, 7}, stride 1, 'same' padding, no bias) over a pyramid: y = dw(x, w) * scale + shift, scale / shift
    constants (a frozen BatchNorm).  Data gradient: the forward launch on dy with reversed, scaled taps (k odd, padding symmetric: exact); weight
    gradient: fd_dwconv_dilated_bwd_weight_nhwc.  fp32 under autocast, like the 3x3 depthwise node."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, weight, scale, shift, segs, K, dil):
        x = x.contiguous()
        y = torch.empty_like(x)
        ops.dwconv_dilated(_r(x), ops.pack_dwk_weight(weight), _r(y), segs, K, dil, scale, shift, ACT_NONE)
        ctx.save_for_backward(x, weight, scale)
        ctx.geom = (segs, K, dil)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, weight, scale = ctx.saved_tensors
        segs, K, dil = ctx.geom
        g = resolve_pending(gy).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            ops.dwconv_dilated(_r(g), ops.pack_dwk_weight_reversed(weight, scale), _r(gx), segs, K, dil)
        if ctx.needs_input_grad[1]:
            gw = ops.dwconv_dilated_wgrad(_r(x), _r(g), segs, K, dil, scale, torch_layout=True)
        return gx, gw, None, None, None, None, None


def dw_dilated_rows(m: nn.Conv2d, x: torch.Tensor, segs: Segs, bn: Optional[nn.Module] = None) -> torch.Tensor:
    """bn(m(x)) on a rows buffer for a dilated depthwise conv `m` and a FROZEN BatchNorm (folded into scale / shift), or m(x) with bn=None."""
    if not _dw_dilated_ok(m, x):
        raise FdError(f"dilated depthwise conv {tuple(m.weight.shape)} dilation {m.dilation} padding {m.padding}: the HIP kernels cover "
                      "k in {3, 5, 7}, stride 1, 'same' padding, 1 <= dilation <= 8, C % 4 == 0, no bias, fp32")
    scale = shift = None
    if bn is not None:
        scale, shift = _bn_fold(bn)
    return _DwDilatedRows.apply(x, m.weight, scale, shift, segs, m.kernel_size[0], m.dilation[0])


# ------------------------------------------------------- MBConv (EfficientNet trunk): strided depthwise k x k, whole block
def round32(c: int) -> int:
    return (c + 31) // 32 * 32


class _DwKxKRows(torch.autograd.Function):
    """Depthwise k x k (k in {3, 5}, stride in {1, 2}, asymmetric static "SAME" padding, no bias) on single-level rows: z = dw(x, w) * scale + shift,
    scale / shift constants (a frozen BatchNorm), no activation (the swish behind it is an act_rows node that keeps z).  Forward fd_dwconv2d_nhwc,
    backward fd_dwconv2d_bwd_data_nhwc / fd_dwconv2d_bwd_weight_nhwc.  fp32 under autocast, like the other depthwise nodes."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, weight, scale, shift, geom):
        N, H, W, K, stride, pad_t, pad_l, Ho, Wo = geom
        x = x.contiguous()
        wkc = ops.pack_dwk_weight(weight)
        y = torch.empty(N * Ho * Wo, x.shape[1], dtype=torch.float32, device=x.device)
        ops.dwconv2d(_r(x), wkc, _r(y), N, H, W, K, stride, pad_t, pad_l, Ho, Wo, scale, shift, ACT_NONE)
        ctx.save_for_backward(x, wkc, scale)
        ctx.geom = geom
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, wkc, scale = ctx.saved_tensors
        N, H, W, K, stride, pad_t, pad_l, Ho, Wo = ctx.geom
        g = resolve_pending(gy).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            ops.dwconv2d_dgrad(_r(g), wkc, _r(gx), N, H, W, K, stride, pad_t, pad_l, Ho, Wo, scale)
        if ctx.needs_input_grad[1]:
            gw = ops.dwconv2d_wgrad(_r(x), _r(g), N, H, W, K, stride, pad_t, pad_l, Ho, Wo, scale, torch_layout=True)
        return gx, gw, None, None, None


def _pad_affine(scale: torch.Tensor, shift: torch.Tensor, padn: int):
    """A folded BatchNorm widened by `padn` pad channels: scale 1, shift 0 (a zero channel stays zero)."""
    return (F.pad(scale, (0, padn), value=1.0), F.pad(shift, (0, padn))) if padn else (scale, shift)


def dw_kxk_rows(m: nn.Conv2d, x: torch.Tensor, segs: Segs, pad, bn: Optional[nn.Module] = None) -> torch.Tensor:
    """bn(m(x)) on single-level rows for an MBConv depthwise conv `m` (k in {3, 5}, stride in {1, 2}; `pad` = its static (before, after) padding) and a FROZEN
    BatchNorm, or m(x) with bn=None.  x may be wider than m (a map held at its width rounded up to 32): the extra channels get zero taps, scale 1 and
    shift 0 inside the autograd graph, so they stay exactly zero and the weight gradient comes back at m's own shape."""
    K, s, Cc = m.kernel_size[0], m.stride[0], m.in_channels
    if not (m.groups == Cc == m.out_channels and m.kernel_size == (K, K) and m.stride == (s, s) and K in (3, 5) and s in (1, 2) and m.dilation == (1, 1)
            and m.bias is None and m.weight.dtype == torch.float32 and _f32(x) and x.shape[1] % 4 == 0 and x.shape[1] >= Cc and segs.nseg == 1
            and 0 <= pad[0] < K and 0 <= pad[1] < K):
        raise FdError(f"depthwise conv {tuple(m.weight.shape)} stride {m.stride} on {x.shape[1]} channels: the HIP nodes cover k in {{3, 5}}, "
                      "stride in {1, 2}, no bias, fp32, C % 4 == 0, one level")
    if bn is not None and not bn_is_frozen(bn):
        raise FdError("dw_kxk_rows folds a FROZEN BatchNorm only")
    N, (H, W) = segs.batch, segs.level_hw()[0]
    Ho, Wo = (H + pad[0] + pad[1] - K) // s + 1, (W + pad[0] + pad[1] - K) // s + 1
    if Ho < 1 or Wo < 1:
        raise FdError(f"depthwise {K}x{K} stride {s} padding {tuple(pad)}: the {H}x{W} map is too small")
    padn = x.shape[1] - Cc
    w = F.pad(m.weight, (0, 0, 0, 0, 0, 0, 0, padn)) if padn else m.weight
    scale = shift = None
    if bn is not None:
        scale, shift = _pad_affine(*_bn_fold(bn), padn)
    return _DwKxKRows.apply(x, w, scale, shift, (N, H, W, K, s, pad[0], pad[0], Ho, Wo))


def conv_rows_wide(m: nn.Conv2d, x: torch.Tensor, segs: Segs, bn: Optional[nn.Module] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_rows for maps held at their width rounded up to 32 with exactly-zero pad channels (the MBConv trunk: widths 16 / 24 / 40 / 48 / 112 / 136 / ...):
    the weight is zero-padded inside the autograd graph -- columns up to x's width, rows up to round32(Cout) -- the folded BatchNorm with scale 1 / shift 0,
    a bias with 0, and the output KEEPS its padded width (its pad channels are zero again).  Autograd slices the parameter gradients back."""
    w, b = m.weight, m.bias
    Cout, Cin = w.shape[0], w.shape[1]
    pin, pout = x.shape[1] - Cin, round32(Cout) - Cout
    if pin < 0 or x.shape[1] % 32:
        raise FdError(f"conv_rows_wide: a {x.shape[1]}-channel map for a conv with {Cin} input channels (expected that width rounded up to 32)")
    if pin or pout:
        w = F.pad(w, (0, 0, 0, 0, 0, pin, 0, pout))
        b = F.pad(b, (0, pout)) if (b is not None and pout) else b
    scale = shift = None
    if bn is not None:
        scale, shift = _pad_affine(*_bn_fold(bn), pout)
    if b is not None:
        shift = b if scale is None else b * scale + shift
    return _ConvRows.apply(x, w, scale, shift, residual, segs, m.stride[0], _pad_of(m), m.dilation[0], ACT_NONE, amp_prec(), False)


def _mbconv_check(blk: nn.Module, x: torch.Tensor, segs: Segs, batch_stats: bool = False) -> None:
    bns = [blk._bn1, blk._bn2] + ([blk._bn0] if blk.expand != 1 else [])
    if batch_stats:
        if not all(_bn_train_wide_ok(b, x) for b in bns):
            raise FdError("MBConv: batch_stats=True needs every BatchNorm of the block in training mode with affine parameters and running statistics "
                          "(C % 4 == 0, C <= 4096)")
    elif not all(bn_is_frozen(b) for b in bns):
        raise FdError("MBConv: the HIP training nodes fold FROZEN BatchNorm layers only (batch statistics in the MBConv trunk are out of scope: "
                      "build the model with freeze_bn=True and keep the backbone's BatchNorm layers in eval mode)")
    convs = [blk._project_conv] + ([blk._expand_conv] if blk.expand != 1 else [])
    if not all(c.kernel_size == (1, 1) and c.stride == (1, 1) and c.groups == 1 and c.bias is None and c.weight.dtype == torch.float32 for c in convs):
        raise FdError("MBConv: 1x1 fp32 expand / project convs without bias expected")
    if x.dim() != 2 or x.shape[1] != round32(blk.cin) or not _f32(x) or segs.nseg != 1 or x.shape[0] != segs.rows:
        raise FdError(f"MBConv: block input must be single-level rows of width round32({blk.cin}) = {round32(blk.cin)} (got {tuple(x.shape)})")
    se_c, se_r = blk._se_reduce, blk._se_expand
    if se_c.bias is None or se_r.bias is None or round32(se_c.in_channels) > 4096 or se_c.out_channels > 1024:
        raise FdError("MBConv: squeeze-excitation with biases, at most 4096 channels and 1024 squeezed channels expected")


def mbconv_rows(blk: nn.Module, x: torch.Tensor, segs: Segs, batch_stats: bool = False, drop_scale: Optional[torch.Tensor] = None):
    """One MBConvBlock (efficientnet_pytorch 0.7.1, parameters in model/backbone/efficientnetv1._MBConv) on single-level rows held at widths rounded up to 32
    with zero pad channels, every op a differentiable HIP node: [expand 1x1 + bn0 -> swish] -> depthwise k x k + bn1 -> swish -> squeeze-excitation ->
    project 1x1 + bn2 (+ the block input when blk.skip).  Returns (rows of width round32(blk.cout), their Segs).  Frozen BatchNorm layers fold into the conv
    launches; with batch_stats=True (opt-in) the three BatchNorms run on batch statistics (batchnorm_train_wide_rows, the swish fused into it).
    drop_scale: the block's drop-connect scales [N] (drop_connect_scale; skip blocks only): the project conv + bn2 run without the fused residual and
    _SampleScaleAddRows computes branch * scale[n] + input.  What is not covered raises FdError: there is no stock fallback."""
    _mbconv_check(blk, x, segs, batch_stats)
    if drop_scale is not None and not blk.skip:
        raise FdError("MBConv: drop-connect applies to blocks with a skip connection only")
    N, (H, W) = segs.batch, segs.level_hw()[0]
    t = x
    if blk.expand != 1:
        if batch_stats:
            t = _bn_wide_rows(blk._bn0, conv_rows_wide(blk._expand_conv, x, segs), ACT_SILU)
        else:
            t = act_rows(conv_rows_wide(blk._expand_conv, x, segs, blk._bn0), ACT_SILU)
    if batch_stats:
        t = _bn_wide_rows(blk._bn1, dw_kxk_rows(blk._depthwise_conv, t, segs, blk.pad), ACT_SILU)
    else:
        t = act_rows(dw_kxk_rows(blk._depthwise_conv, t, segs, blk.pad, blk._bn1), ACT_SILU)
    K, s = blk.kernel, blk.stride
    Ho, Wo = (H + blk.pad[0] + blk.pad[1] - K) // s + 1, (W + blk.pad[0] + blk.pad[1] - K) // s + 1
    so = Segs.make(N, [(Ho, Wo)])
    padn = t.shape[1] - blk._se_reduce.in_channels
    w1, w2, b2 = blk._se_reduce.weight, blk._se_expand.weight, blk._se_expand.bias
    if padn:
        w1, w2, b2 = F.pad(w1, (0, 0, 0, 0, 0, padn)), F.pad(w2, (0, 0, 0, 0, 0, 0, 0, padn)), F.pad(b2, (0, padn))
    t = _SERows.apply(t, w1, blk._se_reduce.bias, w2, b2, N, Ho * Wo)
    if not batch_stats and drop_scale is None:
        return conv_rows_wide(blk._project_conv, t, so, blk._bn2, residual=x if blk.skip else None), so
    if batch_stats:
        t = _bn_wide_rows(blk._bn2, conv_rows_wide(blk._project_conv, t, so), ACT_NONE)
    else:
        t = conv_rows_wide(blk._project_conv, t, so, blk._bn2)
    if blk.skip:
        if drop_scale is None:
            drop_scale = torch.ones(N, dtype=torch.float32, device=t.device)
        t = _SampleScaleAddRows.apply(t, drop_scale, x, N, Ho * Wo)
    return t, so


# ------------------------------------------------------------------- modulated deformable conv (DeformableConv2d)
def _rv_or_copy(t: torch.Tensor) -> Rows:
    r = _rv(t)
    return r if r is not None else Rows(t.contiguous())


class _DeformCols(torch.autograd.Function):
    """The sampler of modulated deformable convolution: (x rows [B*H*W, C], offset rows [M, 2*K*K], mask rows [M, K*K] or None) -> columns
    [M, K*K*C] (fd_deform_im2col_nhwc; M = B*Ho*Wo).  offset / mask may be channel slices of one buffer (the merged side conv's output): they are read
    in place.  mask_act: `mask` holds the modulator's logits and 2 * sigmoid is applied inside, forward and backward.  Backward: fd_deform_bwd_nhwc --
    d_offset / d_mask deterministic, d_x scattered with fp32 atomics into a zeroed buffer.  fp32 under autocast, like the depthwise nodes."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, offset, mask, geom, mask_act):
        B, H, W, K, stride, pad, dil = geom
        x = x.contiguous()
        Ho, Wo = ops.deform_out_hw(H, W, K, stride, pad, dil)
        cols = torch.empty(B * Ho * Wo, K * K * x.shape[1], dtype=torch.float32, device=x.device)
        ops.deform_im2col(_r(x), _rv_or_copy(offset), _rv_or_copy(mask) if mask is not None else None, _r(cols), B, H, W, K, stride, pad, dil, mask_act)
        ctx.save_for_backward(x, offset, mask)
        ctx.geom, ctx.mask_act = geom, mask_act
        return cols

    @staticmethod
    @_bwd
    def backward(ctx, gcols):
        x, offset, mask = ctx.saved_tensors
        B, H, W, K, stride, pad, dil = ctx.geom
        g = resolve_pending(gcols).contiguous()
        M = g.shape[0]
        d_off = torch.empty(M, 2 * K * K, dtype=torch.float32, device=g.device)
        d_mask = torch.empty(M, K * K, dtype=torch.float32, device=g.device) if mask is not None else None
        d_x = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        ops.deform_bwd(_r(g), _r(x), _rv_or_copy(offset), _rv_or_copy(mask) if mask is not None else None, _r(d_off), _r(d_mask) if mask is not None else None,
                       _r(d_x) if d_x is not None else None, B, H, W, K, stride, pad, dil, ctx.mask_act)
        return d_x, d_off, d_mask, None, None


def deform_conv_rows(x: torch.Tensor, offset: torch.Tensor, mask: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, H: int,
                     W: int, stride: int, pad: int, dil: int, mask_act: bool = False) -> torch.Tensor:
    """Modulated deformable convolution on rows: x [B*H*W, C], offset [M, 2*K*K], mask [M, K*K] or None, weight [Cout, C, K, K] -> [M, Cout].  The sampler
    node writes the columns, the GEMM over them is the dense-conv node (_ConvRows: a 1x1 conv over K*K*C channels with weight.permute(0, 2, 3, 1), `bias`
    as its shift), so data gradient, weight gradient and the AMP operand precision are the dense conv's.  Cout is zero-padded to a multiple of 32 inside."""
    Cout, C, K, K2 = weight.shape
    if K != K2 or C % 32 or x.shape[1] != C or weight.dtype != torch.float32:
        raise FdError(f"deformable conv {tuple(weight.shape)} on {x.shape[1]} channels: square kernel, in_channels % 32 == 0, fp32 weights expected")
    if not all(_f32(t) for t in (x, offset, mask) if t is not None):
        raise FdError("deformable conv: fp32 input, offset and mask expected (or any float type under torch.autocast)")
    cols = _DeformCols.apply(x, offset, mask, (B, H, W, K, stride, pad, dil), mask_act)
    w = weight.permute(0, 2, 3, 1).reshape(Cout, K * K * C, 1, 1)
    padn = (-Cout) % 32
    if padn:
        w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, padn))
        bias = F.pad(bias, (0, padn)) if bias is not None else None
    Ho, Wo = ops.deform_out_hw(H, W, K, stride, pad, dil)
    y = _ConvRows.apply(cols, w, None, bias, None, Segs.make(B, [(Ho, Wo)]), 1, 0, 1, ACT_NONE, amp_prec(), False)
    return y[:, :Cout] if padn else y


def deformable_conv2d(m: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """DeformableConv2d.forward on NCHW-shaped x: offset_conv and modulator_conv as ONE launch (2*K*K + K*K channels padded to a multiple of 32), the sampler
    on two channel slices of that buffer (the modulator's 2 * sigmoid applied inside), the GEMM.  No host synchronisation: capturable in a HIP graph."""
    B, _, H, W = x.shape
    k, s, p = m.regular_conv.kernel_size[0], m.regular_conv.stride[0], m.regular_conv.padding[0]
    xr = to_rows(x)
    om = conv_rows(MergedConv(m.offset_conv, m.modulator_conv), xr, Segs.make(B, [(H, W)]), pad_out=True)
    y = deform_conv_rows(xr, om[:, :2 * k * k], om[:, 2 * k * k:], m.regular_conv.weight, m.regular_conv.bias, B, H, W, s, p, 1, mask_act=True)
    return from_rows(y, B, *ops.deform_out_hw(H, W, k, s, p, 1))


def mn_block_rows(blk: nn.Module, x: torch.Tensor, segs: Segs) -> torch.Tensor:
    """MNBlock (modules.py:195-216) on NHWC rows -- one level or a whole pyramid -- with every op a differentiable HIP node:
    x + PW2(SiLU(PW1(BN(dilated depthwise(x))))).  A frozen BatchNorm folds into the depthwise launch.  One in training mode runs on batch statistics
    (batchnorm_train_rows), PER LEVEL on slices of the rows when `segs` holds a pyramid: the reference calls a shared block once per level
    (MNFcos.py:285-297), so the statistics are per level and the running statistics move once per level, in level order."""
    dw, bn = blk.DilatedDepthWiseConv, blk.BN
    if not (_dense_ok(blk.PW1, x) and _dense_ok(blk.PW2, x) and blk.PW1.out_channels % 32 == 0 and blk.PW2.out_channels == x.shape[1]
            and blk.PW1.kernel_size == (1, 1) and blk.PW2.kernel_size == (1, 1) and isinstance(blk.ACT1, nn.SiLU)):
        raise FdError("MNBlock: the HIP training nodes cover fp32 1x1 convs with C % 32 == 0 and out_ch == in_ch (the residual add)")
    if bn_is_frozen(bn):
        t = dw_dilated_rows(dw, x, segs, bn)
    elif _bn_train_ok(bn, x):
        t = dw_dilated_rows(dw, x, segs)
        if segs.nseg == 1:
            t = batchnorm_train_rows(bn, t)
        else:
            per_level = t.split([segs.m_start[i + 1] - segs.m_start[i] for i in range(segs.nseg)], 0)
            t = torch.cat([batchnorm_train_rows(bn, u) for u in per_level], 0)
    else:
        raise FdError(f"MNBlock.BN ({type(bn).__name__}, training={bn.training}): the HIP nodes cover a frozen BatchNorm2d or one in training mode "
                      "with affine parameters, running statistics and C / 4 dividing 256")
    h = act_rows(conv_rows(blk.PW1, t, segs), ACT_SILU)
    return conv_rows(blk.PW2, h, segs, residual=x)


# --------------------------------------------------------------------------------------- GroupNorm + activation
class _GroupNormRows(torch.autograd.Function):
    @staticmethod
    @_fwd32
    def forward(ctx, x, gamma, beta, segs, G, eps, act):
        x = x.contiguous()
        y = torch.empty_like(x)
        ws = ops.groupnorm_workspace(segs, G, x.device)
        gm, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        ops.groupnorm_act(_r(x), gm, bt, _r(y), segs, G, act, ws, eps)
        ctx.save_for_backward(x, gm, bt, ws)
        ctx.geom = (segs, G, eps, act)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, gm, bt, ws = ctx.saved_tensors
        segs, G, eps, act = ctx.geom
        g = gy.contiguous()
        gx = torch.empty_like(x)
        dgamma, dbeta = ops.groupnorm_act_bwd(_r(x), _r(g), gm, bt, _r(gx), segs, G, act, ws, eps)
        return gx, dgamma, dbeta, None, None, None, None


def groupnorm_rows(gn: nn.GroupNorm, x: torch.Tensor, segs: Segs, act=ACT_NONE) -> torch.Tensor:
    """act(GroupNorm(x)) per (level, image) on a rows buffer: two HIP launches forward, three backward."""
    return _GroupNormRows.apply(x, gn.weight, gn.bias, segs, gn.num_groups, gn.eps, _act_id(act))


# ------------------------------------------------------------------- elementwise / pooling / SE / BatchNorm(train) nodes
def relu_mask(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """g * [y > 0] on contiguous rows (the ReLU backward from the saved OUTPUT), one HIP launch."""
    out = torch.empty_like(g)
    ops.act_bwd(_r(y), _r(g), _r(out), ACT_RELU)
    return out


class _ActRows(torch.autograd.Function):
    """y = act(x) on rows with the INPUT saved: SiLU after a BatchNorm (HISFcos.py:100,112) needs the pre-activation."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, act):
        xr = _rv(x)                           # (a channel slice of a wider rows buffer is read in place)
        if xr is None:
            x = x.contiguous()
            xr = _r(x)
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ops.act(xr, _r(y), act)
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ops.act_bwd(_rv(x), _r(gy.contiguous()), _r(gx), ctx.act)
        return gx, None


def act_rows(x: torch.Tensor, act: int) -> torch.Tensor:
    return x if act == ACT_NONE else _ActRows.apply(x, act)


class _PoolAddRows(torch.autograd.Function):
    """y = max_pool2d(x, k, s, pad) (+ add) on single-level rows (FPN down_sample + torch.add, HISFcos.py:131-136,168-177)."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, add, geom):
        B, H, W, k, s, pad = geom
        x = x.contiguous()
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        y = torch.empty(B * Ho * Wo, x.shape[1], dtype=torch.float32, device=x.device)
        ops.maxpool(_r(x), _r(y), B, H, W, k, s, pad, add=_r(add.contiguous()) if add is not None else None)
        ctx.save_for_backward(x)
        ctx.geom = geom
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        B, H, W, k, s, pad = ctx.geom
        g = gy.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            ops.maxpool_bwd(_r(x), _r(g), _r(gx), B, H, W, k, s, pad)
        return gx, (g if ctx.needs_input_grad[1] else None), None


class _UpAddRows(torch.autograd.Function):
    """y = nearest_upsample_x2(x) + lat on single-level rows (HISFcos.py:155-165)."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, lat, geom):
        B, H, W = geom                       # geometry of the LOW-resolution input x
        y = torch.empty_like(lat)
        ops.upsample2x_add(_r(x.contiguous()), _r(lat.contiguous()), _r(y), B, H, W)
        ctx.geom = geom
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        B, H, W = ctx.geom
        g = gy.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(B * H * W, g.shape[1], dtype=torch.float32, device=g.device)
            ops.upsample2x_bwd(_r(g), _r(gx), B, H, W)
        return gx, (g if ctx.needs_input_grad[1] else None), None


class _SERows(torch.autograd.Function):
    """SEBlock (modules.py:107-121) on rows: y = x * sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2), forward and backward on HIP."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, w1, b1, w2, b2, B, HW):
        x = x.contiguous()
        Cc, Cr = x.shape[1], w1.shape[0]
        y = torch.empty_like(x)
        ws = ops.se_workspace(B, HW, Cc, x.device)
        w1f, w2f = w1.detach().reshape(Cr, Cc).contiguous(), w2.detach().reshape(Cc, Cr).contiguous()
        b1f, b2f = b1.detach().contiguous(), b2.detach().contiguous()
        ops.se_scale(_r(x), w1f, b1f, w2f, b2f, _r(y), B, HW, Cr, ws)
        ctx.save_for_backward(x, w1f, b1f, w2f, b2f, ws)
        ctx.geom = (B, HW, Cr, tuple(w1.shape), tuple(w2.shape))
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, w1f, b1f, w2f, b2f, ws = ctx.saved_tensors
        B, HW, Cr, s1, s2 = ctx.geom
        gx = torch.empty_like(x)
        dw1, db1, dw2, db2 = ops.se_scale_bwd(_r(x), _r(gy.contiguous()), w1f, b1f, w2f, b2f, _r(gx), B, HW, Cr, ws)
        return gx, dw1.view(s1), db1, dw2.view(s2), db2, None, None


def se_rows(se: nn.Module, x: torch.Tensor, B: int, HW: int) -> torch.Tensor:
    ex = se.excitation
    return _SERows.apply(x, ex[0].weight, ex[0].bias, ex[2].weight, ex[2].bias, B, HW)


def _se_ok(se: nn.Module, x: torch.Tensor) -> bool:
    ex = getattr(se, "excitation", None)
    return (not _STOCK and ex is not None and len(ex) == 4 and isinstance(ex[1], nn.SiLU) and isinstance(ex[3], nn.Sigmoid)
            and ex[0].bias is not None and ex[2].bias is not None and ex[0].in_channels % 4 == 0 and ex[0].in_channels <= 4096
            and ex[0].out_channels <= 1024 and _f32(x))


class _BatchNormTrainRows(torch.autograd.Function):
    """nn.BatchNorm2d in TRAINING mode + ReLU / SiLU on rows.  Batch statistics per channel over all rows are GroupNorm
    statistics of ONE image with G = C groups, so forward / backward are the GroupNorm kernels (fp64 partial sums in fixed
    order); the running statistics are updated like nn.BatchNorm2d does (momentum, unbiased variance)."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, gamma, beta, rmean, rvar, momentum, eps, act):
        x = x.contiguous()
        rows, Cc = x.shape
        segs = Segs.make(1, [(rows, 1)])
        y = torch.empty_like(x)
        ws = ops.groupnorm_workspace(segs, Cc, x.device)
        gm, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        ops.groupnorm_act(_r(x), gm, bt, _r(y), segs, Cc, act, ws, eps)
        if rmean is not None and momentum is not None:
            ops.batchnorm_update_running(ws, rows, Cc, momentum, eps, rmean, rvar)
        ctx.save_for_backward(x, gm, bt, ws)
        ctx.geom = (segs, eps, act)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x, gm, bt, ws = ctx.saved_tensors
        segs, eps, act = ctx.geom
        gx = torch.empty_like(x)
        dgamma, dbeta = ops.groupnorm_act_bwd(_r(x), _r(gy.contiguous()), gm, bt, _r(gx), segs, x.shape[1], act, ws, eps)
        return gx, dgamma, dbeta, None, None, None, None, None


# ---- nn.SyncBatchNorm: statistics collectives OFF the critical path (round 4) ----
# A layer's statistics cannot be batched with another layer's (data dependence), but the all-reduce need not be WAITED for where it is issued:
#   forward   syncbn_begin() runs phase 1 (this rank's fp64 sums) and issues the all-reduce with async_op=True; the caller enqueues whatever does not
#             depend on the normalised tensor (HisBlock: conv2(x) beside bn1, the SE branch beside bn2; the FPN laterals beside the previous block),
#             then syncbn_finish() waits and runs phase 2.
#   backward  the node issues the all-reduce of (sum dz, sum dz * xhat) asynchronously too and -- when its caller has promised that the ONLY consumer of
#             its input gradient is one of this module's conv nodes (`defer`) -- returns that gradient UNFINISHED with a pending entry; the consumer
#             resolves it (wait + phase 2, same stream) on entry.  Autograd runs the nodes created between begin() and finish() in between (bn1's
#             all-reduce flies under conv2's data / weight gradient kernels, bn2's under the SE backward).
# With RCCL the collective runs on its own stream and wait() is a stream dependency; with gloo (tests) wait() blocks the host after the independent
# launches were enqueued.  SYNC_TRACE records, per collective, how many HIP launches were enqueued between issue and wait (tests assert on it).
SYNC_TRACE = collections.deque(maxlen=4096)      # (bounded: a long multi-rank run appends ~200 entries per step; only tests read it)
# Unfinished input gradients of deferred SyncBatchNorm backward nodes: data_ptr -> (autograd graph-task id of the backward pass that deferred it, closure that
# finishes it).  The task id ties an entry to ITS pass: what a pass that raised before its flush left behind is never applied to a later pass's gradient that
# happens to reuse the address, and is dropped when the next pass defers its first gradient.
_PENDING: dict = {}


def _task_id() -> int:
    return torch._C._current_graph_task_id()


def resolve_pending(g: torch.Tensor) -> torch.Tensor:
    """Called by the conv nodes' backward on their incoming gradient: finishes it if a SyncBatchNorm node of THIS backward pass deferred its second phase."""
    if _PENDING:
        e = _PENDING.get(g.data_ptr())
        if e is not None and e[0] == _task_id():
            del _PENDING[g.data_ptr()]
            e[1]()
    return g


def flush_pending() -> None:
    """Finish every gradient this pass deferred and nobody resolved (safety net, queued at the end of EVERY backward pass that deferred one); entries of other
    (failed) passes are dropped unfinished."""
    tid = _task_id()
    while _PENDING:
        _, (t, fin) = _PENDING.popitem()
        if t == tid or tid < 0:          # (tid < 0: the engine runs the callback outside the task -- finishing a leftover writes its own, dead tensor: harmless)
            fin()


class _SyncHandle:
    __slots__ = ("bn", "x", "act", "group", "buf", "ws", "work", "launches_at_issue", "defer", "wide", "fwd", "bwd", "res_fwd", "f16")


# THE place the synchronised code looks at the kernel family, keyed by syncbn_begin's `wide`: the family's two-phase forward and backward wrappers (both
# pairs take the same arguments) and the forward's residual form where the family has one
_SYNC_KERNELS = {False: (ops.batchnorm_sync_fwd, ops.batchnorm_sync_bwd, None),
                 True: (ops.batchnorm_train_sync_fwd, ops.batchnorm_train_sync_bwd, ops.batchnorm_train_sync_res_fwd)}


def syncbn_begin(bn: nn.Module, x: torch.Tensor, act: int = ACT_NONE, defer_backward: bool = False, wide: bool = False,
                 f16: bool = False) -> "_SyncHandle":
    """Phase 1 of nn.SyncBatchNorm's forward on rows + the asynchronous all-reduce of the [2C + 1] fp64 buffer (sums and row count).  wide: the any-width
    kernel family (fd_batchnorm_train_sync_*; check with _bn_train_wide_ok) on the C-channel view of x [rows, Cw >= C] -- the MBConv trunk's round32(C) maps
    with zero pad channels, which the output and the input gradient keep; otherwise the GroupNorm-route family (fd_batchnorm_sync_*; _bn_train_ok), whose
    callers pass x [rows, C].  Everything behind the choice of the wrappers -- the collective, the handle, SYNC_TRACE, the deferred backward -- is the same.
    f16 (wide only; _bn_f16_ok): x is read as an f16 map and syncbn_finish gives the f16-map node (_SyncBatchNormApplyH); the all-reduced buffer is the
    same fp64 one."""
    import torch.distributed as dist
    if f16 and not wide:
        raise FdError("syncbn_begin(f16=True): the f16-map kernels are the any-width family's (wide=True)")
    h = _SyncHandle()
    h.bn, h.act, h.defer, h.wide, h.f16 = bn, act, defer_backward, wide, f16
    h.fwd, h.bwd, h.res_fwd = _SYNC_KERNELS[wide]          # (everything below calls these: `wide` itself is read nowhere else)
    h.group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    with torch.no_grad():
        xd = (_as_f16(x.detach()) if f16 else x.detach().float()).contiguous()
        rows, Cc = xd.shape[0], bn.num_features
        if xd.shape[1] < Cc or xd.shape[1] % 4:
            raise FdError(f"SyncBatchNorm({Cc}) on rows of shape {tuple(x.shape)}: rows of at least {Cc} channels (a multiple of 4) expected")
        h.buf = torch.empty(2 * Cc + 1, dtype=torch.float64, device=xd.device)
        h.ws = h.fwd(1, Rows(xd, 0, Cc), h.buf, act_id=act)
        h.buf[2 * Cc] = float(rows)                               # this rank's row count rides behind the 2C sums (a device-side fill, no sync)
        h.work = dist.all_reduce(h.buf, group=h.group, async_op=True)       # THE forward collective of this layer (C3), not waited for here
    h.x = x
    h.launches_at_issue = ops.LAUNCHES[0]
    return h


def syncbn_finish(h: "_SyncHandle", res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Phase 2.  res (wide handles, act NONE / ReLU): act(bn(x) + res) in the apply pass, the residual form."""
    bn = h.bn
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if res is not None and (h.res_fwd is None or h.defer):
        raise FdError("syncbn_finish(res=...): the residual form exists for the any-width kernels (wide=True) without a deferred backward")
    node = _SyncBatchNormApplyH if h.f16 else _SyncBatchNormApply
    return node.apply(h.x, bn.weight, bn.bias, res, bn.running_mean, bn.running_var, _bn_momentum(bn), bn.eps, h.act, h)


def _syncbn_backward(x, g, gm, bt, ws, buf, eps, act, group, defer, bwd):
    """The backward of a SyncBatchNorm node on the contiguous incoming gradient g: phase 1 (this rank's sums, dgamma, dbeta), the asynchronous all-reduce,
    and phase 2 -- run here, or left pending for the consuming conv node when `defer`.  bwd: the family's wrapper.  Returns (gx, dgamma, dbeta)."""
    import torch.distributed as dist
    Cc = gm.numel()
    gx = (torch.zeros if x.shape[1] != Cc else torch.empty)(x.shape, dtype=x.dtype, device=x.device)        # (the saved map's type: fp32, f16 in the `H` nodes)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    sums = torch.empty(2 * Cc + 1, dtype=torch.float64, device=x.device)       # [sum dz | sum dz * xhat | global row count]
    xr, gr = Rows(x, 0, Cc), Rows(g, 0, Cc)
    bws = bwd(1, xr, gr, gm, bt, sums, ws, None, dgamma, dbeta, eps, act)
    sums[2 * Cc:].copy_(buf[2 * Cc:])                       # the forward's all-reduced row count, device to device (its own slot: not all-reduced again)
    work = dist.all_reduce(sums[:2 * Cc], group=group, async_op=True)     # THE backward collective of this layer
    at_issue = ops.LAUNCHES[0]

    def finish(xr=xr, gr=gr, gm=gm, bt=bt, gx=gx, sums=sums, ws=ws, bws=bws, work=work):
        SYNC_TRACE.append(("bwd", ops.LAUNCHES[0] - at_issue))
        work.wait()
        bwd(2, xr, gr, gm, bt, sums, ws, Rows(gx, 0, Cc), None, None, eps, act, -1.0, ws=bws)

    if defer:
        # the ONLY consumer of gx is one of this module's conv nodes (conv_norm_begin built the chain): it finishes gx on entry (resolve_pending);
        # the nodes autograd runs before it are enqueued under the collective.  flush_pending at the end of the pass is the safety net.
        tid = _task_id()
        for k in [k for k, e in _PENDING.items() if e[0] != tid]:      # leftovers of a pass that raised before its flush
            del _PENDING[k]
        torch.autograd.Variable._execution_engine.queue_callback(flush_pending)      # always: a stale entry must not suppress this pass's flush
        _PENDING[gx.data_ptr()] = (tid, finish)
    else:
        finish()
    return gx, dgamma, dbeta


def _as_f16(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """An operand of an f16-map node as f16: taken as it is when its producer stored f16 (the case the bottleneck path arranges), else one conversion pass."""
    return t if t is None or t.dtype == torch.float16 else t.to(torch.float16)


def _bn_node_begin(x, gamma, beta, res):
    """What the batch-statistics nodes' forwards start with: contiguous inputs, the C-channel views of x and of an output of x's width and element type (a map
    held wider than C keeps exactly-zero pad channels), detached affine parameters."""
    x = x.contiguous()
    Cc = gamma.numel()
    y = (torch.zeros if x.shape[1] != Cc else torch.empty)(x.shape, dtype=x.dtype, device=x.device)
    return x, y, Rows(x, 0, Cc), Rows(y, 0, Cc), (_r(res.contiguous()) if res is not None else None), gamma.detach().contiguous(), beta.detach().contiguous()


def _bn_node_grad(gy, y, st=torch.float32):
    """The incoming gradient of a batch-statistics node, finished and contiguous, in the node's map type `st`; y (the saved output of a residual form with
    ReLU): times [y > 0], which is the residual's gradient AND the dz of a BatchNorm without activation."""
    g = resolve_pending(gy).contiguous()
    if g.dtype != st:
        g = g.to(st)
    return g if y is None else relu_mask(g, y)


class _SyncBatchNormApply(torch.autograd.Function):
    """Second half of nn.SyncBatchNorm in TRAINING mode + ReLU / SiLU on rows (train.py:101-103 converts the model after the DDP wrap): waits for the
    all-reduce syncbn_begin issued, normalises with the GLOBAL statistics, updates the running statistics with the global row count -- read ON THE
    DEVICE from the all-reduced buffer: ranks whose batches are padded to different H x W hold different row counts (dataset/voc.py:141-171).  Like
    torch's SyncBatchNorm the affine gradients come from the local sums (DDP averages them).  res (or None): the residual form act(bn(x) + res), act NONE /
    ReLU, _BatchNormResRows across ranks -- phase 1 never read the residual; its backward is the mask pass, then the plain backward with ACT_NONE."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act, h):
        return _syncbn_apply_forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act, h)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        return _syncbn_apply_backward(ctx, gy)


def _syncbn_apply_forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act, h):
    """The forward of _SyncBatchNormApply and, on f16 maps, _SyncBatchNormApplyH (the wrappers pick the entry point by the maps' type)."""
    x, y, xr, yr, rr, gm, bt = _bn_node_begin(x, gamma, beta, res)
    SYNC_TRACE.append(("fwd", ops.LAUNCHES[0] - h.launches_at_issue))
    h.work.wait()
    # statistics, running statistics (global count from buf[2C] on the device) and apply in one call
    if rr is None:
        h.fwd(2, xr, h.buf, gm, bt, yr, eps, act, -1.0, momentum, rmean, rvar, ws=h.ws)
    else:
        h.res_fwd(2, xr, h.buf, gm, bt, rr, yr, eps, act, -1.0, momentum, rmean, rvar, ws=h.ws)
    ctx.save_for_backward(x, gm, bt, h.ws, h.buf, y if rr is not None and act == ACT_RELU else None)
    ctx.geom = (eps, act if rr is None else ACT_NONE, h.group, h.defer, h.bwd)
    return y


def _syncbn_apply_backward(ctx, gy):
    x, gm, bt, ws, buf, y = ctx.saved_tensors
    g = _bn_node_grad(gy, y, x.dtype)
    gx, dgamma, dbeta = _syncbn_backward(x, g, gm, bt, ws, buf, *ctx.geom)
    return gx, dgamma, dbeta, (g if ctx.needs_input_grad[3] else None), None, None, None, None, None, None


class _SyncBatchNormApplyH(torch.autograd.Function):
    """_SyncBatchNormApply on f16 MAPS (fd_batchnorm_train_sync_*_nhwc_h; the bottleneck path's opt-in f16_maps under torch.autocast(float16)): no cast on
    entry -- x, the residual and the output are f16, the incoming gradient is taken as f16, dx and the residual's gradient are f16; gamma / beta and their
    gradients, the running statistics and the all-reduced fp64 sums are the fp32 node's.  The deferred backward works as there."""

    @staticmethod
    @_fwd_keep
    def forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act, h):
        return _syncbn_apply_forward(ctx, _as_f16(x), gamma, beta, _as_f16(res), rmean, rvar, momentum, eps, act, h)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        return _syncbn_apply_backward(ctx, gy)


def _bn_momentum(bn: nn.Module):
    """What the batch-statistics nodes carry to the kernels as the blend factor of bn's running statistics: the float momentum, or for momentum=None (the
    cumulative moving average, 1 / num_batches_tracked) the LIVE counter tensor -- the `_cma` entry points read it on the device behind the add_(1) the
    caller has enqueued.  The wrappers take its address in every call and nothing is cached, so a captured forward follows the counter."""
    if bn.momentum is not None:
        return bn.momentum
    if getattr(bn, "num_batches_tracked", None) is None:
        raise FdError(f"{type(bn).__name__}({bn.num_features}) with momentum=None has no num_batches_tracked: the cumulative average needs the counter")
    return bn.num_batches_tracked


def _bn_train_wide_ok(bn: nn.Module, x: torch.Tensor) -> bool:
    """A BatchNorm in training mode that batchnorm_train_wide_rows takes: any width C % 4 == 0 up to 4096 (x may be held wider)."""
    Cc = getattr(bn, "num_features", 0)
    return (not _STOCK and isinstance(bn, BN_TYPES) and bn.training and bn.affine and bn.track_running_stats
            and Cc % 4 == 0 and 4 <= Cc <= 4096 and _f32(x))


def _bn_train_ok(bn: nn.Module, x: torch.Tensor) -> bool:
    """One that batchnorm_train_rows takes: the widths of the GroupNorm-route kernels, C / 4 dividing 256 (so C <= 1024)."""
    return _bn_train_wide_ok(bn, x) and 256 % (bn.num_features // 4) == 0


BN_NARROW, BN_WIDE = "narrow", "wide"


def _bn_family(bn: nn.Module, x: torch.Tensor) -> Optional[str]:
    """The kernel family that runs `bn` on batch statistics: BN_NARROW (the GroupNorm route, batchnorm_train_rows) where its widths allow, else BN_WIDE (the
    any-width kernels, _bn_wide_rows), None: not covered.  THE place this is decided."""
    return BN_NARROW if _bn_train_ok(bn, x) else BN_WIDE if _bn_train_wide_ok(bn, x) else None


def batchnorm_train_rows(bn: nn.Module, x: torch.Tensor, act: int = ACT_NONE) -> torch.Tensor:
    """act(bn(x)) with batch statistics on rows; bn.running_mean / running_var / num_batches_tracked are updated in place like
    nn.BatchNorm2d does (check with _bn_train_ok).  An nn.SyncBatchNorm in an initialised process group of more than one rank
    takes its statistics over all ranks (_SyncBatchNormTrainRows: one all-reduce forward, one backward)."""
    if _is_sync(bn):
        return syncbn_finish(syncbn_begin(bn, x, act))          # one-shot form: nothing enqueued between issue and wait
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return _BatchNormTrainRows.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, _bn_momentum(bn), bn.eps, act)


def _is_sync(bn: nn.Module) -> bool:
    """An nn.SyncBatchNorm in an initialised process group of more than one rank (its statistics span all ranks)."""
    import torch.distributed as dist
    if isinstance(bn, nn.SyncBatchNorm) and dist.is_available() and dist.is_initialized():
        group = bn.process_group if bn.process_group is not None else dist.group.WORLD
        return dist.get_world_size(group) > 1
    return False


def _bn_wide_forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act):
    """The forward of _BatchNormWideRows (res None) and _BatchNormResRows; the backward below is the plain one, in the residual form with ACT_NONE on the
    gradient that the saved output masked."""
    x, y, xr, yr, rr, gm, bt = _bn_node_begin(x, gamma, beta, res)
    if rr is None:
        ws = ops.batchnorm_train_fwd(xr, gm, bt, yr, eps, act, momentum, rmean, rvar)
    else:
        ws = ops.batchnorm_train_res_fwd(xr, gm, bt, rr, yr, eps, act, momentum, rmean, rvar)
    ctx.save_for_backward(x, gm, bt, ws, y if rr is not None and act == ACT_RELU else None)
    ctx.geom = (eps, act if rr is None else ACT_NONE)
    return y


def _bn_wide_backward(ctx, gy):
    """Returns (g, gx, dgamma, dbeta): g is the residual's gradient too."""
    x, gm, bt, ws, y = ctx.saved_tensors
    eps, act = ctx.geom
    Cc = gm.numel()
    g = _bn_node_grad(gy, y, x.dtype)
    gx = (torch.zeros if x.shape[1] != Cc else torch.empty)(x.shape, dtype=x.dtype, device=x.device)
    dgamma, dbeta = ops.batchnorm_train_bwd(Rows(x, 0, Cc), Rows(g, 0, Cc), gm, bt, Rows(gx, 0, Cc), eps, act, ws)
    return g, gx, dgamma, dbeta


class _BatchNormWideRows(torch.autograd.Function):
    """nn.BatchNorm2d in TRAINING mode + ReLU / SiLU at ANY width C % 4 == 0 up to 4096 (fd_batchnorm_train_fwd_nhwc / _bwd_nhwc), on the real-width view of a
    map that may be held wider (the MBConv trunk: round32(C) with zero pad channels): x [rows, Cw >= C], gamma / beta [C].  The output and the input gradient
    have x's width and exactly-zero pad channels.  fp32 under autocast, like the other normalisation nodes."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, gamma, beta, rmean, rvar, momentum, eps, act):
        return _bn_wide_forward(ctx, x, gamma, beta, None, rmean, rvar, momentum, eps, act)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        _, gx, dgamma, dbeta = _bn_wide_backward(ctx, gy)
        return gx, dgamma, dbeta, None, None, None, None, None


class _BatchNormWideRowsH(torch.autograd.Function):
    """_BatchNormWideRows on f16 MAPS (fd_batchnorm_train_fwd_nhwc_h / _bwd_nhwc_h; the bottleneck path's opt-in f16_maps under torch.autocast(float16)): no
    cast on entry -- the forward reads the f16 x, stores an f16 y and saves the f16 x; the backward takes an f16 gradient and returns an f16 dx.  The
    arithmetic is the fp32 node's on the upcast map, rounded once at the store; dgamma / dbeta and the running statistics stay fp32."""

    @staticmethod
    @_fwd_keep
    def forward(ctx, x, gamma, beta, rmean, rvar, momentum, eps, act):
        return _bn_wide_forward(ctx, _as_f16(x), gamma, beta, None, rmean, rvar, momentum, eps, act)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        _, gx, dgamma, dbeta = _bn_wide_backward(ctx, gy)
        return gx, dgamma, dbeta, None, None, None, None, None


def _f16_maps_on(f16_maps: bool) -> bool:
    """The bottleneck path's opt-in f16_maps takes effect: torch.autocast(float16) on nodes that store f16 maps (amp_prec, AMP_F16_STORE).  THE place."""
    return f16_maps and AMP_F16_STORE and amp_prec() == _lib.PREC_F16


def _bn_f16_ok(bn: nn.Module, f16_maps: bool) -> bool:
    """`bn` (in training mode, covered by the any-width kernels) runs on f16 maps: _f16_maps_on and a float momentum -- the cumulative moving average
    (momentum=None) has no f16 form and keeps the fp32 node."""
    return _f16_maps_on(f16_maps) and bn.momentum is not None


def batchnorm_train_wide_rows(bn: nn.Module, x: torch.Tensor, act: int = ACT_NONE, f16: bool = False) -> torch.Tensor:
    """act(bn(x)) with batch statistics on rows at any width C % 4 == 0 up to 4096 (check with _bn_train_wide_ok); x is [rows, C] or a map held at
    round32(C) with zero pad channels, which the output keeps.  Running statistics and num_batches_tracked move like nn.BatchNorm2d's.  This is the
    UNSYNCHRONISED entry point: an nn.SyncBatchNorm spanning more than one rank raises here.  Its synchronised form is syncbn_begin(..., wide=True) /
    syncbn_finish (fd_batchnorm_train_sync_*), which the callers pick through _bn_wide_rows before this function is reached.  f16 (_bn_f16_ok): the f16-map
    node, f16 in and out."""
    Cc = bn.num_features
    if _is_sync(bn):
        raise FdError(f"SyncBatchNorm({Cc}) over more than one rank: the batch-statistics kernels for widths outside C / 4 dividing 256, C <= 1024 "
                      "(fd_batchnorm_train_*) have no synchronised form; keep this layer an nn.BatchNorm2d or freeze it")
    if x.dim() != 2 or x.shape[1] < Cc or x.shape[1] % 4 or x.shape[0] < 2:
        raise FdError(f"batch-statistics BatchNorm({Cc}) on rows of shape {tuple(x.shape)}: at least 2 rows of at least {Cc} channels (a multiple of 4) expected")
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    node = _BatchNormWideRowsH if f16 else _BatchNormWideRows
    return node.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, _bn_momentum(bn), bn.eps, act)


def _bn_wide_rows(bn: nn.Module, x: torch.Tensor, act: int = ACT_NONE, f16: bool = False) -> torch.Tensor:
    """batchnorm_train_wide_rows, or for an nn.SyncBatchNorm spanning ranks its synchronised form in one shot (the MBConv chain is strictly sequential:
    nothing independent exists to enqueue under the collective).  f16: on f16 maps."""
    if _is_sync(bn):
        return syncbn_finish(syncbn_begin(bn, x, act, wide=True, f16=f16))
    return batchnorm_train_wide_rows(bn, x, act, f16)


class _BatchNormResRows(torch.autograd.Function):
    """act(bn(x) + res) with nn.BatchNorm2d in TRAINING mode, act NONE / ReLU, at any width C % 4 == 0 up to 4096 on [rows, C] maps: the output of a ResNet
    bottleneck, relu(bn3(conv3(y2)) + identity), with the add and the ReLU in the apply pass (fd_batchnorm_train_res_fwd_nhwc).  Backward: g = gy * [y > 0]
    (one mask pass over the saved output) is the residual's gradient AND the dz of a BatchNorm without activation, so fd_batchnorm_train_bwd_nhwc with ACT_NONE
    on g gives dx, dgamma, dbeta.  fp32 under autocast, like the other normalisation nodes."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act):
        return _bn_wide_forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        g, gx, dgamma, dbeta = _bn_wide_backward(ctx, gy)
        return gx, dgamma, dbeta, (g if ctx.needs_input_grad[3] else None), None, None, None, None, None


class _BatchNormResRowsH(torch.autograd.Function):
    """_BatchNormResRows on f16 MAPS (fd_batchnorm_train_res_fwd_nhwc_h, fd_batchnorm_train_bwd_nhwc_h): no cast on entry -- x, the residual and the output
    are f16 and the f16 x and y are saved; the backward takes an f16 gradient, runs the mask pass on the f16 activation backward (fd_act_bwd_nhwc_h) and
    returns an f16 dx and the f16 residual gradient; dgamma / dbeta stay fp32."""

    @staticmethod
    @_fwd_keep
    def forward(ctx, x, gamma, beta, res, rmean, rvar, momentum, eps, act):
        return _bn_wide_forward(ctx, _as_f16(x), gamma, beta, _as_f16(res), rmean, rvar, momentum, eps, act)

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        g, gx, dgamma, dbeta = _bn_wide_backward(ctx, gy)
        return gx, dgamma, dbeta, (g if ctx.needs_input_grad[3] else None), None, None, None, None, None


def batchnorm_train_res_rows(bn: nn.Module, x: torch.Tensor, res: torch.Tensor, act: int = ACT_RELU, f16: bool = False) -> torch.Tensor:
    """act(bn(x) + res) with batch statistics on [rows, C] maps, act NONE / ReLU, any width C % 4 == 0 up to 4096 (check with _bn_train_wide_ok): one-shot,
    and for an nn.SyncBatchNorm spanning ranks through its synchronised form.  Gradients for x, gamma, beta and res; running statistics and
    num_batches_tracked move like nn.BatchNorm2d's.  f16 (_bn_f16_ok): the f16-map nodes -- x, res and the output are f16."""
    Cc = getattr(bn, "num_features", 0)
    if act not in (ACT_NONE, ACT_RELU):
        raise FdError("batchnorm_train_res_rows differentiates ACT_NONE / ACT_RELU only (the backward takes its mask from the output)")
    if not _bn_train_wide_ok(bn, x):
        raise FdError(f"batchnorm_train_res_rows: {type(bn).__name__}({Cc}) must be a BatchNorm in training mode with affine parameters, running statistics, "
                      "C % 4 == 0, 4 <= C <= 4096, on floating-point rows")
    if x.dim() != 2 or x.shape[1] != Cc or tuple(res.shape) != tuple(x.shape):
        raise FdError(f"batchnorm_train_res_rows: BatchNorm({Cc}) on rows of shape {tuple(x.shape)} with a residual of shape {tuple(res.shape)}: "
                      f"two [rows, {Cc}] maps expected")
    if _is_sync(bn):
        return syncbn_finish(syncbn_begin(bn, x, act, wide=True, f16=f16), res)
    if x.shape[0] < 2:
        raise FdError(f"batchnorm_train_res_rows: batch statistics need at least 2 rows (got {x.shape[0]})")
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    node = _BatchNormResRowsH if f16 else _BatchNormResRows
    return node.apply(x, bn.weight, bn.bias, res, bn.running_mean, bn.running_var, _bn_momentum(bn), bn.eps, act)


class _SampleScaleAddRows(torch.autograd.Function):
    """y = a * s[n] + r on single-level rows [N * HW, C] (fd_sample_scale_add_nhwc): the drop-connect of an MBConv skip block -- a = the branch, r = the block
    input, s = N fp32 on the device (0 or 1 / (1 - p)).  Backward: the branch's gradient is the same launch on the incoming gradient without r, the skip
    path's is the incoming gradient itself."""

    @staticmethod
    @_fwd32
    def forward(ctx, a, s, r, N, HW):
        a, r, s = a.contiguous(), r.contiguous(), s.detach().float().contiguous()
        y = torch.empty_like(a)
        ops.sample_scale_add(_r(a), s, _r(r), _r(y), N, HW)
        ctx.save_for_backward(s)
        ctx.geom = (N, HW)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        s, = ctx.saved_tensors
        N, HW = ctx.geom
        g = resolve_pending(gy).contiguous()
        ga = None
        if ctx.needs_input_grad[0]:
            ga = torch.empty_like(g)
            ops.sample_scale_add(_r(g), s, None, _r(ga), N, HW)
        return ga, None, (g if ctx.needs_input_grad[2] else None), None, None


def drop_connect_scale(p: float, u: torch.Tensor) -> torch.Tensor:
    """efficientnet_pytorch's drop_connect mask from uniform numbers u [B] on the device: floor((1 - p) + u) / (1 - p), 0 or 1 / (1 - p) per sample."""
    keep = 1.0 - p
    return torch.floor(keep + u.detach().float()) / keep


class _Stem3Rows(torch.autograd.Function):
    """_conv_stem (3x3 stride 2, 3 -> C0, static "SAME" padding, no bias) of the EfficientNet trunk on an NCHW fp32 image batch that needs no gradient, as rows
    [B * h * w, round32(C0)] with zero pad channels: z = conv(x, w) * scale + shift, scale / shift the constants of a frozen _bn0 or None (the raw conv in
    front of a BatchNorm on batch statistics).  No activation: the swish behind it is an act_rows node that keeps z.  Forward fd_nchw3_to_nhwc4 +
    fd_stem_conv_nhwc4, backward fd_stem_conv_bwd_weight_nhwc4; there is no data gradient.  fp32 under autocast."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, weight, scale, shift, geom):
        pad, h, w = geom
        B, _, H, W = x.shape
        C0 = weight.shape[0]
        x4 = torch.empty(B * H * W, 4, dtype=torch.float32, device=x.device)
        ops.nchw3_to_nhwc4(x.contiguous(), x4)
        y = (torch.zeros if round32(C0) != C0 else torch.empty)(B * h * w, round32(C0), dtype=torch.float32, device=x.device)
        ops.stem_conv3(x4, ops.pack_stem3_weight(weight.detach()), Rows(y, 0, C0), B, H, W, 3, 2, pad, pad, h, w, scale, shift, ACT_NONE)
        ctx.save_for_backward(x4, scale)
        ctx.geom = (B, H, W, C0, pad, h, w)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x4, scale = ctx.saved_tensors
        B, H, W, C0, pad, h, w = ctx.geom
        gw = None
        if ctx.needs_input_grad[1]:
            g = resolve_pending(gy).contiguous()
            gw = ops.stem_conv3_wgrad(x4, Rows(g, 0, C0), B, H, W, 3, 2, pad, pad, h, w, scale)
        return None, gw, None, None, None


def effnet_stem_rows(net: nn.Module, x: torch.Tensor, h: int, w: int, batch_stats: bool) -> torch.Tensor:
    """swish(_bn0(_conv_stem(x))) of a TRAINABLE EfficientNet stem as rows of width round32(C0): _Stem3Rows with a frozen _bn0 folded into the launch, or the
    raw conv + batchnorm_train_wide_rows when _bn0 runs on batch statistics; the swish is an act_rows node in both cases."""
    m, bn = net._conv_stem, net._bn0
    if tuple(m.weight.shape[1:]) != (3, 3, 3) or m.bias is not None or m.weight.dtype != torch.float32 or m.out_channels % 4 or m.out_channels > 64:
        raise FdError(f"EfficientNet stem {tuple(m.weight.shape)}: the HIP weight-gradient kernel covers [Cout, 3, 3, 3] fp32 without bias, Cout % 4 == 0, Cout <= 64")
    if batch_stats:
        if not _bn_train_wide_ok(bn, x):
            raise FdError("EfficientNet stem: batch_stats=True needs _bn0 in training mode with affine parameters and running statistics")
        t = _bn_wide_rows(bn, _Stem3Rows.apply(x, m.weight, None, None, (net.stem_pad[0], h, w)), ACT_NONE)
    else:
        if not bn_is_frozen(bn):
            raise FdError("EfficientNet stem: train_stem=True without batch_stats folds a FROZEN _bn0")
        sc, sf = _bn_fold(bn)
        t = _Stem3Rows.apply(x, m.weight, sc, sf, (net.stem_pad[0], h, w))
    return act_rows(t, ACT_SILU)


class NormHandle:
    """What conv_norm_begin returns: either the finished tensor (`y`) or a SyncBatchNorm whose all-reduce is in flight (`sync`)."""
    __slots__ = ("y", "sync")

    def __init__(self, y=None, sync=None):
        self.y, self.sync = y, sync


def conv_norm_begin(m: nn.Conv2d, bn: Optional[nn.Module], x: torch.Tensor, segs: Segs, act: int = ACT_NONE,
                    f16_maps: bool = False) -> Optional["NormHandle"]:
    """conv_norm_act_rows in two halves: everything up to and including the ISSUE of a SyncBatchNorm's statistics all-reduce.  The caller enqueues work
    that does not need the normalised tensor, then calls conv_norm_finish.  (Any other layer kind is simply computed here.)  f16_maps: as there."""
    if bn is not None and not bn_is_frozen(bn) and _is_sync(bn):
        dense, dw, family = _dense_ok(m, x), _dw_ok(m, x), _bn_family(bn, x)
        if _STOCK or not (dense or dw) or family is None or (dw and m.bias is not None):
            return None
        f16 = dense and _bn_f16_ok(bn, f16_maps)
        pre = conv_rows(m, x, segs, None, ACT_NONE, out_f16=f16) if dense else dw_rows(m, x, segs, None, ACT_NONE)
        # the conv node just created is the only consumer of the BatchNorm's input gradient: its backward resolves the deferred second phase
        return NormHandle(sync=syncbn_begin(bn, pre, act, defer_backward=True, wide=f16 or family == BN_WIDE, f16=f16))
    y = conv_norm_act_rows(m, bn, x, segs, act, f16_maps)
    return None if y is None else NormHandle(y=y)


def conv_norm_finish(h: Optional["NormHandle"]) -> Optional[torch.Tensor]:
    if h is None:
        return None
    return h.y if h.sync is None else syncbn_finish(h.sync)


def conv_norm_act_rows(m: nn.Conv2d, bn: Optional[nn.Module], x: torch.Tensor, segs: Segs, act: int = ACT_NONE,
                       f16_maps: bool = False) -> Optional[torch.Tensor]:
    """act(bn(m(x))) on single-level rows with every piece on the HIP kernels, whatever mode `bn` is in: a frozen BatchNorm folds
    into the conv epilogue (ReLU fused, SiLU one extra launch that keeps the pre-activation), a BatchNorm in training mode runs
    on batch statistics (batchnorm_train_rows).  Returns None when a piece is not covered (the caller falls back).
    f16_maps (the bottleneck path's opt-in; dense convs, act NONE / ReLU): under torch.autocast(float16) the output map is f16 -- a frozen BatchNorm's conv
    stores f16, a BatchNorm in training mode with a float momentum runs on the any-width f16-map kernels at EVERY width, behind a raw conv that stores f16."""
    dense, dw = _dense_ok(m, x), _dw_ok(m, x)
    if _STOCK or not (dense or dw):
        return None
    conv = conv_rows if dense else (lambda mm, xx, sg, b=None, a=ACT_NONE: dw_rows(mm, xx, sg, b, a))
    f16_maps = _f16_maps_on(f16_maps) and dense and act in (ACT_NONE, ACT_RELU)
    if bn is None or bn_is_frozen(bn):
        if f16_maps:
            return conv_rows(m, x, segs, bn, act, out_f16=True)
        if act in (ACT_NONE, ACT_RELU):
            return conv(m, x, segs, bn, act)
        return act_rows(conv(m, x, segs, bn, ACT_NONE), act)
    if dw and m.bias is not None:
        return None
    family = _bn_family(bn, x)
    if family is None:
        return None
    if _bn_f16_ok(bn, f16_maps):
        return _bn_wide_rows(bn, conv_rows(m, x, segs, None, ACT_NONE, out_f16=True), act, f16=True)
    return (batchnorm_train_rows if family == BN_NARROW else _bn_wide_rows)(bn, conv(m, x, segs, None, ACT_NONE), act)


# ------------------------------------------------------------------------------------ NCHW-shaped conveniences
def _need_cuda(x: torch.Tensor) -> None:
    if not x.is_cuda:
        raise FdError("pytorch_object_detection_amd runs on the GPU only; there is no CPU fallback (got a CPU tensor)")


def covered(m: nn.Conv2d, bn: Optional[nn.Module], x: torch.Tensor, pad_out: bool = False) -> bool:
    return not _STOCK and (bn is None or bn_is_frozen(bn)) and (_dense_ok(m, x, pad_out) or _dw_ok(m, x))


def conv_bn_act(m: nn.Conv2d, bn: Optional[nn.Module], x: torch.Tensor, act: int = ACT_NONE,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(bn(m(x)) + residual) on NCHW-shaped tensors, act in {ACT_NONE, ACT_RELU}; one HIP launch when covered."""
    _need_cuda(x)
    if covered(m, bn, x) and not (m.groups != 1 and residual is not None):
        B, _, H, W = x.shape
        segs = Segs.make(B, [(H, W)])
        if m.groups == 1:
            y = conv_rows(m, to_rows(x), segs, bn, act, to_rows(residual) if residual is not None else None)
            k, s, p, d = m.kernel_size[0], m.stride[0], _pad_of(m), m.dilation[0]
            return from_rows(y, B, (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1)
        return from_rows(dw_rows(m, to_rows(x), segs, bn, act), B, H, W)
    if not _STOCK and bn is not None and not bn_is_frozen(bn) and covered(m, None, x):
        stock_fallback(f"{type(bn).__name__}({getattr(bn, 'num_features', '?')}) in training mode behind a conv")
        y = bn(conv_bn_act(m, None, x))                     # BN in training mode: conv on HIP, statistics stock
    else:                                                   # documented stock-op fallbacks of the TRAINING forward (module docstring)
        stock_fallback(f"conv {tuple(m.weight.shape)} stride {m.stride[0]} groups {m.groups}" + (f" + {type(bn).__name__}" if bn is not None else ""))
        y = nn.Conv2d.forward(m, x) if bn is None else bn(nn.Conv2d.forward(m, x))
    if residual is not None:
        y = y + residual
    return F.relu(y) if act == ACT_RELU else y


def conv2d(m: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """m(x) with the HIP kernels where they apply."""
    return conv_bn_act(m, None, x)


def stem_frozen(trunk: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """maxpool(relu(bn1(conv1(x)))) of a frozen ResNet stem on the inference kernels (no autograd graph)."""
    B, _, H, W = x.shape
    dev = x.device
    with torch.no_grad():
        x4 = torch.empty(B * H * W, 4, dtype=torch.float32, device=dev)
        ops.nchw3_to_nhwc4(x.float().contiguous(), x4)
        sc, sf = _bn_fold(trunk.bn1)
        s_in = Segs.make(B, [(H, W)])
        s1 = ops.conv_out_segs(s_in, 7, 2, 3, 1)
        H1, W1 = s1.H[0], s1.W[0]
        y1 = torch.empty(s1.rows, 64, dtype=torch.float32, device=dev)
        ops.stem7x7(Rows(x4), ops.pack_stem7_weight(trunk.conv1.weight), Rows(y1), B, H, W, sc, sf, ACT_RELU)
        H2, W2 = (H1 + 2 - 3) // 2 + 1, (W1 + 2 - 3) // 2 + 1
        y2 = torch.empty(B * H2 * W2, 64, dtype=torch.float32, device=dev)
        ops.maxpool(Rows(y1), Rows(y2), B, H1, W1, 3, 2, 1)
    return from_rows(y2, B, H2, W2)


def stem_is_frozen(trunk: nn.Module, x: torch.Tensor) -> bool:
    return (not _STOCK and bn_is_frozen(trunk.bn1) and not trunk.conv1.weight.requires_grad and not x.requires_grad
            and _f32(x) and tuple(trunk.conv1.weight.shape) == (64, 3, 7, 7))


# ------------------------------------------------------------------------------- the trainable 7x7 stem (Cin = 3)
class _StemRows(torch.autograd.Function):
    """conv1 (7x7 stride 2 pad 3, 3 -> 64, no bias) of the ResNet stem on an NCHW fp32 image batch that needs no gradient, as rows [B * H/2 * W/2, 64]:
    y = act(conv(x, w) * scale + shift) with scale / shift the constants of a frozen bn1 (act = ReLU), or the raw conv (scale = shift = None, ACT_NONE) in
    front of a BatchNorm on batch statistics.  Forward: fd_nchw3_to_nhwc4 + the unfused fd_stem7x7_nhwc4 (the map is needed for the ReLU mask and by the
    max-pool's backward).  Backward: fd_stem7x7_bwd_weight_nhwc4, the ReLU mask applied in its dy loader; there is no data gradient.
    Under torch.autocast the node computes in fp32 (_fwd32), like the depthwise and normalisation nodes: the reference's fp16 stem convolution is computed
    wider here."""

    @staticmethod
    @_fwd32
    def forward(ctx, x, weight, scale, shift, act):
        B, _, H, W = x.shape
        x4 = torch.empty(B * H * W, 4, dtype=torch.float32, device=x.device)
        ops.nchw3_to_nhwc4(x.contiguous(), x4)
        y = torch.empty(B * (H // 2) * (W // 2), 64, dtype=torch.float32, device=x.device)
        ops.stem7x7(Rows(x4), ops.pack_stem7_weight(weight.detach()), Rows(y), B, H, W, scale, shift, act)
        ctx.save_for_backward(x4, scale, y if act == ACT_RELU else None)
        ctx.geom = (B, H, W)
        return y

    @staticmethod
    @_bwd
    def backward(ctx, gy):
        x4, scale, y = ctx.saved_tensors
        B, H, W = ctx.geom
        gw = None
        if ctx.needs_input_grad[1]:
            g = resolve_pending(gy)
            gr = _rv(g)
            if gr is None:
                g = g.contiguous()
                gr = _r(g)
            gw = ops.stem7x7_wgrad(Rows(x4), gr, B, H, W, _r(y) if y is not None else None, scale)
        return None, gw, None, None, None


def stem_rows_ok(trunk: nn.Module, x: torch.Tensor) -> bool:
    """What stem_rows covers: the [64, 3, 7, 7] fp32 filter bank without bias, an fp32 image batch of even size that needs no gradient, and bn1 either
    frozen or a BatchNorm in training mode that batchnorm_train_rows takes (a SyncBatchNorm spanning ranks only with the trunk's hip_bn_train switch on:
    without it that keeps the stock path)."""
    m, bn = trunk.conv1, trunk.bn1
    return (not _STOCK and tuple(m.weight.shape) == (64, 3, 7, 7) and m.bias is None and m.weight.dtype == torch.float32 and x.dtype == torch.float32
            and not x.requires_grad and x.dim() == 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and x.shape[2] >= 2 and x.shape[3] >= 2
            and (bn_is_frozen(bn) or (_bn_family(bn, x) == BN_NARROW and (not _is_sync(bn) or getattr(trunk, "hip_bn_train", False)))))


def stem_rows(trunk: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """maxpool(relu(bn1(conv1(x)))) of a TRAINABLE ResNet stem with every op a HIP node (check with stem_rows_ok): _StemRows (frozen bn1 folded into the
    launch, or the raw conv + batchnorm_train_rows on batch statistics) and the max-pool node at (3, 2, 1).  NCHW-shaped channels-last view out."""
    B, _, H, W = x.shape
    bn = trunk.bn1
    if bn_is_frozen(bn):
        sc, sf = _bn_fold(bn)
        t = _StemRows.apply(x, trunk.conv1.weight, sc, sf, ACT_RELU)
    else:
        t = batchnorm_train_rows(bn, _StemRows.apply(x, trunk.conv1.weight, None, None, ACT_NONE), ACT_RELU)
    H1, W1 = H // 2, W // 2
    y2 = _PoolAddRows.apply(t, None, (B, H1, W1, 3, 2, 1))
    return from_rows(y2, B, (H1 + 2 - 3) // 2 + 1, (W1 + 2 - 3) // 2 + 1)
