"""Baseline JPEG files -> decoded uint8 [h, w, 3] CUDA images, the input of forward_raw / detect_raw / collate_train_raw.

The reference decodes on the host with Pillow (dataset/voc.py:69, dataset/pascalvoc.py:28, data/dataload.py:35:
Image.open(path).convert('RGB')).  Here the host keeps the serial part -- file reading, marker parsing, Huffman decoding, the last
one on a small thread pool -- and the device does dequantisation, the inverse DCT, chroma upsampling and YCbCr -> RGB for the whole
batch in two launches (ops.jpeg_idct_u8, ops.jpeg_color_u8).  The pixels are Pillow's, bit for bit.
"""
from __future__ import annotations

import ctypes as C
import io
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _lib, ops
from .._lib import FdError

MAX_THREADS = 16            # the entropy decoders of one batch; never sized by os.cpu_count()


def _pil():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def _load(blob) -> np.ndarray:
    if isinstance(blob, (str, os.PathLike)):
        with open(blob, "rb") as f:
            blob = f.read()
    return ops._jpeg_stream(blob)


class _Staging:
    """One of the decoder's two staging sets: pinned coefficients, pinned tables + jobs, and the event after the copies that read them."""

    def __init__(self):
        self.coef = self.coef_np = self.tab = self.tab_np = self.event = None

    def reserve(self, coef_elems: int, tab_bytes: int) -> None:
        if self.event is not None:
            self.event.synchronize()        # the copies of two batches ago: long done in a running pipeline
        if self.coef is None or self.coef.numel() < coef_elems:
            self.coef = torch.empty(max(coef_elems, 2 * (self.coef.numel() if self.coef is not None else 0)), dtype=torch.int16).pin_memory()
            self.coef_np = self.coef.numpy()
        if self.tab is None or self.tab.numel() < tab_bytes:
            self.tab = torch.empty(max(tab_bytes, 2 * (self.tab.numel() if self.tab is not None else 0)), dtype=torch.uint8).pin_memory()
            self.tab_np = self.tab.numpy()


class JpegDecoder:
    """decode(blobs) -> list of CUDA uint8 [h, w, 3] tensors, one per blob (bytes, a uint8 array, or a path), in order.

    Supported by the HIP path: baseline (SOF0 / 8-bit SOF1) Huffman streams with one scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
    custom Huffman tables and restart intervals included.  Any other well-formed stream (progressive, CMYK, RGB, ...) goes to Pillow
    on the host and is uploaded (fallback="pil", the default, when PIL imports) or raises FdError naming the blob and the reason
    (fallback="raise").  A corrupt stream always raises, before anything is enqueued for the call.

    Per call: every stream parsed, the supported ones Huffman-decoded on min(len(blobs), threads or 16, 16) threads straight into one
    reused pinned int16 buffer, ONE non-blocking copy of the coefficients, ONE of the tables and job records, two launches.  Nothing
    synchronises; two staging sets alternate, so the host half of the next batch may run under the device half of this one."""

    def __init__(self, device="cuda", threads: Optional[int] = None, fallback: str = "pil"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FdError("JpegDecoder runs on the GPU only (the decoded images live there); there is no CPU fallback -- use Pillow for CPU decoding")
        if fallback not in ("pil", "raise"):
            raise FdError(f"JpegDecoder: fallback must be 'pil' or 'raise', not {fallback!r}")
        if threads is not None and (not isinstance(threads, int) or isinstance(threads, bool) or threads < 1):
            raise FdError(f"JpegDecoder: threads must be a positive integer or None, not {threads!r}")
        self.fallback = fallback
        self.threads = min(threads or MAX_THREADS, MAX_THREADS)
        self._pool: Optional[ThreadPoolExecutor] = None
        self._sets = [_Staging(), _Staging()]
        self._turn = 0
        self.keep_last = False      # tools/time_jpeg.py: keep the arguments of the last two launches in self.last
        self.last = None

    # ---------------------------------------------------------------- host half
    def classify(self, blobs: Sequence):
        """Parse every blob and choose its route: -> (streams, infos, routes), routes[i] in ("hip", "pil").  Raises FdError for a corrupt header, and for an
        unsupported stream when there is no fallback to take it.  Host only."""
        blobs = None if isinstance(blobs, (bytes, bytearray, memoryview, str, os.PathLike, np.ndarray)) else list(blobs)
        if not blobs:
            raise FdError("JpegDecoder.decode expects a non-empty list of JPEG streams (bytes, uint8 arrays or paths)")
        streams, infos, routes = [], [], []
        for i, blob in enumerate(blobs):
            s = _load(blob)
            try:
                info = ops.jpeg_parse(s)
            except FdError as e:
                raise FdError(f"JpegDecoder: stream {i} is corrupt: {e}", rc=e.rc) from None
            if info.supported:
                routes.append("hip")
            else:
                reason = _lib.JPEG_REASONS.get(info.reason, f"reason {info.reason}")
                if self.fallback == "raise":
                    raise FdError(f"JpegDecoder: stream {i} is not supported by the HIP path: {reason}", rc=_lib.E_UNSUPPORTED)
                if _pil() is None:
                    raise FdError(f"JpegDecoder: stream {i} is not supported by the HIP path ({reason}) and PIL is not installed to fall back on",
                                  rc=_lib.E_UNSUPPORTED)
                routes.append("pil")
            streams.append(s)
            infos.append(info)
        return streams, infos, routes

    def _entropy(self, streams, infos, idx, offs, st: _Staging) -> None:
        fn = _lib.lib().fd_jpeg_entropy_decode
        base = st.coef_np.ctypes.data

        def one(k: int) -> int:
            i = idx[k]
            return fn(streams[i].ctypes.data, streams[i].size, C.byref(infos[i]), base + 2 * offs[k], int(infos[i].coef_bytes))

        if len(idx) == 1 or self.threads == 1:
            rcs = [one(k) for k in range(len(idx))]
        else:
            if self._pool is None:
                self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="fd_jpeg")     # spawns a thread only when a task has none idle
            rcs = list(self._pool.map(one, range(len(idx))))
        for k, rc in enumerate(rcs):
            if rc != 0:
                raise FdError(f"JpegDecoder: stream {idx[k]} is corrupt: {ops.jpeg_error(rc, 'fd_jpeg_entropy_decode')}", rc=int(rc))

    # ---------------------------------------------------------------- the call
    def decode(self, blobs: Sequence) -> List[torch.Tensor]:
        streams, infos, routes = self.classify(blobs)
        idx = [i for i, r in enumerate(routes) if r == "hip"]
        out: List[Optional[torch.Tensor]] = [None] * len(streams)
        if idx:
            n_jobs = sum(infos[i].ncomp for i in idx)
            offs, total = [], 0
            for i in idx:
                offs.append(total)
                total += int(infos[i].coef_bytes) // 2
            q_bytes, ij_bytes, cj_bytes = 128 * n_jobs, C.sizeof(_lib.JpegIdctJob) * n_jobs, C.sizeof(_lib.JpegColorJob) * len(idx)
            st = self._sets[self._turn]
            self._turn ^= 1
            st.reserve(total, q_bytes + ij_bytes + cj_bytes)
            self._entropy(streams, infos, idx, offs, st)           # raises on a corrupt scan: nothing has been enqueued yet
        pil_pixels = {}
        for i, r in enumerate(routes):
            if r == "pil":
                try:
                    pil_pixels[i] = np.array(_pil().open(io.BytesIO(streams[i].tobytes())).convert("RGB"))
                except Exception as e:      # Pillow's own verdict on a stream it cannot read
                    raise FdError(f"JpegDecoder: stream {i} is not supported by the HIP path and Pillow fails on it: {e}") from None
        for i, px in pil_pixels.items():
            out[i] = torch.from_numpy(px).to(self.device)
        if not idx:
            return out
        dev = self.device
        with torch.cuda.device(dev):
            idct_jobs = (_lib.JpegIdctJob * n_jobs)()
            color_jobs = (_lib.JpegColorJob * len(idx))()
            qt = st.tab_np[:q_bytes].view(np.uint16).reshape(n_jobs, 64)
            j, plane = 0, 0
            for k, i in enumerate(idx):
                info = infos[i]
                out[i] = torch.empty(info.height, info.width, 3, dtype=torch.uint8, device=dev)
                cj = color_jobs[k]
                cj.out, cj.width, cj.height, cj.ncomp, cj.h_samp, cj.v_samp = out[i].data_ptr(), info.width, info.height, info.ncomp, info.h_samp[0], info.v_samp[0]
                coef = offs[k]
                for c in range(info.ncomp):
                    bw, bh = info.bw[c], info.bh[c]
                    ij = idct_jobs[j]
                    ij.coef_off, ij.plane_off, ij.bw, ij.bh, ij.qt = coef, plane, bw, bh, j
                    qt[j] = np.ctypeslib.as_array(info.qt[c])
                    cj.plane_off[c], cj.stride[c], cj.rows[c] = plane, 8 * bw, 8 * bh
                    coef += bw * bh * 64
                    plane += bw * bh * 64
                    j += 1
            C.memmove(st.tab_np.ctypes.data + q_bytes, C.addressof(idct_jobs), ij_bytes)
            C.memmove(st.tab_np.ctypes.data + q_bytes + ij_bytes, C.addressof(color_jobs), cj_bytes)
            coefs = st.coef[:total].to(dev, non_blocking=True)
            tab = st.tab[:q_bytes + ij_bytes + cj_bytes].to(dev, non_blocking=True)
            if st.event is None:
                st.event = torch.cuda.Event()
            st.event.record()
            planes = torch.empty(plane, dtype=torch.uint8, device=dev)
            ops.jpeg_idct_u8(idct_jobs, tab[q_bytes:q_bytes + ij_bytes], coefs, tab[:q_bytes].view(torch.int16).view(n_jobs, 64), planes)
            ops.jpeg_color_u8(color_jobs, tab[q_bytes + ij_bytes:], planes)
            if self.keep_last:
                self.last = dict(idct_jobs=idct_jobs, color_jobs=color_jobs, tab=tab, coefs=coefs, planes=planes, q_bytes=q_bytes, ij_bytes=ij_bytes,
                                 n_jobs=n_jobs, out=[out[i] for i in idx])
        return out


_DECODERS = {}


def decode_jpeg_batch(blobs: Sequence, device="cuda", threads: Optional[int] = None, fallback: str = "pil") -> List[torch.Tensor]:
    """JpegDecoder(device, threads, fallback).decode(blobs), with the decoder (its pinned staging and threads) kept for the next call."""
    key = (str(torch.device(device)), threads, fallback)
    dec = _DECODERS.get(key)
    if dec is None:
        dec = _DECODERS[key] = JpegDecoder(device, threads, fallback)
    return dec.decode(blobs)
