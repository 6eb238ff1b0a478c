"""GPU checks of the two JPEG launches (csrc/fd_jpeg.hip), every comparison exact against the numpy restatement tests/jpeg_ref.py -- which
tests/test_jpeg_cpu.py pins against Pillow on real streams.  The crafted coefficient blocks below (single coefficients at the ends of the 12-bit range, large
quantisers) are pinned by the restatement ONLY: Pillow never sees such streams."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import jpeg_ref as R  # noqa: E402
import lcg  # noqa: E402
from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd._lib import FdError  # noqa: E402
from pytorch_object_detection_amd.data.jpeg import JpegDecoder  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G16 = os.path.join(HERE, "golden", "g16_jpeg.npz")
GUARD, FILL = 64, 0xA7
SIZES = [(1, 1), (1, 5), (2, 4), (5, 6), (7, 3), (8, 8), (9, 17), (15, 16), (16, 15), (17, 33), (31, 2), (3, 31), (33, 47), (40, 48)]


@pytest.fixture(scope="module")
def g16():
    g = np.load(G16)
    return {k: g[k] for k in g.files}


def _upload_jobs(jobs):
    raw = np.frombuffer(bytes(jobs), np.uint8).copy()
    return torch.from_numpy(raw).to(DEV)


def run_idct(items):
    """items: [(int16 [bh][bw][64], 64 table entries)] -> their uint8 planes from ONE launch.  Every plane sits between guard bytes, checked afterwards."""
    n = len(items)
    jobs = (_lib.JpegIdctJob * n)()
    coef_off, plane_off = 0, GUARD
    for j, (c, q) in enumerate(items):
        bh, bw = c.shape[:2]
        jobs[j].coef_off, jobs[j].plane_off, jobs[j].bw, jobs[j].bh, jobs[j].qt = coef_off, plane_off, bw, bh, j
        coef_off += c.size
        plane_off += bh * bw * 64 + GUARD
    coefs = torch.from_numpy(np.concatenate([c.reshape(-1) for c, _ in items]).astype(np.int16)).to(DEV)
    qtabs = torch.from_numpy(np.stack([np.asarray(q, np.int64).astype(np.uint16).view(np.int16) for _, q in items])).to(DEV)
    planes = torch.full((plane_off,), FILL, dtype=torch.uint8, device=DEV)
    ops.jpeg_idct_u8(jobs, _upload_jobs(jobs), coefs, qtabs, planes)
    host = planes.cpu().numpy()
    out, at = [], 0
    for j, (c, _) in enumerate(items):
        bh, bw = c.shape[:2]
        assert (host[at:at + GUARD] == FILL).all(), f"bytes in front of plane {j} were written"
        out.append(host[at + GUARD:at + GUARD + bh * bw * 64].reshape(8 * bh, 8 * bw))
        at += GUARD + bh * bw * 64
    assert (host[at:] == FILL).all(), "bytes behind the last plane were written"
    return out


def run_color(items):
    """items: [(planes list, w, h, hs, vs)] -> uint8 [h][w][3] each from ONE launch; planes and images between guard bytes."""
    n = len(items)
    jobs = (_lib.JpegColorJob * n)()
    blob, out_off, out_total = [], [], 0
    for j, (pl, w, h, hs, vs) in enumerate(items):
        jobs[j].width, jobs[j].height, jobs[j].ncomp, jobs[j].h_samp, jobs[j].v_samp = w, h, len(pl), hs, vs
        for c, p in enumerate(pl):
            jobs[j].plane_off[c], jobs[j].stride[c], jobs[j].rows[c] = sum(b.size for b in blob), p.shape[1], p.shape[0]
            blob.append(np.ascontiguousarray(p, np.uint8).reshape(-1))
        out_total += GUARD
        out_off.append(out_total)
        out_total += -(-h * w * 3 // 4) * 4            # the next image 4-byte aligned again
    out_total += GUARD
    planes = torch.from_numpy(np.concatenate(blob)).to(DEV)
    outs = torch.full((out_total,), FILL, dtype=torch.uint8, device=DEV)
    for j in range(n):
        jobs[j].out = outs.data_ptr() + out_off[j]
    ops.jpeg_color_u8(jobs, _upload_jobs(jobs), planes)
    host = outs.cpu().numpy()
    written = np.zeros(out_total, bool)
    res = []
    for j, (pl, w, h, hs, vs) in enumerate(items):
        res.append(host[out_off[j]:out_off[j] + h * w * 3].reshape(h, w, 3))
        written[out_off[j]:out_off[j] + h * w * 3] = True
    assert (host[~written] == FILL).all(), "bytes outside the images were written"
    return res


def _lcg_i16(n, seed, lo, hi):
    return ((lcg.u01(n, seed) * np.float32(hi - lo)).astype(np.int64) + lo).astype(np.int16)


def test_idct_equals_restatement_on_the_fixture_coefficients(g16):
    items = []
    for i in range(len(g16["params"])):
        blob = g16[f"jpg_{i}"].tobytes()
        hdr = R.parse(blob)
        items += [(c, hdr["qt"][k]) for k, c in enumerate(R.entropy_decode(blob, hdr))]
    got = run_idct(items)
    for j, ((c, q), p) in enumerate(zip(items, got)):
        np.testing.assert_array_equal(p, R.idct_plane(c, q), err_msg=f"job {j}")


def test_idct_equals_restatement_on_crafted_blocks():
    """Pinned by the restatement only (no encoder writes these): both ends of the range-limit wrap and the 64-bit intermediates are reached."""
    items = []
    dc = np.zeros((3, 5, 64), np.int16)                                  # a 3 x 5 grid of DC-only blocks, the whole DC range of a baseline stream and beyond
    dc[:, :, 0] = np.array([-32768, -2048, -1024, -513, -512, -129, -128, -1, 0, 1, 127, 128, 511, 1016, 32767], np.int16).reshape(3, 5)
    items += [(dc, np.ones(64)), (dc, np.full(64, 8)), (dc, np.full(64, 255))]
    for v in (2047, -2048):
        one = np.zeros((8, 8, 64), np.int16)                            # block k: the value at coefficient k alone
        one.reshape(64, 64)[np.arange(64), np.arange(64)] = v
        items += [(one, np.ones(64)), (one, np.full(64, 255))]
    wrapped = 0
    for q in (np.ones(64), np.full(64, 255)):                           # |coef * q| up to 32768 * 255 in every position at once: 64-bit sums
        items.append((_lcg_i16(2 * 3 * 64, 11, -32768, 32767).reshape(2, 3, 64), q))
    items.append((_lcg_i16(64, 12, -1024, 1023).reshape(1, 1, 64), 1 + (lcg.u01(64, 13) * np.float32(255)).astype(np.int64)))       # a 1 x 1 grid
    items.append((_lcg_i16(15 * 64, 14, -300, 300).reshape(3, 5, 64), 1 + (lcg.u01(64, 15) * np.float32(40)).astype(np.int64)))     # 3 x 5, a realistic range
    items.append((np.full((1, 1, 64), -32768, np.int16), np.full(64, 255)))
    got = run_idct(items)
    for j, ((c, q), p) in enumerate(zip(items, got)):
        want = R.idct_plane(c, q)
        np.testing.assert_array_equal(p, want, err_msg=f"crafted item {j}")
        x = c.astype(np.int64) * np.asarray(q, np.int64)
        wrapped += int(np.abs(x).max() * 25172 * 4 > 2 ** 31)
    assert wrapped >= 6                                                  # items whose products leave 32 bits were among them
    # the wrap of libjpeg's range-limit table, both ends: DC 16 * 255 -> v = 510 (+128 clamps to 255), DC -32768 * 255 far outside [-512, 511]
    assert R.range_limit(np.array([-513, -512, -129, -128, 0, 127, 128, 383, 384, 511, 512])).tolist() == [255, 0, 0, 0, 128, 255, 255, 255, 255, 255, 0]


def test_color_equals_restatement_at_every_fixture_size_and_sampling():
    items, k = [], 0
    for hs, vs, nc in ((1, 1, 3), (2, 1, 3), (2, 2, 3), (1, 1, 1)):
        for h, w in SIZES:
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            shapes = [(8 * my * vs, 8 * mx * hs)] + [(8 * my, 8 * mx)] * (nc - 1)
            pl = []
            for c, (r, s) in enumerate(shapes):
                u = lcg.u01(r * s, 700 + 3 * k + c).reshape(r, s)
                p = (u * np.float32(256)).astype(np.uint8)
                if k % 3 == 2:                                           # extremes: the colour clamp and the rounding of the triangle filter
                    p = np.where(u < np.float32(0.4), 0, np.where(u < np.float32(0.8), 255, p)).astype(np.uint8)
                pl.append(p)
            items.append((pl, w, h, hs, vs))
            k += 1
    got = run_color(items)
    for (pl, w, h, hs, vs), px in zip(items, got):
        np.testing.assert_array_equal(px, R.color(pl, w, h, hs, vs), err_msg=f"{len(pl)} planes {h}x{w} sampling {hs}x{vs}")
    # planes wider than the MCU-padded component (another stride), images that end 1 .. 3 pixels into a lane's four
    pl = [(lcg.u01(24 * 40, 31).reshape(24, 40) * np.float32(256)).astype(np.uint8), (lcg.u01(16 * 24, 32).reshape(16, 24) * np.float32(256)).astype(np.uint8),
          (lcg.u01(16 * 24, 33).reshape(16, 24) * np.float32(256)).astype(np.uint8)]
    odd = [(pl, w, h, 2, 2) for h, w in ((17, 33), (23, 39), (3, 7), (1, 2), (1, 3))]
    for (p, w, h, hs, vs), px in zip(odd, run_color(odd)):
        np.testing.assert_array_equal(px, R.color(p, w, h, hs, vs), err_msg=f"{h}x{w}")


def test_a_mixed_batch_in_one_call_equals_one_image_per_call(g16):
    p = g16["params"]
    pick = [i for i in range(len(p)) if (p[i, 1], p[i, 2]) in ((33, 47), (40, 48), (9, 17), (1, 5))][:16]
    assert len(pick) == 16 and len({int(p[i, 0]) for i in pick}) == 4
    blobs = [g16[f"jpg_{i}"].tobytes() for i in pick]
    dec = JpegDecoder(DEV, fallback="raise")
    batch = [t.cpu().numpy() for t in dec.decode(blobs)]
    for i, b, got in zip(pick, blobs, batch):
        single, = dec.decode([b])
        np.testing.assert_array_equal(got, single.cpu().numpy(), err_msg=f"case {i}")
        np.testing.assert_array_equal(got, g16[f"rgb_{i}"], err_msg=f"case {i}")


def test_invalid_jobs_are_rejected_before_any_launch():
    c = np.zeros((2, 3, 64), np.int16)
    c[:, :, 0] = 40
    coefs = torch.from_numpy(c.reshape(-1)).to(DEV)
    qtabs = torch.ones(1, 64, dtype=torch.int16, device=DEV)
    planes = torch.full((6 * 64,), FILL, dtype=torch.uint8, device=DEV)

    def job(**over):
        jobs = (_lib.JpegIdctJob * 1)()
        jobs[0].bw, jobs[0].bh = 3, 2
        for k, v in over.items():
            setattr(jobs[0], k, v)
        return jobs

    for over in (dict(bw=4), dict(bh=0), dict(coef_off=64), dict(plane_off=8), dict(plane_off=-64), dict(qt=1)):
        jobs = job(**over)
        with pytest.raises(FdError) as ei:
            ops.jpeg_idct_u8(jobs, _upload_jobs(jobs), coefs, qtabs, planes)
        assert ei.value.rc == _lib.E_INVAL, over
    with pytest.raises(FdError, match="int16"):
        ops.jpeg_idct_u8(job(), _upload_jobs(job()), coefs.float(), qtabs, planes)
    with pytest.raises(FdError, match="ctypes array"):
        ops.jpeg_idct_u8([], _upload_jobs(job()), coefs, qtabs, planes)
    out = torch.full((16 * 24 * 3,), FILL, dtype=torch.uint8, device=DEV)

    def cjob(**over):
        jobs = (_lib.JpegColorJob * 1)()
        jobs[0].out, jobs[0].width, jobs[0].height, jobs[0].ncomp, jobs[0].h_samp, jobs[0].v_samp = out.data_ptr(), 24, 16, 1, 1, 1
        jobs[0].stride[0], jobs[0].rows[0] = 24, 16
        for k, v in over.items():
            setattr(jobs[0], k, v)
        return jobs

    for over in (dict(width=25), dict(height=17), dict(ncomp=3), dict(h_samp=2), dict(out=out.data_ptr() + 1), dict(out=None)):
        jobs = cjob(**over)
        with pytest.raises(FdError) as ei:
            ops.jpeg_color_u8(jobs, _upload_jobs(jobs), planes)
        assert ei.value.rc == _lib.E_INVAL, over
    torch.cuda.synchronize()
    assert bool((planes == FILL).all()) and bool((out == FILL).all())            # nothing ran
    # ... and the valid forms of the same jobs do run
    ops.jpeg_idct_u8(job(), _upload_jobs(job()), coefs, qtabs, planes)
    ops.jpeg_color_u8(cjob(), _upload_jobs(cjob()), planes)
    want = R.idct_plane(c, np.ones(64))
    np.testing.assert_array_equal(planes.cpu().numpy().reshape(16, 24), want)
    np.testing.assert_array_equal(out.cpu().numpy().reshape(16, 24, 3), R.color([want], 24, 16, 1, 1))
