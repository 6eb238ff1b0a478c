"""tests/golden/make_g16_jpeg.py — the JPEG fixture g16_jpeg.npz: images from lcg.py, encoded AND decoded by Pillow (libjpeg-turbo).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_g16_jpeg.py

Needs PIL only.  Stores data only; the zip entries carry a fixed timestamp, so a second run with the same Pillow reproduces the file
byte for byte.

Supported cases, row i of `params` = (sampling, h, w, quality, restart_marker_blocks, optimize, saturated) with sampling 0 / 1 / 2 / 3 =
4:4:4 / 4:2:2 / 4:2:0 / grayscale: `jpg_i` the byte string, `rgb_i` = np.asarray(Image.open(...).convert('RGB')).
  * every sampling x every size of SIZES (an edge at every MCU boundary +- 1, chroma widths 1, 2 and 3, one-block images), with quality,
    restart interval and optimize cycling so that each sampling sees each quality of (30, 75, 95, 100-on-a-saturated-pattern), each
    restart setting of (0, 1, 3) and optimize=True;
  * every sampling x (17, 33) x every quality x every restart setting.
Unsupported cases, row k of `bad_reason` = the FD_JPEG_R_* code expected for `bad_k`: what Pillow itself writes (progressive, CMYK,
an RGB stream) with `bad_rgb_k` = Pillow's pixels, and supported streams with patched header bytes (arithmetic frame marker, 12-bit
precision, 4:4:0 sampling, a one-component first scan, height 0), which Pillow is not asked to decode.
"""
import io
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import lcg  # noqa: E402

SIZES = [(1, 1), (1, 5), (2, 4), (5, 6), (7, 3), (8, 8), (9, 17), (15, 16), (16, 15), (17, 33), (31, 2), (3, 31), (33, 47), (40, 48)]
QUALITIES = [30, 75, 95, 100]          # 100: on the saturated pattern
RESTARTS = [0, 1, 3]
R_PROGRESSIVE, R_ARITHMETIC, R_PRECISION, R_COMPONENTS, R_RGB, R_SAMPLING, R_MULTISCAN, R_DNL = range(1, 9)


def image(h, w, seed, saturated=False, channels=3):
    """uint8 [h, w, channels]: smooth ramps plus noise, or a random 0 / 255 pattern."""
    u = lcg.u01(h * w * channels, seed).reshape(h, w, channels)
    if saturated:
        return np.where(u < np.float32(0.5), 0, 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    k = (lcg.u01(3 * channels, seed + 7919) * np.float32(9)).astype(np.int64).reshape(3, channels)
    ramp = (y[:, :, None] * (k[0] + 1) * 3 + x[:, :, None] * (k[1] + 2) * 2 + k[2] * 23) % 256
    noise = (u * np.float32(49)).astype(np.int64) - 24
    return np.clip(ramp + noise, 0, 255).astype(np.uint8)


def encode(px, sampling, quality, restart, optimize, **extra):
    img = Image.fromarray(px[:, :, 0], "L") if sampling == 3 else Image.fromarray(px, "RGB")
    kw = dict(quality=quality, optimize=bool(optimize), **extra)
    if sampling != 3:
        kw["subsampling"] = sampling
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_rgb(blob):
    return np.array(Image.open(io.BytesIO(blob)).convert("RGB"))


def _find(blob, marker):
    """Offset of the first segment with this marker byte (walking the segments from SOI)."""
    p = 2
    while p + 4 <= len(blob):
        assert blob[p] == 0xFF
        if blob[p + 1] == marker:
            return p
        p += 2 + ((blob[p + 2] << 8) | blob[p + 3])
    raise ValueError("marker %02x not found" % marker)


def patched(blob, what):
    b = bytearray(blob)
    sof = _find(blob, 0xC0)
    if what == "arithmetic":
        b[sof + 1] = 0xC9
    elif what == "precision":
        b[sof + 4] = 12
    elif what == "dnl":
        b[sof + 5] = b[sof + 6] = 0
    elif what == "sampling":              # the luma of a 4:2:0 stream: 2x2 -> 1x2 (4:4:0)
        assert b[sof + 11] == 0x22
        b[sof + 11] = 0x12
    elif what == "multiscan":             # the first scan holds the luma alone
        sos = _find(blob, 0xDA)
        assert b[sos + 4] == 3
        b[sos:sos + 14] = bytes([0xFF, 0xDA, 0, 8, 1, b[sos + 5], b[sos + 6], 0, 63, 0])
    return bytes(b)


def main():
    arrays, params = {}, []

    def add(sampling, h, w, quality, restart, optimize, seed):
        sat = quality == 100
        blob = encode(image(h, w, seed, sat), sampling, quality, restart, optimize)
        i = len(params)
        arrays[f"jpg_{i}"] = np.frombuffer(blob, np.uint8)
        arrays[f"rgb_{i}"] = pil_rgb(blob)
        params.append((sampling, h, w, quality, restart, int(optimize), int(sat)))

    for sampling in range(4):
        for k, (h, w) in enumerate(SIZES):
            add(sampling, h, w, QUALITIES[k % 4], RESTARTS[k % 3], k % 5 == 4, 1000 * sampling + k)
        for q in QUALITIES:
            for r in RESTARTS:
                add(sampling, 17, 33, q, r, False, 1000 * sampling + 100 + q + r)
    arrays["params"] = np.array(params, np.int32)

    base420 = encode(image(17, 33, 5000), 2, 75, 0, False)
    bad = [(encode(image(17, 33, 5001), 2, 75, 0, False, progressive=True), R_PROGRESSIVE, True)]
    buf = io.BytesIO()
    Image.fromarray(image(9, 17, 5002, channels=4), "CMYK").save(buf, "JPEG", quality=75)
    bad.append((buf.getvalue(), R_COMPONENTS, True))
    try:
        bad.append((encode(image(9, 17, 5003), 0, 75, 0, False, keep_rgb=True), R_RGB, True))
    except TypeError:                      # a Pillow without keep_rgb: the reason stays uncovered by a Pillow-written stream
        pass
    bad += [(patched(base420, "arithmetic"), R_ARITHMETIC, False), (patched(base420, "precision"), R_PRECISION, False),
            (patched(base420, "sampling"), R_SAMPLING, False), (patched(base420, "multiscan"), R_MULTISCAN, False), (patched(base420, "dnl"), R_DNL, False)]
    for k, (blob, reason, decodable) in enumerate(bad):
        arrays[f"bad_{k}"] = np.frombuffer(blob, np.uint8)
        if decodable:
            arrays[f"bad_rgb_{k}"] = pil_rgb(blob)
    arrays["bad_reason"] = np.array([r for _, r, _ in bad], np.int32)

    path = os.path.join(HERE, "g16_jpeg.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"g16_jpeg.npz  {os.path.getsize(path) / 1024:.1f} KB  {len(params)} supported and {len(bad)} unsupported streams")


if __name__ == "__main__":
    main()
