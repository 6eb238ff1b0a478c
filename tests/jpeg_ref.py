"""Baseline JPEG decoding restated in numpy integers: marker parsing, Huffman decoding, dequantisation, libjpeg's jpeg_idct_islow, libjpeg-turbo's fancy
chroma upsampling and YCbCr -> RGB.  The reference of the fd_jpeg_* entry points; itself pinned against Pillow by tests/test_jpeg_cpu.py.
Slow (the Huffman decoder walks a Python string of bits): meant for the tiny images of tests/golden/g16_jpeg.npz."""
import numpy as np

R_NONE, R_PROGRESSIVE, R_ARITHMETIC, R_PRECISION, R_COMPONENTS, R_RGB, R_SAMPLING, R_MULTISCAN, R_DNL = range(9)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Corrupt(ValueError):
    pass


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """-> dict(width, height, ncomp, supported, reason, restart_interval, h_samp, v_samp, bw, bh, qt [ncomp][64] natural order, dc / ac code dicts per
    component, scan_offset).  An unsupported stream comes back with supported = False and a reason as soon as the reason is known."""
    d = bytes(data)
    if len(d) < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt("no SOI")
    hdr = dict(supported=False, reason=R_NONE, restart_interval=0, width=0, height=0, ncomp=0)
    qt, qt_wide, huff, comps, jfif, adobe = {}, {}, {}, None, False, None
    p = 2
    while True:
        if p >= len(d) or d[p] != 0xFF:
            raise Corrupt("marker expected")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt("truncated")
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0x00, 0xD8, 0xD9) or p + 2 > len(d):
            raise Corrupt("bad marker")
        ln = _u16(d, p)
        if ln < 2 or p + ln > len(d):
            raise Corrupt("bad segment length")
        s = d[p + 2:p + ln]
        p += ln
        if m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                n = 128 if pq else 64
                if tq > 3 or pq > 1 or i + 1 + n > len(s):
                    raise Corrupt("bad DQT")
                v = np.frombuffer(s[i + 1:i + 1 + n], dtype=">u2" if pq else np.uint8).astype(np.int64)
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = v
                qt[tq], qt_wide[tq] = t, bool(pq) or int(v.max()) > 255
                i += 1 + n
        elif m == 0xC4:
            i = 0
            while i < len(s):
                if i + 17 > len(s):
                    raise Corrupt("bad DHT")
                tc, th = s[i] >> 4, s[i] & 15
                bits = list(s[i + 1:i + 17])
                if tc > 1 or th > 3 or i + 17 + sum(bits) > len(s):
                    raise Corrupt("bad DHT")
                vals, codes, code, k = s[i + 17:i + 17 + sum(bits)], {}, 0, 0
                for ln_ in range(1, 17):
                    for _ in range(bits[ln_ - 1]):
                        codes[format(code, "0%db" % ln_)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[(tc, th)] = codes
                i += 17 + sum(bits)
        elif m == 0xDD:
            hdr["restart_interval"] = _u16(s, 0)
        elif m == 0xE0:
            jfif = jfif or s[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(s) >= 12 and s[:5] == b"Adobe":
                adobe = s[11]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if comps is not None or len(s) < 6:
                raise Corrupt("bad SOF")
            hdr.update(height=_u16(s, 1), width=_u16(s, 3), ncomp=s[5])
            for lo, why in ((0xC9, R_ARITHMETIC), (0xC2, R_PROGRESSIVE)):
                if m >= lo:
                    return dict(hdr, reason=why)
            if s[0] != 8:
                return dict(hdr, reason=R_PRECISION)
            if s[5] not in (1, 3):
                return dict(hdr, reason=R_COMPONENTS)
            if hdr["height"] == 0:
                return dict(hdr, reason=R_DNL)
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif m == 0xDA:
            if comps is None:
                raise Corrupt("SOS before SOF")
            ns = s[0]
            if ns != len(comps) or [s[1 + 2 * c] for c in range(ns)] != [c[0] for c in comps]:
                return dict(hdr, reason=R_MULTISCAN)
            if len(comps) == 3:
                rgb = False if jfif else (adobe == 0 if adobe is not None else [c[0] for c in comps] == [82, 71, 66])
                if rgb:
                    return dict(hdr, reason=R_RGB)
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    return dict(hdr, reason=R_SAMPLING)
            else:
                comps = [(comps[0][0], 1, 1, comps[0][3])]
            if any(qt_wide[c[3]] for c in comps):
                return dict(hdr, reason=R_PRECISION)
            hs, vs = comps[0][1], comps[0][2]
            mx, my = -(-hdr["width"] // (8 * hs)), -(-hdr["height"] // (8 * vs))
            hdr.update(supported=True, h_samp=[c[1] for c in comps], v_samp=[c[2] for c in comps], mcus_x=mx, mcus_y=my,
                       bw=[mx * c[1] for c in comps], bh=[my * c[2] for c in comps], qt=[qt[c[3]] for c in comps],
                       dc=[huff[(0, s[2 + 2 * c] >> 4)] for c in range(ns)], ac=[huff[(1, s[2 + 2 * c] & 15)] for c in range(ns)], scan_offset=p)
            return hdr


def _intervals(d, p):
    """The entropy-coded bytes after offset p, unstuffed, as one string of bits per restart interval."""
    out, cur = [], []
    while p < len(d):
        b = d[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
        elif p + 1 < len(d) and d[p + 1] == 0x00:
            cur.append(0xFF)
            p += 2
        elif p + 1 < len(d) and 0xD0 <= d[p + 1] <= 0xD7:
            out.append(cur)
            cur = []
            p += 2
        else:
            break
    out.append(cur)
    return ["".join(format(b, "08b") for b in iv) for iv in out]


def entropy_decode(data, hdr):
    """-> [int16 [bh][bw][64] per component], natural order."""
    d = bytes(data)
    ivs = _intervals(d, hdr["scan_offset"])
    nc = hdr["ncomp"]
    coefs = [np.zeros((hdr["bh"][c], hdr["bw"][c], 64), np.int16) for c in range(nc)]
    ri = hdr["restart_interval"]
    state = dict(bits=ivs[0], pos=0)

    def symbol(codes):
        b, p = state["bits"], state["pos"]
        for ln in range(1, 17):
            v = codes.get(b[p:p + ln])
            if v is not None and p + ln <= len(b):
                state["pos"] = p + ln
                return v
        raise Corrupt("no code")

    def receive(s):
        b, p = state["bits"], state["pos"]
        if p + s > len(b):
            raise Corrupt("truncated scan")
        v = int(b[p:p + s], 2)
        state["pos"] = p + s
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v

    pred, mcu = [0] * nc, 0
    for my in range(hdr["mcus_y"]):
        for mx in range(hdr["mcus_x"]):
            if ri and mcu and mcu % ri == 0:
                state = dict(bits=ivs[mcu // ri], pos=0)
                pred = [0] * nc
            for c in range(nc):
                for v in range(hdr["v_samp"][c]):
                    for h in range(hdr["h_samp"][c]):
                        blk = coefs[c][my * hdr["v_samp"][c] + v, mx * hdr["h_samp"][c] + h]
                        s = symbol(hdr["dc"][c])
                        if s:
                            pred[c] += receive(s)
                        blk[0] = np.int64(pred[c]).astype(np.int16)
                        k = 1
                        while k < 64:
                            rs = symbol(hdr["ac"][c])
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                if k > 63:
                                    raise Corrupt("coefficient index past 63")
                                blk[ZIGZAG[k]] = receive(s)
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                break
            mcu += 1
    return coefs


def flat_coefs(coefs):
    return np.concatenate([c.reshape(-1) for c in coefs])


# ------------------------------------------------------------------------------ jpeg_idct_islow
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(x, shift):
    """x: int64 [..., 8] along the last axis -> the eight outputs of one pass of jidctint.c's jpeg_idct_islow, descaled by `shift`."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = x[..., 0], x[..., 4]
    tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([_descale(o, shift) for o in out], axis=-1)


def range_limit(v):
    i = np.asarray(v, np.int64) & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def idct_plane(coefs, q):
    """coefs: int16 [bh][bw][64]; q: 64 table entries, natural order -> uint8 [8 * bh][8 * bw]."""
    bh, bw = coefs.shape[:2]
    # DEQUANTIZE is an int product in libjpeg; then everything is JLONG (64 bits)
    x = (coefs.astype(np.int32) * np.asarray(q, np.int64).astype(np.int32)).astype(np.int64).reshape(bh, bw, 8, 8)
    ws = _idct_1d(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)                    # columns
    ws = ws.astype(np.int32).astype(np.int64)                                 # the int workspace
    px = range_limit(_idct_1d(ws, 18))                                        # rows
    return px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


# ------------------------------------------------------------------------------ upsampling and colour
def _up_h2v1(p):
    """p: int [rows][dw], dw > 2 -> [rows][2 * dw]"""
    p = p.astype(np.int64)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], -1).reshape(p.shape[0], -1)


def _up_h2v2(p):
    """p: int [dh][dw], dw > 2 -> [2 * dh][2 * dw]"""
    p = p.astype(np.int64)
    above, below = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    rows = []
    for nb in (above, below):
        cs = 3 * p + nb
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        even, odd = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        rows.append(np.stack([even, odd], -1).reshape(p.shape[0], -1))
    return np.stack(rows, 1).reshape(2 * p.shape[0], -1)


def upsample(plane, w, h, hs, vs):
    """A chroma plane (any padding) of true size ceil(w / hs) x ceil(h / vs) -> int64 [h][w] at full resolution."""
    dw, dh = -(-w // hs), -(-h // vs)
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:h, :w]
    if dw <= 2:
        p = np.repeat(p, 2, axis=1)
        return (np.repeat(p, 2, axis=0) if vs == 2 else p)[:h, :w]
    return (_up_h2v2(p) if vs == 2 else _up_h2v1(p))[:h, :w]


def color(planes, w, h, hs, vs):
    """planes: [Y] or [Y, Cb, Cr] uint8 planes (MCU-padded or larger) -> uint8 [h][w][3]."""
    y = planes[0][:h, :w].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb, cr = upsample(planes[1], w, h, hs, vs) - 128, upsample(planes[2], w, h, hs, vs) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def planes_of(hdr, coefs):
    return [idct_plane(coefs[c], hdr["qt"][c]) for c in range(hdr["ncomp"])]


def decode(data):
    hdr = parse(data)
    if not hdr["supported"]:
        raise ValueError("unsupported stream, reason %d" % hdr["reason"])
    return color(planes_of(hdr, entropy_decode(data, hdr)), hdr["width"], hdr["height"], hdr["h_samp"][0], hdr["v_samp"][0])
