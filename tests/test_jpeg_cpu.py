"""The JPEG decoder without a GPU: the numpy restatement (tests/jpeg_ref.py) against the pixels Pillow returned (tests/golden/g16_jpeg.npz)
and against live Pillow, the host entry points fd_jpeg_parse / fd_jpeg_entropy_decode against the restatement, the reason codes, truncated streams and
threads, the struct layouts, the new symbols, and JpegDecoder's refusals and fallback choice."""
import ctypes
import io
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import jpeg_ref as R  # noqa: E402
from pytorch_object_detection_amd import _lib, ops  # noqa: E402
from pytorch_object_detection_amd._lib import FdError  # noqa: E402
from pytorch_object_detection_amd.data.jpeg import JpegDecoder, decode_jpeg_batch  # noqa: E402

G16 = os.path.join(HERE, "golden", "g16_jpeg.npz")
NEW = ("fd_jpeg_parse", "fd_jpeg_entropy_decode", "fd_jpeg_idct_u8", "fd_jpeg_color_u8")
SIZES = {(1, 1), (1, 5), (2, 4), (5, 6), (7, 3), (8, 8), (9, 17), (15, 16), (16, 15), (17, 33), (31, 2), (3, 31), (33, 47), (40, 48)}


@pytest.fixture(scope="module")
def g16():
    g = np.load(G16)
    return {k: g[k] for k in g.files}


def _cases(g):
    return [(i, tuple(int(v) for v in p), g[f"jpg_{i}"].tobytes(), g[f"rgb_{i}"]) for i, p in enumerate(g["params"])]


def test_fixture_holds_the_cases_the_decoder_is_pinned_on(g16):
    p = g16["params"]
    for s in range(4):
        rows = p[p[:, 0] == s]
        assert {(int(h), int(w)) for h, w in rows[:, 1:3]} == SIZES, s
        assert set(rows[:, 3]) == {30, 75, 95, 100} and set(rows[:, 4]) == {0, 1, 3} and 1 in rows[:, 5], s
        assert all(int(sat) == int(q == 100) for q, sat in rows[:, [3, 6]])
    assert os.path.getsize(G16) < 300 * 1024
    assert set(g16["bad_reason"]) >= {R.R_PROGRESSIVE, R.R_ARITHMETIC, R.R_PRECISION, R.R_COMPONENTS, R.R_SAMPLING, R.R_MULTISCAN, R.R_DNL}


def test_restatement_equals_the_fixture_pixels(g16):
    for i, p, blob, want in _cases(g16):
        np.testing.assert_array_equal(R.decode(blob), want, err_msg=f"case {i} {p}")


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    import make_g16_jpeg as M
    n = 0
    for sampling in range(4):
        for k, (h, w) in enumerate([(13, 21), (24, 7), (6, 50), (35, 35)]):
            for q, r, opt in ((60, 0, False), (88, 2, True)):
                sat = (k + sampling) % 4 == 3
                blob = M.encode(M.image(h, w, 9000 + 10 * sampling + k, sat), sampling, 100 if sat else q, r, opt)
                want = np.array(Image.open(io.BytesIO(blob)).convert("RGB"))
                np.testing.assert_array_equal(R.decode(blob), want, err_msg=f"sampling {sampling} {h}x{w} q{q} r{r} opt{opt}")
                n += 1
    assert n == 32


def test_host_entry_points_give_the_restatements_headers_and_coefficients(g16):
    for i, p, blob, _ in _cases(g16):
        hdr, info = R.parse(blob), ops.jpeg_parse(blob)
        nc = hdr["ncomp"]
        assert info.supported == 1 and info.reason == _lib.JPEG_R_NONE, i
        assert (info.width, info.height, info.ncomp, info.restart_interval) == (hdr["width"], hdr["height"], nc, hdr["restart_interval"]) == (p[2], p[1], 1 if p[0] == 3 else 3,
                                                                                                                                       info.restart_interval), i
        assert (p[4] == 0) == (info.restart_interval == 0)
        for name in ("h_samp", "v_samp", "bw", "bh"):
            assert list(getattr(info, name))[:nc] == hdr[name], (i, name)
        assert (info.h_max, info.v_max, info.mcus_x, info.mcus_y) == (hdr["h_samp"][0], hdr["v_samp"][0], hdr["mcus_x"], hdr["mcus_y"])
        assert info.scan_offset == hdr["scan_offset"] and info.coef_bytes == 128 * sum(a * b for a, b in zip(hdr["bw"], hdr["bh"]))
        for c in range(nc):
            np.testing.assert_array_equal(np.ctypeslib.as_array(info.qt[c]), hdr["qt"][c])
        want = R.flat_coefs(R.entropy_decode(blob, hdr))
        # into a slice of a larger, dirty buffer: absent coefficients come back zero and nothing beyond coef_bytes is written
        buf = np.full(want.size + 16, 0x5A5A, np.int16)
        got = ops.jpeg_entropy_decode(np.frombuffer(blob, np.uint8), info, out=buf[:want.size])
        np.testing.assert_array_equal(got, want, err_msg=f"case {i} {p}")
        assert (buf[want.size:] == 0x5A5A).all()


def test_unsupported_streams_yield_their_reason(g16):
    names = {getattr(_lib, k) for k in dir(_lib) if k.startswith("JPEG_R_")}
    for k, want in enumerate(g16["bad_reason"]):
        blob = g16[f"bad_{k}"].tobytes()
        info = ops.jpeg_parse(blob)
        assert info.supported == 0 and info.reason == int(want) and info.reason in names, (k, info.reason)
        assert R.parse(blob)["reason"] == int(want)
        rc = _lib.lib().fd_jpeg_entropy_decode(blob, len(blob), ctypes.byref(info), np.zeros(64, np.int16).ctypes.data, 128)
        assert rc == _lib.JPEG_E_UNSUPPORTED
    assert (_lib.JPEG_R_PROGRESSIVE, _lib.JPEG_R_ARITHMETIC, _lib.JPEG_R_PRECISION, _lib.JPEG_R_COMPONENTS, _lib.JPEG_R_RGB, _lib.JPEG_R_SAMPLING,
            _lib.JPEG_R_MULTISCAN, _lib.JPEG_R_DNL) == (R.R_PROGRESSIVE, R.R_ARITHMETIC, R.R_PRECISION, R.R_COMPONENTS, R.R_RGB, R.R_SAMPLING, R.R_MULTISCAN, R.R_DNL)


def _pick(g, sampling, h, w, restart):
    for i, p, blob, _ in _cases(g):
        if p[0] == sampling and (p[1], p[2]) == (h, w) and p[4] == restart and p[3] != 100:
            return blob
    raise AssertionError("no such case")


def test_every_prefix_is_an_error_or_a_success_never_a_crash(g16):
    lib = _lib.lib()
    codes = set(_lib.JPEG_ERRORS)
    for blob in (_pick(g16, 2, 17, 33, 1), _pick(g16, 0, 9, 17, 0)):
        full = ops.jpeg_parse(blob)
        want = ops.jpeg_entropy_decode(blob, full).copy()
        seen = set()
        for n in range(len(blob) + 1):
            part = np.frombuffer(blob[:n] + b"\xa5" * 8, np.uint8)[:n] if n else np.zeros(0, np.uint8)     # bytes beyond n are NOT the stream's
            info = _lib.JpegInfo()
            rc = lib.fd_jpeg_parse(part.ctypes.data, n, ctypes.byref(info))
            assert rc == 0 or rc in codes, (n, rc)
            if n < full.scan_offset:
                assert rc != 0, f"success on a {n}-byte prefix of headers that are {full.scan_offset} bytes long"
                seen.add(rc)
                continue
            assert rc == 0 and info.supported == 1
            out = np.empty(want.size, np.int16)
            rc = lib.fd_jpeg_entropy_decode(part.ctypes.data, n, ctypes.byref(info), out.ctypes.data, out.size * 2)
            assert rc == 0 or rc in codes, (n, rc)
            seen.add(rc)
            if rc == 0:
                np.testing.assert_array_equal(out, want)       # a prefix that decodes holds the whole scan
        assert 0 in seen and _lib.JPEG_E_TRUNCATED in seen
    # a buffer that is too small is refused before anything is written
    info = ops.jpeg_parse(blob)
    out = np.full(want.size, 7, np.int16)
    assert lib.fd_jpeg_entropy_decode(blob, len(blob), ctypes.byref(info), out.ctypes.data, out.size * 2 - 2) == _lib.JPEG_E_BUFFER and (out == 7).all()


def test_both_host_functions_from_eight_threads_at_once(g16):
    cases = _cases(g16)[::3]
    want = [ops.jpeg_entropy_decode(blob, ops.jpeg_parse(blob)).copy() for _, _, blob, _ in cases]
    bad = np.frombuffer(_pick(g16, 1, 33, 47, 0)[:200], np.uint8)

    def work(t):
        for rep in range(3):
            for k in range(t, len(cases), 8):
                got = ops.jpeg_entropy_decode(cases[k][2], ops.jpeg_parse(cases[k][2]))
                if not np.array_equal(got, want[k]):
                    return f"thread {t}: case {k} differs"
                try:                                            # failures interleaved with successes: no shared error state to trample
                    ops.jpeg_entropy_decode(bad, ops.jpeg_parse(bad))
                    return f"thread {t}: the truncated stream decoded"
                except FdError as e:
                    if e.rc != _lib.JPEG_E_TRUNCATED:
                        return f"thread {t}: rc {e.rc}"
        return None

    with ThreadPoolExecutor(8) as pool:
        assert [r for r in pool.map(work, range(8)) if r] == []


def test_jpeg_struct_layouts_match_c():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "fcosdet.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fd_jpeg_info), offsetof(fd_jpeg_info, restart_interval), offsetof(fd_jpeg_info, h_max),
        offsetof(fd_jpeg_info, bw), offsetof(fd_jpeg_info, dc_tab), offsetof(fd_jpeg_info, scan_offset), offsetof(fd_jpeg_info, coef_bytes), offsetof(fd_jpeg_info, qt),
        offsetof(fd_jpeg_info, huff_defined), offsetof(fd_jpeg_info, huff_bits), offsetof(fd_jpeg_info, huff_vals), sizeof(fd_jpeg_idct_job), offsetof(fd_jpeg_idct_job, bw));
      printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(fd_jpeg_idct_job, qt), sizeof(fd_jpeg_color_job), offsetof(fd_jpeg_color_job, plane_off), offsetof(fd_jpeg_color_job, stride),
        offsetof(fd_jpeg_color_job, rows), offsetof(fd_jpeg_color_job, width), offsetof(fd_jpeg_color_job, v_samp));
      printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", FD_JPEG_MAX_COMP, FD_JPEG_R_NONE, FD_JPEG_R_PROGRESSIVE, FD_JPEG_R_ARITHMETIC, FD_JPEG_R_PRECISION,
        FD_JPEG_R_COMPONENTS, FD_JPEG_R_RGB, FD_JPEG_R_SAMPLING, FD_JPEG_R_MULTISCAN, FD_JPEG_R_DNL, FD_JPEG_E_TRUNCATED, FD_JPEG_E_MARKER, FD_JPEG_E_HUFFMAN,
        FD_JPEG_E_COEF_INDEX, FD_JPEG_E_TABLE, FD_JPEG_E_BUFFER, FD_JPEG_E_UNSUPPORTED); return 0; }'''
    exe = os.path.join(ROOT, "oracle", "_build", "abi_probe_jpeg")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    I, J, K = _lib.JpegInfo, _lib.JpegIdctJob, _lib.JpegColorJob
    assert vals == [ctypes.sizeof(I), I.restart_interval.offset, I.h_max.offset, I.bw.offset, I.dc_tab.offset, I.scan_offset.offset, I.coef_bytes.offset, I.qt.offset,
                    I.huff_defined.offset, I.huff_bits.offset, I.huff_vals.offset, ctypes.sizeof(J), J.bw.offset,
                    J.qt.offset, ctypes.sizeof(K), K.plane_off.offset, K.stride.offset, K.rows.offset, K.width.offset, K.v_samp.offset,
                    _lib.JPEG_MAX_COMP, _lib.JPEG_R_NONE, _lib.JPEG_R_PROGRESSIVE, _lib.JPEG_R_ARITHMETIC, _lib.JPEG_R_PRECISION, _lib.JPEG_R_COMPONENTS, _lib.JPEG_R_RGB,
                    _lib.JPEG_R_SAMPLING, _lib.JPEG_R_MULTISCAN, _lib.JPEG_R_DNL, _lib.JPEG_E_TRUNCATED, _lib.JPEG_E_MARKER, _lib.JPEG_E_HUFFMAN, _lib.JPEG_E_COEF_INDEX,
                    _lib.JPEG_E_TABLE, _lib.JPEG_E_BUFFER, _lib.JPEG_E_UNSUPPORTED]
    assert ctypes.sizeof(J) == 32 and ctypes.sizeof(K) == 80 and ctypes.sizeof(I) % 8 == 0       # records of a device table: 8-byte multiples


def test_jpeg_symbols_are_declared_exported_and_built():
    with open(os.path.join(ROOT, "include", "fcosdet.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and name in _lib._SIGS and hasattr(lib, name), name
    for struct in ("fd_jpeg_info", "fd_jpeg_idct_job", "fd_jpeg_color_job"):
        assert "typedef struct " + struct in header, struct
    assert header.index("fd_jpeg_parse(") > header.index("fd_avg_copy_bytes(")


def test_launch_entry_points_reject_invalid_jobs_on_the_host():
    """Both launches validate the HOST copy of the job table before anything is enqueued: FD_E_INVAL and a message, no GPU needed (the pointers are fake)."""
    lib = _lib.lib()
    ptr = ctypes.c_void_p(4096)

    def idct(word, n=1, jobs_dev=ptr, coef_elems=64 * 6, n_q=2, planes_bytes=64 * 6, **over):
        jobs = (_lib.JpegIdctJob * 2)()
        for j in jobs:
            j.bw, j.bh, j.qt = 3, 2, 1
        for k, v in over.items():
            setattr(jobs[n - 1 if n >= 1 else 0], k, v)
        assert lib.fd_jpeg_idct_u8(jobs, jobs_dev, n, ptr, coef_elems, ptr, n_q, ptr, planes_bytes, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    idct(b"null pointer", jobs_dev=None)
    idct(b"job count", n=0)
    idct(b"job count", n=65536)
    idct(b"block grid", bw=0)
    idct(b"block grid", n=2, bh=8193)
    idct(b"coefficients outside", coef_off=1)
    idct(b"coefficients outside", coef_off=-64)
    idct(b"coefficients outside", coef_elems=64 * 6 - 1)
    idct(b"quantisation table", qt=2)
    idct(b"quantisation table", qt=-1)
    idct(b"plane outside", plane_off=8)
    idct(b"plane outside", n=2, plane_off=-8)
    idct(b"plane outside", planes_bytes=64 * 6 + 8, plane_off=4)           # inside, but not a multiple of 8
    idct(b"aligned", jobs_dev=ctypes.c_void_p(4100))

    def color(word, n=1, jobs_dev=ptr, planes_bytes=16 * 16 + 2 * 64, **over):
        jobs = (_lib.JpegColorJob * 2)()
        for j in jobs:                                                      # 4:2:0, 11 x 13: luma plane 16 x 16, chroma planes 8 x 8
            j.out, j.width, j.height, j.ncomp, j.h_samp, j.v_samp = 8192, 13, 11, 3, 2, 2
            j.plane_off[:], j.stride[:], j.rows[:] = [0, 256, 320], [16, 8, 8], [16, 8, 8]
        for k, v in over.items():
            tgt = jobs[n - 1 if n >= 1 else 0]
            if isinstance(v, tuple):
                getattr(tgt, k)[v[0]] = v[1]
            else:
                setattr(tgt, k, v)
        assert lib.fd_jpeg_color_u8(jobs, jobs_dev, n, ptr, planes_bytes, None) == _lib.E_INVAL
        assert word in lib.fd_last_error(), lib.fd_last_error()

    color(b"null pointer", jobs_dev=None)
    color(b"job count", n=0)
    color(b"out", out=None)
    color(b"out", n=2, out=8194)
    color(b"sides", width=0)
    color(b"sides", height=65536)
    color(b"components", ncomp=2)
    color(b"luma sampling", h_samp=1, v_samp=2)
    color(b"luma sampling", h_samp=4)
    color(b"luma sampling", ncomp=1)                                         # one component is 1 x 1
    color(b"smaller than the component", stride=(0, 12))
    color(b"smaller than the component", rows=(2, 5))
    color(b"smaller than the component", width=17)
    color(b"outside the buffer", plane_off=(2, 321))
    color(b"outside the buffer", plane_off=(1, -1))
    color(b"outside the buffer", planes_bytes=16 * 16 + 2 * 64 - 1)


def test_decoder_refusals_and_fallback_choice_without_gpu(g16):
    with pytest.raises(FdError, match="GPU only"):
        JpegDecoder("cpu")
    with pytest.raises(FdError, match="fallback"):
        JpegDecoder("cuda:0", fallback="eager")
    for bad in (0, -1, 2.5, True):
        with pytest.raises(FdError, match="threads"):
            JpegDecoder("cuda:0", threads=bad)
    assert JpegDecoder("cuda:0").threads == 16 and JpegDecoder("cuda:0", threads=64).threads == 16 and JpegDecoder("cuda:0", threads=3).threads == 3
    dec = JpegDecoder("cuda:0", fallback="raise")          # the constructor touches no device
    good = [g16["jpg_0"].tobytes(), g16["jpg_20"], g16["jpg_57"].tobytes()]
    for empty in ([], b"", good[0]):
        with pytest.raises(FdError, match="non-empty list"):
            dec.classify(empty)
    streams, infos, routes = dec.classify(good)
    assert routes == ["hip"] * 3 and [i.supported for i in infos] == [1, 1, 1] and all(s.dtype == np.uint8 for s in streams)
    for k, reason in enumerate(g16["bad_reason"]):
        with pytest.raises(FdError, match=r"stream 1 is not supported by the HIP path: " + re.escape(_lib.JPEG_REASONS[int(reason)])) as ei:
            dec.classify([good[0], g16[f"bad_{k}"].tobytes()])
        assert ei.value.rc == _lib.E_UNSUPPORTED
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    soft = JpegDecoder("cuda:0", fallback="pil")
    if have_pil:
        assert soft.classify([g16["bad_0"].tobytes(), good[1], g16["bad_1"]])[2] == ["pil", "hip", "pil"]
    else:
        with pytest.raises(FdError, match="PIL is not installed"):
            soft.classify([g16["bad_0"].tobytes()])
    # a corrupt stream always raises, whatever the fallback, and names its index
    for d in (dec, soft):
        with pytest.raises(FdError, match="stream 2 is corrupt") as ei:
            d.classify([good[0], good[1], good[2][:100]])
        assert ei.value.rc == _lib.JPEG_E_TRUNCATED
        with pytest.raises(FdError, match="stream 0 is corrupt"):
            d.classify([b"not a jpeg at all", good[0]])
    with pytest.raises(FdError, match="bytes or a uint8 array"):
        dec.classify([3.5])
    with pytest.raises(FdError, match="GPU only"):
        decode_jpeg_batch(good, device="cpu")


def test_decoder_reads_paths(tmp_path, g16):
    p = tmp_path / "a.jpg"
    p.write_bytes(g16["jpg_5"].tobytes())
    streams, infos, routes = JpegDecoder("cuda:0").classify([str(p), p])
    assert routes == ["hip", "hip"] and streams[0].tobytes() == streams[1].tobytes() == g16["jpg_5"].tobytes()
