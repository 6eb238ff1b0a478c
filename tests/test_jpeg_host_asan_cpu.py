"""csrc/fd_jpeg_host.h under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone host program (tests/abi/jpeg_host_check.cpp): every prefix and 2 000
single-byte / single-bit mutations of a handful of fixture streams through fd_jpeg_parse and fd_jpeg_entropy_decode.  Nothing is preloaded, nothing goes through
Python, nothing runs on a GPU: the program is compiled with the host compiler and run as a child process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G16 = os.path.join(HERE, "golden", "g16_jpeg.npz")


def test_host_decoder_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_host_check")
    # the sanitizer runtimes linked statically (clang's default): the program then runs whatever else the loader brings into the process first
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [os.path.join(HERE, "abi", "jpeg_host_check.cpp"), "-o", exe], check=True)
    g = np.load(G16)
    p = g["params"]
    # one stream per sampling, with and without restart markers, one with optimised Huffman tables, one saturated: small ones (every prefix is decoded)
    want = [(0, 9, 17), (1, 17, 33), (2, 15, 16), (3, 16, 15), (2, 7, 3), (1, 8, 8)]
    files = []
    for s, h, w in want:
        i = next(i for i in range(len(p)) if (p[i, 0], p[i, 1], p[i, 2]) == (s, h, w))
        path = tmp_path / f"s{s}_{h}x{w}.jpg"
        path.write_bytes(g[f"jpg_{i}"].tobytes())
        files.append(str(path))
    i = next(i for i in range(len(p)) if p[i, 5] == 1 and p[i, 0] == 2)
    (tmp_path / "opt.jpg").write_bytes(g[f"jpg_{i}"].tobytes())
    files.append(str(tmp_path / "opt.jpg"))
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    line = run.stdout.strip().splitlines()[-1]
    print(line)
    assert f"{len(files)} streams" in line and " 0 inconsistencies" in line and f"{2000 * len(files)} mutations" in line
    decoded, errors = (int(line.split(f" {word}")[0].split()[-1]) for word in ("decoded", "error codes"))
    assert decoded > len(files) and errors > 1000          # both outcomes were exercised
