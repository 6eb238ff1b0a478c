"""The FD_* environment variables the package reads are the ones INTEGRATION.md lists -- no more, no fewer -- and the removed ones stay removed."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch_object_detection_amd")

# closed A/B experiments: the variable, its module constant and the plan-builder branch only it reached were deleted together
REMOVED = ("FD_STEM_KERNEL", "FD_STEM_POOL", "FD_STEM_NCHW", "FD_DUAL_DS", "FD_B2B", "FD_B2B_MIN_ROWS", "FD_TOWER_TAIL_SPLIT", "FD_TOWER_GN_SPLIT",
           "FD_GN_FUSED_TOWER", "FD_FPN_UP_FUSED", "FD_MBCONV_FUSED", "FD_SE_GATE_FUSED", "FD_WAVE_TILE", "FD_NARROW", "FD_W4_SK_TRACE", "FD_CONV_GEMM",
           "FD_W4_SK_P")

_READ = re.compile(r"""(?:environ\s*(?:\.get\s*\(|\[)|getenv\s*\()\s*["'](FD_[A-Z0-9_]+)["']""")


def _sources():
    files = glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)
    for ext in ("hip", "h", "inc"):
        files += glob.glob(os.path.join(PKG, "csrc", "*." + ext))
    assert len(files) > 40, files
    return {f: open(f, encoding="utf-8").read() for f in sorted(files)}


def test_environment_reads_match_the_documented_knob_list():
    read = set()
    for text in _sources().values():
        read.update(_READ.findall(text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    listed = set()
    for line in doc.splitlines():
        if line.startswith("- `FD_"):       # one bullet per variable (or per pair that belongs together), names in front of the dash
            listed.update(re.findall(r"`(FD_[A-Z0-9_]+)", line.split("—")[0]))
    assert len(read) >= 10 and read == listed, f"read but not listed: {sorted(read - listed)}; listed but not read: {sorted(listed - read)}"


def test_removed_knobs_are_gone_from_the_package():
    for path, text in _sources().items():
        for name in REMOVED:
            assert not re.search(r"(?<![A-Z0-9_])" + name + r"(?![A-Z0-9_])", text), f"{name} is back in {os.path.relpath(path, ROOT)}"
