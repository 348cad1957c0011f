"""The workspace carve of spg_csr_binop_nnz / spg_csr_binop (BoLayout / bo_layout,
spmm_amd/csrc/spg_format_layouts.hpp), checked without a device.

The header is host arithmetic; it runs built into tests/hip/binop_layout_check.cpp, a stand-alone
program with its own main, compiled with g++ -- once plainly and once more with
-fsanitize=address,undefined, run as a program of its own (it is never loaded into python).  Over
nnz(A), nnz(B) in {0, 1, 2047, 2048, 2049, 2^31 - 1, 2^31, 2^32 + 5} (from 2^31 on with 64-bit
positions only) and rows in {0, 2048, 2049}:

  every region starts on a multiple of 256;
  the regions ascend in carve order without overlap and without a gap of 256 bytes or more, their
  sizes restated here from the shapes;
  `total` is the end of the last region rounded up to 256, plus 256;
  the chunk counts are the entry counts over GM_CHUNK, rounded up.

This is arithmetic on 64-bit counts: nothing is allocated, whatever the entry count says.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE, GM_CHUNK = 2048, 1024
NNZ = [0, 1, 2047, 2048, 2049, (1 << 31) - 1, 1 << 31, (1 << 32) + 5]
ROWS = [0, 2048, 2049]


def _table():
    return [f"{bits} {rows} 300 {na} {nb}" for bits in (32, 64) for rows in ROWS for na in NNZ for nb in NNZ
            if bits == 64 or max(na, nb) < (1 << 31)]      # (check_csr: an int32 row pointer holds nnz)


def _build(directory, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = os.path.join(str(directory), "binop_layout_check" + ("_san" if sanitize else ""))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "spmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hip", "binop_layout_check.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = r.stdout.splitlines()
    assert len(rows) == len(lines)
    return {ln: {k: int(v) for k, v in (f.split("=") for f in row.split())} for ln, row in zip(lines, rows)}


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def layouts(request, tmp_path_factory):
    return _ask(_build(tmp_path_factory.mktemp("binop_layout"), request.param), _table())


def _up(x):
    return -(-x // 256) * 256


def _ceil(a, b):
    return -(-a // b)


def _status(n):
    return 8 * ((_ceil(n, SCAN_TILE) if n > 0 else 1) + 1)


def _regions(line):
    bits, rows, _, na, nb = (int(w) for w in line.split())
    ips = bits // 8
    return [("scalars", 128), ("status_a", _status(na)), ("status_b", _status(nb)), ("status_r", _status(rows)),
            ("SA", ips * (na + 1)), ("SB", ips * (nb + 1)), ("cnt", 8 * (rows + 1))]


def test_the_table_reaches_every_size():
    t = _table()
    assert len(t) == len(set(t)) == 3 * (6 * 6 + 8 * 8)
    assert f"64 2049 300 {(1 << 32) + 5} {(1 << 32) + 5}" in t and f"32 0 300 {(1 << 31) - 1} 0" in t
    assert not any(ln.startswith("32 ") and str(1 << 31) in ln.split()[3:] for ln in t)


def test_regions_are_aligned_ordered_and_disjoint(layouts):
    for line, L in layouts.items():
        end = 0
        assert L["scalars"] == 0
        for name, size in _regions(line):
            assert L[name] % 256 == 0, (line, name)
            assert L[name] >= end, f"{line}: {name} at {L[name]} starts inside the region before it (ends {end})"
            assert L[name] < end + 256, f"{line}: a gap before {name}"
            end = L[name] + size
        assert L["total"] == _up(end) + 256, (line, L["total"], end)
        assert sorted(L) == sorted([n for n, _ in _regions(line)] + ["chunksA", "chunksB", "total"])


def test_chunk_counts(layouts):
    for line, L in layouts.items():
        _, _, _, na, nb = (int(w) for w in line.split())
        assert L["chunksA"] == _ceil(na, GM_CHUNK) and L["chunksB"] == _ceil(nb, GM_CHUNK), line


def test_sizes_past_int32(layouts):
    """The two mark arrays of 2^32 + 5 entries each take 8 bytes per position: more than 2^36 bytes."""
    L = layouts[f"64 2049 300 {(1 << 32) + 5} {(1 << 32) + 5}"]
    assert L["SB"] - L["SA"] == _up(8 * ((1 << 32) + 6)) and L["total"] > 1 << 36
