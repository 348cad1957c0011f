"""seg_place (spmm_amd/csrc/seg_place.hpp): where the segments of a dense tile's B records go.

The function is host and device text at once; here it runs on the host, built into
tests/hip/seg_place_check.cpp with g++ (no device).  Lists of segment lengths go in, the placed
byte offsets and the plan-time bound (seg_bound) come out, and for every list:

  1. no segment of <= 128 bytes crosses a 128-byte boundary;
  2. no segment touches more lines than ceil(L / 128) + (1 if L > 128 else 0);
  3. the segments keep their order and do not overlap;
  4. the end of the last segment is within the bound.

test_block_placement_within_bound places the same lists, and adversarial ones (one 1-record
segment per block of 64, at its start and at its end), the way the device pass does -- every 64
segments from a line boundary, each block rounded up to whole lines -- and checks the end against
seg_bound list by list and summed over all lists (the tiles of one workspace).

The compact layout (every segment right behind the one before) satisfies 2-4 on every list used
here; what the placement adds is 1, and the lists are checked to contain segments the compact
layout does carry across a boundary.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 128
REC_BYTES = (10, 6, 12, 20)     # f64, f32, complex64, complex128 records


def _lines(x, L):
    return 0 if L == 0 else (x + L - 1) // LINE - x // LINE + 1


def _lists():
    rng = np.random.default_rng(20240607)
    out = []
    for rb in REC_BYTES:
        per_line = LINE // rb
        out.append((rb, [0] * 200))                                            # all empty
        # every multiple of a line, one record either side of it (in records: the lengths whose
        # byte counts bracket 128, 256, ...), alone and alternating with single records
        edge = sorted({max(0, (m * LINE) // rb + d) for m in range(1, 5) for d in (-1, 0, 1)})
        out.append((rb, edge * 20))
        out.append((rb, [v for e in edge * 20 for v in (e, 1)]))
        for e in edge:
            out.append((rb, [e] * 70))
        out.append((rb, [per_line] * 100))                                     # as long as fits one line
        out.append((rb, [1] * 500))
        for mean in (1.5, 10.25, 25.0, 100.0):                                 # random lists
            out.append((rb, rng.poisson(mean, 600).tolist()))
        out.append((rb, rng.integers(0, 3 * per_line, 600).tolist()))
        out.append((rb, np.where(rng.random(600) < 0.7, 0, rng.integers(1, 40, 600)).tolist()))
    return out


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("seg_place") / "seg_place_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "spmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hip", "seg_place_check.cpp"), "-o", exe], check=True)
    lists = _lists()
    blists = lists + _block_lists()
    text = "".join(" ".join(str(v) for v in [rb] + list(lens)) + "\n" for rb, lens in lists)
    text += "".join("blocks " + " ".join(str(v) for v in [rb] + list(lens)) + "\n" for rb, lens in blists)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(lists) + len(blists)
    out = [(rb, lens, row[0], row[1:]) for (rb, lens), row in zip(lists, rows)]
    return out, [(rb, lens, row[0], row[1], row[2:]) for (rb, lens), row in zip(blists, rows[len(lists):])]


def _block_lists():
    out = []
    for rb in REC_BYTES:
        out.append((rb, ([1] + [0] * 63) * 40))          # one record per block, at its start
        out.append((rb, ([0] * 63 + [1]) * 40))          # ... at its end
        out.append((rb, ([0] * 31 + [1] + [0] * 32) * 40 + [1]))
        out.append((rb, [LINE // rb + 1] * 640))         # every segment one record over a line
        out.append((rb, [0] * 64 + [3] * 64 + [0] * 64))
    return out


def test_block_placement_within_bound(placed):
    total_end = total_nnz = total_segs = 0
    for rb, lens, bound, end, starts in placed[1]:
        assert len(starts) == len(lens)
        prev = 0
        for b0 in range(0, len(lens), 64):
            assert starts[b0] % LINE == 0 and starts[b0] >= prev          # a block starts on a line
            x = starts[b0]
            for n, at in zip(lens[b0:b0 + 64], starts[b0:b0 + 64]):
                L = n * rb
                assert x <= at < x + LINE and _lines(at, L) <= -(-L // LINE) + (1 if L > LINE else 0)
                if 0 < L <= LINE:
                    assert at // LINE == (at + L - 1) // LINE
                x = at + L
            prev = x
        assert end % LINE == 0 and prev <= end < prev + LINE
        assert end <= bound, (rb, end, bound)
        if rb == 10:      # the lists of one record size together: the tiles of one workspace
            total_end, total_nnz, total_segs = total_end + end, total_nnz + sum(lens), total_segs + len(lens)
    assert total_end <= 10 * total_nnz + 126 * min(total_nnz, total_segs)


def test_placement_properties(placed):
    compact_crossings = 0
    for rb, lens, bound, starts in placed[0]:
        assert len(starts) == len(lens)
        end, cx = 0, 0
        for n, at in zip(lens, starts):
            L = n * rb
            what = f"rec_bytes={rb} L={L} at={at} end-before={end}"
            assert at >= end, what                                  # 3: order kept, no overlap
            assert at % 2 == 0 and at - end < LINE, what            # (a move is less than a line)
            if 0 < L <= LINE:
                assert at // LINE == (at + L - 1) // LINE, what     # 1
                compact_crossings += cx // LINE != (cx + L - 1) // LINE
            assert _lines(at, L) <= -(-L // LINE) + (1 if L > LINE else 0), what   # 2
            assert _lines(at, L) <= _lines(end, L), what            # (never more lines than unmoved)
            if L == 0:
                assert at == end, what
            end = at + L
            cx += L
        assert end <= bound, (rb, end, bound)                       # 4
        assert cx <= bound and bound == cx + 126 * min(sum(lens), len(lens))
    assert compact_crossings > 1000     # the compact layout does not have property 1 on these lists


def test_placement_keeps_what_fits(placed):
    """A segment that already touches no more lines than its length needs stays where it is."""
    for rb, lens, _, starts in placed[0]:
        end = 0
        for n, at in zip(lens, starts):
            L = n * rb
            if _lines(end, L) <= -(-L // LINE):
                assert at == end
            else:
                assert at == -(-end // LINE) * LINE
            end = at + L
