"""The workspace carves of the format operations (spmm_amd/csrc/spg_format_layouts.hpp): where the
regions of a caller's workspace lie and what the size queries answer, for spg_csr2csc, spg_csrgeam,
spg_dense2csr, spg_canonicalize and spg_csr_extract.

The header is host arithmetic; here it runs built into tests/hip/format_layouts_check.cpp with g++
(no device).  Shape lines go in, every field of the matching layout comes out, and over a fixed
table of the smallest shapes on each seam:

  (a) structure   every region starts on a multiple of 256, the regions a mode has ascend in carve
                  order without overlap (their sizes restated here from the shapes), `total` is the
                  end of the last one rounded up to 256 plus 256, and a region the mode does not
                  need is absent (offset 0, no bytes in `total`);
  (b) widths      pass counts, key widths and first shifts, derived here from the shapes alone;
  (c) recording   every printed field equals tests/golden/format_layouts.json, recorded by the same
                  program when the carves were moved out of spgemm.hip unchanged.  No tolerance;
  (d) the cap     for the geometry tests/large_offsets.py uses past 2**31 entries, every layout's
                  `total` is at most the workspace share planned_bytes allots to its test (the GPU
                  tests cap their memory by that figure).

This is arithmetic on 64-bit counts: nothing is allocated, whatever the entry count says.
"""
import json
import os
import shutil
import subprocess

import pytest

from tests import large_offsets as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "format_layouts.json")

SCAN_TILE, TR_CHUNK, TR_RADIX, GM_CHUNK, DV_S, DV_T = 2048, 2048, 256, 1024, 1024, 64
NNZ = [0, 1, 2047, 2048, 2049, (1 << 31) - 1, 1 << 31, (1 << 32) + 5]
WIDTHS = [256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1]      # one .. four digit passes, each side of a seam
SORT, SUM, DROP = 1, 2, 4
ROW_SELS = ["whole", "range 3 1 500", "range 999 -2 500", "list 70"]
LIST_COUNTS = [0, 1, 300, 2047, 2048, 2049]


def _fits(bits, nnz):
    return bits == 64 or nnz < (1 << 31)          # (check_csr: an int32 row pointer holds nnz)


def _table():
    """Every shape line of the test, in a fixed order."""
    out = []
    for bits in (32, 64):
        for nnz in (n for n in NNZ if _fits(bits, n)):
            out += [f"tr {bits} 1000 {cols} {nnz}" for cols in WIDTHS + [1]]
            out += [f"gm {bits} {rows} 300 {nnz} {nb}" for rows in (0, 2048, 2049)
                    for nb in (0, 2049, NNZ[-1]) if _fits(bits, nb)]
            out += [f"gm {bits} 2049 300 2049 {nnz}"]
            for coo in (0, 1):
                for ops in range(8):
                    if not coo and ops == 0:
                        continue                   # (cn_check: CSR input with nothing to do)
                    shapes = [(65536, 65536), (65536, 65537)] if nnz in (0, 2049, NNZ[-1]) else [(65536, 65537)]
                    if nnz == 2049:
                        shapes += [(1, 1), (256, 257), ((1 << 24) + 1, 256), (300, (1 << 31) - 1)]
                    out += [f"cn {bits} {m} {n} {nnz} {coo} {ops}" for m, n in shapes]
            for rsel in ROW_SELS:
                out += [f"ex {bits} 1000 70000 {nnz} {rsel} {ksel}"
                        for ksel in ("whole", "range 69999 -3 2049", "list 300")]
        for cols in WIDTHS + [1]:
            out += [f"ex {bits} 1000 {cols} 2049 whole list {k}" for k in LIST_COUNTS]
    for order in ("row", "col"):
        for rows in (0, 1, DV_T - 1, DV_T, DV_T + 1, (1 << 24) + 1):
            out += [f"dn {order} {rows} {cols}" for cols in (0, 1, DV_S - 1, DV_S, DV_S + 1, 65537)]
    return list(dict.fromkeys(out))      # (the sweeps meet in a few shapes)


def _build(directory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = os.path.join(str(directory), "format_layouts_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "spmm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hip", "format_layouts_check.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, lines):
    """{shape line: {field: value}} by the program."""
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, check=True)
    rows = r.stdout.splitlines()
    assert len(rows) == len(lines)
    return {ln: {k: int(v) for k, v in (f.split("=") for f in row.split())} for ln, row in zip(lines, rows)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("format_layouts"))


@pytest.fixture(scope="module")
def layouts(exe):
    return _ask(exe, _table())


# ------------------------------------------------------------------ the carves restated

def _up(x):
    return -(-x // 256) * 256


def _ceil(a, b):
    return -(-a // b)


def _status(n):
    return 8 * ((_ceil(n, SCAN_TILE) if n > 0 else 1) + 1)


def _bits(extent):
    return max(1, (extent - 1).bit_length()) if extent > 0 else 1


def _sel_count(words, extent):
    """(kind, count, step, consumed words) of a selection at the head of `words`."""
    if words[0] == "whole":
        return "whole", extent, 1, 1
    if words[0] == "range":
        count = int(words[3])
        return "range", count, int(words[2]) if count > 1 else 1, 4
    return "list", int(words[1]), 1, 2


def _regions(line):
    """([(field, bytes)] of the regions this shape has, in carve order; [fields it has not];
    {field: value} derived from the shape alone)."""
    w = line.split()
    op = w[0]
    scal = ("scalars", 128)
    if op == "tr":
        ips, cols, nnz = int(w[1]) // 8, int(w[3]), int(w[4])
        passes = max(1, _ceil(_bits(cols), 8))
        chunks, nbuf = _ceil(nnz, TR_CHUNK), min(passes - 1, 2)
        rec = _up(4 * nnz) * 2 + _up(ips * nnz)
        have = [scal, ("status", _status(TR_RADIX * chunks)), ("table", ips * (TR_RADIX * chunks + 1)),
                ("skeys", 4 * nnz)] + [(f"buf{b}", rec) for b in range(nbuf)]
        derived = dict(passes=passes, chunks=chunks, nbuf=nbuf, keys=0, rowids=_up(4 * nnz), pos=2 * _up(4 * nnz))
        return have, [f"buf{b}" for b in range(nbuf, 2)], derived
    if op == "gm":
        ips, rows, na, nb = int(w[1]) // 8, int(w[2]), int(w[4]), int(w[5])
        have = [scal, ("status_b", _status(nb)), ("status_r", _status(rows)), ("S", ips * (nb + 1)),
                ("cnt", 8 * (rows + 1))]
        return have, [], dict(chunksA=_ceil(na, GM_CHUNK), chunksB=_ceil(nb, GM_CHUNK))
    if op == "dn":
        col, rows, cols = w[1] == "col", int(w[2]), int(w[3])
        nseg = max(1, _ceil(cols, DV_S))
        entries = rows * nseg
        have = [scal, ("status", _status(entries)), ("table", 8 * (entries + 1))]
        return have, [], dict(nseg=nseg, entries=entries, tasks=_ceil(rows, DV_T) * nseg if col else entries)
    if op == "cn":
        ips, rows, cols, nnz, coo, ops = int(w[1]) // 8, int(w[2]), int(w[3]), int(w[4]), int(w[5]), int(w[6])
        sort, marks = bool(ops & (SORT | SUM)), bool(ops & (SUM | DROP))
        cbits, rbits = _bits(cols), _bits(rows)
        k64 = cbits + rbits > 32
        shift0 = 0 if sort else cbits
        passes = _ceil(cbits + rbits - shift0, 8) if sort or coo else 0
        chunks = _ceil(nnz, TR_CHUNK)
        have, lacks = [scal], []
        if passes:
            have += [("status_t", _status(TR_RADIX * chunks)), ("table", ips * (TR_RADIX * chunks + 1))]
        else:
            lacks += ["status_t", "table", "buf0", "buf1"]
        if marks:
            have += [("status_k", _status(nnz)), ("kept", ips * (nnz + 1))]
        else:
            lacks += ["status_k", "kept"]
        if passes:
            have += [(f"buf{b}", (8 if ips == 4 and not k64 else 16) * nnz) for b in range(2)]
        derived = dict(sum=int(bool(ops & SUM)), drop=int(bool(ops & DROP)), marks=int(marks), cbits=cbits, rbits=rbits,
                       k64=int(k64), shift0=shift0, passes=passes, chunks=chunks)
        return have, lacks, derived
    assert op == "ex"
    ips, rows, cols, nnz = int(w[1]) // 8, int(w[2]), int(w[3]), int(w[4])
    rkind, rcount, rstep, used = _sel_count(w[5:], rows)
    kkind, kcount, _, _ = _sel_count(w[5 + used:], cols)
    kmode = {"whole": 0, "range": 1, "list": 2}[kkind]
    s64 = kmode == 2 or ips == 8
    have, lacks = [scal, ("status_r", _status(rcount)), ("cnt", 8 * (rcount + 1))], []
    if kmode:
        have += [("status_e", _status(nnz)), ("S", (8 if s64 else 4) * (nnz + 1))]
    else:
        lacks += ["status_e", "S"]
    passes = kchunks = 0
    if kmode == 2:
        passes, kchunks = _ceil(_bits(cols), 8), _ceil(kcount, TR_CHUNK)
        have += [("status_t", _status(TR_RADIX * kchunks)), ("table", 4 * (TR_RADIX * kchunks + 1)),
                 ("colptr", 4 * (cols + 1)), ("buf0", 8 * kcount), ("buf1", 8 * kcount)]
    else:
        lacks += ["status_t", "table", "colptr", "buf0", "buf1"]
    derived = dict(kmode=kmode, s64=int(s64), contig=int(kmode == 0 and rkind != "list" and rstep == 1), passes=passes,
                   kchunks=kchunks, rcount=rcount, kcount=kcount)
    return have, lacks, derived


# ------------------------------------------------------------------ (a) structure

def test_regions_are_aligned_ordered_and_disjoint(layouts):
    for line, L in layouts.items():
        have, lacks, _ = _regions(line)
        end = 0
        for name, size in have:
            assert L[name] % 256 == 0, (line, name)
            assert L[name] >= end, f"{line}: {name} at {L[name]} starts inside the region before it (ends {end})"
            assert L[name] < end + 256, f"{line}: a gap before {name}"
            end = L[name] + size
        assert L["total"] == _up(end) + 256, (line, L["total"], end)
        for name in lacks:
            assert L[name] == 0, f"{line}: {name} is carved though the mode has no use for it"
        if line.startswith("tr"):      # inside one record buffer: keys | row ids | positions
            assert L["keys"] == 0 and L["rowids"] % 256 == 0 and L["pos"] % 256 == 0
            assert L["keys"] + 4 * int(line.split()[4]) <= L["rowids"] and L["rowids"] + 4 * int(line.split()[4]) <= L["pos"]


def test_unneeded_regions_are_not_carved(layouts):
    """The three examples by name: no table without passes, no S for K = all, no kept marks
    without SUM or DROP_ZEROS."""
    seen = set()
    for line, L in layouts.items():
        w = line.split()
        if w[0] == "cn":
            if L["passes"] == 0:
                assert (L["table"], L["status_t"], L["buf0"], L["buf1"]) == (0, 0, 0, 0), line
                seen.add("no passes")
            if not int(w[6]) & (SUM | DROP):
                assert (L["kept"], L["status_k"]) == (0, 0), line
                seen.add("no marks")
        if w[0] == "ex" and L["kmode"] == 0:
            assert (L["S"], L["status_e"], L["colptr"]) == (0, 0, 0), line
            seen.add("K = all")
    assert seen == {"no passes", "no marks", "K = all"}


# ------------------------------------------------------------------ (b) pass counts and key widths

def test_derived_fields(layouts):
    for line, L in layouts.items():
        for name, want in _regions(line)[2].items():
            assert L[name] == want, f"{line}: {name} is {L[name]}, the shape says {want}"


def test_pass_counts_and_key_widths(layouts):
    # the transpose: one to four passes at the widths on each side of a byte of cols - 1
    tr = {int(ln.split()[3]): L["passes"] for ln, L in layouts.items() if ln.startswith("tr 64 ") and ln.endswith(" 2049")}
    assert [tr[c] for c in WIDTHS] == [1, 2, 2, 3, 3, 4] and tr[1] == 1
    # a column list of the extraction: the same rule over cols
    ex = {int(ln.split()[3]): L["passes"] for ln, L in layouts.items() if ln.startswith("ex 32 ") and ln.endswith("list 300")
          and "whole list" in ln}
    assert [ex[c] for c in WIDTHS] == [1, 2, 2, 3, 3, 4]
    cn = {ln: L for ln, L in layouts.items() if ln.startswith("cn")}
    # two 65536s fit a 32-bit key, one column more does not
    assert not any(L["k64"] for ln, L in cn.items() if " 65536 65536 " in ln)
    assert all(L["k64"] for ln, L in cn.items() if " 65536 65537 " in ln)
    for ln, L in cn.items():
        coo, ops = int(ln.split()[5]), int(ln.split()[6])
        # Only the rows are sorted (the first digit starts at cbits) exactly when neither SORT nor
        # SUM is asked for.  With passes to run that is COO input alone -- with no op, or with
        # DROP_ZEROS, which drops after the grouping and asks for no column order either.
        assert (L["shift0"] == L["cbits"]) == (not ops & (SORT | SUM)), ln
        if L["passes"] and L["shift0"]:
            assert coo and ops in (0, DROP), ln
        if coo and ops == 0:
            assert L["shift0"] == L["cbits"] and L["passes"] == -(-L["rbits"] // 8), ln
        assert (L["passes"] == 0) == (not coo and ops == DROP), ln      # CSR with DROP_ZEROS alone: no sort
    # S is int64 under any column list, whatever A's row pointer
    assert all(L["s64"] for ln, L in layouts.items() if ln.startswith("ex") and L["kmode"] == 2)
    assert any(not L["s64"] for ln, L in layouts.items() if ln.startswith("ex 32 ") and L["kmode"] == 1)


# ------------------------------------------------------------------ (c) the recording

def test_every_field_equals_the_recording(layouts):
    with open(GOLDEN) as f:
        golden = json.load(f)
    fields, rows = golden["fields"], golden["rows"]
    assert sorted(rows) == sorted(layouts), "the table and the recording list different shapes"
    for line, L in layouts.items():
        names = fields[line.split()[0]]
        assert sorted(L) == sorted(names), f"{line}: the program prints {sorted(L)}"
        assert [L[n] for n in names] == rows[line], f"{line}: {L}, recorded {dict(zip(names, rows[line]))}"


# ------------------------------------------------------------------ (d) the memory cap past 2**31 entries

def test_full_geometry_workspaces_within_planned_share(exe):
    g = lo.Geometry(**lo.FULL)
    assert g.nnz > 1 << 31
    share = lo.workspace_share(g)
    touched, Bs = g.small_operand()
    canon_nnz = (g.pad_nnz + sum(len(g.canon_marked_row(i)[0]) - g.L for i in g.marked_rows())
                 + int(g.canon_tail_input()[0][-1]))
    ask = {
        "csr2csc": [f"tr 64 {g.rows} {g.W} {g.nnz}"],
        # big + small and small + big, each with a workspace of its own
        "csrgeam": [f"gm 64 {g.rows} {g.W} {g.nnz} {Bs.nnz}", f"gm 64 {g.rows} {g.W} {Bs.nnz} {g.nnz}"],
        "canonicalize_sum": [f"cn 64 {g.rows} {g.W} {canon_nnz} 0 {SORT | SUM}"],
        "canonicalize_drop": [f"cn 64 {g.rows} {g.W} {g.nnz} 0 {DROP}"],
        "canonicalize_coo": [f"cn 64 {g.rows} {g.W} {g.nnz} 1 0"],
        "dense": [f"dn row {g.rows} {g.W}"],
        # cusparse.dense2csr, then cusparse.csrgeam2 of big + small
        "shim": [f"dn row {g.rows} {g.W}", f"gm 64 {g.rows} {g.W} {g.nnz} {Bs.nnz}"],
    }
    got = _ask(exe, sorted({ln for lines in ask.values() for ln in lines}))
    for test, lines in ask.items():
        total = sum(got[ln]["total"] for ln in lines)
        print(f"{test}: the carves ask for {total} bytes, planned_bytes allots {share[test]}")
        assert total <= share[test], f"{test}: the carves ask for {total} bytes, planned_bytes allots {share[test]}"


if __name__ == "__main__":      # records tests/golden/format_layouts.json anew (only when a carve is meant to change)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        answers = _ask(_build(d), _table())
    names = {}
    for ln, L in answers.items():
        names.setdefault(ln.split()[0], list(L))
    with open(GOLDEN, "w") as f:
        json.dump({"fields": names, "rows": {ln: [L[n] for n in names[ln.split()[0]]] for ln, L in answers.items()}},
                  f, separators=(",", ":"))
        f.write("\n")
