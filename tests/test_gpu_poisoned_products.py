"""The product kernels on poisoned, guarded buffers (tests/guarded.py).

The other parity tests hand the library fresh `torch.empty` arrays, which the caching allocator
usually recycles from the product before -- holding that product's correct C -- and they never
look outside an array.  Here every array the library writes (the workspace at exactly its queried
size, C's row pointer, indices and values, the tile-major values, the 16-bit column parts) lies
between two 4096-byte guard bands, is filled with 0xFF (an unwritten value is a NaN pattern, an
unwritten index -1) or 0x00 (for a kernel that relies on garbage being nonzero) before the call,
and the inputs are compared with what was uploaded afterwards.  Every result is bit for bit the
oracle's (inst.assert_same, no tolerance).

Per case of tests/instantiations.py (inst.run_poisoned): both poisons under ALG1, ALG2 and chunked
ALG3; spg_symbolic called twice (int32 then int64 row pointer) before spg_numeric on every path;
four products in one workspace that is poisoned once and then carries each product's leftovers
into the next; ALG1's hand-off of C in the workspace, copied out and in place; spg_spgemm_ws.
Outside the table: the two inputs on which ALG1's single pass gives up, spg_numeric_tiles over
partial tile ranges in both orders, and the 16-bit column split / join.

Guarded, per entry point (A's and B's arrays are compared with a second upload instead):
  spg_plan / spg_symbolic / spg_numeric   workspace, C.indptr (both calls of a repeated
                                          spg_symbolic), C.indices, C.values
  spg_result_in_workspace                 the views must lie inside the workspace's interior
  spg_spgemm_ws                           workspace, C.indptr; C.indices / C.values where it
                                          returns the live plan
  spg_tile_values / spg_numeric_tiles     tile-major values, workspace, C's three arrays
  spg_cols16_split / spg_cols16_join      block_starts, lo16, the joined indices
  spg_spmv, spg_spmm                      x / B and y / C with their leading-dimension padding
                                          (tests/test_gpu_dense_seams.py)
Not guarded: the handle's own scratch and pinned mirror (not reachable from outside), the
buffers cusparse.spgemm allocates itself, spg_tile_value_offsets' host array, and anything
further than 4096 bytes from an array.

What the poison shows that recycled buffers hide, tried on scratch builds that only omit stores:
k_numeric skipping the last store of the last row of every ALG3 chunk after the first fails
test_poisoned_case[general-*] here while test_instantiation[general-*], which runs the same
chunks after ALG1 and ALG2 have filled the recycled arrays, passes; k_spmv and k_spmm_col not
storing an empty row fail tests/test_gpu_dense_seams.py and nothing older.

Notes on reach: sparse8192-f64 has five numeric tiles in ONE value tile (record group 8), so its
only spg_numeric_tiles call is the whole product; sparse8192-f64-rg1 has the same inputs in five.
The two redo paths behind ALG1's single pass in spg_symbolic are each pinned by an assertion on
spg_result_in_workspace: an output past the estimate (estimate_overflow_pair on k_row: C is not in
the workspace), and a row the pass refuses (short-kshort-f64: k_short sets its fail flag for the
65-entry row, so nothing of that case stays in the workspace).  short64-kshort-f64 is that case
without the row: k_short's single pass holds, the repeated spg_symbolic only rescans the counts it
recorded, and C stays in the workspace.  long_row_pair on k_row reaches
neither: its 300-entry row is listed for the general kernel and C stays in the workspace, which
is asserted too.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import instantiations as inst

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests import instantiations as inst
inst.child_main({case!r}, {out!r}, "poisoned")
"""


def _run(case, tmp_path):
    env = inst.CASE[case].env
    if not any(k in env for k in inst.CHILD_ENV):
        return inst.run_poisoned(case)
    out = str(tmp_path / "poisoned.npz")      # a switch read once per process: a fresh one
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, case=case, out=out)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return inst.load_child(out)[0]


@pytest.mark.parametrize("case", inst.CASE_IDS)
def test_poisoned_case(case, tmp_path):
    c = inst.CASE[case]
    ref = inst.reference(case)
    ref_alpha = inst.reference(case, inst.alpha_of(c.dname))
    out = _run(case, tmp_path)
    want = {f"fill/{alg}/{fill:#04x}" for alg in inst.ALGS for fill in inst.POISON_FILLS}
    want |= {f"{k}/{alg}" for alg in inst.ALGS for k in ("resym", "resym-first")}
    want |= {f"stale/{i}/{alg}" for i, alg in enumerate(inst.STALE_ORDER)}
    want |= {"handoff/copy", "ws/1", "ws/2", "flags"}
    assert want <= set(out) <= want | {"handoff/inplace"}, sorted(set(out) ^ want)
    for key in sorted(out):
        kind = key.split("/")[0]
        if kind in ("fill", "resym", "stale"):
            inst.assert_same(out[key], ref, f"{case} {key}")
        elif kind in ("handoff", "ws"):
            inst.assert_same(out[key], ref_alpha, f"{case} {key}")
    # widths: both poisons saw both row-pointer widths
    for ai, alg in enumerate(inst.ALGS):
        for fi, fill in enumerate(inst.POISON_FILLS):
            cp = inst.POISON_WIDTHS[(ai + fi) % 2][1]
            assert out[f"fill/{alg}/{fill:#04x}"][0].dtype == (np.int32 if cp == 32 else np.int64)
    seen = {(fill, inst.POISON_WIDTHS[(ai + fi) % 2]) for ai in range(3) for fi, fill in enumerate(inst.POISON_FILLS)}
    assert len(seen) == 4
    # the repeated spg_symbolic: both row pointers the oracle's, nnzC the same both times
    for alg in inst.ALGS:
        p1, nn, _ = out[f"resym-first/{alg}"]
        assert p1.dtype == np.int32 and out[f"resym/{alg}"][0].dtype == np.int64
        assert np.array_equal(p1.astype(np.int64), np.asarray(ref[0], dtype=np.int64)), f"{case} alg={alg}: first row pointer"
        assert int(nn[0]) == int(nn[1]) == len(ref[1]), (case, alg, nn)
    # ALG1's hand-off: the short cases on k_row keep C in the workspace (their output is within
    # the estimate: tests/test_poisoned_products_cpu.py), so the in-place sequence and
    # spg_spgemm_ws's workspace result ran.  On k_short (short-kshort-f64) the single pass refuses
    # the 65-entry row (nA > 64 sets LB_FAIL) and the product is redone two-phase: nothing stays in
    # the workspace.  short64-kshort-f64 has no such row: k_short's single pass holds, and C stays
    # in the workspace through the two spg_symbolic calls of "resym".  No other path has a single pass.
    flags = [int(v) for v in out["flags"][1]]
    assert ("handoff/inplace" in out) == bool(flags[0])
    k_row_short = c.expect["path"] == "short" and not c.env
    single_pass_holds = k_row_short or case == "short64-kshort-f64"
    assert flags == ([1, 1, 0] if single_pass_holds else [0, 0, 0]), (case, flags)


@pytest.mark.parametrize("which", ["estimate_overflow", "long_row"])
def test_alg1_single_pass_gives_up_on_poisoned_buffers(which):
    """The two inputs tests/test_gpu_parity.py stresses ALG1's single pass with, on both poisons,
    and ALG2 in the same setting: an output past the estimate (the pass gives up, C is redone
    two-phase) and an A row past the 64 entries a wave takes (k_row lists it and carries on; the
    refusal of such a row is k_short's, pinned by test_poisoned_case[short-kshort-f64])."""
    from oracle import oracle
    A, B = getattr(inst, which + "_pair")()
    dA, dB = inst.Uploaded(A), inst.Uploaded(B)
    ref = oracle.spgemm(A, B, alpha=1.5, keep_zeros=True, sort=True)
    for fill in inst.POISON_FILLS:
        for alg in (1, 2):
            ex = {}
            got = inst.run_abi(dA, dB, alg, 1.5, inst.CF, 32, 32, fill=fill, extra=ex)
            inst.assert_same(got, ref, f"{which} alg={alg} fill={fill:#04x}")
            # estimate_overflow: nnz(C) is past the estimate, the single pass gave up and C was
            # redone two-phase; long_row: k_row lists the 300-entry row for the general kernel
            # and the pass holds (C stays in the workspace, copied out by spg_numeric)
            assert ex["in_workspace"] == (which == "long_row" and alg == 1), (which, alg)
    # and with the repeated spg_symbolic after the pass gave up
    got = inst.run_abi(dA, dB, 1, 1.5, inst.CF, 32, 64, first_cp=32, extra=ex)
    inst.assert_same(got, ref, f"{which} repeated spg_symbolic")
    assert np.array_equal(ex["first"][0].astype(np.int64), np.asarray(ref[0], dtype=np.int64))
    assert ex["first"][1] == ex["nnz"] == len(ref[1])


# value tiles: dense2048 has 9; sparse8192's five numeric tiles form ONE record group of 8, so its
# only call is the whole product -- the rg1 case has the same inputs in 5 value tiles
TILE_CASES = {"dense2048-f64": 9, "sparse8192-f64": 1, "sparse8192-f64-rg1": 5}


@pytest.mark.parametrize("case", list(TILE_CASES))
def test_numeric_tiles_partial_ranges(case):
    c = inst.CASE[case]
    A, B, _ = inst.inputs(case)
    ref = inst.reference(case)
    results, left, tiles = inst.run_tiles(A, B, 1.0, 32, 64, c.env)
    assert tiles == TILE_CASES[case], tiles
    names = [name for name, _ in inst.tile_groupings(tiles)]
    assert set(results) == set(names) and len(names) == (5 if tiles > 1 else 1)
    for name, ranges in inst.tile_groupings(tiles):
        inst.assert_same(results[name], ref, f"{case} {name}")
        # the calls are partial: poison is left after every call but the last, none after it
        assert len(left[name]) == len(ranges)
        assert all(n > 0 for n in left[name][:-1]) and left[name][-1] == 0, (case, name, left[name])
        assert all(a > b for a, b in zip(left[name], left[name][1:])), (case, name, left[name])


@pytest.mark.parametrize("ip", [32, 64])
@pytest.mark.parametrize("cols", inst.COLS16_WIDTHS)
def test_cols16_round_trip_guarded(cols, ip):
    from spmm_amd import _lib
    from tests.guarded import guarded
    M = inst.cols16_matrix(cols)      # (its rows: tests/test_poisoned_products_cpu.py)
    rows, nnz = M.shape[0], M.nnz
    starts, lo16 = inst.cols16_split_host(M)
    nb1 = starts.shape[1]
    dM = inst.Uploaded(M)
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    for fill in inst.POISON_FILLS:
        what = f"cols={cols} IP={ip} fill={fill:#04x}"
        gs = guarded(rows * nb1, "uint32", fill, "cuda:0", "block_starts")
        gl = guarded(nnz, "uint16", fill, "cuda:0", "lo16")
        gj = guarded(nnz, "int32", fill, "cuda:0", "joined indices")
        v = dM.view(ip)
        _lib.check(h.lib.spg_cols16_split(h.ptr, ctypes.byref(v), ctypes.c_void_p(gs.data_ptr()),
                                          ctypes.c_void_p(gl.data_ptr())), "spg_cols16_split")
        vj = _lib.SpgCsr(rows, cols, nnz, dM.indptr[ip].data_ptr(), gj.data_ptr(), 0, ip, v.value_type)
        _lib.check(h.lib.spg_cols16_join(h.ptr, ctypes.byref(vj), ctypes.c_void_p(gs.data_ptr()),
                                         ctypes.c_void_p(gl.data_ptr())), "spg_cols16_join")
        torch.cuda.synchronize()
        got_s = gs.bytes().cpu().numpy().view(np.uint32).reshape(rows, nb1)
        got_l = gl.bytes().cpu().numpy().view(np.uint16)
        assert np.array_equal(got_s, starts), what
        assert np.array_equal(got_l, lo16), what
        assert np.array_equal(gj.t.cpu().numpy(), M.indices), what
        for g in (gs, gl, gj):
            g.check(f"{what} {g.name}")
        dM.check_unchanged(what)
