"""Submatrix extraction (spg_csr_extract_nnz / spg_csr_extract) on a matrix of more than 2**31 stored
entries: the operand of tests/large_offsets.py (2**31 + 102 pad entries and a tail behind them,
int64 row pointer, fp32), built on the device, with the memory gate of
tests/test_gpu_large_offsets.py -- each test prints the device bytes it needs and skips only when
torch.cuda.mem_get_info() reports less.

  * the tail rows as a list (reversed, one of them twice) x the column range [64, 192): every source
    position, and every index into the scanned marks S, lies above 2**31; compared with scipy's
    result on the tail bit for bit;
  * spg_csr_extract_nnz over all rows and all columns into an int32 row pointer: SPG_STATUS_OVERFLOW
    with *nnzC == nnz (the count path alone; no output arrays).
"""
import ctypes

import numpy as np
import pytest

from tests import index_cases as ic
from tests import large_offsets as lo
from tests.guarded import guarded
from tests.test_gpu_large_offsets import _desc, _handle, _operand_intact, _require, big   # noqa: F401  (big: the fixture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OVERFLOW = 100
INT32_MAX = 2 ** 31 - 1


def test_tail_rows_by_list_and_a_column_range(big):
    from spmm_amd import _lib
    g, A = big.g, big.A
    assert big.full and g.pad_nnz > INT32_MAX
    h = _handle()
    va = _desc(A)
    order = list(range(g.rows - 1, g.pad_rows - 1, -1)) + [g.pad_rows + 5]
    idx = torch.tensor(order, dtype=torch.int32, device=DEV)
    rows = _lib.SpgSel(0, 0, len(order), idx.data_ptr())
    cols = _lib.SpgSel(64, 1, 128, None)
    need, nnz = ctypes.c_size_t(0), ctypes.c_int64(-1)
    st = h.lib.spg_csr_extract_nnz(h.ptr, ctypes.byref(va), ctypes.byref(rows), ctypes.byref(cols), None,
                                   _lib.SPG_INDEX_32I, ctypes.byref(nnz), ctypes.byref(need), None)
    assert st == 0 and need.value > 8 * g.nnz, (st, need.value)       # S: one int64 per stored entry
    _require("spg_csr_extract", 3 * 8192 + 16 * g.tail.nnz + lo.planned_bytes(g)["validate"], need.value)
    ws = guarded(need.value, np.uint8, 0xFF, DEV, "workspace")
    cp = guarded(len(order) + 1, np.int32, 0xFF, DEV, "C.indptr")
    have = ctypes.c_size_t(need.value)
    st = h.lib.spg_csr_extract_nnz(h.ptr, ctypes.byref(va), ctypes.byref(rows), ctypes.byref(cols),
                                   ctypes.c_void_p(cp.data_ptr()), _lib.SPG_INDEX_32I, ctypes.byref(nnz),
                                   ctypes.byref(have), ctypes.c_void_p(ws.data_ptr()))
    assert st == 0, st
    T = g.tail
    local = [r - g.pad_rows for r in order]
    R = T[local][:, 64:192]
    assert nnz.value == R.nnz > 0
    cj = guarded(R.nnz, np.int32, 0xFF, DEV, "C.indices")
    cx = guarded(R.nnz, np.float32, 0xFF, DEV, "C.values")
    vc = _lib.SpgCsr(len(order), 128, R.nnz, cp.data_ptr(), cj.data_ptr(), cx.data_ptr(), _lib.SPG_INDEX_32I,
                     _lib.SPG_R_32F)
    st = h.lib.spg_csr_extract(h.ptr, ctypes.byref(va), ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(vc),
                               ctypes.c_size_t(need.value), ctypes.c_void_p(ws.data_ptr()))
    assert st == 0, st
    torch.cuda.synchronize()
    for b in (cp, cj, cx, ws):
        b.check("spg_csr_extract " + b.name)
    got = (cp.t.cpu().numpy(), cj.t.cpu().numpy(), cx.t.cpu().numpy())
    ic.same_arrays((R.indptr, R.indices, R.data), got, "against scipy")
    ic.same_arrays(ic.expected(T, ("list", local), ("range", 64, 1, 128)), got, "against the rule")
    del ws
    _operand_intact(big)


def test_all_rows_overflow_an_int32_row_pointer(big):
    from spmm_amd import _lib
    g, A = big.g, big.A
    h = _handle()
    va = _desc(A)
    need, nnz = ctypes.c_size_t(0), ctypes.c_int64(-1)
    st = h.lib.spg_csr_extract_nnz(h.ptr, ctypes.byref(va), None, None, None, _lib.SPG_INDEX_32I, ctypes.byref(nnz),
                                   ctypes.byref(need), None)
    assert st == 0 and 0 < need.value < 16 * (g.rows + 1) + (1 << 20), (st, need.value)    # no per-entry array
    _require("spg_csr_extract_nnz", 4 * (g.rows + 1) + 2 * 8192, need.value)
    ws = guarded(need.value, np.uint8, 0xFF, DEV, "workspace")
    cp = guarded(g.rows + 1, np.int32, 0xFF, DEV, "C.indptr")
    have = ctypes.c_size_t(need.value)
    st = h.lib.spg_csr_extract_nnz(h.ptr, ctypes.byref(va), None, None, ctypes.c_void_p(cp.data_ptr()),
                                   _lib.SPG_INDEX_32I, ctypes.byref(nnz), ctypes.byref(have),
                                   ctypes.c_void_p(ws.data_ptr()))
    assert st == OVERFLOW and nnz.value == g.nnz > INT32_MAX, (st, nnz.value)
    torch.cuda.synchronize()
    cp.check("spg_csr_extract_nnz C.indptr")
    ws.check("spg_csr_extract_nnz workspace")
    # the same pass into an int64 row pointer is A's own
    cp64 = guarded(g.rows + 1, np.int64, 0xFF, DEV, "C.indptr")
    st = h.lib.spg_csr_extract_nnz(h.ptr, ctypes.byref(va), None, None, ctypes.c_void_p(cp64.data_ptr()),
                                   _lib.SPG_INDEX_64I, ctypes.byref(nnz), ctypes.byref(have),
                                   ctypes.c_void_p(ws.data_ptr()))
    assert st == 0 and nnz.value == g.nnz, (st, nnz.value)
    torch.cuda.synchronize()
    cp64.check("spg_csr_extract_nnz C.indptr")
    assert torch.equal(cp64.t, A.indptr)
