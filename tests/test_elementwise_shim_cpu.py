"""What the element-wise entries of the Python shim (spmm_amd/cusparse.py: _binop_arrays, csrbinop,
_mul_dense_arrays, multiply_by_dense) ask of the engine, call by call, on the CPU: driven on small
CPU tensors against the fake library of tests/test_shim_calls_cpu.py, whose helpers are imported.

  the order of the calls: size query, structure call, value call;
  an int64 row pointer tried after an OVERFLOW answer;
  nnz(C) == 0: empty arrays and no value call;
  the op code that is passed;
  the dense view: order, ld and broadcast extents for row-major, column-major and strided tensors;
  every error with its type and message.
"""
import numpy as np
import pytest
import torch

from spmm_amd import _lib, cusparse as cs
from tests.test_shim_calls_cpu import C64, F64, I32, I64, OVERFLOW, _A, _args_of, _coo, _csc, _drive

BINOP = "spg_csr_binop_nnz"
ROW, COL = _lib.SPG_ORDER_ROW, _lib.SPG_ORDER_COL


def _binop(a, b, op):
    return lambda tr: cs._binop_arrays(*_args_of(a), *_args_of(b), (3, 4), op)


def _names(out):
    return [c[0] for c in out["calls"]]


@pytest.mark.parametrize("op", [0, 1, 2])
def test_call_order_and_op(op):
    out = _drive({BINOP: [{"size": 512}, {"nnz": 2}]}, _binop(_A(), _A(), op))
    assert _names(out) == ["get_handle", "set_stream", BINOP, BINOP, "spg_csr_binop"]
    query, structure, values = out["calls"][2:]
    # name, handle, op, A, B, C's row pointer, its type, &nnz, &ws_bytes, ws
    assert query[2] == structure[2] == values[2] == op
    assert query[5] == "null" and query[6] == 32 and query[9] == "null"                  # the size query
    assert structure[5] == "ptr" and structure[6] == 32 and structure[9] == "ptr"
    assert structure[8] == {"ref": "c_ulong", "value": 512} and values[6] == 512 and values[7] == "ptr"
    for call in (query, structure, values):
        for view in call[3:5]:
            assert view["struct"] == "SpgCsr" and (view["rows"], view["cols"], view["nnz"]) == (3, 4, 5)
            assert view["indptr_type"] == 32 and view["value_type"] == _lib.SPG_R_64F
            assert view["indptr"] == view["indices"] == view["values"] == "ptr"
    c = values[5]
    assert (c["rows"], c["cols"], c["nnz"], c["indptr_type"], c["value_type"]) == (3, 4, 2, 32, _lib.SPG_R_64F)
    assert out["result"] == [["torch.float64", [2], [1]], ["torch.int32", [2], [1]], ["torch.int32", [4], [1]]]


def test_overflow_retries_with_an_int64_row_pointer():
    out = _drive({BINOP: [{"size": 512}, {"status": OVERFLOW}, {"nnz": 2}]}, _binop(_A(), _A(), 0))
    assert _names(out)[2:] == [BINOP, BINOP, BINOP, "spg_csr_binop"]
    assert [c[6] for c in out["calls"][2:5]] == [32, 32, 64]
    assert out["calls"][5][5]["indptr_type"] == 64 and out["calls"][5][3]["indptr_type"] == 32   # C's, the operands'
    assert out["result"][2] == ["torch.int64", [4], [1]]


def test_operand_row_pointers_and_a_second_overflow():
    """The operands' row pointers are converted to one type, int32 while both entry counts fit; an
    OVERFLOW answer for the int64 row pointer too is raised."""
    out = _drive({BINOP: [{"size": 512}, {"nnz": 2}]}, _binop(_A(ipd=I64), _A(), 1))
    assert [v["indptr_type"] for v in out["calls"][3][3:5]] == [32, 32]
    out = _drive({BINOP: [{"size": 512}, {"status": OVERFLOW}, {"status": OVERFLOW}]}, _binop(_A(), _A(), 1))
    assert out["raises"] == ["SpgError", "spg_csr_binop_nnz: SPG_STATUS_OVERFLOW"]


def test_empty_result_makes_no_value_call():
    out = _drive({BINOP: [{"size": 512}, {"nnz": 0}]}, _binop(_A(), _A(), 0))
    assert _names(out)[2:] == [BINOP, BINOP]
    assert out["result"] == [["torch.float64", [0], [1]], ["torch.int32", [0], [1]], ["torch.int32", [4], [1]]]


def test_empty_operands_are_still_evaluated():
    """nnz(A) == 0 still runs both calls (0 * inf is NaN): null indices and values, a row pointer."""
    out = _drive({BINOP: [{"size": 512}, {"nnz": 1}]}, _binop(_A(0), _A(dt=F64), 0))
    assert _names(out)[2:] == [BINOP, BINOP, "spg_csr_binop"]
    a = out["calls"][3][3]
    assert (a["nnz"], a["indptr"], a["indices"], a["values"]) == (0, "ptr", "null", "null")


def test_complex_value_type():
    out = _drive({BINOP: [{"size": 512}, {"nnz": 2}]}, _binop(_A(dt=C64), _A(dt=C64), 2))
    assert out["calls"][3][3]["value_type"] == _lib.SPG_C_32F and out["result"][0][0] == "torch.complex64"


# ------------------------------------------------------------------ the dense view
def _mul_dense(d, a=None, **kw):
    a = a or _A()
    return lambda tr: cs._mul_dense_arrays(*_args_of(a), (3, 4), d, **kw)


@pytest.mark.parametrize("name,d,want", [
    ("full_row_major", torch.ones(3, 4, dtype=F64), (3, 4, 4, ROW)),
    ("full_col_major", torch.ones(4, 3, dtype=F64).t(), (3, 4, 3, COL)),
    ("full_padded_ld", torch.ones(3, 9, dtype=F64)[:, :4], (3, 4, 9, ROW)),
    ("full_col_major_padded", torch.ones(4, 7, dtype=F64).t()[:3], (3, 4, 7, COL)),
    ("full_strided_is_copied", torch.ones(3, 8, dtype=F64)[:, ::2], (3, 4, 4, ROW)),
    ("row_vector", torch.ones(1, 4, dtype=F64), (1, 4, 4, ROW)),
    ("row_vector_expanded", torch.ones(4, dtype=F64).reshape(1, -1), (1, 4, 4, ROW)),
    ("col_vector", torch.ones(3, 1, dtype=F64), (3, 1, 1, ROW)),
    ("col_vector_of_a_matrix", torch.ones(3, 5, dtype=F64)[:, 2:3], (3, 1, 5, ROW)),
    ("one_by_one", torch.ones(1, 1, dtype=F64), (1, 1, 1, ROW)),
])
def test_dense_views(name, d, want):
    out = _drive({}, _mul_dense(d))
    assert _names(out) == ["get_handle", "set_stream", "spg_csr_mul_dense"]
    _, _, a, view, dst = out["calls"][2]
    assert (view["rows"], view["cols"], view["ld"], view["order"]) == want, name
    assert view["struct"] == "SpgDense" and view["values"] == "ptr" and view["value_type"] == _lib.SPG_R_64F
    assert (a["rows"], a["cols"], a["nnz"]) == (3, 4, 5) and dst == "ptr"
    assert out["result"] == ["torch.float64", [5], [1]]


def test_mul_dense_in_place_int64_and_empty():
    a = _A(ipd=I64)
    out = _drive({}, _mul_dense(torch.ones(3, 4, dtype=F64), a, out=a.data))
    assert out["calls"][2][2]["indptr_type"] == 64 and out["result"] == ["torch.float64", [5], [1]]
    out = _drive({}, _mul_dense(torch.ones(3, 4, dtype=F64), _A(0)))
    assert out["calls"] == [] and out["result"] == ["torch.float64", [0], [1]]      # nothing to write: no call


# ------------------------------------------------------------------ errors
def _raises(thunk, available=True):
    out = _drive({}, lambda tr: thunk(), available)
    assert out["calls"] == [], out["calls"]
    return tuple(out["raises"])


def test_csrbinop_errors():
    A, loose = _A(), _A(canonical=False)
    B = cs.csr_matrix._from_parts(torch.ones(1, dtype=F64), torch.zeros(1, dtype=I32), torch.tensor([0, 1, 1], dtype=I32),
                                  (2, 4), canonical=True)
    assert _raises(lambda: cs.csrbinop(A, A, "multiply"), False) == ("RuntimeError", "csrbinop is not available.")
    assert _raises(lambda: cs.csrbinop(_csc(A), A, "multiply")) == (
        "TypeError", "unsupported type (actual: <class 'spmm_amd.sparse.csc_matrix'>)")
    assert _raises(lambda: cs.csrbinop(A, _coo(), "maximum")) == (
        "TypeError", "unsupported type (actual: <class 'spmm_amd.sparse.coo_matrix'>)")
    assert _raises(lambda: cs.csrbinop(A, A, "divide")) == (
        "ValueError", "op must be one of multiply, maximum, minimum (actual: 'divide')")
    assert _raises(lambda: cs.csrbinop(loose, A, "minimum"))[0] == "AssertionError"
    assert _raises(lambda: cs.csrbinop(A, loose, "minimum"))[0] == "AssertionError"
    assert _raises(lambda: cs.csrbinop(A, B, "multiply")) == ("ValueError", "inconsistent shapes")
    assert _raises(lambda: cs.csrbinop(A, A, "multiply")) == (
        "RuntimeError", "csrbinop needs device-resident operands on one device")


def test_multiply_by_dense_errors():
    A, T = _A(), torch.ones(3, 4, dtype=F64)
    assert _raises(lambda: cs.multiply_by_dense(A, T), False) == ("RuntimeError", "multiply_by_dense is not available.")
    assert _raises(lambda: cs.multiply_by_dense(_csc(A), T)) == (
        "TypeError", "unsupported type (actual: <class 'spmm_amd.sparse.csc_matrix'>)")
    assert _raises(lambda: cs.multiply_by_dense(A, [[1.0]])) == ("TypeError", "unsupported type (actual: <class 'list'>)")
    for bad in (torch.ones(4), torch.ones(3, 5), torch.ones(2, 4), np.ones((4, 3))):
        assert _raises(lambda bad=bad: cs.multiply_by_dense(A, bad)) == ("ValueError", "inconsistent shapes")
    assert _raises(lambda: cs.multiply_by_dense(A, T)) == (
        "RuntimeError", "multiply_by_dense needs device-resident operands")
    assert _raises(lambda: cs._mul_dense_arrays(*_args_of(A), (3, 4), torch.ones(3, 4))) == (
        "TypeError", "d must be a tensor of the matrix's type on its device")
    assert _raises(lambda: cs._mul_dense_arrays(*_args_of(A), (3, 4), torch.ones(2, 4, dtype=F64))) == (
        "ValueError", "inconsistent shapes")


def test_a_library_without_the_entry_points_is_unavailable(monkeypatch):
    """A device and a library that has the addition but not these symbols: the same RuntimeError,
    and no call."""
    monkeypatch.setattr(cs, "has_elementwise", lambda: False)
    A = _A()
    assert _raises(lambda: cs.csrbinop(A, A, "multiply")) == ("RuntimeError", "csrbinop is not available.")
    assert _raises(lambda: cs.multiply_by_dense(A, torch.ones(3, 4, dtype=F64))) == (
        "RuntimeError", "multiply_by_dense is not available.")
