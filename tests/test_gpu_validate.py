"""spg_validate_csr on the device (k_validate, spmm_amd/csrc/spgemm_kernels.hpp, and the host
decode of its two flag words in spmm_amd/csrc/spgemm.hip) against the loop reference of
tests/validate_cases.py, on the list tests/test_validate_cpu.py checks case by case.

Bar: status 0 and the reference's verdict for every case, with both row-pointer types; a verdict
never leaks from one call on a handle into the next (the flags live in handle scratch); the
host-only argument checks answer as include/spgemm.h states; one validate is one launch.

No case reads outside an allocation (validate_cases.reads_stay_inside, asserted before every
launch): only the values of the row pointer are ever wrong, and a row with a bad pointer is left
before an index is read.
"""
import ctypes

import numpy as np
import pytest

from tests import validate_cases as vc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOT_INITIALIZED, INVALID_VALUE, NOT_SUPPORTED = 1, 3, 10
CASES = vc.cases()
IDS = [c.id for c in CASES]
IPS = [torch.int32, torch.int64]
VALUE_TYPES = [torch.float32, torch.float64, torch.complex64, torch.complex128]


def _handle():
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream(0).cuda_stream)
    return h


class _Operand:
    """The device arrays of a case and their spg_csr_t, built the way cusparse._view builds it: an
    empty matrix has null indices and values."""

    def __init__(self, case, ip, vt=torch.float64, indices=None):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT
        assert vc.reads_stay_inside(case)
        self.case, nnz = case, case.nnz
        self.indptr = torch.from_numpy(case.indptr.copy()).to(ip).to(DEV)
        self.indices = torch.from_numpy((case.indices if indices is None else indices).copy()).to(DEV)
        self.data = torch.ones(nnz, dtype=vt, device=DEV)
        assert self.indptr.numel() == case.rows + 1 and self.indices.numel() == nnz
        self.view = _lib.SpgCsr(case.rows, case.cols, nnz, self.indptr.data_ptr(),
                                self.indices.data_ptr() if nnz else 0, self.data.data_ptr() if nnz else 0,
                                _IT[ip], _VT[vt])

    def matrix(self):
        from spmm_amd.sparse import csr_matrix
        return csr_matrix._from_parts(self.data, self.indices, self.indptr, (self.case.rows, self.case.cols),
                                      canonical=None)


def _validate(op, h=None):
    """(status, verdict) of one spg_validate_csr call; the verdict word starts at 7."""
    h = h or _handle()
    out = ctypes.c_int(7)
    st = h.lib.spg_validate_csr(h.ptr, ctypes.byref(op.view), ctypes.byref(out))
    return st, out.value


# ------------------------------------------------------------------ 1. the list
@pytest.mark.parametrize("ip", IPS, ids=["i32", "i64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_verdict_equals_reference(case, ip):
    want = vc.canon_status(case.indptr, case.indices, case.cols, case.nnz)
    assert want == case.expect
    assert _validate(_Operand(case, ip)) == (0, want)
    if case.repaired is not None:       # the same matrix with the pair repaired
        assert vc.canon_status(case.indptr, case.repaired, case.cols, case.nnz) == 1
        assert _validate(_Operand(case, ip, indices=case.repaired)) == (0, 1)


@pytest.mark.parametrize("ip", IPS, ids=["i32", "i64"])
@pytest.mark.parametrize("vt", [t for t in VALUE_TYPES if t != torch.float64], ids=["f32", "c64", "c128"])
def test_verdict_does_not_depend_on_the_value_type(vt, ip):
    for cid in (vc.CANONICAL_ID, vc.VIOLATING_ID):
        case = vc.by_id(cid)
        assert _validate(_Operand(case, ip, vt)) == (0, case.expect)


# ------------------------------------------------------------------ 2. handle state
def _sequence(ip):
    ops = [_Operand(vc.by_id(cid), ip) for cid in vc.SEQUENCE]
    assert [op.case.expect for op in ops] == list(vc.SEQUENCE_VERDICTS) == [-1, 1, 0, 1, -1, 1]
    return ops


@pytest.mark.parametrize("ip", IPS, ids=["i32", "i64"])
def test_no_verdict_leaks_into_the_next_call(ip):
    """-1, 1, 0, 1, -1, 1 on one handle, no synchronisation but validate's own."""
    h = _handle()
    ops = _sequence(ip)
    got = [_validate(op, h) for op in ops]
    assert got == [(0, v) for v in vc.SEQUENCE_VERDICTS]


@pytest.mark.parametrize("ip", IPS, ids=["i32", "i64"])
def test_no_verdict_leaks_across_another_call_on_the_handle(ip):
    """The same sequence with a spg_csr2csc between validates: it works on this handle too."""
    from spmm_amd import cusparse
    h = _handle()
    ops = _sequence(ip)
    T = _Operand(vc.by_id("r513-base"), ip)
    want_t = vc.by_id("r513-base")
    got, transposes = [], []
    for op in ops:
        got.append(_validate(op, h))
        transposes.append(cusparse._csr2csc_arrays(T.data, T.indices, T.indptr, want_t.rows, want_t.cols))
    assert got == [(0, v) for v in vc.SEQUENCE_VERDICTS]
    torch.cuda.synchronize()
    counts = np.bincount(want_t.indices, minlength=want_t.cols)
    for _, _, tp in transposes:      # and the transposes came out whole
        assert np.array_equal(np.diff(tp.cpu().numpy().astype(np.int64)), counts)


def test_sequence_on_a_side_stream():
    """cusparse.validate_csr under torch.cuda.stream(s): the handle follows torch's stream and
    validate waits on it."""
    from spmm_amd import cusparse
    ops = _sequence(torch.int32)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(0))
    with torch.cuda.stream(s):
        got = [cusparse.validate_csr(op.matrix()) for op in ops]
    torch.cuda.current_stream(0).wait_stream(s)
    assert got == list(vc.SEQUENCE_VERDICTS)
    assert [cusparse.validate_csr(op.matrix()) for op in ops] == list(vc.SEQUENCE_VERDICTS)   # and back on the current one
    M = ops[2].matrix()
    assert M.has_canonical_format is False and M._canonical is False
    M = ops[1].matrix()
    assert M.has_canonical_format is True and M._canonical is True


# ------------------------------------------------------------------ 3. status codes (host only, no launch)
def test_status_codes():
    from spmm_amd import _lib
    h = _handle()
    h.set_timing(True)
    try:
        op = _Operand(vc.by_id(vc.CANONICAL_ID), torch.int32)
        out = ctypes.c_int(7)
        res = ctypes.byref(out)

        def call(edit=None, handle=h.ptr, view=True, result=res):
            v = _lib.SpgCsr.from_buffer_copy(op.view)
            if edit is not None:
                edit(v)
            return h.lib.spg_validate_csr(handle, ctypes.byref(v) if view else None, result)

        def setter(name, value):
            return lambda v: setattr(v, name, value)
        assert call(handle=None) == NOT_INITIALIZED
        assert call(result=None) == INVALID_VALUE
        assert call(view=False) == INVALID_VALUE
        assert call(setter("rows", -1)) == INVALID_VALUE
        assert call(setter("indptr", None)) == INVALID_VALUE
        assert call(setter("indices", None)) == INVALID_VALUE          # nnz > 0
        assert call(setter("indptr_type", 16)) == INVALID_VALUE
        assert call(setter("value_type", 2)) == NOT_SUPPORTED
        assert out.value == 7                                          # no verdict was written
        assert h.get_timing()["validate"][1] == 0                      # and nothing was launched
        assert call() == 0 and out.value == 1
    finally:
        h.set_timing(False)


# ------------------------------------------------------------------ 4. timing
@pytest.mark.parametrize("ip", IPS, ids=["i32", "i64"])
def test_one_validate_is_one_launch(ip):
    h = _handle()
    full, empty, none = (_Operand(vc.by_id(cid), ip) for cid in ("r513-base", "r257-nnz0", "rows0"))
    h.set_timing(True)
    try:
        assert h.get_timing()["validate"][1] == 0
        assert _validate(full, h) == (0, 1)
        assert h.get_timing()["validate"][1] == 1
        assert _validate(empty, h) == (0, 1)                           # rows without entries: still one launch
        assert h.get_timing()["validate"][1] == 2
        assert _validate(none, h) == (0, 1)                            # no rows: none
        t = h.get_timing()
        assert t["validate"][1] == 2
        assert all(launches == 0 for name, (_, launches) in t.items() if name != "validate")
    finally:
        h.set_timing(False)
