"""The canonical-format check without a device: the reference of tests/validate_cases.py against
scipy and the C oracle, every generated case against the claim in its name, and the torch form
behind ``csr_matrix.has_canonical_format`` (CPU tensors) against the reference on the whole list.
tests/test_gpu_validate.py runs the same list through spg_validate_csr.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle
from tests import validate_cases as vc

torch = pytest.importorskip("torch")

CASES = vc.cases()
IDS = [c.id for c in CASES]


def test_the_list_covers_what_it_should():
    kinds = {c.kind for c in CASES}
    assert kinds == {"canonical", "one_violation", "row_boundary_drops", "single_entry_row", "one_bad_index",
                     "violation_and_bad_index", "bad_indptr"}
    assert {c.rows for c in CASES} == {0, *vc.ROW_COUNTS}
    assert max(c.rows for c in CASES) <= 600 and max(c.nnz for c in CASES) < 6000
    assert any(c.nnz == 0 and c.rows > vc.BLOCK for c in CASES)
    rows_hit = {(c.rows, c.at[0]) for c in CASES if c.kind == "one_violation"}
    assert rows_hit == {(r, f) for r in vc.ROW_COUNTS for f in vc.fault_rows(r)}
    assert vc.fault_rows(513) == [0, 255, 256, 512] and vc.fault_rows(1) == [0]
    assert tuple(vc.by_id(i).expect for i in vc.SEQUENCE) == vc.SEQUENCE_VERDICTS
    assert vc.by_id(vc.CANONICAL_ID).expect == 1 and vc.by_id(vc.VIOLATING_ID).expect == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_case_reads_outside_its_arrays(case):
    assert vc.reads_stay_inside(case)
    assert case.indptr.dtype == np.int64 and case.indices.dtype == np.int32
    assert np.abs(case.indptr).max() <= vc.INT32_MAX      # every row pointer fits both index types


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_gives_the_stated_verdict(case):
    assert vc.canon_status(case.indptr, case.indices, case.cols, case.nnz) == case.expect
    if case.repaired is not None:
        assert vc.canon_status(case.indptr, case.repaired, case.cols, case.nnz) == 1


@pytest.mark.parametrize("case", [c for c in CASES if c.expect != -1], ids=[c.id for c in CASES if c.expect != -1])
def test_reference_equals_scipy_and_the_oracle(case):
    """On well-formed, in-range input the verdict is scipy's has_canonical_format (on a matrix
    built for this question alone) and the C oracle's."""
    for indices in (case.indices,) + (() if case.repaired is None else (case.repaired,)):
        want = vc.canon_status(case.indptr, indices, case.cols, case.nnz) == 1
        S = sp.csr_matrix((np.ones(case.nnz), indices.copy(), case.indptr.copy()), shape=(case.rows, case.cols))
        assert bool(S.has_canonical_format) == want
        assert oracle.has_canonical_format((case.indptr, indices, np.ones(case.nnz), (case.rows, case.cols))) == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_has_the_property_its_name_claims(case):
    p, j, kind = case.indptr, case.indices, case.kind
    formed = vc.well_formed_rows(p, case.nnz)
    if kind != "bad_indptr":
        assert len(formed) == case.rows and int(p[0]) == 0 and int(p[-1]) == case.nnz
    if kind == "canonical":
        assert not vc.violating_pairs(p, j) and not vc.out_of_range(j, case.cols)
        if case.id.endswith("-base"):
            lens = np.diff(p)
            assert set(lens.tolist()) <= {0, 1, 2, vc.LONG}
            if case.rows >= 16:
                assert set(lens.tolist()) == {0, 1, 2, vc.LONG}
                assert not lens[:3].any() and not lens[-3:].any()      # a run of empty rows at each end
    elif kind == "one_violation":
        r, e = case.at
        n = int(p[r + 1] - p[r])
        assert e in (1, n - 1) and n == vc.LONG
        assert vc.violating_pairs(p, j) == [(r, e)] and not vc.out_of_range(j, case.cols)
        q = int(p[r]) + e
        want = {"dup": int(j[q - 1]), "down1": int(j[q - 1]) - 1, "to0": 0}[case.id.split("-")[2]]
        assert int(j[q]) == want and 0 <= want <= int(j[q - 1])
        assert np.flatnonzero(case.repaired != j).tolist() == [q]
        assert not vc.violating_pairs(p, case.repaired)
    elif kind == "row_boundary_drops":
        assert not vc.violating_pairs(p, j) and not vc.out_of_range(j, case.cols)
        full = [i for i in range(case.rows) if p[i + 1] > p[i]]
        pairs = list(zip(full, full[1:]))
        assert all(int(j[p[b]]) <= int(j[p[a + 1] - 1]) for a, b in pairs)      # every boundary drops or ties
        if case.rows > 1:
            assert any(b > a + 1 for a, b in pairs) and any(b == a + 1 for a, b in pairs)
            assert any(int(j[p[b]]) < int(j[p[a + 1] - 1]) for a, b in pairs)
        if case.rows > vc.BLOCK:
            assert (vc.BLOCK - 1, vc.BLOCK) in pairs
    elif kind == "single_entry_row":
        r, c = case.at
        assert p[r + 1] - p[r] == 1 and int(j[p[r]]) == c and c in (0, case.cols - 1)
        assert not vc.violating_pairs(p, j) and not vc.out_of_range(j, case.cols)
    elif kind == "one_bad_index":
        r, e = case.at
        q = int(p[r]) + e
        assert vc.out_of_range(j, case.cols) == [q] and q in (0, case.nnz - 1)
        assert int(j[q]) in (-1, case.cols, vc.INT32_MAX)
    elif kind == "violation_and_bad_index":
        assert len(vc.out_of_range(j, case.cols)) == 1 and (0, 1) in vc.violating_pairs(p, j)
    else:
        assert kind == "bad_indptr" and len(formed) < case.rows
        base = vc.build(case.rows, {0: vc.LONG, case.rows - 1: vc.LONG})
        assert np.array_equal(j, base[1])                                      # the indices are untouched
        assert np.count_nonzero(p != base[0]) == (2 if case.id == "r1-indptr-decreasing" else 1)


# ------------------------------------------------------------------ the torch form
@pytest.mark.parametrize("ipd", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_torch_form_equals_reference(case, ipd):
    from spmm_amd.sparse import _validate_torch, csr_matrix
    p = torch.from_numpy(case.indptr.copy()).to(ipd)
    for indices, want in ((case.indices, case.expect),) + (() if case.repaired is None else ((case.repaired, 1),)):
        j = torch.from_numpy(indices.copy())
        assert _validate_torch(p, j, case.nnz, case.cols) == want
        A = csr_matrix._from_parts(torch.ones(case.nnz, dtype=torch.float64), j, p, (case.rows, case.cols),
                                   canonical=None)
        assert A.has_canonical_format is (want == 1) and A._canonical is (want == 1)


def test_validate_csr_still_refuses_cpu_operands():
    """cusparse.validate_csr is the device entry point (tests/golden/shim_calls.json records its
    entry check); the property picks the torch form by itself."""
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    c = vc.by_id(vc.VIOLATING_ID)
    A = csr_matrix((np.ones(c.nnz), c.indices.copy(), c.indptr.copy()), shape=(c.rows, c.cols), device="cpu")
    assert A._canonical is None
    with pytest.raises(RuntimeError, match="validate_csr needs device-resident operands"):
        cusparse.validate_csr(A)
    assert A.has_canonical_format is False


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    out = ctypes.c_int(7)
    assert lib.spg_validate_csr(None, ctypes.byref(_lib.SpgCsr()), ctypes.byref(out)) == 1   # NOT_INITIALIZED
    assert out.value == 7
