"""Every entry point outside the product path on a matrix of more than 2**31 stored entries, through
the C ABI with SPG_INDEX_64I operands and fp32 values: spg_validate_csr, spg_spmv, spg_spmm,
spg_csr2csc, spg_csrgeam_nnz / spg_csrgeam, spg_canonicalize_nnz / spg_canonicalize, spg_csr2dense,
spg_dense2csr_nnz / spg_dense2csr, spg_cols16_split / spg_cols16_join, and the Python shim's retry
after SPG_STATUS_OVERFLOW.

The operand (tests/large_offsets.py) is built on the device from a closed form and never passes
through the host: 8589935 pad rows of 250 small integers over 256 columns -- 2147483750 entries, row
8589934 straddling offset 2**31 -- and a tail of a few hundred standard_normal rows whose every entry
sits above 2**31.  The pad part of each result is compared with the closed form on the device, in
slices of at most 2**26 entries, exactly (integers, or bits moved); the tail part bit for bit with
scipy or the oracle.  tests/test_large_offsets_cpu.py holds the same models to scipy on whole
matrices at small sizes.  Outputs are tests.guarded buffers poisoned 0xFF, and the operands are
compared with their closed form again after the calls.  An assertion names the first differing
slice, row and offset.

Each test prints the device bytes it needs (its arrays plus the library's answer to the size query)
and skips only when torch.cuda.mem_get_info() reports less.  Not covered: the product kernels with
nnz(A) or nnz(B) >= 2**31, anything past 2**32, value types other than fp32 at this size.
"""
import ctypes
import types

import numpy as np
import pytest

from oracle import oracle
from tests import large_offsets as lo
from tests import special_values as sv
from tests.guarded import guarded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32, I64 = 32, 64
OVERFLOW, INVALID_VALUE = 100, 3
INT32_MAX = 2 ** 31 - 1
F32 = 0                                    # SPG_R_32F
COEFS = [(1.0, 0.0), (2.0, 0.5)]           # exactly representable; 0.5 * y0 is exact (y0 even)
_OPERAND = [0]                             # bytes of the shared operand once the fixture has built it


def _handle():
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    return h


def _desc(M, indptr_type=I64, rows=None, cols=None, nnz=None):
    from spmm_amd import _lib
    return _lib.SpgCsr(M.rows if rows is None else rows, M.cols if cols is None else cols,
                       M.nnz if nnz is None else nnz, M.indptr.data_ptr(), M.indices.data_ptr(),
                       M.values.data_ptr() if M.values is not None else 0, indptr_type, F32)


def _f(v):
    return ctypes.c_float(float(v))


def _require(what, arrays, workspace=0, planned=None):
    """Print the test's need and skip only when the device reports less free memory.  planned:
    large_offsets.planned_bytes' figure for this test, which the CPU suite holds under the cap."""
    need = int(arrays) + int(workspace)
    assert need + _OPERAND[0] < lo.CAP_BYTES, f"{what}: {(need + _OPERAND[0]) / lo.GiB:.1f} GiB is over the cap"
    assert planned is None or need <= planned, f"{what}: needs {need} bytes, planned_bytes says {planned}"
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    print(f"[memory] {what}: needs {need / lo.GiB:.1f} GiB beyond the shared operand "
          f"(arrays {arrays / lo.GiB:.1f} + workspace {workspace / lo.GiB:.1f}), {free / lo.GiB:.1f} GiB free")
    if free < need:
        pytest.skip(f"{what}: needs {need / lo.GiB:.1f} GiB, {free / lo.GiB:.1f} GiB free")


def _chunks(n, step):
    for a in range(0, n, step):
        yield a, min(a + step, n)


def _same_bytes(got, want, what, g):
    """Two equally long flat tensors of 4-byte elements, byte for byte, in slices."""
    assert got.numel() == want.numel(), f"{what}: {got.numel()} entries, expected {want.numel()}"
    for n, (a, b) in enumerate(_chunks(got.numel(), g.slice_entries)):
        d = lo.first_difference(got[a:b].view(torch.int32), want[a:b].view(torch.int32))
        assert d is None, f"{what}: slice {n}, first difference at offset {a + d[0]}"


def _same_host(got, want, what):
    got, want = got.cpu().numpy(), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32 if got.itemsize == 4 else np.uint64) !=
                         want.reshape(-1).view(np.uint32 if want.itemsize == 4 else np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:4].tolist()}"


def _operand_intact(b):
    d = b.g.first_pad_difference(b.A)
    assert d is None, f"the operand changed: {d}"
    p, j, x = b.g.tail_of(b.A)
    assert np.array_equal(p, b.g.tail.indptr) and np.array_equal(j, b.g.tail.indices)
    assert np.array_equal(x.view(np.uint32), b.g.tail.data.view(np.uint32)), "the operand's tail values changed"


@pytest.fixture(scope="module")
def big():
    g = lo.Geometry(**lo.FULL)
    _require("the shared operand", g.csr_bytes() + lo.planned_bytes(g)["validate"])
    A = g.build(DEV)
    _OPERAND[0] = A.nbytes()
    b = types.SimpleNamespace(g=g, A=A, full=g.nnz > INT32_MAX)
    _operand_intact(b)
    yield b
    del b.A, A
    _OPERAND[0] = 0
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ validate

def _validate(M):
    h = _handle()
    out = ctypes.c_int(7)
    va = _desc(M)
    st = h.lib.spg_validate_csr(h.ptr, ctypes.byref(va), ctypes.byref(out))
    assert st == 0, st
    return out.value


def test_validate(big):
    g, A = big.g, big.A
    assert _validate(A) == 1
    lens = np.diff(g.tail.indptr)
    t = int(np.flatnonzero(lens >= 2)[-1])                         # the last tail row with two entries
    e = g.pad_nnz + int(g.tail.indptr[t])
    assert e >= g.pad_nnz and (not big.full or e > 1 << 31)
    pair = A.indices[e:e + 2].clone()
    A.indices[e:e + 2] = pair.flip(0)
    try:
        assert _validate(A) == 0, "two adjacent indices swapped in the last tail row"
    finally:
        A.indices[e:e + 2] = pair
    assert _validate(A) == 1
    one = A.indices[e + 1].clone()
    A.indices[e + 1] = g.W
    try:
        assert _validate(A) == -1, f"index {g.W} at offset {e + 1}"
    finally:
        A.indices[e + 1] = one
    s = g.marked_rows()[1]                                           # and inside the straddling row
    e = (s + 1) * g.L - 1
    one = A.indices[e].clone()
    A.indices[e] = A.indices[e - 1]
    try:
        assert _validate(A) == 0, f"a duplicate at offset {e} (row {s})"
    finally:
        A.indices[e] = one
    assert _validate(A) == 1
    _operand_intact(big)


# ------------------------------------------------------------------------------------ SpMV, SpMM

def _check_product_pad(g, view_of, X, alpha, beta, what):
    """view_of(a, b): the result's rows [a, b) as (b - a,) or (b - a, n)."""
    for n, (a, b) in enumerate(g.row_slices()):
        want = g.expect_product_pad(a, b, X, alpha, beta)
        d = lo.first_difference(view_of(a, b), want)
        if d is not None:
            r = a + d[0]
            got = view_of(a, b)[d]
            raise AssertionError(f"{what}: slice {n}, row {r} (offsets {r * g.L}..{(r + 1) * g.L - 1})"
                                 f"{', column %d' % d[1] if len(d) > 1 else ''}: got {float(got)}, expected {float(want[d])}")


def test_spmv(big):
    g, A = big.g, big.A
    _require("spg_spmv", 2 * (g.rows * 4 + 3 * 4096) + lo.planned_bytes(g)["validate"], planned=lo.planned_bytes(g)["spmv"])
    h = _handle()
    x = lo.x_vector(g.W)
    gx = guarded(g.W, np.float32, 0xFF, DEV, "x")
    gx.t.copy_(torch.from_numpy(np.array(x)))
    x_bytes = gx.bytes().clone()
    s_tail = oracle.spmv(g.tail, x)
    va = _desc(A)
    for alpha, beta in COEFS:
        what = f"spg_spmv alpha={alpha} beta={beta}"
        gy = guarded(g.rows, np.float32, 0xFF, DEV, "y")            # (0xFF: NaN where nothing is stored)
        if beta != 0:
            for a, b in _chunks(g.rows, g.slice_entries):
                gy.t[a:b] = g.y0_rows(a, b, DEV)
        al, be = _f(alpha), _f(beta)
        st = h.lib.spg_spmv(h.ptr, ctypes.byref(va), ctypes.c_void_p(gx.data_ptr()), ctypes.byref(al), ctypes.byref(be),
                            ctypes.c_void_p(gy.data_ptr()))
        assert st == 0, st
        torch.cuda.synchronize()
        wrong = []                      # the pad and the tail are both looked at before anything is raised
        try:
            _check_product_pad(g, lambda a, b: gy.t[a:b], gx.t, alpha, beta, what)
        except AssertionError as e:
            wrong.append("pad: " + str(e))
        want = sv.axpby(alpha, s_tail, beta, g.tail_y0())
        got = gy.t[g.pad_rows:].cpu().numpy()
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        if bad.size:
            wrong.append(f"tail: {what}: {bad.size} of {g.tail_rows} tail rows differ, first tail rows {bad[:6].tolist()} "
                         f"(rows {(bad[:6] + g.pad_rows).tolist()}), offsets from {g.pad_nnz + int(g.tail.indptr[bad[0]])}")
        assert not wrong, "; ".join(wrong)
        gy.check(what + " y")
        gx.check(what + " x")
        assert torch.equal(gx.bytes(), x_bytes), f"{what}: x changed"
        del gy
    _operand_intact(big)


# (order, n, leading dimension beyond the minor extent): k_spmm_row_packed with 16-byte accesses,
# k_spmm_row with scalar ones (33 lanes per row, an odd leading dimension), k_spmm_col
SPMM_LAYOUTS = [("row", 8, 0), ("row", 33, 0), ("col", 3, 3)]


@pytest.mark.parametrize("order,n,pad", SPMM_LAYOUTS, ids=["row_packed", "row", "col"])
def test_spmm(big, order, n, pad):
    from spmm_amd import _lib
    g, A = big.g, big.A
    row = order == "row"
    _require(f"spg_spmm {order} n={n}", 2 * (g.rows + pad) * n * 4 + lo.planned_bytes(g)["validate"],
             planned=lo.planned_bytes(g)["spmm"])
    h = _handle()
    B = lo.b_matrix(g.W, n)
    S_tail = oracle.spmm(g.tail, B)
    ldb, ldc = (n, n) if row else (g.W + pad, g.rows + pad)
    gb = guarded((g.W, ldb) if row else (n, ldb), np.float32, 0xFF, DEV, "B")
    (gb.t if row else gb.t[:, :g.W]).copy_(torch.from_numpy(np.array(B if row else B.T)))
    b_bytes = gb.bytes().clone()
    Bd = torch.from_numpy(np.array(B)).to(DEV)
    code = _lib.SPG_ORDER_ROW if row else _lib.SPG_ORDER_COL
    vb = _lib.SpgDense(g.W, n, ldb, gb.data_ptr(), code, F32)
    va = _desc(A)
    for alpha, beta in COEFS:
        what = f"spg_spmm {order}-major n={n} alpha={alpha} beta={beta}"
        gc = guarded((g.rows, ldc) if row else (n, ldc), np.float32, 0xFF, DEV, "C")
        if beta != 0:
            for a, b in _chunks(g.rows, g.slice_entries // 64):
                if row:
                    gc.t[a:b] = g.y0_rows(a, b, DEV, n)
                else:
                    gc.t[:, a:b] = g.y0_rows(a, b, DEV)[None, :]
        vc = _lib.SpgDense(g.rows, n, ldc, gc.data_ptr(), code, F32)
        al, be = _f(alpha), _f(beta)
        st = h.lib.spg_spmm(h.ptr, ctypes.byref(va), ctypes.byref(vb), ctypes.byref(al), ctypes.byref(be), ctypes.byref(vc))
        assert st == 0, st
        torch.cuda.synchronize()
        _check_product_pad(g, (lambda a, b: gc.t[a:b]) if row else (lambda a, b: gc.t[:, a:b].t()), Bd, alpha, beta, what)
        want = sv.axpby(alpha, S_tail, beta, g.tail_y0(n))
        got = (gc.t[g.pad_rows:] if row else gc.t[:, g.pad_rows:g.rows].t()).cpu().numpy()
        bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
        assert bad.size == 0, f"{what}: {len(bad)} tail elements differ, first (tail row, column) {bad[:6].tolist()}"
        if not row and pad:
            assert bool((gc.t[:, g.rows:].contiguous().view(torch.uint8) == 0xFF).all()), f"{what}: padding written"
        gc.check(what + " C")
        gb.check(what + " B")
        assert torch.equal(gb.bytes(), b_bytes), f"{what}: B changed"
        del gc
    _operand_intact(big)


# ------------------------------------------------------------------------------------ transpose

def test_csr2csc(big):
    from spmm_amd import _lib
    g, A = big.g, big.A
    h = _handle()
    va = _desc(A)
    tp = guarded(g.W + 1, np.int64, 0xFF, DEV, "AT.indptr")
    vt = _lib.SpgCsr(g.W, g.rows, g.nnz, tp.data_ptr(), 0, 0, I64, F32)
    need = ctypes.c_size_t(0)
    assert h.lib.spg_csr2csc(h.ptr, ctypes.byref(va), ctypes.byref(vt), ctypes.byref(need), None) == 0
    _require("spg_csr2csc", g.nnz * 8 + 3 * 8192 + lo.planned_bytes(g)["validate"], need.value,
             planned=lo.planned_bytes(g)["csr2csc"])
    tj = guarded(g.nnz, np.int32, 0xFF, DEV, "AT.indices")
    tx = guarded(g.nnz, np.float32, 0xFF, DEV, "AT.values")
    ws = guarded(need.value, np.uint8, 0xFF, DEV, "workspace")
    vt.indices, vt.values = tj.data_ptr(), tx.data_ptr()
    st = h.lib.spg_csr2csc(h.ptr, ctypes.byref(va), ctypes.byref(vt), ctypes.byref(need), ctypes.c_void_p(ws.data_ptr()))
    assert st == 0, st
    torch.cuda.synchronize()
    p = g.csc_indptr()
    got_p = tp.t.cpu().numpy()
    bad = np.flatnonzero(got_p != p)
    assert bad.size == 0, f"AT.indptr differs first at row {bad[:4].tolist()}: {got_p[bad[:4]].tolist()} vs {p[bad[:4]].tolist()}"
    cnt = g.csc_pad_counts()
    tail_p, tail_j, tail_x = g.csc_tail()
    parts_j, parts_x = [], []
    for j in range(g.W):
        a, m = int(p[j]), int(p[j]) + int(cnt[j])
        rows, vals = g.csc_pad_row(j, DEV)
        d = lo.first_difference(tj.t[a:m], rows)
        assert d is None, f"AT row {j} (slice {j}): index at offset {a + d[0]} is {int(tj.t[a + d[0]])}, expected {int(rows[d])}"
        d = lo.first_bit_difference(tx.t[a:m], vals)
        assert d is None, f"AT row {j} (slice {j}): value at offset {a + d[0]} is {float(tx.t[a + d[0]])}, expected {float(vals[d])}"
        parts_j.append(tj.t[m:int(p[j + 1])])
        parts_x.append(tx.t[m:int(p[j + 1])])
        assert int(p[j + 1]) - m == tail_p[j + 1] - tail_p[j]
    _same_host(torch.cat(parts_j), tail_j, "AT tail parts, indices (the tail's tocsc(), rows shifted)")
    _same_host(torch.cat(parts_x), tail_x, "AT tail parts, values")
    for b in (tp, tj, tx, ws):
        b.check("spg_csr2csc " + b.name)
    del tj, tx, ws
    _operand_intact(big)


# ------------------------------------------------------------------------------------ addition

class _Geam:
    """One addition through the ABI: the size query, the structure pass into a guarded row pointer of
    either width, the value pass into guarded arrays."""

    def __init__(self, A, B):
        self.h = _handle()
        self.rows = A.rows
        self.va, self.vb = _desc(A), _desc(B)
        self.need = ctypes.c_size_t(0)
        self.nnz = ctypes.c_int64(-1)
        st = self.h.lib.spg_csrgeam_nnz(self.h.ptr, ctypes.byref(self.va), ctypes.byref(self.vb), None, I64,
                                        ctypes.byref(self.nnz), ctypes.byref(self.need), None)
        assert st == 0 and self.need.value > 0, st
        self.ws = None

    def structure(self, width):
        if self.ws is None:
            self.ws = guarded(self.need.value, np.uint8, 0xFF, DEV, "workspace")
        self.cp = guarded(self.rows + 1, np.int32 if width == I32 else np.int64, 0xFF, DEV, "C.indptr")
        self.nnz = ctypes.c_int64(-1)
        have = ctypes.c_size_t(self.need.value)
        st = self.h.lib.spg_csrgeam_nnz(self.h.ptr, ctypes.byref(self.va), ctypes.byref(self.vb),
                                        ctypes.c_void_p(self.cp.data_ptr()), width, ctypes.byref(self.nnz),
                                        ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))
        self.cp.check("spg_csrgeam_nnz C.indptr")
        self.ws.check("spg_csrgeam_nnz workspace")
        return st

    def values(self, alpha, beta, cj=None, cx=None):
        from spmm_amd import _lib
        n = int(self.nnz.value)
        self.cj = guarded(n, np.int32, 0xFF, DEV, "C.indices") if cj is None else cj
        self.cx = guarded(n, np.float32, 0xFF, DEV, "C.values") if cx is None else cx
        vc = _lib.SpgCsr(self.rows, self.va.cols, n, self.cp.data_ptr(), self.cj.data_ptr(), self.cx.data_ptr(), I64, F32)
        al, be = _f(alpha), _f(beta)
        st = self.h.lib.spg_csrgeam(self.h.ptr, ctypes.byref(al), ctypes.byref(self.va), ctypes.byref(be),
                                    ctypes.byref(self.vb), ctypes.byref(vc), ctypes.c_size_t(self.need.value),
                                    ctypes.c_void_p(self.ws.data_ptr()))
        assert st == 0, st
        torch.cuda.synchronize()
        for b in (self.cp, self.cj, self.cx, self.ws):
            b.check("spg_csrgeam " + b.name)


def _check_sum(g, A, cp, cj, cx, touched, Cs, extra, what):
    """C = A (+-) small against the model: the row pointer everywhere, the untouched pad rows slice
    against slice with A's entries, the touched rows against scipy."""
    tt = torch.from_numpy(touched).to(DEV)
    ex = torch.from_numpy(extra).to(DEV)
    for n, (a, b) in enumerate(_chunks(g.rows + 1, g.slice_entries)):
        i = torch.arange(a, b, dtype=torch.int64, device=DEV)
        want = A.indptr[a:b] + ex[torch.bucketize(i, tt)]            # the gain of the touched rows before row i
        d = lo.first_difference(cp[a:b], want)
        assert d is None, f"{what}: C.indptr slice {n}, row {a + d[0]}: {int(cp[a + d[0]])}, expected {int(want[d])}"
    marked = [int(r) for r in touched if r < g.pad_rows]
    prev = 0
    for n, r in enumerate(marked + [g.pad_rows]):                    # the untouched runs of pad rows
        lo_, hi_ = prev * g.L, r * g.L
        for k, (a, b) in enumerate(_chunks(hi_ - lo_, g.slice_entries)):
            a, b = a + lo_, b + lo_
            sh = int(extra[n])
            for got, src, name in ((cj, A.indices, "indices"), (cx, A.values, "values")):
                d = lo.first_difference(got[a + sh:b + sh].view(torch.int32), src[a:b].view(torch.int32))
                assert d is None, (f"{what}: {name} of untouched rows {prev}..{r - 1}, slice {k}: C offset {a + sh + d[0]} "
                                   f"is not A's offset {a + d[0]} (row {(a + d[0]) // g.L})")
        prev = r + 1
    sp_ = Cs.indptr.astype(np.int64)
    for n, r in enumerate(marked):                                   # the marked rows, one by one
        a = r * g.L + int(extra[n])
        m = int(sp_[n + 1] - sp_[n])
        _same_host(cj[a:a + m], Cs.indices[sp_[n]:sp_[n + 1]], f"{what}: indices of marked row {r} at offset {a}")
        _same_host(cx[a:a + m], Cs.data[sp_[n]:sp_[n + 1]], f"{what}: values of marked row {r} at offset {a}")
    a = g.pad_nnz + int(extra[len(marked)])                          # the tail, in one piece
    _same_host(cj[a:], Cs.indices[sp_[len(marked)]:], f"{what}: indices of the tail from offset {a}")
    _same_host(cx[a:], Cs.data[sp_[len(marked)]:], f"{what}: values of the tail from offset {a}")


def test_csrgeam(big):
    g, A = big.g, big.A
    touched, Bs = g.small_operand()
    B = g.spread_small(touched, Bs, DEV)
    b_copy = [t.clone() for t in (B.indptr, B.indices, B.values)]
    Cs, extra = g.expect_sum(touched, Bs, 1, 1)
    nnzc = g.nnz + int(extra[-1])
    big_small, small_big = _Geam(A, B), _Geam(B, A)
    _require("spg_csrgeam", 2 * (nnzc * 8 + (g.rows + 1) * 8) + B.nbytes() * 2 + lo.planned_bytes(g)["validate"],
             big_small.need.value + small_big.need.value, planned=lo.planned_bytes(g)["csrgeam"])
    # int32 row pointer: OVERFLOW exactly when nnz(C) does not fit, *nnzC set all the same
    st = big_small.structure(I32)
    assert big_small.nnz.value == nnzc, f"*nnzC {big_small.nnz.value}, expected {nnzc}"
    assert st == (OVERFLOW if nnzc > INT32_MAX else 0), st
    assert big_small.structure(I64) == 0 and big_small.nnz.value == nnzc
    big_small.values(1, 1)
    c1 = big_small
    _check_sum(g, A, c1.cp.t, c1.cj.t, c1.cx.t, touched, Cs, extra, "big + small")
    # the roles swapped: the in-place scan over B's marks runs past 2**31; a + b == b + a, byte for byte
    assert small_big.structure(I64) == 0 and small_big.nnz.value == nnzc
    small_big.values(1, 1)
    assert torch.equal(small_big.cp.t, c1.cp.t), "small + big: C.indptr differs from big + small"
    _same_bytes(small_big.cj.t, c1.cj.t, "small + big vs big + small, indices", g)
    _same_bytes(small_big.cx.t, c1.cx.t, "small + big vs big + small, values", g)
    # the subtraction, into the second result's buffers
    Cm, extra_m = g.expect_sum(touched, Bs, 1, -1)
    assert np.array_equal(extra_m, extra)
    cj, cx = small_big.cj, small_big.cx
    cj.refill()
    cx.refill()
    big_small.values(1, -1, cj, cx)
    _check_sum(g, A, big_small.cp.t, cj.t, cx.t, touched, Cm, extra_m, "big - small")
    for t, c in zip((B.indptr, B.indices, B.values), b_copy):
        assert torch.equal(t, c), "the small operand changed"
    del big_small, small_big, c1, cj, cx
    _operand_intact(big)


# ------------------------------------------------------------------------------------ canonicalisation

class _Canon:
    """One canonicalisation through the ABI, step by step, into guarded outputs."""

    def __init__(self, M, ops, coo_rows=None, indptr_type=I64):
        self.h = _handle()
        self.M, self.ops = M, ops
        self.va = _desc(M, indptr_type)
        self.rows_p = None if coo_rows is None else ctypes.c_void_p(coo_rows.data_ptr())
        self.need = ctypes.c_size_t(0)
        self.nnz = ctypes.c_int64(-1)
        self.ws = None

    def query(self):
        return self.h.lib.spg_canonicalize_nnz(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops, None, I64,
                                               ctypes.byref(self.nnz), ctypes.byref(self.need), None)

    def structure(self, width):
        if self.ws is None:
            self.ws = guarded(self.need.value, np.uint8, 0xFF, DEV, "workspace")
        self.cp = guarded(self.M.rows + 1, np.int32 if width == I32 else np.int64, 0xFF, DEV, "C.indptr")
        self.nnz = ctypes.c_int64(-1)
        have = ctypes.c_size_t(self.need.value)
        st = self.h.lib.spg_canonicalize_nnz(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops,
                                             ctypes.c_void_p(self.cp.data_ptr()), width, ctypes.byref(self.nnz),
                                             ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))
        self.cp.check("spg_canonicalize_nnz C.indptr")
        self.ws.check("spg_canonicalize_nnz workspace")
        return st

    def values(self):
        from spmm_amd import _lib
        n = int(self.nnz.value)
        self.cj = guarded(n, np.int32, 0xFF, DEV, "C.indices")
        self.cx = guarded(n, np.float32, 0xFF, DEV, "C.values")
        vc = _lib.SpgCsr(self.M.rows, self.M.cols, n, self.cp.data_ptr(), self.cj.data_ptr(), self.cx.data_ptr(), I64, F32)
        st = self.h.lib.spg_canonicalize(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops, ctypes.byref(vc),
                                         ctypes.c_size_t(self.need.value), ctypes.c_void_p(self.ws.data_ptr()))
        assert st == 0, st
        torch.cuda.synchronize()
        for b in (self.cp, self.cj, self.cx, self.ws):
            b.check("spg_canonicalize " + b.name)
        return lo.Csr(self.M.rows, self.M.cols, self.cp.t, self.cj.t, self.cx.t)


def _check_tail(g, C, base, want, what):
    """C's rows behind the pad against (indptr, indices, values) on the host; base: C's entries
    before them."""
    p = C.indptr[g.pad_rows:].cpu().numpy() - base
    assert np.array_equal(p, np.asarray(want[0], dtype=np.int64)), f"{what}: the tail's row pointer"
    _same_host(C.indices[base:], np.asarray(want[1], dtype=np.int32), f"{what}: the tail's indices from offset {base}")
    _same_host(C.values[base:], np.asarray(want[2], dtype=np.float32), f"{what}: the tail's values from offset {base}")


def test_canonicalize_sort_sum(big):
    from tests import canon_cases as cc
    g = big.g
    ops = cc.SORT | cc.SUM
    planned = lo.planned_bytes(g)
    _require("spg_canonicalize SORT|SUM (before the size query)", 2 * g.csr_bytes() + planned["validate"])
    M, tail_want = g.build_canon_input(DEV)
    m_copy_p = M.indptr.clone()
    nnzc = g.pad_nnz + int(tail_want[1].size)
    # an SPG_INDEX_32I input descriptor of this nnz: INVALID_VALUE and nothing launched
    if M.nnz > INT32_MAX:
        h = _handle()
        h.set_timing(True)
        c32 = _Canon(M, ops, indptr_type=I32)
        assert c32.query() == INVALID_VALUE
        assert all(n == 0 for _, n in h.get_timing().values()), h.get_timing()
        h.set_timing(False)
    c = _Canon(M, ops)
    assert c.query() == 0 and c.need.value > 0
    _require("spg_canonicalize SORT|SUM", M.nbytes() + nnzc * 8 + (g.rows + 1) * 12 + planned["validate"], c.need.value,
             planned=planned["canonicalize_sum"])
    st = c.structure(I32)
    assert c.nnz.value == nnzc, f"*nnzC {c.nnz.value}, expected {nnzc}"
    assert st == (OVERFLOW if nnzc > INT32_MAX else 0), st
    assert c.structure(I64) == 0 and c.nnz.value == nnzc
    C = c.values()
    d = g.first_pad_difference(C)
    assert d is None, f"SORT|SUM of the reversed variant is not the forward pad: {d}"
    _check_tail(g, C, g.pad_nnz, tail_want, "SORT|SUM")
    assert torch.equal(M.indptr, m_copy_p), "the input's row pointer changed"
    del c, C, M


def test_canonicalize_drop_zeros(big):
    from tests import canon_cases as cc
    g = big.g
    planned = lo.planned_bytes(g)
    kept = g.dropped_pad_nnz()
    nnzc = kept + int(g.tail.nnz)
    _require("spg_canonicalize DROP_ZEROS (before the size query)", g.csr_bytes() + planned["validate"])
    Z = g.build(DEV, zeros=True)
    c = _Canon(Z, cc.DROP)
    assert c.query() == 0 and c.need.value > 0
    _require("spg_canonicalize DROP_ZEROS", Z.nbytes() + nnzc * 8 + (g.rows + 1) * 8 + planned["validate"], c.need.value,
             planned=planned["canonicalize_drop"])
    assert c.structure(I64) == 0
    assert c.nnz.value == nnzc, f"*nnzC {c.nnz.value}, expected {nnzc}"
    C = c.values()
    off = 0
    for n, (a, b) in enumerate(g.row_slices()):
        counts, cols, vals = g.dropped_pad(a, b, DEV)
        want_p = off + torch.cumsum(counts, 0) - counts
        d = lo.first_difference(C.indptr[a:b], want_p)
        assert d is None, f"DROP_ZEROS: slice {n}: C.indptr of row {a + d[0]} is {int(C.indptr[a + d[0]])}, expected {int(want_p[d])}"
        m = int(cols.numel())
        d = lo.first_difference(C.indices[off:off + m], cols)
        assert d is None, f"DROP_ZEROS: slice {n} (rows {a}..{b - 1}): index at C offset {off + d[0]}"
        d = lo.first_bit_difference(C.values[off:off + m], vals)
        assert d is None, f"DROP_ZEROS: slice {n} (rows {a}..{b - 1}): value at C offset {off + d[0]}"
        off += m
    assert off == kept
    _check_tail(g, C, kept, (g.tail.indptr, g.tail.indices, g.tail.data), "DROP_ZEROS")
    d = g.first_pad_difference(Z, zeros=True)
    assert d is None, f"the input changed: {d}"
    del c, C, Z


def test_canonicalize_coo(big):
    g, A = big.g, big.A
    planned = lo.planned_bytes(g)
    _require("spg_canonicalize COO (before the size query)", 12 * g.nnz + planned["validate"])
    rows, cols, vals = g.build_coo(DEV)
    M = lo.Csr(g.rows, g.W, A.indptr, cols, vals)                  # (the row pointer of a COO input is ignored)
    c = _Canon(M, 0, coo_rows=rows)
    c.va.indptr = 0
    assert c.query() == 0 and c.need.value > 0
    _require("spg_canonicalize COO", 12 * g.nnz + g.csr_bytes() + planned["validate"], c.need.value,
             planned=planned["canonicalize_coo"])
    assert c.structure(I64) == 0 and c.nnz.value == g.nnz
    C = c.values()
    assert torch.equal(C.indptr, A.indptr), "COO -> CSR: the row pointer is not the forward matrix's"
    d = g.first_pad_difference(C)
    assert d is None, f"COO -> CSR (odd rows first, then even rows): {d}"
    _check_tail(g, C, g.pad_nnz, (g.tail.indptr, g.tail.indices, g.tail.data), "COO -> CSR")
    del c, C, M, rows, cols, vals
    _operand_intact(big)


# ------------------------------------------------------------------------------------ dense

def _todense(A, g, order, pad):
    from spmm_amd import _lib
    h = _handle()
    row = order == "row"
    ld = g.W if row else g.rows + pad
    D = guarded((g.rows, ld) if row else (g.W, ld), np.float32, 0xFF, DEV, f"D ({order}-major)")
    vd = _lib.SpgDense(g.rows, g.W, ld, D.data_ptr(), _lib.SPG_ORDER_ROW if row else _lib.SPG_ORDER_COL, F32)
    va = _desc(A)
    st = h.lib.spg_csr2dense(h.ptr, ctypes.byref(va), ctypes.byref(vd))
    assert st == 0, st
    torch.cuda.synchronize()
    D.check("spg_csr2dense " + D.name)
    return D, vd


def _check_dense(g, D, order, zeros, what):
    row = order == "row"
    for n, (a, b) in enumerate(g.row_slices()):
        want = g.pad_dense(a, b, DEV, zeros)
        got = D.t[a:b] if row else D.t[:, a:b].t()
        d = lo.first_bit_difference(got, want)
        assert d is None, (f"{what}: slice {n}, row {a + d[0]} (offsets from {(a + d[0]) * g.L}), column {d[1]}: "
                           f"{float(got[d])}, expected {float(want[d])}")
    got = D.t[g.pad_rows:] if row else D.t[:, g.pad_rows:g.rows].t()
    _same_host(got.contiguous(), g.tail.toarray(), f"{what}: the tail against toarray()")
    if not row:
        assert bool((D.t[:, g.rows:].contiguous().view(torch.uint8) == 0xFF).all()), f"{what}: padding written"


class _FromDense:
    def __init__(self, vd, rows, cols):
        self.h, self.vd, self.rows, self.cols = _handle(), vd, rows, cols
        self.need, self.nnz = ctypes.c_size_t(0), ctypes.c_int64(-1)
        st = self.h.lib.spg_dense2csr_nnz(self.h.ptr, ctypes.byref(vd), None, I64, ctypes.byref(self.nnz),
                                          ctypes.byref(self.need), None)
        assert st == 0 and self.need.value > 0, st
        self.ws = None

    def structure(self, width):
        if self.ws is None:
            self.ws = guarded(self.need.value, np.uint8, 0xFF, DEV, "workspace")
        self.cp = guarded(self.rows + 1, np.int32 if width == I32 else np.int64, 0xFF, DEV, "C.indptr")
        self.nnz = ctypes.c_int64(-1)
        have = ctypes.c_size_t(self.need.value)
        st = self.h.lib.spg_dense2csr_nnz(self.h.ptr, ctypes.byref(self.vd), ctypes.c_void_p(self.cp.data_ptr()), width,
                                          ctypes.byref(self.nnz), ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))
        self.cp.check("spg_dense2csr_nnz C.indptr")
        self.ws.check("spg_dense2csr_nnz workspace")
        return st

    def values(self):
        from spmm_amd import _lib
        n = int(self.nnz.value)
        self.cj = guarded(n, np.int32, 0xFF, DEV, "C.indices")
        self.cx = guarded(n, np.float32, 0xFF, DEV, "C.values")
        vc = _lib.SpgCsr(self.rows, self.cols, n, self.cp.data_ptr(), self.cj.data_ptr(), self.cx.data_ptr(), I64, F32)
        st = self.h.lib.spg_dense2csr(self.h.ptr, ctypes.byref(self.vd), ctypes.byref(vc),
                                      ctypes.c_size_t(self.need.value), ctypes.c_void_p(self.ws.data_ptr()))
        assert st == 0, st
        torch.cuda.synchronize()
        for b in (self.cp, self.cj, self.cx, self.ws):
            b.check("spg_dense2csr " + b.name)
        return lo.Csr(self.rows, self.cols, self.cp.t, self.cj.t, self.cx.t)


def test_csr2dense_and_back(big):
    g, A = big.g, big.A
    dense = g.rows * g.W * 4
    _require("spg_csr2dense / spg_dense2csr (before the size query)",
             2 * dense + 12 * g.W + g.csr_bytes() + lo.planned_bytes(g)["validate"])
    Dr, vdr = _todense(A, g, "row", 0)
    _check_dense(g, Dr, "row", False, "spg_csr2dense row-major")
    Dc, vdc = _todense(A, g, "col", 3)
    _check_dense(g, Dc, "col", False, "spg_csr2dense column-major ld = rows + 3")
    # back from the row-major D: int32 overflows with *nnzC set, int64 gives A's three arrays
    f = _FromDense(vdr, g.rows, g.W)
    _require("spg_csr2dense / spg_dense2csr", 2 * dense + 12 * g.W + g.csr_bytes() + lo.planned_bytes(g)["validate"],
             f.need.value, planned=lo.planned_bytes(g)["dense"])
    st = f.structure(I32)
    assert f.nnz.value == g.nnz, f"*nnzC {f.nnz.value}, expected {g.nnz}"
    assert st == (OVERFLOW if g.nnz > INT32_MAX else 0), st
    assert f.structure(I64) == 0 and f.nnz.value == g.nnz
    C = f.values()
    for n, (a, b) in enumerate(_chunks(g.rows + 1, g.slice_entries)):
        d = lo.first_difference(C.indptr[a:b], A.indptr[a:b])
        assert d is None, f"dense -> CSR: C.indptr slice {n}, row {a + d[0]}"
    _same_bytes(C.indices, A.indices, "dense -> CSR: indices against A's", g)
    _same_bytes(C.values, A.values, "dense -> CSR: values against A's", g)
    del f, C, Dr
    # the zeros variant written into the column-major D: +0.0 and -0.0 are dropped
    for a, b in g.row_slices():
        Dc.t[:, a:b] = g.pad_dense(a, b, DEV, zeros=True).t()
    _check_dense(g, Dc, "col", True, "the zeros variant in D")
    f = _FromDense(vdc, g.rows, g.W)
    kept = g.dropped_pad_nnz()
    assert f.structure(I64) == 0
    assert f.nnz.value == kept + g.tail.nnz, f"*nnzC {f.nnz.value}, expected {kept + g.tail.nnz}"
    C = f.values()
    off = 0
    for n, (a, b) in enumerate(g.row_slices()):
        counts, cols, vals = g.dropped_pad(a, b, DEV)
        want_p = off + torch.cumsum(counts, 0) - counts
        d = lo.first_difference(C.indptr[a:b], want_p)
        assert d is None, f"dense with zeros -> CSR: slice {n}: C.indptr of row {a + d[0]}"
        m = int(cols.numel())
        d = lo.first_difference(C.indices[off:off + m], cols)
        assert d is None, f"dense with zeros -> CSR: slice {n} (rows {a}..{b - 1}): index at C offset {off + d[0]}"
        d = lo.first_bit_difference(C.values[off:off + m], vals)
        assert d is None, f"dense with zeros -> CSR: slice {n} (rows {a}..{b - 1}): value at C offset {off + d[0]}"
        off += m
    _check_tail(g, C, kept, (g.tail.indptr, g.tail.indices, g.tail.data), "dense with zeros -> CSR")
    Dc.check("spg_dense2csr D")
    del f, C, Dc
    _operand_intact(big)


# ------------------------------------------------------------------------------------ 16-bit columns

def test_cols16(big):
    from spmm_amd import distributed as dist
    from spmm_amd.sparse import csr_matrix
    g = big.g
    h = _handle()
    _require("spg_cols16_split / spg_cols16_join", lo.planned_bytes(g)["cols16"])
    M = g.build(DEV, mul=lo.WIDE_MUL, cols=lo.WIDE_COLS, values=False)
    vm = _desc(M)
    starts = guarded((g.rows, 2), np.int32, 0xFF, DEV, "block_starts")      # (uint32 bits)
    lo16 = guarded(g.nnz, np.int16, 0xFF, DEV, "lo16")
    st = h.lib.spg_cols16_split(h.ptr, ctypes.byref(vm), ctypes.c_void_p(starts.data_ptr()), ctypes.c_void_p(lo16.data_ptr()))
    assert st == 0, st
    torch.cuda.synchronize()
    for n, (a, b) in enumerate(_chunks(g.nnz, g.slice_entries)):
        d = lo.first_difference(lo16.t[a:b].to(torch.int32) & 0xFFFF, M.indices[a:b] & 0xFFFF)
        assert d is None, f"lo16: slice {n}, offset {a + d[0]}"
    for n, (a, b) in enumerate(g.row_slices()):
        want = g.block_starts_pad(a, b, DEV)
        d = lo.first_difference(starts.t[a:b], want)
        assert d is None, (f"block_starts: slice {n}, row {a + d[0]} (offsets from {(a + d[0]) * g.L}), block {d[1] + 1}: "
                           f"{int(starts.t[a + d[0], d[1]])}, expected {int(want[d])}")
    T = g.tail
    host = csr_matrix._from_parts(torch.from_numpy(np.array(T.data)), torch.from_numpy(T.indices.astype(np.int32) * lo.WIDE_MUL),
                                  torch.from_numpy(T.indptr.astype(np.int64)), (g.tail_rows, lo.WIDE_COLS), canonical=True)
    want_starts, _ = dist._cols16_split_host(host, 2)
    assert torch.equal(starts.t[g.pad_rows:].cpu(), want_starts), "block_starts of the tail"
    for b in (starts, lo16):
        b.check("spg_cols16_split " + b.name)
    out = guarded(g.nnz, np.int32, 0xFF, DEV, "joined indices")
    vj = _desc(lo.Csr(g.rows, lo.WIDE_COLS, M.indptr, out.t, None))
    st = h.lib.spg_cols16_join(h.ptr, ctypes.byref(vj), ctypes.c_void_p(starts.data_ptr()), ctypes.c_void_p(lo16.data_ptr()))
    assert st == 0, st
    torch.cuda.synchronize()
    _same_bytes(out.t, M.indices, "spg_cols16_join against the indices", g)
    out.check("spg_cols16_join indices")
    d = g.first_pad_difference(M, mul=lo.WIDE_MUL)
    assert d is None, f"the operand changed: {d}"
    del M, starts, lo16, out


# ------------------------------------------------------------------------------------ the Python shim

def test_python_shim_retries_with_int64(big):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    g, A = big.g, big.A
    dense = g.rows * g.W * 4
    touched, Bs = g.small_operand()
    _, extra = g.expect_sum(touched, Bs, 1, 1)
    nnzc = g.nnz + int(extra[-1])
    _require("cusparse.dense2csr / cusparse.csrgeam2",
             max(dense + g.csr_bytes(), 2 * (g.rows + 1) * 8 + nnzc * 8 + Bs.nnz * 8) + lo.planned_bytes(g)["validate"],
             24 * (g.rows + 1) + 8 * Bs.nnz + 4096,       # (the shim queries for itself: table + counts + marks)
             planned=lo.planned_bytes(g)["shim"])
    D = torch.empty((g.rows, g.W), dtype=torch.float32, device=DEV)
    for a, b in g.row_slices():
        D[a:b] = g.pad_dense(a, b, DEV)
    D[g.pad_rows:] = torch.from_numpy(g.tail.toarray()).to(DEV)
    C = cusparse.dense2csr(D)
    del D
    assert C.indptr.dtype == (torch.int64 if big.full else torch.int32)
    assert torch.equal(C.indptr.to(torch.int64), A.indptr), "dense2csr: indptr"
    _same_bytes(C.indices, A.indices, "cusparse.dense2csr: indices against A's", g)
    _same_bytes(C.data, A.values, "cusparse.dense2csr: values against A's", g)
    del C
    B = g.spread_small(touched, Bs, DEV)
    a = csr_matrix._from_parts(A.values, A.indices, A.indptr, (g.rows, g.W), canonical=True)
    b = csr_matrix._from_parts(B.values, B.indices, B.indptr, (g.rows, g.W), canonical=True)
    C = cusparse.csrgeam2(a, b)
    assert C.indptr.dtype == (torch.int64 if big.full else torch.int32) and C.nnz == nnzc
    Cs, extra = g.expect_sum(touched, Bs, 1, 1)
    _check_sum(g, A, C.indptr.to(torch.int64), C.indices, C.data, touched, Cs, extra, "cusparse.csrgeam2")
    del C, a, b, B
    _operand_intact(big)
