"""``spgemm`` -- the drop-in for ``cupyx.cusparse.spgemm`` (the reference's hot-path
boundary, modify_src/cupy-src/cupyx/cusparse.py:2007-2142), backed by libmi355_spgemm.so.

Same signature, argument meaning and error behaviour as the reference:

* ``RuntimeError('spgemm is not available.')`` when the engine cannot run
  (``check_availability``, cusparse.py:169-186 / :2022-2023);
* ``TypeError`` for a non-CSR operand (:2026-2029), ``ValueError('mismatched shape')``
  (:2032-2033), ``assert a.has_canonical_format`` (:2030-2031);
* dtype promotion of the operands (``_cast_common_type``, :52-56);
* ``alg``: 1 -> ALG1 (single pass), 2 -> ALG2 (two phase), 3 -> ALG3 (chunked two phase,
  uses ``chunk_fraction``), anything else -> the library default.  Note: the reference maps
  ``alg=1`` to CUSPARSE_SPGEMM_DEFAULT (cusparse.py:2056-2057) while its C++ "ALG1" driver
  uses CUSPARSE_SPGEMM_ALG1; here ``alg=1`` always means ALG1.
* ``verbose`` prints the workspace size like the reference prints buff2 (:2106-2107).

Device memory comes from torch's caching allocator on the current device; work runs on the
current torch stream.  The result's ``indptr`` is int32 when nnz(C) < 2**31, int64 beyond.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import torch

from . import _fastpath, _lib
from ._lib import SpgCsr, SpgError, check
from .sparse import _axis_selector, _indptr_dtype, coo_matrix, csc_matrix, csr_matrix

_VT = {torch.float32: _lib.SPG_R_32F, torch.float64: _lib.SPG_R_64F,
       torch.complex64: _lib.SPG_C_32F, torch.complex128: _lib.SPG_C_64F}
# host alpha of C's value type: one scalar, or a (real, imag) pair for complex
_ALPHA_CT = {torch.float32: (ctypes.c_float, 1), torch.float64: (ctypes.c_double, 1),
             torch.complex64: (ctypes.c_float, 2), torch.complex128: (ctypes.c_double, 2)}
_IT = {torch.int32: _lib.SPG_INDEX_32I, torch.int64: _lib.SPG_INDEX_64I}
_ALG = {1: _lib.SPG_ALG1, 2: _lib.SPG_ALG2, 3: _lib.SPG_ALG3}


@dataclass
class SpgemmStats:
    """Accounting of the last spgemm call on this process (for the profilers)."""
    alg: int = 0
    workspace_bytes: int = 0
    peak_bytes: int = 0        # workspace + C (spg_peak_bytes)
    num_products: int = -1
    nnz: int = 0


last_stats = SpgemmStats()


_available = None


def check_availability(name: str) -> bool:
    """True when the named routine can run here (a gfx950 device and the built library).
    Memoized like the reference's ``@_util.memoize()`` check (cusparse.py:169-186)."""
    global _available
    if name not in ("spgemm", "spmv", "spmm", "validate_csr", "csr2csc", "csc2csr", "csrgeam2", "csrgeam",
                    "canonicalize", "csrsort", "csr2dense", "csc2dense", "dense2csr", "dense2csc",
                    "denseToSparse", "sparseToDense", "extract"):
        raise ValueError(f"No available version information specified for {name}")
    if _available is None:
        try:
            _available = bool(torch.cuda.is_available())
            if _available:
                _lib.get_handle(torch.cuda.current_device())
        except Exception:
            _available = False
    return _available


def _check_type(x, kinds) -> None:
    if not isinstance(x, kinds):
        raise TypeError("unsupported type (actual: {})".format(type(x)))


def _check_device(x, name: str) -> None:
    if x.device.type != "cuda":
        raise RuntimeError(f"{name} needs device-resident operands")


def _guard(name: str, x=None, kinds=None) -> None:
    """What a public function opens with, in this order: the routine can run here, and (with
    `kinds`) its operand has one of these types and sits on a GPU."""
    if not check_availability(name):
        raise RuntimeError(f"{name} is not available.")
    if kinds is not None:
        _check_type(x, kinds)
        _check_device(x, name)


def _view(rows, cols, nnz, indptr, indices, data, dtype, index_dtype=None) -> SpgCsr:
    """The spg_csr_t of CSR arrays; an empty matrix has null indices and values.  ``data`` None:
    the structure alone.  ``indptr`` None (COO input): no row pointer, of type `index_dtype`."""
    return SpgCsr(rows, cols, nnz, indptr.data_ptr() if indptr is not None else 0,
                  indices.data_ptr() if nnz else 0, data.data_ptr() if nnz and data is not None else 0,
                  _IT[index_dtype or indptr.dtype], _VT[dtype])


def _csr_view(m: csr_matrix) -> SpgCsr:
    return _view(m.shape[0], m.shape[1], m.nnz, m.indptr, m.indices, m.data, m.data.dtype)


def _current_stream_ptr(dev: int) -> int:
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # (no Stream object per call)
    return raw(dev) if raw is not None else torch.cuda.current_stream(dev).cuda_stream


def _handle_on(dev) -> _lib.Handle:
    """This thread's handle for the device of `dev`, set to the current torch stream."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    h = _lib.get_handle(idx)
    h.set_stream(_current_stream_ptr(idx))
    return h


def _handle_for(m: csr_matrix) -> _lib.Handle:
    return _handle_on(m.device)


def _alpha_of(dtype, alpha):
    """A host scalar of the value type: one number, or a (real, imag) pair for complex."""
    ct, nparts = _ALPHA_CT[dtype]
    return (ct * 2)(complex(alpha).real, complex(alpha).imag) if nparts == 2 else ct(float(alpha))


def _sized_workspace(call, where: str, dev, verbose_alg=None):
    """The size query ``call(byref(ws_bytes), None)`` and a workspace of that size:
    (ws, ws_bytes, its pointer).  The caller keeps `ws` until its last call with it is queued."""
    ws_bytes = ctypes.c_size_t(0)
    check(call(ctypes.byref(ws_bytes), None), where)
    if verbose_alg is not None:
        print("USING ALG", verbose_alg, "workspace GB =", ws_bytes.value / (1024 ** 3))
    # from torch's caching allocator on the current stream (the library works on that stream,
    # so a later reuse of the block is ordered after this operation)
    ws = torch.empty(max(ws_bytes.value, 1), dtype=torch.uint8, device=dev)
    return ws, ws_bytes, ctypes.c_void_p(ws.data_ptr())


def _structure(call, rows: int, indptr_dtypes, dev):
    """``call(row pointer, its index type)`` into a fresh row pointer of each dtype in turn
    while the answer is OVERFLOW (nnz(C) past int32): (the last status, the row pointer)."""
    for it in indptr_dtypes:
        indptr = torch.empty(rows + 1, dtype=it, device=dev)
        st = call(ctypes.c_void_p(indptr.data_ptr()), _IT[it])
        if st != _lib.STATUS_OVERFLOW:
            break
    return st, indptr


def _empty_c(rows, cols, nnz, indptr, dtype, dev):
    """(data, indices, view) of a result whose row pointer is filled: its arrays, to be written."""
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=dtype, device=dev)
    return data, indices, _view(rows, cols, nnz, indptr, indices, data, dtype)


def _two_phase(h, names, sargs, vargs, rows, cols, dtype, indptr_dtypes, dev):
    """The frame of a format operation with a structure call and a value call (include/spgemm.h):

        names[0](h, *sargs, C's row pointer, its index type, &nnz, &ws_bytes, ws)
        names[1](h, *vargs, C, ws_bytes, ws)

    The size query (null pointers, the first of `indptr_dtypes`), the workspace, the structure
    call -- once more per further dtype while it answers OVERFLOW; one dtype: OVERFLOW raises --
    then C's arrays, rows x cols of `dtype`, and the value call.  `vargs` may be a callable that
    gives them: it runs after the structure call (csrgeam2 converts its scalars there).
    (data, indices, indptr) of C."""
    structure = functools.partial(getattr(h.lib, names[0]), h.ptr, *sargs)
    nnz = ctypes.c_int64(0)
    nnz_p, it0 = ctypes.byref(nnz), _IT[indptr_dtypes[0]]
    ws, ws_bytes, wp = _sized_workspace(lambda wb, p: structure(None, it0, nnz_p, wb, p), names[0], dev)
    wb = ctypes.byref(ws_bytes)
    st, indptr = _structure(lambda ip, it: structure(ip, it, nnz_p, wb, wp), rows, indptr_dtypes, dev)
    check(st, names[0])
    data, indices, vc = _empty_c(rows, cols, int(nnz.value), indptr, dtype, dev)
    vargs = vargs() if callable(vargs) else vargs
    check(getattr(h.lib, names[1])(h.ptr, *vargs, ctypes.byref(vc), ws_bytes, wp), names[1])
    return data, indices, indptr


@contextlib.contextmanager
def _planned(h, a, b, algo, cf, verbose_alg=None):
    """spg_plan (size query) -> workspace -> spg_plan (build): (plan, workspace bytes) for the
    block, with the workspace and the operand views kept; spg_plan_destroy on the way out."""
    va, vb = _csr_view(a), _csr_view(b)
    plan = ctypes.c_void_p()

    def call(ws_bytes, ws):
        return h.lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), algo, cf, ws_bytes, ws,
                              None if ws is None else ctypes.byref(plan))
    ws, ws_bytes, wp = _sized_workspace(call, "spg_plan", a.device, verbose_alg)
    check(call(ctypes.byref(ws_bytes), wp), "spg_plan")
    try:
        yield plan, ws_bytes.value
    finally:
        h.lib.spg_plan_destroy(plan)


def validate_csr(m: csr_matrix) -> int:
    """1 canonical, 0 unsorted/duplicates, -1 malformed (spg_validate_csr)."""
    _check_device(m, "validate_csr")
    h = _handle_for(m)
    v = _csr_view(m)
    res = ctypes.c_int(0)
    check(h.lib.spg_validate_csr(h.ptr, ctypes.byref(v), ctypes.byref(res)), "spg_validate_csr")
    return res.value


def _cols16_nb1(cols: int) -> int:
    """Interior 65536-column block starts per row (include/spgemm.h, spg_cols16_*)."""
    return max(0, -(-int(cols) // 65536) - 1)


def _cols16_split(m: csr_matrix):
    """(block_starts int32 [rows, nb1], lo16 int16 [nnz]) of a device CSR (spg_cols16_split)."""
    rows, nb1 = m.shape[0], _cols16_nb1(m.shape[1])
    starts = torch.empty((rows, nb1), dtype=torch.int32, device=m.device)
    lo16 = torch.empty(m.nnz, dtype=torch.int16, device=m.device)
    h = _handle_for(m)
    v = _view(rows, m.shape[1], m.nnz, m.indptr, m.indices, None, torch.float64)
    check(h.lib.spg_cols16_split(h.ptr, ctypes.byref(v), ctypes.c_void_p(starts.data_ptr() if starts.numel() else 0),
                                 ctypes.c_void_p(lo16.data_ptr() if m.nnz else 0)), "spg_cols16_split")
    return starts, lo16


def _cols16_join(indptr: torch.Tensor, starts: torch.Tensor, lo16: torch.Tensor, shape) -> torch.Tensor:
    """int32 column indices from a device (indptr, block starts, low halves) (spg_cols16_join)."""
    rows, cols = shape
    nnz = lo16.numel()
    out = torch.empty(nnz, dtype=torch.int32, device=indptr.device)
    h = _handle_on(indptr.device)
    v = _view(rows, cols, nnz, indptr, out, None, torch.float64)
    check(h.lib.spg_cols16_join(h.ptr, ctypes.byref(v), ctypes.c_void_p(starts.data_ptr() if starts.numel() else 0),
                                ctypes.c_void_p(lo16.data_ptr() if nnz else 0)), "spg_cols16_join")
    return out


_VALUE_DTYPES = (torch.float32, torch.float64, torch.complex64, torch.complex128)


def _cast_common_type(a: csr_matrix, b: csr_matrix):
    if a.data.dtype is b.data.dtype and a.data.dtype in _VALUE_DTYPES:   # (the per-call common case)
        return a, b
    dt = np.promote_types(a.dtype, b.dtype)
    if dt not in (np.float32, np.float64, np.complex64, np.complex128):
        raise TypeError(f"spgemm supports float32/float64/complex64/complex128, got {dt}")
    return a.astype(dt), b.astype(dt)


def spgemm(a, b, alpha=1, alg=0, chunk_fraction=0.2, verbose=False):
    """Matrix-matrix product for CSR matrices: ``C = alpha * A * B``.

    Args:
        a (csr_matrix): sparse matrix A (m x k), canonical format.
        b (csr_matrix): sparse matrix B (k x n), canonical format.
        alpha (scalar): coefficient.
        alg (int): 1, 2, 3 select ALG1/ALG2/ALG3; other values the default.
        chunk_fraction (float): ALG3 chunk size as a fraction of the products, (0, 1].
        verbose (bool): print the workspace size.

    Returns:
        csr_matrix: C, with sorted column indices and structural entries kept.
    """
    return _spgemm(a, b, alpha, alg, chunk_fraction, verbose)


def _spgemm(a, b, alpha=1, alg=0, chunk_fraction=0.2, verbose=False, before_numeric=None, by_tiles=None,
            values_first=True):
    """spgemm, plus `before_numeric`: a callable run after the symbolic pass and before the
    numeric pass reads the values (the multi-GPU path waits there for B's values to arrive
    over RCCL; spmm_amd.distributed).  With it the call takes the ctypes path (the native
    shim runs both passes in one call); ALG1 runs it first (its count and numeric passes
    are queued together).

    `by_tiles(geom)`: the numeric pass by column-tile groups (spg_numeric_tiles), called
    exactly once per product, BEFORE the symbolic pass (the plan's tile layout needs only
    B's structure, so B's values can travel while the symbolic pass runs; _spgemm_by_tiles;
    ``values_first=False``: after it, round 4's order, for the bench's comparison).
    `geom` is None when the plan cannot
    run by tiles (not the tile path, several row chunks, ALG1); then `by_tiles` makes
    b.data complete and returns None, and spg_numeric runs.  Otherwise geom is a dict
    (tile_width, tiles, offsets: the tiles + 1 tile-major value offsets, tile_values(): B's
    values permuted tile-major by this plan, dtype: the plan's value type) and `by_tiles` returns (tm, groups): the
    tile-major values tensor and an iterable of (tile_begin, tile_end) ranges, each yielded
    once its slice of tm is ready on the current stream, together covering every tile."""
    _guard("spgemm")
    assert a.ndim == b.ndim == 2
    _check_type(a, csr_matrix)
    _check_type(b, csr_matrix)
    assert a.has_canonical_format
    assert b.has_canonical_format
    if a.shape[1] != b.shape[0]:
        raise ValueError("mismatched shape")
    if a.device != b.device:
        raise ValueError("operands are on different devices")

    m, _ = a.shape
    _, n = b.shape
    a, b = _cast_common_type(a, b)
    if a.indptr.dtype != b.indptr.dtype:   # the engine takes one row-pointer type for A and B
        a = csr_matrix((a.data, a.indices, a.indptr.to(torch.int64)), shape=a.shape, canonical=True)
        b = csr_matrix((b.data, b.indices, b.indptr.to(torch.int64)), shape=b.shape, canonical=True)
        # (the constructor narrows a row pointer that fits back to int32: this is what widens them)
        a.indptr, b.indptr = a.indptr.to(torch.int64), b.indptr.to(torch.int64)
    algo = _ALG.get(alg, _lib.SPG_ALG_DEFAULT)
    if algo == _lib.SPG_ALG3 and not (0.0 < float(chunk_fraction) <= 1.0):
        raise ValueError(f"chunk_fraction must be in (0,1], got {chunk_fraction}")

    dev = a.device
    h = _handle_for(a)
    cf = float(chunk_fraction)
    fp = _fastpath.get() if before_numeric is None and by_tiles is None else None
    if before_numeric is not None and algo == _lib.SPG_ALG1:
        before_numeric()
        before_numeric = None
    if by_tiles is not None and algo == _lib.SPG_ALG1:
        if by_tiles(None) is not None:
            raise RuntimeError("by_tiles must complete B's values when geom is None")
        by_tiles = None
    if by_tiles is not None:
        return _spgemm_by_tiles(h, a, b, alpha, algo, cf, by_tiles, verbose, values_first)
    if fp is not None:   # the same sequence in one native call (csrc/fastpath.cpp)
        al = complex(alpha)
        st, data, indices, indptr, wsb, peak = fp.spgemm(
            h.ptr.value, m, a.shape[1], n, a.indptr, a.indices, a.data, b.indptr, b.indices, b.data,
            int(algo), cf, al.real, al.imag)
        check(st, "spg_spgemm_ws")
        if verbose:
            print("USING ALG", alg, "workspace GB =", wsb / (1024 ** 3))
        return _product(data, indices, indptr, (m, n), False, algo, wsb, peak)
    lib = h.lib
    va, vb = _csr_view(a), _csr_view(b)
    ws, ws_bytes, wp = _sized_workspace(
        lambda wb, p: lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), algo, cf, wb, p, None),
        "spg_plan", dev, alg if verbose else None)
    al = _alpha_of(a.data.dtype, alpha)
    nnz, peak = ctypes.c_int64(0), ctypes.c_size_t(0)
    pj, px, plan = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    # plan -> symbolic (nnz(C) to the host) -> numeric in one call (spg_spgemm_ws)
    wide, tries = _indptr_tries(a, b)
    st, indptr = _structure(
        lambda ip, it: lib.spg_spgemm_ws(h.ptr, ctypes.byref(va), ctypes.byref(vb), algo, cf, ctypes.byref(al), wp,
                                         ws_bytes.value, ip, it, ctypes.byref(nnz), ctypes.byref(pj),
                                         ctypes.byref(px), ctypes.byref(peak), ctypes.byref(plan)), m, tries, dev)
    check(st, "spg_spgemm_ws")
    nnzc = int(nnz.value)
    if pj.value:
        # ALG1: C sits compact (scaled) in the workspace -- views of it
        base = ws.data_ptr()
        oj, ox = pj.value - base, px.value - base
        indices = ws[oj:oj + 4 * nnzc].view(torch.int32)
        data = ws[ox:ox + a.data.element_size() * nnzc].view(a.data.dtype)
    else:
        try:
            data, indices, vc = _empty_c(m, n, nnzc, indptr, a.data.dtype, dev)
            if before_numeric is not None:
                before_numeric()
            check(lib.spg_numeric(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc)), "spg_numeric")
        finally:
            lib.spg_plan_destroy(plan)
    return _product(data, indices, indptr, (m, n), wide, algo, ws_bytes.value, peak.value)


def _indptr_tries(a, b):
    """(wide, the row-pointer dtypes to try) of a product: int64 once nnz(C) >= 2**31, and int64
    first (`wide`) when the expected product count reaches 2**31 -- an overflowing int32 try
    would redo the plan and the symbolic pass."""
    wide = a.nnz * (b.nnz / max(b.shape[0], 1)) >= 2 ** 31
    return wide, ((torch.int64,) if wide else (torch.int32, torch.int64))


def _product(data, indices, indptr, shape, wide, algo, ws_bytes, peak):
    """The product's csr_matrix, its accounting left in last_stats."""
    nnzc = int(indices.numel())
    if wide and nnzc < 2 ** 31:
        indptr = indptr.to(torch.int32)   # the int32 contract when the result fits
    last_stats.alg, last_stats.workspace_bytes = int(algo), int(ws_bytes)
    last_stats.peak_bytes, last_stats.nnz = int(peak), nnzc
    return csr_matrix._from_parts(data, indices, indptr, shape, canonical=True)


def _spgemm_by_tiles(h, a, b, alpha, algo, cf, by_tiles, verbose, values_first=True):
    """_spgemm with `by_tiles` (the row-block step of spmm_amd.distributed): spg_plan, then
    the tile geometry -- spg_tile_value_offsets builds the plan's tile layout from B's
    structure alone -- and ``by_tiles(geom)``, which starts B's values travelling group by
    group; only then spg_symbolic, which runs while they arrive, and the numeric tiles of
    each group as it is released (spg_numeric after the row-major fallback)."""
    lib = h.lib
    m, n = a.shape[0], b.shape[1]
    dev = a.device
    with _planned(h, a, b, algo, cf, algo if verbose else None) as (plan, ws_bytes):
        al = _alpha_of(a.data.dtype, alpha)
        if values_first:
            geom = _tile_geometry(h, plan, b)
            got = by_tiles(geom)
        nnz = ctypes.c_int64(0)
        wide, tries = _indptr_tries(a, b)
        st, indptr = _structure(lambda ip, it: lib.spg_symbolic(h.ptr, plan, ip, it, ctypes.byref(nnz)), m, tries, dev)
        check(st, "spg_symbolic")
        if not values_first:
            geom = _tile_geometry(h, plan, b)
            got = by_tiles(geom)
        if got is not None and geom is None:
            raise RuntimeError("by_tiles returned tile groups for a plan that cannot run by tiles")
        data, indices, vc = _empty_c(m, n, int(nnz.value), indptr, a.data.dtype, dev)
        if got is None:
            check(lib.spg_numeric(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc)), "spg_numeric")
        else:
            _numeric_groups(h, plan, al, vc, got, geom)
        peak = ctypes.c_size_t(0)
        check(lib.spg_peak_bytes(plan, ctypes.byref(peak)), "spg_peak_bytes")
    return _product(data, indices, indptr, (m, n), wide, algo, ws_bytes, peak.value)


def _tile_geometry(h, plan, b):
    """The by_tiles geometry of a plan (see _spgemm), or None when it cannot run by tiles."""
    lib = h.lib
    info = _lib.SpgPlanInfo()
    check(lib.spg_plan_info(plan, ctypes.byref(info), None, 0), "spg_plan_info")
    # (a development library built without the tile-group entry points: spg_numeric)
    has_tiles = all(hasattr(lib, f) for f in ("spg_tile_value_offsets", "spg_tile_values", "spg_numeric_tiles"))
    if not (has_tiles and info.path == 2 and info.n_chunks == 1):
        return None
    # value tiles: record_group adjacent numeric tiles (include/spgemm.h)
    rg = max(1, int(info.record_group))
    G = (int(info.tiles_per_row) + rg - 1) // rg
    offs = (ctypes.c_int64 * (G + 1))()
    st = lib.spg_tile_value_offsets(h.ptr, plan, offs, G + 1)
    if st == _lib.STATUS_NOT_SUPPORTED:
        return None
    check(st, "spg_tile_value_offsets")

    def tile_values():
        tm = torch.empty(max(b.nnz, 1), dtype=b.data.dtype, device=b.data.device)
        check(lib.spg_tile_values(h.ptr, plan, ctypes.c_void_p(tm.data_ptr())), "spg_tile_values")
        return tm[:b.nnz]
    return {"tile_width": int(info.tile_width) * rg, "tiles": G,
            "offsets": np.frombuffer(offs, dtype=np.int64).copy(), "tile_values": tile_values,
            "dtype": b.data.dtype}


def _numeric_groups(h, plan, al, vc, got, geom):
    """spg_numeric_tiles for each (tile_begin, tile_end) group `by_tiles` releases."""
    tm, groups = got
    covered = 0
    for g0, g1 in groups:
        if g0 != covered:
            raise RuntimeError(f"tile groups must be consecutive: expected {covered}, got {g0}")
        check(h.lib.spg_numeric_tiles(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc),
                                      ctypes.c_void_p(tm.data_ptr() if tm.numel() else 0), int(g0), int(g1)),
              "spg_numeric_tiles")
        covered = g1
    if covered != geom["tiles"]:
        raise RuntimeError(f"tile groups covered {covered} of {geom['tiles']} tiles")


def _sparse_operand(name: str, a, transa: bool):
    """(A as a csr_matrix, transa) of spmv's / spmm's sparse operand: a CSC matrix goes through
    its free transpose with ``transa`` flipped (as the reference does), a COO matrix through CSR."""
    _guard(name)
    if isinstance(a, csc_matrix):
        a = a.T
        transa = not transa
    _check_type(a, (csr_matrix, coo_matrix))
    if isinstance(a, coo_matrix):
        a = a.tocsr()
    return a, transa


def _promoted(name: str, a, dense_dtype):
    """A in the common value type of A and the dense operand."""
    dt = np.promote_types(a.dtype, np.dtype(str(dense_dtype).replace("torch.", "")))
    if dt not in (np.float32, np.float64, np.complex64, np.complex128):
        raise TypeError(f"{name} supports float32/float64/complex64/complex128, got {dt}")
    return a.astype(dt)


def spmv(a, x, y=None, alpha=1, beta=0, transa=False):
    """y = alpha * op(A) x + beta * y -- the drop-in for ``cupyx.cusparse.spmv``
    (modify_src/cupy-src/cupyx/cusparse.py:1373-1432), on ``spg_spmv``.

    A is csr_matrix, csc_matrix or coo_matrix (CSC goes through its transpose as the
    reference does, COO through CSR).  x, y are 1-D tensors (or numpy arrays, uploaded).
    With CSR A, alpha = 1 and beta = 0 the result equals scipy's ``A @ x`` bit for bit; so do
    ``transa=True`` and a CSC operand against scipy's ``A.T @ x`` / ``A @ x``: the transpose is
    spg_csr2csc's stable counting sort, scipy's own (csr_tocsc), so the sums keep scipy's order.
    """
    a, transa = _sparse_operand("spmv", a, transa)
    if transa:
        a = a.transpose_csr()
    dev = a.device
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(dev)
    if a.shape[1] != x.numel():
        raise ValueError("dimension mismatch")
    assert a.has_canonical_format
    m = a.shape[0]
    a = _promoted("spmv", a, x.dtype)
    tdt = a.data.dtype
    x = x.to(tdt).contiguous()
    if y is None:
        y = torch.zeros(m, dtype=tdt, device=dev)
    else:
        if not isinstance(y, torch.Tensor) or y.numel() != m:
            raise ValueError("dimension mismatch")
        if y.dtype != tdt or not y.is_contiguous():
            raise TypeError("y must be a contiguous tensor of the result type")
    if a.nnz == 0:       # the reference fills 0 (cusparse.py:1414-1416)
        y.fill_(0)
        return y
    h = _handle_for(a)
    va = _csr_view(a)
    al, be = _alpha_of(tdt, alpha), _alpha_of(tdt, beta)
    check(h.lib.spg_spmv(h.ptr, ctypes.byref(va), ctypes.c_void_p(x.data_ptr()), ctypes.byref(al),
                         ctypes.byref(be), ctypes.c_void_p(y.data_ptr())), "spg_spmv")
    return y


def _dense_layout(t: torch.Tensor, prefer=None):
    """(order, ld) of a 2-D tensor the engine can address in place, or None: unit stride
    along columns is SPG_ORDER_ROW with ld = stride(0), unit stride along rows is
    SPG_ORDER_COL with ld = stride(1).  An extent of 1 leaves its stride free, so such a
    tensor may read as either order: `prefer` picks (row-major otherwise)."""
    r, c = t.shape
    s0, s1 = t.stride()
    row = col = None
    if (c <= 1 or s1 == 1) and (r <= 1 or s0 >= c):
        row = (_lib.SPG_ORDER_ROW, max(s0 if r > 1 else c, 1))
    if (r <= 1 or s0 == 1) and (c <= 1 or s1 >= r):
        col = (_lib.SPG_ORDER_COL, max(s1 if c > 1 else r, 1))
    if prefer == _lib.SPG_ORDER_COL and col is not None:
        return col
    return row or col


def _dense_view(t: torch.Tensor, order: int, ld: int) -> _lib.SpgDense:
    return _lib.SpgDense(t.shape[0], t.shape[1], ld, t.data_ptr() if t.numel() else 0, order, _VT[t.dtype])


def _in_order(t: torch.Tensor, order: int) -> torch.Tensor:
    """A copy of t with unit stride along columns (ROW) or rows (COL)."""
    return t.contiguous() if order == _lib.SPG_ORDER_ROW else t.t().contiguous().t()


def spmm(a, b, c=None, alpha=1, beta=0, transa=False, transb=False):
    """C = alpha * op(A) op(B) + beta * C -- the drop-in for ``cupyx.cusparse.spmm``
    (modify_src/cupy-src/cupyx/cusparse.py:1440-1513), on ``spg_spmm``.

    A is csr_matrix, csc_matrix or coo_matrix (CSC goes through its transpose as the
    reference does, COO through CSR).  b, c are 2-D tensors (or numpy arrays, uploaded) in
    row-major or column-major layout, read from their strides; ``transb`` is a view and moves
    no data.  The reference takes F-contiguous arrays only; both orders run here, and the
    result has b's order (c's when c is given).  With CSR A, alpha = 1 and beta = 0 the result
    equals scipy's ``A @ B`` bit for bit; so do ``transa=True`` and a CSC operand against scipy's
    ``A.T @ B`` / ``A @ B`` (the transpose is spg_csr2csc's stable counting sort, as in scipy).
    """
    a, transa = _sparse_operand("spmm", a, transa)
    if not isinstance(b, torch.Tensor):
        b = torch.from_numpy(np.asarray(b))
    assert a.ndim == b.ndim == 2
    if transb:
        b = b.t()
    a_shape = a.shape if not transa else a.shape[::-1]
    if a_shape[1] != b.shape[0]:
        raise ValueError("dimension mismatch")
    if transa:
        a = a.transpose_csr()
    assert a.has_canonical_format
    dev = a.device
    m, n = a_shape[0], b.shape[1]
    a = _promoted("spmm", a, b.dtype)
    tdt = a.data.dtype
    b = b.to(device=dev, dtype=tdt)
    lc = None
    if c is not None:
        if not isinstance(c, torch.Tensor):
            c = torch.from_numpy(np.asarray(c)).to(dev)
        if c.ndim != 2 or c.shape[0] != m or c.shape[1] != n:
            raise ValueError("dimension mismatch")
        if c.dtype != tdt or c.device != dev:
            raise TypeError("c must be a tensor of the result type on A's device")
        lc = _dense_layout(c)
        if lc is None:
            raise ValueError("c must have unit stride along its rows or its columns")
    lb = _dense_layout(b, prefer=lc[0] if lc else None)
    if lb is None or (lc is not None and lb[0] != lc[0]):   # copied into c's order (row-major without c)
        order = lc[0] if lc else _lib.SPG_ORDER_ROW
        b = _in_order(b, order)
        lb = _dense_layout(b, prefer=order)
    if c is None:        # zeros in b's order (the reference: zeros((m, n), dtype, 'F'), cusparse.py:1486-1487)
        c = torch.zeros((m, n), dtype=tdt, device=dev) if lb[0] == _lib.SPG_ORDER_ROW \
            else torch.zeros((n, m), dtype=tdt, device=dev).t()
        lc = _dense_layout(c, prefer=lb[0])
    if a.nnz == 0:       # the reference fills 0 (cusparse.py:1490-1492)
        c.fill_(0)
        return c
    h = _handle_for(a)
    va = _csr_view(a)
    vb, vc = _dense_view(b, *lb), _dense_view(c, *lc)
    al, be = _alpha_of(tdt, alpha), _alpha_of(tdt, beta)
    check(h.lib.spg_spmm(h.ptr, ctypes.byref(va), ctypes.byref(vb), ctypes.byref(al), ctypes.byref(be),
                         ctypes.byref(vc)), "spg_spmm")
    return c


# has_*: True when the loaded library exports the operation's entry points (added within 0.2.0:
# an older development build lacks them, and the containers then keep their torch form)

def has_csr2csc() -> bool:
    return _lib.exports(*_lib.CSR2CSC)


def has_csrgeam() -> bool:
    return _lib.exports(*_lib.CSRGEAM)


def has_canonicalize() -> bool:
    return _lib.exports(*_lib.CANONICALIZE)


def has_extract() -> bool:
    return _lib.exports(*_lib.EXTRACT)


def has_dense_convert() -> bool:
    return _lib.exports(*_lib.DENSE_CONVERT)


def _csr2csc_arrays(data, indices, indptr, rows: int, cols: int):
    """(data, indices, indptr) of the transpose of the rows x cols CSR arrays, on spg_csr2csc:
    the CSC arrays of the same matrix.  indptr comes back int32 whenever nnz fits."""
    dev = data.device
    nnz = int(data.numel())
    ipd = _indptr_dtype(nnz)
    out_data = torch.empty(nnz, dtype=data.dtype, device=dev)
    out_indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    if nnz == 0:         # the reference fills zeros without a call (cusparse.py:1023-1024)
        return out_data, out_indices, torch.zeros(cols + 1, dtype=ipd, device=dev)
    data, indices, indptr = data.contiguous(), indices.contiguous(), indptr.to(ipd).contiguous()
    out_indptr = torch.empty(cols + 1, dtype=ipd, device=dev)
    h = _handle_on(dev)
    va = _view(rows, cols, nnz, indptr, indices, data, data.dtype)
    vt = _view(cols, rows, nnz, out_indptr, out_indices, out_data, data.dtype)

    def call(ws_bytes, ws):
        return h.lib.spg_csr2csc(h.ptr, ctypes.byref(va), ctypes.byref(vt), ws_bytes, ws)
    ws, ws_bytes, wp = _sized_workspace(call, "spg_csr2csc", dev)
    check(call(ctypes.byref(ws_bytes), wp), "spg_csr2csc")
    return out_data, out_indices, out_indptr


def csr2csc(x):
    """CSR -> CSC of the same matrix -- the drop-in for ``cupyx.cusparse.csr2csc``
    (modify_src/cupy-src/cupyx/cusparse.py:1014-1035), on ``spg_csr2csc``.  Stable: every
    column keeps x's stored entry order, so the arrays equal scipy's ``tocsc()`` array for array
    (duplicates kept), and the values are moved bit for bit."""
    _guard("csr2csc", x, csr_matrix)
    m, n = x.shape
    data, indices, indptr = _csr2csc_arrays(x.data, x.indices, x.indptr, m, n)
    return csc_matrix((data, indices, indptr), shape=x.shape, canonical=True if x._canonical is True else None)


def csc2csr(x):
    """CSC -> CSR of the same matrix -- the drop-in for ``cupyx.cusparse.csc2csr``
    (modify_src/cupy-src/cupyx/cusparse.py:1092-1113): spg_csr2csc on the CSC arrays read as
    the CSR of the transpose.  Equals scipy's ``tocsr()`` array for array."""
    if not check_availability("csc2csr"):
        raise RuntimeError("csr2csc is not available.")   # (it has always named csr2csc)
    _check_type(x, csc_matrix)
    _check_device(x, "csc2csr")
    m, n = x.shape
    data, indices, indptr = _csr2csc_arrays(x.data, x.indices, x.indptr, n, m)
    return csr_matrix._from_parts(data, indices, indptr, (m, n), canonical=True if x._canonical is True else None)


def _csrgeam_arrays(ax, aj, ap, bx, bj, bp, shape, alpha, beta):
    """(data, indices, indptr) of alpha * A + beta * B for the CSR arrays of two canonical
    matrices of one shape and value type, on spg_csrgeam_nnz + spg_csrgeam."""
    dev, dt = ax.device, ax.dtype
    m, n = shape
    na, nb = int(ax.numel()), int(bx.numel())
    # nnz(C) <= nnz(A) + nnz(B): int32 row pointers whenever that bound fits, so no retry
    ipd = _indptr_dtype(na + nb)
    h = _handle_on(dev)
    ap, bp = ap.to(ipd).contiguous(), bp.to(ipd).contiguous()
    aj, ax, bj, bx = aj.contiguous(), ax.contiguous(), bj.contiguous(), bx.contiguous()
    va, vb = ctypes.byref(_view(m, n, na, ap, aj, ax, dt)), ctypes.byref(_view(m, n, nb, bp, bj, bx, dt))
    return _two_phase(h, ("spg_csrgeam_nnz", "spg_csrgeam"), (va, vb), lambda: (
        ctypes.byref(_alpha_of(dt, alpha)), va, ctypes.byref(_alpha_of(dt, beta)), vb), m, n, dt, (ipd,), dev)


def csrgeam2(a, b, alpha=1, beta=1):
    """Matrix-matrix addition ``C = alpha * A + beta * B`` -- the drop-in for
    ``cupyx.cusparse.csrgeam2`` (modify_src/cupy-src/cupyx/cusparse.py:525-591), on
    ``spg_csrgeam_nnz`` + ``spg_csrgeam``.

    Args:
        a (csr_matrix): sparse matrix A, canonical format.
        b (csr_matrix): sparse matrix B, canonical format, A's shape.
        alpha (scalar): coefficient for A.
        beta (scalar): coefficient for B.

    Returns:
        csr_matrix: C, canonical; its structure is the union of the two patterns (an entry that
        cancels stays as an explicit 0) and its values equal scipy's after dropping exact zeros.
    """
    _guard("csrgeam2")
    _check_type(a, csr_matrix)
    _check_type(b, csr_matrix)
    assert a.has_canonical_format
    assert b.has_canonical_format
    if a.shape != b.shape:
        raise ValueError("inconsistent shapes")
    if a.device.type != "cuda" or b.device != a.device:
        raise RuntimeError("csrgeam2 needs device-resident operands on one device")
    a, b = _cast_common_type(a, b)
    parts = _csrgeam_arrays(a.data, a.indices, a.indptr, b.data, b.indices, b.indptr, a.shape, alpha, beta)
    return csr_matrix._from_parts(*parts, a.shape, canonical=True)


csrgeam = csrgeam2


def has_elementwise() -> bool:
    return _lib.exports(*_lib.ELEMENTWISE)


_BINOPS = {"multiply": _lib.SPG_BINOP_MUL, "maximum": _lib.SPG_BINOP_MAX, "minimum": _lib.SPG_BINOP_MIN}


def _binop_arrays(ax, aj, ap, bx, bj, bp, shape, op: int):
    """(data, indices, indptr) of op(A, B) (an SPG_BINOP_* code) for the CSR arrays of two canonical
    matrices of one shape and value type, on spg_csr_binop_nnz + spg_csr_binop.  The operands' row
    pointers are int32 whenever both entry counts fit; C's is tried as int32 first and as int64
    after an OVERFLOW answer."""
    dev, dt = ax.device, ax.dtype
    m, n = shape
    na, nb = int(ax.numel()), int(bx.numel())
    ipd = _indptr_dtype(max(na, nb))
    h = _handle_on(dev)
    ap, bp = ap.to(ipd).contiguous(), bp.to(ipd).contiguous()
    aj, ax, bj, bx = aj.contiguous(), ax.contiguous(), bj.contiguous(), bx.contiguous()
    va, vb = ctypes.byref(_view(m, n, na, ap, aj, ax, dt)), ctypes.byref(_view(m, n, nb, bp, bj, bx, dt))
    tries = (torch.int32, torch.int64) if ipd is torch.int32 else (torch.int64,)
    # _two_phase's steps, with one branch it has not: C's structure depends on the values, so
    # nnz(C) == 0 is an ordinary answer here, and then there is nothing for a value call to write
    structure = functools.partial(h.lib.spg_csr_binop_nnz, h.ptr, op, va, vb)
    nnz = ctypes.c_int64(0)
    nnz_p = ctypes.byref(nnz)
    ws, ws_bytes, wp = _sized_workspace(lambda wb, p: structure(None, _IT[tries[0]], nnz_p, wb, p),
                                        "spg_csr_binop_nnz", dev)
    wb = ctypes.byref(ws_bytes)
    st, indptr = _structure(lambda ip, it: structure(ip, it, nnz_p, wb, wp), m, tries, dev)
    check(st, "spg_csr_binop_nnz")
    data, indices, vc = _empty_c(m, n, int(nnz.value), indptr, dt, dev)
    if nnz.value:
        check(h.lib.spg_csr_binop(h.ptr, op, va, vb, ctypes.byref(vc), ws_bytes, wp), "spg_csr_binop")
    return data, indices, indptr


def csrbinop(a, b, op):
    """Element-wise ``op(A, B)`` of two CSR matrices, ``op`` one of ``"multiply"``, ``"maximum"``,
    ``"minimum"`` -- what cupyx's ``csr_matrix.multiply`` / ``maximum`` / ``minimum`` compute with
    kernels of their own (modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:328-342, :297-326), on
    ``spg_csr_binop_nnz`` + ``spg_csr_binop``.

    Args:
        a (csr_matrix): sparse matrix A, canonical format.
        b (csr_matrix): sparse matrix B, canonical format, A's shape.
        op (str): the operation's name.

    Returns:
        csr_matrix: C, canonical: over the union of the two patterns the entries whose result is
        not zero, array for array what scipy's ``A.multiply(B)`` / ``A.maximum(B)`` /
        ``A.minimum(B)`` gives.
    """
    if not (check_availability("csrgeam2") and has_elementwise()):   # a device, and a library with the entry points
        raise RuntimeError("csrbinop is not available.")
    _check_type(a, csr_matrix)
    _check_type(b, csr_matrix)
    if op not in _BINOPS:
        raise ValueError(f"op must be one of {', '.join(_BINOPS)} (actual: {op!r})")
    assert a.has_canonical_format
    assert b.has_canonical_format
    if a.shape != b.shape:
        raise ValueError("inconsistent shapes")
    if a.device.type != "cuda" or b.device != a.device:
        raise RuntimeError("csrbinop needs device-resident operands on one device")
    a, b = _cast_common_type(a, b)
    parts = _binop_arrays(a.data, a.indices, a.indptr, b.data, b.indices, b.indptr, a.shape, _BINOPS[op])
    return csr_matrix._from_parts(*parts, a.shape, canonical=True)


def _mul_dense_arrays(data, indices, indptr, shape, d: torch.Tensor, out=None):
    """data[e] * d[i, j] for every stored entry e = (i, j) of the m x n CSR arrays, on
    spg_csr_mul_dense: a new tensor, or ``out`` (which may be ``data`` itself).  ``d`` is a 2-D
    tensor of data's dtype on its device, m or 1 rows by n or 1 columns (an extent of 1 is
    broadcast), addressed in place when it has unit stride along its rows or its columns and
    copied row-major otherwise."""
    dev, dt = data.device, data.dtype
    m, n = shape
    nnz = int(data.numel())
    if d.ndim != 2 or d.shape[0] not in (m, 1) or d.shape[1] not in (n, 1):
        raise ValueError("inconsistent shapes")
    if d.dtype != dt or d.device != dev:
        raise TypeError("d must be a tensor of the matrix's type on its device")
    if out is None:
        out = torch.empty(nnz, dtype=dt, device=dev)
    if nnz == 0:
        return out
    layout = _dense_layout(d)
    if layout is None:
        d = _in_order(d, _lib.SPG_ORDER_ROW)
        layout = _dense_layout(d)
    data, indices, indptr = data.contiguous(), indices.contiguous(), indptr.contiguous()
    h = _handle_on(dev)
    va = _view(m, n, nnz, indptr, indices, data, dt)
    vd = _dense_view(d, *layout)
    check(h.lib.spg_csr_mul_dense(h.ptr, ctypes.byref(va), ctypes.byref(vd), ctypes.c_void_p(out.data_ptr())),
          "spg_csr_mul_dense")
    return out


def multiply_by_dense(a, d):
    """Element-wise ``A.multiply(d)`` for a CSR matrix and a dense operand that broadcasts to its
    shape -- cupyx's ``multiply_by_dense`` (modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:617-718),
    on ``spg_csr_mul_dense``.  ``d`` is a 2-D tensor (or numpy array, uploaded) of shape (m, n),
    (1, n), (m, 1) or (1, 1).  Every stored entry is kept, products that are zero included: the
    result is a csr_matrix on copies of A's structure, which need not be canonical."""
    if not (check_availability("csrgeam2") and has_elementwise()):   # a device, and a library with the entry points
        raise RuntimeError("multiply_by_dense is not available.")
    _check_type(a, csr_matrix)
    if not isinstance(d, (torch.Tensor, np.ndarray)):
        raise TypeError("unsupported type (actual: {})".format(type(d)))
    if not isinstance(d, torch.Tensor):
        d = torch.from_numpy(np.asarray(d))
    if d.ndim != 2 or d.shape[0] not in (a.shape[0], 1) or d.shape[1] not in (a.shape[1], 1):
        raise ValueError("inconsistent shapes")
    _check_device(a, "multiply_by_dense")
    a = _promoted("multiply_by_dense", a, d.dtype)
    d = d.to(device=a.device, dtype=a.data.dtype)
    data = _mul_dense_arrays(a.data, a.indices, a.indptr, a.shape, d)
    return csr_matrix._from_parts(data, a.indices.clone(), a.indptr.clone(), a.shape, canonical=a._canonical)


def _canonicalize_arrays(data, indices, indptr, coo_rows, shape, ops: int, indptr_dtype=None):
    """(data, indices, indptr) of the m x n matrix after ``ops`` (a sum of the SPG_CANON_* bits),
    on spg_canonicalize_nnz + spg_canonicalize.  The input is CSR (``coo_rows`` None) or COO
    (``coo_rows`` the int32 row of every entry, ``indptr`` None).  The row pointer comes back as
    ``indptr_dtype``, by default int32 whenever the stored entries fit."""
    dev, dt = data.device, data.dtype
    m, n = int(shape[0]), int(shape[1])
    nnz = int(data.numel())
    ipd = _indptr_dtype(nnz)
    cpd = indptr_dtype or ipd
    if nnz == 0:
        return (torch.empty(0, dtype=dt, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.zeros(m + 1, dtype=cpd, device=dev))
    h = _handle_on(dev)
    data, indices = data.contiguous(), indices.to(torch.int32).contiguous()
    if coo_rows is not None:
        coo_rows, indptr = coo_rows.to(torch.int32).contiguous(), None
    else:
        indptr = indptr.to(ipd).contiguous()
    va = _view(m, n, nnz, indptr, indices, data, dt, ipd)
    rows_p = ctypes.c_void_p(coo_rows.data_ptr()) if coo_rows is not None else None
    args = (ctypes.byref(va), rows_p, ops)
    # one row-pointer type, the caller's: an OVERFLOW raises
    return _two_phase(h, ("spg_canonicalize_nnz", "spg_canonicalize"), args, args, m, n, dt, (cpd,), dev)


def canonicalize(x, sort=True, sum_duplicates=True, eliminate_zeros=False):
    """A new ``csr_matrix`` from a ``csr_matrix`` or ``coo_matrix``: its entries grouped by row
    (COO input, always), sorted by column inside each row, stably (``sort``), duplicates summed
    one by one in stored order (``sum_duplicates``, implies ``sort``) and exact zeros dropped
    afterwards (``eliminate_zeros``) -- what cupyx spreads over ``csrsort`` / ``coosort`` /
    ``coo2csr`` (modify_src/cupy-src/cupyx/cusparse.py:832-984), ``sum_duplicates`` and
    ``eliminate_zeros``, in one pass over ``spg_canonicalize_nnz`` + ``spg_canonicalize``.  The
    result is flagged canonical when duplicates were summed."""
    _guard("canonicalize", x, (csr_matrix, coo_matrix))
    ops = ((_lib.SPG_CANON_SORT if sort else 0) | (_lib.SPG_CANON_SUM if sum_duplicates else 0) |
           (_lib.SPG_CANON_DROP_ZEROS if eliminate_zeros else 0))
    if isinstance(x, coo_matrix):
        parts = _canonicalize_arrays(x.data, x.col, None, x.row, x.shape, ops)
        was = None
    elif ops == 0:   # a CSR matrix with nothing to do
        return x.copy()
    else:
        parts = _canonicalize_arrays(x.data, x.indices, x.indptr, None, x.shape, ops)
        was = x._canonical
    return csr_matrix._from_parts(*parts, x.shape, canonical=True if sum_duplicates or was is True else None)


def csrsort(x):
    """Sorts the indices of every row of ``x`` in place, stably, duplicates kept -- the drop-in
    for ``cupyx.cusparse.csrsort`` (modify_src/cupy-src/cupyx/cusparse.py:832-867), on
    ``spg_canonicalize`` with SPG_CANON_SORT."""
    _guard("csrsort", x, csr_matrix)
    if x._canonical is True:
        return
    x.data, x.indices, _ = _canonicalize_arrays(x.data, x.indices, x.indptr, None, x.shape, _lib.SPG_CANON_SORT,
                                                x.indptr.dtype)
    x._canonical = None   # sorted now; canonical when it holds no duplicates


def _sel_view(sel):
    """(pointer to the spg_sel_t of a selection, what keeps its memory alive): ``None`` the whole
    axis, ``(start, step, count)`` a range, a device tensor a list."""
    if sel is None:
        return None, None
    if isinstance(sel, tuple):
        v = _lib.SpgSel(int(sel[0]), int(sel[1]), int(sel[2]), None)
        return ctypes.byref(v), v
    idx = sel.to(torch.int32).contiguous()
    v = _lib.SpgSel(0, 1, int(idx.numel()), idx.data_ptr() if idx.numel() else None)
    return ctypes.byref(v), (v, idx)


def _extract_arrays(data, indices, indptr, shape, rows_sel, cols_sel):
    """(data, indices, indptr) of the submatrix [rows_sel, cols_sel] of the m x n CSR arrays, on
    spg_csr_extract_nnz + spg_csr_extract.  A selection is ``None`` (the whole axis), a range
    ``(start, step, count)`` or a device tensor of in-range int32 indices.  The row pointer comes
    back int32, or int64 when nnz(C) does not fit (the structure call is then repeated)."""
    dev, dt = data.device, data.dtype
    m, n = int(shape[0]), int(shape[1])
    nnz = int(data.numel())
    ipd = _indptr_dtype(nnz)
    h = _handle_on(dev)
    data, indices, indptr = data.contiguous(), indices.to(torch.int32).contiguous(), indptr.to(ipd).contiguous()
    va = _view(m, n, nnz, indptr, indices, data, dt)
    rp, rkeep = _sel_view(rows_sel)   # (rkeep, ckeep: the selections' memory, held until the return)
    cp, ckeep = _sel_view(cols_sel)
    nr = m if rows_sel is None else rows_sel[2] if isinstance(rows_sel, tuple) else int(rows_sel.numel())
    nc = n if cols_sel is None else cols_sel[2] if isinstance(cols_sel, tuple) else int(cols_sel.numel())
    args = (ctypes.byref(va), rp, cp)
    return _two_phase(h, ("spg_csr_extract_nnz", "spg_csr_extract"), args, args, nr, nc, dt,
                      (torch.int32, torch.int64), dev)


def extract(x, rows=None, cols=None):
    """The submatrix ``x[rows, cols]`` of a ``csr_matrix`` or ``csc_matrix`` in its own format --
    what cupyx's ``__getitem__`` does with kernels of its own
    (modify_src/cupy-src/cupyx/scipy/sparse/_index.py:348, :45-115; _compressed.py:403, :566, :643,
    :665), on ``spg_csr_extract_nnz`` + ``spg_csr_extract``.  Per axis: ``None`` (everything), a
    ``slice`` with any step, or an int sequence / array / tensor in any order, repeats allowed --
    always one selection per axis (outer indexing), also when both are lists.  Rows keep their
    stored entry order and values are moved bit for bit; the arrays equal scipy's array for array
    wherever the column list has no repeat (repeats come in ascending list position)."""
    _guard("extract", x, (csr_matrix, csc_matrix))
    m, n = x.shape
    return x._extract(_axis_selector(rows, m, x.device), _axis_selector(cols, n, x.device))


def _new_dense(m: int, n: int, dtype, dev, order: str) -> torch.Tensor:
    if order not in ("C", "F"):
        raise ValueError("order must be 'C' or 'F'")
    return torch.empty((m, n), dtype=dtype, device=dev) if order == "C" \
        else torch.empty((n, m), dtype=dtype, device=dev).t()


def _check_out(out, m: int, n: int, dtype, dev) -> torch.Tensor:
    if not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch tensor")
    if out.ndim != 2 or tuple(out.shape) != (m, n):
        raise ValueError("out must have the matrix's shape")
    if out.dtype != dtype or out.device != dev:
        raise TypeError("out must be a tensor of the matrix's type on its device")
    if _dense_layout(out) is None:
        raise ValueError("out must have unit stride along its rows or its columns")
    return out


def _todense_into(data, indices, indptr, rows: int, cols: int, view: torch.Tensor) -> None:
    """spg_csr2dense of the rows x cols CSR arrays into `view` (rows x cols, a layout
    _dense_layout accepts); every element of the extent is written, no padding touched."""
    if rows == 0 or cols == 0:
        return
    nnz = int(data.numel())
    h = _handle_on(data.device)
    ipd = indptr.dtype if indptr.dtype in _IT else torch.int64
    if ipd == torch.int32 and nnz > 2 ** 31 - 1:
        ipd = torch.int64
    indptr, indices, data = indptr.to(ipd).contiguous(), indices.to(torch.int32).contiguous(), data.contiguous()
    va = _view(rows, cols, nnz, indptr, indices, data, data.dtype)
    vd = _dense_view(view, *_dense_layout(view))
    check(h.lib.spg_csr2dense(h.ptr, ctypes.byref(va), ctypes.byref(vd)), "spg_csr2dense")


def _compressed2dense(x, kind, name: str, out, order: str) -> torch.Tensor:
    _guard(name, x, kind)
    m, n = x.shape
    out = _new_dense(m, n, x.data.dtype, x.device, order) if out is None else \
        _check_out(out, m, n, x.data.dtype, x.device)
    if kind is csr_matrix:
        _todense_into(x.data, x.indices, x.indptr, m, n, out)
    else:   # the CSC arrays are the CSR of the transpose: the same kernel on the swapped view
        _todense_into(x.data, x.indices, x.indptr, n, m, out.t())
    return out


def csr2dense(x, out=None, order="C"):
    """The CSR matrix ``x`` as a dense 2-D tensor on its device -- the drop-in for
    ``cupyx.cusparse.csr2dense`` (modify_src/cupy-src/cupyx/cusparse.py:768-797), on
    ``spg_csr2dense``.  ``x`` need not be canonical: every element is 0 + v1 + v2 + ... over its
    stored entries in stored order, so the result equals scipy's ``toarray()`` bit for bit and is
    the same from run to run.  ``out`` may be any row- or column-major view with a leading
    dimension (only the extent is written); without it the result is ``order`` 'C' or 'F'."""
    return _compressed2dense(x, csr_matrix, "csr2dense", out, order)


def csc2dense(x, out=None, order="C"):
    """The CSC matrix ``x`` as a dense 2-D tensor -- the drop-in for ``cupyx.cusparse.csc2dense``
    (modify_src/cupy-src/cupyx/cusparse.py:800-829): ``spg_csr2dense`` on the CSC arrays read as
    the CSR of the transpose, into the transposed view of the result; no transpose is made."""
    return _compressed2dense(x, csc_matrix, "csc2dense", out, order)


def sparseToDense(x, out=None):
    """A csr_matrix, csc_matrix or coo_matrix as a dense 2-D tensor -- the drop-in for
    ``cupyx.cusparse.sparseToDense`` (modify_src/cupy-src/cupyx/cusparse.py:1805-1833).  COO
    entries are grouped by row first, stably (spg_canonicalize with no op), so duplicates are
    still added in stored order."""
    _guard("sparseToDense")
    if isinstance(x, csr_matrix):
        return csr2dense(x, out=out)
    if isinstance(x, csc_matrix):
        return csc2dense(x, out=out)
    _check_type(x, coo_matrix)
    _check_device(x, "sparseToDense")
    m, n = x.shape
    out = _new_dense(m, n, x.data.dtype, x.device, "C") if out is None else \
        _check_out(out, m, n, x.data.dtype, x.device)
    _todense_into(*_canonicalize_arrays(x.data, x.col, None, x.row, x.shape, 0), m, n, out)
    return out


def _dense2csr_arrays(t: torch.Tensor):
    """(data, indices, indptr) of the canonical CSR form of the 2-D device tensor ``t`` (any
    strides), on spg_dense2csr_nnz + spg_dense2csr.  int32 indptr unless nnz needs int64."""
    dev, dt = t.device, t.dtype
    m, n = int(t.shape[0]), int(t.shape[1])
    lay = _dense_layout(t)
    if lay is None:
        t = t.contiguous()
        lay = _dense_layout(t)
    h = _handle_on(dev)
    vd = (ctypes.byref(_dense_view(t, *lay)),)
    return _two_phase(h, ("spg_dense2csr_nnz", "spg_dense2csr"), vd, vd, m, n, dt, (torch.int32, torch.int64), dev)


def _check_dense_operand(x, name: str) -> torch.Tensor:
    _guard(name)
    _check_type(x, torch.Tensor)
    if x.ndim != 2:
        raise ValueError("expected a 2-D tensor")
    if x.dtype not in _VT:
        raise TypeError(f"{name} supports float32/float64/complex64/complex128, got {x.dtype}")
    _check_device(x, name)
    return x


def dense2csr(x):
    """The 2-D device tensor ``x`` as a canonical csr_matrix -- the drop-in for
    ``cupyx.cusparse.dense2csr`` (modify_src/cupy-src/cupyx/cusparse.py:1188-1228), on
    ``spg_dense2csr_nnz`` + ``spg_dense2csr``.  An element is kept iff it is != 0 (+-0 dropped;
    denormals, +-inf and NaN kept) and moved bit for bit: scipy's ``csr_matrix(x)`` array for
    array.  Row-major and column-major strides are read as they are, anything else is copied."""
    x = _check_dense_operand(x, "dense2csr")
    return csr_matrix._from_parts(*_dense2csr_arrays(x), x.shape, canonical=True)


def dense2csc(x):
    """The 2-D device tensor ``x`` as a canonical csc_matrix -- the drop-in for
    ``cupyx.cusparse.dense2csc`` (modify_src/cupy-src/cupyx/cusparse.py:1146-1185): the CSR
    conversion of the transposed view, which moves no data."""
    x = _check_dense_operand(x, "dense2csc")
    return csc_matrix(_dense2csr_arrays(x.t()), shape=x.shape, canonical=True)


def denseToSparse(x, format="csr"):
    """``x`` as a csr_matrix, csc_matrix or coo_matrix -- the drop-in for
    ``cupyx.cusparse.denseToSparse`` (modify_src/cupy-src/cupyx/cusparse.py:1733-1802)."""
    if format == "csr":
        return dense2csr(x)
    if format == "csc":
        return dense2csc(x)
    if format != "coo":
        raise TypeError("unsupported format (actual: {})".format(format))
    c = dense2csr(_check_dense_operand(x, "denseToSparse"))
    return coo_matrix((c.data, (c._row_ids(), c.indices.to(torch.int64))), shape=c.shape)


def num_products(a: csr_matrix, b: csr_matrix) -> int:
    """P = number of scalar products of A.B (cusparseSpGEMM_getNumProducts); GFLOPS = 2P/t."""
    h = _handle_for(a)
    with _planned(h, a, b, _lib.SPG_ALG2, 0.2) as (plan, _):
        p = ctypes.c_int64(0)
        check(h.lib.spg_num_products(h.ptr, plan, ctypes.byref(p)), "spg_num_products")
        return int(p.value)


def plan_info(a: csr_matrix, b: csr_matrix, alg: int = 0, chunk_fraction: float = 0.2) -> dict:
    """What spgemm(a, b, alg, chunk_fraction) runs (spg_plan_info): the kernel path, the
    tile geometry and the row chunks (ALG3's chunk cut).  A diagnostic for tests/profilers."""
    h = _handle_for(a)
    with contextlib.ExitStack() as after, \
            _planned(h, a, b, _ALG.get(alg, _lib.SPG_ALG_DEFAULT), float(chunk_fraction)) as (plan, _):
        # (once there is a plan: the stream is synchronised after the plan is destroyed)
        after.callback(lambda: torch.cuda.current_stream(a.device).synchronize())
        info = _lib.SpgPlanInfo()
        check(h.lib.spg_plan_info(plan, ctypes.byref(info), None, 0), "spg_plan_info")
        rows = (ctypes.c_int64 * (info.n_chunks + 1))()
        check(h.lib.spg_plan_info(plan, ctypes.byref(info), rows, info.n_chunks + 1), "spg_plan_info")
        return {"path": ("general", "short", "tile")[info.path], "tile_width": info.tile_width,
                "tiles_per_row": info.tiles_per_row, "dense_tiles": bool(info.dense_tiles),
                "lds_ordered": bool(info.lds_ordered), "record_group": int(info.record_group),
                "chunk_rows": [int(x) for x in rows]}


__all__ = ["spgemm", "spmv", "spmm", "csr2csc", "csc2csr", "csrgeam2", "csrgeam", "canonicalize", "csrsort",
           "extract", "check_availability", "num_products", "validate_csr", "SpgError",
           "last_stats"]
