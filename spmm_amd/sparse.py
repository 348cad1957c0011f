"""Device-resident sparse containers for the SpGEMM path (torch tensors in HBM).

Mirrors the part of ``cupyx.scipy.sparse`` that the reference's hot path goes through:

* ``csr_matrix`` with int32 ``indices``, int32 (or int64 when nnz >= 2**31) ``indptr`` and
  f32/f64 ``data`` (modify_src/cupy-src/cupyx/scipy/sparse/_compressed.py:229-230,286-287
  force int32; int64 is added so configs with nnz >= 2**31 are representable);
* ``A @ B`` dispatch: ``__matmul__`` -> ``__mul__`` -> ``sum_duplicates()`` on both operands
  -> ``spgemm`` (_base.py:130-134, _csr.py:151-166); a dense right operand goes to ``spmv``
  (1-D, _csr.py:190-216) or ``spmm`` (2-D, _csr.py:217-225);
* ``has_canonical_format`` evaluated on the device (the reference's
  ``_has_canonical_format_kern``, _compressed.py:177-192, here ``spg_validate_csr``);
* ``csc_matrix`` / ``coo_matrix`` operands of ``@`` are converted to CSR first
  (_csr.py:167-184);
* ``csr_matrix.tocsc()`` / ``.transpose()`` / ``.T`` (_csr.py:512-533) and
  ``csc_matrix((data, indices, indptr), shape=...)``;
* ``A + B``, ``A - B`` and ``-A`` (``_add``, _compressed.py:321-360; ``_add_sparse``,
  _csr.py:84-96 and _csc.py:250-262): ``sum_duplicates()`` on both operands, then
  ``cusparse.csrgeam2`` (``spg_csrgeam``) for device tensors and the torch form of the same
  rule otherwise; a csc result for csc operands, through the free transposes.
* ``A[rows, cols]`` on ``csr_matrix`` / ``csc_matrix`` (``__getitem__``, _index.py:348;
  _compressed.py:403, :566, :643, :665): ints, slices with any step, index arrays (outer
  indexing) and boolean masks per axis, on ``spg_csr_extract`` for device tensors and the torch
  form of the same rule otherwise.

CSR <-> CSC conversion of device tensors runs in libmi355_spgemm.so (``spg_csr2csc``, a stable
counting sort: scipy's own order, so transposed products stay bit-exact with scipy), and so do
``sum_duplicates()``, ``eliminate_zeros()`` and ``coo_matrix.tocsr()`` (``spg_canonicalize``: a
stable sort by (row, column), duplicates added one by one in stored order).  For tensors that are
not on a GPU all of these run as torch ops with the same results.  The multiply itself runs only
in the library.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
             np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128,
             np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}
_NP_OF = {v: k for k, v in _TORCH_OF.items()}

INT32_MAX = 2 ** 31 - 1


def _indptr_dtype(nnz: int) -> torch.dtype:
    """int32 row pointers while the entry count fits (CuPy's type), int64 beyond."""
    return torch.int32 if nnz <= INT32_MAX else torch.int64


def _as_tensor(x, dtype: torch.dtype, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")


def _engine_has(t: torch.Tensor, symbols, extent: int = 0) -> bool:
    """An operation on these tensors runs in the engine: they sit on a GPU, `extent` (where the
    engine keeps that axis in int32 ids) fits, and the loaded library exports the operation's
    symbols (otherwise the torch form of the same rule serves)."""
    return t.device.type == "cuda" and extent <= INT32_MAX and _lib.exports(*symbols)


def _stable_by_index(data, indices, indptr, n_major: int, n_minor: int):
    """The torch form of scipy's csr_tocsc: the (data, indices, indptr) of the other
    compressed format, every output segment in stored entry order, duplicates kept."""
    counts = (indptr[1:] - indptr[:-1]).to(torch.int64)
    major = torch.repeat_interleave(torch.arange(n_major, device=data.device), counts)
    _, order = torch.sort(indices.to(torch.int64), stable=True)
    ipd = torch.int32 if data.numel() <= INT32_MAX else torch.int64
    return (data[order].contiguous(), major[order].to(torch.int32),
            _indptr_from_rows(indices.to(torch.int64), n_minor, ipd))


_VALUE_TYPES = (torch.float32, torch.float64, torch.complex64, torch.complex128)


def _dense_operand(x, dtype, device) -> torch.Tensor:
    """The 2-D tensor a container is built from: a torch tensor or a numpy array, cast to
    ``dtype`` when given and moved to ``device`` (a numpy array: the default device)."""
    if x.ndim != 2:
        raise ValueError("expected a 2-D array")
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(x if x.flags.writeable else x.copy())   # (F-ordered arrays keep their strides)
        device = device or _default_device()
    else:
        t = x
        device = device or x.device
    if dtype is not None:
        t = t.to(_TORCH_OF[np.dtype(dtype)])
    if t.dtype not in _VALUE_TYPES:
        raise TypeError(f"unsupported dtype {t.dtype}")
    return t.to(device)


def _dense_to_csr(t: torch.Tensor):
    """(data, indices, indptr) of scipy's csr_matrix(t) for a 2-D tensor: spg_dense2csr's rule
    (include/spgemm.h) -- an element is kept iff its bits without the sign(s) are nonzero, kept
    values are copied, columns ascend.  The engine for device tensors, torch ops otherwise."""
    if _engine_has(t, _lib.DENSE_CONVERT):
        from . import cusparse
        return cusparse._dense2csr_arrays(t)
    m = int(t.shape[0])
    parts = torch.view_as_real(t) if t.is_complex() else t
    bits = parts.contiguous().view(torch.int32 if parts.dtype == torch.float32 else torch.int64)
    keep = (bits & (0x7FFFFFFF if parts.dtype == torch.float32 else 0x7FFFFFFFFFFFFFFF)) != 0
    if t.is_complex():
        keep = keep.any(dim=-1)
    nz = keep.nonzero()   # row-major: rows ascend, columns ascend inside a row
    rows, cols = nz[:, 0], nz[:, 1]
    ipd = _indptr_dtype(rows.numel())
    return t[rows, cols].contiguous(), cols.to(torch.int32), _indptr_from_rows(rows, m, ipd)


def _compressed_to_dense(data, indices, indptr, n_major: int, n_minor: int) -> torch.Tensor:
    """The n_major x n_minor row-major dense form of compressed arrays as torch ops --
    spg_csr2dense's rule (include/spgemm.h): every element is 0 + v1 + v2 + ... over its stored
    entries in stored order, each add rounded on its own, complex values part by part."""
    parts = torch.view_as_real(data) if data.is_complex() else data
    flat = torch.zeros((n_major * n_minor,) + tuple(parts.shape[1:]), dtype=parts.dtype, device=data.device)
    if data.numel():
        counts = (indptr[1:] - indptr[:-1]).to(torch.int64)
        major = torch.repeat_interleave(torch.arange(n_major, device=data.device), counts)
        key_s, order = torch.sort(major * max(n_minor, 1) + indices.to(torch.int64), stable=True)
        uniq, runs = torch.unique_consecutive(key_s, return_counts=True)
        vals = parts[order].clone()
        starts = torch.zeros(runs.numel(), dtype=torch.int64, device=data.device)
        starts[1:] = torch.cumsum(runs, 0)[:-1]
        vals[starts] = torch.zeros_like(vals[starts]) + vals[starts]   # the sum starts from +0
        flat[uniq] = _segmented_sequential_sum(vals, runs)
    flat = flat.reshape((n_major, n_minor) + tuple(parts.shape[1:]))
    return torch.view_as_complex(flat) if data.is_complex() else flat


def _ordered(dense: torch.Tensor, order, out):
    """A row-major result in the asked order ('C', 'F' or None), or copied into ``out``."""
    if order not in (None, "C", "F"):
        raise ValueError("order must be 'C' or 'F'")
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor")
        if tuple(out.shape) != tuple(dense.shape):
            raise ValueError("out must have the matrix's shape")
        if out.dtype != dense.dtype or out.device != dense.device:
            raise TypeError("out must be a tensor of the matrix's type on its device")
        out.copy_(dense)
        return out
    return dense.t().contiguous().t() if order == "F" else dense.contiguous()


def _negated(x: torch.Tensor) -> torch.Tensor:
    """-x as a flip of every sign bit (torch's complex negative is 0 - x on some paths, which
    leaves a +0.0 part at +0.0)."""
    return torch.view_as_complex(-torch.view_as_real(x)) if x.is_complex() else -x


def _scaled(coef, x: torch.Tensor) -> torch.Tensor:
    """coef == 1 ? x : coef * x with every product and sum rounded on its own.  A complex product
    is spelled out on the real parts, (ac - bd) + (ad + bc)i: torch's own complex multiply may
    fuse them."""
    if coef == 1:
        return x
    if not x.is_complex():
        return x * torch.tensor(float(coef), dtype=x.dtype, device=x.device)
    c = complex(coef)
    xr = torch.view_as_real(x)
    re, im = xr[..., 0], xr[..., 1]
    cr = torch.tensor(c.real, dtype=re.dtype, device=x.device)
    ci = torch.tensor(c.imag, dtype=re.dtype, device=x.device)
    return torch.view_as_complex(torch.stack((cr * re - ci * im, cr * im + ci * re), dim=-1).contiguous())


def _geam_torch(a: "csr_matrix", b: "csr_matrix", alpha, beta) -> "csr_matrix":
    """alpha*A + beta*B of two canonical CSR matrices as torch ops -- spg_csrgeam's rule
    (include/spgemm.h): the union of the two patterns, va + vb where both have the entry, va + 0 or
    0 + vb elsewhere, entries that cancel kept; (1, -1) is the subtraction, a + (-b)."""
    if a.shape != b.shape:
        raise ValueError("inconsistent shapes")
    m, n = a.shape
    dt = _TORCH_OF[np.dtype(np.promote_types(a.dtype, b.dtype))]
    minus = alpha == 1 and beta == -1   # the subtraction A - B: -b by a sign flip, no product
    va, vb = _scaled(alpha, a.data.to(dt)), (_negated(b.data.to(dt)) if minus else _scaled(beta, b.data.to(dt)))
    ka = a._row_ids() * max(n, 1) + a.indices.to(torch.int64)
    kb = b._row_ids() * max(n, 1) + b.indices.to(torch.int64)
    keys = torch.unique(torch.cat((ka, kb)))   # sorted: row-major, columns ascending
    pa, pb = torch.searchsorted(keys, ka), torch.searchsorted(keys, kb)
    # sums on the real parts: torch's complex add is x + (1+0j) * y, and that complex product
    # turns an infinite part of y into a NaN in its other part
    parts = torch.view_as_real if dt.is_complex else (lambda t: t)
    b_at = parts(torch.zeros(keys.numel(), dtype=dt, device=a.device))   # vb; where B has no entry +0,
    if minus:                                                            # or -0 for a - 0
        b_at = -b_at
    b_at[pb] = parts(vb)
    out = b_at + torch.zeros_like(b_at)   # B-only: 0 + vb
    out[pa] = parts(va) + b_at[pa]        # both: va + vb; A-only: va + 0
    data = torch.view_as_complex(out) if dt.is_complex else out
    rows = torch.div(keys, max(n, 1), rounding_mode="floor")
    ipd = torch.int32 if keys.numel() <= INT32_MAX else torch.int64
    return csr_matrix._from_parts(data, (keys - rows * max(n, 1)).to(torch.int32),
                                  _indptr_from_rows(rows, m, ipd), (m, n), canonical=True)


def _mul_rn(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x * y element by element with every product and sum rounded on its own: a complex product
    is (ac - bd) + (ad + bc)i on the real parts (torch's own complex multiply may fuse them)."""
    if not x.is_complex():
        return x * y
    xr, yr = torch.view_as_real(x), torch.view_as_real(y)
    a, b, c, d = xr[..., 0], xr[..., 1], yr[..., 0], yr[..., 1]
    return torch.view_as_complex(torch.stack((a * c - b * d, a * d + b * c), dim=-1).contiguous())


def _nonzero_bits(x: torch.Tensor) -> torch.Tensor:
    """x != 0 decided on the integer bits (spg_dense2csr's test): +-0 false; denormals, +-inf and
    NaN true; a complex value false only when both parts are +-0."""
    parts = torch.view_as_real(x) if x.is_complex() else x
    bits = parts.contiguous().view(torch.int32 if parts.dtype == torch.float32 else torch.int64)
    keep = (bits & (0x7FFFFFFF if parts.dtype == torch.float32 else 0x7FFFFFFFFFFFFFFF)) != 0
    return keep.any(dim=-1) if x.is_complex() else keep


def _less(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x < y; for complex values scipy's lexicographic order, re first."""
    if not x.is_complex():
        return x < y
    xr, yr = torch.view_as_real(x), torch.view_as_real(y)
    return torch.where(xr[..., 0] == yr[..., 0], xr[..., 1] < yr[..., 1], xr[..., 0] < yr[..., 0])


def _select(take_y: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """take_y ? y : x, the chosen operand moved bit for bit."""
    if not x.is_complex():
        return torch.where(take_y, y, x)
    return torch.view_as_complex(torch.where(take_y[..., None], torch.view_as_real(y), torch.view_as_real(x)).contiguous())


_BINOP_NAMES = ("multiply", "maximum", "minimum")


def _binop_torch(a: "csr_matrix", b: "csr_matrix", op: str) -> "csr_matrix":
    """op(A, B) of two canonical CSR matrices as torch ops -- spg_csr_binop's rule
    (include/spgemm.h): over the union of the two patterns r = op(a, b), an operand without the
    entry contributing +0; the entries with r != 0 (on the bits) are kept.  multiply: a * b;
    maximum: a < b ? b : a; minimum: b < a ? b : a."""
    if op not in _BINOP_NAMES:
        raise ValueError(f"op must be one of {', '.join(_BINOP_NAMES)} (actual: {op!r})")
    if a.shape != b.shape:
        raise ValueError("inconsistent shapes")
    m, n = a.shape
    dt = _TORCH_OF[np.dtype(np.promote_types(a.dtype, b.dtype))]
    ka = a._row_ids() * max(n, 1) + a.indices.to(torch.int64)
    kb = b._row_ids() * max(n, 1) + b.indices.to(torch.int64)
    keys = torch.unique(torch.cat((ka, kb)))   # sorted: row-major, columns ascending
    a_at = torch.zeros(keys.numel(), dtype=dt, device=a.device)
    b_at = torch.zeros(keys.numel(), dtype=dt, device=a.device)
    a_at[torch.searchsorted(keys, ka)] = a.data.to(dt)
    b_at[torch.searchsorted(keys, kb)] = b.data.to(dt)
    if op == "multiply":
        r = _mul_rn(a_at, b_at)
    elif op == "maximum":
        r = _select(_less(a_at, b_at), a_at, b_at)
    else:
        r = _select(_less(b_at, a_at), a_at, b_at)
    keep = _nonzero_bits(r)
    keys, r = keys[keep], r[keep].contiguous()
    rows = torch.div(keys, max(n, 1), rounding_mode="floor")
    ipd = _indptr_dtype(keys.numel())
    return csr_matrix._from_parts(r, (keys - rows * max(n, 1)).to(torch.int32),
                                  _indptr_from_rows(rows, m, ipd), (m, n), canonical=True)


def _mul_dense_torch(data, indices, indptr, n_major: int, d: torch.Tensor) -> torch.Tensor:
    """data[e] * d[i, j] for every stored entry e = (i, j) of compressed arrays as torch ops --
    spg_csr_mul_dense's rule: d has n_major or 1 rows and n_minor or 1 columns, an extent of 1 is
    broadcast."""
    counts = (indptr[1:] - indptr[:-1]).to(torch.int64)
    major = torch.repeat_interleave(torch.arange(n_major, device=data.device), counts)
    minor = indices.to(torch.int64)
    i = major if d.shape[0] > 1 else torch.zeros_like(major)
    j = minor if d.shape[1] > 1 else torch.zeros_like(minor)
    return _mul_rn(data, d[i, j])


def _is_scalar(x) -> bool:
    """A Python or numpy number, or a 0-d array or tensor."""
    return isinstance(x, (int, float, complex, np.number, np.bool_)) or (
        isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim == 0)


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _axis_selector(key, extent: int, device):
    """One axis of an indexing key as the selection spg_csr_extract takes: ``None`` (the whole
    axis), a range ``(start, step, count)``, or a 1-D int32 tensor of in-range indices on
    ``device``.  Slices are normalised as Python does, negative indices wrapped, boolean masks
    converted with ``torch.nonzero``; bounds are checked on the device with one min / max read.
    ``IndexError`` as scipy raises it."""
    if key is None or key is Ellipsis:
        return None
    if isinstance(key, slice):
        start, stop, step = key.indices(extent)
        count = len(range(start, stop, step))
        if count == extent and (step == 1 or extent <= 1):
            return None
        return (start if count else 0, step if count > 1 else 1, count)
    if _is_int(key):
        i = int(key)
        if i < -extent or i >= extent:
            raise IndexError(f"index ({i}) out of range")
        return (i + extent if i < 0 else i, 1, 1)
    if isinstance(key, torch.Tensor):
        idx = key
    else:
        try:
            idx = torch.from_numpy(np.ascontiguousarray(np.asarray(key)))
        except TypeError:
            raise IndexError("arrays used as indices must be of integer (or boolean) type") from None
    if idx.ndim == 2 and 1 in idx.shape and idx.dtype != torch.bool:   # an np.ix_-shaped key
        idx = idx.reshape(-1)
    if idx.ndim != 1:
        raise IndexError("an index array must be one-dimensional (or np.ix_-shaped)")
    idx = idx.to(device)
    if idx.dtype == torch.bool:
        if idx.numel() != extent:
            raise IndexError(f"boolean index has {idx.numel()} entries, the axis {extent}")
        return torch.nonzero(idx).reshape(-1).to(torch.int32)
    if idx.numel() == 0:
        return torch.empty(0, dtype=torch.int32, device=device)
    if idx.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise IndexError("arrays used as indices must be of integer (or boolean) type")
    idx = idx.to(torch.int64)
    lo, hi = (int(v) for v in torch.aminmax(idx))
    if lo < -extent or hi >= extent:
        raise IndexError(f"index ({lo if lo < -extent else hi}) out of range")
    if lo < 0:
        idx = torch.where(idx < 0, idx + extent, idx)
    return idx.to(torch.int32).contiguous()


def _selector_count(sel, extent: int) -> int:
    return extent if sel is None else sel[2] if isinstance(sel, tuple) else int(sel.numel())


def _extract_torch(data, indices, indptr, n_major: int, n_minor: int, major_sel, minor_sel):
    """(data, indices, indptr) of the submatrix as torch ops -- spg_csr_extract's rule
    (include/spgemm.h): output segment i is source segment sel(i) in stored order; an entry with
    minor index j stays as j (the whole axis), becomes (j - start) / step where the range holds it,
    or one entry per position of j in the list, positions ascending (a stable sort of the list)."""
    dev = data.device
    ip = indptr.to(torch.int64)
    if major_sel is None:
        r = torch.arange(n_major, device=dev)
    elif isinstance(major_sel, tuple):
        r = major_sel[0] + major_sel[1] * torch.arange(major_sel[2], device=dev)
    else:
        r = major_sel.to(torch.int64)
    nr = int(r.numel())
    starts = ip[r]
    lens = ip[r + 1] - starts
    seg = torch.repeat_interleave(torch.arange(nr, device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    e = starts[seg] + (torch.arange(seg.numel(), device=dev) - first[seg])
    j = indices[e].to(torch.int64)
    if minor_sel is None:
        minor = j
    elif isinstance(minor_sel, tuple):
        start, step, count = minor_sel
        d = j - start
        t = torch.div(d, step, rounding_mode="trunc")
        ok = (t * step == d) & (t >= 0) & (t < count)
        e, seg, minor = e[ok], seg[ok], t[ok]
    else:
        idx = minor_sel.to(torch.int64)
        _, colpos = torch.sort(idx, stable=True)   # positions grouped by listed index, ascending inside one
        colptr = torch.zeros(n_minor + 1, dtype=torch.int64, device=dev)
        if idx.numel():
            colptr[1:] = torch.cumsum(torch.bincount(idx, minlength=n_minor), 0)
        mult = colptr[j + 1] - colptr[j]
        src = torch.repeat_interleave(torch.arange(j.numel(), device=dev), mult)
        u = torch.arange(src.numel(), device=dev) - (torch.cumsum(mult, 0) - mult)[src]
        minor = colpos[colptr[j[src]] + u]
        e, seg = e[src], seg[src]
    ipd = torch.int32 if e.numel() <= INT32_MAX else torch.int64
    return data[e].contiguous(), minor.to(torch.int32), _indptr_from_rows(seg, nr, ipd)


def _validate_torch(indptr, indices, nnz: int, n_minor: int) -> int:
    """spg_validate_csr's verdict (include/spgemm.h) as torch ops, for tensors the engine does not
    serve: -1 when a segment has a start below 0, an end before its start or an end past ``nnz``,
    or when an index one of the segments reads is outside [0, n_minor); else 0 when two
    neighbouring entries of one segment do not ascend strictly; else 1."""
    ip = indptr.to(torch.int64)
    p0, p1 = ip[:-1], ip[1:]
    if p0.numel() == 0:
        return 1
    if bool(((p0 < 0) | (p1 < p0) | (p1 > nnz)).any()):
        return -1
    first = int(ip[0])   # (well-formed segments follow one another: they read [ip[0], ip[-1]))
    j = indices[first:int(ip[-1])].to(torch.int64)
    if j.numel() == 0:
        return 1
    if bool(((j < 0) | (j >= n_minor)).any()):
        return -1
    seg = torch.repeat_interleave(torch.arange(p0.numel(), device=ip.device), p1 - p0)
    return 0 if bool(((j[1:] <= j[:-1]) & (seg[1:] == seg[:-1])).any()) else 1


def _extract_compressed(data, indices, indptr, n_major: int, n_minor: int, major_sel, minor_sel, canonical):
    """The selected major segments and minor indices of compressed arrays, with the canonical
    flag of the result: ``True`` when the source's is and the minor axis is kept or cut by an
    ascending range, else unknown (``None``: checked lazily) -- a list or a descending range
    reorders a segment, and any selection may leave out what made the source non-canonical."""
    if _engine_has(data, _lib.EXTRACT, n_minor):
        from . import cusparse
        parts = cusparse._extract_arrays(data, indices, indptr, (n_major, n_minor), major_sel, minor_sel)
    else:
        parts = _extract_torch(data, indices, indptr, n_major, n_minor, major_sel, minor_sel)
    keeps = minor_sel is None or (isinstance(minor_sel, tuple) and minor_sel[1] > 0)
    return parts, (True if keeps and canonical is True else None)


def isspmatrix(x) -> bool:
    return isinstance(x, _SparseBase)


class _SparseBase:
    ndim = 2

    # ------------------------------------------------------------------ addition
    # (cupyx _base.py:104-114, :154-155: every format adds through its CSR form)
    def __add__(self, other):
        return self.tocsr().__add__(other)

    def __radd__(self, other):
        return self.tocsr().__radd__(other)

    def __sub__(self, other):
        return self.tocsr().__sub__(other)

    def __rsub__(self, other):
        return self.tocsr().__rsub__(other)

    def __neg__(self):
        return -self.tocsr()

    # ------------------------------------------------------------------ element-wise operations
    # (cupyx _base.py: every format multiplies, and takes maximum / minimum, through its CSR form)
    def multiply(self, other):
        return self.tocsr().multiply(other)

    def maximum(self, other):
        return self.tocsr().maximum(other)

    def minimum(self, other):
        return self.tocsr().minimum(other)

    def __mul__(self, other):
        return self.tocsr()._scale(other) if _is_scalar(other) else NotImplemented

    __rmul__ = __mul__

    def __truediv__(self, other):
        raise NotImplementedError("division of a sparse matrix is not supported")

    __rtruediv__ = __truediv__

    def _compare(self, other):
        if isspmatrix(other) or _is_dense(other) or _is_scalar(other):
            raise NotImplementedError("comparison of sparse matrices is not supported")
        return NotImplemented

    __eq__ = __ne__ = __lt__ = __le__ = __gt__ = __ge__ = _compare
    __hash__ = object.__hash__

    @property
    def shape(self):
        return self._shape

    @property
    def dtype(self):
        return _NP_OF[self.data.dtype]

    @property
    def nnz(self) -> int:
        return int(self.data.numel())

    @property
    def device(self):
        return self.data.device

    def toarray(self) -> np.ndarray:
        return self.get().toarray()

    def todense(self, order=None, out=None) -> torch.Tensor:
        """The matrix as a dense 2-D tensor on its device (cupyx _csr.py:383-428, _csc.py and
        _coo.py todense): every element is 0 + v1 + v2 + ... over its stored entries in stored
        order, scipy's ``toarray()`` bit for bit.  ``order`` 'C' (the default) or 'F'; ``out`` any
        row- or column-major view of the matrix's shape, type and device.  spg_csr2dense for
        device tensors, else the torch form of the same rule."""
        raise NotImplementedError

    def __matmul__(self, other):
        return self.tocsr().__matmul__(other)


class _Compressed(_SparseBase):
    """What csr_matrix and csc_matrix share: the ``+`` / ``-`` dispatch of cupyx
    _compressed.py:321-360."""

    def _add_sparse(self, other, alpha, beta):
        raise NotImplementedError

    def _add(self, other, lhs_negative, rhs_negative):
        if np.isscalar(other):
            if other == 0:
                if lhs_negative:
                    return -self
                return self.copy()
            raise NotImplementedError("adding a nonzero scalar to a sparse matrix is not supported")
        if isspmatrix(other):
            alpha = -1 if lhs_negative else 1
            beta = -1 if rhs_negative else 1
            return self._add_sparse(other, alpha, beta)
        # (a dense operand: the reference adds self.todense(); dense results are not produced here)
        return NotImplemented

    def __add__(self, other):
        return self._add(other, False, False)

    def __radd__(self, other):
        return self._add(other, False, False)

    def __sub__(self, other):
        return self._add(other, False, True)

    def __rsub__(self, other):
        return self._add(other, True, False)

    def __neg__(self):
        """Elementwise negative over the same structure (cupyx _data.py:36-38)."""
        out = self.copy()
        out.data = _negated(self.data)
        return out

    # ------------------------------------------------------------------ element-wise operations
    def _binop_sparse(self, other, op: str):
        raise NotImplementedError

    def _with_data(self, data):
        """A matrix of this format with ``data`` on copies of this structure, the canonical flag kept."""
        arrays = (data, self.indices.clone(), self.indptr.clone())
        if self.format == "csr":
            return csr_matrix._from_parts(*arrays, self._shape, canonical=self._canonical)
        return csc_matrix(arrays, shape=self._shape, canonical=self._canonical)

    def _scale(self, s):
        """self * s for a scalar (cupyx _data.py _mul_scalar): the structure copied, every value
        multiplied, in the common type of the matrix and the scalar."""
        s = s.item() if isinstance(s, (torch.Tensor, np.ndarray)) else s
        dt = np.result_type(self.dtype, s)
        if np.dtype(dt) not in _TORCH_OF or _TORCH_OF[np.dtype(dt)] not in _VALUE_TYPES:
            raise TypeError(f"unsupported dtype {dt}")
        data = self.data.to(_TORCH_OF[np.dtype(dt)])
        scaled = _scaled(s, data)
        return self._with_data(scaled.clone() if scaled is data else scaled)

    def _mul_dense(self, d):
        """self.multiply(d) for a dense vector or matrix that broadcasts to this shape."""
        m, n = self._shape
        if isinstance(d, np.ndarray):
            d = torch.from_numpy(d if d.flags.writeable else d.copy())
        if d.ndim == 1:
            d = d.reshape(1, -1)   # a 1-D operand is a row vector
        if d.ndim != 2:
            raise ValueError("could not interpret dimensions")
        r, c = int(d.shape[0]), int(d.shape[1])
        if not all(x == y or x == 1 or y == 1 for x, y in ((r, m), (c, n))):
            raise ValueError("inconsistent shapes")
        if r not in (m, 1) or c not in (n, 1):
            raise NotImplementedError("multiply by a dense operand larger than the sparse matrix "
                                      "(broadcasting the sparse operand) is not supported")
        dt = np.promote_types(self.dtype, np.dtype(str(d.dtype).replace("torch.", "")))
        if np.dtype(dt) not in _TORCH_OF or _TORCH_OF[np.dtype(dt)] not in _VALUE_TYPES:
            raise TypeError(f"unsupported dtype {dt}")
        tdt = _TORCH_OF[np.dtype(dt)]
        data, d = self.data.to(tdt), d.to(device=self.device, dtype=tdt)
        csr = self.format == "csr"
        if not csr:   # the CSC arrays are the CSR of the transpose
            d = d.t()
        n_major, n_minor = (m, n) if csr else (n, m)
        if _engine_has(data, _lib.ELEMENTWISE):
            from . import cusparse
            return self._with_data(cusparse._mul_dense_arrays(data, self.indices, self.indptr, (n_major, n_minor), d))
        return self._with_data(_mul_dense_torch(data, self.indices, self.indptr, n_major, d))

    def multiply(self, other):
        """Point-wise multiplication by a scalar, a dense vector or matrix, or a sparse matrix of
        this shape (cupyx _csr.py:328-342): scipy's ``multiply``.  A sparse operand gives the
        canonical matrix of the nonzero products (spg_csr_binop); a dense one, of shape (m, n),
        (1, n), (m, 1), (1, 1) or (n,), scales every stored entry on a copy of this structure
        (spg_csr_mul_dense); a scalar scales the data."""
        if _is_scalar(other):
            return self._scale(other)
        if isspmatrix(other):
            return self._binop_sparse(other, "multiply")
        if _is_dense(other):
            return self._mul_dense(other)
        raise TypeError("expected scalar, dense matrix/vector or csr matrix")

    def _maximum_minimum(self, other, op: str):
        if _is_scalar(other) or _is_dense(other):
            raise NotImplementedError(f"{op} with a scalar or a dense operand is not supported")
        if isspmatrix(other):
            return self._binop_sparse(other, op)
        raise TypeError("expected scalar, dense matrix/vector or csr matrix")

    def maximum(self, other):
        """Element-wise maximum with a sparse matrix of this shape (cupyx _csr.py:297-326): scipy's
        ``maximum``, the entries that come out zero dropped."""
        return self._maximum_minimum(other, "maximum")

    def minimum(self, other):
        """Element-wise minimum with a sparse matrix of this shape: scipy's ``minimum``."""
        return self._maximum_minimum(other, "minimum")

    def __mul__(self, other):
        return self._scale(other) if _is_scalar(other) else NotImplemented

    def __rmul__(self, other):
        return self._scale(other) if _is_scalar(other) else NotImplemented

    # ------------------------------------------------------------------ indexing
    def _extract(self, rows_sel, cols_sel):
        """self[rows, cols] for two selections of ``_axis_selector``'s kind, in this format: a CSC
        matrix is the same extraction on its arrays with the selections swapped."""
        m, n = self._shape
        if rows_sel is None and cols_sel is None:
            return self.copy()
        csr = self.format == "csr"
        n_major, n_minor = (m, n) if csr else (n, m)
        major, minor = (rows_sel, cols_sel) if csr else (cols_sel, rows_sel)
        (data, indices, indptr), canon = _extract_compressed(self.data, self.indices, self.indptr, n_major, n_minor,
                                                              major, minor, self._canonical)
        shape = (_selector_count(rows_sel, m), _selector_count(cols_sel, n))
        if csr:
            return csr_matrix._from_parts(data, indices, indptr, shape, canonical=canon)
        return csc_matrix((data, indices, indptr), shape=shape, canonical=canon)

    def __getitem__(self, key):
        """``A[rows, cols]`` as scipy gives it (cupyx _index.py:348): per axis an int, a slice with
        any step, an integer sequence / array / tensor (negative entries wrapped, any order,
        repeats allowed) or a boolean mask.  Index arrays are read as OUTER indexing, one per axis:
        ``A[rows][:, cols]``, ``A[np.ix_(rows, cols)]``-shaped keys and ``A[rows, c0:c1]`` name the
        same submatrix.  An int gives a 1 x n or m x 1 matrix, ``A[i, j]`` the element (the sum of
        its stored duplicates) as a Python scalar, ``A[:]`` a copy.  Two 1-D index arrays at once
        are scipy's inner (pointwise) indexing, a different operation with a dense result:
        ``NotImplementedError``.  spg_csr_extract for device tensors, else the torch form of the
        same rule."""
        if not isinstance(key, tuple):
            key = (key, slice(None))
        elif len(key) == 1:
            key = (key[0], slice(None))
        elif len(key) != 2:
            raise IndexError("a sparse matrix takes at most two indices")

        def scalar(k):   # 0-d arrays and tensors index like ints
            if isinstance(k, (np.ndarray, torch.Tensor)) and k.ndim == 0 and k.dtype not in (np.bool_, torch.bool):
                return int(k)
            return k

        rk, ck = scalar(key[0]), scalar(key[1])

        def array_ndim(k):
            if isinstance(k, (slice, type(None), type(Ellipsis))) or _is_int(k):
                return None
            return k.ndim if isinstance(k, (np.ndarray, torch.Tensor)) else np.ndim(k)

        if array_ndim(rk) == 1 and array_ndim(ck) == 1:
            if len(rk) != len(ck):
                raise IndexError("shape mismatch: the two index arrays do not broadcast")
            raise NotImplementedError(
                "two index arrays select elements pointwise (scipy's inner indexing), which gives a dense "
                "vector and is another operation; for the submatrix use A[rows][:, cols] or np.ix_(rows, cols)")
        m, n = self._shape
        out = self._extract(_axis_selector(rk, m, self.device), _axis_selector(ck, n, self.device))
        if _is_int(rk) and _is_int(ck):   # (scipy's _get_intXint: duplicates summed)
            return out.data.sum().item()
        return out


class csr_matrix(_Compressed):
    """Compressed sparse row matrix on the device.

    ``csr_matrix(S)``            from a scipy.sparse matrix (uploaded),
    ``csr_matrix((data, indices, indptr), shape=(m, n))`` from arrays / tensors,
    ``csr_matrix((m, n), dtype=...)`` empty matrix.
    """
    format = "csr"

    def __init__(self, arg1, shape=None, dtype=None, device=None, canonical=None):
        device = torch.device(device) if device is not None else None
        if isinstance(arg1, csr_matrix):
            device = device or arg1.device
            self.data = arg1.data.to(device)
            self.indices, self.indptr = arg1.indices.to(device), arg1.indptr.to(device)
            self._shape = arg1.shape
            self._canonical = arg1._canonical
        elif isinstance(arg1, tuple) and len(arg1) == 2 and all(isinstance(s, (int, np.integer)) for s in arg1):
            device = device or _default_device()
            m, n = int(arg1[0]), int(arg1[1])
            dt = _TORCH_OF[np.dtype(dtype or np.float64)]
            self.data = torch.empty(0, dtype=dt, device=device)
            self.indices = torch.empty(0, dtype=torch.int32, device=device)
            self.indptr = torch.zeros(m + 1, dtype=torch.int32, device=device)
            self._shape = (m, n)
            self._canonical = True
        elif isinstance(arg1, tuple) and len(arg1) == 3:
            if shape is None:
                raise ValueError("shape is required for (data, indices, indptr)")
            device = device or (arg1[0].device if isinstance(arg1[0], torch.Tensor) else _default_device())
            data, indices, indptr = arg1
            ddt = np.dtype(dtype) if dtype is not None else (
                _NP_OF[data.dtype] if isinstance(data, torch.Tensor) else np.asarray(data).dtype)
            self.data = _as_tensor(data, _TORCH_OF[np.dtype(ddt)], device)
            self.indices = _as_tensor(indices, torch.int32, device)
            # int32 row pointers whenever they fit (CuPy casts to int32), int64 beyond
            ipd = _indptr_dtype(self.data.numel())
            self.indptr = _as_tensor(indptr, ipd, device)
            self._shape = (int(shape[0]), int(shape[1]))
            self._canonical = canonical
        elif hasattr(arg1, "tocsr"):   # scipy.sparse matrix / array
            device = device or _default_device()
            S = arg1.tocsr()
            if dtype is not None:
                S = S.astype(dtype)
            canon = bool(S.has_canonical_format)
            ipd = _indptr_dtype(S.nnz)
            self.data = _as_tensor(S.data, _TORCH_OF[np.dtype(S.dtype)], device)
            self.indices = _as_tensor(S.indices, torch.int32, device)
            self.indptr = _as_tensor(S.indptr, ipd, device)
            self._shape = tuple(int(s) for s in S.shape)
            self._canonical = canon
        elif isinstance(arg1, (torch.Tensor, np.ndarray)):   # a dense matrix (cupyx _csr.py:60-80)
            t = _dense_operand(arg1, dtype, device)
            self.data, self.indices, self.indptr = _dense_to_csr(t)
            self._shape = (int(t.shape[0]), int(t.shape[1]))
            self._canonical = True
        else:
            raise TypeError(f"unsupported csr_matrix argument {type(arg1)}")
        if self.data.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
            raise TypeError(f"unsupported dtype {self.data.dtype}")
        if self.indptr.numel() != self._shape[0] + 1:
            raise ValueError("indptr length must be rows + 1")

    @classmethod
    def _from_parts(cls, data, indices, indptr, shape, canonical=True):
        """Wrap device tensors as-is (no conversion, no copy) -- the shim's result path."""
        self = cls.__new__(cls)
        self.data, self.indices, self.indptr = data, indices, indptr
        self._shape = (int(shape[0]), int(shape[1]))
        self._canonical = canonical
        return self

    # ------------------------------------------------------------------ structure
    @property
    def has_canonical_format(self) -> bool:
        """indices sorted strictly increasing inside each row (no duplicates).  Evaluated
        on the device with spg_validate_csr and cached, as CuPy caches it; for tensors that are
        not on a GPU, the torch form of the same rule."""
        if self._canonical is None:
            if _engine_has(self.data, ("spg_validate_csr",), self._shape[1]):
                from . import cusparse
                self._canonical = cusparse.validate_csr(self) == 1
            else:
                self._canonical = _validate_torch(self.indptr, self.indices, self.nnz, self._shape[1]) == 1
        return self._canonical

    @has_canonical_format.setter
    def has_canonical_format(self, v: bool):
        self._canonical = bool(v)

    @property
    def has_sorted_indices(self) -> bool:
        return self.has_canonical_format

    def _row_ids(self) -> torch.Tensor:
        counts = (self.indptr[1:] - self.indptr[:-1]).to(torch.int64)
        return torch.repeat_interleave(torch.arange(self._shape[0], device=self.device), counts)

    def sum_duplicates(self) -> None:
        """Sort indices and add up duplicates in place (cupyx _compressed.py:971-991).
        Duplicates are added in stored order, sequentially: spg_canonicalize for device
        tensors, else the torch form of the same rule."""
        if self._canonical is True or (self._canonical is None and self.has_canonical_format):
            return
        m, n = self._shape
        if _engine_has(self.data, _lib.CANONICALIZE, max(self._shape)):
            from . import cusparse
            self.data, self.indices, self.indptr = cusparse._canonicalize_arrays(
                self.data, self.indices, self.indptr, None, self._shape, _lib.SPG_CANON_SUM, self.indptr.dtype)
            self._canonical = True
            return
        rows = self._row_ids()
        key = rows * max(n, 1) + self.indices.to(torch.int64)
        key_s, order = torch.sort(key, stable=True)
        data_s = self.data[order]
        uniq, counts = torch.unique_consecutive(key_s, return_counts=True)
        if uniq.numel() == key_s.numel():
            new_data = data_s
        else:
            new_data = _segmented_sequential_sum(data_s, counts)
        urow = torch.div(uniq, max(n, 1), rounding_mode="floor")
        self.indices = (uniq - urow * max(n, 1)).to(torch.int32)
        self.data = new_data.contiguous()
        self.indptr = _indptr_from_rows(urow, m, self.indptr.dtype)
        self._canonical = True

    def sort_indices(self) -> None:
        """Sort the indices of every row in place, stably, duplicates kept (cupyx
        _compressed.py sort_indices, on csrsort): ``cusparse.csrsort`` for device tensors, else a
        stable torch sort by (row, column).  A matrix flagged canonical is left alone; any other
        is sorted afterwards and canonical when it holds no duplicates (the flag: unknown)."""
        if self._canonical is True:
            return
        if _engine_has(self.data, _lib.CANONICALIZE, max(self._shape)):
            from . import cusparse
            cusparse.csrsort(self)
            return
        key = self._row_ids() * max(self._shape[1], 1) + self.indices.to(torch.int64)
        _, order = torch.sort(key, stable=True)
        self.data, self.indices = self.data[order].contiguous(), self.indices[order].contiguous()
        self._canonical = None

    def eliminate_zeros(self) -> None:
        """Drop the stored entries that equal zero, in place, the stored order kept (cupyx
        _csr.py:288-302): spg_canonicalize for device tensors, else the torch form.  A canonical
        matrix stays canonical; one that was not may have lost the twin of its only duplicate, so
        once an entry is dropped its flag is unknown."""
        before = self.nnz
        if _engine_has(self.data, _lib.CANONICALIZE, max(self._shape)):
            from . import cusparse
            self.data, self.indices, self.indptr = cusparse._canonicalize_arrays(
                self.data, self.indices, self.indptr, None, self._shape, _lib.SPG_CANON_DROP_ZEROS,
                self.indptr.dtype)
        else:
            keep = self.data != 0
            if bool(keep.all()):
                return
            rows = self._row_ids()[keep]
            self.data = self.data[keep].contiguous()
            self.indices = self.indices[keep].contiguous()
            self.indptr = _indptr_from_rows(rows, self._shape[0], self.indptr.dtype)
        if self._canonical is False and self.nnz != before:
            self._canonical = None

    # ------------------------------------------------------------------ conversion
    def astype(self, dtype):
        dt = _TORCH_OF[np.dtype(dtype)]
        if dt == self.data.dtype:
            return self
        out = csr_matrix(self)
        out.data = self.data.to(dt)
        return out

    def copy(self):
        out = csr_matrix(self)
        out.data, out.indices, out.indptr = self.data.clone(), self.indices.clone(), self.indptr.clone()
        return out

    def tocsr(self, copy=False):
        return self.copy() if copy else self

    def todense(self, order=None, out=None) -> torch.Tensor:
        if _engine_has(self.data, _lib.DENSE_CONVERT):
            from . import cusparse
            if order not in (None, "C", "F"):
                raise ValueError("order must be 'C' or 'F'")
            return cusparse.csr2dense(self, out=out, order=order or "C")
        return _ordered(_compressed_to_dense(self.data, self.indices, self.indptr, *self._shape), order, out)

    def get(self):
        """Copy to the host as a scipy.sparse.csr_matrix (cupy's .get())."""
        import scipy.sparse as sp
        return sp.csr_matrix((self.data.cpu().numpy(), self.indices.cpu().numpy(),
                              self.indptr.cpu().numpy()), shape=self._shape)

    # ------------------------------------------------------------------ products
    def __mul__(self, other):
        """CSR x sparse: CuPy's _csr.py:151-166 order -- canonicalise both, then spgemm.
        CSR x dense vector (_csr.py:190-216): canonicalise, then spmv.
        CSR x dense matrix (_csr.py:217-225): canonicalise, then spmm.
        CSR x scalar (_csr.py:153-155): the data scaled."""
        from . import cusparse
        if _is_scalar(other):
            return self._scale(other)
        if isinstance(other, (csc_matrix, coo_matrix)):
            other = other.tocsr()
        if isinstance(other, csr_matrix):
            self.sum_duplicates()
            other.sum_duplicates()
            return cusparse.spgemm(self, other)
        if _is_vector(other):
            self.sum_duplicates()
            return cusparse.spmv(self, other)
        if _is_matrix(other):
            self.sum_duplicates()
            return cusparse.spmm(self, other)
        if _is_dense(other) and other.ndim > 2:
            raise ValueError("could not interpret dimensions")
        return NotImplemented

    def _add_sparse(self, other, alpha, beta):
        """alpha*self + beta*other (cupyx _csr.py:84-96): canonicalise both, then csrgeam2 --
        spg_csrgeam for device tensors, else the torch form of the same rule."""
        self.sum_duplicates()
        other = other.tocsr()
        other.sum_duplicates()
        if _engine_has(self.data, _lib.CSRGEAM) and other.device == self.device:
            from . import cusparse
            return cusparse.csrgeam2(self, other, alpha, beta)
        return _geam_torch(self, other, alpha, beta)

    def _binop_sparse(self, other, op: str):
        """op(self, other) for a sparse operand (cupyx _csr.py:297-342): canonicalise both, then
        spg_csr_binop for device tensors, else the torch form of the same rule."""
        self.sum_duplicates()
        other = other.tocsr()
        other.sum_duplicates()
        if other.shape != self.shape:
            raise NotImplementedError(f"{op} of sparse matrices of different shapes (broadcasting) is not supported")
        if _engine_has(self.data, _lib.ELEMENTWISE) and other.device == self.device:
            from . import cusparse
            return cusparse.csrbinop(self, other, op)
        return _binop_torch(self, other, op)

    def tocsc(self, copy=False) -> "csc_matrix":
        """The same matrix in CSC, array for array what scipy's ``tocsc()`` gives (every
        column in stored entry order, duplicates kept): spg_csr2csc for device tensors."""
        if _engine_has(self.data, _lib.CSR2CSC):
            from . import cusparse
            return cusparse.csr2csc(self)
        data, indices, indptr = _stable_by_index(self.data, self.indices, self.indptr, *self._shape)
        return csc_matrix((data, indices, indptr), shape=self._shape,
                          canonical=True if self._canonical is True else None)

    def transpose(self, axes=None, copy=False) -> "csc_matrix":
        """The transpose as a csc_matrix over the same arrays (cupyx _csr.py:512-533)."""
        if axes is not None:
            raise ValueError("Sparse matrices do not support an 'axes' parameter because "
                             "swapping dimensions is the only logical permutation.")
        m, n = self._shape
        arrays = (self.data, self.indices, self.indptr)
        if copy:
            arrays = tuple(a.clone() for a in arrays)
        return csc_matrix(arrays, shape=(n, m), canonical=self._canonical)

    @property
    def T(self) -> "csc_matrix":
        return self.transpose()

    def transpose_csr(self) -> "csr_matrix":
        """A^T as a canonical CSR matrix: spg_csr2csc for device tensors (a canonical A gives a
        canonical A^T; otherwise duplicates are then summed in stored order, as the torch path
        does), else through COO with rows and columns swapped."""
        m, n = self._shape
        if _engine_has(self.data, _lib.CSR2CSC):
            from . import cusparse
            t = cusparse.csr2csc(self)
            out = csr_matrix._from_parts(t.data, t.indices, t.indptr, (n, m), canonical=t._canonical)
            out.sum_duplicates()
            return out
        counts = (self.indptr[1:] - self.indptr[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(m, device=self.device), counts)
        return coo_matrix((self.data, (self.indices.to(torch.int64), rows)), shape=(n, m),
                          device=self.device).tocsr()

    def __matmul__(self, other):
        return self.__mul__(other)

    def dot(self, other):
        return self.__mul__(other)

    def __repr__(self):
        return (f"<{self._shape[0]}x{self._shape[1]} csr_matrix of type {self.dtype} with "
                f"{self.nnz} stored elements on {self.device}>")


def _is_dense(x) -> bool:
    return isinstance(x, (torch.Tensor, np.ndarray))


def _is_vector(x) -> bool:
    return _is_dense(x) and x.ndim == 1


def _is_matrix(x) -> bool:
    return _is_dense(x) and x.ndim == 2


class coo_matrix(_SparseBase):
    """Coordinate-format operand (only what CSR conversion needs)."""
    format = "coo"

    def __matmul__(self, other):
        """COO x dense vector -> spmv, x dense matrix -> spmm (through CSR)."""
        if _is_vector(other):
            from . import cusparse
            return cusparse.spmv(self, other)
        if _is_matrix(other):
            from . import cusparse
            return cusparse.spmm(self, other)
        return super().__matmul__(other)

    def __init__(self, arg1, shape=None, device=None):
        if hasattr(arg1, "tocoo"):
            S = arg1.tocoo()
            device = device or _default_device()
            self.data = _as_tensor(S.data, _TORCH_OF[np.dtype(S.dtype)], device)
            self.row = _as_tensor(S.row, torch.int64, device)
            self.col = _as_tensor(S.col, torch.int64, device)
            self._shape = tuple(int(s) for s in S.shape)
        else:
            data, (row, col) = arg1
            device = device or (data.device if isinstance(data, torch.Tensor) else _default_device())
            self.data = data.to(device) if isinstance(data, torch.Tensor) else _as_tensor(
                data, _TORCH_OF[np.asarray(data).dtype], device)
            self.row = _as_tensor(row, torch.int64, device)
            self.col = _as_tensor(col, torch.int64, device)
            self._shape = (int(shape[0]), int(shape[1]))

    def tocsr(self) -> csr_matrix:
        """The same matrix as a canonical CSR matrix, duplicates summed in stored order (cupyx
        _coo.py tocsr: sum_duplicates, then coo2csr): spg_canonicalize for device tensors, else
        the torch form of the same rule."""
        m, n = self._shape
        if _engine_has(self.data, _lib.CANONICALIZE, max(self._shape)):
            from . import cusparse
            data, indices, indptr = cusparse._canonicalize_arrays(self.data, self.col, None, self.row, self._shape,
                                                                  _lib.SPG_CANON_SUM)
            if indptr.dtype == torch.int64 and data.numel() <= INT32_MAX:
                indptr = indptr.to(torch.int32)
            return csr_matrix._from_parts(data, indices, indptr, (m, n), canonical=True)
        key = self.row * max(n, 1) + self.col
        key_s, order = torch.sort(key, stable=True)
        data_s = self.data[order]
        uniq, counts = torch.unique_consecutive(key_s, return_counts=True)
        data_u = data_s if uniq.numel() == key_s.numel() else _segmented_sequential_sum(data_s, counts)
        urow = torch.div(uniq, max(n, 1), rounding_mode="floor")
        ipd = _indptr_dtype(uniq.numel())
        return csr_matrix((data_u, (uniq - urow * max(n, 1)).to(torch.int32),
                           _indptr_from_rows(urow, m, ipd)), shape=(m, n), canonical=True)

    def sum_duplicates(self) -> None:
        """Sort the entries by (row, column) and add up duplicates in place, in stored order,
        sequentially; the matrix stays COO (cupyx _coo.py:356-400).  Through ``tocsr()``: the
        row ids are read back off the CSR row pointer."""
        c = self.tocsr()
        self.data, self.col, self.row = c.data, c.indices.to(torch.int64), c._row_ids()

    def eliminate_zeros(self) -> None:
        """Drop the stored entries that equal zero, in place, the stored order kept (cupyx
        _coo.py:270-287).  Three masked copies: grouping the entries by row, which is what the
        engine's COO input does first, would change the stored order."""
        keep = self.data != 0
        self.data, self.row, self.col = self.data[keep].contiguous(), self.row[keep], self.col[keep]

    def todense(self, order=None, out=None) -> torch.Tensor:
        if _engine_has(self.data, _lib.DENSE_CONVERT) and max(self._shape) <= INT32_MAX:
            from . import cusparse
            d = cusparse.sparseToDense(self, out=out)
            return d if out is not None else _ordered(d, order, None)
        # grouped by row, stably, duplicates kept: the per-element order is the stored one
        key = self.row * max(self._shape[1], 1) + self.col
        _, perm = torch.sort(key, stable=True)
        rows = self.row[perm]
        ipd = _indptr_dtype(rows.numel())
        return _ordered(_compressed_to_dense(self.data[perm], self.col[perm], _indptr_from_rows(
            rows, self._shape[0], ipd), *self._shape), order, out)

    def get(self):
        import scipy.sparse as sp
        return sp.coo_matrix((self.data.cpu().numpy(), (self.row.cpu().numpy(), self.col.cpu().numpy())),
                             shape=self._shape)


class csc_matrix(_Compressed):
    """Compressed-column matrix on the device.

    ``csc_matrix(S)``            from a scipy.sparse matrix (uploaded),
    ``csc_matrix((data, indices, indptr), shape=(m, n))`` from arrays / tensors (tensors of the
    stored types on the target device are kept as they are, not copied).
    """
    format = "csc"

    def __matmul__(self, other):
        """CSC x dense vector -> spmv, x dense matrix -> spmm (cusparse.py:1395-1401,
        :1467-1473: csc.T is CSR, transposed op)."""
        if _is_vector(other):
            from . import cusparse
            return cusparse.spmv(self, other)
        if _is_matrix(other):
            from . import cusparse
            return cusparse.spmm(self, other)
        return super().__matmul__(other)

    def __init__(self, arg1, device=None, shape=None, canonical=None):
        if isinstance(arg1, tuple) and len(arg1) == 3:
            if shape is None:
                raise ValueError("shape is required for (data, indices, indptr)")
            data, indices, indptr = arg1
            device = torch.device(device) if device is not None else (
                data.device if isinstance(data, torch.Tensor) else _default_device())
            ddt = _NP_OF[data.dtype] if isinstance(data, torch.Tensor) else np.asarray(data).dtype
            self.data = _as_tensor(data, _TORCH_OF[np.dtype(ddt)], device)
            self.indices = _as_tensor(indices, torch.int32, device)
            ipd = _indptr_dtype(self.data.numel())
            self.indptr = _as_tensor(indptr, ipd, device)
            self._shape = (int(shape[0]), int(shape[1]))
            self._canonical = canonical
            if self.data.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
                raise TypeError(f"unsupported dtype {self.data.dtype}")
            if self.indptr.numel() != self._shape[1] + 1:
                raise ValueError("indptr length must be columns + 1")
            return
        if isinstance(arg1, (torch.Tensor, np.ndarray)):   # a dense matrix: the CSR form of its transposed view
            t = _dense_operand(arg1, None, torch.device(device) if device is not None else None)
            self.data, self.indices, self.indptr = _dense_to_csr(t.t())
            self._shape = (int(t.shape[0]), int(t.shape[1]))
            self._canonical = True
            return
        if isinstance(arg1, _SparseBase):   # a container of this package: its CSC form, the flag carried
            S = arg1 if isinstance(arg1, csc_matrix) else arg1.tocsr().tocsc()
            device = torch.device(device) if device is not None else S.device
            self.data, self.indices, self.indptr = S.data.to(device), S.indices.to(device), S.indptr.to(device)
            self._shape, self._canonical = S.shape, S._canonical
            return
        if not hasattr(arg1, "tocsc"):
            raise TypeError(f"unsupported csc_matrix argument {type(arg1)}")
        S = arg1.tocsc()
        device = device or _default_device()
        self.data = _as_tensor(S.data, _TORCH_OF[np.dtype(S.dtype)], device)
        self.indices = _as_tensor(S.indices, torch.int32, device)
        self.indptr = _as_tensor(S.indptr, torch.int64, device)
        self._shape = tuple(int(s) for s in S.shape)
        self._canonical = True if S.has_canonical_format else None

    @property
    def T(self) -> csr_matrix:
        """Transpose as CSR without data movement (CuPy returns csr for csc.T)."""
        m, n = self._shape
        ipd = _indptr_dtype(self.nnz)
        return csr_matrix((self.data, self.indices, self.indptr.to(ipd)), shape=(n, m))

    def transpose(self, axes=None, copy=False) -> csr_matrix:
        """The transpose as a csr_matrix over the same arrays, the canonical flag carried over
        (cupyx _csc.py transpose)."""
        if axes is not None:
            raise ValueError("Sparse matrices do not support an 'axes' parameter because "
                             "swapping dimensions is the only logical permutation.")
        out = self.T
        if copy:
            out = out.copy()
        out._canonical = self._canonical
        return out

    def copy(self):
        return csc_matrix((self.data.clone(), self.indices.clone(), self.indptr.clone()), shape=self._shape,
                          canonical=self._canonical)

    def tocsc(self, copy=False):
        return self.copy() if copy else self

    def _add_sparse(self, other, alpha, beta):
        """alpha*self + beta*other as a csc_matrix: the CSR addition of the two free transposes
        (cupyx _csc.py:250-262)."""
        other = other.tocsc() if isinstance(other, (csr_matrix, csc_matrix)) else other.tocsr().tocsc()
        return self.transpose()._add_sparse(other.transpose(), alpha, beta).transpose()

    def _binop_sparse(self, other, op: str):
        """op(self, other) as a csc_matrix: a canonical CSC is the canonical CSR of the transpose and
        the operations commute with transposition, so it is the CSR operation of the two free
        transposes."""
        other = other.tocsc() if isinstance(other, (csr_matrix, csc_matrix)) else other.tocsr().tocsc()
        return self.transpose()._binop_sparse(other.transpose(), op).transpose()

    def tocsr(self) -> csr_matrix:
        """The same matrix in CSR: spg_csr2csc for device tensors (a canonical CSC gives a
        canonical CSR; otherwise duplicates are then summed in stored order, as the torch path
        does), else through COO."""
        m, n = self._shape
        if _engine_has(self.data, _lib.CSR2CSC):
            from . import cusparse
            out = cusparse.csc2csr(self)
            out.sum_duplicates()
            return out
        counts = (self.indptr[1:] - self.indptr[:-1]).to(torch.int64)
        cols = torch.repeat_interleave(torch.arange(n, device=self.device), counts)
        return coo_matrix((self.data, (self.indices.to(torch.int64), cols)), shape=(m, n),
                          device=self.device).tocsr()

    def todense(self, order=None, out=None) -> torch.Tensor:
        m, n = self._shape
        if _engine_has(self.data, _lib.DENSE_CONVERT):
            from . import cusparse
            if order not in (None, "C", "F"):
                raise ValueError("order must be 'C' or 'F'")
            return cusparse.csc2dense(self, out=out, order=order or "C")
        return _ordered(_compressed_to_dense(self.data, self.indices, self.indptr, n, m).t(), order, out)

    def get(self):
        import scipy.sparse as sp
        return sp.csc_matrix((self.data.cpu().numpy(), self.indices.cpu().numpy(),
                              self.indptr.cpu().numpy()), shape=self._shape)


def isspmatrix_csr(x) -> bool:
    return isinstance(x, csr_matrix)


def _indptr_from_rows(rows: torch.Tensor, m: int, dtype) -> torch.Tensor:
    counts = torch.bincount(rows, minlength=m) if rows.numel() else torch.zeros(
        m, dtype=torch.int64, device=rows.device)
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=rows.device)
    indptr[1:] = torch.cumsum(counts, 0)
    return indptr.to(dtype)


def _segmented_sequential_sum(vals: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """Sum consecutive runs of `vals` (run lengths `counts`), each run left to right.
    Deterministic: runs are summed element by element in stored order."""
    nseg = counts.numel()
    starts = torch.zeros(nseg, dtype=torch.int64, device=vals.device)
    starts[1:] = torch.cumsum(counts, 0)[:-1]
    out = vals[starts].clone()
    maxc = int(counts.max()) if nseg else 0
    for r in range(1, maxc):
        sel = counts > r
        idx = starts[sel] + r
        out[sel] = out[sel] + vals[idx]
    return out
