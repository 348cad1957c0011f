"""A CSR matrix with more than 2**31 stored entries that never passes through the host, and what
every entry point outside the product path must make of it.  Shared by
tests/test_large_offsets_cpu.py (the models against scipy, at scaled-down geometries) and
tests/test_gpu_large_offsets.py (the kernels against the models, at full size).  A plain helper
module (no pytest hooks); everything is a closed form or generated from seeds; works on CPU
tensors as well as on the device.

The matrix is a PAD block followed by a TAIL.

  pad    pad_rows rows of exactly L entries over W columns, canonical.  Row i holds every column c
         with (c + i) % W >= W - L: all but a cyclic run of W - L columns that starts at (-i) % W.
         Its value is ((31 * i + 17 * c) % 61) - 30, with 0 replaced by 31: a nonzero integer of
         magnitude at most 31 that depends on row and column.  Integer values make every sum exact
         in fp32 in any order (EXACT_BOUND), so the pad's expected results need no ordering model.
  tail   a few hundred rows of standard_normal values behind the pad, built on the host as a scipy
         matrix: lengths 0, 1, 63, 64, 65 and W, a run of empty rows, the 71 rows of
         dense_seams.row_major_matrix (W == 256) and random lengths.  Its expected results come
         from scipy and the oracle; ordered sums are its job.

FULL is the smallest geometry at which a 32-bit signed entry position goes wrong: 8589935 rows of
250 entries are 2147483750 entries, row 8589934 holds offsets 2147483500 .. 2147483749 and
straddles 2**31, and every tail entry sits above 2**31.  Rows still fit 24 bits.  Nothing here
reaches 2**32.

Variants, all closed forms: `reverse` (every pad row stored in descending column order), `zeros`
(the value at (i, c) replaced by +0.0 where (7 * i + 3 * c) % 11 == 0 and by -0.0 where it is 1),
`mul` (every column multiplied by 547 over 140000 columns: three blocks of 65536 columns), and the
COO order of build_coo(): all odd rows' entries, then all even rows'.

Everything runs in slices of at most SLICE entries: no torch operation sees more, and no host array
is proportional to the entry count.  The big arrays are allocated once and filled through views.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests import canon_cases as cc
from tests import dense_seams as ds
from tests.instantiations import seed_of

SLICE = 1 << 26                       # entries (or dense elements) one torch operation may see
FULL = dict(pad_rows=8589935, L=250, W=256)
VMAX = 31                             # largest |pad value|
XMAX = 3                              # largest |x| and |B| element of the dense operands
WIDE_MUL, WIDE_COLS = 547, 140000
CAP_BYTES = 160 << 30                 # no test may need more device memory than this
GiB = float(1 << 30)


def _torch():
    import torch
    return torch


def pad_value(i, c):
    """The pad's value at (row i, column c) for int64 tensors (or numpy arrays) that broadcast."""
    v = (31 * i + 17 * c) % 61 - 30
    return v + 31 * (v == 0)          # 0 -> 31


def zero_kind(i, c):
    """0: the `zeros` variant stores +0.0 at (i, c); 1: -0.0; anything else: the value stays."""
    return (7 * i + 3 * c) % 11


def x_vector(W):
    """The dense vector of the SpMV runs: integers in [-3, 3], float32, read-only."""
    x = ((5 * np.arange(W)) % 7 - 3).astype(np.float32)
    x.setflags(write=False)
    return x


def b_matrix(W, n):
    """The dense B (W x n) of the SpMM runs: integers in [-3, 3], float32, read-only."""
    B = ((5 * np.arange(W)[:, None] + 3 * np.arange(n)[None, :]) % 7 - 3).astype(np.float32)
    B.setflags(write=False)
    return B


def y0_of(i):
    """The y (or C) that beta multiplies, at row i: even integers in [-8, 8], so 0.5 * y0 is exact."""
    return 2 * ((3 * i) % 9 - 4)


def make_tail(W, seed="tail"):
    """The tail as a canonical scipy CSR matrix (float32, int32 indices), read-only."""
    rng = np.random.default_rng(seed_of("large_offsets", seed, W))
    lens = [min(n, W) for n in (0, 1, 63, 64, 65, W)] + [0] * 9
    rows = [np.sort(rng.choice(W, n, replace=False)) for n in lens]
    if W == ds.ROW_MAJOR_COLS:            # the lengths on each side of the SpMM batches and unrolls
        S = ds.row_major_matrix("f32")
        rows += [S.indices[S.indptr[r]:S.indptr[r + 1]] for r in range(S.shape[0])]
    rows += [np.sort(rng.choice(W, int(n), replace=False)) for n in rng.integers(0, W + 1, 100)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    T = sp.csr_matrix((rng.standard_normal(indices.size).astype(np.float32), indices, indptr), shape=(len(rows), W))
    assert T.has_canonical_format and np.count_nonzero(T.data) == T.nnz
    for a in (T.data, T.indices, T.indptr):
        a.setflags(write=False)
    return T


class Csr:
    """Three tensors and a shape: indptr (int64), indices (int32), values (float32)."""

    def __init__(self, rows, cols, indptr, indices, values):
        self.rows, self.cols, self.indptr, self.indices, self.values = rows, cols, indptr, indices, values
        self.nnz = int(indices.numel())

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.indptr, self.indices, self.values) if t is not None)


class Geometry:
    """(pad_rows, L, W, tail): the matrix of the module docstring.  `slice_entries` bounds every
    torch operation (the CPU tests lower it so that a small matrix still takes several slices)."""

    def __init__(self, pad_rows, L, W, tail=None, slice_entries=SLICE):
        assert 0 < L <= W and pad_rows >= 1
        self.pad_rows, self.L, self.W, self.G = int(pad_rows), int(L), int(W), int(W - L)
        self.tail = make_tail(W) if tail is None else tail
        assert self.tail.shape[1] == W
        self.tail_rows = int(self.tail.shape[0])
        self.rows = self.pad_rows + self.tail_rows
        self.pad_nnz = self.pad_rows * self.L
        self.nnz = self.pad_nnz + int(self.tail.nnz)
        self.slice_entries = int(slice_entries)
        self.slice_rows = max(1, self.slice_entries // self.W)

    # ---- arithmetic of the geometry (no allocation)

    def straddling_row(self, boundary=1 << 31):
        """The pad row whose entries lie on both sides of offset `boundary` (None: a row starts
        exactly there or the pad ends below it)."""
        r = boundary // self.L
        return r if r < self.pad_rows and r * self.L < boundary < (r + 1) * self.L else None

    def marked_rows(self, boundary=1 << 31):
        """The pad rows the small operands touch: the first, the straddling one (or the middle
        one), the last."""
        s = self.straddling_row(boundary)
        return sorted({0, self.pad_rows // 2 if s is None else s, self.pad_rows - 1})

    def row_slices(self, r0=0, r1=None):
        """(a, b) row ranges that cover pad rows [r0, r1), each at most slice_entries wide."""
        r1 = self.pad_rows if r1 is None else r1
        for a in range(r0, r1, self.slice_rows):
            yield a, min(a + self.slice_rows, r1)

    def csr_bytes(self, nnz=None, rows=None):
        """Bytes of a float32 CSR matrix with an int64 row pointer."""
        return ((self.rows if rows is None else rows) + 1) * 8 + (self.nnz if nnz is None else nnz) * 8

    # ---- the pad's closed forms

    def _i(self, r0, r1, device):
        return _torch().arange(r0, r1, dtype=_torch().int64, device=device)[:, None]

    def pad_cols(self, r0, r1, device, reverse=False):
        """Columns of pad rows [r0, r1) in stored order: int64 (r1 - r0, L), by (row, position)."""
        torch = _torch()
        i = self._i(r0, r1, device)
        k = torch.arange(self.L, dtype=torch.int64, device=device)[None, :]
        s = (-i) % self.W                                  # first column of the row's gap
        over = s + self.G - self.W                         # > 0: the gap wraps round the last column
        c = torch.where(over > 0, k + over, torch.where(k < s, k, k + self.G))
        return c.flip(1) if reverse else c

    def pad_vals(self, r0, r1, cols, zeros=False):
        """float32 values of pad rows [r0, r1) at the columns `cols` (pad_cols' result)."""
        torch = _torch()
        i = self._i(r0, r1, cols.device)
        v = pad_value(i, cols).to(torch.float32)
        if zeros:
            z = zero_kind(i, cols)
            v = torch.where(z == 0, torch.zeros_like(v), torch.where(z == 1, -torch.zeros_like(v), v))
        return v

    def pad_dense(self, r0, r1, device, zeros=False):
        """Pad rows [r0, r1) as a dense float32 (r1 - r0, W) block, by (row, column): the pattern
        test itself, not a scatter of pad_cols."""
        torch = _torch()
        i = self._i(r0, r1, device)
        c = torch.arange(self.W, dtype=torch.int64, device=device)[None, :]
        held = (c + i) % self.W >= self.G
        v = self.pad_vals(r0, r1, c.expand(r1 - r0, self.W), zeros)
        return torch.where(held, v, torch.zeros_like(v))

    def pad_row_host(self, i, reverse=False):
        """(columns int32, values float32) of pad row i as numpy arrays, from the definition."""
        c = np.array([c for c in range(self.W) if (c + i) % self.W >= self.G], dtype=np.int64)
        v = pad_value(np.int64(i), c).astype(np.float32)
        if reverse:
            c, v = c[::-1], v[::-1]
        return c.astype(np.int32), v

    # ---- building operands

    def fill_pad(self, indices, values, offset, r0, r1, reverse=False, zeros=False, mul=1):
        """Write pad rows [r0, r1) into the flat arrays from entry `offset` on, slice by slice.
        Either array may be None."""
        dev = (indices if indices is not None else values).device
        for a, b in self.row_slices(r0, r1):
            lo, hi = offset + (a - r0) * self.L, offset + (b - r0) * self.L
            c = self.pad_cols(a, b, dev, reverse)
            if indices is not None:
                indices[lo:hi].view(b - a, self.L).copy_(c * mul)
            if values is not None:
                values[lo:hi].view(b - a, self.L).copy_(self.pad_vals(a, b, c, zeros))

    def pad_indptr(self, out, shift=0):
        """out[0 : pad_rows + 1] = i * L + shift."""
        torch = _torch()
        for a in range(0, self.pad_rows + 1, self.slice_entries):
            b = min(a + self.slice_entries, self.pad_rows + 1)
            out[a:b] = torch.arange(a, b, dtype=torch.int64, device=out.device) * self.L + shift

    def build(self, device, reverse=False, zeros=False, mul=1, cols=None, values=True):
        """The whole matrix on `device`.  The tail always arrives in canonical order, with its
        own values."""
        torch = _torch()
        indptr = torch.empty(self.rows + 1, dtype=torch.int64, device=device)
        indices = torch.empty(self.nnz, dtype=torch.int32, device=device)
        vals = torch.empty(self.nnz, dtype=torch.float32, device=device) if values else None
        self.pad_indptr(indptr)
        indptr[self.pad_rows:] = torch.from_numpy(self.tail.indptr.astype(np.int64) + self.pad_nnz).to(device)
        self.fill_pad(indices, vals, 0, 0, self.pad_rows, reverse, zeros, mul)
        indices[self.pad_nnz:] = torch.from_numpy(self.tail.indices.astype(np.int32) * np.int32(mul)).to(device)
        if values:
            vals[self.pad_nnz:] = torch.from_numpy(np.array(self.tail.data)).to(device)
        return Csr(self.rows, self.W if cols is None else cols, indptr, indices, vals)

    def first_pad_difference(self, M, reverse=False, zeros=False, mul=1):
        """None when M's pad part still equals the closed form bit for bit, else a message that
        names the first differing slice, row and offset."""
        torch = _torch()
        for n, (a, b) in enumerate(self.row_slices()):
            lo, hi = a * self.L, b * self.L
            c = self.pad_cols(a, b, M.indices.device, reverse)
            bad = M.indices[lo:hi].view(b - a, self.L) != (c * mul).to(torch.int32)
            if M.values is not None:
                want = self.pad_vals(a, b, c, zeros)
                bad |= M.values[lo:hi].view(b - a, self.L).view(torch.int32) != want.view(torch.int32)
            if bool(bad.any()):
                r, k = (int(v) for v in bad.nonzero()[0])
                return f"slice {n}: row {a + r}, offset {(a + r) * self.L + k}"
            p = M.indptr[a:b + 1]
            if not torch.equal(p, torch.arange(a, b + 1, dtype=torch.int64, device=p.device) * self.L):
                return f"slice {n}: row pointer of rows {a}..{b}"
        return None

    def tail_of(self, M):
        """M's tail part as host arrays (indptr rebased to 0, indices, values)."""
        p = M.indptr[self.pad_rows:].cpu().numpy() - self.pad_nnz
        x = None if M.values is None else M.values[self.pad_nnz:].cpu().numpy()
        return p, M.indices[self.pad_nnz:].cpu().numpy(), x

    # ---- y = alpha * A x + beta * y0 and C = alpha * A B + beta * C0

    def y0_rows(self, r0, r1, device, n=None):
        """y0 (n None) or the row-constant C0 (r1 - r0, n) of rows [r0, r1), float32."""
        y = y0_of(self._i(r0, r1, device)).to(_torch().float32)
        return y[:, 0] if n is None else y.expand(r1 - r0, n)

    def expect_product_pad(self, r0, r1, X, alpha, beta):
        """alpha * (pad rows [r0, r1)) @ X + beta * y0 for an integer X (W,) or (W, n) on the
        device: float32, exact (float64 holds every intermediate), so a numeric == is the check."""
        torch = _torch()
        D = self.pad_dense(r0, r1, X.device).to(torch.float64)
        S = D @ X.to(torch.float64)
        y0 = self.y0_rows(r0, r1, X.device, None if X.dim() == 1 else X.shape[1]).to(torch.float64)
        out = alpha * S + beta * y0
        assert float(out.abs().max()) < EXACT_BOUND
        return out.to(torch.float32)

    def tail_y0(self, n=None):
        i = np.arange(self.pad_rows, self.rows, dtype=np.int64)
        y = y0_of(i).astype(np.float32)
        return y if n is None else np.ascontiguousarray(np.broadcast_to(y[:, None], (self.tail_rows, n)))

    # ---- the transpose

    def csc_pad_counts(self):
        """Per column j, the number of pad rows that hold it (int64 numpy, W entries)."""
        j, r = np.arange(self.W)[:, None], np.arange(self.W)[None, :]
        held = (j + r) % self.W >= self.G                           # row residue r holds column j
        full, rem = divmod(self.pad_rows, self.W)
        return full * self.L + held[:, :rem].sum(axis=1).astype(np.int64)

    def csc_indptr(self):
        """The transpose's row pointer (int64 numpy, W + 1 entries): per column, the pad rows that
        hold it, then the tail's entries of that column."""
        cnt = self.csc_pad_counts() + np.diff(self.tail.tocsc().indptr).astype(np.int64)
        return np.concatenate([[0], np.cumsum(cnt)])

    def csc_pad_row(self, j, device):
        """(rows int32, values float32) of the pad part of the transpose's row j, in order."""
        torch = _torch()
        res = np.array(sorted((t - j) % self.W for t in range(self.G, self.W)), dtype=np.int64)
        n = int(self.csc_pad_counts()[j])
        k = torch.arange(n, dtype=torch.int64, device=device)
        i = (k // self.L) * self.W + torch.from_numpy(res).to(device)[k % self.L]
        return i.to(torch.int32), pad_value(i, j).to(torch.float32)

    def csc_tail(self):
        """The tail's transpose: scipy's tocsc() of the tail, the row ids shifted behind the pad."""
        T = self.tail.tocsc()
        return T.indptr.astype(np.int64), T.indices.astype(np.int32) + np.int32(self.pad_rows), T.data

    # ---- zeros dropped (DROP_ZEROS on the `zeros` variant; the dense round trip with zeros)

    def dropped_pad(self, r0, r1, device):
        """What remains of pad rows [r0, r1) of the `zeros` variant once its zeros are gone:
        (entries per row int64, columns int32 flat, values float32 flat), in stored order."""
        torch = _torch()
        c = self.pad_cols(r0, r1, device)
        keep = zero_kind(self._i(r0, r1, device), c) > 1
        return keep.sum(1), c[keep].to(torch.int32), self.pad_vals(r0, r1, c)[keep]

    def dropped_pad_nnz(self):
        """Entries of the whole pad that the `zeros` variant keeps (host arithmetic: zero_kind
        has period 11 in i and the pattern period W, so one period of 11 * W rows is counted)."""
        per = 11 * self.W
        i, c = np.arange(per, dtype=np.int64)[:, None], np.arange(self.W, dtype=np.int64)[None, :]
        kept = (((c + i) % self.W >= self.G) & (zero_kind(i, c) > 1)).sum(axis=1)
        full, rem = divmod(self.pad_rows, per)
        return int(full * kept.sum() + kept[:rem].sum())

    # ---- 16-bit columns of the `mul` variant

    def block_starts_pad(self, r0, r1, device, mul=WIDE_MUL, cols=WIDE_COLS):
        """block_starts of pad rows [r0, r1) of the matrix with columns c * mul: per interior block
        boundary b * 65536, the number of the row's entries below it.  uint32 bits as int32,
        (r1 - r0, 2) for the three blocks of WIDE_COLS."""
        torch = _torch()
        i = self._i(r0, r1, device)
        c = torch.arange(self.W, dtype=torch.int64, device=device)[None, :]
        held = (c + i) % self.W >= self.G
        nb1 = -(-cols // 65536) - 1                             # interior block boundaries
        out = [(held & (c * mul < (b << 16))).sum(1) for b in range(1, nb1 + 1)]
        return torch.stack(out, dim=1).to(torch.int32)

    # ---- COO order: all odd rows' entries, then all even rows'

    def coo_segments(self):
        """[(parity, first entry of that parity's block)]: odd rows first."""
        odd_pad = self.pad_rows // 2
        t = np.diff(self.tail.indptr).astype(np.int64)
        r = np.arange(self.pad_rows, self.rows)
        odd_total = odd_pad * self.L + int(t[r % 2 == 1].sum())
        return [(1, 0), (0, odd_total)]

    def build_coo(self, device, values=True):
        """(coo_rows int32, indices int32, values float32 or None): the forward matrix's entries,
        all odd rows' first and then all even rows', each row's entries in canonical order."""
        torch = _torch()
        rows = torch.empty(self.nnz, dtype=torch.int32, device=device)
        cols = torch.empty(self.nnz, dtype=torch.int32, device=device)
        vals = torch.empty(self.nnz, dtype=torch.float32, device=device) if values else None
        half = max(1, self.slice_rows)
        tp = self.tail.indptr
        for parity, off in self.coo_segments():
            first = parity                                            # first pad row of this parity
            count = (self.pad_rows - first + 1) // 2
            for a in range(0, count, half):
                b = min(a + half, count)
                i = (first + 2 * torch.arange(a, b, dtype=torch.int64, device=device))[:, None]
                k = torch.arange(self.L, dtype=torch.int64, device=device)[None, :]
                s = (-i) % self.W
                over = s + self.G - self.W
                c = torch.where(over > 0, k + over, torch.where(k < s, k, k + self.G))
                lo, hi = off + a * self.L, off + b * self.L
                rows[lo:hi].view(b - a, self.L).copy_(i.expand(b - a, self.L))
                cols[lo:hi].view(b - a, self.L).copy_(c)
                if values:
                    vals[lo:hi].view(b - a, self.L).copy_(pad_value(i, c))
            pos = off + count * self.L
            for t in range(self.tail_rows):
                if (self.pad_rows + t) % 2 != parity:
                    continue
                n = int(tp[t + 1] - tp[t])
                rows[pos:pos + n] = self.pad_rows + t
                cols[pos:pos + n] = torch.from_numpy(self.tail.indices[tp[t]:tp[t + 1]].astype(np.int32)).to(device)
                if values:
                    vals[pos:pos + n] = torch.from_numpy(np.array(self.tail.data[tp[t]:tp[t + 1]])).to(device)
                pos += n
        return rows, cols, vals

    # ---- the small operand of the additions

    def small_operand(self, seed="geam-b", boundary=1 << 31):
        """B of `big + small`: populated only in the marked pad rows and the tail, and holding in
        each marked row the columns the pad lacks there besides shared ones.  Returns (touched,
        B_small): the touched row ids (marked rows, then every tail row) and B's touched rows as a
        scipy CSR matrix of len(touched) x W; every other row of B is empty."""
        rng = np.random.default_rng(seed_of("large_offsets", seed, self.pad_rows, self.L, self.W))
        marked = self.marked_rows(boundary)
        rows = []
        for n, i in enumerate(marked):
            gap = [c for c in range(self.W) if (c + i) % self.W < self.G]
            if n == 0:
                cols = np.arange(self.W)                                      # a full row
            else:
                cols = np.union1d(gap, rng.choice(self.W, min(self.W, 40 * n), replace=False))
            rows.append(np.sort(cols))
        for t in range(self.tail_rows):
            have = self.tail.indices[self.tail.indptr[t]:self.tail.indptr[t + 1]]
            kind = t % 4                                  # empty, the same pattern, disjoint-ish, random
            if kind == 0:
                cols = np.zeros(0, np.int64)
            elif kind == 1:
                cols = have
            else:
                cols = np.sort(rng.choice(self.W, int(rng.integers(0, self.W + 1)), replace=False))
            rows.append(np.asarray(cols, dtype=np.int64))
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        indices = np.concatenate(rows).astype(np.int32)
        Bs = sp.csr_matrix((rng.standard_normal(indices.size).astype(np.float32), indices, indptr),
                           shape=(len(rows), self.W))
        touched = np.array(marked + list(range(self.pad_rows, self.rows)), dtype=np.int64)
        return touched, Bs

    def touched_rows_of_A(self, touched):
        """A's rows `touched` (marked pad rows from the definition, then the tail) as scipy CSR."""
        marked = [int(i) for i in touched if i < self.pad_rows]
        parts = [self.pad_row_host(i) for i in marked]
        top = sp.csr_matrix((np.concatenate([v for _, v in parts]), np.concatenate([c for c, _ in parts]),
                             np.arange(len(parts) + 1, dtype=np.int32) * self.L), shape=(len(parts), self.W))
        return sp.vstack([top, self.tail]).tocsr()

    def spread_small(self, touched, Bs, device):
        """The small operand as a full-height Csr on `device`."""
        torch = _torch()
        counts = torch.zeros(self.rows, dtype=torch.int64, device=device)
        counts[torch.from_numpy(touched).to(device)] = torch.from_numpy(np.diff(Bs.indptr).astype(np.int64)).to(device)
        indptr = torch.zeros(self.rows + 1, dtype=torch.int64, device=device)
        for a in range(0, self.rows, self.slice_entries):               # a running cumulative sum
            b = min(a + self.slice_entries, self.rows)
            indptr[a + 1:b + 1] = counts[a:b].cumsum(0) + indptr[a]
        return Csr(self.rows, self.W, indptr, torch.from_numpy(Bs.indices.astype(np.int32)).to(device),
                   torch.from_numpy(np.array(Bs.data)).to(device))

    def expect_sum(self, touched, Bs, alpha, beta):
        """alpha * A + beta * B on the touched rows by scipy, and how the result lies in C:
        (Cs, extra) with Cs the touched rows of C as scipy CSR (canonical, nothing cancelled) and
        extra[n] the entries C has gained over A before touched row n starts (extra[-1]: in all).
        An untouched row r between touched rows n - 1 and n is A's row moved by extra[n]."""
        from tests import geam_cases as gc
        As = self.touched_rows_of_A(touched)
        p, j, x = gc.reference_full(As, Bs, alpha, beta)
        Cs = sp.csr_matrix((x, j, p), shape=As.shape)
        assert np.count_nonzero(x) == x.size, "a sum cancelled: scipy's structure would differ from the engine's"
        gain = np.diff(p) - np.diff(As.indptr)
        return Cs, np.concatenate([[0], np.cumsum(gain)]).astype(np.int64)

    # ---- the non-canonical input of SORT | SUM

    def canon_tail_input(self, seed="canon-tail"):
        """The tail as SORT | SUM's input: every row reversed, a third of the entries stored again
        (a duplicate, after the row's own entries), and rows of canon_cases.short_row_triplets in
        the rows that were empty.  Returns (indptr, indices, values) in stored order (numpy)."""
        rng = np.random.default_rng(seed_of("large_offsets", seed, self.W))
        sr, sc, sv_ = cc.short_row_triplets(self.tail_rows, self.W, np.float32, seed_of(seed, "short"))
        tp, rows_c, rows_v = self.tail.indptr, [], []
        for t in range(self.tail_rows):
            c, v = self.tail.indices[tp[t]:tp[t + 1]][::-1], self.tail.data[tp[t]:tp[t + 1]][::-1]
            if c.size == 0:
                sel = sr == t
                c, v = sc[sel].astype(np.int32), sv_[sel]
            else:
                again = rng.random(c.size) < 1 / 3
                c = np.concatenate([c, c[again]])
                v = np.concatenate([v, rng.standard_normal(int(again.sum())).astype(np.float32)])
            rows_c.append(c.astype(np.int32))
            rows_v.append(v.astype(np.float32))
        indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_c])]).astype(np.int64)
        return indptr, np.concatenate(rows_c), np.concatenate(rows_v)

    SPLIT = 7        # a marked row's duplicated entries are stored as (v - 7) in place and 7 at the row's end

    def canon_marked_row(self, i):
        """Pad row i as SORT | SUM's input: reversed, every fifth entry's value lowered by SPLIT,
        and SPLIT stored again under the same column at the end of the row.  The sums are the
        forward row exactly (integers)."""
        c, v = self.pad_row_host(i, reverse=True)
        dup = np.arange(c.size) % 5 == 2
        v = v.copy()
        v[dup] -= self.SPLIT
        return np.concatenate([c, c[dup]]), np.concatenate([v, np.full(int(dup.sum()), self.SPLIT, np.float32)])

    def build_canon_input(self, device, boundary=1 << 31):
        """The `reverse` variant with duplicates in the marked pad rows and in the tail, as a Csr
        on `device`, plus the tail's expected output (indptr, indices, values) by canon_cases.restate.
        SORT | SUM of it is the forward pad exactly, followed by that tail."""
        torch = _torch()
        marked = self.marked_rows(boundary)
        hosts = {i: self.canon_marked_row(i) for i in marked}
        tp, tj, tx = self.canon_tail_input()
        extra = sum(len(c) - self.L for c, _ in hosts.values())
        nnz = self.pad_nnz + extra + int(tp[-1])
        indptr = torch.empty(self.rows + 1, dtype=torch.int64, device=device)
        indices = torch.empty(nnz, dtype=torch.int32, device=device)
        vals = torch.empty(nnz, dtype=torch.float32, device=device)
        self.pad_indptr(indptr)
        shift, prev = 0, 0
        for i in marked + [self.pad_rows]:
            if i > prev:
                self.fill_pad(indices, vals, prev * self.L + shift, prev, i, reverse=True)
            if i == self.pad_rows:
                break
            c, v = hosts[i]
            lo = i * self.L + shift
            indices[lo:lo + len(c)] = torch.from_numpy(np.ascontiguousarray(c)).to(device)
            vals[lo:lo + len(c)] = torch.from_numpy(np.ascontiguousarray(v)).to(device)
            shift += len(c) - self.L
            indptr[i + 1:self.pad_rows + 1] += len(c) - self.L
            prev = i + 1
        base = self.pad_nnz + extra
        indptr[self.pad_rows:] = torch.from_numpy(tp + base).to(device)
        indices[base:] = torch.from_numpy(tj).to(device)
        vals[base:] = torch.from_numpy(tx).to(device)
        want = cc.restate((self.tail_rows, self.W), cc.rows_of(tp), tj, tx, cc.SORT | cc.SUM)
        return Csr(self.rows, self.W, indptr, indices, vals), want


EXACT_BOUND = float(1 << 24)          # integers below it are exact in fp32, whatever the order of the sum


def exactness_margin(L, alpha=2.0, beta=0.5, ymax=8):
    """An upper bound of |alpha * sum + beta * y0| over a row of L pad entries against an integer
    operand: it must stay below EXACT_BOUND for the pad's expected products to need no order."""
    return abs(alpha) * L * VMAX * XMAX + abs(beta) * ymax


def first_difference(got, want):
    """Index tuple of the first element where two equally shaped tensors differ (numeric !=, so a
    NaN poison differs from everything), or None."""
    bad = got != want
    if not bool(bad.any()):
        return None
    return tuple(int(v) for v in bad.nonzero()[0])


def first_bit_difference(got, want):
    """The same on the bit patterns of two float32 tensors."""
    torch = _torch()
    return first_difference(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


# ---- device bytes per test at a geometry: the arrays the test allocates (the library's own answer
# ---- to the size query is added by the test, and estimated here for the cap)

def workspace_share(g):
    """{test: the bytes of planned_bytes' figure that stand for the library's workspaces}.  They
    restate the carves of spmm_amd/csrc/spg_format_layouts.hpp for int64 positions, per entry: a
    digit table of 1 byte (256 counters of 8 bytes per 2048 entries), the transpose's sorted
    columns 4, a sort's two record buffers 16 each, the kept marks 8, the addition's marks 8 per
    entry of its second operand and 8 per row, the dense table 8 per row; the look-back words,
    scalars and alignment are covered by 1 % on top.  tests/test_format_layouts_cpu.py holds the
    carves themselves under these figures."""
    def ws(per_entry, per_row=0):
        return int(1.01 * (per_entry * g.nnz + per_row * g.rows))
    return {
        "csr2csc": ws(1 + 4),
        "csrgeam": ws(8, 48),                    # the swapped roles mark all of A
        "canonicalize_sum": ws(1 + 8 + 32),      # table + marks + records
        "canonicalize_drop": ws(8),
        "canonicalize_coo": ws(1 + 32),
        "dense": ws(0, 8),                       # the table
        "shim": ws(0, 24),
    }


def planned_bytes(g):
    """{test: device bytes it needs beyond the shared forward operand}, plus "operand" itself: the
    arrays the test allocates, the temporaries of one slice ("validate" is those alone) and the
    workspace (workspace_share); everything small is covered by 256 MiB.  The GPU tests print what
    the size queries answer and add that instead."""
    A = g.csr_bytes()
    n = g.nnz
    slice_tmp = 16 * 8 * g.slice_entries
    dense = g.rows * g.W * 4
    ws = workspace_share(g)
    slack = 1 << 28          # guard bands, small operands, the dense operands of the products
    plan = {
        "operand": A,
        "validate": slice_tmp,
        "spmv": 2 * g.rows * 4 + slice_tmp,
        "spmm": 2 * g.rows * 33 * 4 + slice_tmp,
        "csr2csc": A + ws["csr2csc"] + slice_tmp,
        "csrgeam": 2 * A + ws["csrgeam"] + slice_tmp,                     # two results
        "canonicalize_sum": 2 * A + ws["canonicalize_sum"] + slice_tmp,   # the input, C
        "canonicalize_drop": 2 * A + ws["canonicalize_drop"] + slice_tmp,
        "canonicalize_coo": A + 12 * n + ws["canonicalize_coo"] + slice_tmp,
        "dense": 2 * dense + A + ws["dense"] + slice_tmp,                 # D in both orders, C
        "cols16": (4 + 2 + 4) * n + 16 * g.rows + slice_tmp,              # wide indices, lo16, joined indices, starts
        "shim": dense + A + ws["shim"] + slice_tmp,
    }
    return {k: v + (slack if k not in ("operand", "validate") else 0) for k, v in plan.items()}
