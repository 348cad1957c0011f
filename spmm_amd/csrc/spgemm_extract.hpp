// spgemm_extract.hpp -- C = A[R, K], a submatrix of a CSR matrix: spg_csr_extract_nnz /
// spg_csr_extract, the device form of scipy's get_csr_submatrix, csr_row_index, csr_row_slice and
// csr_column_index1 / csr_column_index2 (cupyx's own kernels behind csr_matrix.__getitem__,
// modify_src/cupy-src/cupyx/scipy/sparse/_index.py:348 and :45-115, _compressed.py:403, :566,
// :643, :665; no cuSPARSE call).
//
// R is a row range with any step or a list of rows, K all columns, a column range with any step
// or a list of columns; lists in any order, repeats allowed.  Output row i is source row
// sel_r(i) walked in stored order; a stored entry (j, v) gives
//   K = all     one entry (j, v);
//   K = range   one entry ((j - start) / step, v) iff step divides j - start and the quotient
//               lies in [0, count);
//   K = list    one entry (t, v) for every position t with idx[t] == j, positions ascending.
// Values are moved as raw bits (integer loads and stores of their width).
//
// Flat over entries, every position a function of the structures alone:
//   k_ex_pack     (column list) the records (key = idx[t], pos = t); the passes of
//                 spg_canonicalize's sort (k_tr_hist, k_scan_lb, k_cn_scatter) group them by
//                 column, stably, and k_tr_indptr reads colptr (cols + 1 entries) off the sorted
//                 keys: the sorted records are colpos, positions ascending inside a column;
//   k_ex_mark     one lane per stored entry e of A: mult[e], 0 or 1 by the range test, or
//                 colptr[j + 1] - colptr[j] for a list;
//   k_scan_lb     mult in place -> S, the exclusive prefix (nnz(A) + 1 entries).  mult depends on
//                 the entry's column alone, so one S serves every selected row and every repeat of
//                 it.  S is int64 for a list (its total is bounded by nnz(A) * k), A's row-pointer
//                 type for a range (mult <= 1).  K = all: S is the identity and is not built;
//   k_ex_count    per output row i, r = sel_r(i): S[Ap[r + 1]] - S[Ap[r]];
//   k_scan_lb     the counts -> C's row pointer, the total -> nnz(C);
//   k_ex_fill     one lane per OUTPUT position o, 64 consecutive per step, one wave per chunk of
//                 EX_CHUNK: i = the row of o in Cp, r = sel_r(i), q = o - Cp[i]; the source entry e
//                 is the last position of A's row r with S[e] - S[Ap[r]] <= q (a binary search in
//                 S), u = q - (S[e] - S[Ap[r]]) the repeat number; the column is
//                 colpos[colptr[j] + u], (j - start) / step or j, the value Ax[e].  When a step's
//                 64 outputs lie in one output row the search window is bounded once from the
//                 step's first and last lane, as gm_find does.  Writes are coalesced, reads a
//                 gather.  K = all over a step-1 row range is one contiguous span of A and is
//                 copied lane for lane.
// No atomic anywhere (the sort's LDS histogram adds are integer counts); results are identical
// from run to run.
//
// IP is A's row-pointer type, CP C's, SP S's; V the raw-bit type of the value's width.
#pragma once

#include "spg_device.hpp"
#include "spg_format_layouts.hpp" // EX_ALL / EX_RANGE / EX_LIST, EX_REC_BYTES
#include "spgemm_canon.hpp"       // CnRec, CnKeys, the sort passes
#include "spgemm_transpose.hpp"   // tr_row_of

namespace spg {

constexpr int EX_WPB = 4;        // waves per workgroup
constexpr int EX_CHUNK = 1024;   // output entries per wave chunk (16 steps of 64)
constexpr int EX_BLOCK = 256;

// (EX_ALL / EX_RANGE / EX_LIST, the column selection's mode: spg_format_layouts.hpp)

using ExRec = CnRec<int32_t, uint32_t>;   // (listed column, position in the list)
static_assert(sizeof(ExRec) == EX_REC_BYTES, "ex_layout's record size");

// The row selection: sel_r(i).
struct ExRows {
    const int32_t* index;   // nullptr: start + i * step
    int64_t start, step;
    __device__ __forceinline__ int64_t operator()(int64_t i) const {
        return index ? (int64_t)index[i] : start + i * step;
    }
};

// The column selection as the kernels read it.
struct ExCols {
    int mode;                    // EX_ALL / EX_RANGE / EX_LIST
    int64_t start, step, count;  // EX_RANGE (step != 0)
    const int32_t* colptr;       // EX_LIST: cols + 1 entries
    const ExRec* colpos;         // EX_LIST: the list's positions grouped by column
};

// The last position e in [lo, hi] with S[e] <= t (S[lo] <= t).
template <typename SP>
__device__ __forceinline__ int64_t ex_last_le(const SP* __restrict__ S, int64_t lo, int64_t hi, int64_t t) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)S[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The records of a column list in list order.
__global__ __launch_bounds__(EX_BLOCK) void k_ex_pack(int64_t k, const int32_t* __restrict__ idx,
                                                     ExRec* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (t >= k) return;
    ExRec r;
    r.key = (uint32_t)idx[t];
    r.pos = (int32_t)t;
    out[t] = r;
}

// mult[e]: the output entries stored entry e gives in any selected row.
template <typename SP>
__global__ __launch_bounds__(EX_BLOCK) void k_ex_mark(int64_t nnz, const int32_t* __restrict__ Aj, ExCols K,
                                                     SP* __restrict__ mult) {
    const int64_t e = (int64_t)blockIdx.x * EX_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const int64_t j = Aj[e];
    int64_t m;
    if (K.mode == EX_LIST) {
        m = (int64_t)K.colptr[j + 1] - (int64_t)K.colptr[j];
    } else {
        const int64_t d = j - K.start, t = d / K.step;
        m = (t * K.step == d && t >= 0 && t < K.count) ? 1 : 0;
    }
    mult[e] = (SP)m;
}

// Entries of output row i.  S == nullptr: K = all.
template <typename IP, typename SP>
__global__ __launch_bounds__(EX_BLOCK) void k_ex_count(int64_t nr, ExRows R, const IP* __restrict__ Ap,
                                                      const SP* __restrict__ S, int64_t* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * EX_BLOCK + threadIdx.x; i < nr; i += (int64_t)gridDim.x * EX_BLOCK) {
        const int64_t r = R(i);
        const int64_t a0 = (int64_t)Ap[r], a1 = (int64_t)Ap[r + 1];
        cnt[i] = S ? (int64_t)S[a1] - (int64_t)S[a0] : a1 - a0;
    }
}

// C's indices and values.  contig: K = all over a step-1 row range.
template <typename IP, typename CP, typename SP, typename V>
__global__ __launch_bounds__(EX_WPB * WAVE) void k_ex_fill(int64_t nr, int64_t nnzC, int64_t chunks, ExRows R,
                                                          ExCols K, bool contig, const IP* __restrict__ Ap,
                                                          const int32_t* __restrict__ Aj,
                                                          const V* __restrict__ Ax, const SP* __restrict__ S,
                                                          const CP* __restrict__ Cp, int32_t* __restrict__ Cj,
                                                          V* __restrict__ Cx) {
    const int l = lane_id();
    const int64_t chunk = (int64_t)blockIdx.x * EX_WPB + (threadIdx.x >> 6);
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    const int64_t o0 = chunk * EX_CHUNK, o1 = min(nnzC, o0 + EX_CHUNK);
    if (contig) {   // output position o is A's entry Ap[first row] + o
        const int64_t base = (int64_t)Ap[R.start];
        for (int64_t o = o0 + l; o < o1; o += WAVE) {
            Cj[o] = Aj[base + o];
            Cx[o] = Ax[base + o];
        }
        return;
    }
    const int64_t ilo = tr_row_of(Cp, 0, nr - 1, o0);         // output rows of the chunk's first and
    const int64_t ihi = tr_row_of(Cp, ilo, nr - 1, o1 - 1);   // last entry (wave-uniform)
    for (int64_t b0 = o0; b0 < o1; b0 += WAVE) {
        const bool active = b0 + l < o1;
        const int64_t o = active ? b0 + l : b0;   // (an inactive lane carries the step's first entry)
        const int last = (int)min((int64_t)WAVE, o1 - b0) - 1;
        const int64_t i = tr_row_of(Cp, ilo, ihi, o);
        const int64_t r = R(i);
        const int64_t a0 = (int64_t)Ap[r];
        const int64_t q = o - (int64_t)Cp[i];
        int64_t e = a0 + q, u = 0;
        if (S) {
            const int64_t t = (int64_t)S[a0] + q;
            int64_t lo = a0, hi = (int64_t)Ap[r + 1] - 1;
            const int64_t i0 = __shfl((long long)i, 0, WAVE);
            if ((int64_t)Cp[i0 + 1] > b0 + last) {   // one output row: every source lies between the first's and the last's
                lo = ex_last_le(S, lo, hi, (int64_t)__shfl((long long)t, 0, WAVE));
                hi = ex_last_le(S, lo, hi, (int64_t)__shfl((long long)t, last, WAVE));
            }
            e = ex_last_le(S, lo, hi, t);
            u = t - (int64_t)S[e];
        }
        if (!active) continue;
        const int64_t j = Aj[e];
        int32_t col = (int32_t)j;
        if (K.mode == EX_RANGE) col = (int32_t)((j - K.start) / K.step);
        else if (K.mode == EX_LIST) col = K.colpos[(int64_t)K.colptr[j] + u].pos;
        Cj[o] = col;
        Cx[o] = Ax[e];
    }
}

}  // namespace spg
