// spgemm_binop.hpp -- element-wise C = op(A, B), op in {multiply, maximum, minimum}, for canonical
// CSR operands: spg_csr_binop_nnz / spg_csr_binop, the device form of scipy's
// csr_binop_csr_canonical (cupyx's csr_matrix.multiply and _maximum_minimum,
// cupy-src/cupyx/scipy/sparse/_csr.py:328-342 and :297-326, with its kernels multiply_by_csr
// :733-835 and binopt_csr :880-945); and out = A.values * D(i, j) per stored entry of A:
// spg_csr_mul_dense (multiply_by_dense, _csr.py:617-718).
//
// The addition's walk (spgemm_geam.hpp: flat over the stored entries, one lane per entry, a wave
// per chunk of GM_CHUNK entries, partners by windowed binary search) with one difference: which
// entries C holds depends on the values.  Over the union of the two patterns r = op(a, b), the
// operand without the entry contributing +0, and (column, r) is kept iff r != 0.
//
//   k_bo_mark   one lane per A entry e: KA[e] = keep(op(a_e, b or 0)); one lane per B entry j:
//               KB[j] = A's row lacks j's column && keep(op(0, b_j));
//   k_scan_lb   KA and KB in place -> SA, SB, the exclusive prefixes (nnz + 1 entries each, the
//               last the total);
//   k_bo_count  per row: SA[Ap[r+1]] - SA[Ap[r]] + SB[Bp[r+1]] - SB[Bp[r]];
//   k_scan_lb   the counts -> C's row pointer, the total -> nnz(C);
//   k_bo_fill   a kept A entry e of row r, with lb its column's lower bound in B's row, goes to
//               Cp[r] + (SA[e] - SA[Ap[r]]) + (SB[Bp[r] + lb] - SB[Bp[r]]) -- the kept A entries
//               and the kept B-only entries left of it; a kept B-only entry j goes to
//               Cp[r] + (SB[j] - SB[Bp[r]]) + (SA[Ap[r] + la] - SA[Ap[r]]), la its column's lower
//               bound in A's row.
// Every position is a function of the scanned marks alone: no atomic, nothing depends on the
// order in which anything lands, results are identical from run to run, C's columns ascend.
// Whether the fill stores an entry is read off the marks (SA[e + 1] != SA[e]), so it writes
// exactly the positions the structure pass counted; the value it stores is bo_apply again, the
// function the mark pass tested.
//
// keep: r != 0 decided on the integer bits, spg_dense2csr's test (spgemm_dense.hpp): +-0 dropped,
// denormals, +-inf and NaN kept, a complex value dropped only when both parts are +-0.
//
// Every entry position is IP (the operands' row-pointer type) or CP (C's): the int64
// instantiations carry 64-bit positions in SA, SB and in C's row pointer.
#pragma once

#include "spg_device.hpp"
#include "spg_format_layouts.hpp"
#include "spgemm_geam.hpp"   // gm_walk, gm_find, GM_WPB

namespace spg {

constexpr int BO_MUL = 0, BO_MAX = 1, BO_MIN = 2;   // spg_binop_t's numbers

// x < y: IEEE for the real types (false with a NaN on either side), scipy's lexicographic
// order of complex_wrapper for the complex ones.
__device__ __forceinline__ bool bo_less(float x, float y) { return x < y; }
__device__ __forceinline__ bool bo_less(double x, double y) { return x < y; }
template <typename R> __device__ __forceinline__ bool bo_less(cplx<R> x, cplx<R> y) {
    return x.re == y.re ? x.im < y.im : x.re < y.re;
}

// r = op(a, b).  MUL: one rounded product (complex: (ac - bd) + (ad + bc)i, each product and sum
// rounded on its own).  MAX: a < b ? b : a, MIN: b < a ? b : a -- one operand moved bit for bit.
template <typename T>
__device__ __forceinline__ T bo_apply(int op, T a, T b) {
    if (op == BO_MUL) return mul_rn(a, b);
    if (op == BO_MAX) return bo_less(a, b) ? b : a;
    return bo_less(b, a) ? b : a;
}

// r != 0 on the bits without their sign(s)
__device__ __forceinline__ bool bo_keep(float r) { return (__float_as_uint(r) & 0x7fffffffu) != 0; }
__device__ __forceinline__ bool bo_keep(double r) {
    return ((unsigned long long)__double_as_longlong(r) & 0x7fffffffffffffffull) != 0;
}
template <typename R> __device__ __forceinline__ bool bo_keep(cplx<R> r) { return bo_keep(r.re) || bo_keep(r.im); }

// The marks.  Chunks [0, chunksA) walk A's entries, [chunksA, chunksA + chunksB) B's.
template <typename IP, typename T>
__global__ __launch_bounds__(GM_WPB * WAVE) void k_bo_mark(int op, int64_t rows, int64_t nnzA, int64_t chunksA,
                                                          int64_t nnzB, int64_t chunksB,
                                                          const IP* __restrict__ Ap,
                                                          const int32_t* __restrict__ Aj,
                                                          const T* __restrict__ Ax, const IP* __restrict__ Bp,
                                                          const int32_t* __restrict__ Bj,
                                                          const T* __restrict__ Bx, IP* __restrict__ KA,
                                                          IP* __restrict__ KB) {
    const int64_t chunk = (int64_t)blockIdx.x * GM_WPB + (threadIdx.x >> 6);
    if (chunk >= chunksA + chunksB) return;   // (no workgroup barrier below)
    if (chunk < chunksA) {
        gm_walk(nnzA, chunk, Ap, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const int32_t col = active ? Aj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Bp, Bj, r, col, one_row, last, end);
            if (!active) return;
            T b = (T)0;   // (the operand without the entry is +0)
            if (p < end && Bj[p] == col) b = Bx[p];
            KA[e] = (IP)(bo_keep(bo_apply(op, Ax[e], b)) ? 1 : 0);
        });
    } else {
        gm_walk(nnzB, chunk - chunksA, Bp, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const int32_t col = active ? Bj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Ap, Aj, r, col, one_row, last, end);
            if (!active) return;
            const bool only = !(p < end && Aj[p] == col);
            KB[e] = (IP)((only && bo_keep(bo_apply(op, (T)0, Bx[e]))) ? 1 : 0);
        });
    }
}

// Entries of C's row r: the kept ones of A's row plus the kept B-only ones.
template <typename IP>
__global__ __launch_bounds__(256) void k_bo_count(int64_t rows, const IP* __restrict__ Ap,
                                                const IP* __restrict__ Bp, const IP* __restrict__ SA,
                                                const IP* __restrict__ SB, int64_t* __restrict__ cnt) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
        cnt[r] = ((int64_t)SA[Ap[r + 1]] - (int64_t)SA[Ap[r]]) + ((int64_t)SB[Bp[r + 1]] - (int64_t)SB[Bp[r]]);
}

// C's indices and values.  Chunks as in k_bo_mark.
template <typename IP, typename CP, typename T>
__global__ __launch_bounds__(GM_WPB * WAVE) void k_bo_fill(int op, int64_t rows, int64_t nnzA, int64_t chunksA,
                                                          int64_t nnzB, int64_t chunksB,
                                                          const IP* __restrict__ Ap,
                                                          const int32_t* __restrict__ Aj,
                                                          const T* __restrict__ Ax, const IP* __restrict__ Bp,
                                                          const int32_t* __restrict__ Bj,
                                                          const T* __restrict__ Bx, const IP* __restrict__ SA,
                                                          const IP* __restrict__ SB, const CP* __restrict__ Cp,
                                                          int32_t* __restrict__ Cj, T* __restrict__ Cx) {
    const int64_t chunk = (int64_t)blockIdx.x * GM_WPB + (threadIdx.x >> 6);
    if (chunk >= chunksA + chunksB) return;   // (no workgroup barrier below)
    if (chunk < chunksA) {
        gm_walk(nnzA, chunk, Ap, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const bool mine = active && SA[e + 1] != SA[e];   // kept
            if (__ballot(mine) == 0) return;
            const int32_t col = active ? Aj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Bp, Bj, r, col, one_row, last, end);
            if (!mine) return;
            T b = (T)0;
            if (p < end && Bj[p] == col) b = Bx[p];
            const int64_t o = (int64_t)Cp[r] + ((int64_t)SA[e] - (int64_t)SA[Ap[r]]) +
                              ((int64_t)SB[p] - (int64_t)SB[Bp[r]]);
            Cj[o] = col;
            Cx[o] = bo_apply(op, Ax[e], b);
        });
    } else {
        gm_walk(nnzB, chunk - chunksA, Bp, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const bool mine = active && SB[e + 1] != SB[e];   // B-only and kept
            if (__ballot(mine) == 0) return;
            const int32_t col = active ? Bj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Ap, Aj, r, col, one_row, last, end);
            if (!mine) return;
            const int64_t o = (int64_t)Cp[r] + ((int64_t)SB[e] - (int64_t)SB[Bp[r]]) +
                              ((int64_t)SA[p] - (int64_t)SA[Ap[r]]);
            Cj[o] = col;
            Cx[o] = bo_apply(op, (T)0, Bx[e]);
        });
    }
}

// out[e] = A.values[e] * D(row of e, Aj[e]).  sr / sc: elements between consecutive rows / columns
// of D, 0 along an axis of extent 1 (broadcast: its index reads element 0).  A need not be
// canonical: the row comes from the row pointer alone.  out may be A's values themselves (each
// lane reads its entry before it writes it).
template <typename IP, typename T>
__global__ __launch_bounds__(GM_WPB * WAVE) void k_bo_mul_dense(int64_t rows, int64_t nnz, int64_t chunks,
                                                               const IP* __restrict__ Ap,
                                                               const int32_t* __restrict__ Aj, const T* Ax,
                                                               const T* __restrict__ D, int64_t sr, int64_t sc,
                                                               T* out) {
    const int64_t chunk = (int64_t)blockIdx.x * GM_WPB + (threadIdx.x >> 6);
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    gm_walk(nnz, chunk, Ap, rows, [&](int64_t e, int64_t r, bool active, bool, int) {
        if (!active) return;
        out[e] = mul_rn(Ax[e], D[r * sr + (int64_t)Aj[e] * sc]);
    });
}

}  // namespace spg
