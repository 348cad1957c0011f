// spgemm_geam.hpp -- C = alpha*A + beta*B for canonical CSR operands: spg_csrgeam_nnz /
// spg_csrgeam, the device form of scipy's csr_plus_csr / csr_minus_csr (cusparseXcsrgeam2Nnz and
// cusparse<t>csrgeam2 as called by cupyx.cusparse.csrgeam2,
// modify_src/cupy-src/cupyx/cusparse.py:525-591).
//
// Flat over the stored entries: one lane per entry, 64 consecutive entries per step, one wave per
// contiguous chunk of GM_CHUNK entries, so a row of 50,000 entries spreads over as many waves as
// 50,000 entries of short rows do.  A lane finds its row by a search of the row pointer between
// the rows of its chunk's first and last entry, and its column in the OTHER matrix's row by binary
// search.  When a step's 64 entries lie in one row their targets lie in a narrow window of the
// other row: the window is bounded once per step from the step's first and last column (two
// searches every lane makes alike), and each lane searches only inside it.
//
//   k_geam_mark   one lane per B entry j: only[j] = 1 when A's row has no entry in j's column;
//   k_scan_lb     `only` in place -> S, the exclusive prefix (nnz(B) + 1 entries, the last the total);
//   k_geam_count  per row: len(A row) + S[Bp[r+1]] - S[Bp[r]];
//   k_scan_lb     the counts -> C's row pointer, the total -> nnz(C);
//   k_geam_fill   A's entry i of row r, with lb its column's lower bound in B's row, goes to
//                 Cp[r] + i + (S[Bp[r] + lb] - S[Bp[r]]) -- the B-only entries left of it -- and
//                 adds B's value when B has the column; a B-only entry j goes to
//                 Cp[r] + (S[j] - S[Bp[r]]) + (its column's lower bound in A's row).
// Every position is a function of the two structures alone: no atomic, nothing depends on the
// order in which anything lands, results are identical from run to run, C's columns ascend.
//
// Values: va = alpha == 1 ? a : alpha * a, vb likewise, va + vb where both patterns have the
// entry, va + 0 and 0 + vb elsewhere (scipy's binary op adds the missing operand as +0, which
// turns a -0.0 component into +0.0), every operation separately rounded (mul_rn / add_rn).  The
// pair (1, -1) is the subtraction A - B, scipy's csr_minus_csr: a - b, a - 0 and 0 - b part by
// part, formed as a + (-b) with the sign flipped and no product (a complex product with (-1, 0)
// would turn an infinite part of b into a NaN in its other part).  No shortcut on a value:
// beta == 0 still walks B and gives 0 * inf = NaN.
//
// Every entry position is IP (the operands' row-pointer type) or CP (C's): the int64
// instantiations carry 64-bit positions in S and in C's row pointer.
#pragma once

#include "spg_device.hpp"
#include "spg_format_layouts.hpp"   // GM_CHUNK (entries per wave chunk)
#include "spgemm_transpose.hpp"     // tr_row_of

namespace spg {

constexpr int GM_WPB = 4;                            // waves per workgroup

// The first position in [lo, hi) of Xj whose column is >= col (hi when there is none).
__device__ __forceinline__ int64_t gm_lower_bound(const int32_t* __restrict__ Xj, int64_t lo, int64_t hi,
                                                  int32_t col) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (Xj[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Walks chunk `chunk` of M's entries 64 at a time and calls f(e, r, active, one_row, last) in
// every lane: e the lane's entry, r its row, active whether e is inside the chunk (an inactive
// lane carries the step's first row, so r is always a valid row), one_row (wave-uniform) whether
// all the step's entries lie in one row, last the step's last active lane.
template <typename IP, typename F>
__device__ __forceinline__ void gm_walk(int64_t nnz, int64_t chunk, const IP* __restrict__ Mp, int64_t rows, F&& f) {
    const int l = lane_id();
    const int64_t e0 = chunk * GM_CHUNK, e1 = min(nnz, e0 + GM_CHUNK);
    const int64_t rlo = tr_row_of(Mp, 0, rows - 1, e0);       // rows of the chunk's first and
    const int64_t rhi = tr_row_of(Mp, rlo, rows - 1, e1 - 1);   // last entry (wave-uniform)
    for (int64_t b0 = e0; b0 < e1; b0 += WAVE) {
        const int64_t e = b0 + l;
        const bool active = e < e1;
        const int last = (int)min((int64_t)WAVE, e1 - b0) - 1;
        const int64_t r = tr_row_of(Mp, rlo, rhi, active ? e : b0);
        const int64_t r0 = __shfl((long long)r, 0, WAVE);
        const bool one_row = (int64_t)Mp[r0 + 1] > b0 + last;
        f(e, r, active, one_row, last);
    }
}

// Lower bound of the lane's column in row r of X (an absolute position in [Xp[r], end], end =
// Xp[r + 1]).  Called by all 64 lanes; one_row / last as gm_walk gives them.
template <typename IP>
__device__ __forceinline__ int64_t gm_find(const IP* __restrict__ Xp, const int32_t* __restrict__ Xj, int64_t r,
                                           int32_t col, bool one_row, int last, int64_t& end) {
    int64_t lo = (int64_t)Xp[r], hi = end = (int64_t)Xp[r + 1];
    if (one_row) {   // the step's columns ascend: every target lies between the first's and the last's
        lo = gm_lower_bound(Xj, lo, end, __shfl(col, 0, WAVE));
        hi = gm_lower_bound(Xj, lo, end, __shfl(col, last, WAVE));
    }
    return gm_lower_bound(Xj, lo, hi, col);
}

// -x: the sign of every part flipped, exactly.
__device__ __forceinline__ float gm_neg(float x) { return -x; }
__device__ __forceinline__ double gm_neg(double x) { return -x; }
template <typename R> __device__ __forceinline__ cplx<R> gm_neg(cplx<R> x) { return cplx<R>(-x.re, -x.im); }

// vb of B's value b: b, -b (the subtraction A - B) or beta * b.
template <typename T>
__device__ __forceinline__ T gm_scaled(T b, T beta, bool b_one, bool minus) {
    return b_one ? b : minus ? gm_neg(b) : mul_rn(beta, b);
}

// only[j] = 1 when B's entry j has no partner in A's row, else 0.
template <typename IP>
__global__ __launch_bounds__(GM_WPB * WAVE) void k_geam_mark(int64_t rows, int64_t nnzB, int64_t chunks,
                                                            const IP* __restrict__ Ap,
                                                            const int32_t* __restrict__ Aj,
                                                            const IP* __restrict__ Bp,
                                                            const int32_t* __restrict__ Bj, IP* __restrict__ only) {
    const int64_t chunk = (int64_t)blockIdx.x * GM_WPB + (threadIdx.x >> 6);
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    gm_walk(nnzB, chunk, Bp, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
        const int32_t col = active ? Bj[e] : 0;
        int64_t end;
        const int64_t p = gm_find(Ap, Aj, r, col, one_row, last, end);
        if (active) only[e] = (IP)((p < end && Aj[p] == col) ? 0 : 1);
    });
}

// Entries of C's row r: A's plus the B-only ones.
template <typename IP>
__global__ __launch_bounds__(256) void k_geam_count(int64_t rows, const IP* __restrict__ Ap,
                                                  const IP* __restrict__ Bp, const IP* __restrict__ S,
                                                  int64_t* __restrict__ cnt) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256)
        cnt[r] = ((int64_t)Ap[r + 1] - (int64_t)Ap[r]) + ((int64_t)S[Bp[r + 1]] - (int64_t)S[Bp[r]]);
}

// C's indices and values.  Chunks [0, chunksA) walk A's entries, [chunksA, chunksA + chunksB) B's.
template <typename IP, typename CP, typename T>
__global__ __launch_bounds__(GM_WPB * WAVE) void k_geam_fill(int64_t rows, int64_t nnzA, int64_t chunksA,
                                                            int64_t nnzB, int64_t chunksB,
                                                            const IP* __restrict__ Ap,
                                                            const int32_t* __restrict__ Aj,
                                                            const T* __restrict__ Ax, const IP* __restrict__ Bp,
                                                            const int32_t* __restrict__ Bj,
                                                            const T* __restrict__ Bx, const IP* __restrict__ S,
                                                            const CP* __restrict__ Cp, int32_t* __restrict__ Cj,
                                                            T* __restrict__ Cx, T alpha, T beta) {
    const int64_t chunk = (int64_t)blockIdx.x * GM_WPB + (threadIdx.x >> 6);
    if (chunk >= chunksA + chunksB) return;   // (no workgroup barrier below)
    const bool a_one = alpha == (T)1, b_one = beta == (T)1;
    const bool minus = a_one && beta == gm_neg((T)1);   // A - B: vb = -b, the sign flipped, no product
    const T b_none = minus ? gm_neg((T)0) : (T)0;       // B's value where it has no entry: a - 0 is a + (-0)
    if (chunk < chunksA) {
        gm_walk(nnzA, chunk, Ap, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const int32_t col = active ? Aj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Bp, Bj, r, col, one_row, last, end);
            if (!active) return;
            T v = Ax[e];
            if (!a_one) v = mul_rn(alpha, v);
            T w = b_none;   // (an A-only entry is va + 0, as in scipy: a -0.0 component becomes +0.0)
            if (p < end && Bj[p] == col) w = gm_scaled(Bx[p], beta, b_one, minus);
            v = add_rn(v, w);
            const int64_t o = (int64_t)Cp[r] + (e - (int64_t)Ap[r]) + ((int64_t)S[p] - (int64_t)S[Bp[r]]);
            Cj[o] = col;
            Cx[o] = v;
        });
    } else {
        gm_walk(nnzB, chunk - chunksA, Bp, rows, [&](int64_t e, int64_t r, bool active, bool one_row, int last) {
            const bool mine = active && S[e + 1] != S[e];   // B-only
            if (__ballot(mine) == 0) return;
            const int32_t col = active ? Bj[e] : 0;
            int64_t end;
            const int64_t p = gm_find(Ap, Aj, r, col, one_row, last, end);
            if (!mine) return;
            const T w = add_rn((T)0, gm_scaled(Bx[e], beta, b_one, minus));
            const int64_t o = (int64_t)Cp[r] + ((int64_t)S[e] - (int64_t)S[Bp[r]]) + (p - (int64_t)Ap[r]);
            Cj[o] = col;
            Cx[o] = w;
        });
    }
}

}  // namespace spg
