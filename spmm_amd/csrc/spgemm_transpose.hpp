// spgemm_transpose.hpp -- AT = A^T as CSR (A in CSC): spg_csr2csc, the device form of scipy's
// csr_tocsc (cusparseCsr2cscEx2 as called by cupyx.cusparse.csr2csc,
// modify_src/cupy-src/cupyx/cusparse.py:1014-1065).
//
// A stable counting sort of A's entries by column: the entries of output row j keep A's stored
// (row-major) order, duplicates and unsorted rows included, which is exactly what scipy's
// tocsc() gives.  Values are moved as raw bits (integer loads and stores of their width), so NaN
// signs and payloads, +-0, denormals and +-inf arrive unchanged.
//
// The sort is a least-significant-digit radix sort over 8-bit digits of the column index, with
// as many passes as cols - 1 has bytes (<= 256 columns: one, <= 65536: two, ...).  A pass is
//   k_tr_hist     one wave per contiguous chunk of TR_CHUNK entries: a 256-bin digit histogram in
//                 the wave's LDS (integer adds: a count does not depend on their order) into the
//                 digit-major table[digit][chunk];
//   k_scan_lb     the table in place -> the first output position of every (digit, chunk);
//   k_tr_scatter  the same wave walks the same chunk 64 entries at a time.  A lane's rank among
//                 the lanes with its digit comes from eight ballots (the peer mask, AND-ed bit by
//                 bit) and a popcount of the peers below it; the wave's LDS cursor of that digit
//                 gives the base and the lowest peer bumps it by the peer count.
// The last pass also leaves the sorted columns in the workspace, and k_tr_indptr reads AT's row
// pointer off them: indptr[c] = the number of entries with a column below c, a binary search per
// column.  No global atomic anywhere (per-entry device-scope counting atomics cost 0.82 ms of a
// 2.7 ms transpose on config 4's A).
// Stable by construction: equal digits are placed by (chunk, batch of 64, lane) ascending, i.e.
// in the order the pass read them; no position depends on when an LDS add landed.
//
// A record is (column, source row, source position).  The first pass reads the columns from A
// and finds each entry's row by a search of A's row pointer between the chunk's first and last
// row; later passes carry the three fields through two ping-pong buffers.  The last pass writes
// AT's indices (the source row) and gathers every value once from its source position (one
// 16-byte access for complex128) instead of moving values through the passes.
//
// Every position is IP (the row-pointer type): the int64 instantiation carries 64-bit entry
// positions in the table, the cursors and the records.
#pragma once

#include "spg_device.hpp"
#include "spg_format_layouts.hpp"   // TR_CHUNK (entries per wave chunk), TR_RADIX (8-bit digits)

namespace spg {

constexpr int TR_WPB = 4;                          // waves per workgroup
constexpr int TR_BLOCK_ENTRIES = TR_WPB * TR_CHUNK;   // entries per workgroup (8192)

// Raw bits of a value: 4, 8 or 16 bytes.  (8-byte alignment: a complex128 array is only promised
// its component's alignment; gfx950 takes the 16 bytes as one access all the same.)
struct alignas(8) TrBits16 { uint64_t lo, hi; };
template <int BYTES> struct TrBits;
template <> struct TrBits<4> { using type = uint32_t; };
template <> struct TrBits<8> { using type = uint64_t; };
template <> struct TrBits<16> { using type = TrBits16; };

__device__ __forceinline__ int tr_digit(int32_t key, int shift) { return (int)(((uint32_t)key >> shift) & 255u); }
__device__ __forceinline__ int tr_digit(uint32_t key, int shift) { return (int)((key >> shift) & 255u); }
__device__ __forceinline__ int tr_digit(uint64_t key, int shift) { return (int)((key >> shift) & 255u); }

// Where a pass's keys come from: a plain array of column indices (spg_csr2csc); the sort records
// of spg_canonicalize are another (CnKeys).  KS(e) is entry e's key.
struct TrKeys {
    const int32_t* keys;
    __device__ __forceinline__ uint32_t operator()(int64_t e) const { return (uint32_t)keys[e]; }
};

// The row of entry e: the last r in [lo, hi] with Ap[r] <= e (Ap[lo] <= e; empty rows skipped).
template <typename IP>
__device__ __forceinline__ int64_t tr_row_of(const IP* __restrict__ Ap, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)Ap[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Digit histogram of every chunk into table[digit * chunks + chunk].
template <typename IP, typename KS = TrKeys>
__global__ __launch_bounds__(TR_WPB * WAVE) void k_tr_hist(int64_t nnz, int64_t chunks, KS keys, int shift,
                                                          IP* __restrict__ table) {
    __shared__ uint32_t hist_s[TR_WPB][TR_RADIX];
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    const int64_t chunk = (int64_t)blockIdx.x * TR_WPB + wv;
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    uint32_t* hist = hist_s[wv];
    for (int d = l; d < TR_RADIX; d += WAVE) hist[d] = 0;
    wsync();
    const int64_t e0 = chunk * TR_CHUNK, e1 = min(nnz, e0 + TR_CHUNK);
    for (int64_t e = e0 + l; e < e1; e += WAVE) atomicAdd(&hist[tr_digit(keys(e), shift)], 1u);
    wsync();
    for (int d = l; d < TR_RADIX; d += WAVE) table[(int64_t)d * chunks + chunk] = (IP)hist[d];
}

// The ballot-rank placement of one batch of 64 records (every lane of the wave calls it): the
// output position of this lane's record with digit d -- the wave's LDS cursor of that digit plus
// the lane's rank among the active lanes with the same digit -- and the cursor moved past them.
template <typename IP>
__device__ __forceinline__ int64_t tr_place(bool active, int d, IP* cur) {
    unsigned long long peers = __ballot(active);   // active lanes with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long m = __ballot(active && bit);
        peers &= bit ? m : ~m;
    }
    const int rank = lane_rank(peers);
    const IP base = active ? cur[d] : (IP)0;
    wsync();
    if (active && rank == 0) cur[d] = base + (IP)__popcll(peers);
    wsync();
    return (int64_t)base + rank;
}

// One pass's scatter.  table: the scanned histogram.  FIRST: records come from A (kin = A's
// indices, Ap / rows for the row search); otherwise from (kin, rin, pin).  LAST: AT's indices and
// values are written (Ax gathered by source position) and kout takes the sorted columns; otherwise
// the records go to (kout, rout, pout).
template <typename IP, typename V, bool FIRST, bool LAST>
__global__ __launch_bounds__(TR_WPB * WAVE) void k_tr_scatter(int64_t nnz, int64_t chunks, int shift,
                                                             const int32_t* __restrict__ kin,
                                                             const int32_t* __restrict__ rin,
                                                             const IP* __restrict__ pin,
                                                             const IP* __restrict__ Ap, int64_t rows,
                                                             const IP* __restrict__ table,
                                                             int32_t* __restrict__ kout, int32_t* __restrict__ rout,
                                                             IP* __restrict__ pout, const V* __restrict__ Ax,
                                                             int32_t* __restrict__ ATj, V* __restrict__ ATx) {
    __shared__ IP cur_s[TR_WPB][TR_RADIX];
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    const int64_t chunk = (int64_t)blockIdx.x * TR_WPB + wv;
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    IP* cur = cur_s[wv];
    for (int d = l; d < TR_RADIX; d += WAVE) cur[d] = table[(int64_t)d * chunks + chunk];
    wsync();
    const int64_t e0 = chunk * TR_CHUNK, e1 = min(nnz, e0 + TR_CHUNK);
    int64_t rlo = 0, rhi = 0;   // rows of the chunk's first and last entry (wave-uniform)
    if (FIRST) {
        rlo = tr_row_of(Ap, 0, rows - 1, e0);
        rhi = tr_row_of(Ap, rlo, rows - 1, e1 - 1);
    }
    for (int64_t b0 = e0; b0 < e1; b0 += WAVE) {
        const int64_t e = b0 + l;
        const bool active = e < e1;
        int32_t key = 0, row = 0;
        IP pos = 0;
        if (active) {
            key = kin[e];
            if (FIRST) {
                row = (int32_t)tr_row_of(Ap, rlo, rhi, e);
                pos = (IP)e;
            } else {
                row = rin[e];
                pos = pin[e];
            }
        }
        const int64_t o = tr_place(active, tr_digit(key, shift), cur);
        if (active) {
            if (LAST) {
                kout[o] = key;
                ATj[o] = row;
                ATx[o] = Ax[(int64_t)pos];
            } else {
                kout[o] = key;
                rout[o] = row;
                pout[o] = pos;
            }
        }
    }
}

// AT's row pointer from the sorted columns: indptr[c] = the number of entries whose column is
// below c, for every c in [0, cols] (columns compare as the unsigned numbers the digits sorted).
// With `kept` (spg_canonicalize_nnz: the exclusive prefix of the kept marks over the sorted
// entries) the count is of kept entries only, kept[that number].
template <typename IP, typename OUT = IP, typename KS = TrKeys>
__global__ __launch_bounds__(256) void k_tr_indptr(int64_t nnz, int64_t cols, KS skeys,
                                                 OUT* __restrict__ ATp, const IP* __restrict__ kept) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= cols; c += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = nnz;   // the first entry with a column >= c
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)skeys(mid) < c) lo = mid + 1;
            else hi = mid;
        }
        ATp[c] = (OUT)(kept ? (int64_t)kept[lo] : lo);
    }
}

}  // namespace spg
