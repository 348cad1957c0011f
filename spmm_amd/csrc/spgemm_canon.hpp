// spgemm_canon.hpp -- canonicalisation of CSR or COO input: spg_canonicalize_nnz /
// spg_canonicalize, the device form of scipy's coo_tocsr, csr_sort_indices, csr_sum_duplicates and
// csr_eliminate_zeros (cusparseXcsrsort, cusparseXcoosort and cusparseXcoo2csr as called by
// cupyx.cusparse.csrsort / coosort / coo2csr, modify_src/cupy-src/cupyx/cusparse.py:832-867,
// :908-954, :957-984, and the kernels behind cupyx's sum_duplicates and eliminate_zeros,
// modify_src/cupy-src/cupyx/scipy/sparse/_compressed.py:971-991, _csr.py:288-302,
// _coo.py:270-287, :356-400).
//
// A stable sort of (key, source position) records, key = row << cbits | column with cbits the
// bits of cols - 1: the least-significant-digit radix sort of spg_csr2csc (k_tr_hist, k_scan_lb,
// the ballot-rank placement tr_place) over the key's 8-bit digits, the column's bits first, then
// the row's.  The key is 32 bits wide when the bits of rows - 1 and of cols - 1 fit (two 65536s
// do), else 64, so a record is one 8- or 16-byte access and a pass moves nothing else; the pass
// count is the key's bits over 8, rounded up.  k_cn_pack makes the records from A (the column from
// A's indices, the row from the COO row array or a search of A's row pointer, the position the
// entry's own); the passes carry them through two ping-pong buffers.  Values never move through
// the passes: no sort kernel knows the value type.  COO input with no op is grouped by the passes
// over the row's bits alone (scipy's coo_tocsr order); CSR input with DROP_ZEROS alone is not
// sorted at all and its entries are their own records.
//
// After the sort, one lane per sorted entry:
//   k_cn_mark     kept[i] = 1 when entry i stays: under SUM when it heads its run (its key differs
//                 from its predecessor's), under DROP_ZEROS when its value -- its run's sum under
//                 SUM -- is not zero;
//   k_scan_lb     kept[] in place -> the exclusive prefix: a kept entry's place in C, the total nnz(C);
//   k_tr_indptr   C's row pointer off the sorted keys: kept[the first entry with a row >= r]
//                 (k_cn_indptr for unsorted CSR input: kept[Ap[r]]);
//   k_cn_fill     every kept entry writes its column and its value: the raw bits of A's value
//                 at its source position, and under SUM the run's later values added to it one by
//                 one in stored order (the sort is stable, so the sorted order of a run is its stored
//                 order).  The head's lane walks the whole run wherever it ends -- another wave's or
//                 another workgroup's entries included -- so a sum never depends on the launch
//                 geometry; a run of n entries is a loop of n - 1 adds in one lane, which is the rule.
// With SUM | DROP_ZEROS the sum is formed twice, in k_cn_mark to test it and in k_cn_fill to
// store it, instead of holding nnz values in the workspace between the two calls.
// No global atomic; every position is a function of the input alone.
//
// Every position is IP (the width A's indptr_type names) or CP (C's row pointer); K is the key type.
#pragma once

#include "spg_device.hpp"
#include "spgemm_transpose.hpp"

namespace spg {

constexpr int CN_BLOCK = 256;

// A sort record; 8 bytes for a 32-bit key and 32-bit positions, else 16.
template <typename IP, typename K>
struct alignas(sizeof(IP) + sizeof(K) == 8 ? 8 : 16) CnRec {
    K key;
    IP pos;
};

// The records' keys as k_tr_hist reads them, and their rows as k_tr_indptr searches them.
template <typename IP, typename K>
struct CnKeys {
    const CnRec<IP, K>* rec;
    int shift;   // 0: the whole key; cbits: the row
    __device__ __forceinline__ K operator()(int64_t e) const { return (K)(rec[e].key >> shift); }
};

// where k_cn_pack reads an entry's row from
constexpr int CN_FROM_CSR = 1;   // a search of Ap
constexpr int CN_FROM_COO = 2;   // the COO row array

// The records of A's entries in stored order: key = row << cbits | column, pos = the entry.
template <typename IP, typename K, int FROM>
__global__ __launch_bounds__(TR_WPB * WAVE) void k_cn_pack(int64_t nnz, int64_t chunks, int cbits,
                                                          const int32_t* __restrict__ Aj,
                                                          const int32_t* __restrict__ coo_rows,
                                                          const IP* __restrict__ Ap, int64_t rows,
                                                          CnRec<IP, K>* __restrict__ out) {
    const int l = lane_id();
    const int64_t chunk = (int64_t)blockIdx.x * TR_WPB + uniform((int)(threadIdx.x >> 6));
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    const int64_t e0 = chunk * TR_CHUNK, e1 = min(nnz, e0 + TR_CHUNK);
    int64_t rlo = 0, rhi = 0;   // rows of the chunk's first and last entry (wave-uniform)
    if (FROM == CN_FROM_CSR) {
        rlo = tr_row_of(Ap, 0, rows - 1, e0);
        rhi = tr_row_of(Ap, rlo, rows - 1, e1 - 1);
    }
    for (int64_t e = e0 + l; e < e1; e += WAVE) {
        const uint32_t row = FROM == CN_FROM_CSR ? (uint32_t)tr_row_of(Ap, rlo, rhi, e) : (uint32_t)coo_rows[e];
        CnRec<IP, K> r;
        r.key = ((K)row << cbits) | (K)(uint32_t)Aj[e];
        r.pos = (IP)e;
        out[e] = r;
    }
}

// One pass's scatter of the records by the digit at `shift` of their key.  table: the scanned
// histogram of the same digits (k_tr_hist over the same records).
template <typename IP, typename K>
__global__ __launch_bounds__(TR_WPB * WAVE) void k_cn_scatter(int64_t nnz, int64_t chunks, int shift,
                                                             const CnRec<IP, K>* __restrict__ in,
                                                             const IP* __restrict__ table,
                                                             CnRec<IP, K>* __restrict__ out) {
    __shared__ IP cur_s[TR_WPB][TR_RADIX];
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    const int64_t chunk = (int64_t)blockIdx.x * TR_WPB + wv;
    if (chunk >= chunks) return;   // (no workgroup barrier below)
    IP* cur = cur_s[wv];
    for (int d = l; d < TR_RADIX; d += WAVE) cur[d] = table[(int64_t)d * chunks + chunk];
    wsync();
    const int64_t e0 = chunk * TR_CHUNK, e1 = min(nnz, e0 + TR_CHUNK);
    for (int64_t b0 = e0; b0 < e1; b0 += WAVE) {
        const int64_t e = b0 + l;
        const bool active = e < e1;
        CnRec<IP, K> r;
        r.key = 0;
        r.pos = 0;
        if (active) r = in[e];
        const int64_t o = tr_place(active, tr_digit(r.key, shift), cur);
        if (active) out[o] = r;
    }
}

// The value of sorted entry i: A's value at its source position (rec == nullptr: i itself), the
// bits untouched; under SUM, i heading its run, the run's later values added in order.
template <typename IP, typename K, typename T, bool SUM>
__device__ __forceinline__ T cn_value(int64_t nnz, const CnRec<IP, K>* __restrict__ rec, const T* __restrict__ Ax,
                                      int64_t i) {
    T v = Ax[rec ? (int64_t)rec[i].pos : i];
    if constexpr (SUM) {
        const K key = rec[i].key;
        for (int64_t k = i + 1; k < nnz; ++k) {
            const CnRec<IP, K> r = rec[k];
            if (r.key != key) break;
            v = add_rn(v, Ax[(int64_t)r.pos]);
        }
    }
    return v;
}

// kept[i] of every sorted entry (see the head of the file).  T is not used without DROP.
template <typename IP, typename K, typename T, bool SUM, bool DROP>
__global__ __launch_bounds__(CN_BLOCK) void k_cn_mark(int64_t nnz, const CnRec<IP, K>* __restrict__ rec,
                                                     const T* __restrict__ Ax, IP* __restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * CN_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    bool keep = true;
    if constexpr (SUM) keep = i == 0 || rec[i].key != rec[i - 1].key;
    if constexpr (DROP) {
        if (keep) keep = cn_value<IP, K, T, SUM>(nnz, rec, Ax, i) != (T)0;
    }
    kept[i] = (IP)(keep ? 1 : 0);
}

// C's row pointer for unsorted CSR input (DROP_ZEROS alone): the kept entries before row r's first.
template <typename IP, typename CP>
__global__ __launch_bounds__(CN_BLOCK) void k_cn_indptr(int64_t rows, const IP* __restrict__ Ap,
                                                       const IP* __restrict__ kept, CP* __restrict__ Cp) {
    const int64_t r = (int64_t)blockIdx.x * CN_BLOCK + threadIdx.x;
    if (r <= rows) Cp[r] = (CP)kept[(int64_t)Ap[r]];
}

// C's indices and values.  kept: the scanned marks (nullptr: every entry stays where it is);
// rec == nullptr: unsorted CSR input, the columns are A's (Aj).  Without SUM, T is the raw-bit
// type of the value's width.
template <typename IP, typename K, typename T, bool SUM>
__global__ __launch_bounds__(CN_BLOCK) void k_cn_fill(int64_t nnz, const CnRec<IP, K>* __restrict__ rec, K cmask,
                                                     const int32_t* __restrict__ Aj, const T* __restrict__ Ax,
                                                     const IP* __restrict__ kept, int32_t* __restrict__ Cj,
                                                     T* __restrict__ Cx) {
    const int64_t i = (int64_t)blockIdx.x * CN_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    int64_t o = i;
    if (kept) {
        o = (int64_t)kept[i];
        if ((int64_t)kept[i + 1] == o) return;
    }
    Cj[o] = rec ? (int32_t)(rec[i].key & cmask) : Aj[i];
    Cx[o] = cn_value<IP, K, T, SUM>(nnz, rec, Ax, i);
}

}  // namespace spg
