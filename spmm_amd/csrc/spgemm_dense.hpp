// spgemm_dense.hpp -- the dense boundary: spg_csr2dense (scipy's csr_todense, A.toarray()) and
// spg_dense2csr_nnz / spg_dense2csr (scipy's csr_matrix(D)).  (cusparse csr2dense / dense2csr and
// cusparseSparseToDense / cusparseDenseToSparse as called by cupyx.cusparse,
// modify_src/cupy-src/cupyx/cusparse.py:768, :800, :1146, :1188, :1733, :1805; cupyx's own
// kernels, modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:383-428 and :1158-1210.)
//
// csr2dense.  Both are bandwidth-bound; the compulsory traffic here is one write of D.  A memset
// pass plus a scatter of 4..16-byte global stores would write D twice, the second time a sector
// per entry.  Instead a workgroup owns a band of DV_R rows x a window of DV_W columns in LDS:
//   - one wave owns a row of the window (wave w the rows w, w + 4, ...): it zeroes the row in
//     LDS, walks the row's stored entries 64 at a time in stored order and adds those whose
//     column lies in the window;
//   - two entries of one batch with the same column are found with the ballot peer mask (as
//     tr_place does for digits) and applied in rank rounds: round r is the lanes of rank r, a
//     plain LDS read-add-write.  A batch without duplicates -- every batch of a canonical row --
//     is one round; no add's position in the sum depends on timing, so every element is
//     0 + v1 + v2 + ... in stored order, each add separately rounded: scipy's loop;
//   - the window then streams out: row-major with 16-byte stores when D's base and ld * sizeof
//     are multiples of 16 (spg_spmm's rule), element by element otherwise; column-major as the
//     same tile read transposed, each column's run of the band's rows contiguous.
// A row wider than one window is walked once per window, entries outside it skipped.  An LDS row
// is DV_W + DV_PAD elements: the pad keeps rows 16-byte aligned and spreads the transposed read
// (8 rows x 8 columns per wave) over the 32 banks, 2 lanes per bank, the least 64 lanes can have.
// complex128: 8 x 520 x 16 B = 65 KiB per workgroup, two per CU.
//
// dense2csr.  Compulsory traffic is two reads of D and one write of C.  Every row is cut into
// segments of DV_S columns:
//   k_dn_count   one count per (row, segment) into a row-major table: a ballot and a popcount per
//                64 elements;
//   k_scan_lb    the table in place -> every segment's first output position (and the total);
//   k_dn_indptr  C's row pointer: the first segment of every row, then the total;
//   k_dn_fill    re-reads the segment and places each kept element at base + lane_rank(ballot),
//                so columns ascend by construction and no position depends on timing.
// A 1 x 10^6 matrix gets as many waves as 1024 x 1024.  Row-major D is read with 16-byte loads
// under the alignment rule above (a lane then holds 16 / sizeof consecutive elements; its rank is
// the sum of the per-element ballots' ranks).  Column-major D is read as 64 x 64 tiles transposed
// through LDS (65-element rows: no bank conflict either way), so global reads run along columns;
// a workgroup owns 64 rows x one segment and wave w the rows 16w .. 16w + 15, lane k keeping row
// k's running position.
// An element is kept iff its bits, sign bit(s) masked off, are nonzero -- value != 0 decided on
// the integers, so no float mode can flush a denormal: +-0 dropped, denormals, +-inf and NaN
// kept, a complex value dropped only when both parts are +-0.  Kept values are moved as raw
// bits (NaN sign and payload included), the transpose's rule.
// Positions are CP (C's row-pointer type): the int64 instantiation carries 64-bit positions.
#pragma once

#include "spg_device.hpp"
#include "spg_format_layouts.hpp"   // DV_S, DV_T
#include "spgemm_transpose.hpp"     // TrBits16

namespace spg {

constexpr int DV_WPB = 4;       // waves per workgroup
constexpr int DV_W = 512;       // csr2dense: columns of the LDS window
constexpr int DV_R = 8;         // csr2dense: rows of the band
constexpr int DV_PAD = 8;       // csr2dense: pad elements of an LDS row
constexpr int DV_WBITS = 9;     // bits of a column inside the window
// (DV_S, dense2csr's columns per segment, and DV_T, its column-major tile edge: spg_format_layouts.hpp)
constexpr int DV_RPW = DV_T / DV_WPB;   // dense2csr, column-major: rows per wave (16)
static_assert((1 << DV_WBITS) == DV_W, "window bits");
static_assert(DV_S % (WAVE * 4) == 0, "a segment starts on a 16-byte chunk for every value type");

// 16 raw bytes (may alias any value type)
typedef uint32_t dn_vec __attribute__((ext_vector_type(4), may_alias));

// Raw bits of a value and the keep rule (value != 0 on the integers).
template <typename T> struct DnBits;
template <> struct DnBits<float> {
    using type = uint32_t;
    static __device__ __forceinline__ bool keep(type b) { return (b & 0x7fffffffu) != 0; }
};
template <> struct DnBits<double> {
    using type = uint64_t;
    static __device__ __forceinline__ bool keep(type b) { return (b & 0x7fffffffffffffffull) != 0; }
};
template <> struct DnBits<cplx<float>> {
    using type = uint64_t;
    static __device__ __forceinline__ bool keep(type b) { return (b & 0x7fffffff7fffffffull) != 0; }
};
template <> struct DnBits<cplx<double>> {
    using type = TrBits16;
    static __device__ __forceinline__ bool keep(type b) { return ((b.lo | b.hi) & 0x7fffffffffffffffull) != 0; }
};

// ----------------------------------------------------------------------------- csr2dense
// Tile t = band * wins + win (windows fastest: neighbouring workgroups re-read the same rows'
// entries from L2).  COL: D is column-major.  VEC: 16-byte stores (row-major only).
template <typename T, typename IP, bool COL, bool VEC>
__global__ __launch_bounds__(DV_WPB * WAVE) void k_csr2dense(int64_t rows, int64_t cols, int64_t wins,
                                                            int64_t tiles, const IP* __restrict__ Ap,
                                                            const int32_t* __restrict__ Aj,
                                                            const T* __restrict__ Ax, T* __restrict__ D,
                                                            int64_t ld) {
    __shared__ __attribute__((aligned(16))) T tile[DV_R][DV_W + DV_PAD];
    constexpr int E = 16 / (int)sizeof(T);   // elements per 16 bytes
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t band = t / wins, win = t - band * wins;
        const int64_t r0 = band * DV_R, c0 = win * DV_W;
        const int nr = (int)min((int64_t)DV_R, rows - r0), nc = (int)min((int64_t)DV_W, cols - c0);
        for (int rr = wv; rr < nr; rr += DV_WPB) {
            T* acc = tile[rr];
            for (int c = l; c < nc; c += WAVE) acc[c] = T(0);
            wsync();
            const int64_t e0 = (int64_t)Ap[r0 + rr], e1 = (int64_t)Ap[r0 + rr + 1];
            for (int64_t b0 = e0; b0 < e1; b0 += WAVE) {
                const int64_t e = b0 + l;
                const bool active = e < e1;
                const int64_t rel64 = active ? (int64_t)Aj[e] - c0 : -1;
                const bool in = rel64 >= 0 && rel64 < nc;
                const unsigned long long any = __ballot(in);
                if (any == 0) continue;
                const int rel = in ? (int)rel64 : 0;
                unsigned long long peers = any;   // the in-window lanes with this lane's column
#pragma unroll
                for (int b = 0; b < DV_WBITS; ++b) {
                    const bool bit = (rel >> b) & 1;
                    const unsigned long long m = __ballot(in && bit);
                    peers &= bit ? m : ~m;
                }
                const int rank = lane_rank(peers);
                const T v = in ? Ax[e] : T(0);
                for (int r = 0;; ++r) {   // round r: the lanes of rank r (one round without duplicates)
                    if (in && rank == r) acc[rel] = add_rn(acc[rel], v);
                    wsync();
                    if (__ballot(in && rank > r) == 0) break;
                }
            }
            if (!COL) {   // the wave streams its own row out
                T* out = D + (r0 + rr) * ld + c0;
                if (VEC) {
                    const int chunks = (nc + E - 1) / E;
                    for (int k = l; k < chunks; k += WAVE) {
                        const int c = k * E;
                        if (c + E <= nc) {
                            *reinterpret_cast<dn_vec*>(out + c) = *reinterpret_cast<const dn_vec*>(acc + c);
                        } else {
                            for (int j = c; j < nc; ++j) out[j] = acc[j];
                        }
                    }
                } else {
                    for (int c = l; c < nc; c += WAVE) out[c] = acc[c];
                }
                wsync();   // (the row is zeroed again by this wave's next tile)
            }
        }
        if (COL) {   // the tile transposed: nr consecutive rows per column
            __syncthreads();
            const int total = nr * nc;
            for (int idx = (int)threadIdx.x; idx < total; idx += DV_WPB * WAVE) {
                const int c = idx / nr, rr = idx - c * nr;
                D[(r0 + rr) + (c0 + c) * ld] = tile[rr][c];
            }
            __syncthreads();
        }
    }
}

// ----------------------------------------------------------------------------- dense2csr
// One (row, segment) of a row-major D: the columns [s0, s1) of the row at `row`.  FILL: places the
// kept elements from *slot on; otherwise counts them into *slot.  E: elements per lane and step
// (16 / sizeof with 16-byte loads, else 1).
template <typename T, typename CP, int E, bool FILL>
__device__ __forceinline__ void dn_row_segment(const typename DnBits<T>::type* __restrict__ row, int64_t s0,
                                               int64_t s1, CP* __restrict__ slot, int32_t* __restrict__ Cj,
                                               typename DnBits<T>::type* __restrict__ Cx) {
    using B = typename DnBits<T>::type;
    const int l = lane_id();
    int64_t base = FILL ? (int64_t)*slot : 0;
    for (int64_t b0 = s0; b0 < s1; b0 += WAVE * E) {
        const int64_t c = b0 + (int64_t)l * E;
        B v[E];
        bool whole = false;   // the lane's E elements in one 16-byte load
        if constexpr (E > 1) {
            if ((whole = c + E <= s1)) {
                const dn_vec raw = *reinterpret_cast<const dn_vec*>(row + c);
                __builtin_memcpy(v, &raw, 16);
            }
        }
        if (!whole) {
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = c + j < s1 ? row[c + j] : B{};
        }
        bool kept[E];
        int before = 0, total = 0;   // kept elements of the lanes below this one / of the step
#pragma unroll
        for (int j = 0; j < E; ++j) {
            kept[j] = c + j < s1 && DnBits<T>::keep(v[j]);
            const unsigned long long m = __ballot(kept[j]);
            before += lane_rank(m);
            total += __popcll(m);
        }
        if (FILL) {
            int64_t o = base + before;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                if (kept[j]) {
                    Cj[o] = (int32_t)(c + j);
                    Cx[o] = v[j];
                    ++o;
                }
            }
        }
        base += total;
    }
    if (!FILL && l == 0) *slot = (CP)base;
}

// Row-major D: one wave per (row, segment), table[row * nseg + segment].
template <typename T, typename CP, int E, bool FILL>
__device__ __forceinline__ void dn_row_kernel(int64_t cols, int64_t nseg, int64_t tasks,
                                              const typename DnBits<T>::type* __restrict__ D, int64_t ld,
                                              CP* __restrict__ table, int32_t* __restrict__ Cj,
                                              typename DnBits<T>::type* __restrict__ Cx) {
    const int wv = uniform((int)(threadIdx.x >> 6));
    for (int64_t task = (int64_t)blockIdx.x * DV_WPB + wv; task < tasks; task += (int64_t)gridDim.x * DV_WPB) {
        const int64_t r = task / nseg, sg = task - r * nseg;
        const int64_t s0 = sg * DV_S, s1 = min(cols, s0 + DV_S);
        dn_row_segment<T, CP, E, FILL>(D + r * ld, s0, s1, table + task, Cj, Cx);
    }
}

// Column-major D: one workgroup per (64 rows, segment), 64 x 64 tiles transposed through LDS.
template <typename T, typename CP, bool FILL>
__device__ __forceinline__ void dn_col_kernel(int64_t rows, int64_t cols, int64_t nseg, int64_t tasks,
                                              const typename DnBits<T>::type* __restrict__ D, int64_t ld,
                                              CP* __restrict__ table, int32_t* __restrict__ Cj,
                                              typename DnBits<T>::type* __restrict__ Cx) {
    using B = typename DnBits<T>::type;
    __shared__ B tile[DV_T][DV_T + 1];   // [column][row]
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const int64_t rg = task / nseg, sg = task - rg * nseg;
        const int64_t r0 = rg * DV_T, s0 = sg * DV_S, s1 = min(cols, s0 + DV_S);
        const int nr = (int)min((int64_t)DV_T, rows - r0);
        // lane k < 16 keeps the running count / position of the wave's row k
        const int64_t myrow = r0 + wv * DV_RPW + l;
        const bool keeper = l < DV_RPW && myrow < rows;
        long long run = 0;
        if (FILL && keeper) run = (long long)table[myrow * nseg + sg];
        for (int64_t c0 = s0; c0 < s1; c0 += DV_T) {
            const int nc = (int)min((int64_t)DV_T, s1 - c0);
            for (int cc = wv; cc < nc; cc += DV_WPB) tile[cc][l] = l < nr ? D[(r0 + l) + (c0 + cc) * ld] : B{};
            __syncthreads();
            for (int k = 0; k < DV_RPW; ++k) {
                const int rr = wv * DV_RPW + k;
                if (rr >= nr) break;   // (wave-uniform)
                const B v = l < nc ? tile[l][rr] : B{};
                const bool kept = l < nc && DnBits<T>::keep(v);
                const unsigned long long m = __ballot(kept);
                if (FILL) {
                    const long long base = __shfl(run, k, WAVE);
                    if (kept) {
                        const int64_t o = (int64_t)base + lane_rank(m);
                        Cj[o] = (int32_t)(c0 + l);
                        Cx[o] = v;
                    }
                }
                if (l == k) run += __popcll(m);
            }
            __syncthreads();
        }
        if (!FILL && keeper) table[myrow * nseg + sg] = (CP)run;
    }
}

template <typename T, typename CP, int E, bool COL>
__global__ __launch_bounds__(DV_WPB * WAVE) void k_dn_count(int64_t rows, int64_t cols, int64_t nseg, int64_t tasks,
                                                           const typename DnBits<T>::type* __restrict__ D,
                                                           int64_t ld, CP* __restrict__ table) {
    if constexpr (COL) dn_col_kernel<T, CP, false>(rows, cols, nseg, tasks, D, ld, table, nullptr, nullptr);
    else dn_row_kernel<T, CP, E, false>(cols, nseg, tasks, D, ld, table, nullptr, nullptr);
}

template <typename T, typename CP, int E, bool COL>
__global__ __launch_bounds__(DV_WPB * WAVE) void k_dn_fill(int64_t rows, int64_t cols, int64_t nseg, int64_t tasks,
                                                          const typename DnBits<T>::type* __restrict__ D,
                                                          int64_t ld, CP* __restrict__ table,
                                                          int32_t* __restrict__ Cj,
                                                          typename DnBits<T>::type* __restrict__ Cx) {
    if constexpr (COL) dn_col_kernel<T, CP, true>(rows, cols, nseg, tasks, D, ld, table, Cj, Cx);
    else dn_row_kernel<T, CP, E, true>(cols, nseg, tasks, D, ld, table, Cj, Cx);
}

// C's row pointer off the scanned table: the first segment of every row, then the total.
template <typename CP>
__global__ __launch_bounds__(256) void k_dn_indptr(int64_t rows, int64_t nseg, const CP* __restrict__ table,
                                                 CP* __restrict__ Cp) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= rows; r += (int64_t)gridDim.x * 256)
        Cp[r] = table[r * nseg];
}

}  // namespace spg
