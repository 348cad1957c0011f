// spgemm_spmm.hpp -- C = alpha * A B + beta * C for CSR A and dense B, C (the product the
// reference times against SpGEMM in others/spmm/spMM.py and others/spmm/diff_matrix_size.py,
// reached through cupyx.cusparse.spmm, modify_src/cupy-src/cupyx/cusparse.py:1440-1513).
//
// Bit-identical to scipy's csr_matvecs: every C(i,c) is summed sequentially in A's entry
// order from 0 (((0 + a0 b0) + a1 b1) + ...), products and sums separately rounded -- k_spmv's
// rule per column of B.  No LDS accumulation, no barriers, no atomics.
//
// Row-major B and C (k_spmm_row, k_spmm_row_packed): lanes run along C's columns, so a lane's
// sum is sequential by construction.  A wave owns one row and one strip of 64 * V columns (V
// elements = 16 bytes per lane when the operands are 16-byte aligned, V = 1 otherwise); it
// reads the row's entries 64 at a time (coalesced), then walks the batch with wave-uniform
// readlanes, so every B row is one coalesced request.  The gathers of SPMM_UNROLL entries are
// issued before the first add consumes one: the adds are a dependent chain, the gathers are not.
// A narrow B (at most 32 lanes wide) packs several rows into a wave, each lane group walking
// its own row.
//
// Column-major B and C (k_spmm_col): lanes run along 64 consecutive rows as in k_spmv (A's
// entries staged through LDS coalesced, C's column stores coalesced); each lane keeps
// SpmmColGeom::NC column accumulators and sums its own row's products in entry order.
//
// Every dense offset (Aj * ldb, row * ldc, strip offsets) is formed in 64 bits.
#pragma once

#include "spg_device.hpp"
#include "spgemm_row.hpp"   // readlane_v

namespace spg {

constexpr int SPMM_WPB = 4;
constexpr int SPMM_UNROLL = 8;      // B-row gathers in flight per wave (k_spmm_row)
constexpr int SPMM_UNROLL_P = 4;    // per lane group (k_spmm_row_packed)
constexpr int SPMM_CH = 512;        // A entries staged per wave per chunk (k_spmm_col)

// V consecutive values moved as one access (16 bytes when V > 1).
template <typename T, int V> struct alignas(V == 1 ? alignof(T) : sizeof(T) * V) SpmmVec { T v[V]; };

// Elements per lane that make a 16-byte access.
template <typename T> struct SpmmGeom { static constexpr int VMAX = 16 / (int)sizeof(T); };

template <typename T> struct SpmmColGeom { static constexpr int NC = sizeof(T) >= 16 ? 4 : 8; };

// p[0..V) into out: one access when all V are inside the matrix (nv == V), else the first nv.
template <typename T, int V, bool FULL>
__device__ __forceinline__ void spmm_load(const T* __restrict__ p, int nv, T (&out)[V]) {
    if (FULL || nv == V) {
        const SpmmVec<T, V> x = *reinterpret_cast<const SpmmVec<T, V>*>(p);
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = x.v[v];
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = v < nv ? p[v] : (T)0;
    }
}

// c[0..nv) = alpha * acc + beta * c; c is read only when beta != 0.
template <typename T, int V, bool FULL>
__device__ __forceinline__ void spmm_epilogue(T* __restrict__ c, int nv, const T (&acc)[V], T alpha, T beta) {
    T old[V];
    if (beta != (T)0) spmm_load<T, V, FULL>(c, nv, old);
    T out[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        T r = alpha == (T)1 ? acc[v] : mul_rn(alpha, acc[v]);
        if (beta != (T)0) r = add_rn(r, mul_rn(beta, old[v]));
        out[v] = r;
    }
    if (FULL || nv == V) {
        SpmmVec<T, V> x;
#pragma unroll
        for (int v = 0; v < V; ++v) x.v[v] = out[v];
        *reinterpret_cast<SpmmVec<T, V>*>(c) = x;
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (v < nv) c[v] = out[v];
    }
}

// One row's walk for one strip: acc += row . B[:, c0 .. c0 + V) in entry order.  a, b, Bc
// wave-uniform apart from Bc's lane offset; nv = this lane's valid columns (V when FULL).
template <typename T, int V, bool FULL>
__device__ __forceinline__ void spmm_walk(int64_t a, int64_t b, const int32_t* __restrict__ Aj,
                                          const T* __restrict__ Ax, const T* __restrict__ Bc, int64_t ldb,
                                          int nv, T (&acc)[V]) {
    const int l = lane_id();
    for (int64_t e0 = a; e0 < b; e0 += WAVE) {
        const int cnt = (int)min((int64_t)WAVE, b - e0);
        const int my_j = l < cnt ? Aj[e0 + l] : 0;
        const T my_x = l < cnt ? Ax[e0 + l] : (T)0;
        int k = 0;
        for (; k + SPMM_UNROLL <= cnt; k += SPMM_UNROLL) {
            T bv[SPMM_UNROLL][V];
#pragma unroll
            for (int u = 0; u < SPMM_UNROLL; ++u) {
                const int64_t j = readlane_i(my_j, k + u);
                if (FULL || nv > 0) spmm_load<T, V, FULL>(Bc + j * ldb, nv, bv[u]);
            }
#pragma unroll
            for (int u = 0; u < SPMM_UNROLL; ++u) {
                const T x = readlane_v(my_x, k + u);
#pragma unroll
                for (int v = 0; v < V; ++v)
                    if (FULL || v < nv) acc[v] = add_rn(acc[v], mul_rn(x, bv[u][v]));
            }
        }
        for (; k < cnt; ++k) {
            const int64_t j = readlane_i(my_j, k);
            const T x = readlane_v(my_x, k);
            T bv[V];
            if (FULL || nv > 0) spmm_load<T, V, FULL>(Bc + j * ldb, nv, bv);
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (FULL || v < nv) acc[v] = add_rn(acc[v], mul_rn(x, bv[v]));
        }
    }
}

// Row-major, one wave per (row, strip of 64 * V columns); task = row * strips + strip, so the
// waves of a block share A's row.  The grid strides over the tasks.
template <typename T, typename IP, int V>
__global__ __launch_bounds__(SPMM_WPB * WAVE) void k_spmm_row(int64_t rows, int64_t n, int64_t strips,
                                                            const IP* __restrict__ Ap,
                                                            const int32_t* __restrict__ Aj,
                                                            const T* __restrict__ Ax, const T* __restrict__ B,
                                                            int64_t ldb, T alpha, T beta, T* __restrict__ C,
                                                            int64_t ldc) {
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    const int64_t tasks = rows * strips;
    const int64_t step = (int64_t)gridDim.x * SPMM_WPB;
    for (int64_t t = (int64_t)blockIdx.x * SPMM_WPB + wv; t < tasks; t += step) {
        const int64_t row = t / strips;
        const int64_t s0 = (t - row * strips) * (int64_t)(WAVE * V);   // strip's first column
        const int64_t c0 = s0 + (int64_t)l * V;
        const int64_t a = (int64_t)Ap[row], b = (int64_t)Ap[row + 1];
        T acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = (T)0;
        if (s0 + WAVE * V <= n) {   // (wave-uniform)
            spmm_walk<T, V, true>(a, b, Aj, Ax, B + c0, ldb, V, acc);
            spmm_epilogue<T, V, true>(C + row * ldc + c0, V, acc, alpha, beta);
        } else {
            const int nv = (int)max((int64_t)0, min((int64_t)V, n - c0));
            spmm_walk<T, V, false>(a, b, Aj, Ax, B + c0, ldb, nv, acc);
            if (nv > 0) spmm_epilogue<T, V, false>(C + row * ldc + c0, nv, acc, alpha, beta);
        }
    }
}

// Row-major, narrow B: n <= (1 << lgs) * V columns, 64 >> lgs rows per wave.  Each group of
// 1 << lgs lanes walks its own row, its lanes loading the same A entry.
template <typename T, typename IP, int V>
__global__ __launch_bounds__(SPMM_WPB * WAVE) void k_spmm_row_packed(int64_t rows, int64_t n, int lgs,
                                                                   const IP* __restrict__ Ap,
                                                                   const int32_t* __restrict__ Aj,
                                                                   const T* __restrict__ Ax,
                                                                   const T* __restrict__ B, int64_t ldb, T alpha,
                                                                   T beta, T* __restrict__ C, int64_t ldc) {
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    const int rpw = WAVE >> lgs;   // rows per wave
    const int64_t tasks = (rows + rpw - 1) / rpw;
    const int64_t step = (int64_t)gridDim.x * SPMM_WPB;
    const int64_t c0 = (int64_t)(l & ((1 << lgs) - 1)) * V;
    for (int64_t t = (int64_t)blockIdx.x * SPMM_WPB + wv; t < tasks; t += step) {
        const int64_t row = t * rpw + (l >> lgs);
        const int nv = row < rows ? (int)max((int64_t)0, min((int64_t)V, n - c0)) : 0;
        if (nv == 0) continue;
        const int64_t a = (int64_t)Ap[row], b = (int64_t)Ap[row + 1];
        const T* Bc = B + c0;
        T acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = (T)0;
        for (int64_t e = a; e < b; e += SPMM_UNROLL_P) {
            T bv[SPMM_UNROLL_P][V];
            T x[SPMM_UNROLL_P];
#pragma unroll
            for (int u = 0; u < SPMM_UNROLL_P; ++u)
                if (e + u < b) {
                    const int64_t j = Aj[e + u];
                    x[u] = Ax[e + u];
                    spmm_load<T, V, false>(Bc + j * ldb, nv, bv[u]);
                }
#pragma unroll
            for (int u = 0; u < SPMM_UNROLL_P; ++u)
                if (e + u < b) {
#pragma unroll
                    for (int v = 0; v < V; ++v)
                        if (v < nv) acc[v] = add_rn(acc[v], mul_rn(x[u], bv[u][v]));
                }
        }
        spmm_epilogue<T, V, false>(C + row * ldc + c0, nv, acc, alpha, beta);
    }
}

// Column-major: a wave takes 64 consecutive rows and NC consecutive columns; task = column
// strip * row groups + row group.  A's entries of the row group go through LDS in chunks of SPMM_CH
// (coalesced reads), then each lane walks its own row's entries in order.
template <typename T, typename IP>
__global__ __launch_bounds__(SPMM_WPB * WAVE) void k_spmm_col(int64_t rows, int64_t n, int64_t cstrips,
                                                            const IP* __restrict__ Ap,
                                                            const int32_t* __restrict__ Aj,
                                                            const T* __restrict__ Ax, const T* __restrict__ B,
                                                            int64_t ldb, T alpha, T beta, T* __restrict__ C,
                                                            int64_t ldc) {
    constexpr int NC = SpmmColGeom<T>::NC;
    __shared__ int32_t j_s[SPMM_WPB][SPMM_CH];
    __shared__ T x_s[SPMM_WPB][SPMM_CH];
    const int l = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    int32_t* js = j_s[wv];
    T* xs = x_s[wv];
    const int64_t tasks = ((rows + WAVE - 1) / WAVE) * cstrips;
    const int64_t step = (int64_t)gridDim.x * SPMM_WPB;
    for (int64_t t = (int64_t)blockIdx.x * SPMM_WPB + wv; t < tasks; t += step) {
        const int64_t rgs = (rows + WAVE - 1) / WAVE;
        // tasks run column strip outermost: the waves in flight gather from one strip's NC columns
        // of B, a slab that fits L2
        const int64_t rg = t % rgs;
        const int64_t cb = t / rgs * NC;   // first column
        const int nc = (int)min((int64_t)NC, n - cb);     // columns of this strip (>= 1)
        const int64_t r0 = rg * WAVE, r1 = min(rows, r0 + WAVE);
        const int64_t row = r0 + l;
        const int64_t a = row < rows ? (int64_t)Ap[row] : 0;
        const int64_t b = row < rows ? (int64_t)Ap[row + 1] : 0;
        const int64_t e0 = (int64_t)Ap[r0], e1 = (int64_t)Ap[r1];
        const T* Bc = B + cb * ldb;
        T acc[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = (T)0;
        for (int64_t c = e0; c < e1; c += SPMM_CH) {
            const int64_t ce = min(e1, c + SPMM_CH);
            for (int64_t e = c + l; e < ce; e += WAVE) {
                js[e - c] = Aj[e];
                xs[e - c] = Ax[e];
            }
            wsync();
            const int64_t lo = max(a, c), hi = min(b, ce);
            for (int64_t e = lo; e < hi; ++e) {
                const T* bp = Bc + (int64_t)js[e - c];
                const T x = xs[e - c];
                T bv[NC];
#pragma unroll
                for (int q = 0; q < NC; ++q)
                    if (q < nc) bv[q] = bp[q * ldb];
#pragma unroll
                for (int q = 0; q < NC; ++q)
                    if (q < nc) acc[q] = add_rn(acc[q], mul_rn(x, bv[q]));
            }
            wsync();
        }
        if (row < rows) {
            T* cp = C + cb * ldc + row;
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nc) {
                    T v = alpha == (T)1 ? acc[q] : mul_rn(alpha, acc[q]);
                    if (beta != (T)0) v = add_rn(v, mul_rn(beta, cp[q * ldc]));
                    cp[q * ldc] = v;
                }
        }
    }
}

}  // namespace spg
