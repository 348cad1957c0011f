// spgemm_cols16.hpp -- 16-bit columns for the structure broadcast: spg_cols16_split /
// spg_cols16_join (include/spgemm.h).  The two kernels stand outside namespace spg (the names
// profiles and traces know them by).
#pragma once

#include "spg_device.hpp"

// One wave per row.  Split: every column's low half, and where the row's columns reach each
// interior block start c * 65536 (the first entry whose high half is >= c; the row length
// when none is).  Each start is written by exactly one lane: the entry whose high half
// steps over it, or the tail loop for blocks past the row's last column.
template <typename IP>
__global__ __launch_bounds__(256) void k_cols16_split(int64_t rows, const IP* __restrict__ Mp,
                                                      const int32_t* __restrict__ Mj, int nb1,
                                                      uint32_t* __restrict__ starts, uint16_t* __restrict__ lo16) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int l = spg::lane_id();
    const int64_t b = (int64_t)Mp[row];
    const uint32_t len = (uint32_t)((int64_t)Mp[row + 1] - b);
    uint32_t* __restrict__ st = starts + row * nb1;
    for (uint32_t i = l; i < len; i += spg::WAVE) {
        const uint32_t c = (uint32_t)Mj[b + i];
        lo16[b + i] = (uint16_t)(c & 0xffffu);
        const int hi = min((int)(c >> 16), nb1);   // (clamped: a column past M's width writes nothing past the row's starts)
        const int hp = i ? min((int)((uint32_t)Mj[b + i - 1] >> 16), nb1) : 0;
        for (int q = hp + 1; q <= hi; ++q) st[q - 1] = i;
    }
    const int hl = len ? (int)((uint32_t)Mj[b + len - 1] >> 16) : 0;
    for (int q = hl + 1 + l; q <= nb1; q += spg::WAVE) st[q - 1] = len;
}

// Join: column = (block << 16) | low half, the block = the number of interior starts <= the
// entry's offset in its row (the starts ascend; a binary search over the row's nb1 starts).
template <typename IP>
__global__ __launch_bounds__(256) void k_cols16_join(int64_t rows, const IP* __restrict__ Mp, int nb1,
                                                     const uint32_t* __restrict__ starts,
                                                     const uint16_t* __restrict__ lo16, int32_t* __restrict__ Mj) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int l = spg::lane_id();
    const int64_t b = (int64_t)Mp[row];
    const uint32_t len = (uint32_t)((int64_t)Mp[row + 1] - b);
    const uint32_t* __restrict__ st = starts + row * nb1;
    for (uint32_t i = l; i < len; i += spg::WAVE) {
        int lo = 0, hi = nb1;   // first q with st[q] > i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (st[mid] <= i) lo = mid + 1; else hi = mid;
        }
        Mj[b + i] = (int32_t)(((uint32_t)lo << 16) | (uint32_t)lo16[b + i]);
    }
}
