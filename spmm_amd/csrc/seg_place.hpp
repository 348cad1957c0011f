// seg_place.hpp -- where the segments of a dense tile's B records go (host and device: the
// workspace bound of a plan and the device pass that places the segments use the same text;
// plain C++, so a host-only program can include it).
//
// The vector L1 fetches records in 128-byte lines ("packed segments"), and a
// dense fp64 tile's segment is about 100 bytes at an arbitrary even offset: back to back, a
// segment touches 1.78 lines where 1.25 would do.  So a segment that would touch more lines at
// its compact place than its length needs starts at the next line instead; every other segment
// stays where it is, and two short segments may share a line.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPG_HD __host__ __device__
#else
#define SPG_HD
#endif

namespace spg {

constexpr uint32_t SEG_LINE = 128;   // bytes of a line
constexpr int SEG_BLK = 64;          // B rows of a tile that one lane places, from a line boundary
// Segments are placed only where a tile's expected segment is at most this many bytes: longer
// ones take several lines wherever they start, and the placement passes would cost more than
// the lines they save (measured: fp32 entry runs of 600 bytes).
constexpr uint32_t SEG_PLACE_MAX = 256;

// Start of a segment of L bytes that would start at byte x of a line-aligned array.
SPG_HD inline uint32_t seg_place(uint32_t x, uint32_t L) {
    if (L == 0) return x;
    const uint32_t here = (x + L - 1) / SEG_LINE - x / SEG_LINE + 1;
    return here > (L + SEG_LINE - 1) / SEG_LINE ? (x + SEG_LINE - 1) / SEG_LINE * SEG_LINE : x;
}

// Bytes the placed records of `nnz` entries in `segs` segments take at most, whatever their
// lengths: a segment moves by at most SEG_LINE - 2 bytes (offsets are even) and only a non-empty
// one moves.  A block of SEG_BLK segments that starts at a line and is rounded up to whole lines
// stays inside it: its first non-empty segment does not move, and the rounding takes its place.
SPG_HD inline uint64_t seg_bound(uint64_t nnz, uint64_t segs, uint32_t rec_bytes) {
    return nnz * rec_bytes + (uint64_t)(SEG_LINE - 2) * (nnz < segs ? nnz : segs);
}

}   // namespace spg
