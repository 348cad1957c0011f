// spg_format_layouts.hpp -- the workspace carves of the format operations (spg_csr2csc,
// spg_csrgeam, spg_csr_binop, spg_dense2csr, spg_canonicalize, spg_csr_extract): where every region of a caller's
// workspace lies and how many bytes the size query answers.  Pure host arithmetic over the
// operands' shapes: no HIP, so tests/hip/format_layouts_check.cpp builds it with a plain C++17
// compiler and tests/test_format_layouts_cpu.py pins every answer without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "spgemm.h"

namespace spg {

// Geometry a carve and a kernel share: the kernels walk chunks, tiles and segments of exactly
// these sizes and the carves below size the tables they fill.  Defined here and nowhere else; the
// kernel headers include this one.
constexpr int WPB = 4;                          // waves per block
constexpr int BLOCK = 256;                      // threads per block: WPB waves (spgemm_kernels.hpp asserts it)
constexpr int SCAN_ITEMS = 8;                   // k_scan_lb: elements per thread
constexpr int SCAN_TILE = BLOCK * SCAN_ITEMS;   // k_scan_lb: elements per tile (2048)
constexpr int TR_CHUNK = 2048;                  // radix sort: entries per wave chunk
constexpr int TR_RADIX = 256;                   // radix sort: 8-bit digits
constexpr int GM_CHUNK = 1024;                  // csrgeam: entries per wave chunk (16 steps of 64)
constexpr int DV_S = 1024;                      // dense2csr: columns per segment
constexpr int DV_T = 64;                        // dense2csr, column-major: tile edge
constexpr int EX_ALL = 0, EX_RANGE = 1, EX_LIST = 2;   // extract: the column selection's mode
constexpr size_t EX_REC_BYTES = 8;              // extract: sizeof(ExRec), a (listed column, position) record

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

inline size_t vbytes(spg_dtype_t t) {
    return t == SPG_C_64F ? 16 : (t == SPG_R_64F || t == SPG_C_32F) ? 8 : 4;
}

inline size_t index_bytes(spg_index_t t) { return t == SPG_INDEX_64I ? 8 : 4; }

// Workspace carving.  A cursor over offsets from the workspace's base: take(bytes) returns the
// current offset and advances to the next 256-byte boundary.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += align_up(bytes);
        return at;
    }
    // how every format layout opens and closes: the 16 int64 scalars a scan reports into come
    // first, and the size to ask for is the carved bytes plus 256 of slack for the base alignment
    size_t scalars() { return take(16 * sizeof(int64_t)); }
    size_t total() const { return off + 256; }
};

inline int64_t grid_for(int64_t rows, int per_block) { return (rows + per_block - 1) / per_block; }

inline int64_t scan_tiles(int64_t n) { return n > 0 ? (n + SCAN_TILE - 1) / SCAN_TILE : 1; }
// bytes of the status words of a look-back scan over n elements: a ticket + one word per tile
inline size_t status_bytes(int64_t n) { return sizeof(unsigned long long) * (size_t)(scan_tiles(n) + 1); }

// bits of an index below `extent`: the bits of extent - 1 (at least one)
inline int index_bits(int64_t extent) {
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < extent) ++b;
    return b;
}

// Workspace carve of spg_csr2csc (offsets from the 256-byte aligned base).
struct TrLayout {
    int passes = 1;            // 8-bit digit passes: the bytes of cols - 1 (at least one)
    int64_t chunks = 0;        // wave chunks of TR_CHUNK entries
    int nbuf = 0;              // ping-pong record buffers the passes need (0, 1 or 2)
    size_t scalars = 0, status = 0, table = 0, skeys = 0, buf[2] = {0, 0};
    size_t keys = 0, rowids = 0, pos = 0;   // inside one record buffer
    size_t total = 0;          // bytes to ask for (256 of slack for the base alignment)
};

inline TrLayout tr_layout(const spg_csr_t& A) {
    TrLayout L;
    const size_t ips = index_bytes(A.indptr_type);
    const uint64_t top = A.cols > 0 ? (uint64_t)(A.cols - 1) : 0;
    L.passes = top >= (1ull << 24) ? 4 : top >= (1ull << 16) ? 3 : top >= (1ull << 8) ? 2 : 1;
    L.chunks = (A.nnz + TR_CHUNK - 1) / TR_CHUNK;
    L.nbuf = std::min(L.passes - 1, 2);
    Carver c;
    L.scalars = c.scalars();
    L.status = c.take(status_bytes(TR_RADIX * L.chunks));
    L.table = c.take(ips * ((size_t)TR_RADIX * (size_t)L.chunks + 1));   // (+ 1: the scan writes its total)
    L.skeys = c.take(sizeof(int32_t) * (size_t)A.nnz);   // the sorted columns (the last pass -> k_tr_indptr)
    Carver rec;   // one record buffer: keys | row ids | positions
    L.keys = rec.take(sizeof(int32_t) * (size_t)A.nnz);
    L.rowids = rec.take(sizeof(int32_t) * (size_t)A.nnz);
    L.pos = rec.take(ips * (size_t)A.nnz);
    for (int b = 0; b < L.nbuf; ++b) L.buf[b] = c.take(rec.off);
    L.total = c.total();
    return L;
}

// Workspace carve of spg_csrgeam_nnz / spg_csrgeam (offsets from the 256-byte aligned base).
struct GmLayout {
    int64_t chunksA = 0, chunksB = 0;   // wave chunks of GM_CHUNK entries
    size_t scalars = 0;                 // 16 int64: [0] a scan's total, [1] its overflow flag
    size_t status_b = 0, status_r = 0;  // look-back words of the scan over B's entries / over the rows
    size_t S = 0;                       // nnz(B) + 1 IP: B-only marks, scanned in place (kept for the value pass)
    size_t cnt = 0;                     // rows + 1 int64: entries per row of C
    size_t total = 0;                   // bytes to ask for (256 of slack for the base alignment)
};

inline GmLayout gm_layout(const spg_csr_t& A, const spg_csr_t& B) {
    GmLayout L;
    const size_t ips = index_bytes(A.indptr_type);
    L.chunksA = (A.nnz + GM_CHUNK - 1) / GM_CHUNK;
    L.chunksB = (B.nnz + GM_CHUNK - 1) / GM_CHUNK;
    Carver c;
    L.scalars = c.scalars();
    L.status_b = c.take(status_bytes(B.nnz));
    L.status_r = c.take(status_bytes(A.rows));
    L.S = c.take(ips * ((size_t)B.nnz + 1));
    L.cnt = c.take(sizeof(int64_t) * ((size_t)A.rows + 1));
    L.total = c.total();
    return L;
}

// Workspace carve of spg_csr_binop_nnz / spg_csr_binop (offsets from the 256-byte aligned base).
// SA and SB stay for the value call.
struct BoLayout {
    int64_t chunksA = 0, chunksB = 0;   // wave chunks of GM_CHUNK entries
    size_t scalars = 0;                 // 16 int64: [0] a scan's total, [1] its overflow flag
    size_t status_a = 0, status_b = 0, status_r = 0;   // look-back words of the scans over A's entries / B's / the rows
    size_t SA = 0;                      // nnz(A) + 1 IP: A's kept marks, scanned in place
    size_t SB = 0;                      // nnz(B) + 1 IP: the kept B-only marks, scanned in place
    size_t cnt = 0;                     // rows + 1 int64: entries per row of C
    size_t total = 0;                   // bytes to ask for (256 of slack for the base alignment)
};

inline BoLayout bo_layout(const spg_csr_t& A, const spg_csr_t& B) {
    BoLayout L;
    const size_t ips = index_bytes(A.indptr_type);
    L.chunksA = (A.nnz + GM_CHUNK - 1) / GM_CHUNK;
    L.chunksB = (B.nnz + GM_CHUNK - 1) / GM_CHUNK;
    Carver c;
    L.scalars = c.scalars();
    L.status_a = c.take(status_bytes(A.nnz));
    L.status_b = c.take(status_bytes(B.nnz));
    L.status_r = c.take(status_bytes(A.rows));
    L.SA = c.take(ips * ((size_t)A.nnz + 1));
    L.SB = c.take(ips * ((size_t)B.nnz + 1));
    L.cnt = c.take(sizeof(int64_t) * ((size_t)A.rows + 1));
    L.total = c.total();
    return L;
}

// Workspace carve of spg_dense2csr_nnz / spg_dense2csr (offsets from the 256-byte aligned base).
struct DnLayout {
    int64_t nseg = 1;        // segments of DV_S columns per row
    int64_t entries = 0;     // rows * nseg: the (row, segment) table
    int64_t tasks = 0;       // wave tasks (row-major) or workgroup tasks (column-major)
    size_t scalars = 0;      // 16 int64: [0] the scan's total, [1] its overflow flag
    size_t status = 0;       // look-back words of the scan over the table
    size_t table = 0;        // entries + 1 positions (8 bytes each, whatever C's row-pointer type)
    size_t total = 0;        // bytes to ask for (256 of slack for the base alignment)
};

inline DnLayout dn_layout(const spg_dense_t& D) {
    DnLayout L;
    L.nseg = std::max<int64_t>(1, grid_for(D.cols, DV_S));
    L.entries = D.rows * L.nseg;
    L.tasks = D.order == SPG_ORDER_COL ? grid_for(D.rows, DV_T) * L.nseg : L.entries;
    Carver c;
    L.scalars = c.scalars();
    L.status = c.take(status_bytes(L.entries));
    L.table = c.take(sizeof(int64_t) * ((size_t)L.entries + 1));
    L.total = c.total();
    return L;
}

// Workspace carve of spg_canonicalize_nnz / spg_canonicalize (offsets from the 256-byte aligned
// base).  The sorted records stay in buf[passes & 1] and the scanned marks in `kept` for the
// value call.
struct CnLayout {
    bool sum = false, drop = false;
    bool marks = false;         // SUM or DROP_ZEROS: kept[] exists
    int cbits = 1, rbits = 1;   // key = row << cbits | column
    bool k64 = false;           // the key takes 64 bits
    int shift0 = 0;             // the first digit's shift: 0, or cbits when only the rows are sorted (COO, no op)
    int passes = 0;             // 0: CSR input with DROP_ZEROS alone, no sort (the entries are their own records)
    int64_t chunks = 0;         // wave chunks of TR_CHUNK entries
    size_t scalars = 0;         // 16 int64: [0] a scan's total
    size_t status_t = 0, status_k = 0;   // look-back words of the table scans / of the scan over kept[]
    size_t table = 0;           // 256 * chunks + 1 IP: a pass's digit histogram, scanned in place
    size_t kept = 0;            // nnz + 1 IP: the kept marks, scanned in place
    size_t buf[2] = {0, 0};     // ping-pong record buffers (k_cn_pack writes buf[0])
    size_t total = 0;           // bytes to ask for (256 of slack for the base alignment)
};

inline CnLayout cn_layout(const spg_csr_t& A, bool coo, unsigned ops) {
    CnLayout L;
    const size_t ips = index_bytes(A.indptr_type);
    const size_t nnz = (size_t)A.nnz;
    L.sum = (ops & SPG_CANON_SUM) != 0;
    L.drop = (ops & SPG_CANON_DROP_ZEROS) != 0;
    L.marks = L.sum || L.drop;
    const bool sort = L.sum || (ops & SPG_CANON_SORT) != 0;
    L.cbits = index_bits(A.cols);
    L.rbits = index_bits(A.rows);
    L.k64 = L.cbits + L.rbits > 32;
    L.shift0 = sort ? 0 : L.cbits;
    L.passes = sort || coo ? (L.cbits + L.rbits - L.shift0 + 7) / 8 : 0;
    L.chunks = (A.nnz + TR_CHUNK - 1) / TR_CHUNK;
    Carver c;
    L.scalars = c.scalars();
    if (L.passes) {
        L.status_t = c.take(status_bytes(TR_RADIX * L.chunks));
        L.table = c.take(ips * ((size_t)TR_RADIX * (size_t)L.chunks + 1));   // (+ 1: the scan writes its total)
    }
    if (L.marks) {
        L.status_k = c.take(status_bytes(A.nnz));
        L.kept = c.take(ips * (nnz + 1));
    }
    const size_t rec = (ips == 4 && !L.k64 ? 8 : 16) * nnz;   // sizeof(CnRec<IP, K>) each
    for (int b = 0; b < (L.passes ? 2 : 0); ++b) L.buf[b] = c.take(rec);
    L.total = c.total();
    return L;
}

// One axis' selection after the host checks: a NULL spg_sel_t is the whole axis, a range of at
// most one member has step 1.
struct ExSel {
    bool whole = true;
    int64_t start = 0, step = 1, count = 0;
    const int32_t* index = nullptr;
};

// `sel` over an axis of `extent` members, checked on the host (list entries are not read).
inline spg_status_t ex_sel(const spg_sel_t* sel, int64_t extent, ExSel& out) {
    out = ExSel{};
    out.count = extent;
    if (!sel) return SPG_STATUS_SUCCESS;
    out.whole = false;
    out.count = sel->count;
    out.index = sel->index;
    if (sel->count < 0) return SPG_STATUS_INVALID_VALUE;
    if (sel->count > 2147483647LL) return SPG_STATUS_NOT_SUPPORTED;
    if (sel->index) return SPG_STATUS_SUCCESS;
    if (sel->count > 1 && sel->step == 0) return SPG_STATUS_INVALID_VALUE;
    out.start = sel->start;
    out.step = sel->count > 1 ? sel->step : 1;
    if (sel->count > 0) {
        const __int128 last = (__int128)out.start + (__int128)(out.count - 1) * out.step;
        if (out.start < 0 || out.start >= extent || last < 0 || last >= extent) return SPG_STATUS_INVALID_VALUE;
    }
    return SPG_STATUS_SUCCESS;
}

// Workspace carve of spg_csr_extract_nnz / spg_csr_extract (offsets from the 256-byte aligned
// base).  S, and with a column list colptr and the sorted records, stay for the value call.
struct ExLayout {
    int kmode = EX_ALL;
    bool s64 = false;           // S is int64 (a column list, or A's row pointer is)
    bool contig = false;        // K = all over a step-1 row range: one span of A
    int passes = 0;             // sort passes over the listed columns' bits
    int64_t kchunks = 0;        // wave chunks of TR_CHUNK list positions
    size_t scalars = 0;         // 16 int64: [0] a scan's total, [1] its overflow flag
    size_t status_e = 0, status_r = 0, status_t = 0;   // look-back words: over A's entries / the output rows / the sort's table
    size_t S = 0;               // nnz(A) + 1 SP: mult, scanned in place
    size_t cnt = 0;             // nr + 1 int64: entries per output row
    size_t table = 0;           // 256 * kchunks + 1 int32: a pass's digit histogram, scanned in place
    size_t colptr = 0;          // cols + 1 int32
    size_t buf[2] = {0, 0};     // ping-pong records of the list (k_ex_pack writes buf[0])
    size_t total = 0;           // bytes to ask for (256 of slack for the base alignment)
};

inline ExLayout ex_layout(const spg_csr_t& A, const ExSel& R, const ExSel& K) {
    ExLayout L;
    L.kmode = K.whole ? EX_ALL : K.index ? EX_LIST : EX_RANGE;
    L.s64 = L.kmode == EX_LIST || A.indptr_type == SPG_INDEX_64I;
    L.contig = L.kmode == EX_ALL && !R.index && R.step == 1;
    Carver c;
    L.scalars = c.scalars();
    L.status_r = c.take(status_bytes(R.count));
    L.cnt = c.take(sizeof(int64_t) * ((size_t)R.count + 1));
    if (L.kmode != EX_ALL) {
        L.status_e = c.take(status_bytes(A.nnz));
        L.S = c.take((L.s64 ? 8 : 4) * ((size_t)A.nnz + 1));
    }
    if (L.kmode == EX_LIST) {
        L.passes = (index_bits(A.cols) + 7) / 8;
        L.kchunks = (K.count + TR_CHUNK - 1) / TR_CHUNK;
        L.status_t = c.take(status_bytes(TR_RADIX * L.kchunks));
        L.table = c.take(sizeof(int32_t) * ((size_t)TR_RADIX * (size_t)L.kchunks + 1));
        L.colptr = c.take(sizeof(int32_t) * ((size_t)A.cols + 1));
        for (int b = 0; b < 2; ++b) L.buf[b] = c.take(EX_REC_BYTES * (size_t)K.count);
    }
    L.total = c.total();
    return L;
}

}  // namespace spg
