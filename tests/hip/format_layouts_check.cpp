// Host driver of spmm_amd/csrc/spg_format_layouts.hpp for tests/test_format_layouts_cpu.py (plain
// C++, no device).  One shape per input line; the matching layout's every field comes out on one
// line as name=value pairs, regions as byte offsets from the workspace's base:
//   tr IPBITS rows cols nnz                          -> tr_layout   (spg_csr2csc)
//   gm IPBITS rows cols nnzA nnzB                    -> gm_layout   (spg_csrgeam)
//   dn ORDER rows cols            (ORDER: row | col) -> dn_layout   (spg_dense2csr)
//   cn IPBITS rows cols nnz COO OPS                  -> cn_layout   (spg_canonicalize)
//   ex IPBITS rows cols nnz  RSEL  KSEL              -> ex_layout   (spg_csr_extract)
// with a selection `whole`, `range START STEP COUNT` or `list COUNT` (a list's entries are never
// read).  A selection ex_sel rejects prints `status=<code>` alone.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "spg_format_layouts.hpp"

using namespace spg;

namespace {

spg_csr_t csr(std::istream& in, bool with_nnz = true) {
    int bits = 0;
    spg_csr_t A{};
    in >> bits >> A.rows >> A.cols;
    if (with_nnz) in >> A.nnz;
    A.indptr_type = bits == 64 ? SPG_INDEX_64I : SPG_INDEX_32I;
    A.value_type = SPG_R_32F;
    return A;
}

// reads one selection; `sel` is what the entry point would be handed (nullptr: the whole axis)
const spg_sel_t* selection(std::istream& in, spg_sel_t& store) {
    static const int32_t never_read = 0;
    std::string kind;
    in >> kind;
    store = spg_sel_t{};
    if (kind == "whole") return nullptr;
    if (kind == "range") in >> store.start >> store.step >> store.count;
    else {
        in >> store.count;
        store.index = &never_read;
    }
    return &store;
}

void put(const char* name, long long v) { std::printf("%s=%lld ", name, v); }
void put(const char* name, size_t v) { std::printf("%s=%zu ", name, v); }
#define PUT(L, f) put(#f, L.f)
#define PUTI(L, f) put(#f, (long long)L.f)

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "tr") {
            const TrLayout L = tr_layout(csr(in));
            PUTI(L, passes); PUTI(L, chunks); PUTI(L, nbuf); PUT(L, scalars); PUT(L, status); PUT(L, table);
            PUT(L, skeys); put("buf0", L.buf[0]); put("buf1", L.buf[1]); PUT(L, keys); PUT(L, rowids); PUT(L, pos);
            PUT(L, total);
        } else if (op == "gm") {
            spg_csr_t A = csr(in), B = A;
            in >> B.nnz;
            const GmLayout L = gm_layout(A, B);
            PUTI(L, chunksA); PUTI(L, chunksB); PUT(L, scalars); PUT(L, status_b); PUT(L, status_r); PUT(L, S);
            PUT(L, cnt); PUT(L, total);
        } else if (op == "dn") {
            std::string order;
            spg_dense_t D{};
            in >> order >> D.rows >> D.cols;
            D.order = order == "col" ? SPG_ORDER_COL : SPG_ORDER_ROW;
            D.ld = D.order == SPG_ORDER_COL ? D.rows : D.cols;
            D.value_type = SPG_R_32F;
            const DnLayout L = dn_layout(D);
            PUTI(L, nseg); PUTI(L, entries); PUTI(L, tasks); PUT(L, scalars); PUT(L, status); PUT(L, table);
            PUT(L, total);
        } else if (op == "cn") {
            const spg_csr_t A = csr(in);
            int coo = 0;
            unsigned ops = 0;
            in >> coo >> ops;
            const CnLayout L = cn_layout(A, coo != 0, ops);
            PUTI(L, sum); PUTI(L, drop); PUTI(L, marks); PUTI(L, cbits); PUTI(L, rbits); PUTI(L, k64);
            PUTI(L, shift0); PUTI(L, passes); PUTI(L, chunks); PUT(L, scalars); PUT(L, status_t); PUT(L, status_k);
            PUT(L, table); PUT(L, kept); put("buf0", L.buf[0]); put("buf1", L.buf[1]); PUT(L, total);
        } else if (op == "ex") {
            const spg_csr_t A = csr(in);
            spg_sel_t rs, ks;
            const spg_sel_t* rows = selection(in, rs);
            const spg_sel_t* cols = selection(in, ks);
            ExSel R, K;
            spg_status_t st = ex_sel(rows, A.rows, R);
            if (!st) st = ex_sel(cols, A.cols, K);
            if (st) {
                put("status", (long long)st);
            } else {
                const ExLayout L = ex_layout(A, R, K);
                PUTI(L, kmode); PUTI(L, s64); PUTI(L, contig); PUTI(L, passes); PUTI(L, kchunks); PUT(L, scalars);
                PUT(L, status_e); PUT(L, status_r); PUT(L, status_t); PUT(L, S); PUT(L, cnt); PUT(L, table);
                PUT(L, colptr); put("buf0", L.buf[0]); put("buf1", L.buf[1]); PUT(L, total);
                put("rcount", (long long)R.count); put("kcount", (long long)K.count);
            }
        } else {
            std::fprintf(stderr, "unknown operation: %s\n", op.c_str());
            return 2;
        }
        if (!in) {
            std::fprintf(stderr, "short line: %s\n", line.c_str());
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
