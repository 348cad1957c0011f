// Host driver of bo_layout (spmm_amd/csrc/spg_format_layouts.hpp, the workspace carve of
// spg_csr_binop_nnz / spg_csr_binop) for tests/test_elementwise_layout_cpu.py: plain C++, host
// arithmetic only, no device.  One shape per input line,
//   IPBITS rows cols nnzA nnzB
// and the layout's every field comes out on one line as name=value pairs, regions as byte offsets
// from the workspace's base.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "spg_format_layouts.hpp"

using namespace spg;

namespace {
void put(const char* name, long long v) { std::printf("%s=%lld ", name, v); }
void put(const char* name, size_t v) { std::printf("%s=%zu ", name, v); }
#define PUT(L, f) put(#f, L.f)
#define PUTI(L, f) put(#f, (long long)L.f)
}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int bits = 0;
        spg_csr_t A{};
        if (!(in >> bits)) continue;
        in >> A.rows >> A.cols >> A.nnz;
        A.indptr_type = bits == 64 ? SPG_INDEX_64I : SPG_INDEX_32I;
        A.value_type = SPG_R_32F;
        spg_csr_t B = A;
        in >> B.nnz;
        if (!in) {
            std::fprintf(stderr, "short line: %s\n", line.c_str());
            return 2;
        }
        const BoLayout L = bo_layout(A, B);
        PUTI(L, chunksA); PUTI(L, chunksB); PUT(L, scalars); PUT(L, status_a); PUT(L, status_b); PUT(L, status_r);
        PUT(L, SA); PUT(L, SB); PUT(L, cnt); PUT(L, total);
        std::printf("\n");
    }
    return 0;
}
