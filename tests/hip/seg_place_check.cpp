// Host driver of spmm_amd/csrc/seg_place.hpp for tests/test_seg_place_cpu.py (plain C++, no
// device).  stdin: one list per line, "<record bytes> <records of segment 0> <of segment 1> ...".
// stdout, per list: "<bound> <start of segment 0> <start of segment 1> ..." -- the byte offsets
// seg_place gives the segments when they are placed one after another from offset 0, and
// seg_bound's figure for the list.  A line that starts with "blocks" places the list as the
// device pass does (k_seg_place): every SEG_BLK segments from a line boundary, the block rounded
// up to whole lines; its output has the end of the last block after the bound:
// "<bound> <end> <start 0> ...".
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "seg_place.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        const bool blocks = line.rfind("blocks", 0) == 0;
        std::istringstream in(blocks ? line.substr(6) : line);
        uint32_t rb;
        if (!(in >> rb)) continue;
        std::ostringstream out;
        uint32_t x = 0, base = 0, n;
        uint64_t nnz = 0, segs = 0;
        while (in >> n) {
            if (blocks && segs > 0 && segs % spg::SEG_BLK == 0) {
                base += (x + spg::SEG_LINE - 1) / spg::SEG_LINE * spg::SEG_LINE;
                x = 0;
            }
            const uint32_t at = spg::seg_place(x, n * rb);
            out << ' ' << base + at;
            x = at + n * rb;
            nnz += n;
            ++segs;
        }
        std::cout << spg::seg_bound(nnz, segs, rb);
        if (blocks) std::cout << ' ' << base + (x + spg::SEG_LINE - 1) / spg::SEG_LINE * spg::SEG_LINE;
        std::cout << out.str() << '\n';
    }
    return 0;
}
