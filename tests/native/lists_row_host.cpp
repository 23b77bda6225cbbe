// lists_row_host.cpp -- the row scan a lane of k_lists_lanes runs (csrc/k_lists_row.hip.h) on the CPU, for
// tests/test_lists_row_host.py.
//
// Built by the test with the host compiler and -fsanitize=address,undefined.  The row has exactly the K words the
// kernel's lane owns, so a read or write past it stops the program.
//
// Input (argv[1], binary): per case  uint32 K, arrival (0 / 1), chain, ulo, uhi, then K cells.
// Output (stdout), one line a case:
//   <case> <n> <c0> <overflow 0/1> <n_cov> <n_match> <last_base> <id>:<count> ...
// with the n - 1 staged entries after entry 0 (id = neighbour id + 1; count as the out-list stores it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pbdagcon_amd/csrc/k_lists_row.hip.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: lists_row_host cases.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t h[5];
    for (unsigned k = 0; std::fread(h, sizeof(uint32_t), 5, f) == 5; k++) {
        const uint32_t K = h[0];
        uint32_t *row = static_cast<uint32_t *>(std::malloc(K ? K * sizeof(uint32_t) : 1));
        if (K && std::fread(row, sizeof(uint32_t), K, f) != K) { std::fprintf(stderr, "case %u: short input\n", k); return 2; }
        const DgLaneRow s = h[1] ? dg_lane_row<true>(row, K, h[2], h[3], h[4]) : dg_lane_row<false>(row, K, h[2], h[3], h[4]);
        std::printf("%u %u %u %u %u %u %u", k, s.n, s.c0, s.overflow ? 1u : 0u, s.n_cov, s.n_match, s.last_base);
        if (s.n - 1u > K) { std::fprintf(stderr, "case %u: %u entries from %u cells\n", k, s.n - 1u, K); return 3; }
        for (uint32_t j = 1; j < s.n; j++) std::printf(" %u:%u", DG_CELL_ID(row[j - 1u]), dg_lane_count(s, row[j - 1u]));
        std::printf("\n");
        std::free(row);
    }
    std::fclose(f);
    return 0;
}
