// site_link_host.cpp -- the pair test of k_lk_pairs (dg_lk_cells, dg_lk_pair and dg_lk_rows of csrc/k_site_link.hip.h) on
// the CPU, for tests/test_site_link_host.py.
//
// Built by the test with the host compiler and -fsanitize=address,undefined.  Every case's four rows are allocations of
// exactly `words` words, so a read past a row stops the program.  The counts are taken twice, by the header's words and
// population counts and by a loop over the single bits; the two must agree, and so must dg_lk_rows and dg_lk_pair.
//
// Input (argv[1], binary): per case  uint32 words, max_conflict_ppm, min_cell, then the rows P_i, M_i, P_j, M_j.
// Output (stdout), one line a case:  <case> <pp> <mm> <pm> <mp> <partners 0 | 1>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define DG_LK_HOST_ONLY
#include "../../pbdagcon_amd/csrc/k_site_link.hip.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: site_link_host cases.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t h[3];
    for (unsigned k = 0; std::fread(h, sizeof(uint32_t), 3, f) == 3; k++) {
        const uint32_t words = h[0], ppm = h[1], min_cell = h[2];
        unsigned long long *row[4];
        for (auto &r : row) {
            r = static_cast<unsigned long long *>(std::malloc(words ? words * sizeof(unsigned long long) : 1));
            if (words && std::fread(r, sizeof(unsigned long long), words, f) != words) { std::fprintf(stderr, "case %u: short input\n", k); return 2; }
        }
        uint32_t c[4], b[4] = {0u, 0u, 0u, 0u};
        dg_lk_cells(row[0], row[1], row[2], row[3], words, c);
        for (uint64_t x = 0; x < (uint64_t)words * 64u; x++) {
            const bool pi = (row[0][x >> 6] >> (x & 63u)) & 1u, mi = (row[1][x >> 6] >> (x & 63u)) & 1u;
            const bool pj = (row[2][x >> 6] >> (x & 63u)) & 1u, mj = (row[3][x >> 6] >> (x & 63u)) & 1u;
            b[0] += pi && pj; b[1] += mi && mj; b[2] += pi && mj; b[3] += mi && pj;
        }
        if (std::memcmp(c, b, sizeof c)) { std::fprintf(stderr, "case %u: words say %u %u %u %u, bits say %u %u %u %u\n", k, c[0], c[1], c[2], c[3], b[0], b[1], b[2], b[3]); return 3; }
        const bool by_cells = dg_lk_pair(c[0], c[1], c[2], c[3], ppm, min_cell), by_rows = dg_lk_rows(row[0], row[1], row[2], row[3], words, ppm, min_cell);
        if (by_cells != by_rows) { std::fprintf(stderr, "case %u: dg_lk_pair says %d, dg_lk_rows %d\n", k, by_cells, by_rows); return 3; }
        std::printf("%u %u %u %u %u %d\n", k, c[0], c[1], c[2], c[3], by_rows ? 1 : 0);
        for (auto &r : row) std::free(r);
    }
    std::fclose(f);
    return 0;
}
