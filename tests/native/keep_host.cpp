// keep_host.cpp -- the step a wave of k_win_keep runs (dg_keep_step of csrc/k_keep.hip.h) on the CPU, for
// tests/test_keep_host.py.
//
// Built by the test with the host compiler and -fsanitize=address,undefined.  The wave is played as the kernel plays it:
// 64 positions a step from the segment's front, the two ballots made from exactly the n words the segment owns (a read
// past them stops the program), the step, out of the loop when it says so, then lane 0's record.
//
// Input (argv[1], binary): per case  uint32 n, lo, hi, then n positions (bit 31 may be set: it is masked, as on the device).
// Output (stdout), one line a case:  <case> <i0> <i1> <p_first> <p_last> <steps taken>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define DG_KEEP_HOST_ONLY
#include "../../pbdagcon_amd/csrc/k_keep.hip.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: keep_host cases.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t h[3];
    for (unsigned k = 0; std::fread(h, sizeof(uint32_t), 3, f) == 3; k++) {
        const uint32_t n = h[0], lo = h[1], hi = h[2];
        uint32_t *pw = static_cast<uint32_t *>(std::malloc(n ? n * sizeof(uint32_t) : 1));
        if (n && std::fread(pw, sizeof(uint32_t), n, f) != n) { std::fprintf(stderr, "case %u: short input\n", k); return 2; }
        DgKeepState s = {0u, 0u};
        uint32_t i1 = n, steps = 0;
        for (uint32_t base = 0; base < n; base += 64u) {
            unsigned long long m_lo = 0, m_hi = 0;
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const uint32_t i = base + lane;
                const uint32_t P = i < n ? pw[i] & ~0x80000000u : 0u;
                if (i < n && P > lo) m_lo |= 1ull << lane;
                if (i < n && P > hi) m_hi |= 1ull << lane;
            }
            steps++;
            // (bits at or above the valid lanes must not count: set them all, the step is to mask them)
            const uint32_t nvalid = n - base < 64u ? n - base : 64u;
            if (nvalid < 64u) { m_lo |= ~0ull << nvalid; m_hi |= ~0ull << nvalid; }
            if (dg_keep_step(m_lo, m_hi, base, nvalid, s, i1)) break;
        }
        uint32_t rec[4] = {0u, 0u, 0u, 0u};
        if (s.have && i1 > s.i0) {
            if (i1 > n) { std::fprintf(stderr, "case %u: i1 %u of %u bases\n", k, i1, n); return 3; }
            rec[0] = s.i0; rec[1] = i1; rec[2] = pw[s.i0] & ~0x80000000u; rec[3] = pw[i1 - 1u] & ~0x80000000u;
        }
        std::printf("%u %u %u %u %u %u\n", k, rec[0], rec[1], rec[2], rec[3], steps);
        std::free(pw);
    }
    std::fclose(f);
    return 0;
}
