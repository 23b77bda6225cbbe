// pileup.h -- pbdagcon --pileup / --sites: the counts of dagcon_pileup and dagcon_pileup_sites as text lines (host only).
//
// One line per position, tab-separated: RNAME POS REF DEPTH A C G T N DEL INS.
//   - POS is 1-based, in target coordinates (a window's positions plus its begin);
//   - REF is the target's byte where the input carries the target's bases (the record inputs), '.' otherwise;
//   - DEPTH = A + C + G + T + N + DEL; a position without depth has no line.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../../include/dagcon.h"

// --pileup FILE, --sites FILE [--site-min-frac F] [--site-min-count N]
struct DgPileOpts {
    std::string pileup, sites;
    uint32_t min_frac_ppm = 200000u, min_count = 2u;       // this build's own defaults: 0.2 of the depth, two alignments
    bool frac_set = false, count_set = false;
    bool on() const { return !pileup.empty() || !sites.empty(); }
};

// n: the eight counts of the position (A C G T N DEL INS 0); pos0: 0-based; ref: the byte, or 0 for '.'
inline void dg_pileup_line(std::string &out, const std::string &name, uint64_t pos0, char ref, const uint16_t *n) {
    const unsigned depth = (unsigned)n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
    char buf[160];
    snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", (unsigned long long)pos0 + 1ull, ref ? ref : '.', depth,
             (unsigned)n[0], (unsigned)n[1], (unsigned)n[2], (unsigned)n[3], (unsigned)n[4], (unsigned)n[5], (unsigned)n[6]);
    out += name; out += buf;
}

// every position with depth of pipeline target g whose own coordinate lies in [lo, hi); shift: what its coordinates lack
// to the target's (a window's begin); tb: the target's bases from its coordinate 0, or NULL
inline void dg_pileup_lines(std::string &out, const std::string &name, const dagcon_pileup &pu, uint32_t g, uint64_t lo, uint64_t hi,
                            uint64_t shift, const char *tb) {
    const uint64_t b = pu.pos_begin[g], n = pu.pos_begin[g + 1] - b;
    for (uint64_t p = lo; p < hi && p < n; p++) {
        const uint16_t *c = pu.counts + 8 * (b + p);
        if (!(c[0] | c[1] | c[2] | c[3] | c[4] | c[5])) continue;
        dg_pileup_line(out, name, p + shift, tb ? tb[p + shift] : 0, c);
    }
}

// the same for the sites of pipeline target g
inline void dg_site_lines(std::string &out, const std::string &name, const dagcon_pileup_sites &ps, uint32_t g, uint64_t lo, uint64_t hi,
                          uint64_t shift, const char *tb) {
    for (uint64_t s = ps.site_begin[g]; s < ps.site_begin[g + 1]; s++) {
        const uint64_t p = ps.pos[s];
        if (p < lo || p >= hi) continue;
        dg_pileup_line(out, name, p + shift, tb ? tb[p + shift] : 0, ps.counts + 8 * s);
    }
}
