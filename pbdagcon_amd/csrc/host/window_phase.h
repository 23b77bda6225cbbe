// window_phase.h -- `pbdagcon --window W --phase-windows`: the read labels of neighbouring windows joined into blocks
// (include/dagcon.h, rule 9), as far as the host has a hand in it (host only; tests/window_phase_twin.py is its twin).
//
// Inside a group of windows the links are the device's (dagcon_fetch_window_phase).  Between two groups -- the last
// window of one, the first of the next, same target -- the host applies rules 9.2 to 9.4 to that one pair from the arrays
// it has fetched anyway (dg_wp_pair, dg_wp_step), and the orientation and the block carry over: the output does not depend
// on --batch-targets.
//
// --haplotag FILE with --phase-windows, one line per record that has at least one taken piece: RNAME QNAME HAP SITES PS.
//   - a record's pieces with an oriented label != 0 vote.  The block with the most such pieces is the record's block, ties
//     to the lower block.  V = (#label 1) - (#label 2) among its pieces in that block; HAP is 1 for V > 0, 2 for V < 0,
//     else 0;
//   - PS is 1 + the core begin of the block's first window, `.` when no piece is labelled;
//   - SITES counts the record's signed entries at sites inside the cores of their windows: no site counts twice.
// --site-reads FILE with --phase-windows: the line of site_reads.h for the entries at sites inside the core of their
// window, POS in target coordinates; sites ascend, a site's reads are in record order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "site_reads.h"

// --phase-windows [--phase-min-links N] [--phase-max-conflict F]
struct DgWinPhaseOpts {
    bool on = false, links_set = false, conflict_set = false;
    unsigned min_links = 0, max_conflict_ppm = 0;          // 0: the library's defaults, 3 and 250000
};

// rule 9.3 (0: the defaults)
inline bool dg_wp_linked(uint64_t same, uint64_t diff, uint32_t min_links, uint32_t max_conflict_ppm) {
    const uint64_t ml = min_links ? min_links : 3u, ppm = max_conflict_ppm ? max_conflict_ppm : 250000u;
    const uint64_t hi = std::max(same, diff), lo = std::min(same, diff);
    return hi >= ml && hi > lo && lo * 1000000ull <= ppm * (hi + lo);
}

// a taken piece of a window: its record, and its label in the window's own names (0, 1, 2)
struct DgWpPiece { uint64_t rec; uint8_t hap; };

// rule 9.2 for one pair of windows; either list ascends in rec (the pieces of a window keep the order of their records)
inline void dg_wp_pair(const std::vector<DgWpPiece> &prev, const std::vector<DgWpPiece> &cur, uint32_t &same, uint32_t &diff) {
    same = diff = 0;
    size_t i = 0;
    for (const DgWpPiece &c : cur) {
        while (i < prev.size() && prev[i].rec < c.rec) i++;
        if (i == prev.size()) break;
        if (prev[i].rec != c.rec || !c.hap || !prev[i].hap) continue;
        if (prev[i].hap == c.hap) same++; else diff++;
    }
}

// rule 9.4 for window w: its orientation and block from its predecessor's (has_prev: rule 9.1)
struct DgWpLink { uint8_t flip; uint64_t block; };
inline DgWpLink dg_wp_step(bool has_prev, const DgWpLink &prev, uint64_t w, uint32_t same, uint32_t diff, uint32_t min_links, uint32_t max_conflict_ppm) {
    if (!has_prev || !dg_wp_linked(same, diff, min_links, max_conflict_ppm)) return DgWpLink{0, w};
    return DgWpLink{(uint8_t)(prev.flip ^ (diff > same ? 1u : 0u)), prev.block};
}

// a piece's vote: the block of its window and its oriented label
struct DgWpVote { uint64_t block; uint8_t hap; };

// the record's HAP and block from its pieces; false: no piece is labelled
inline bool dg_wp_vote(const std::vector<DgWpVote> &pieces, unsigned &hap, uint64_t &block) {
    std::vector<DgWpVote> v;
    for (const DgWpVote &p : pieces) if (p.hap) v.push_back(p);
    hap = 0; block = 0;
    if (v.empty()) return false;
    std::sort(v.begin(), v.end(), [](const DgWpVote &a, const DgWpVote &b) { return a.block < b.block; });
    size_t best_n = 0;
    long long best_v = 0;
    for (size_t i = 0; i < v.size();) {
        size_t z = i;
        long long vote = 0;
        for (; z < v.size() && v[z].block == v[i].block; z++) vote += v[z].hap == 1u ? 1 : -1;
        if (z - i > best_n) { best_n = z - i; best_v = vote; block = v[i].block; }      // (blocks ascend: a tie stays with the lower)
        i = z;
    }
    hap = best_v > 0 ? 1u : best_v < 0 ? 2u : 0u;
    return true;
}

// ps: 1 + the core begin of the block's first window (labelled == false: `.`)
inline void dg_wp_haplotag_line(std::string &out, const std::string &rname, const std::string &qname, unsigned hap, uint64_t sites, bool labelled, uint64_t ps) {
    char buf[64];
    snprintf(buf, sizeof buf, "\t%u\t%llu\t", hap, (unsigned long long)sites);
    out += rname; out += '\t'; out += qname; out += buf;
    if (labelled) out += std::to_string(ps); else out += '.';
    out += '\n';
}

// --site-reads: the lines of window g = [begin, ..) whose taken alignments are [x0, x1) of sr, for its sites at window
// positions [lo, hi) (its core).  name(x): the read name of alignment x
template <class Name>
inline void dg_wp_site_read_lines(std::string &out, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_reads &sr, uint32_t g,
                                  uint64_t x0, uint64_t x1, uint32_t lo, uint32_t hi, uint32_t begin, Name name) {
    const uint64_t s0 = ps.site_begin[g], ns = ps.site_begin[g + 1] - s0;
    if (!ns || x0 == x1) return;
    // the entries are alignment by alignment; the file is site by site: count, prefix, place (the reads stay in their order)
    std::vector<uint64_t> at(ns + 1, 0);
    for (uint64_t e = sr.ent_begin[x0]; e < sr.ent_begin[x1]; e++) at[sr.ent_site[e] - s0 + 1]++;
    for (uint64_t k = 0; k < ns; k++) at[k + 1] += at[k];
    std::vector<uint64_t> who(at[ns]);
    std::vector<uint8_t> code(at[ns]);
    std::vector<uint64_t> to(at.begin(), at.end() - 1);
    for (uint64_t x = x0; x < x1; x++)
        for (uint64_t e = sr.ent_begin[x]; e < sr.ent_begin[x + 1]; e++) {
            const uint64_t j = to[sr.ent_site[e] - s0]++;
            who[j] = x; code[j] = sr.ent_code[e];
        }
    for (uint64_t k = 0; k < ns; k++) {
        const uint32_t p = ps.pos[s0 + k];
        if (p < lo || p >= hi) continue;
        for (uint64_t j = at[k]; j < at[k + 1]; j++) dg_site_read_line(out, rname, (uint64_t)p + begin, name(who[j]), code[j]);
    }
}
