// hap_contigs.h -- `pbdagcon --window W --phase-windows --hap-contigs FILE [--hap-windows FILE]`: two phased sequences per
// phase block, joined across windows from the consensus of each window's two read groups (host only;
// tests/hap_contigs_twin.py is its twin).
//
// Per group of windows, behind the first batch's fetch and the plain stitch (windows.h), which stay as they are: the
// window phase gives flip and block per window (rule 9 of include/dagcon.h, with the host's link across the groups), the
// tally gives split; then dagcon_set_window_keep with the windows' cores, dagcon_upload_haps_swapped(swap = flip), run,
// fetch, dagcon_fetch_hap_map, dagcon_fetch_window_keep.  The derived batch's positions are never fetched: of every
// segment the device hands back its kept part [i0, i1) and the positions of its two ends (rule 12), 16 bytes.
//
// The stitch (DgHapStitch), per label g in {1, 2} over the derived windows of that label in window order.  A kept part
// continues the piece before it iff it was cut at its core begin (i0 > 0), that piece is the kept part just before it in
// this order, comes from window w - 1, was cut at its core end, and block[w] == block[w - 1].  In every other case there
// is a break: an unsplit window in between has no derived window, so the piece before it is not from w - 1.  The state
// carries across the groups of --batch-targets.  Pieces shorter than -m are dropped.  The join works on the keep records,
// so it is O(segments); the bases move with append of [i0, i1).
//
// --hap-contigs FILE, FASTA: >RNAME/hap{1|2}/PS/t0_t1 with t0 = p_first + window begin - 1 and t1 = p_last + window begin
//   (target coordinates) and PS = 1 + the core begin of the block's first window, as --haplotag prints it.  A target's
//   records are ordered by t0, label 1 before label 2 at equal t0.
// --hap-windows FILE, tab-separated.  One line per window: #window RNAME BEGIN END PS N1 N2 N0 SEP AGREE DISAGREE SPLIT
//   (BEGIN, END: the core, 0-based half-open; the counts of rule 6 for the window); behind it one line per site with a phase
//   inside the window's core: RNAME POS PHASE P1 M1 P2 M2, POS 1-based in target coordinates.  All of it is in the block's
//   orientation: under flip N1 / N2 and P1 M1 / P2 M2 change places and PHASE changes sign; SEP, AGREE, DISAGREE and SPLIT
//   are symmetric.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct DgHapPiece {
    long long t0 = 0, t1 = 0;
    uint64_t block = 0;
    std::string seq;
};

// the pieces of one label of one target, fed derived window by derived window in order
struct DgHapStitch {
    std::vector<DgHapPiece> pieces;
    long long open_w = -1;                                 // window of the last kept part, if it was cut at its core end
    uint64_t open_block = 0;                               // and that window's block
    void reset() { pieces.clear(); open_w = -1; open_block = 0; }
    // one segment of n bases of window w = [begin, ..) of `block`, with its keep record
    void add(long long w, uint32_t begin, uint64_t block, const char *seq, uint32_t n, uint32_t i0, uint32_t i1, uint32_t p_first, uint32_t p_last) {
        if (i1 <= i0 || i1 > n) return;
        if (i0 > 0 && open_w >= 0 && open_w == w - 1 && open_block == block && !pieces.empty()) {
            DgHapPiece &p = pieces.back();
            p.t1 = (long long)p_last + begin;
            p.seq.append(seq + i0, i1 - i0);
        } else {
            pieces.emplace_back();
            DgHapPiece &p = pieces.back();
            p.t0 = (long long)p_first + begin - 1; p.t1 = (long long)p_last + begin; p.block = block;
            p.seq.assign(seq + i0, i1 - i0);
        }
        open_w = i1 < n ? w : -1;
        open_block = block;
    }
};

// >RNAME/hap{1|2}/PS/t0_t1
inline void dg_hap_contig_record(std::string &out, const std::string &rname, unsigned label, uint64_t ps, long long t0, long long t1, const std::string &seq) {
    char buf[96];
    snprintf(buf, sizeof buf, "/hap%u/%llu/%lld_%lld\n", label, (unsigned long long)ps, t0, t1);
    out += '>'; out += rname; out += buf;
    out += seq; out += '\n';
}

// a target's records: by t0, label 1 before label 2 at equal t0; pieces shorter than min_len are dropped.  ps(block): 1 +
// the core begin of the block's first window
template <class Ps>
inline void dg_hap_contig_records(std::string &out, const std::string &rname, const DgHapStitch st[2], size_t min_len, Ps ps) {
    struct Ref { long long t0; unsigned label; const DgHapPiece *p; };
    std::vector<Ref> v;
    for (unsigned g = 0; g < 2; g++)
        for (const DgHapPiece &p : st[g].pieces)
            if (p.seq.size() >= min_len) v.push_back(Ref{p.t0, g + 1u, &p});
    std::stable_sort(v.begin(), v.end(), [](const Ref &a, const Ref &b) { return a.t0 != b.t0 ? a.t0 < b.t0 : a.label < b.label; });
    for (const Ref &r : v) dg_hap_contig_record(out, rname, r.label, ps(r.p->block), r.p->t0, r.p->t1, r.p->seq);
}

// #window RNAME BEGIN END PS N1 N2 N0 SEP AGREE DISAGREE SPLIT, in the block's orientation
inline void dg_hap_window_line(std::string &out, const std::string &rname, uint64_t begin, uint64_t end, uint64_t ps, uint32_t n1, uint32_t n2, uint32_t n0,
                               uint32_t n_sep, uint32_t agree, uint32_t disagree, unsigned split, bool flip) {
    char buf[192];
    if (flip) std::swap(n1, n2);
    snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", (unsigned long long)begin, (unsigned long long)end, (unsigned long long)ps,
             n1, n2, n0, n_sep, agree, disagree, split);
    out += "#window\t"; out += rname; out += buf;
}

// RNAME POS PHASE P1 M1 P2 M2 (pos1: 1-based, target coordinates; c: P1 M1 P2 M2 in the window's own names), in the block's orientation
inline void dg_hap_window_site_line(std::string &out, const std::string &rname, uint64_t pos1, int phase, const uint16_t *c, bool flip) {
    char buf[128];
    const unsigned a = flip ? 2 : 0, b = flip ? 0 : 2;
    snprintf(buf, sizeof buf, "\t%llu\t%d\t%u\t%u\t%u\t%u\n", (unsigned long long)pos1, flip ? -phase : phase, (unsigned)c[a], (unsigned)c[a + 1], (unsigned)c[b], (unsigned)c[b + 1]);
    out += rname; out += buf;
}
