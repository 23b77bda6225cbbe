// site_reads.h -- pbdagcon --site-reads / --haplotag: the arrays of dagcon_site_reads as text lines (host only).
//
// --site-reads FILE, one line per entry, tab-separated: RNAME POS QNAME ALLELE INS.
//   - POS is 1-based, as in --sites; ALLELE is one of A C G T N *, with * for a deleted base; INS is 0 or 1: the read
//     has inserted bases behind the position (which bases is not compared);
//   - a target's lines are in the order of its sites, a site's in the order of the reads' records.
// --haplotag FILE, one line per alignment the graph took: RNAME QNAME HAP SITES.
//   - HAP is 0 (unassigned), 1 or 2; SITES is the number of the read's entries that carry a sign (include/dagcon.h, rule 3;
//     with --link-sites an entry at a site that is not linked carries none, rule 13).
// --linked-sites FILE, one line per site: RNAME POS PARTNERS LINKED, POS 1-based as in --sites (rule 13).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/dagcon.h"

// --site-reads FILE, --haplotag FILE
struct DgSiteReadOpts {
    std::string site_reads, haplotag;
    bool on() const { return !site_reads.empty() || !haplotag.empty(); }
    bool phase() const { return !haplotag.empty(); }
};

// --link-sites [--link-max-conflict F] [--link-min-cell N] [--link-min-partners N] [--link-reach N], --linked-sites FILE
// (which implies --link-sites); 0: the library's default
struct DgLinkOpts {
    bool on = false, opts_set = false;
    std::string linked;
    dagcon_site_link_opts o = {0u, 0u, 0u, 0u};
};

// the sign of an entry at a site with the eight counts n (A C G T N DEL INS 0): rule 3 of dagcon_site_reads; linked: the
// site's byte of dagcon_fetch_site_link, 0 mutes it (rule 13.5) -- without --link-sites every site counts as linked
inline int dg_sr_sign(uint8_t code, const uint16_t *n, const unsigned linked = 1u) {
    if (!linked) return 0;
    unsigned depth = 0, k1 = 0;
    for (unsigned k = 0; k < 6; k++) { depth += n[k]; if (n[k] > n[k1]) k1 = k; }
    unsigned k2 = 7, c2 = 0;
    for (unsigned k = 0; k < 6; k++)
        if (k != k1 && n[k] > c2) { c2 = n[k]; k2 = k; }
    const unsigned ins = n[6], rest = depth >= ins ? depth - ins : 0u;
    if ((ins < rest ? ins : rest) > c2) return (code & 8u) ? -1 : 1;
    const unsigned cls = code & 7u;
    return cls == k1 ? 1 : cls == k2 ? -1 : 0;
}

inline void dg_site_read_line(std::string &out, const std::string &rname, uint64_t pos0, const std::string &qname, uint8_t code) {
    char buf[48];
    snprintf(buf, sizeof buf, "\t%llu\t", (unsigned long long)pos0 + 1ull);
    out += rname; out += buf; out += qname;
    out += '\t'; out += "ACGTN*??"[code & 7u]; out += '\t'; out += (code & 8u) ? '1' : '0'; out += '\n';
}

inline void dg_linked_site_line(std::string &out, const std::string &rname, uint64_t pos0, unsigned partners, unsigned linked) {
    char buf[64];
    snprintf(buf, sizeof buf, "\t%llu\t%u\t%u\n", (unsigned long long)pos0 + 1ull, partners, linked);
    out += rname; out += buf;
}

// the sites of pipeline target g whose position lies in [lo, hi) (a window's core; a whole target: 0 and its length);
// base: the target coordinate of the pipeline target's position 0
inline void dg_linked_site_lines(std::string &out, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_link &sl, uint32_t g, uint32_t lo,
                                 uint32_t hi, uint64_t base) {
    for (uint64_t s = ps.site_begin[g]; s < ps.site_begin[g + 1]; s++)
        if (ps.pos[s] >= lo && ps.pos[s] < hi) dg_linked_site_line(out, rname, base + ps.pos[s], sl.partners[s], sl.linked[s]);
}

inline void dg_haplotag_line(std::string &out, const std::string &rname, const std::string &qname, unsigned hap, uint64_t n_signed) {
    char buf[48];
    snprintf(buf, sizeof buf, "\t%u\t%llu\n", hap, (unsigned long long)n_signed);
    out += rname; out += '\t'; out += qname; out += buf;
}

// The lines of pipeline target g, whose taken alignments are [x0, x1) of sr (aln_tgt ascends: the caller walks it once).
// qnames: the batch's read names, indexed by aln_src.  reads / tags: where the lines go, or NULL.  linked: a byte per site
// (dagcon_fetch_site_link), or NULL without --link-sites
inline void dg_site_read_lines(std::string *reads, std::string *tags, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_reads &sr,
                               uint32_t g, uint64_t x0, uint64_t x1, const std::vector<std::string> &qnames, const uint8_t *linked = nullptr) {
    const uint64_t s0 = ps.site_begin[g], ns = ps.site_begin[g + 1] - s0;
    if (tags)
        for (uint64_t x = x0; x < x1; x++) {
            uint64_t n_signed = 0;
            for (uint64_t e = sr.ent_begin[x]; e < sr.ent_begin[x + 1]; e++) n_signed += dg_sr_sign(sr.ent_code[e], ps.counts + 8 * sr.ent_site[e], linked ? linked[sr.ent_site[e]] : 1u) != 0;
            dg_haplotag_line(*tags, rname, qnames[sr.aln_src[x]], sr.hap ? sr.hap[x] : 0u, n_signed);
        }
    if (!reads || !ns) return;
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
    for (uint64_t k = 0; k < ns; k++)
        for (uint64_t j = at[k]; j < at[k + 1]; j++) dg_site_read_line(*reads, rname, ps.pos[s0 + k], qnames[sr.aln_src[who[j]]], code[j]);
}
