// site_reads.h -- pbdagcon --site-reads / --haplotag: the arrays of dagcon_site_reads as text lines (host only).
//
// --site-reads FILE, one line per entry, tab-separated: RNAME POS QNAME ALLELE INS.
//   - POS is 1-based, as in --sites; ALLELE is one of A C G T N *, with * for a deleted base; INS is 0 or 1: the read
//     has inserted bases behind the position (which bases is not compared);
//   - a target's lines are in the order of its sites, a site's in the order of the reads' records.
// --haplotag FILE, one line per alignment the graph took: RNAME QNAME HAP SITES.
//   - HAP is 0 (unassigned), 1 or 2; SITES is the number of the read's entries that carry a sign (include/dagcon.h, rule 3).
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

// the sign of an entry at a site with the eight counts n (A C G T N DEL INS 0): rule 3 of dagcon_site_reads
inline int dg_sr_sign(uint8_t code, const uint16_t *n) {
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

inline void dg_haplotag_line(std::string &out, const std::string &rname, const std::string &qname, unsigned hap, uint64_t n_signed) {
    char buf[48];
    snprintf(buf, sizeof buf, "\t%u\t%llu\n", hap, (unsigned long long)n_signed);
    out += rname; out += '\t'; out += qname; out += buf;
}

// The lines of pipeline target g, whose taken alignments are [x0, x1) of sr (aln_tgt ascends: the caller walks it once).
// qnames: the batch's read names, indexed by aln_src.  reads / tags: where the lines go, or NULL
inline void dg_site_read_lines(std::string *reads, std::string *tags, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_reads &sr,
                               uint32_t g, uint64_t x0, uint64_t x1, const std::vector<std::string> &qnames) {
    const uint64_t s0 = ps.site_begin[g], ns = ps.site_begin[g + 1] - s0;
    if (tags)
        for (uint64_t x = x0; x < x1; x++) {
            uint64_t n_signed = 0;
            for (uint64_t e = sr.ent_begin[x]; e < sr.ent_begin[x + 1]; e++) n_signed += dg_sr_sign(sr.ent_code[e], ps.counts + 8 * sr.ent_site[e]) != 0;
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
