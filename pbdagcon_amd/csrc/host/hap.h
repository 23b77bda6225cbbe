// hap.h -- pbdagcon --hap-consensus / --hap-sites: the tally of dagcon_hap_tally as text lines, and the names of the
// groups' records (host only).
//
// --hap-sites FILE, tab-separated.  One line per target: #target RNAME N1 N2 N0 SEP AGREE DISAGREE SPLIT (include/dagcon.h,
//   rule 6); behind it one line per site of the target with a phase: RNAME POS PHASE P1 M1 P2 M2, POS as in --sites.
// --hap-consensus FILE: one FASTA record per segment of every group of a split target, >RNAME/hap{1|2}/r0_r1.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../../include/dagcon.h"

// --hap-consensus FILE, --hap-sites FILE, --hap-vcf FILE (hap_vcf.h) [--hap-min-sites N] [--hap-min-reads N]
struct DgHapOpts {
    std::string consensus, sites, vcf;
    unsigned min_sites = 0, min_reads = 0;      // 0: the library's defaults
    bool sites_set = false, reads_set = false;
    bool on() const { return !consensus.empty() || !sites.empty() || !vcf.empty(); }
};

inline void dg_hap_target_line(std::string &out, const std::string &rname, uint32_t n1, uint32_t n2, uint32_t n0, uint32_t n_sep, uint32_t agree,
                               uint32_t disagree, unsigned split) {
    char buf[96];
    snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", n1, n2, n0, n_sep, agree, disagree, split);
    out += "#target\t"; out += rname; out += buf;
}

// c: P1 M1 P2 M2
inline void dg_hap_site_line(std::string &out, const std::string &rname, uint64_t pos0, int phase, const uint16_t *c) {
    char buf[96];
    snprintf(buf, sizeof buf, "\t%llu\t%d\t%u\t%u\t%u\t%u\n", (unsigned long long)pos0 + 1ull, phase, (unsigned)c[0], (unsigned)c[1], (unsigned)c[2], (unsigned)c[3]);
    out += rname; out += buf;
}

// the id a group's records are written under: RNAME/hap1 or RNAME/hap2 (the writer adds /r0_r1)
inline std::string dg_hap_id(const std::string &rname, unsigned label) {
    return rname + (label == 1u ? "/hap1" : "/hap2");
}
