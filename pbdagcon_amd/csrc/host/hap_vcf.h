// hap_vcf.h -- pbdagcon --hap-vcf: diploid calls from the two groups' consensus as VCFv4.2 with one sample (host only).
//
// An unsplit target's lines are the edits of its one consensus: GT 1/1, INFO PAIR=UNSPLIT;DP=span;AD=ref,alt.
// A split target's lines are the edits of its two groups (dagcon_set_hap_calls, include/dagcon.h rule 11), merged by
// (t_pos, label); the HOM mate of label 2 is not written.  GT is group 1 | group 2:
//   label 1: HET 1|0, HOM 1|1, CLASH and NOCOVER 1|.        label 2: HET 0|1, CLASH and NOCOVER .|1
// INFO is PAIR=HET|HOM|CLASH|NOCOV, then DP1=span;AD1=ref,alt of the label-1 edit, DP2 / AD2 of the label-2 edit (a HOM line
// has both).  FORMAT is GT:PS with PS 1: a split target is one block.  RNAME POS . REF ALT are anchored as in --vcf (vcf.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/dagcon.h"
#include "vcf.h"

// an edit of a target or a group: its place, its alt bytes, its support; of a group also its state and the index of its
// mate among the other group's edits (-1: none)
struct DgHapVcfEdit {
    uint32_t t_pos, t_len;
    std::string alt;
    uint32_t span, n_ref, n_alt;
    unsigned state;
    long long mate;
};

inline void dg_hap_vcf_header(std::string &out, const std::string &contigs) {
    out += "##fileformat=VCFv4.2\n";
    out += contigs;
    out += "##INFO=<ID=PAIR,Number=1,Type=String,Description=\"UNSPLIT: the target was not split, the edit is the one consensus' own; HET: only this "
           "group's consensus carries the edit and the other covers it; HOM: both carry it; CLASH: the other group carries another edit that touches "
           "it; NOCOV: the other group has no consensus there (this build's own rule, parity unpinned)\">\n"
           "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Unsplit target: alignments that span the edit's window\">\n"
           "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Unsplit target: spanning alignments that carry the target's allele, the consensus' allele\">\n"
           "##INFO=<ID=DP1,Number=1,Type=Integer,Description=\"Alignments of group 1 that span the edit's window\">\n"
           "##INFO=<ID=AD1,Number=R,Type=Integer,Description=\"Spanning alignments of group 1 that carry the target's allele, the edit's allele\">\n"
           "##INFO=<ID=DP2,Number=1,Type=Integer,Description=\"Alignments of group 2 that span the edit's window\">\n"
           "##INFO=<ID=AD2,Number=R,Type=Integer,Description=\"Spanning alignments of group 2 that carry the target's allele, the edit's allele\">\n"
           "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype: group 1 | group 2 of a split target, 1/1 on an unsplit one\">\n"
           "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set: a split target is one block\">\n"
           "##pbdagcon_note=the reads the split left unlabelled are in both groups: DP1 + DP2 may exceed the target's depth\n"
           "##pbdagcon_note=a CLASH is written as two records, 1|. and .|1, not as one record 1|2; REF and ALT are not normalised\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n";
}

// tb: the target's bases [0, tlen)
inline void dg_hap_vcf_unsplit(std::string &out, const std::string &name, const char *tb, uint32_t tlen, const std::vector<DgHapVcfEdit> &edits) {
    char info[128];
    for (const DgHapVcfEdit &e : edits) {
        dg_vcf_anchored(out, name, tb, tlen, e.t_pos, e.t_len, e.alt.data(), (uint32_t)e.alt.size());
        snprintf(info, sizeof info, "\t.\t.\tPAIR=UNSPLIT;DP=%u;AD=%u,%u\tGT\t1/1\n", e.span, e.n_ref, e.n_alt);
        out += info;
    }
}

inline void dg_hap_vcf_split(std::string &out, const std::string &name, const char *tb, uint32_t tlen, const std::vector<DgHapVcfEdit> &g1,
                             const std::vector<DgHapVcfEdit> &g2) {
    static const char *const pair[4] = {"NOCOV", "HET", "CLASH", "HOM"};
    size_t i = 0, j = 0;
    char buf[192];
    while (i < g1.size() || j < g2.size()) {
        // by (t_pos, label): label 1 first where the two begin at the same place
        const bool first = j >= g2.size() || (i < g1.size() && g1[i].t_pos <= g2[j].t_pos);
        const DgHapVcfEdit &e = first ? g1[i++] : g2[j++];
        const unsigned label = first ? 1u : 2u;
        if (!first && e.state == DAGCON_HC_HOM) continue;                       // written with its mate
        dg_vcf_anchored(out, name, tb, tlen, e.t_pos, e.t_len, e.alt.data(), (uint32_t)e.alt.size());
        snprintf(buf, sizeof buf, "\t.\t.\tPAIR=%s;DP%u=%u;AD%u=%u,%u", pair[e.state & 3u], label, e.span, label, e.n_ref, e.n_alt);
        out += buf;
        if (e.state == DAGCON_HC_HOM && e.mate >= 0 && (size_t)e.mate < g2.size()) {
            const DgHapVcfEdit &m = g2[(size_t)e.mate];
            snprintf(buf, sizeof buf, ";DP2=%u;AD2=%u,%u", m.span, m.n_ref, m.n_alt);
            out += buf;
        }
        const char *other = e.state == DAGCON_HC_HOM ? "1" : e.state == DAGCON_HC_HET ? "0" : ".";
        out += "\tGT:PS\t";
        if (first) { out += "1|"; out += other; } else { out += other; out += "|1"; }
        out += ":1\n";
    }
}
