// vcf.h -- pbdagcon --vcf: the edits of dagcon_edits with the counts of dagcon_edit_support as VCFv4.2 lines (host only).
//
// One line per edit, in output order: RNAME POS . REF ALT . . DP=span;AD=ref,alt;WIN=gL+1-gR.
//   - an edit with bytes on both sides keeps its own coordinates: POS = t_pos + 1;
//   - a pure insertion or deletion takes the target base in front of it as anchor on both sides: POS = t_pos;
//   - at position 0 it takes the base behind it instead: POS = 1 (a target with no base left on either side of the edit
//     has no anchor: the empty side is written as '.').
// WIN is the group's window as a 1-based closed interval; an empty window [g, g) reads g+1-g.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

inline void dg_vcf_header(std::string &out) {
    out += "##fileformat=VCFv4.2\n";
}

inline void dg_vcf_contig(std::string &out, const std::string &name, uint32_t tlen) {
    out += "##contig=<ID=" + name + ",length=" + std::to_string(tlen) + ">\n";
}

inline void dg_vcf_columns(std::string &out) {
    out += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Alignments that span the edit's window (this build's own rule, parity unpinned)\">\n"
           "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Spanning alignments that carry the target's allele, the consensus' allele\">\n"
           "##INFO=<ID=WIN,Number=1,Type=String,Description=\"Window of the edit's group on the target, 1-based, closed: every place the same change could be written\">\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
}

// the first five columns of a line, RNAME POS . REF ALT, anchored by the rule above (--hap-vcf writes them too)
// tb: the target's bases [0, tlen); alt: the c_len replacing bytes
inline void dg_vcf_anchored(std::string &out, const std::string &name, const char *tb, uint32_t tlen, uint32_t t_pos, uint32_t t_len,
                            const char *alt, uint32_t c_len) {
    std::string ref(tb + t_pos, t_len), al(alt, c_len);
    uint64_t pos = (uint64_t)t_pos + 1;
    if (!t_len || !c_len) {
        if (t_pos > 0) { ref.insert(ref.begin(), tb[t_pos - 1]); al.insert(al.begin(), tb[t_pos - 1]); pos = t_pos; }
        else if (t_pos + t_len < tlen) { ref += tb[t_pos + t_len]; al += tb[t_pos + t_len]; pos = 1; }
        else { if (ref.empty()) ref = "."; if (al.empty()) al = "."; pos = 1; }
    }
    out += name; out += '\t'; out += std::to_string(pos); out += "\t.\t"; out += ref; out += '\t'; out += al;
}

inline void dg_vcf_line(std::string &out, const std::string &name, const char *tb, uint32_t tlen, uint32_t t_pos, uint32_t t_len,
                        const char *alt, uint32_t c_len, uint32_t span, uint32_t n_ref, uint32_t n_alt, uint32_t gL, uint32_t gR) {
    dg_vcf_anchored(out, name, tb, tlen, t_pos, t_len, alt, c_len);
    char info[128];
    snprintf(info, sizeof info, "\t.\t.\tDP=%u;AD=%u,%u;WIN=%u-%u\n", span, n_ref, n_alt, gL + 1u, gR);
    out += info;
}
