// joined.h -- pbdagcon --joined-alleles / --joined-vcf: the tables of dagcon_joined_sites as text lines (host only; rule 10.5
// of include/dagcon.h).
//
// --joined-alleles FILE, one line per joined allele of a run's table, tab-separated:
//   RNAME POS END REF SPAN PARTIAL ALLELE COUNT H1 H2 H0
//   - POS and END: the run's first and last position, 1-based inclusive; REF: the target's bytes there, "." without them;
//   - SPAN, PARTIAL: the alignments with a column at every position of the run, and at some but not all of them;
//   - ALLELE: what COUNT of the spanning alignments show between the run's first target base and the one behind its last:
//     the texts of the sites' alleles one after the other, "-" for none, "*" when the allele is opaque (a site's allele
//     past the 15th of its table, or a long one);
//   - a target's runs ascending, a run's alleles by COUNT descending, ties by the joined keys' own order;
//   - H1 H2 H0: the COUNT alignments by the label of the split (1, 2, none); "." without a split.
// --joined-vcf FILE, VCFv4.2, one record per run with at least one ALT:
//   RNAME POS . REF ALT . . DP=spanning;PART=partial;AD=ref,alt1,..[;AD1=..;AD2=..]
//   - REF is the run's target bytes; ALT is every joined allele that is not opaque, whose bases differ from the run's
//     target bases as the pile-up classifies them, and that has COUNT >= --site-min-count.  Joined alleles with the same
//     bases (the same bases split differently over the sites) are one ALT, their counts added; AD's first number counts
//     every allele that is not opaque and has the target's bases;
//   - an empty ALT has no text of its own: every allele of its record then takes the target base in front as anchor,
//     POS = the anchor's; at position 1 the base behind the run instead; a run that covers its whole target has no record;
//   - shared leading and trailing bases of REF and ALT are NOT trimmed.  No genotype is called.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "alleles.h"

// --joined-alleles FILE, --joined-vcf FILE
struct DgJoinedOpts {
    std::string alleles, vcf;
    bool on() const { return !alleles.empty() || !vcf.empty(); }
};

// The text of a joined key over the m sites from s0 on (rule 10.5).  al_begin / al_key: dagcon_site_alleles' arrays.
// false: the allele is opaque, and out is "*"
inline bool dg_joined_text(std::string &out, uint64_t key, const uint64_t *al_begin, const uint64_t *al_key, uint64_t s0, uint32_t m) {
    out.clear();
    for (uint32_t j = 0; j < m && j < 16u; j++) {
        const unsigned c = (unsigned)(key >> (4u * (15u - j))) & 15u;
        const uint64_t a0 = al_begin[s0 + j], a1 = al_begin[s0 + j + 1];
        if (c == 15u || c >= a1 - a0 || (al_key[a0 + c] & DG_ALLELE_LONG)) { out = "*"; return false; }
        if (al_key[a0 + c]) out += dg_allele_str(al_key[a0 + c]);
    }
    if (out.empty()) out = "-";
    return true;
}

// ref: the run's target bytes, or NULL for '.'; hap: c1 c2 c0, or NULL for '.'
inline void dg_joined_allele_line(std::string &out, const std::string &rname, uint64_t pos0, uint32_t m, const char *ref, uint32_t span, uint32_t partial,
                                  const std::string &text, uint32_t count, const uint16_t *hap) {
    out += rname; out += '\t'; out += std::to_string(pos0 + 1); out += '\t'; out += std::to_string(pos0 + m); out += '\t';
    if (ref) out.append(ref, m); else out += '.';
    out += '\t'; out += std::to_string(span); out += '\t'; out += std::to_string(partial); out += '\t'; out += text; out += '\t'; out += std::to_string(count);
    for (int j = 0; j < 3; j++) { out += '\t'; out += hap ? std::to_string((unsigned)hap[j]) : std::string("."); }
    out += '\n';
}

inline void dg_joined_vcf_header(std::string &out, const std::string &contigs, bool split) {
    out += "##fileformat=VCFv4.2\n"
           "##source=pbdagcon --joined-vcf (this build's own rule, parity unpinned)\n";
    out += contigs;
    out += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Alignments with a column at every target base of the record's run of adjacent sites\">\n"
           "##INFO=<ID=PART,Number=1,Type=Integer,Description=\"Alignments with a column at some but not all of them: not counted in AD\">\n"
           "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Alignments of DP that show the REF bases and each ALT between the run's first target base and the one behind its last\">\n";
    if (split)
        out += "##INFO=<ID=AD1,Number=R,Type=Integer,Description=\"AD among the alignments of read group 1\">\n"
               "##INFO=<ID=AD2,Number=R,Type=Integer,Description=\"AD among the alignments of read group 2\">\n";
    out += "##pbdagcon_note=adjacent sites are joined into runs of at most 16: a longer stretch is several records\n"
           "##pbdagcon_note=shared leading and trailing bases of REF and ALT are not trimmed\n"
           "##pbdagcon_note=no genotype is called\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
}

// tb: the target's bases [0, tlen); the run [pos0, pos0 + m); its table: n joined alleles (text, opaque, count, hap: c1 c2
// c0 per allele or NULL).  A run without an ALT, and a run that covers its whole target, has no record
inline void dg_joined_vcf_record(std::string &out, const std::string &rname, const char *tb, uint32_t tlen, uint32_t pos0, uint32_t m, uint32_t span, uint32_t partial,
                                 const std::vector<std::string> &text, const std::vector<uint8_t> &opaque, const uint32_t *count, const uint16_t *hap, uint32_t min_count) {
    if (!m || pos0 >= tlen || m > tlen - pos0 || m == tlen) return;
    std::string cls;                                                       // the run's target bases as the pile-up classifies them
    for (uint32_t j = 0; j < m; j++) { const char b = (char)(tb[pos0 + j] & 0xDF); cls += b == 'A' || b == 'C' || b == 'G' || b == 'T' ? b : 'N'; }
    struct Alt { std::string text; uint64_t ad[3]; };
    std::vector<Alt> alt;
    uint64_t ref_ad[3] = {0, 0, 0};
    bool empty = false;
    for (size_t i = 0; i < text.size(); i++) {
        if (opaque[i]) continue;
        const std::string bases = text[i] == "-" ? std::string() : text[i];
        const uint64_t add[3] = {count[i], hap ? hap[3 * i] : 0u, hap ? hap[3 * i + 1] : 0u};
        if (bases == cls) { for (int j = 0; j < 3; j++) ref_ad[j] += add[j]; continue; }
        if (count[i] < min_count) continue;
        auto at = std::find_if(alt.begin(), alt.end(), [&](const Alt &a) { return a.text == bases; });
        if (at == alt.end()) { alt.push_back({bases, {0, 0, 0}}); at = alt.end() - 1; }
        for (int j = 0; j < 3; j++) at->ad[j] += add[j];
        empty = empty || bases.empty();
    }
    if (alt.empty()) return;
    std::string front, behind;
    uint64_t pos = (uint64_t)pos0 + 1;
    if (empty) {
        if (pos0 > 0) { front = std::string(1, tb[pos0 - 1]); pos = pos0; }
        else behind = std::string(1, tb[pos0 + m]);
    }
    out += rname; out += '\t'; out += std::to_string(pos); out += "\t.\t"; out += front + std::string(tb + pos0, m) + behind; out += '\t';
    for (size_t a = 0; a < alt.size(); a++) { if (a) out += ','; out += front + alt[a].text + behind; }
    out += "\t.\t.\tDP="; out += std::to_string(span); out += ";PART="; out += std::to_string(partial);
    static const char *const name[3] = {";AD=", ";AD1=", ";AD2="};
    for (int j = 0; j < (hap ? 3 : 1); j++) {
        out += name[j]; out += std::to_string(ref_ad[j]);
        for (const Alt &a : alt) { out += ','; out += std::to_string(a.ad[j]); }
    }
    out += '\n';
}

// The lines of pipeline target g.  lines / vcf: where they go, or NULL; tb: the target's bases, or NULL (no REF, no VCF)
inline void dg_joined_lines(std::string *lines, std::string *vcf, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_alleles &sa,
                            const dagcon_joined_sites &js, uint32_t g, const char *tb, uint32_t tlen, uint32_t min_count) {
    const uint64_t s0 = ps.site_begin[g], s1 = ps.site_begin[g + 1];
    uint64_t r = (uint64_t)(std::lower_bound(js.run_begin, js.run_begin + js.n_runs, s0) - js.run_begin);
    std::vector<std::string> text;
    std::vector<uint8_t> opaque;
    for (; r < js.n_runs && js.run_begin[r] < s1; r++) {
        const uint64_t b = js.run_begin[r], a0 = js.jal_begin[r], a1 = js.jal_begin[r + 1];
        const uint32_t m = (uint32_t)(js.run_begin[r + 1] - b), pos0 = ps.pos[b];
        text.assign((size_t)(a1 - a0), std::string()); opaque.assign((size_t)(a1 - a0), 0);
        for (uint64_t i = a0; i < a1; i++) opaque[i - a0] = !dg_joined_text(text[i - a0], js.key[i], sa.al_begin, sa.key, b, m);
        if (lines)
            for (uint64_t i = a0; i < a1; i++)
                dg_joined_allele_line(*lines, rname, pos0, m, tb ? tb + pos0 : nullptr, js.spanning[r], js.partial[r], text[i - a0], js.count[i],
                                      js.hap_count ? js.hap_count + 3 * i : nullptr);
        if (vcf && tb)
            dg_joined_vcf_record(*vcf, rname, tb, tlen, pos0, m, js.spanning[r], js.partial[r], text, opaque, js.count + a0, js.hap_count ? js.hap_count + 3 * a0 : nullptr, min_count);
    }
}
