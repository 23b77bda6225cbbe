// alleles.h -- pbdagcon --site-alleles / --site-vcf: the tables of dagcon_site_alleles as text lines (host only), and the
// text of an allele's key (dagcon_allele_text is dg_allele_text).
//
// --site-alleles FILE, one line per allele of a site's table, tab-separated: RNAME POS REF DEPTH ALLELE COUNT H1 H2 H0.
//   - POS, REF and DEPTH as in --sites; ALLELE is the read's bases between this target base and the next: the bases, "-"
//     for none (a deletion), a trailing "+" when there are more than 20 (alleles that agree in their first 20 are one);
//   - a target's sites ascending, a site's alleles by COUNT descending, ties by the alleles' own order;
//   - H1 H2 H0: the COUNT reads by the label of the split (1, 2, none); "." without a split.
// --site-vcf FILE, VCFv4.2, one record per site with at least one ALT: RNAME POS . REF ALT . . DP=..;AD=..[;AD1=..;AD2=..].
//   - ALT is every allele of the table that is not long, is not the REF base and has COUNT >= --site-min-count;
//   - an empty ALT has no text of its own: every allele of its record then takes the target base in front as anchor,
//     POS = the anchor's; at position 1 the base behind instead; a target of one base has no records;
//   - adjacent sites are NOT joined: a deletion of three bases is three records.  No genotype is called.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/dagcon.h"

// --site-alleles FILE, --site-vcf FILE
struct DgAlleleOpts {
    std::string alleles, vcf;
    bool on() const { return !alleles.empty() || !vcf.empty(); }
};

#define DG_ALLELE_LONG (1ull << 60)

// rule 8 of include/dagcon.h: 20 places of 3 bits from bit 57 down, codes 1..5 for A C G T N, 0 behind the last base; bit 60: long
inline int dg_allele_text(uint64_t key, char *out, size_t cap) {
    if (!out || (key >> 61)) return DAGCON_ERR_INVALID_ARG;
    char buf[24];
    size_t n = 0;
    for (int j = 0; j < 20; j++) {
        const unsigned code = (unsigned)(key >> (3 * (19 - j))) & 7u;
        if (!code) {
            // the bases are a prefix: nothing stands behind the first empty place
            if (key & ((1ull << (3 * (19 - j))) - 1ull)) return DAGCON_ERR_INVALID_ARG;
            break;
        }
        if (code > 5u) return DAGCON_ERR_INVALID_ARG;
        buf[n++] = "ACGTN"[code - 1u];
    }
    const bool is_long = (key & DG_ALLELE_LONG) != 0;
    if (is_long && n != 20) return DAGCON_ERR_INVALID_ARG;
    if (!n) buf[n++] = '-';
    if (is_long) buf[n++] = '+';
    if (cap < n + 1) return DAGCON_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) out[i] = buf[i];
    out[n] = 0;
    return DAGCON_OK;
}

inline std::string dg_allele_str(uint64_t key) {
    char buf[24];
    return dg_allele_text(key, buf, sizeof buf) == DAGCON_OK ? std::string(buf) : std::string("?");
}

// the key of the one-base allele a target byte stands for (the pile-up's classification)
inline uint64_t dg_allele_ref_key(char ref) {
    unsigned code = 5u;
    switch (ref & 0xDF) { case 'A': code = 1u; break; case 'C': code = 2u; break; case 'G': code = 3u; break; case 'T': code = 4u; break; default: break; }
    return (uint64_t)code << 57;
}

// n: the site's eight counts; ref: the byte, or 0 for '.'; hap: c1 c2 c0, or NULL for '.'
inline void dg_site_allele_line(std::string &out, const std::string &rname, uint64_t pos0, char ref, const uint16_t *n, uint64_t key, uint32_t count,
                                const uint16_t *hap) {
    const unsigned depth = (unsigned)n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
    char buf[96];
    snprintf(buf, sizeof buf, "\t%llu\t%c\t%u\t", (unsigned long long)pos0 + 1ull, ref ? ref : '.', depth);
    out += rname; out += buf; out += dg_allele_str(key);
    if (hap) snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%u\n", count, (unsigned)hap[0], (unsigned)hap[1], (unsigned)hap[2]);
    else snprintf(buf, sizeof buf, "\t%u\t.\t.\t.\n", count);
    out += buf;
}

inline void dg_site_vcf_header(std::string &out, const std::string &contigs, bool split) {
    out += "##fileformat=VCFv4.2\n"
           "##source=pbdagcon --site-vcf (this build's own rule, parity unpinned)\n";
    out += contigs;
    out += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Alignments with a column at the site's target base\">\n"
           "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Alignments that show the REF allele and each ALT allele between this target base and the next\">\n";
    if (split)
        out += "##INFO=<ID=AD1,Number=R,Type=Integer,Description=\"AD among the alignments of read group 1\">\n"
               "##INFO=<ID=AD2,Number=R,Type=Integer,Description=\"AD among the alignments of read group 2\">\n";
    out += "##pbdagcon_note=adjacent sites are not joined: a deletion of three bases is three records\n"
           "##pbdagcon_note=no genotype is called\n"
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
}

// tb: the target's bases [0, tlen); the site's table: n_al alleles (key, count, hap: c1 c2 c0 per allele or NULL); a site
// without an ALT, and every site of a target of one base, has no record
inline void dg_site_vcf_record(std::string &out, const std::string &rname, const char *tb, uint32_t tlen, uint32_t pos0, const uint16_t *n,
                               const uint64_t *key, const uint32_t *count, const uint16_t *hap, uint64_t n_al, uint32_t min_count) {
    if (tlen < 2u || pos0 >= tlen) return;
    const uint64_t ref_key = dg_allele_ref_key(tb[pos0]);
    std::vector<uint64_t> alt;
    uint64_t ref_at = n_al;
    bool empty = false;
    for (uint64_t i = 0; i < n_al; i++) {
        if (key[i] == ref_key) { ref_at = i; continue; }
        if ((key[i] & DG_ALLELE_LONG) || count[i] < min_count) continue;
        alt.push_back(i);
        empty = empty || key[i] == 0;
    }
    if (alt.empty()) return;
    std::string ref(1, tb[pos0]), front, behind;
    uint64_t pos = (uint64_t)pos0 + 1;
    if (empty) {
        if (pos0 > 0) { front = std::string(1, tb[pos0 - 1]); pos = pos0; }
        else behind = std::string(1, tb[1]);
    }
    out += rname; out += '\t'; out += std::to_string(pos); out += "\t.\t"; out += front + ref + behind; out += '\t';
    for (size_t a = 0; a < alt.size(); a++) {
        if (a) out += ',';
        out += front; if (key[alt[a]]) out += dg_allele_str(key[alt[a]]); out += behind;
    }
    const unsigned depth = (unsigned)n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
    out += "\t.\t.\tDP="; out += std::to_string(depth); out += ";AD="; out += std::to_string(ref_at < n_al ? count[ref_at] : 0u);
    for (uint64_t i : alt) { out += ','; out += std::to_string(count[i]); }
    for (int j = 0; j < 2 && hap; j++) {
        out += j ? ";AD2=" : ";AD1="; out += std::to_string(ref_at < n_al ? (unsigned)hap[3 * ref_at + j] : 0u);
        for (uint64_t i : alt) { out += ','; out += std::to_string((unsigned)hap[3 * i + j]); }
    }
    out += '\n';
}

// The lines of pipeline target g.  lines / vcf: where they go, or NULL; tb: the target's bases, or NULL (no REF, no VCF)
inline void dg_site_allele_lines(std::string *lines, std::string *vcf, const std::string &rname, const dagcon_pileup_sites &ps, const dagcon_site_alleles &sa,
                                 uint32_t g, const char *tb, uint32_t tlen, uint32_t min_count) {
    for (uint64_t s = ps.site_begin[g]; s < ps.site_begin[g + 1]; s++) {
        const uint64_t a0 = sa.al_begin[s], a1 = sa.al_begin[s + 1];
        const uint16_t *n = ps.counts + 8 * s;
        if (lines)
            for (uint64_t i = a0; i < a1; i++)
                dg_site_allele_line(*lines, rname, ps.pos[s], tb ? tb[ps.pos[s]] : 0, n, sa.key[i], sa.count[i], sa.hap_count ? sa.hap_count + 3 * i : nullptr);
        if (vcf && tb)
            dg_site_vcf_record(*vcf, rname, tb, tlen, ps.pos[s], n, sa.key + a0, sa.count + a0, sa.hap_count ? sa.hap_count + 3 * a0 : nullptr, a1 - a0, min_count);
    }
}
