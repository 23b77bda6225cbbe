// sam.h -- what `pbdagcon --sam --ref` needs of SAM and FASTA text: the reference sequences by name, CIGAR text to
// BAM-encoded ops (len << 4 | op, op 0..8 = M I D N S H P = X: dagcon_cigar_batch in include/dagcon.h), the @SQ lines
// of the header against the FASTA.  Text only (BAM: bam.h; PAF: paf.h).  Line ends are LF (a CR in front of it is dropped
// with the line's last field, as the .m5 parser drops it).
// `pbdagcon --sam --md` needs no FASTA: the targets' names and lengths come from the @SQ lines (dg_sam_header_refs), every
// record's MD:Z: text (dg_sam_md: the first optional field that begins MD:Z:) goes to the device as it lies in the line,
// and the device rebuilds the target bases from CIGAR, SEQ and that text (include/dagcon.h, dagcon_md_tags; this build's
// own rule, parity unpinned).  Records without the tag are skipped and counted.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

// FLAG bits that keep a record out: unmapped, secondary
#define DG_SAM_UNMAPPED 0x4u
#define DG_SAM_SECONDARY 0x100u
#define DG_SAM_REVERSE 0x10u

struct DgRefSeqs {
    std::string bases;                                     // every sequence, line ends removed, bytes as they are
    struct Span { uint64_t off; uint32_t len; };
    std::unordered_map<std::string, Span> by_name;         // name: the header line up to its first blank
    const Span *find(const char *s, size_t n) const {
        auto it = by_name.find(std::string(s, n));
        return it == by_name.end() ? nullptr : &it->second;
    }
};

// a whole file; false with a message in err
inline bool dg_slurp(const std::string &path, std::string &text, std::string &err) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { err = "error opening file: " + path; return false; }
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    return true;
}

// the line of text that begins at pos: its length without the LF and a CR in front of it; pos moves behind the line
inline size_t dg_line(const char *data, size_t size, size_t &pos) {
    const char *line = data + pos;
    const char *nl = (const char *)memchr(line, '\n', size - pos);
    const size_t ll = nl ? (size_t)(nl - line) : size - pos;
    pos += ll + (nl ? 1 : 0);
    return ll && line[ll - 1] == '\r' ? ll - 1 : ll;
}

// reads a FASTA file; false with a message in err
inline bool dg_read_fasta(const std::string &path, DgRefSeqs &ref, std::string &err) {
    std::string text;
    if (!dg_slurp(path, text, err)) return false;
    ref.bases.reserve(text.size());
    std::string name;
    uint64_t begin = 0;
    bool open = false;
    auto close_rec = [&]() -> bool {
        if (!open) return true;
        const uint64_t len = ref.bases.size() - begin;
        if (len > 0xFFFFFFFFull) { err = "sequence " + name + " is too long"; return false; }
        if (!ref.by_name.emplace(name, DgRefSeqs::Span{begin, (uint32_t)len}).second) { err = "sequence " + name + " occurs twice in " + path; return false; }
        return true;
    };
    size_t pos = 0;
    while (pos < text.size()) {
        const char *line = text.data() + pos;
        const size_t ll = dg_line(text.data(), text.size(), pos);
        if (ll == 0) continue;
        if (line[0] == '>') {
            if (!close_rec()) return false;
            size_t e = 1;
            while (e < ll && line[e] != ' ' && line[e] != '\t') e++;
            name.assign(line + 1, e - 1);
            begin = ref.bases.size();
            open = true;
        } else {
            if (!open) { err = path + " does not begin with a '>' line"; return false; }
            ref.bases.append(line, ll);
        }
    }
    return close_rec();
}

inline int dg_cigar_code(char ch) {
    switch (ch) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
        default: return -1;
    }
}

// ops of a CIGAR field, -1 when it is not <digits><op> repeated with lengths below 2^28.  out (when given) receives them.
// A length of 0 and the op N are passed on: the library names them (DAGCON_ERR_NONCONFORMING for the record's target).
inline long dg_cigar_ops(const char *s, size_t n, uint32_t *out) {
    long k = 0;
    size_t i = 0;
    while (i < n) {
        uint64_t v = 0;
        size_t d = 0;
        for (; i < n && s[i] >= '0' && s[i] <= '9'; i++, d++) {
            v = v * 10 + (uint64_t)(s[i] - '0');
            if (v >= (1ull << 28)) return -1;
        }
        if (!d || i >= n) return -1;
        const int code = dg_cigar_code(s[i++]);
        if (code < 0) return -1;
        if (out) out[k] = ((uint32_t)v << 4) | (uint32_t)code;
        k++;
    }
    return k;
}

// One line of SAM text: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ [QUAL ...], tab-separated.  The one splitter
// of the host: fields 0..9, the rule that keeps a record out (FLAG 0x4 or 0x100, or RNAME, CIGAR or SEQ '*') and the
// number of the CIGAR's ops.  flag_of(field, length) reads FLAG the caller's way; every caller words its own errors.
struct DgSamLine {
    const char *f[10]; size_t fl[10];
    const char *rest; size_t rest_len;                     // what follows SEQ's tab: QUAL and the optional fields
    int nf;                                                // fields found, at most 10
    uint32_t flag;
    long nops;                                             // DG_SAM_RECORD only
};
enum DgSamWhat { DG_SAM_RECORD, DG_SAM_NO_RECORD /* empty, or a header line */, DG_SAM_SKIPPED, DG_SAM_FEW_FIELDS, DG_SAM_BAD_CIGAR };
template <class FlagOf>
inline DgSamWhat dg_sam_split(const char *line, size_t ll, DgSamLine &s, FlagOf flag_of) {
    s.nf = 0;
    s.rest = line + ll; s.rest_len = 0;
    if (ll == 0 || line[0] == '@') return DG_SAM_NO_RECORD;
    for (size_t i = 0; s.nf < 10;) {
        const char *tab = (const char *)memchr(line + i, '\t', ll - i);
        const size_t j = tab ? (size_t)(tab - line) : ll;
        s.f[s.nf] = line + i; s.fl[s.nf] = j - i; s.nf++;
        if (!tab) break;
        i = j + 1;
        if (s.nf == 10) { s.rest = line + i; s.rest_len = ll - i; }
    }
    if (s.nf < 10) return DG_SAM_FEW_FIELDS;
    s.flag = (uint32_t)flag_of(s.f[1], s.fl[1]);
    auto star = [&](int k) { return s.fl[k] == 1 && s.f[k][0] == '*'; };
    if ((s.flag & (DG_SAM_UNMAPPED | DG_SAM_SECONDARY)) || star(2) || star(5) || star(9)) return DG_SAM_SKIPPED;
    s.nops = dg_cigar_ops(s.f[5], s.fl[5], nullptr);
    return s.nops < 0 ? DG_SAM_BAD_CIGAR : DG_SAM_RECORD;
}

// the text behind the first optional field of a split line that begins MD:Z: (the fields behind QUAL); false: there is none
inline bool dg_sam_md(const DgSamLine &s, const char *&md, uint32_t &md_len) {
    const char *p = s.rest, *end = s.rest + s.rest_len;
    for (int field = 0; p < end; field++) {
        const char *tab = (const char *)memchr(p, '\t', (size_t)(end - p));
        const char *e = tab ? tab : end;
        if (field >= 1 && e - p >= 5 && memcmp(p, "MD:Z:", 5) == 0) { md = p + 5; md_len = (uint32_t)(e - p - 5); return true; }
        if (!tab) break;
        p = tab + 1;
    }
    return false;
}

// the CIGAR text of BAM-encoded ops (--dump-parsed)
inline std::string dg_cigar_text(const uint32_t *ops, size_t n) {
    std::string s;
    for (size_t i = 0; i < n; i++) { s += std::to_string(ops[i] >> 4); s += "MIDNSHP=X"[ops[i] & 15u]; }
    return s;
}

// the header lines at the start of the text: an @SQ whose LN disagrees with the FASTA sequence of its SN is an error
inline bool dg_sam_check_header(const char *data, size_t size, const DgRefSeqs &ref, std::string &err) {
    size_t pos = 0;
    unsigned long long lineno = 0;
    while (pos < size && data[pos] == '@') {
        const char *line = data + pos;
        const size_t ll = dg_line(data, size, pos);
        lineno++;
        if (ll < 4 || memcmp(line, "@SQ\t", 4) != 0) continue;
        const char *sn = nullptr, *ln = nullptr;
        size_t snl = 0, lnl = 0;
        size_t i = 4;
        while (i < ll) {
            const char *tab = (const char *)memchr(line + i, '\t', ll - i);
            const size_t j = tab ? (size_t)(tab - line) : ll;
            if (j - i >= 3 && line[i + 2] == ':') {
                if (line[i] == 'S' && line[i + 1] == 'N') { sn = line + i + 3; snl = j - i - 3; }
                if (line[i] == 'L' && line[i + 1] == 'N') { ln = line + i + 3; lnl = j - i - 3; }
            }
            i = j + 1;
        }
        if (!sn || !ln) continue;
        const DgRefSeqs::Span *sp = ref.find(sn, snl);
        if (!sp) continue;                                 // (a sequence no record may name: nothing to compare)
        uint64_t v = 0;
        for (size_t k = 0; k < lnl && ln[k] >= '0' && ln[k] <= '9' && v < (1ull << 40); k++) v = v * 10 + (uint64_t)(ln[k] - '0');
        if (v != sp->len) {
            err = "line " + std::to_string(lineno) + ": @SQ SN:" + std::string(sn, snl) + " has LN:" + std::string(ln, lnl) +
                  " but the --ref sequence of that name has " + std::to_string(sp->len) + " bases";
            return false;
        }
    }
    return true;
}

// --md: the targets are the header's @SQ lines, names and lengths only (ref.bases stays empty, a span's off is unused);
// false with a message in err for an @SQ without SN or LN, an LN that is no number below 2^32, or a name that occurs twice
inline bool dg_sam_header_refs(const char *data, size_t size, DgRefSeqs &ref, std::string &err) {
    size_t pos = 0;
    unsigned long long lineno = 0;
    while (pos < size && data[pos] == '@') {
        const char *line = data + pos;
        const size_t ll = dg_line(data, size, pos);
        lineno++;
        if (ll < 4 || memcmp(line, "@SQ\t", 4) != 0) continue;
        const char *sn = nullptr, *ln = nullptr;
        size_t snl = 0, lnl = 0;
        for (size_t i = 4; i < ll;) {
            const char *tab = (const char *)memchr(line + i, '\t', ll - i);
            const size_t j = tab ? (size_t)(tab - line) : ll;
            if (j - i >= 3 && line[i + 2] == ':') {
                if (line[i] == 'S' && line[i + 1] == 'N') { sn = line + i + 3; snl = j - i - 3; }
                if (line[i] == 'L' && line[i + 1] == 'N') { ln = line + i + 3; lnl = j - i - 3; }
            }
            i = j + 1;
        }
        uint64_t v = 0;
        size_t k = 0;
        for (; ln && k < lnl && ln[k] >= '0' && ln[k] <= '9' && v < (1ull << 40); k++) v = v * 10 + (uint64_t)(ln[k] - '0');
        if (!sn || !ln || !lnl || k < lnl || v > 0xFFFFFFFFull) { err = "line " + std::to_string(lineno) + ": an @SQ line needs SN and a numeric LN below 2^32"; return false; }
        if (!ref.by_name.emplace(std::string(sn, snl), DgRefSeqs::Span{0, (uint32_t)v}).second) { err = "line " + std::to_string(lineno) + ": @SQ SN:" + std::string(sn, snl) + " occurs twice"; return false; }
    }
    return true;
}
