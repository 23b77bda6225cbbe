// paf.h -- what `pbdagcon --paf --ref --reads` and `pbdagcon --paf --cs --ref` need of PAF text and of a reads file.
//
// A PAF line (minimap2 -c) does not carry the read: qname qlen qs qe strand tname tlen ts te nmatch alen mapq and then
// tags name a slice [qs, qe) of a read that lies once in another file, and for a '-' line the cg:Z: CIGAR is written
// against the reverse complement of that slice.  A record of the pipeline is then: pos = ts + 1, q_len = qe - qs, the
// read bases the slice AS THE READS FILE HAS IT (a pointer into DgPafInput::reads; whoever fills a batch copies it with
// memcpy), reverse = (strand == '-'): the device reads the slice backwards and complemented
// (dagcon_upload_cigar_strand in include/dagcon.h).  No base is touched here; dg_paf_revcomp serves --dump-parsed only.
//
// minimap2 orders PAF by query, so the reader groups: targets come in --ref order, a target's records in file order
// (that order is addAln order: it is semantics).  tp:A:S lines are skipped as secondary SAM records are; lines without
// cg:Z: are skipped and counted (aligning them is not built).  A cg that does not consume exactly te - ts target bases
// takes its target out, with a warning that names the line, as the library takes out the target of a record whose cg
// does not consume exactly qe - qs read bases (DAGCON_ERR_NONCONFORMING).  MD:Z:, QUAL and gzip are not read.
// Line ends are LF (a CR in front of it is dropped, as sam.h drops it).
//
// --cs (minimap2 --cs, with or without -c): the text behind cs:Z: and the target are the whole alignment, so there is no
// reads file and the query name is not looked up; qlen, qs and qe are checked among themselves.  A record is then
// pos = ts + 1, q_len = qe - qs, t_span = te - ts and the text, found by its tab and not looked into: the device decodes
// it (dagcon_upload_cs in include/dagcon.h) and takes out the target of a record whose text does not give exactly q_len
// read bases and t_span target bases.  The text is in the target's orientation: the strand is carried for printing only.
// Lines without cs:Z: are skipped and counted.  dg_cs_decode serves --dump-parsed only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "intake.h"
#include "sam.h"

// the complement of include/dagcon.h: A<->T, C<->G in either case, every other byte as it is
inline char dg_paf_comp(char c) {
    switch (c) {
        case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
        default: return c;
    }
}
// for printing only (--dump-parsed)
inline std::string dg_paf_revcomp(const char *s, size_t n) {
    std::string out(n, 0);
    for (size_t i = 0; i < n; i++) out[i] = dg_paf_comp(s[n - 1 - i]);
    return out;
}

// for printing only (--dump-parsed): the read and the ops of a cs text by the rule of include/dagcon.h, against the target's
// bases t[0, tlen) from pos; false when the text breaks the grammar or runs past the target
inline bool dg_cs_decode(const char *cs, size_t n, const char *t, size_t tlen, uint32_t pos, std::string &read, std::vector<uint32_t> &ops) {
    auto isop = [](char c) { return c == ':' || c == '*' || c == '+' || c == '-' || c == '=' || c == '~'; };
    auto letter = [](char c) { return (unsigned)((c & 0xDF) - 'A') < 26u; };
    auto upper = [](char c) { return (char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
    read.clear(); ops.clear();
    if (pos == 0) return false;
    size_t ti = pos - 1u;
    for (size_t i = 0; i < n;) {
        const char op = cs[i];
        if (!isop(op) || op == '~') return false;
        size_t j = i + 1;
        while (j < n && !isop(cs[j])) j++;
        const size_t len = j - i - 1;
        if (len == 0) return false;
        if (op == ':') {
            uint64_t v = 0;
            if (len > 9) return false;
            for (size_t k = i + 1; k < j; k++) { if (cs[k] < '0' || cs[k] > '9') return false; v = v * 10 + (uint64_t)(cs[k] - '0'); }
            if (v == 0 || v >= (1u << 28) || ti + v > tlen) return false;
            read.append(t + ti, (size_t)v); ti += (size_t)v;
            ops.push_back((uint32_t)v << 4 | 7u);
        } else {
            for (size_t k = i + 1; k < j; k++) if (!letter(cs[k])) return false;
            if (op == '*') {
                if (len != 2) return false;
                read += upper(cs[i + 2]); ti += 1;
                ops.push_back(1u << 4 | 8u);
            } else {
                if (op != '-') for (size_t k = i + 1; k < j; k++) read += upper(cs[k]);
                if (op != '+') ti += len;
                ops.push_back((uint32_t)len << 4 | (op == '=' ? 7u : op == '+' ? 1u : 2u));
            }
        }
        i = j;
    }
    return ti <= tlen;
}

// reads a four-line FASTQ file: the names (first word of the @ line) and the bases; QUAL is not read
inline bool dg_read_fastq(const std::string &path, DgRefSeqs &reads, std::string &err) {
    std::string text;
    if (!dg_slurp(path, text, err)) return false;
    reads.bases.reserve(text.size() / 2);
    size_t pos = 0;
    unsigned long long lineno = 0;
    const char *ln[4]; size_t ll[4];
    while (pos < text.size()) {
        int k = 0;
        for (; k < 4 && pos < text.size(); k++) {
            ln[k] = text.data() + pos;
            ll[k] = dg_line(text.data(), text.size(), pos);
            lineno++;
            if (k == 0 && ll[0] == 0) { k = -1; continue; }       // blank lines between records
        }
        if (k == 0) break;
        if (k < 4 || ll[0] < 1 || ln[0][0] != '@' || ll[2] < 1 || ln[2][0] != '+') {
            err = path + ": line " + std::to_string(lineno) + ": not a four-line FASTQ record (@name, bases, +, qualities)";
            return false;
        }
        size_t e = 1;
        while (e < ll[0] && ln[0][e] != ' ' && ln[0][e] != '\t') e++;
        const std::string name(ln[0] + 1, e - 1);
        if (ll[1] > 0xFFFFFFFFull) { err = "sequence " + name + " is too long"; return false; }
        if (!reads.by_name.emplace(name, DgRefSeqs::Span{reads.bases.size(), (uint32_t)ll[1]}).second) {
            err = "sequence " + name + " occurs twice in " + path;
            return false;
        }
        reads.bases.append(ln[1], ll[1]);
    }
    return true;
}

// the reads file: FASTA (multi-line) or four-line FASTQ, told apart by the first byte
inline bool dg_read_reads(const std::string &path, DgRefSeqs &reads, std::string &err) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { err = "error opening file: " + path; return false; }
    const int c = fgetc(f);
    fclose(f);
    if (c == EOF) return true;
    if (c == '>') return dg_read_fasta(path, reads, err);
    if (c == '@') return dg_read_fastq(path, reads, err);
    err = path + " is neither FASTA ('>') nor FASTQ ('@'); gzip is not read";
    return false;
}

struct DgPafRec {
    const char *tname; uint32_t tname_len;                 // in the PAF text
    const char *qname; uint32_t qname_len;
    uint32_t pos;                                          // ts + 1
    const char *q; uint32_t q_len;                         // the slice [qs, qe) as the reads file has it
    const char *read; uint32_t read_len, qs;               // the whole read (--dump-parsed)
    bool reverse;
    const char *cg; uint32_t cg_len, nops;                 // the text behind cg:Z: (--cs: behind cs:Z:, nops 0)
    uint32_t t_span;                                       // te - ts
    DgRefSeqs::Span tspan;                                 // the target in --ref
    unsigned long long line;
};

struct DgPafInput {
    DgRefSeqs reads;
    bool cs = false;                                       // --cs: the cs:Z: tag instead of cg:Z: and a reads file
    std::vector<DgPafRec> recs;                            // grouped: targets in --ref order, file order inside a target
    unsigned long long n_secondary = 0, n_nocg = 0;

    static bool num(const char *s, size_t n, uint64_t &v) {
        v = 0;
        if (!n) return false;
        for (size_t i = 0; i < n; i++) {
            if (s[i] < '0' || s[i] > '9') return false;
            v = v * 10 + (uint64_t)(s[i] - '0');
            if (v > 0xFFFFFFFFull) return false;
        }
        return true;
    }

    // parses the whole text; false with a message in err (it names the line).  Warnings go to stderr
    bool parse(const char *data, size_t size, const DgRefSeqs &ref, std::string &err) {
        size_t p = 0;
        unsigned long long lineno = 0;
        std::unordered_set<std::string> dropped;           // targets taken out by a cg that does not fit [ts, te)
        auto fail = [&](const std::string &what) { err = "line " + std::to_string(lineno) + ": " + what; return false; };
        while (p < size) {
            const char *line = data + p;
            const size_t ll = dg_line(data, size, p);
            lineno++;
            if (ll == 0) continue;
            const char *f[12]; size_t fl[12]; int nf = 0;
            size_t i = 0;
            bool more = false;                             // tags follow field 12
            for (; nf < 12;) {
                const char *tab = (const char *)memchr(line + i, '\t', ll - i);
                const size_t j = tab ? (size_t)(tab - line) : ll;
                f[nf] = line + i; fl[nf] = j - i; nf++;
                i = j + 1;
                if (!tab) break;
                more = nf == 12;
            }
            if (nf < 12) return fail("a PAF line has 12 fields and then tags, this one has " + std::to_string(nf) + " fields");
            const char *cg = nullptr; size_t cgl = 0;
            bool secondary = false;
            while (more && i <= ll) {
                const char *tab = (const char *)memchr(line + i, '\t', ll - i);
                const size_t j = tab ? (size_t)(tab - line) : ll;
                if (j - i >= 5 && memcmp(line + i, cs ? "cs:Z:" : "cg:Z:", 5) == 0) { cg = line + i + 5; cgl = j - i - 5; }
                if (j - i == 6 && memcmp(line + i, "tp:A:S", 6) == 0) secondary = true;
                if (!tab) break;
                i = j + 1;
            }
            if (secondary) { n_secondary++; continue; }
            if (!cg) { n_nocg++; continue; }
            if (fl[4] != 1 || (f[4][0] != '+' && f[4][0] != '-')) return fail("strand is '" + std::string(f[4], std::min<size_t>(fl[4], 20)) + "', not + or -");
            uint64_t qlen, qs, qe, tlen, ts, te;
            if (!num(f[1], fl[1], qlen) || !num(f[2], fl[2], qs) || !num(f[3], fl[3], qe) || !num(f[6], fl[6], tlen) ||
                !num(f[7], fl[7], ts) || !num(f[8], fl[8], te))
                return fail("a length or a coordinate is not an unsigned 32-bit number");
            if (qs >= qe || qe > qlen) return fail("query slice [" + std::to_string(qs) + ", " + std::to_string(qe) + ") is empty or runs past the query length " + std::to_string(qlen));
            if (ts > te || te > tlen) return fail("target range [" + std::to_string(ts) + ", " + std::to_string(te) + ") is reversed or runs past the target length " + std::to_string(tlen));
            const DgRefSeqs::Span *rd = cs ? nullptr : reads.find(f[0], fl[0]);
            if (!rd && !cs) return fail("query " + std::string(f[0], fl[0]) + " is not a sequence of --reads");
            const DgRefSeqs::Span *tg = ref.find(f[5], fl[5]);
            if (!tg) return fail("target " + std::string(f[5], fl[5]) + " is not a sequence of --ref");
            if (!cs && qlen != rd->len) return fail("query " + std::string(f[0], fl[0]) + " has length " + std::to_string(qlen) + " here but " + std::to_string(rd->len) + " bases in --reads");
            if (tlen != tg->len) return fail("target " + std::string(f[5], fl[5]) + " has length " + std::to_string(tlen) + " here but " + std::to_string(tg->len) + " bases in --ref");
            DgPafRec r;
            r.tname = f[5]; r.tname_len = (uint32_t)fl[5];
            r.qname = f[0]; r.qname_len = (uint32_t)fl[0];
            r.pos = (uint32_t)ts + 1u;
            r.read = nullptr; r.read_len = 0; r.qs = (uint32_t)qs;
            r.q = nullptr; r.q_len = (uint32_t)(qe - qs);
            r.reverse = f[4][0] == '-';
            r.cg = cg; r.cg_len = (uint32_t)cgl; r.nops = 0;
            r.t_span = (uint32_t)(te - ts);
            r.tspan = *tg;
            r.line = lineno;
            if (cs) {                                      // the text is not looked into: the device decodes and judges it
                if (cgl > 0xFFFFFFFFull) return fail("the cs:Z: tag is too long");
                recs.push_back(r);
                continue;
            }
            // the CIGAR through sam.h's parser; the target bases it consumes against te - ts
            std::vector<uint32_t> ops;
            const long k = dg_cigar_ops(cg, cgl, nullptr);
            if (k < 0) return fail("malformed cg:Z: " + std::string(cg, std::min<size_t>(cgl, 60)));
            ops.resize((size_t)k);
            dg_cigar_ops(cg, cgl, ops.data());
            uint64_t nt = 0;
            for (uint32_t op : ops) if ((1u << (op & 15u)) & 0x185u) nt += op >> 4;    // M D = X
            const std::string tname(f[5], fl[5]);
            if (nt != te - ts) {
                fprintf(stderr, "pbdagcon: warning: target %s skipped (line %llu: cg:Z: consumes %llu target bases, te - ts is %llu)\n",
                        tname.c_str(), lineno, (unsigned long long)nt, (unsigned long long)(te - ts));
                dropped.insert(tname);
                continue;
            }
            r.read = reads.bases.data() + rd->off; r.read_len = rd->len;
            r.q = r.read + qs; r.nops = (uint32_t)k;
            recs.push_back(r);
        }
        if (!dropped.empty())
            recs.erase(std::remove_if(recs.begin(), recs.end(), [&](const DgPafRec &r) { return dropped.count(std::string(r.tname, r.tname_len)) != 0; }), recs.end());
        // --ref order: a sequence's offset into the FASTA's bases ascends with its place in the file (the name breaks the
        // tie of empty sequences); stable, so a target's records stay in file order
        std::stable_sort(recs.begin(), recs.end(), [](const DgPafRec &a, const DgPafRec &b) {
            if (a.tspan.off != b.tspan.off) return a.tspan.off < b.tspan.off;
            const int c = memcmp(a.tname, b.tname, std::min(a.tname_len, b.tname_len));
            return c ? c < 0 : a.tname_len < b.tname_len;
        });
        if (n_nocg && cs) fprintf(stderr, "pbdagcon: %llu PAF lines without a cs:Z: tag skipped (run minimap2 with --cs)\n", n_nocg);
        else if (n_nocg) fprintf(stderr, "pbdagcon: %llu PAF lines without a cg:Z: tag skipped (run minimap2 with -c)\n", n_nocg);
        return true;
    }
};

// a parsed line as the pipeline's record, the one place a DgPafRec becomes one.  cg:Z: lines: the read's slice as the
// reads file has it, the strand and the CIGAR text; cs:Z: lines: the text, q_len the read bases it claims, no bases, no ops
inline void dg_paf_rec(const DgPafRec &p, bool cs, DgAlnRec &r) {
    r = DgAlnRec{};
    r.rname = p.tname; r.rname_len = p.tname_len; r.target = &p.tspan;
    r.qname = p.qname; r.qname_len = p.qname_len;
    r.pos = p.pos; r.q_len = p.q_len;
    r.reverse = p.reverse;
    r.where = p.line;
    if (cs) { r.cs = p.cg; r.cs_len = p.cg_len; r.t_span = p.t_span; return; }
    r.q = p.q; r.read = p.read; r.read_len = p.read_len; r.qs = p.qs;
    r.cigar = p.cg; r.cigar_len = p.cg_len; r.nops = p.nops;
}

// the grouped records as windows.h's driver takes them
template <DgRecordKind K>
struct DgPafSourceOf {
    static constexpr DgRecordKind kind = K;
    const DgPafInput &in;
    size_t at = 0;
    unsigned long long skipped;
    DgPafSourceOf(const DgPafInput &i) : in(i), skipped(i.n_secondary) {}
    int next(DgAlnRec &r) {
        if (at >= in.recs.size()) return 0;
        dg_paf_rec(in.recs[at++], K == DG_REC_CS, r);
        return 1;
    }
};
using DgPafSource = DgPafSourceOf<DG_REC_STRANDED>;
using DgPafCsSource = DgPafSourceOf<DG_REC_CS>;
