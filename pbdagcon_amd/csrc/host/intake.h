// intake.h -- where the command-line hosts hand alignment records to the library: the one record every format becomes (DgAlnRec),
// one description per kind of input (dg_kind: what the messages say; dg_blob_bytes, dg_blob, dg_rec_ops: what of a record goes to the
// device), a batch's arrays, the call that picks the entry point, the warning texts, and the one place a context is made and
// given --max-error / --max-depth (DgPick).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/dagcon.h"
#include "sam.h"

enum DgRecordKind {
    DG_REC_PLAIN,       // --sam: one base a byte                          dagcon_consensus_cigar / _cigar_windows
    DG_REC_PACKED,      // --bam: two bases a byte                         dagcon_consensus_cigar_packed
    DG_REC_STRANDED,    // --paf: one base a byte, a flag per record       dagcon_consensus_cigar_strand
    DG_REC_CS,          // --paf --cs: no bases, cs:Z: text per record     dagcon_consensus_cs
    DG_REC_PLAIN_MD,    // --sam --md: one base a byte, MD:Z: text per record, no --ref       dagcon_consensus_cigar_md
    DG_REC_PACKED_MD    // --bam --md: two bases a byte, MD:Z: text per record, no --ref      dagcon_consensus_cigar_md (packed)
};
constexpr bool dg_kind_md(DgRecordKind k) { return k == DG_REC_PLAIN_MD || k == DG_REC_PACKED_MD; }
constexpr bool dg_kind_sam(DgRecordKind k) { return k == DG_REC_PLAIN || k == DG_REC_PLAIN_MD; }       // SAM text
constexpr bool dg_kind_bam(DgRecordKind k) { return k == DG_REC_PACKED || k == DG_REC_PACKED_MD; }     // BAM records, packed bases

// what the messages of a kind say
struct DgKindDesc {
    const char *flag, *entry;                              // the command line's flags and the library's entry point (timing lines)
    const char *unit;                                      // what DgAlnRec::where counts: what an error names
    const char *format;                                    // the file format a user is told to sort
    const char *skipped_what;                              // behind the number of records left out
    const char *nonconforming;                             // why DAGCON_ERR_NONCONFORMING came back for a target or a window
};
#define DG_CIGAR_UNFIT "a record's CIGAR does not fit its SEQ or its target, or holds N or a length of 0"
#define DG_MD_UNFIT "a record's CIGAR does not fit its SEQ or its target, its MD:Z: text breaks the grammar or does not cover the target bases of its CIGAR, or the MD:Z: texts of the target disagree"
inline const DgKindDesc &dg_kind(DgRecordKind k) {
    static const DgKindDesc d[6] = {
        {"--sam", "dagcon_consensus_cigar", "line", "SAM", "SAM records skipped (FLAG 0x4 or 0x100, or RNAME, CIGAR or SEQ '*')", DG_CIGAR_UNFIT},
        {"--bam", "dagcon_consensus_cigar_packed", "record", "BAM", "BAM records skipped (FLAG 0x4 or 0x100, refID < 0, no CIGAR or no SEQ)", DG_CIGAR_UNFIT},
        {"--paf", "dagcon_consensus_cigar_strand", "line", "SAM", "PAF lines skipped (tp:A:S)", DG_CIGAR_UNFIT},
        {"--paf --cs", "dagcon_consensus_cs", "line", "SAM", "PAF lines skipped (tp:A:S)",
         "a line's cs:Z: text breaks the grammar or does not fit its qe - qs, its te - ts or its target"},
        {"--sam --md", "dagcon_consensus_cigar_md", "line", "SAM", "SAM records skipped (FLAG 0x4 or 0x100, or RNAME, CIGAR or SEQ '*')", DG_MD_UNFIT},
        {"--bam --md", "dagcon_consensus_cigar_md", "record", "BAM", "BAM records skipped (FLAG 0x4 or 0x100, refID < 0, no CIGAR or no SEQ)", DG_MD_UNFIT}};
    return d[k];
}

// One alignment record, whatever it was read from (dg_sam_rec below, dg_bam_rec in bam.h, dg_paf_rec in paf.h).  Nothing
// is copied: every pointer points into the input, the --ref bases or the reads.
struct DgAlnRec {
    const char *rname; uint32_t rname_len;                 // the target's name
    const DgRefSeqs::Span *target;                         // its bases in --ref; NULL: --ref has no such sequence (the caller words the error)
    const char *qname; uint32_t qname_len;                 // the read's name (--dump-parsed)
    uint32_t pos;                                          // 1-based, SAM POS
    const char *q; uint32_t q_len;                         // the read bases, one a byte (packed: two a byte; cs: none); q_len counts bases
    const char *cigar; uint32_t cigar_len;                 // plain, stranded: the CIGAR text
    const uint8_t *bam_ops;                                // packed: the ops as they lie in the record (not aligned)
    uint32_t nops;                                         // ops of cigar / bam_ops (cs: 0)
    const char *cs; uint32_t cs_len, t_span;               // cs: the text behind cs:Z: and the target bases the line claims (te - ts)
    const char *md; uint32_t md_len;                       // md kinds: the text behind MD:Z:
    bool reverse;                                          // the record's strand is '-' (stranded: the ops are written against the reverse
                                                           // complement of q, dagcon_upload_cigar_strand; every other kind: for printing)
    const char *read; uint32_t read_len, qs;               // stranded: the whole read and where q begins in it (--dump-parsed)
    unsigned long long where;                              // the line or the record's ordinal (dg_kind().unit): what an error names
};

// bytes of a record in a batch's q blob, and where they come from
inline size_t dg_blob_bytes(DgRecordKind k, const DgAlnRec &r) { return k == DG_REC_CS ? r.cs_len : dg_kind_bam(k) ? ((size_t)r.q_len + 1) / 2 : r.q_len; }
inline const char *dg_blob(DgRecordKind k, const DgAlnRec &r) { return k == DG_REC_CS ? r.cs : r.q; }
// the record's nops BAM-encoded ops to dst
inline void dg_rec_ops(DgRecordKind k, const DgAlnRec &r, uint32_t *dst) {
    if (dg_kind_bam(k)) memcpy(dst, r.bam_ops, (size_t)r.nops * 4);
    else if (k != DG_REC_CS) dg_cigar_ops(r.cigar, r.cigar_len, dst);
}

// a split SAM line (DG_SAM_RECORD) as a record; pos: POS as the caller reads it; want_md: the md kinds look for the tag
inline void dg_sam_rec(const DgSamLine &l, uint32_t pos, unsigned long long lineno, const DgRefSeqs &ref, DgAlnRec &r, bool want_md = false) {
    r = DgAlnRec{};
    r.rname = l.f[2]; r.rname_len = (uint32_t)l.fl[2]; r.target = ref.find(l.f[2], l.fl[2]);
    r.qname = l.f[0]; r.qname_len = (uint32_t)l.fl[0];
    r.pos = pos;                                           // 1-based, as Alignment::start
    r.q = l.f[9]; r.q_len = (uint32_t)l.fl[9];             // (SEQ is in the target's orientation either way)
    r.cigar = l.f[5]; r.cigar_len = (uint32_t)l.fl[5]; r.nops = (uint32_t)l.nops;
    r.reverse = (l.flag & DG_SAM_REVERSE) != 0;
    r.where = lineno;
    if (want_md && !dg_sam_md(l, r.md, r.md_len)) r.md = nullptr;     // (a record without the tag is skipped by the caller)
}

// the arrays of a batch: a dagcon_cigar_batch (DG_REC_CS: q_off / q_blob / q_bytes are the cs texts, op_begin / ops unused)
// and what the stranded and the cs kinds add to it
struct DgRecordArrays {
    dagcon_cigar_batch cb;
    const uint8_t *reverse;                                        // DG_REC_STRANDED
    const uint32_t *cs_len, *t_span;                               // DG_REC_CS
    dagcon_md_tags md;                                             // the md kinds (cb.t_blob is then not read)
};

// windows NULL: whole targets
inline int dg_consensus_records(dagcon_ctx *ctx, DgRecordKind kind, const DgRecordArrays &a, const dagcon_windows *windows, dagcon_results *r) {
    const dagcon_cigar_batch &cb = a.cb;
    if (kind == DG_REC_CS) {
        dagcon_cs_batch sb;
        memset(&sb, 0, sizeof sb);
        sb.n_targets = cb.n_targets; sb.tlen = cb.tlen; sb.t_off = cb.t_off; sb.t_blob = cb.t_blob; sb.t_bytes = cb.t_bytes;
        sb.rec_begin = cb.rec_begin; sb.pos = cb.pos; sb.q_len = cb.q_len; sb.t_span = a.t_span;
        sb.cs_off = cb.q_off; sb.cs_len = a.cs_len; sb.cs_blob = cb.q_blob; sb.cs_bytes = cb.q_bytes;
        return dagcon_consensus_cs(ctx, &sb, windows, r);
    }
    if (dg_kind_md(kind)) return dagcon_consensus_cigar_md(ctx, &cb, windows, &a.md, kind == DG_REC_PACKED_MD, r);
    return kind == DG_REC_PACKED ? dagcon_consensus_cigar_packed(ctx, &cb, windows, r)
         : kind == DG_REC_STRANDED ? dagcon_consensus_cigar_strand(ctx, &cb, windows, a.reverse, r)
         : windows ? dagcon_consensus_cigar_windows(ctx, &cb, windows, r) : dagcon_consensus_cigar(ctx, &cb, r);
}

// why a target or a window was skipped: its status as a warning's text
inline const char *dg_status_text(int status, const char *nonconforming) {
    return status == DAGCON_ERR_NONCONFORMING ? nonconforming : status == DAGCON_ERR_UNSUPPORTED ? "too large" : "internal error";
}

// --max-error F / --max-depth N: the records are picked on the device (dagcon_set_record_filter; include/dagcon.h has the rule)
struct DgPick {
    uint32_t max_error_ppm = 1000000u, max_depth = 0;
    bool error_set = false, depth_set = false;
    bool on() const { return error_set || depth_set; }
    // the flags as a timing line names them
    std::string text() const {
        char buf[96] = "";
        int k = 0;
        if (error_set) k += snprintf(buf + k, sizeof buf - k, " --max-error %u.%06u", max_error_ppm / 1000000u, max_error_ppm % 1000000u);
        if (depth_set) snprintf(buf + k, sizeof buf - k, " --max-depth %u", max_depth);
        return buf;
    }
};
// --max-error's text as parts per million, without floating point: 0 or 1, then optionally a point and one to six digits;
// at most 1.  "0.15" is exactly 150000
inline bool dg_parse_ppm(const char *s, uint32_t *ppm) {
    if (s[0] != '0' && s[0] != '1') return false;
    uint32_t v = (uint32_t)(s[0] - '0') * 1000000u;
    const char *p = s + 1;
    if (*p == '.') {
        uint32_t scale = 100000u, digits = 0;
        for (p++; *p >= '0' && *p <= '9' && digits < 6; p++, digits++, scale /= 10u) v += (uint32_t)(*p - '0') * scale;
        if (!digits) return false;
    }
    if (*p || v > 1000000u) return false;
    *ppm = v;
    return true;
}
// what the pick did to the records of the last call on ctx, one DAGCON_FATE_* byte per record; NULL: no filter is set
inline const uint8_t *dg_record_fates(dagcon_ctx *ctx, uint64_t *n) {
    dagcon_record_stats st;
    if (dagcon_fetch_record_stats(ctx, &st) != DAGCON_OK) return nullptr;
    *n = st.n;
    return st.fate;
}
// --md: the records left out for want of the tag, one line
inline void dg_report_no_md(DgRecordKind k, unsigned long long n) {
    if (n) fprintf(stderr, "pbdagcon: %llu %s records without an MD:Z: tag skipped (samtools calmd or minimap2 --MD write it)\n", n, dg_kind_sam(k) ? "SAM" : "BAM");
}
inline void dg_report_pick(const DgPick &pick, unsigned long long over_error, unsigned long long over_depth) {
    if (pick.on()) fprintf(stderr, "pbdagcon: records left out: %llu by --max-error, %llu by --max-depth\n", over_error, over_depth);
}

// a context for the command line's options, with the record filter --max-error / --max-depth ask for (pick NULL: none);
// a failure is reported here (there is no CPU fallback)
inline int dg_create(unsigned min_cov, unsigned min_len, unsigned trim, int device, uint32_t flags, const DgPick *pick, dagcon_ctx **ctx) {
    dagcon_opts dopt;
    dagcon_default_opts(&dopt);
    dopt.min_cov = min_cov; dopt.min_len = min_len; dopt.trim = trim;
    dopt.min_weight = (int32_t)min_cov;                    // main.cpp:261,279 (quirk Q1)
    dopt.device = device; dopt.flags = flags;
    const int rc = dagcon_create(&dopt, ctx);
    if (rc != DAGCON_OK) { fprintf(stderr, "pbdagcon: no usable MI355X as device %d (dagcon_create = %d); there is no CPU fallback\n", device, rc); return rc; }
    if (pick && pick->on()) {
        const dagcon_record_filter f = {pick->max_error_ppm, pick->max_depth};
        const int rf = dagcon_set_record_filter(*ctx, &f);
        if (rf != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(*ctx)); dagcon_destroy(*ctx); *ctx = nullptr; return rf; }
    }
    return rc;
}
