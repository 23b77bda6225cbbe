// windows.h -- `pbdagcon --sam|--bam|--paf [--cs] --ref F --window W [--overlap O]`: targets of any length; of any depth
// with --max-depth N, which keeps at most N pieces per window (picked on the device, include/dagcon.h).  Without it a
// window holds at most DAGCON_MAX_COVERAGE (4,094) pieces that pass -m: one piece more and the run ends with the
// library's "too large" error.
//
// Window i of a target has the core [iW, min((i + 1)W, tlen)) and is run as [max(0, iW - O), min(tlen, (i + 1)W + O));
// a target of at most W bases is one window.  Windows go to the device in groups of about --batch-targets
// (dagcon_consensus_cigar_windows on a DAGCON_FLAG_BASE_POS context, with DAGCON_FLAG_BASE_SUPPORT for --fastq); a group
// gets only the records whose [s, e) meets it, which the host knows from the ops it has parsed.  Records of one RNAME
// must be consecutive and ascending in POS, as in a coordinate-sorted SAM.  The records come from a source of DgAlnRecs
// (DgSamSource, DgBamSource; DgPafSource and DgPafCsSource in paf.h; a cs record's [s, e) is the line's own [ts, te)) and go
// to the device as intake.h says for the source's kind; grouping, batching and the stitch do not know which.
// The md kinds (--sam --md, --bam --md) have no --ref: a group's targets are laid out back to back in a blob the device
// rebuilds (dagcon_consensus_cigar_md), and --edits takes its REF column from dagcon_fetch_md_targets, group by group (every
// record that covers a base of a group's windows is in the group, so a group's stretch of a target is the whole run's).
//
// The stitch (DgStitch; tests/window_twin.py: stitch is its numpy twin).  With g = pos + window begin the 1-based
// target position of a consensus base (dagcon_fetch_positions): of a window's segment the bases from the first one
// with g > core begin up to, not including, the first one from there on with g > core end are kept -- first crossings
// only, nothing assumes that g is monotone; a segment whose kept part is empty is ignored.  A segment was cut at its
// core begin when bases lie in front of the kept part, at its core end when bases lie behind it.  A kept part that was
// cut at its core begin continues the piece before it when that piece ends with the kept part just before it, comes
// from the window just before, and was cut at its core end; in every other case there is a break.  Joined pieces
// shorter than -m are dropped.  A record is >RNAME/t0_t1 with t0 = g of the first base - 1 and t1 = g of the last:
// target coordinates (in this mode only; everywhere else the name holds indexes into the consensus string, quirk Q5).
//
// The edits of a piece (--edits FILE; tests/edits_twin.py: stitch_edits is the twin).  A segment's edits (include/dagcon.h,
// dagcon_edits; t_pos + window begin) cut it into blocks in target order: a stretch of bases equal to their target bases,
// then an edit, and so on.  Of the kept part [i0, i1) of a segment:
//   - a stretch of equal bases is clipped to [i0, i1) and its target bases with it;
//   - an edit's inserted bases go where the stitch puts them: those inside [i0, i1) are kept, so a run that a cut splits
//     is split with it;
//   - an edit's target bases go with the base behind the edit (the first base behind its inserted bases): they are the
//     piece's when that base is in [i0, i1).  The part of a run in front of a cut is a plain insertion where the edit
//     begins; the edit's target bases stand in front of whatever is kept behind the cut.
// A piece that starts at a break begins at the target base of its first kept base: an edit's target bases directly in
// front of it (a leading deletion) are not the piece's, and inserted bases it begins with are an insertion at its begin.
// A kept part that continues a piece begins where that piece ended: target bases between that end and the part's first
// block are deleted by the joined piece (where the two windows agree that is the part's own leading deletion, or
// nothing), and a block that reaches back over that end -- the windows disagree -- gives the bases it holds twice as an
// insertion there.  The same clamp keeps a piece behind a break from beginning in front of the end of the piece before
// it, so the pieces of a target never overlap.  Edits that come to touch in target and piece are one edit; the trim of
// include/dagcon.h is not applied again.  The span [e0, e1) these edits refer to is written on the #piece line: it is
// the record's t0_t1 except where the first or last kept base is an inserted base (its g is that of the target base
// behind it) or a window disagrees with the one before it.  Per piece: ref[e0, e1) with the edits applied is the piece.
//
// The pile-up (--pileup FILE, --sites FILE; pileup.h) needs no stitch: the cores tile the target, so the line of target
// position p is that of position p - begin of the window whose core holds p, written group by group in window order.
//
// The read split across windows (--phase-windows with --site-reads FILE / --haplotag FILE; window_phase.h has the lines
// and the host's part of the rule, include/dagcon.h rule 9 the rule).  Every group is uploaded with the pile-up, the site
// reads with phase on and dagcon_set_window_phase; inside a group the links are the device's, between two groups the host
// links the one pair of windows from the pieces it kept of the last window, and orientation and block carry over.
//
// The phased contigs (--phase-windows with --hap-contigs FILE / --hap-windows FILE; hap_contigs.h has the stitch, the
// records and the lines).  Every group is also uploaded with dagcon_set_hap_consensus; behind the group's own results the
// derived batch of its split windows runs in the block's orientation (dagcon_upload_haps_swapped with the windows' flip)
// under dagcon_set_window_keep with the windows' cores, and its segments are joined per label from the keep records.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/dagcon.h"
#include "bam.h"
#include "fastq.h"
#include "hap_contigs.h"
#include "intake.h"
#include "pileup.h"
#include "sam.h"
#include "window_phase.h"

struct DgPieceEdit { long long t_pos, t_len, c_off, c_len; };   // target [t_pos, t_pos + t_len) -> seq[c_off, c_off + c_len)

struct DgStitchPiece {
    long long t0 = 0, t1 = 0;
    std::string seq;
    std::vector<uint16_t> weight, depth;                   // --fastq: sliced as the bases are
    long long e0 = 0, e1 = 0;                              // --edits: the target span the edits apply to
    std::vector<DgPieceEdit> edits;
};

// one segment's edits as dagcon_fetch_edits hands them out (positions relative to the window)
struct DgSegEdits {
    uint32_t t0; uint64_t n;
    const uint32_t *t_pos, *t_len; const uint64_t *c_off; const uint32_t *c_len;
    uint64_t c_base;                                       // the segment's seq_off
};

// the pieces of one target, fed window by window in order
struct DgStitch {
    std::vector<DgStitchPiece> pieces;
    long long open_w = -1;                                 // window of the last piece, if it was cut at its core end
    long long last_end = 0;                                // --edits: where the last piece's span ends
    void reset() { pieces.clear(); open_w = -1; last_end = 0; }
    // the edits of the kept part [i0, i1) of a segment, which is already the tail of the last piece (the rule above)
    void add_edits(bool cont, uint32_t begin, uint32_t i0, uint32_t i1, uint32_t n, const DgSegEdits &ed) {
        DgStitchPiece &p = pieces.back();
        const long long shift = (long long)p.seq.size() - i1;          // segment index + shift = index in p.seq
        long long at = 0;
        bool first = true;
        auto put = [&](long long tb, long long tl, long long cb, long long cl) {
            if (!tl && !cl) return;
            if (!p.edits.empty()) {
                DgPieceEdit &l = p.edits.back();
                if (l.t_pos + l.t_len == tb && l.c_off + l.c_len == cb) { l.t_len += tl; l.c_len += cl; return; }
            }
            p.edits.push_back(DgPieceEdit{tb, tl, cb, cl});
        };
        // a block clipped to the kept part: target [tb, te), segment bases [cb, ce); equal: the bases are their target's
        auto block = [&](bool equal, long long tb, long long te, long long cb, long long ce) {
            cb += shift; ce += shift;
            if (first) {
                first = false;
                if (cont) at = p.e1; else p.e0 = at = std::max(equal ? tb : te, last_end);
            }
            if (!equal) { const long long e = std::max(te, at); put(at, e - at, cb, ce - cb); at = e; return; }
            if (te <= at) { put(at, 0, cb, ce - cb); return; }
            if (tb < at) { put(at, 0, cb, at - tb); cb += at - tb; tb = at; }
            if (tb > at) put(at, tb - at, cb, 0);
            at = te;
        };
        auto equal_run = [&](long long c_lo, long long c_hi, long long t_lo) {
            const long long cb = std::max<long long>(c_lo, i0), ce = std::min<long long>(c_hi, i1);
            if (cb < ce) block(true, t_lo + (cb - c_lo), t_lo + (ce - c_lo), cb, ce);
        };
        long long c = 0, t = (long long)ed.t0 + begin;
        for (uint64_t k = 0; k < ed.n; k++) {
            const long long tp = (long long)ed.t_pos[k] + begin, tl = ed.t_len[k], co = (long long)(ed.c_off[k] - ed.c_base), cl = ed.c_len[k];
            equal_run(c, co, t);
            const long long behind = co + cl, cb = std::max<long long>(co, i0), ce = std::min<long long>(behind, i1);
            const bool takes = behind >= i0 && behind < i1;            // the edit's target bases are this part's
            if (cb < ce) block(false, tp, takes ? tp + tl : tp, cb, ce);
            else if (takes && tl) block(false, tp, tp + tl, behind, behind);
            c = behind; t = tp + tl;
        }
        equal_run(c, n, t);
        p.e1 = last_end = at;
    }
    // one segment of window wi = [begin, ..), core [c0, c1); weight / depth may be NULL; ed: NULL without --edits
    void add(long long wi, uint32_t begin, uint32_t c0, uint32_t c1, const char *seq, const uint32_t *pos, uint32_t n,
             const uint16_t *weight, const uint16_t *depth, const DgSegEdits *ed = nullptr) {
        uint32_t i0 = 0;
        while (i0 < n && (uint64_t)pos[i0] + begin <= c0) i0++;
        if (i0 == n) return;
        uint32_t i1 = i0;
        while (i1 < n && (uint64_t)pos[i1] + begin <= c1) i1++;
        if (i1 <= i0) return;
        const long long last_g = (long long)pos[i1 - 1] + begin;
        const bool cont = i0 > 0 && open_w >= 0 && open_w == wi - 1 && !pieces.empty();
        if (cont) {
            DgStitchPiece &p = pieces.back();
            p.t1 = last_g;
            p.seq.append(seq + i0, i1 - i0);
            if (weight) { p.weight.insert(p.weight.end(), weight + i0, weight + i1); p.depth.insert(p.depth.end(), depth + i0, depth + i1); }
        } else {
            pieces.emplace_back();
            DgStitchPiece &p = pieces.back();
            p.t0 = (long long)pos[i0] + begin - 1; p.t1 = last_g;
            p.seq.assign(seq + i0, i1 - i0);
            if (weight) { p.weight.assign(weight + i0, weight + i1); p.depth.assign(depth + i0, depth + i1); }
        }
        if (ed) add_edits(cont, begin, i0, i1, n, *ed);
        open_w = i1 < n ? wi : -1;
    }
};

struct DgWinOpts {
    unsigned min_cov, min_len, trim, window, overlap;
    size_t batch_targets;
    bool fastq, verbose;
    int device;
    DgPick pick;                                           // --max-error / --max-depth
    const char *edits;                                     // --edits FILE, or NULL
    FILE *pileup = nullptr, *sites = nullptr;              // --pileup / --sites: open files, or NULL (the caller closes them)
    uint32_t site_min_count = 0, site_min_ppm = 0;
    FILE *site_reads = nullptr, *haplotag = nullptr;       // --phase-windows with --site-reads / --haplotag: open files, or NULL
    DgWinPhaseOpts wp;
    FILE *hap_contigs = nullptr, *hap_windows = nullptr;   // --phase-windows with --hap-contigs / --hap-windows: open files, or NULL
    uint32_t hap_min_sites = 0, hap_min_reads = 0;         // --hap-min-sites / --hap-min-reads (0: the library's defaults)
    bool hc() const { return hap_contigs || hap_windows; }
    const dagcon_site_link_opts *link = nullptr;           // --link-sites with --phase-windows: its options, or NULL
    FILE *linked_sites = nullptr;                          // --linked-sites: an open file, or NULL
};

// SAM text: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL
template <bool MD>
struct DgSamSourceT {
    static constexpr DgRecordKind kind = MD ? DG_REC_PLAIN_MD : DG_REC_PLAIN;
    const char *data; size_t size, p = 0;
    const DgRefSeqs &ref;
    unsigned long long lineno = 0, skipped = 0, no_md = 0;
    DgSamSourceT(const char *d, size_t n, const DgRefSeqs &rf) : data(d), size(n), ref(rf) {}
    // 1: a record; 0: the end; -1: an error (printed)
    int next(DgAlnRec &r) {
        while (p < size) {
            const char *line = data + p;
            const size_t ll = dg_line(data, size, p);
            lineno++;
            DgSamLine sl;
            // the leading digits of a field; POS stops at 2^40 and is clamped to 32 bits
            auto digits = [](const char *f, size_t n, bool stop) { uint64_t v = 0; for (size_t i = 0; i < n && f[i] >= '0' && f[i] <= '9' && !(stop && v >= (1ull << 40)); i++) v = v * 10 + (uint64_t)(f[i] - '0'); return v; };
            switch (dg_sam_split(line, ll, sl, [&](const char *f, size_t n) { return digits(f, n, false); })) {
                case DG_SAM_NO_RECORD: continue;
                case DG_SAM_SKIPPED: skipped++; continue;
                case DG_SAM_FEW_FIELDS: fprintf(stderr, "pbdagcon: line %llu: a SAM record has 11 fields, this one has fewer than 10 fields\n", lineno); return -1;
                case DG_SAM_BAD_CIGAR: fprintf(stderr, "pbdagcon: line %llu: malformed CIGAR %.*s\n", lineno, (int)std::min<size_t>(sl.fl[5], 60), sl.f[5]); return -1;
                case DG_SAM_RECORD: break;
            }
            const uint64_t pos = digits(sl.f[3], sl.fl[3], true);
            dg_sam_rec(sl, pos > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pos, lineno, ref, r, MD);
            if (MD && !r.md) { no_md++; continue; }
            return 1;
        }
        return 0;
    }
};
using DgSamSource = DgSamSourceT<false>;
using DgSamMdSource = DgSamSourceT<true>;

// BAM records (bam.h); the header's references were checked against --ref when the file was opened
template <bool MD>
struct DgBamSourceT {
    static constexpr DgRecordKind kind = MD ? DG_REC_PACKED_MD : DG_REC_PACKED;
    DgBamReader &bam;
    const DgRefSeqs &ref;
    unsigned long long skipped = 0, no_md = 0;
    DgBamSourceT(DgBamReader &b, const DgRefSeqs &rf) : bam(b), ref(rf) {}
    int next(DgAlnRec &r) {
        for (;;) {
            DgBamRec br;
            std::string err;
            const int rc = bam.next(br, err);
            skipped = bam.n_skipped;
            if (rc < 0) fprintf(stderr, "pbdagcon: format error: %s\n", err.c_str());
            if (rc > 0) dg_bam_rec(bam, br, ref, r, MD);
            if (MD && rc > 0 && !r.md) { no_md++; continue; }
            return rc;
        }
    }
};
using DgBamSource = DgBamSourceT<false>;
using DgBamMdSource = DgBamSourceT<true>;

// the records a source left out for want of an MD:Z: tag (the md sources count them)
template <class Source> auto dg_source_no_md(const Source &s, int) -> decltype(s.no_md) { return s.no_md; }
template <class Source> unsigned long long dg_source_no_md(const Source &, long) { return 0; }

// the whole run; the process's exit status
template <class Source>
inline int dg_run_windows(const DgWinOpts &o, Source &src, const DgRefSeqs &ref) {
    struct Rec { uint32_t pos, s, e, q_len; const char *q; size_t q_bytes; uint64_t op0; uint32_t nops; bool reverse; uint32_t t_span; const char *md; uint32_t md_len; };   // q, q_bytes: its bytes of the q blob
    struct Tgt { std::string name; DgRefSeqs::Span sp; std::vector<Rec> recs; uint32_t max_span = 0; std::vector<uint8_t> fate; std::string rebuilt; std::vector<std::string> qnames; };   // fate: DAGCON_FATE_* per record, over all groups; rebuilt: md kinds with --edits, the target as the device made it
    constexpr bool MD = dg_kind_md(Source::kind);
    std::vector<Tgt> tgts;
    std::vector<uint32_t> ops;
    std::unordered_map<std::string, int> seen;
    // ---- the records, grouped by target ----
    const DgKindDesc &kd = dg_kind(Source::kind);
    DgAlnRec ar{};
    for (int have; (have = src.next(ar)) != 0;) {
        if (have < 0) return 1;
        ops.resize(ops.size() + ar.nops);
        dg_rec_ops(Source::kind, ar, ops.data() + ops.size() - ar.nops);
        const std::string rname(ar.rname, ar.rname_len);
        if (tgts.empty() || tgts.back().name != rname) {
            if (!ar.target) { fprintf(stderr, MD ? "pbdagcon: %s %llu: RNAME %s has no @SQ line / reference in the header\n" : "pbdagcon: %s %llu: RNAME %s is not a sequence of --ref\n", kd.unit, ar.where, rname.c_str()); return 1; }
            if (!seen.emplace(rname, 1).second) { fprintf(stderr, "pbdagcon: %s %llu: records of RNAME %s come back after another target's (records of one RNAME must be consecutive)\n", kd.unit, ar.where, rname.c_str()); return 1; }
            tgts.emplace_back();
            tgts.back().name = rname; tgts.back().sp = *ar.target;
        }
        Tgt &t = tgts.back();
        Rec r;
        r.pos = ar.pos;
        if (!t.recs.empty() && r.pos < t.recs.back().pos) { fprintf(stderr, "pbdagcon: %s %llu: POS %u of RNAME %s is below that of the record before it (--window needs records ascending in POS, as in a coordinate-sorted SAM)\n", kd.unit, ar.where, r.pos, rname.c_str()); return 1; }
        r.q = dg_blob(Source::kind, ar); r.q_len = ar.q_len; r.q_bytes = dg_blob_bytes(Source::kind, ar); r.op0 = ops.size() - ar.nops; r.nops = ar.nops;
        r.reverse = (Source::kind == DG_REC_STRANDED) && ar.reverse;
        r.t_span = ar.t_span;
        r.md = ar.md; r.md_len = ar.md_len;
        const long k = (long)ar.nops;
        // [s, e) by the rule of include/dagcon.h (a non-conforming record: clipped into the target, at least one base)
        uint64_t nt = 0;
        for (long i = 0; i < k; i++) { const uint32_t op = ops[r.op0 + i]; if ((1u << (op & 15u)) & 0x185u) nt += op >> 4; }
        if ((Source::kind == DG_REC_CS)) nt = ar.t_span;                        // (the device holds the text to it)
        const uint64_t tl = t.sp.len;
        uint64_t s0 = r.pos ? r.pos - 1u : 0u, e0 = s0 + (nt & 0xFFFFFFFFull);
        if (tl && s0 > tl - 1) s0 = tl - 1;
        if (e0 < s0 + 1) e0 = s0 + 1;
        if (e0 > tl) e0 = tl;
        r.s = (uint32_t)s0; r.e = (uint32_t)e0;
        t.max_span = std::max(t.max_span, r.e > r.s ? r.e - r.s : 0u);
        t.recs.push_back(r);
        if (o.wp.on) t.qnames.emplace_back(ar.qname, ar.qname_len);        // --phase-windows: the files name the reads
    }
    if (o.verbose && src.skipped) fprintf(stderr, "pbdagcon: %llu %s\n", src.skipped, kd.skipped_what);
    dg_report_no_md(Source::kind, dg_source_no_md(src, 0));
    // ---- the windows of every target, in target order ----
    struct Win { uint32_t tgt, idx, begin, end, c0, c1; };
    std::vector<Win> wins;
    for (uint32_t g = 0; g < tgts.size(); g++) {
        const uint64_t tl = tgts[g].sp.len;
        if (!tl) continue;
        const uint64_t nw = (tl + o.window - 1) / o.window;
        for (uint64_t i = 0; i < nw; i++) {
            const uint64_t c0 = i * o.window, c1 = std::min<uint64_t>((i + 1) * o.window, tl);
            wins.push_back(Win{g, (uint32_t)i, (uint32_t)(c0 > o.overlap ? c0 - o.overlap : 0), (uint32_t)std::min<uint64_t>(tl, (i + 1) * (uint64_t)o.window + o.overlap), (uint32_t)c0, (uint32_t)c1});
        }
    }
    dagcon_ctx *ctx = nullptr;
    int rc = dg_create(o.min_cov, o.min_len, o.trim, o.device, DAGCON_FLAG_BASE_POS | (o.fastq ? DAGCON_FLAG_BASE_SUPPORT : 0u), &o.pick, &ctx);
    if (rc != DAGCON_OK) return 1;
    FILE *ef = nullptr;
    unsigned long long n_edits = 0;
    if (o.edits) {
        if ((rc = dagcon_set_edits(ctx, 1)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); return 1; }
        if (!(ef = fopen(o.edits, "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.edits); dagcon_destroy(ctx); return 1; }
    }
    // --pileup / --sites: a position's line comes from the window whose core holds it
    const bool pile = o.pileup || o.sites, want_rebuilt = ef || pile;
    if (pile || o.wp.on) {
        const dagcon_pileup_opts po = {o.site_min_count, o.site_min_ppm};
        if ((rc = dagcon_set_pileup(ctx, &po)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); if (ef) fclose(ef); dagcon_destroy(ctx); return 1; }
    }
    if (o.wp.on) {
        const dagcon_site_reads_opts so = {1u, 0u};
        const dagcon_window_phase_opts wo = {o.wp.min_links, o.wp.max_conflict_ppm};
        if ((rc = dagcon_set_site_reads(ctx, &so)) != DAGCON_OK || (rc = dagcon_set_window_phase(ctx, &wo)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); if (ef) fclose(ef); dagcon_destroy(ctx); return 1; }
    }
    if (o.link && (rc = dagcon_set_site_link(ctx, o.link)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); if (ef) fclose(ef); dagcon_destroy(ctx); return 1; }
    if (o.hc()) {
        const dagcon_hap_opts ho = {o.hap_min_sites, o.hap_min_reads};
        if ((rc = dagcon_set_hap_consensus(ctx, &ho)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); if (ef) fclose(ef); dagcon_destroy(ctx); return 1; }
    }
    // --hap-contigs: the two labels' pieces of the current target of the derived batches (its state carries across the groups)
    DgHapStitch hst[2];
    long long hc_tgt = -1;
    std::string contigs_out, hapwin_out;
    unsigned long long n_derived = 0;
    auto flush_contigs = [&]() {
        if (hc_tgt >= 0 && o.hap_contigs) dg_hap_contig_records(contigs_out, tgts[(size_t)hc_tgt].name, hst, o.min_len, [&](uint64_t block) { return (uint64_t)wins[block].c0 + 1u; });
        hst[0].reset(); hst[1].reset();
    };
    // --phase-windows: per record of the current target its pieces' votes and its signed entries inside the cores; the
    // last window of the group before (its target, its link, its taken pieces) for the link across the groups
    struct RecAcc { bool taken = false; uint64_t sites = 0; std::vector<DgWpVote> pieces; };
    std::vector<RecAcc> acc;
    long long prev_tgt = -1;
    DgWpLink prev_link{0, 0};
    std::vector<DgWpPiece> prev_pieces;
    unsigned long long n_blocks = 0;
    std::string pile_out, site_out, reads_out, tags_out, linked_out;
    for (Tgt &t : tgts) t.fate.assign(t.recs.size(), 0);
    int status = 0;
    DgStitch st;
    std::string out;
    long long cur_tgt = -1;
    auto flush_target = [&]() {
        if (cur_tgt < 0) return true;
        for (const DgStitchPiece &p : st.pieces)
            if (p.seq.size() >= o.min_len && !dg_append_result(out, o.fastq, tgts[(size_t)cur_tgt].name, p.t0, p.t1, p.seq.data(), (uint32_t)p.seq.size(), p.weight.data(), p.depth.data())) return false;
        fwrite(out.data(), 1, out.size(), stdout);
        out.clear();
        if (ef) {
            // a #piece line with the span its edits apply to, then the edits: REF from --ref, ALT from the piece
            Tgt &t = tgts[(size_t)cur_tgt];
            const char *tb = MD ? t.rebuilt.data() : ref.bases.data() + t.sp.off;
            for (const DgStitchPiece &p : st.pieces) {
                if (p.seq.size() < o.min_len) continue;
                out += "#piece " + t.name + " " + std::to_string(p.e0) + " " + std::to_string(p.e1) + "\n";
                for (const DgPieceEdit &e : p.edits) {
                    out += t.name + "\t" + std::to_string(e.t_pos) + "\t" + std::to_string(e.t_pos + e.t_len) + "\t";
                    if (e.t_len) out.append(tb + e.t_pos, (size_t)e.t_len); else out += '-';
                    out += '\t';
                    if (e.c_len) out.append(p.seq.data() + e.c_off, (size_t)e.c_len); else out += '-';
                    out += '\n';
                }
                n_edits += p.edits.size();
            }
            fwrite(out.data(), 1, out.size(), ef);
            out.clear();
        }
        if (o.wp.on) {
            // --haplotag: the records of the target that have a taken piece, in record order
            const Tgt &t = tgts[(size_t)cur_tgt];
            for (size_t i = 0; i < acc.size() && o.haplotag; i++) {
                if (!acc[i].taken) continue;
                unsigned hap = 0;
                uint64_t block = 0;
                const bool labelled = dg_wp_vote(acc[i].pieces, hap, block);
                dg_wp_haplotag_line(tags_out, t.name, t.qnames[i], hap, acc[i].sites, labelled, labelled ? (uint64_t)wins[block].c0 + 1u : 0u);
            }
            acc.clear();
        }
        std::string().swap(tgts[(size_t)cur_tgt].rebuilt);
        st.reset();
        return true;
    };
    // ---- groups of windows ----
    for (size_t w0 = 0; w0 < wins.size() && status == 0;) {
        const size_t w1 = std::min(wins.size(), w0 + std::max<size_t>(1, o.batch_targets));
        // the batch: the targets the group touches, each with the records that meet the group's stretch of it
        std::vector<uint32_t> b_tlen, b_pos, b_qlen, b_ops, w_t, w_b, w_e;
        std::vector<uint64_t> b_toff, b_rec{0}, b_qoff, b_opb{0};
        std::string qblob;
        std::vector<uint8_t> b_rev;                            // stranded sources: one flag per record
        std::vector<uint32_t> b_cslen, b_tspan;                // cs sources: qblob holds the texts
        std::vector<uint8_t *> b_fate;                         // where each record's fate is kept (a record goes out with every group it meets)
        std::vector<uint32_t> b_idx;                           // --phase-windows: each record's index among its target's
        std::vector<uint64_t> b_mdoff;                         // md sources: the texts, back to back in mdblob
        std::vector<uint32_t> b_mdlen;
        std::string mdblob;
        uint64_t t_bytes = 0;                                  // md sources: the group's targets back to back
        struct Stretch { Tgt *t; uint64_t off; uint32_t lo, hi; };
        std::vector<Stretch> stretches;                        // md sources with --edits: what of each target the group rebuilds
        for (size_t a = w0; a < w1;) {
            size_t z = a;
            while (z < w1 && wins[z].tgt == wins[a].tgt) z++;
            Tgt &t = tgts[wins[a].tgt];
            const uint32_t lo = wins[a].begin, hi = wins[z - 1].end;
            const uint32_t bt = (uint32_t)b_tlen.size();
            b_tlen.push_back(t.sp.len); b_toff.push_back(MD ? t_bytes : t.sp.off);
            if (MD) { if (want_rebuilt) stretches.push_back(Stretch{&t, t_bytes, lo, hi}); t_bytes += t.sp.len; }
            // records are ascending in s: none that starts more than the longest span in front of lo reaches it
            const uint32_t from = lo > t.max_span ? lo - t.max_span : 0u;
            auto it = std::lower_bound(t.recs.begin(), t.recs.end(), from, [](const Rec &r, uint32_t v) { return r.s < v; });
            for (; it != t.recs.end() && it->s < hi; ++it) {
                if (it->e <= lo) continue;
                b_fate.push_back(&t.fate[(size_t)(it - t.recs.begin())]);
                if (o.wp.on) b_idx.push_back((uint32_t)(it - t.recs.begin()));
                b_pos.push_back(it->pos); b_qoff.push_back(qblob.size()); b_qlen.push_back(it->q_len);
                qblob.append(it->q, it->q_bytes);
                if ((Source::kind == DG_REC_CS)) { b_cslen.push_back((uint32_t)it->q_bytes); b_tspan.push_back(it->t_span); }
                b_ops.insert(b_ops.end(), ops.begin() + (long)it->op0, ops.begin() + (long)(it->op0 + it->nops));
                b_opb.push_back(b_ops.size());
                if ((Source::kind == DG_REC_STRANDED)) b_rev.push_back(it->reverse ? 1 : 0);
                if (MD) { b_mdoff.push_back(mdblob.size()); b_mdlen.push_back(it->md_len); mdblob.append(it->md, it->md_len); }
            }
            b_rec.push_back(b_pos.size());
            for (size_t k = a; k < z; k++) { w_t.push_back(bt); w_b.push_back(wins[k].begin); w_e.push_back(wins[k].end); }
            a = z;
        }
        DgRecordArrays ra{};
        ra.cb.n_targets = (uint32_t)b_tlen.size(); ra.cb.tlen = b_tlen.data(); ra.cb.t_off = b_toff.data();
        ra.cb.t_blob = MD ? nullptr : ref.bases.data(); ra.cb.t_bytes = MD ? t_bytes : ref.bases.size();
        ra.md.md_off = b_mdoff.data(); ra.md.md_len = b_mdlen.data(); ra.md.md_blob = mdblob.data(); ra.md.md_bytes = mdblob.size();
        ra.cb.rec_begin = b_rec.data(); ra.cb.pos = b_pos.data(); ra.cb.q_off = b_qoff.data(); ra.cb.q_len = b_qlen.data();
        ra.cb.q_blob = qblob.data(); ra.cb.q_bytes = qblob.size(); ra.cb.op_begin = b_opb.data(); ra.cb.ops = b_ops.data();
        ra.reverse = b_rev.data(); ra.cs_len = b_cslen.data(); ra.t_span = b_tspan.data();
        dagcon_windows dw;
        dw.n_windows = (uint32_t)w_t.size(); dw.target = w_t.data(); dw.begin = w_b.data(); dw.end = w_e.data();
        dagcon_results r;
        rc = dg_consensus_records(ctx, Source::kind, ra, &dw, &r);
        const uint32_t *pos = nullptr;
        uint64_t npos = 0;
        dagcon_support sup;
        memset(&sup, 0, sizeof sup);
        if (rc == DAGCON_OK) rc = dagcon_fetch_positions(ctx, &pos, &npos);
        if (rc == DAGCON_OK && o.fastq) rc = dagcon_fetch_support(ctx, &sup);
        dagcon_edits ed;
        memset(&ed, 0, sizeof ed);
        if (rc == DAGCON_OK && ef) rc = dagcon_fetch_edits(ctx, &ed);
        dagcon_pileup pu;
        memset(&pu, 0, sizeof pu);
        if (rc == DAGCON_OK && o.pileup) rc = dagcon_fetch_pileup(ctx, &pu);
        dagcon_pileup_sites ps;
        memset(&ps, 0, sizeof ps);
        if (rc == DAGCON_OK && (o.sites || o.wp.on)) rc = dagcon_fetch_pileup_sites(ctx, &ps);
        dagcon_site_reads sr;
        memset(&sr, 0, sizeof sr);
        dagcon_window_phase wp;
        memset(&wp, 0, sizeof wp);
        if (rc == DAGCON_OK && o.wp.on) rc = dagcon_fetch_site_reads(ctx, &sr);
        if (rc == DAGCON_OK && o.wp.on) rc = dagcon_fetch_window_phase(ctx, &wp);
        dagcon_site_link sl;
        memset(&sl, 0, sizeof sl);
        if (rc == DAGCON_OK && o.link) rc = dagcon_fetch_site_link(ctx, &sl);
        uint64_t sr_x = 0;                                     // the taken alignments ascend in their window: one walk
        std::vector<DgWpLink> links(o.hc() ? w1 - w0 : 0, DgWpLink{0, 0});    // --hap-contigs / --hap-windows: every window's link in the run's terms
        DgWpLink first_link{0, 0};                             // the link of the group's first window, in the run's terms
        if (rc == DAGCON_OK && want_rebuilt && MD) {           // REF of the edits and of the pile-up lines: the group's stretch of every target, as the device rebuilt it
            const char *tb = nullptr;
            uint64_t tn = 0;
            rc = dagcon_fetch_md_targets(ctx, &tb, &tn);
            for (size_t k = 0; rc == DAGCON_OK && k < stretches.size(); k++) {
                const Stretch &x = stretches[k];
                if (x.t->rebuilt.empty()) x.t->rebuilt.assign(x.t->sp.len, 'N');
                memcpy(&x.t->rebuilt[x.lo], tb + x.off + x.lo, x.hi - x.lo);
            }
        }
        if (rc != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); status = 1; break; }
        uint64_t n_fate = 0;
        if (const uint8_t *fate = dg_record_fates(ctx, &n_fate))
            for (uint64_t i = 0; i < n_fate && i < b_fate.size(); i++) *b_fate[i] |= fate[i];
        for (size_t k = w0; k < w1; k++) {
            const Win &w = wins[k];
            if ((long long)w.tgt != cur_tgt) {
                if (!flush_target()) { status = 1; break; }
                cur_tgt = w.tgt;
                if (o.wp.on) acc.assign(tgts[w.tgt].recs.size(), RecAcc());
            }
            const size_t g = k - w0;
            if (o.wp.on) {
                const Tgt &t = tgts[w.tgt];
                const uint64_t x0 = sr_x;
                while (sr_x < sr.n_aln && sr.aln_tgt[sr_x] == g) sr_x++;
                // the window's link in the run's terms: the first of a group by the host's pair rule against the last window of
                // the group before, the others from the device's arrays (its block 0 is the first window's)
                DgWpLink link;
                if (g == 0) {
                    std::vector<DgWpPiece> cur;
                    for (uint64_t x = x0; x < sr_x; x++) cur.push_back(DgWpPiece{b_idx[sr.aln_src[x]], sr.hap[x]});
                    uint32_t same = 0, diff = 0;
                    const bool has_prev = prev_tgt == (long long)w.tgt;
                    if (has_prev) dg_wp_pair(prev_pieces, cur, same, diff);
                    link = first_link = dg_wp_step(has_prev, prev_link, k, same, diff, o.wp.min_links, o.wp.max_conflict_ppm);
                } else if (wp.block[g] == 0) link = DgWpLink{(uint8_t)(wp.flip[g] ^ first_link.flip), first_link.block};
                else link = DgWpLink{wp.flip[g], (uint64_t)w0 + wp.block[g]};
                n_blocks += link.block == k;
                if (o.hc()) links[g] = link;
                const bool turn = wp.block[g] == 0 && first_link.flip != 0;     // (the device oriented block 0 as if its first window were unlinked)
                const uint32_t lo = w.c0 - w.begin, hi = w.c1 - w.begin;
                for (uint64_t x = x0; x < sr_x; x++) {
                    RecAcc &a = acc[b_idx[sr.aln_src[x]]];
                    const uint8_t h = wp.hap[x];
                    a.taken = true;
                    a.pieces.push_back(DgWpVote{link.block, (uint8_t)(h && turn ? 3u - h : h)});
                    for (uint64_t e = sr.ent_begin[x]; e < sr.ent_begin[x + 1]; e++) {
                        const uint32_t p = ps.pos[sr.ent_site[e]];
                        a.sites += p >= lo && p < hi && dg_sr_sign(sr.ent_code[e], ps.counts + 8 * sr.ent_site[e], o.link ? sl.linked[sr.ent_site[e]] : 1u) != 0;
                    }
                }
                if (o.linked_sites) dg_linked_site_lines(linked_out, t.name, ps, sl, (uint32_t)g, lo, hi, w.begin);
                if (o.site_reads) dg_wp_site_read_lines(reads_out, t.name, ps, sr, (uint32_t)g, x0, sr_x, lo, hi, w.begin, [&](uint64_t x) -> const std::string & { return t.qnames[b_idx[sr.aln_src[x]]]; });
                if (k + 1 == w1) {
                    prev_tgt = w.tgt; prev_link = link;
                    prev_pieces.clear();
                    for (uint64_t x = x0; x < sr_x; x++) prev_pieces.push_back(DgWpPiece{b_idx[sr.aln_src[x]], sr.hap[x]});
                }
            }
            if (pile) {
                const Tgt &t = tgts[w.tgt];
                const char *tb = MD ? t.rebuilt.data() : ref.bases.data() + t.sp.off;
                if (o.pileup) dg_pileup_lines(pile_out, t.name, pu, (uint32_t)g, w.c0 - w.begin, w.c1 - w.begin, w.begin, tb);
                if (o.sites) dg_site_lines(site_out, t.name, ps, (uint32_t)g, w.c0 - w.begin, w.c1 - w.begin, w.begin, tb);
            }
            if (r.target_status[g] != DAGCON_OK)
                fprintf(stderr, "pbdagcon: warning: %s window [%u, %u) skipped (%s)\n", tgts[w.tgt].name.c_str(), w.begin, w.end,
                        dg_status_text(r.target_status[g], MD ? kd.nonconforming : DG_CIGAR_UNFIT));
            if (o.verbose) fprintf(stderr, "pbdagcon: %s window %u [%u, %u): %llu segments\n", tgts[w.tgt].name.c_str(), w.idx, w.begin, w.end,
                                   (unsigned long long)(r.seg_begin[g + 1] - r.seg_begin[g]));
            for (uint64_t s = r.seg_begin[g]; s < r.seg_begin[g + 1]; s++) {
                const uint64_t off = r.seq_off[s];
                DgSegEdits se{};
                if (ef) {
                    const uint64_t e0 = ed.edit_begin[s];
                    se = DgSegEdits{ed.seg_t0[s], ed.edit_begin[s + 1] - e0, ed.t_pos + e0, ed.t_len + e0, ed.c_off + e0, ed.c_len + e0, off};
                }
                st.add(w.idx, w.begin, w.c0, w.c1, r.seq_blob + off, pos + off, r.seq_len[s],
                       o.fastq ? sup.weight + off : nullptr, o.fastq ? sup.depth + off : nullptr, ef ? &se : nullptr);
            }
        }
        // ---- the derived batch of the group's split windows, in the block's orientation (last: it takes the place of
        // everything the fetches above point at) ----
        if (o.hc() && status == 0) {
            const uint32_t nw = (uint32_t)(w1 - w0);
            dagcon_hap_tally ht;
            memset(&ht, 0, sizeof ht);
            if ((rc = dagcon_fetch_hap_tally(ctx, &ht)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); status = 1; break; }
            std::vector<uint32_t> k_lo(nw), k_hi(nw);
            std::vector<uint8_t> swap(nw);
            for (uint32_t g = 0; g < nw; g++) {
                const Win &w = wins[w0 + g];
                k_lo[g] = w.c0 - w.begin; k_hi[g] = w.c1 - w.begin; swap[g] = links[g].flip;
                if (!o.hap_windows) continue;
                const std::string &name = tgts[w.tgt].name;
                const bool flip = links[g].flip != 0;
                dg_hap_window_line(hapwin_out, name, w.c0, w.c1, (uint64_t)wins[links[g].block].c0 + 1u, ht.n1[g], ht.n2[g], ht.n0[g], ht.n_sep[g], ht.agree[g], ht.disagree[g], ht.split[g], flip);
                for (uint64_t s = ps.site_begin[g]; s < ps.site_begin[g + 1]; s++)
                    if (sr.phase[s] && ps.pos[s] >= k_lo[g] && ps.pos[s] < k_hi[g])
                        dg_hap_window_site_line(hapwin_out, name, (uint64_t)ps.pos[s] + w.begin + 1u, sr.phase[s], ht.site_counts + 4 * s, flip);
            }
            if (o.hap_contigs) {
                const dagcon_window_keep_opts ko = {nw, k_lo.data(), k_hi.data()};
                dagcon_results r2;
                dagcon_hap_map hm;
                dagcon_window_keep wk;
                memset(&hm, 0, sizeof hm); memset(&wk, 0, sizeof wk);
                if ((rc = dagcon_set_window_keep(ctx, &ko)) == DAGCON_OK) rc = dagcon_upload_haps_swapped(ctx, swap.data());
                if (rc == DAGCON_OK) rc = dagcon_run(ctx);
                if (rc == DAGCON_OK) rc = dagcon_fetch(ctx, &r2);
                if (rc == DAGCON_OK) rc = dagcon_fetch_hap_map(ctx, &hm);
                if (rc == DAGCON_OK) rc = dagcon_fetch_window_keep(ctx, &wk);          // (the derived batch's positions stay on the device)
                if (rc == DAGCON_OK) rc = dagcon_set_window_keep(ctx, nullptr);       // (the next group's own upload runs without it)
                if (rc != DAGCON_OK || wk.n_segments != r2.n_segments) { fprintf(stderr, "pbdagcon: %s\n", rc != DAGCON_OK ? dagcon_last_error(ctx) : "the kept parts do not match the segments"); status = 1; break; }
                for (uint32_t d = 0; d < hm.n_targets; d++) {
                    const uint32_t g = hm.src_target[d];
                    const Win &w = wins[w0 + g];
                    if ((long long)w.tgt != hc_tgt) { flush_contigs(); hc_tgt = w.tgt; }
                    if (r2.target_status[d] != DAGCON_OK)
                        fprintf(stderr, "pbdagcon: warning: %s window [%u, %u) hap%u skipped (%s)\n", tgts[w.tgt].name.c_str(), w.begin, w.end, (unsigned)hm.label[d],
                                dg_status_text(r2.target_status[d], MD ? kd.nonconforming : DG_CIGAR_UNFIT));
                    for (uint64_t s = r2.seg_begin[d]; s < r2.seg_begin[d + 1]; s++)
                        hst[hm.label[d] == 2u ? 1 : 0].add(w.idx, w.begin, links[g].block, r2.seq_blob + r2.seq_off[s], r2.seq_len[s], wk.i0[s], wk.i1[s], wk.p_first[s], wk.p_last[s]);
                }
                n_derived += hm.n_targets;
            }
            if (o.hap_windows && fwrite(hapwin_out.data(), 1, hapwin_out.size(), o.hap_windows) != hapwin_out.size()) { fprintf(stderr, "pbdagcon: error writing the --hap-windows file\n"); status = 1; }
            if (o.hap_contigs && fwrite(contigs_out.data(), 1, contigs_out.size(), o.hap_contigs) != contigs_out.size()) { fprintf(stderr, "pbdagcon: error writing the --hap-contigs file\n"); status = 1; }
            hapwin_out.clear(); contigs_out.clear();
        }
        if (o.pileup && fwrite(pile_out.data(), 1, pile_out.size(), o.pileup) != pile_out.size()) { fprintf(stderr, "pbdagcon: error writing the --pileup file\n"); status = 1; }
        if (o.sites && fwrite(site_out.data(), 1, site_out.size(), o.sites) != site_out.size()) { fprintf(stderr, "pbdagcon: error writing the --sites file\n"); status = 1; }
        if (o.site_reads && fwrite(reads_out.data(), 1, reads_out.size(), o.site_reads) != reads_out.size()) { fprintf(stderr, "pbdagcon: error writing the --site-reads file\n"); status = 1; }
        if (o.haplotag && fwrite(tags_out.data(), 1, tags_out.size(), o.haplotag) != tags_out.size()) { fprintf(stderr, "pbdagcon: error writing the --haplotag file\n"); status = 1; }
        if (o.linked_sites && fwrite(linked_out.data(), 1, linked_out.size(), o.linked_sites) != linked_out.size()) { fprintf(stderr, "pbdagcon: error writing the --linked-sites file\n"); status = 1; }
        pile_out.clear(); site_out.clear(); reads_out.clear(); tags_out.clear(); linked_out.clear();
        w0 = w1;
    }
    if (status == 0 && !flush_target()) status = 1;
    if (o.haplotag && !tags_out.empty() && fwrite(tags_out.data(), 1, tags_out.size(), o.haplotag) != tags_out.size()) { fprintf(stderr, "pbdagcon: error writing the --haplotag file\n"); status = 1; }
    if (status == 0 && o.hap_contigs) {
        flush_contigs();
        if (fwrite(contigs_out.data(), 1, contigs_out.size(), o.hap_contigs) != contigs_out.size()) { fprintf(stderr, "pbdagcon: error writing the --hap-contigs file\n"); status = 1; }
    }
    if (o.wp.on && o.verbose) fprintf(stderr, "pbdagcon: --phase-windows: %llu blocks over %zu windows\n", n_blocks, wins.size());
    if (o.hap_contigs && o.verbose) fprintf(stderr, "pbdagcon: --hap-contigs: %llu derived windows\n", n_derived);
    unsigned long long over_error = 0, over_depth = 0;
    for (const Tgt &t : tgts)
        for (const uint8_t f : t.fate) { over_error += (f & DAGCON_FATE_MAX_ERROR) != 0; over_depth += (f & DAGCON_FATE_MAX_DEPTH) != 0; }
    dg_report_pick(o.pick, over_error, over_depth);
    fflush(stdout);
    if (ef) {
        if (fclose(ef) != 0) { fprintf(stderr, "pbdagcon: error writing %s\n", o.edits); status = 1; }
        if (o.verbose) fprintf(stderr, "pbdagcon: %llu edits written to %s\n", n_edits, o.edits);
    }
    dagcon_destroy(ctx);
    return status;
}
