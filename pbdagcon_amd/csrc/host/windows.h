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
#include "intake.h"
#include "sam.h"

struct DgStitchPiece {
    long long t0 = 0, t1 = 0;
    std::string seq;
    std::vector<uint16_t> weight, depth;                   // --fastq: sliced as the bases are
};

// the pieces of one target, fed window by window in order
struct DgStitch {
    std::vector<DgStitchPiece> pieces;
    long long open_w = -1;                                 // window of the last piece, if it was cut at its core end
    void reset() { pieces.clear(); open_w = -1; }
    // one segment of window wi = [begin, ..), core [c0, c1); weight / depth may be NULL
    void add(long long wi, uint32_t begin, uint32_t c0, uint32_t c1, const char *seq, const uint32_t *pos, uint32_t n,
             const uint16_t *weight, const uint16_t *depth) {
        uint32_t i0 = 0;
        while (i0 < n && (uint64_t)pos[i0] + begin <= c0) i0++;
        if (i0 == n) return;
        uint32_t i1 = i0;
        while (i1 < n && (uint64_t)pos[i1] + begin <= c1) i1++;
        if (i1 <= i0) return;
        const long long last_g = (long long)pos[i1 - 1] + begin;
        if (i0 > 0 && open_w >= 0 && open_w == wi - 1 && !pieces.empty()) {
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
        open_w = i1 < n ? wi : -1;
    }
};

struct DgWinOpts {
    unsigned min_cov, min_len, trim, window, overlap;
    size_t batch_targets;
    bool fastq, verbose;
    int device;
    DgPick pick;                                           // --max-error / --max-depth
};

// SAM text: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL
struct DgSamSource {
    static constexpr DgRecordKind kind = DG_REC_PLAIN;
    const char *data; size_t size, p = 0;
    const DgRefSeqs &ref;
    unsigned long long lineno = 0, skipped = 0;
    DgSamSource(const char *d, size_t n, const DgRefSeqs &rf) : data(d), size(n), ref(rf) {}
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
            dg_sam_rec(sl, pos > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pos, lineno, ref, r);
            return 1;
        }
        return 0;
    }
};

// BAM records (bam.h); the header's references were checked against --ref when the file was opened
struct DgBamSource {
    static constexpr DgRecordKind kind = DG_REC_PACKED;
    DgBamReader &bam;
    const DgRefSeqs &ref;
    unsigned long long skipped = 0;
    DgBamSource(DgBamReader &b, const DgRefSeqs &rf) : bam(b), ref(rf) {}
    int next(DgAlnRec &r) {
        DgBamRec br;
        std::string err;
        const int rc = bam.next(br, err);
        skipped = bam.n_skipped;
        if (rc < 0) fprintf(stderr, "pbdagcon: format error: %s\n", err.c_str());
        if (rc > 0) dg_bam_rec(bam, br, ref, r);
        return rc;
    }
};

// the whole run; the process's exit status
template <class Source>
inline int dg_run_windows(const DgWinOpts &o, Source &src, const DgRefSeqs &ref) {
    struct Rec { uint32_t pos, s, e, q_len; const char *q; size_t q_bytes; uint64_t op0; uint32_t nops; bool reverse; uint32_t t_span; };   // q, q_bytes: its bytes of the q blob
    struct Tgt { std::string name; DgRefSeqs::Span sp; std::vector<Rec> recs; uint32_t max_span = 0; std::vector<uint8_t> fate; };   // fate: DAGCON_FATE_* per record, over all groups
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
            if (!ar.target) { fprintf(stderr, "pbdagcon: %s %llu: RNAME %s is not a sequence of --ref\n", kd.unit, ar.where, rname.c_str()); return 1; }
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
    }
    if (o.verbose && src.skipped) fprintf(stderr, "pbdagcon: %llu %s\n", src.skipped, kd.skipped_what);
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
        for (size_t a = w0; a < w1;) {
            size_t z = a;
            while (z < w1 && wins[z].tgt == wins[a].tgt) z++;
            Tgt &t = tgts[wins[a].tgt];
            const uint32_t lo = wins[a].begin, hi = wins[z - 1].end;
            const uint32_t bt = (uint32_t)b_tlen.size();
            b_tlen.push_back(t.sp.len); b_toff.push_back(t.sp.off);
            // records are ascending in s: none that starts more than the longest span in front of lo reaches it
            const uint32_t from = lo > t.max_span ? lo - t.max_span : 0u;
            auto it = std::lower_bound(t.recs.begin(), t.recs.end(), from, [](const Rec &r, uint32_t v) { return r.s < v; });
            for (; it != t.recs.end() && it->s < hi; ++it) {
                if (it->e <= lo) continue;
                b_fate.push_back(&t.fate[(size_t)(it - t.recs.begin())]);
                b_pos.push_back(it->pos); b_qoff.push_back(qblob.size()); b_qlen.push_back(it->q_len);
                qblob.append(it->q, it->q_bytes);
                if ((Source::kind == DG_REC_CS)) { b_cslen.push_back((uint32_t)it->q_bytes); b_tspan.push_back(it->t_span); }
                b_ops.insert(b_ops.end(), ops.begin() + (long)it->op0, ops.begin() + (long)(it->op0 + it->nops));
                b_opb.push_back(b_ops.size());
                if ((Source::kind == DG_REC_STRANDED)) b_rev.push_back(it->reverse ? 1 : 0);
            }
            b_rec.push_back(b_pos.size());
            for (size_t k = a; k < z; k++) { w_t.push_back(bt); w_b.push_back(wins[k].begin); w_e.push_back(wins[k].end); }
            a = z;
        }
        DgRecordArrays ra{};
        ra.cb.n_targets = (uint32_t)b_tlen.size(); ra.cb.tlen = b_tlen.data(); ra.cb.t_off = b_toff.data();
        ra.cb.t_blob = ref.bases.data(); ra.cb.t_bytes = ref.bases.size();
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
        if (rc != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); status = 1; break; }
        uint64_t n_fate = 0;
        if (const uint8_t *fate = dg_record_fates(ctx, &n_fate))
            for (uint64_t i = 0; i < n_fate && i < b_fate.size(); i++) *b_fate[i] |= fate[i];
        for (size_t k = w0; k < w1; k++) {
            const Win &w = wins[k];
            if ((long long)w.tgt != cur_tgt) {
                if (!flush_target()) { status = 1; break; }
                cur_tgt = w.tgt;
            }
            const size_t g = k - w0;
            if (r.target_status[g] != DAGCON_OK)
                fprintf(stderr, "pbdagcon: warning: %s window [%u, %u) skipped (%s)\n", tgts[w.tgt].name.c_str(), w.begin, w.end,
                        dg_status_text(r.target_status[g], DG_CIGAR_UNFIT));
            if (o.verbose) fprintf(stderr, "pbdagcon: %s window %u [%u, %u): %llu segments\n", tgts[w.tgt].name.c_str(), w.idx, w.begin, w.end,
                                   (unsigned long long)(r.seg_begin[g + 1] - r.seg_begin[g]));
            for (uint64_t s = r.seg_begin[g]; s < r.seg_begin[g + 1]; s++) {
                const uint64_t off = r.seq_off[s];
                st.add(w.idx, w.begin, w.c0, w.c1, r.seq_blob + off, pos + off, r.seq_len[s],
                       o.fastq ? sup.weight + off : nullptr, o.fastq ? sup.depth + off : nullptr);
            }
        }
        w0 = w1;
    }
    if (status == 0 && !flush_target()) status = 1;
    unsigned long long over_error = 0, over_depth = 0;
    for (const Tgt &t : tgts)
        for (const uint8_t f : t.fate) { over_error += (f & DAGCON_FATE_MAX_ERROR) != 0; over_depth += (f & DAGCON_FATE_MAX_DEPTH) != 0; }
    dg_report_pick(o.pick, over_error, over_depth);
    fflush(stdout);
    dagcon_destroy(ctx);
    return status;
}
