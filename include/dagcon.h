/*
 * dagcon.h -- C ABI of the MI355X-native DAGCon consensus engine.
 *
 * This is the drop-in boundary for the hot path of verdurin/pbdagcon.  The
 * reference has no FFI: its seam is the body of the Consensus worker,
 *
 *     src/cpp/main.cpp:130-138   (pbdagcon)     src/cpp/dazcon.cpp:76-89 (dazcon)
 *
 *         AlnGraphBoost ag(tlen | backbone);
 *         for each alignment: if (|qstr| < minLen) continue;
 *                             normalizeGaps; trimAln(trim); ag.addAln;
 *         ag.mergeNodes();
 *         ag.consensus(seqs, minWeight, minLen);
 *
 * One call of dagcon_consensus() replaces that sequence for a whole batch of
 * independent targets.  Everything crosses the boundary as plain pointers and
 * sizes (structure-of-arrays blobs); no C++ or torch types.  INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * All functions return DAGCON_OK (0) or a negative dagcon_status; no
 * exceptions cross the boundary.  A context is single-owner: one host thread
 * drives it; work inside is asynchronous on the context's HIP stream.
 */
#ifndef DAGCON_H
#define DAGCON_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAGCON_ABI_VERSION 2   /* 2: per-target status in dagcon_results, dagcon_host_alloc/free */

typedef enum dagcon_status {
    DAGCON_OK = 0,
    DAGCON_ERR_INVALID_ARG = -1,    /* NULL pointer, inconsistent sizes */
    DAGCON_ERR_NO_DEVICE = -2,      /* HIP runtime / gfx950 device unavailable: never falls back to CPU */
    DAGCON_ERR_HIP = -3,            /* a HIP call failed, see dagcon_last_error */
    DAGCON_ERR_NONCONFORMING = -4,  /* an alignment would drive the reference into undefined
                                       behaviour (AlnGraphBoost.cpp:64-107: start < 1, target bases
                                       past tlen, bytes outside printable ASCII) */
    DAGCON_ERR_UNSUPPORTED = -5,    /* more alignments per target than DAGCON_MAX_COVERAGE, a target too
                                       large for 25-bit vertex ids, an undefined bit in dagcon_opts.flags */
    DAGCON_ERR_WORKSPACE = -6,      /* device workspace could not be grown */
    DAGCON_ERR_INTERNAL = -7,       /* device-side invariant violated */
    DAGCON_ERR_STATE = -8           /* call sequence error (run before upload, ...) */
} dagcon_status;

#define DAGCON_MAX_COVERAGE 4094u   /* alignments per target that pass the min_len filter */

/* dagcon_opts.flags */
#define DAGCON_FLAG_RAW_ALIGNMENTS 1u /* skip normalizeGaps/trimAln: feed strings to addAln as they
                                         are (what test/cpp/AlnGraphBoostTest.cpp:11-47 does) */
#define DAGCON_FLAG_STOP_AFTER_BUILD 2u /* debug: stop after addAln (no merge, no consensus) so that
                                           dagcon_debug_graph shows the graph before mergeNodes */
#define DAGCON_FLAG_STOP_AFTER_MERGE 4u /* debug: stop after mergeNodes */
#define DAGCON_FLAG_DEBUG_RESWEEP 16u   /* debug: treat the segmented bestPath sweep as inexact, so that
                                           every target takes the one-piece re-sweep (tests only; targets that take
                                           it by themselves, scores past 2^22: tests/test_bestpath_bound.py) */
#define DAGCON_FLAG_LOCAL_ALIGN 32u    /* dagcon_align / dagcon_consensus_pre align local ends (see dagcon_align):
                                          read ends that do not align stay out of the alignment */
#define DAGCON_FLAG_BASE_SUPPORT 64u  /* keep the support of every consensus base: dagcon_fetch_support */
#define DAGCON_FLAG_BASE_POS 256u     /* keep the target position of every consensus base: dagcon_fetch_positions */
#define DAGCON_FLAGS_ALL (DAGCON_FLAG_RAW_ALIGNMENTS | DAGCON_FLAG_STOP_AFTER_BUILD | \
                          DAGCON_FLAG_STOP_AFTER_MERGE | DAGCON_FLAG_DEBUG_RESWEEP | DAGCON_FLAG_LOCAL_ALIGN | \
                          DAGCON_FLAG_BASE_SUPPORT | DAGCON_FLAG_BASE_POS)
                                        /* dagcon_create refuses any other bit (DAGCON_ERR_UNSUPPORTED) */

/* Mirrors ProgramOpts (src/cpp/ProgramOpts.hpp:8-36) for this path. */
typedef struct dagcon_opts {
    uint32_t min_cov;    /* -c: targets with fewer alignments are skipped (main.cpp:66-72,118) */
    uint32_t min_len;    /* -m: alignment pre-filter on raw |qstr| (main.cpp:132) and minimum
                            emitted segment length (AlnGraphBoost.cpp:359,371) */
    uint32_t trim;       /* -t: trimAln length (main.cpp:134) */
    int32_t  min_weight; /* consensus minWeight; <0 means "= min_cov" as main.cpp:261,279 does */
    int32_t  device;     /* HIP device ordinal */
    uint32_t flags;
    uint32_t max_segments; /* workers per target for mergeNodes (bestPath: three times as many): a
                              target is swept in up to this many pieces, split at backbone vertices
                              every read passes through (the result does not depend on it).
                              0 = automatic, 1 = one sequential sweep per target, at most 64 */
    uint32_t min_segment_len; /* shortest backbone stretch given a worker of its own; 0 = default (768; down to 192 for small batches) */
} dagcon_opts;

/* Defaults of pbdagcon (main.cpp:181-211): -c 6 -m 500 -t 50. */
void dagcon_default_opts(dagcon_opts *o);

/*
 * A batch of independent targets.  Alignment a of target t is
 * a in [aln_begin[t], aln_begin[t+1]); its strings are qstr[aln_off[a] ..
 * aln_off[a]+aln_len[a]) and the same range of tstr (equal lengths, as
 * Alignment.hpp:35-37 requires).  aln_start is 1-based (Alignment.hpp:21-22).
 * Order of alignments inside a target is the order the reference would call
 * addAln in; it is semantics (adjacency order).
 */
typedef struct dagcon_batch {
    uint32_t n_targets;
    const uint32_t *tlen;        /* [n_targets] backbone length (Alignment::tlen) */
    const uint64_t *aln_begin;   /* [n_targets+1] */
    const uint32_t *aln_start;   /* [n_alns] */
    const uint64_t *aln_off;     /* [n_alns] byte offset into qstr / tstr */
    const uint32_t *aln_len;     /* [n_alns] */
    const char *qstr;            /* query blob  */
    const char *tstr;            /* target blob */
    uint64_t blob_bytes;         /* size of each blob */
    const char *backbone;        /* optional: real backbone bases (dazcon.cpp:76); NULL = 'N'
                                    backbone filled in by the reads (main.cpp:130) */
    const uint64_t *backbone_off;/* [n_targets] offsets into backbone when it is given */
} dagcon_batch;

/*
 * Consensus segments, CnsResult (AlnGraphBoost.hpp:63-66) for every target.
 * Segments of target t are s in [seg_begin[t], seg_begin[t+1]).  range0/range1
 * index the target's consensus string (quirk Q5), seq is seq_blob[seq_off[s] ..
 * +seq_len[s]).  The arrays are owned by the context and stay valid until the
 * next dagcon_upload / dagcon_consensus / dagcon_destroy on it.
 */
typedef struct dagcon_results {
    uint32_t n_targets;
    uint64_t n_segments;
    const uint64_t *seg_begin;   /* [n_targets+1] */
    const int32_t *range0;       /* [n_segments] */
    const int32_t *range1;       /* [n_segments] */
    const uint64_t *seq_off;     /* [n_segments] */
    const uint32_t *seq_len;     /* [n_segments] */
    const char *seq_blob;
    uint64_t seq_bytes;
    /* ABI 2.  A failure is confined to its target, as in the reference, where an assert or the
     * undefined behaviour behind it hits one worker's one target (AlnGraphBoost.cpp:71-72):
     * target_status[t] is DAGCON_OK or the dagcon_status that target alone failed with
     * (DAGCON_ERR_NONCONFORMING, DAGCON_ERR_UNSUPPORTED: too large, DAGCON_ERR_INTERNAL); a failed
     * target has no segments, every other target of the batch is complete and exact.  The call
     * that filled the struct still returns DAGCON_OK; dagcon_last_error describes the first failure. */
    const int32_t *target_status; /* [n_targets] */
    uint32_t n_failed;            /* targets whose status is not DAGCON_OK */
} dagcon_results;

/*
 * Per-base support of the consensus (a context created with DAGCON_FLAG_BASE_SUPPORT).  The reference has no such
 * output: this is this build's own definition, PARITY UNPINNED.  Entry i describes seq_blob[i] of the results, so
 * segment s has [seq_off[s], seq_off[s] + seq_len[s]) of both arrays; n == seq_bytes, and a failed target, which has
 * no segments, has no entries.  For the best-path vertex v a consensus base comes from (AlnGraphBoost.cpp:375-459):
 *   weight[i]  v's node weight after mergeNodes (the value consensus compares with minWeight);
 *   depth[i]   the coverage of _bbMap[v], the backbone vertex whose coverage bestPath charges for v.
 * With K the target's alignment count (<= DAGCON_MAX_COVERAGE): depth <= K, weight <= K + 1.  addAln adds 1 to a
 * coverage per read that consumes the position and 1 to a weight per read that passes through the vertex, once per read;
 * a backbone vertex starts at weight 1 (AlnGraphBoost.cpp:32,54).  mergeNodes unites siblings that every one of their
 * reads goes through next (or came from) only, so no read passes through two of them, and adds their weights; a merged
 * vertex holds at most one backbone vertex.  A target where either value would exceed 65,535 fails with
 * DAGCON_ERR_INTERNAL; no value wraps.  The arrays are owned by the context, valid as long as the results of the same fetch.
 * dagcon_fetch_support is valid after dagcon_fetch, dagcon_consensus or dagcon_consensus_pre on such a context, and
 * returns DAGCON_ERR_STATE otherwise: without the flag, before a fetch, or under DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE.
 */
typedef struct dagcon_support {
    uint64_t n;                  /* == dagcon_results.seq_bytes */
    const uint16_t *weight;      /* [n] */
    const uint16_t *depth;       /* [n] */
} dagcon_support;

/* Per-stage device time of the last dagcon_run, from HIP events on the
 * context's stream (milliseconds), plus the algorithmic byte count SURVEY.md
 * section 8(d) defines. */
typedef struct dagcon_timings {
    float ms_total;          /* first kernel start -> last kernel end */
    float ms_normalize;      /* stage a1: count + normalizeGaps + trimAln */
    float ms_build;          /* stage a2: carve + init + emit + adjacency lists */
    float ms_merge;          /* stage b : mergeNodes */
    float ms_bestpath;       /* stage c : bestPath + consensus segmentation */
    uint64_t algorithmic_bytes; /* sum(|q|+|t|) over alignments passing min_len + output bases */
    uint64_t consensus_bases;   /* sum of emitted segment lengths */
    uint64_t n_alignments;      /* alignments that passed min_len and reached the device */
    uint64_t n_columns;         /* normalised, trimmed columns threaded into graphs */
    uint64_t n_nodes;           /* graph vertices before merging, all targets */
    uint32_t reruns;            /* times the batch was re-run after growing the workspace */
    uint32_t merge_segments;    /* pieces the targets of the batch were swept in, all targets */
} dagcon_timings;

typedef struct dagcon_ctx dagcon_ctx;

int  dagcon_abi_version(void);
int  dagcon_create(const dagcon_opts *opts, dagcon_ctx **out);
void dagcon_destroy(dagcon_ctx *ctx);
const char *dagcon_last_error(const dagcon_ctx *ctx);

/* The drop-in call: replaces main.cpp:130-138 for every target of the batch.
 * Equivalent to dagcon_upload + dagcon_run + dagcon_fetch. */
int dagcon_consensus(dagcon_ctx *ctx, const dagcon_batch *batch, dagcon_results *results);

/* The same work in three steps, so that a caller can keep inputs resident in
 * HBM and time the device path alone (bench.py does). */
int dagcon_upload(dagcon_ctx *ctx, const dagcon_batch *batch); /* host filter + H2D, synchronous */
int dagcon_run(dagcon_ctx *ctx);                               /* enqueue all kernels, asynchronous */
int dagcon_sync(dagcon_ctx *ctx);                              /* wait for the stream */
int dagcon_fetch(dagcon_ctx *ctx, dagcon_results *results);    /* sync + status check + D2H */
int dagcon_get_timings(dagcon_ctx *ctx, dagcon_timings *out);  /* after dagcon_sync / dagcon_fetch */
int dagcon_fetch_support(dagcon_ctx *ctx, dagcon_support *out); /* DAGCON_FLAG_BASE_SUPPORT: see dagcon_support */

/*
 * Per-base target position of the consensus (a context created with DAGCON_FLAG_BASE_POS; independent of
 * DAGCON_FLAG_BASE_SUPPORT, either alone or both).  (*pos)[i] describes seq_blob[i]; *n == seq_bytes.  It is _bbMap[v] of
 * the best-path vertex v the base comes from, as a vertex index of the reference: p in 1 .. tlen is target base p
 * (AlnGraphBoost.cpp:34,57); an inserted vertex has the position of the next target base, up to tlen + 1 (:101); after
 * mergeNodes a survivor keeps its own value.  The values need NOT be monotone along a segment: a merged insertion can
 * carry a position above that of the backbone vertex that follows it.  This is what lets a caller join the results of
 * neighbouring windows of one long target at a target coordinate (range0 / range1 only index the consensus string, Q5).
 * Lifetime and state rules of dagcon_fetch_support: DAGCON_ERR_STATE without the flag, before a fetch, or under
 * DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE; the array is owned by the context, valid as long as the results of the same fetch.
 */
int dagcon_fetch_positions(dagcon_ctx *ctx, const uint32_t **pos, uint64_t *n);

/*
 * Edits: where the consensus differs from its target (off by default; a context switch like dagcon_set_record_filter,
 * on a context created with DAGCON_FLAG_BASE_POS).  The reference has no such output: this is this build's own
 * definition, PARITY UNPINNED.  The device derives the list from the best path itself, nothing is aligned: a consensus
 * base comes from a backbone vertex (a target base kept) or from an inserted vertex (a base added), and a target
 * position that lies between two consecutive backbone bases of the path and is neither is a base dropped.
 * Segment s of the results lies on a target of a record upload (with windows: on a window, and every position below
 * is relative to the window, whose bases are t_blob[t_off + begin ..]).  Its bases are i = 0 .. n - 1; those from a
 * backbone vertex are j_0 < .. < j_m with the 1-based target positions P (dagcon_fetch_positions), which rise strictly.
 *   - span: seg_t0 = P(j_0) - 1, seg_t1 = P(j_m), 0-based half-open [t0, t1); a segment without a backbone base has
 *     t0 = t1 = (the position of its first base) - 1;
 *   - one raw edit per pair of consecutive backbone bases j_a, j_b with inserted bases between them (j_b - j_a > 1) or
 *     target bases skipped (P(j_b) - P(j_a) > 1): it replaces target bases [P(j_a), P(j_b) - 1) (0-based) by the
 *     consensus bases (j_a, j_b);
 *   - the inserted bases in front of j_0 are an insertion at t0, those behind j_m an insertion at t1, a segment
 *     without a backbone base is one insertion at t0;
 *   - trim: equal leading bytes of the replaced target bytes and the replacing bytes are taken off both (exact bytes,
 *     case counts) and both starts advance, then equal trailing bytes; an edit with nothing left on either side is
 *     dropped.
 * Edits of segment s are e in [edit_begin[s], edit_begin[s + 1]), in ascending target order and disjoint: target
 * bases [t_pos, t_pos + t_len) become seq_blob[c_off, c_off + c_len).  c_off is defined also when c_len == 0: the index
 * of the consensus base the deletion stands in front of (seq_off[s] + seq_len[s] cannot occur: a segment's last edit
 * with c_len == 0 lies in front of j_m).  Where a target's bases lie in seq_blob is not fixed from run to run (seq_off
 * says where), so c_off is reproducible as c_off - seq_off[s], not as a number.
 * INVARIANT: walking the target's bases [seg_t0, seg_t1) and replacing [t_pos, t_pos + t_len) by seq_blob[c_off,
 * c_off + c_len) for every edit of s yields the segment's sequence exactly.  It rests on: the byte of a backbone base
 * is its target byte (an 'N' backbone is filled from tstr, which the record intake copies from t_blob).  That holds
 * for every backbone vertex a read passes through, so for every base a min_weight of 2 or more lets out.
 * dagcon_set_edits: DAGCON_ERR_STATE on a context without DAGCON_FLAG_BASE_POS.  The switch holds for every later
 * dagcon_upload_cigar* / _packed / _strand / dagcon_upload_cs (and the dagcon_consensus_* of those); with it off no
 * kernel, buffer or copy differs from a context that never heard of it.  With it on, three more kernels run behind the
 * consensus (csrc/k_edits.hip.h), the edit arrays come back in the fetch's second round, and the 4 bytes a base of
 * dagcon_fetch_positions are copied only when that is called.
 * dagcon_fetch_edits is valid after a fetch that followed such an upload with the switch on; DAGCON_ERR_STATE
 * otherwise: switch off, dagcon_consensus / dagcon_consensus_pre (no single target on the device), before a fetch, or
 * under DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE.  A failed target has no segments and no edits.  The arrays are owned by
 * the context, valid as long as the results of the same fetch (as dagcon_support).
 */
typedef struct dagcon_edits {
    uint64_t n_segments, n;              /* n_segments == dagcon_results.n_segments */
    const uint32_t *seg_t0, *seg_t1;     /* [n_segments] */
    const uint64_t *edit_begin;          /* [n_segments + 1] */
    const uint32_t *t_pos, *t_len;       /* [n] */
    const uint64_t *c_off;               /* [n] into seq_blob */
    const uint32_t *c_len;               /* [n] */
} dagcon_edits;
int dagcon_set_edits(dagcon_ctx *ctx, int on);
int dagcon_fetch_edits(dagcon_ctx *ctx, dagcon_edits *out);

/*
 * Read support per edit: how many alignments stand behind each edit of dagcon_edits (off by default; a second switch
 * behind dagcon_set_edits).  This is this build's own rule, PARITY UNPINNED: the reference has no such output.
 * DAGCON_FLAG_BASE_SUPPORT cannot answer the question: it has a weight only for vertices on the best path, a deletion
 * has no base to carry a weight, and the target's own allele is not on the path.
 * Everything is relative to a target of the pipeline: a target of the batch, or with windows a window.
 *   - T[0, tlen) are its bytes as the record intake left them.
 *   - A segment has span [t0, t1) and consensus bytes S.
 *   - Its edits are e_0 .. e_{m-1}, ascending, as (t_pos, t_len, c, c_len) with c relative to S.
 *   - x ~ y means the two bytes are equal after clearing bit 0x20 in both.
 * 1. Window of an edit.  Start with L = t_pos, R = t_pos + t_len.  Clamps: lo = t_pos + t_len of the edit before it, or
 *    t0 for the first edit; hi = t_pos of the edit behind it, or t1 for the last edit.  Only a pure insertion or a pure
 *    deletion is extended, that is an edit where exactly one of t_len, c_len is 0.  Let u be the k bytes of the
 *    non-empty side.  Left: while L > lo and T[L-1] ~ u[(k-1-j) mod k], with j the steps taken so far, do L--.  Right:
 *    while R < hi and T[R] ~ u[j mod k], do R++.  So the window covers every place the same indel could have been
 *    written in a repeat.  L and R are non-decreasing along the segment.
 * 2. Groups.  Edit i > 0 joins the group of edit i-1 iff L_i <= R_{i-1}: the windows touch or overlap.  A group's
 *    window is [gL, gR) = [L of its first edit, R of its last edit).  Its ref allele is T[gL, gR).  Its alt allele is
 *    S[cL, cR), with cL = c_first - (t_pos_first - gL) and cR = c_last + c_len_last + (gR - t_pos_last - t_len_last).
 *    The edits invariant makes the bytes between edits identical on both sides.  Two groups of a segment are separated
 *    by at least one target base.
 * 3. The alignments counted are the target's alignments of at least min_len columns, as the graph took them: after
 *    normalizeGaps and trimAln, and non-empty.  Alignment a has columns (q, t).  Its first target base is s0 (its
 *    start after the trim, 0-based).  It covers [s0, e0).  A column's coordinate tc is s0 plus the target-base columns
 *    in front of it.
 *    Spanning: the alignment spans the group iff both hold: gL > 0 ? s0 <= gL-1 : s0 == 0, and
 *    gR < tlen ? e0-1 >= gR : e0 == tlen.
 *    Allele: the alignment's allele is its q bytes other than the gap, taken from the columns with tc >= gL and
 *    (tc < gR, or tc == gR with a gap in t).  Insertions at either end of the window belong to it.
 *    Flanks: the flanks are good iff the column holding target base gL-1 has a read base ~ its target base, and
 *    likewise for the column of base gR.  A flank exists when gL > 0 (left flank) or gR < tlen (right flank).  A flank
 *    that does not exist asks nothing.
 *    Class: alt: the flanks are good and the allele ~ the alt allele (same length, byte by byte).  ref: otherwise, the
 *    flanks are good and the allele ~ the ref allele.  other: every remaining spanning alignment.  Alt is tested first.
 * 4. Output is per edit, n == dagcon_edits.n, in the same order.  Every edit of a group carries the group's values:
 *    w_begin = gL, w_end = gR, span: the spanning alignments, alt: those in class alt, ref: those in class ref.
 *    alt + ref <= span <= the target's alignment count.  A failed target has no entries.
 * dagcon_set_edit_support: DAGCON_ERR_STATE unless dagcon_set_edits is on; turning edits off turns this off.  With the
 * switch off no kernel, buffer, launch or copy differs; with it on three more kernels run behind the edit kernels
 * (csrc/k_evidence.hip.h) and the arrays come back in the fetch's second round beside the edit records.
 * dagcon_fetch_edit_support is valid exactly when dagcon_fetch_edits is and the switch was on at the upload;
 * DAGCON_ERR_STATE otherwise.  The arrays are owned by the context, valid as long as the results of the same fetch.
 */
typedef struct dagcon_edit_support {
    uint64_t n;                                          /* == dagcon_edits.n */
    const uint32_t *w_begin, *w_end, *span, *alt, *ref;  /* [n] */
} dagcon_edit_support;
int dagcon_set_edit_support(dagcon_ctx *ctx, int on);
int dagcon_fetch_edit_support(dagcon_ctx *ctx, dagcon_edit_support *out);

/*
 * Pile-up: what the alignments show at every target position, and the positions where a second allele has support (off
 * by default; a context switch like dagcon_set_record_filter).  This is this build's own rule, PARITY UNPINNED: the
 * reference has no such output.  DAGCON_FLAG_BASE_SUPPORT gives the weight of the winning vertex and a depth, not the
 * alternatives; dagcon_edit_support counts only at edits.  It needs neither DAGCON_FLAG_BASE_POS nor the edits, and it
 * holds for every way in: dagcon_consensus, dagcon_consensus_pre, every record upload, with or without windows.
 * Everything is relative to a target of the pipeline: a target of the batch, or with windows a window.
 * 1. The alignments counted are exactly those the graph took: the target's alignments of at least min_len columns,
 *    after normalizeGaps and trimAln, and non-empty; records that dagcon_set_record_filter leaves out are not among them.
 *    A target below min_cov has no graph and counts nothing.
 * 2. Alignment a has columns (q, t), '-' is the gap.  Its first target base after the trim is s0 (0-based).  The
 *    coordinate tc of a column is s0 plus the columns with t != '-' in front of it.
 *      t != '-', q == '-'    DEL[tc] += 1
 *      t != '-', q != '-'    one of A[tc], C[tc], G[tc], T[tc] += 1, by q & 0xDF (letter case does not count); any other
 *                            byte: N[tc] += 1
 *      t == '-', q != '-'    an inserted base; it belongs to the target base in front of it, tc - 1.  A run of inserted
 *                            columns counts its alignment once: INS[tc - 1] += 1 at the run's first column, which is
 *                            the inserted column whose neighbour in front, in the same alignment, has t != '-'.  Inserted
 *                            columns in front of the alignment's first target-base column have no such neighbour and
 *                            count nowhere
 *      both '-'              nowhere
 * 3. Layout: eight uint16_t per position, A C G T N DEL INS 0.  depth = A + C + G + T + N + DEL is not stored.
 *    INS <= depth always: the column in front of a run's first column is a target-base column of the same alignment.
 *    A count is at most DAGCON_MAX_COVERAGE (4094): 16 bits hold it.  On the device two counters share a 32-bit word
 *    and an add is one 32-bit atomic add of 1 or 1 << 16; neither half can carry into the other.
 * 4. A failed target (target_status != DAGCON_OK) has all-zero counts and no sites.
 * 5. Sites, given min_count and min_frac_ppm: with s2 the second largest of the six counts A C G T N DEL (ties as
 *    they fall: a 3/3 split has s2 = 3) and m = max(s2, min(INS, depth - INS)), position p is a site iff depth > 0 and
 *    m >= min_count and m * 1000000 >= min_frac_ppm * depth, in 64-bit integers, no floating point.  With 0 / 0 every
 *    position with depth is a site.  The sites of a target are listed in ascending position.
 * dagcon_set_pileup: NULL turns it off; min_frac_ppm > 1000000 is DAGCON_ERR_INVALID_ARG (the switch stays as it was).
 * The switch and its thresholds are read at the upload (dagcon_upload and every other upload, the dagcon_consensus* calls
 * among them).  With it off no kernel, buffer, memset, launch or copy differs from a context that never heard of it.
 * With it on, the counters are cleared and four kernels (csrc/k_pileup.hip.h) run behind the consensus in every
 * execution of the run, the site list comes back with dagcon_fetch, and the counts, 16 bytes a position, stay on the
 * device and are copied only when dagcon_fetch_pileup is called.  On a DAGCON_FLAG_RAW_ALIGNMENTS context the column
 * arena is filled too, with the strings as given: the switch is accepted and the same rule counts on those columns.
 * dagcon_fetch_pileup / dagcon_fetch_pileup_sites are valid after a dagcon_fetch of an upload made with the switch on;
 * DAGCON_ERR_STATE otherwise: switch off at the upload, before a fetch, or under DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE.
 * The arrays are owned by the context, valid as long as the results of the same fetch.
 */
typedef struct dagcon_pileup_opts { uint32_t min_count, min_frac_ppm; } dagcon_pileup_opts;
int dagcon_set_pileup(dagcon_ctx *ctx, const dagcon_pileup_opts *o);   /* NULL: off (the default) */
typedef struct dagcon_pileup {       /* counts[8 * (pos_begin[t] + p)] .. : A C G T N DEL INS 0 of position p of target t */
    uint32_t n_targets; const uint64_t *pos_begin; const uint16_t *counts;   /* pos_begin: [n_targets + 1] */
} dagcon_pileup;
int dagcon_fetch_pileup(dagcon_ctx *ctx, dagcon_pileup *out);
typedef struct dagcon_pileup_sites { /* sites of target t: [site_begin[t], site_begin[t + 1]) */
    uint32_t n_targets; const uint64_t *site_begin; const uint32_t *pos; const uint16_t *counts;   /* counts: eight per site */
} dagcon_pileup_sites;
int dagcon_fetch_pileup_sites(dagcon_ctx *ctx, dagcon_pileup_sites *out);

/*
 * Site reads: which alignment shows which allele at each site of the pile-up, and a split of a target's alignments into
 * two groups that agree site after site (off by default; a context switch like dagcon_set_pileup, which it needs).  A
 * heterozygous site and a collapsed repeat copy are carried by the same reads at every site; a systematic error is not.
 * This is this build's own rule, PARITY UNPINNED: the reference has no such output.  Everything is relative to a target
 * of the pipeline: a target of the batch, or with windows a window.
 * 1. The taken alignments are those of rule 1 of the pile-up: at least min_len columns, normalised, trimmed, non-empty,
 *    of a target with a graph (not below min_cov, not failed), not left out by dagcon_set_record_filter.  They are
 *    numbered x = 0 .. n_aln - 1 in the order the pipeline holds them: batch order with the others removed.  aln_tgt[x]
 *    is the target (the window), aln_src[x] the index the caller gave the alignment by: the alignment index of a
 *    dagcon_batch, the record index of every record batch (with windows: the piece's record) and of a dagcon_pre_batch.
 * 2. Entries.  Alignment x has an entry at site k (position p of its target) iff it has a column with a target base at
 *    coordinate p (rule 2 of the pile-up).  An entry holds one byte, code = cls | ins << 3: cls 0..5 for A C G T N DEL by
 *    exactly the classification of that rule, ins = 1 iff an insertion run of this alignment is counted at p by the
 *    pile-up's INS rule.  The inserted bases themselves are not compared: two alignments that insert different bases
 *    behind p carry the same code (dagcon_set_site_alleles, rule 8 below, compares them).  The entries of an alignment are in ascending position, ent_begin[x] .. ent_begin[x + 1];
 *    ent_site is an index into the arrays of dagcon_fetch_pileup_sites.  For every site the entries' classes add up to
 *    the site's six counts and their ins bits to its INS.
 * 3. Signs.  An entry gets M in {+1, 0, -1} from its site's counts, s2 the second largest of the six as in the site rule.
 *    If min(INS, depth - INS) > s2 the site is an insertion site: M = -1 if ins, else +1.  Otherwise it is a base site:
 *    k1 is the class with the largest count, ties to the lowest index; k2 the class with the largest count among the
 *    others, ties to the lowest index, and only if that count is > 0; M = +1 for cls == k1, -1 for cls == k2, else 0.
 * 4. The split (phase != 0), per target, in integers, nothing in it depends on an order.  The seed is the taken alignment
 *    with the most entries of M != 0, ties to the lowest x; without one everything of the target stays 0.  sigma[k] =
 *    M(seed, k) at the seed's entries, 0 elsewhere.  Then exactly `rounds` rounds of two steps:
 *      h[x]     = sgn(sum over k of M(x, k) * sigma[k])    for every alignment of the target
 *      sigma[k] = sgn(sum over x of M(x, k) * h[x])        for every site of the target
 *    with sgn(0) = 0 (the device stops at a round that changes nothing: the answer is the same).  hap[x] is 1 for h = +1,
 *    2 for h = -1, 0 for unassigned: no informative site, a tie, or more than `rounds` read-overlap hops from the seed.
 *    phase[k] = sigma[k].  A round carries the labels one hop of overlapping reads further; rounds = 0 means the default,
 *    8, this build's own choice: a target tiled by reads more than `rounds` hops deep leaves the far reads unassigned.
 *    More than two groups are not looked for, and windows are labelled each on its own.
 * 5. A failed target (target_status != DAGCON_OK) has no taken alignments, no entries and no phase.
 * dagcon_set_site_reads: NULL turns it off; rounds > 64 is DAGCON_ERR_INVALID_ARG (the switch stays as it was).  The
 * switch is read at the upload and needs dagcon_set_pileup on at the same upload.  With either off at the upload no
 * kernel, buffer, memset, launch or copy differs from a context that never heard of it, and dagcon_fetch_site_reads is
 * DAGCON_ERR_STATE; the same before a dagcon_fetch and under DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE.  With both on, the
 * kernels of csrc/k_site_reads.hip.h run behind the pile-up's in every execution of the run; the entry arena grows by a
 * re-run (at thresholds 0 / 0 every target-base column is an entry).  The arrays stay on the device and are copied only
 * when dagcon_fetch_site_reads is called.  They are owned by the context, valid as long as the results of the same fetch.
 */
typedef struct dagcon_site_reads_opts { uint32_t phase, rounds; } dagcon_site_reads_opts;   /* rounds 0: the default, 8 */
int dagcon_set_site_reads(dagcon_ctx *ctx, const dagcon_site_reads_opts *o);   /* NULL: off (the default) */
typedef struct dagcon_site_reads {
    uint64_t n_aln; const uint32_t *aln_tgt; const uint64_t *aln_src;      /* the taken alignments */
    const uint64_t *ent_begin;                                             /* [n_aln + 1] */
    const uint64_t *ent_site; const uint8_t *ent_code;                     /* ent_site: index into dagcon_pileup_sites' arrays */
    const uint8_t *hap; const int8_t *phase;                               /* [n_aln], [sites]; NULL when phase was off */
} dagcon_site_reads;
int dagcon_fetch_site_reads(dagcon_ctx *ctx, dagcon_site_reads *out);

/*
 * Consensus per read group: a tally of the two-way split, and a second batch derived on the device from the first (off by
 * default; a context switch that needs dagcon_set_pileup and dagcon_set_site_reads with phase != 0 on at the same upload).
 * This is this build's own rule, PARITY UNPINNED, in the terms of rules 1 to 4 of the site reads above.
 * 6. The tally.  Per site k of target t, four counts over the entries (x, k) with M(x, k) != 0 and hap[x] != 0:
 *      P1: hap 1, M = +1     M1: hap 1, M = -1     P2: hap 2, M = +1     M2: hap 2, M = -1
 *    With sigma = phase[k]: agree_k = P1 + M2 for sigma = +1, M1 + P2 for sigma = -1, 0 for sigma = 0; disagree_k is the
 *    other pair under the same condition.  The site is SEPARATING iff sigma != 0 and both terms of agree_k are >= 1: each
 *    label shows its own allele there at least once.
 *    Per target: n1, n2, n0 the taken alignments with hap 1, 2, 0; n_sep the number of separating sites; agree and disagree
 *    the sums of agree_k and disagree_k over its sites; K the alignments the pipeline holds for the target, those of at
 *    least min_len columns (taken or not).  The target is SPLIT iff its status is DAGCON_OK and n_sep >= min_sites and
 *    n1 >= min_reads and n2 >= min_reads and K - n2 >= max(1, min_cov) and K - n1 >= max(1, min_cov).  Everything is in
 *    integers; nothing depends on an order.  min_sites = 0 / min_reads = 0 mean the defaults 2 and 3, this build's own
 *    choice: one site is what a systematic error gives, and three reads a label are the least that outvote one error.
 * 7. The groups.  Group g (1, 2) of a split target holds the target's alignments among those K whose hap is g or 0, in
 *    their own order; the alignments that are not taken (empty after the trim) are in both groups too.  Unlabelled reads
 *    carry the regions without sites, where the groups do not differ: without them a group's consensus would break off
 *    wherever its labelled reads end.  K - n2 and K - n1 are the sizes of groups 1 and 2: the last two conditions of rule 6
 *    say that either group is a target the pipeline builds a graph for.
 * dagcon_set_hap_consensus: NULL turns it off.  The switch is read at the upload; with any of the three switches off at
 * the upload no buffer, memset, launch or copy differs from a context that never heard of it and no kernel does other
 * work (k_norm_chunk tests one kernel argument, NULL for every batch but dagcon_upload_haps' own, whose groups share
 * strings and so cannot share the scratch that lies at a string's offset), and
 * dagcon_fetch_hap_tally and dagcon_upload_haps are DAGCON_ERR_STATE; the same before a dagcon_fetch and under
 * DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE.  With all three on, the kernels of csrc/k_hap.hip.h run behind the split in
 * every execution of the run.
 * dagcon_fetch_hap_tally: the arrays are copied when it is called (the per-target records also by dagcon_upload_haps).
 * A failed target has zeros and is not split; site_counts holds P1 M1 P2 M2 per site of dagcon_fetch_pileup_sites, which
 * leaves out a failed target's sites.  Owned by the context, valid as long as the results of the same fetch.
 * dagcon_upload_haps: valid exactly when dagcon_fetch_hap_tally is.  It copies hap[] (one byte an alignment) and the
 * per-target records to the host and uploads a batch of two targets per split target, in target order, label 1 then
 * label 2, by rule 7, with the tlen (and the backbone, if the first batch had one) of its target.  The strings are those
 * the first batch left on the device, whichever way they came in: none crosses the bus and none is copied.  It is an
 * upload like any other: the results of the first batch and dagcon_fetch_md_targets stop being valid, every optional
 * output (edits, edit support, pile-up, site reads, site alleles, joined sites, tally) is off for the derived batch and its fetch DAGCON_ERR_STATE (but for dagcon_set_hap_calls, rule 11 below, and dagcon_set_window_keep, rule 12),
 * the record filter has nothing to do, and a second dagcon_upload_haps in a row is DAGCON_ERR_STATE.  min_cov, min_len,
 * trim, min_weight and the context's flags (DAGCON_FLAG_BASE_SUPPORT / _BASE_POS with their fetches among them) hold as
 * for dagcon_upload; a group with fewer reads than min_weight lets few bases out, which is the caller's option to set as
 * for any shallow target.  No split target: a batch of 0 targets, which runs and fetches with n_targets == 0.  A
 * dagcon_upload_haps that fails leaves the context as any failed upload does: the first batch's results are gone.  Then
 * dagcon_run / dagcon_sync / dagcon_fetch as ever: per group the result is that of dagcon_consensus on the group's
 * strings, byte for byte.
 * dagcon_fetch_hap_map: what the derived batch holds; valid from dagcon_upload_haps to the next upload.
 */
typedef struct dagcon_hap_opts { uint32_t min_sites, min_reads; } dagcon_hap_opts;  /* 0, 0: the defaults 2 and 3, this build's own choice */
int dagcon_set_hap_consensus(dagcon_ctx *ctx, const dagcon_hap_opts *o);   /* NULL: off (the default) */
typedef struct dagcon_hap_tally {
    uint32_t n_targets;
    const uint32_t *n1, *n2, *n0, *n_sep, *agree, *disagree;   /* [n_targets] */
    const uint8_t *split;                                      /* [n_targets] */
    const uint16_t *site_counts;                               /* P1 M1 P2 M2 per site of dagcon_fetch_pileup_sites */
} dagcon_hap_tally;
int dagcon_fetch_hap_tally(dagcon_ctx *ctx, dagcon_hap_tally *out);
int dagcon_upload_haps(dagcon_ctx *ctx);                       /* then dagcon_run / _sync / _fetch as ever */
typedef struct dagcon_hap_map {
    uint32_t n_targets;                /* 2 x the split targets; == dagcon_results.n_targets of the fetch that follows */
    const uint32_t *src_target;        /* [n_targets] target of the first batch, ascending; label 1 then label 2 */
    const uint8_t *label;              /* [n_targets] 1 or 2 */
    const uint64_t *aln_begin;         /* [n_targets + 1] */
    const uint64_t *aln_src;           /* the caller's index of each alignment: dagcon_site_reads.aln_src's meaning */
} dagcon_hap_map;
int dagcon_fetch_hap_map(dagcon_ctx *ctx, dagcon_hap_map *out);

/*
 * Site alleles: the alleles themselves at the sites of the pile-up, counted per site and named per entry (off by
 * default; a context switch that needs dagcon_set_pileup and dagcon_set_site_reads on at the same upload).  The code of
 * rule 2 of the site reads says A C G T N DEL and "an insertion run starts here"; normalizeGaps writes a mismatch as the
 * target base dropped and the read base inserted behind it, so a substitution is DEL + ins and the base it put there
 * lives in the inserted run alone.  This is this build's own rule, PARITY UNPINNED, in the terms of the pile-up and of
 * rules 1 to 7 above.
 * 8. The allele of an entry.  Entry (x, k) is alignment x at site k, at position p.  Let i be the column of x with
 *    t != '-' and coordinate p, and R the columns i + 1, i + 2, .. for as long as they lie inside the alignment's trimmed
 *    columns and have t == '-' and q != '-'.  The allele is the byte string q[i] (left out when it is '-') followed by
 *    the q bytes of R: the read's bases between target base p and target base p + 1.  Each byte is mapped as the pile-up
 *    classifies: b & 0xDF in A C G T gives that letter, anything else N.  Its length L may be 0: a deletion.  By
 *    construction cls == DEL iff q[i] == '-', and the entry's ins bit is set iff R is not empty.
 *    The key is a 64-bit integer with the codes A = 1, C = 2, G = 3, T = 4, N = 5: base j < min(L, 20) contributes
 *    code << (3 * (19 - j)), and bit 60 is set iff L > 20 (the allele is LONG).  Unsigned comparison of keys is
 *    lexicographic on the first 20 bases, a shorter allele before its extensions, long alleles last.  Long alleles
 *    with the same first 20 bases have the same key and COUNT AS ONE ALLELE: the rule does not look past 20 bases.
 *    Text: the bases, "-" for the empty allele, a trailing "+" when long (dagcon_allele_text).
 *    The table of a site: the distinct keys of its entries, each with its count, ordered by count descending, ties by
 *    key ascending; alleles [al_begin[k], al_begin[k + 1]).  The counts add up to the site's depth, the sum of its six
 *    counters.  ent_allele[e] is the index of entry e's key within its site's table, e in the order of
 *    dagcon_fetch_site_reads' entries.  With phase on at the upload each allele also has c1, c2, c0: its entries whose
 *    alignment has hap 1, 2, 0; c1 + c2 + c0 == count.  A failed target has no alleles and no entries.
 * dagcon_set_site_alleles: the switch is read at the upload; without dagcon_set_pileup and dagcon_set_site_reads on at
 * the same upload it is as if off.  With it off no kernel, buffer, memset, launch or copy differs from a context that
 * never heard of it.  With it on, the kernels of csrc/k_alleles.hip.h run behind those of the site reads (the counts per
 * label behind the split) in every execution of the run; they need no arena of their own: the entries of a site number
 * its depth, and a table is no longer than that.  The arrays stay on the device and are copied only when
 * dagcon_fetch_site_alleles is called (the tables are gathered into arrays of their own size by one more kernel then:
 * 16 bytes an allele; a run holds 20 bytes an entry and 28 a site), which converts them as dagcon_fetch_site_reads converts its own (it calls it):
 * the sites are those of dagcon_fetch_pileup_sites in their order, the entries those of dagcon_fetch_site_reads in
 * theirs.  DAGCON_ERR_STATE wherever dagcon_fetch_site_reads is, and when the switch was off at the upload; the derived
 * batch of dagcon_upload_haps has it off.  Owned by the context, valid as long as the results of the same fetch.
 * dagcon_allele_text: host only, needs no device and no context; cap counts the terminating 0 (22 bytes hold every key).
 * DAGCON_ERR_INVALID_ARG for a buffer too small and for an integer that is no key.
 */
typedef struct dagcon_site_alleles {
    uint64_t n_sites;                 /* the sites of dagcon_fetch_pileup_sites, same order */
    const uint64_t *al_begin;         /* [n_sites + 1] */
    const uint64_t *key;              /* [n] */
    const uint32_t *count;            /* [n] */
    const uint16_t *hap_count;        /* [3 n]: c1 c2 c0; NULL when phase was off */
    uint64_t n_ent;                   /* the entries of dagcon_fetch_site_reads, same order */
    const uint16_t *ent_allele;       /* [n_ent] index within the entry's site */
} dagcon_site_alleles;
int dagcon_set_site_alleles(dagcon_ctx *ctx, int on);
int dagcon_fetch_site_alleles(dagcon_ctx *ctx, dagcon_site_alleles *out);
int dagcon_allele_text(uint64_t key, char *out, size_t cap);   /* host only; needs no device */

/*
 * Joined sites: adjacent sites of the pile-up joined into runs, and per run what its alignments show at all of its sites
 * at once (off by default; a context switch that needs dagcon_set_pileup, dagcon_set_site_reads and
 * dagcon_set_site_alleles on at the same upload).  The tables of rule 8 keep every position on its own: a deletion of
 * three bases is three sites with the empty allele, and two neighbouring substitutions no longer say whether the same
 * alignments carry both.  This is this build's own rule, PARITY UNPINNED, in the terms of rules 1 to 8 above.
 * 10. 10.1 Runs.  Take the sites in the order of dagcon_fetch_pileup_sites.  Site k > 0 CONTINUES site k - 1 iff both have
 *          the same target and pos[k] == pos[k - 1] + 1.  A maximal chain of continuing sites is a stretch.  A stretch is
 *          cut, from its first site, into runs of at most DG_JN_SITES = 16 sites: site k is a run head iff it does not
 *          continue, or (k - first site of its stretch) % 16 == 0.  Every site lies in exactly one run; run r holds the
 *          sites [run_begin[r], run_begin[r + 1]), m is its length.  The last position of one target and position 0 of
 *          the next are never joined.
 *     10.2 Members.  Alignment x SPANS run r iff it has an entry (rule 2) at every site of r; it is a PARTIAL member iff
 *          it has an entry at at least one site of r but not at all of them.  spanning[r] and partial[r] count the two
 *          kinds.  An alignment's target columns are consecutive positions, so its entries are consecutive sites.  For
 *          every site k of r: depth(k) = spanning[r] + the partial members with an entry at k.
 *     10.3 The joined key of a spanning member is a 64-bit integer.  Let a_j be ent_allele of its entry at the run's j-th
 *          site, the index in that site's table (rule 8), and c_j = min(a_j, 15).  Then key = the sum over j < m of
 *          c_j << (4 * (15 - j)); the unused low nibbles are 0.  Nibble 15 means "allele 15 or later of that site's
 *          table": such alleles COUNT AS ONE, as long alleles do in rule 8.
 *     10.4 The table of a run: the distinct keys of its spanning members, each with its count, ordered by count
 *          descending, ties by key ascending (unsigned); joined alleles [jal_begin[r], jal_begin[r + 1]).  The counts add
 *          up to spanning[r].  With phase on at the upload each joined allele also has c1, c2, c0 by hap of the alignment;
 *          c1 + c2 + c0 == count.  ent_joined[e], one value per entry in the order of dagcon_fetch_site_reads, is the
 *          index of the alignment's key in the table of the run that holds the entry's site, or 0xFFFF for a partial
 *          member; all m entries of a spanning member carry the same value.  A failed target has no runs.
 *     10.5 Text (host only; the command line's, csrc/host/joined.h).  A joined allele's bases are the texts of its sites'
 *          alleles one after the other (dagcon_allele_text without "-"), or "-" when all are empty.  The allele is OPAQUE
 *          and prints "*" when a nibble is 15 or a site's allele is long.
 *     Nothing in the rule depends on an order.
 * dagcon_set_site_join: the switch is read at the upload; without the three switches it rests on on at the same upload it
 * is as if off.  With it off no kernel, buffer, memset, launch or copy differs from a context that never heard of it.
 * With it on, the kernels of csrc/k_join.hip.h run behind those of the alleles in every execution of the run; they need
 * no arena of their own: the spanning members of a run number at most the depth of its first site, and a table is no
 * longer than that (a run holds 20 bytes an entry and 36 a site more).  The arrays stay on the device and are copied only
 * when dagcon_fetch_joined_sites is called (the tables are gathered by one more kernel then: 16 bytes a joined allele),
 * which converts them as dagcon_fetch_site_alleles converts its own (it calls it).  DAGCON_ERR_STATE wherever
 * dagcon_fetch_site_alleles is, and when the switch was off at the upload; the derived batch of dagcon_upload_haps has it
 * off.  Owned by the context, valid as long as the results of the same fetch.
 */
#define DG_JN_SITES 16u
typedef struct dagcon_joined_sites {
    uint64_t n_runs;
    const uint64_t *run_begin;   /* [n_runs + 1] into the sites of dagcon_fetch_pileup_sites */
    const uint32_t *spanning;    /* [n_runs] */
    const uint32_t *partial;     /* [n_runs] */
    const uint64_t *jal_begin;   /* [n_runs + 1] */
    const uint64_t *key;         /* [n] */
    const uint32_t *count;       /* [n] */
    const uint16_t *hap_count;   /* [3 n] c1 c2 c0; NULL when phase was off */
    uint64_t n_ent;              /* the entries of dagcon_fetch_site_reads, same order */
    const uint16_t *ent_joined;  /* [n_ent] index within the table of the entry's run; 0xFFFF: a partial member */
} dagcon_joined_sites;
int dagcon_set_site_join(dagcon_ctx *ctx, int on);
int dagcon_fetch_joined_sites(dagcon_ctx *ctx, dagcon_joined_sites *out);

/*
 * Phase across windows: the read labels of neighbouring windows joined into blocks (off by default; a context switch that
 * needs a windows upload with dagcon_set_pileup and dagcon_set_site_reads with phase != 0 on at the same upload).  Rule 4
 * labels every window on its own: the seed of a window is label 1, so label 1 of one window and label 1 of the next are
 * unrelated names.  A record that crosses a window boundary has a piece in both windows, and both pieces have a label.
 * This is this build's own rule, PARITY UNPINNED, in the terms of rules 1 to 4 of the site reads above.
 * 9. Given W windows (target[] ascending, begin[] ascending inside a target):
 *    9.1 Predecessor.  Window w has the predecessor w - 1 iff w > 0 and target[w] == target[w - 1].
 *    9.2 Pair counts.  For a window w with a predecessor, over the records that have a taken alignment (rule 1) in both
 *        w - 1 and w with hap != 0 in both: same[w] counts those whose two labels are equal, diff[w] those whose labels
 *        differ.  Without a predecessor both are 0.  A record has at most one piece per window, so nothing is counted
 *        twice.  A failed window, a window below min_cov and a window without an informative site have no labelled
 *        alignments: they link to nothing on either side.
 *    9.3 Link.  hi = max(same, diff), lo = min(same, diff).  Window w is linked to its predecessor iff hi >= min_links
 *        and hi > lo and lo * 1000000 <= max_conflict_ppm * (hi + lo), in 64-bit integers.  min_links == 0 means the
 *        default 3 (the reasoning of min_reads in rule 6: the least that outvotes one error), max_conflict_ppm == 0 the
 *        default 250000; both defaults are this build's own choice.
 *    9.4 Orientation and blocks.  An unlinked window has flip[w] = 0 and block[w] = w.  A linked window has
 *        flip[w] = flip[w - 1] ^ (diff[w] > same[w]) and block[w] = block[w - 1].  A block is a maximal run of linked
 *        windows; its id is the index of its first window.
 *    9.5 Oriented labels.  hap[x] is the site reads' hap[x] when that is 0 or flip of its window is 0, else 3 - hap[x];
 *        phase[k] is the site reads' phase[k], negated when flip of the site's window is 1.  x is in the order of
 *        dagcon_fetch_site_reads, k in the order of dagcon_fetch_pileup_sites.  The arrays of dagcon_fetch_site_reads,
 *        dagcon_fetch_hap_tally and dagcon_fetch_site_alleles stay per window.
 *    Nothing in the rule depends on an order.
 * dagcon_set_window_phase: NULL turns it off; max_conflict_ppm > 1000000 is DAGCON_ERR_INVALID_ARG (the switch stays as it
 * was).  The switch is read at the upload and takes effect for an upload with windows, by any of the window entry points
 * (dagcon_upload_cigar_windows, _packed, _strand, _cs, _md with windows != NULL), made with the pile-up and the site reads
 * with phase != 0 on.  In every other case it is as if off: no kernel, buffer, memset, launch or copy differs from a
 * context that never heard of it, and dagcon_fetch_window_phase is DAGCON_ERR_STATE; the same wherever
 * dagcon_fetch_site_reads is.  The derived batch of dagcon_upload_haps has it off.  With it on, the host uploads 4 bytes an
 * alignment (its record) and 4 a window (its target), and the kernels of csrc/k_winlink.hip.h run right behind the split in
 * every execution of the run.  The arrays stay on the device and are copied only when dagcon_fetch_window_phase is called,
 * which converts them as dagcon_fetch_site_reads converts its own (it calls it).  Owned by the context, valid as long as
 * the results of the same fetch.
 */
typedef struct dagcon_window_phase_opts { uint32_t min_links, max_conflict_ppm; } dagcon_window_phase_opts;   /* 0, 0: the defaults 3 and 250000 */
int dagcon_set_window_phase(dagcon_ctx *ctx, const dagcon_window_phase_opts *o);   /* NULL: off (the default) */
typedef struct dagcon_window_phase {
    uint32_t n_windows; const uint32_t *same, *diff, *block; const uint8_t *flip;   /* [n_windows] */
    uint64_t n_aln;   const uint8_t *hap;     /* oriented; the alignments of dagcon_fetch_site_reads, same order */
    uint64_t n_sites; const int8_t *phase;    /* oriented; the sites of dagcon_fetch_pileup_sites, same order */
} dagcon_window_phase;
int dagcon_fetch_window_phase(dagcon_ctx *ctx, dagcon_window_phase *out);

/*
 * Hap calls: the edits of the two groups of a split target against their common target, and for every edit whether the
 * other group carries it too (off by default; a context switch that needs dagcon_set_edits on).  The consensus of a group
 * is the evidence: no likelihood, no limit on an allele's length.
 * THIS BUILD'S OWN RULE, PARITY UNPINNED (the reference has no such output; tests/hap_calls_twin.py is its twin).
 * 11. The derived targets of dagcon_upload_haps come in pairs: label 1 at an even d, label 2 at d ^ 1, both with the source
 *     target src_target[d] (dagcon_fetch_hap_map).  With the switch in effect the derived batch reports its edits
 *     (dagcon_fetch_edits, dagcon_fetch_positions; dagcon_fetch_edit_support iff the first batch ran with it) by the rules
 *     of those fetches word for word, "target" read as "the source target (window) of the derived target": the edits
 *     INVARIANT holds against the source target's bytes, and the support counts are over the group's alignments (the
 *     unlabelled reads are in both groups, so the two groups' span may add up to more than the target's depth).
 *     For an edit e = (t_pos, t_len, alt = seq_blob[c_off, c_off + c_len)) of derived target d, with d' = d ^ 1:
 *     Occupied interval: o(e) = [t_pos, t_pos + max(t_len, 1)); a pure insertion occupies the base behind it.  Inside one
 *     derived target the occupied intervals are disjoint and t_pos rises strictly over all of its segments (one edit per
 *     gap between consecutive backbone bases, segments cut from one best path).
 *     HOM (3):     d' has an edit with the same t_pos, t_len, c_len and the same alt bytes (exact bytes: case counts, as in
 *                  the edits' trim); mate[e] is that edit.
 *     CLASH (2):   otherwise, d' has an edit e' with o(e) and o(e') not disjoint; mate[e] is the lowest such e'.  (An
 *                  insertion at p clashes with a substitution of [p, p + 1); substitutions of [p, p + 1) and
 *                  [p + 1, p + 2) do not clash.)
 *     HET (1):     otherwise, some segment of d' has t0' <= t_pos and t_pos + t_len <= t1': the partner's consensus is
 *                  there and shows the target; mate = none.
 *     NOCOVER (0): otherwise; all edits of a target whose partner failed (target_status != DAGCON_OK) or has no segment;
 *                  mate = none.
 *     HOM is tested first, then CLASH, then the cover.  HOM and CLASH are symmetric: mate[mate[e]] == e for HOM, and the
 *     mate of a CLASH is itself CLASH.  Nothing in the rule depends on an order.
 * dagcon_set_hap_calls: DAGCON_ERR_STATE unless dagcon_set_edits is on; turning the edits off turns it off.  The switch is
 * read at dagcon_upload_haps and takes effect only when the first batch was a record upload (whole targets or windows) that
 * ran with the edits.  In every other case (a string or dagcon_consensus_pre first batch, edits off at the first upload,
 * the switch off) it is as if off: the derived batch runs with no optional output, exactly as described above, and no
 * kernel, buffer, memset, launch or copy differs.  In effect, dagcon_upload_haps uploads 8 bytes a derived target (where
 * its source target's bases lie in the record intake's target blob, which is still on the device) and k_hap_calls
 * (csrc/k_hap_calls.hip.h) runs behind the edit kernels in every execution of the run.
 * dagcon_fetch_hap_calls: the arrays (9 bytes an edit) are copied when it is called and brought from the device's edit
 * order to that of dagcon_fetch_edits (failed targets drop out, mate is re-indexed).  A mate outside the partner's edits
 * or a state above 3 is DAGCON_ERR_INTERNAL.  DAGCON_ERR_STATE wherever dagcon_fetch_edits is, when the switch did not take
 * effect at dagcon_upload_haps, before the derived batch's dagcon_fetch, and after any later upload.  A derived batch of 0
 * targets has n == 0.  Owned by the context, valid as long as the results of the same fetch.
 */
#define DAGCON_HC_NOCOVER 0
#define DAGCON_HC_HET     1
#define DAGCON_HC_CLASH   2
#define DAGCON_HC_HOM     3
int dagcon_set_hap_calls(dagcon_ctx *ctx, int on);
typedef struct dagcon_hap_calls {
    uint64_t n;              /* == dagcon_edits.n of the same fetch, same order */
    const uint8_t  *state;   /* [n] DAGCON_HC_* */
    const uint64_t *mate;    /* [n] index into the same arrays; UINT64_MAX: none */
} dagcon_hap_calls;
int dagcon_fetch_hap_calls(dagcon_ctx *ctx, dagcon_hap_calls *out);

/*
 * The groups in the caller's orientation (host only).  dagcon_upload_haps names the groups of a split target by the labels
 * of that target alone (rule 4: the seed is label 1).  A caller that has joined the labels of neighbouring windows (rule 9:
 * flip, and whatever it links across its own uploads) says which targets carry the other naming:
 * dagcon_upload_haps_swapped is dagcon_upload_haps in everything -- when it is valid, what it uploads, what it leaves --
 * but for this: for a split target t with swap[t] != 0 the two groups change names.  The derived target with label 1 holds
 * the target's alignments whose hap is 2 or 0, the one with label 2 those whose hap is 1 or 0 (rule 7 otherwise).  Pairs
 * stay at d, d ^ 1, label 1 first; dagcon_hap_map.label is the caller's name after the swap, aln_src keeps its meaning; rule
 * 11 holds unchanged on the pairs.  swap has one byte per target of the first batch; NULL swaps nothing, and
 * dagcon_upload_haps is this call with NULL.
 */
int dagcon_upload_haps_swapped(dagcon_ctx *ctx, const uint8_t *swap);   /* swap: [n_targets of the first batch], or NULL */

/*
 * The kept part of every segment of a window, cut on the device (off by default; a context switch that needs
 * DAGCON_FLAG_BASE_POS).  A window is consensus'd with an overlap on either side, and a stitch keeps of each segment the
 * part inside the window's core.  Finding that part from dagcon_fetch_positions costs 4 bytes a base across the bus and a
 * walk over every base on the host; the device finds it while the positions are still in HBM and hands back 16 bytes a
 * segment.
 * THIS BUILD'S OWN RULE, PARITY UNPINNED (the reference has no windows; tests/hap_contigs_twin.py: keep is its twin).
 * 12. Given lo[t] <= hi[t] per target (window) t.  Take a segment of n bases on target t; P(i) is the value
 *     dagcon_fetch_positions gives for its base i, 1-based and relative to the window.
 *     i0 is the least i with P(i) > lo[t].  i1 is the least i >= i0 with P(i) > hi[t], or n if there is none.  Only first
 *     crossings count and nothing assumes that P is monotone: a base in front of i0 with P > hi does not count.
 *     The kept part is [i0, i1), with p_first = P(i0) and p_last = P(i1 - 1).  It is empty when no i0 exists or when
 *     i1 == i0; the record is then 0 0 0 0.
 *     With lo = core begin - window begin and hi = core end - window begin this is the cut a stitch of overlapping
 *     windows makes: "cut at the core begin" is i0 > 0, "cut at the core end" is i1 < n.
 * dagcon_set_window_keep: the arrays are copied by the call; NULL turns it off.  DAGCON_ERR_STATE on a context without
 * DAGCON_FLAG_BASE_POS; lo[t] > hi[t] is DAGCON_ERR_INVALID_ARG and the switch stays as it was.  The switch is read at two
 * points: at a windows upload, by any of the window entry points, and at dagcon_upload_haps / _swapped behind a windows
 * upload, where derived target d takes lo / hi of src_target[d].  At both points n must equal the number of windows of the
 * first batch: otherwise the upload returns DAGCON_ERR_INVALID_ARG before any launch (and leaves the context as any failed
 * upload does).  In every other case it is as if off: no kernel, buffer, memset, launch or copy differs from a context
 * that never heard of it.  In effect, the host uploads 8 bytes a target and k_win_keep (csrc/k_keep.hip.h) runs behind
 * k_bp_join (behind the edit kernels where those run) in every execution of the run, re-runs included; and, as with the
 * edits, the positions stay on the device and are copied only when dagcon_fetch_positions is called.
 * dagcon_fetch_window_keep: the records (16 bytes a segment) are copied when it is called and brought from the device's
 * segment order to that of dagcon_results, as dagcon_fetch_edits does for its arrays: a failed target has no segments and
 * so no records.  DAGCON_ERR_STATE wherever dagcon_fetch_positions is, when the switch did not take effect at the upload,
 * before the batch's dagcon_fetch, and after any later upload.  Owned by the context, valid as long as the results of the
 * same fetch.
 */
typedef struct dagcon_window_keep_opts { uint32_t n; const uint32_t *lo, *hi; } dagcon_window_keep_opts;   /* copied by the call */
int dagcon_set_window_keep(dagcon_ctx *ctx, const dagcon_window_keep_opts *o);    /* NULL: off (the default) */
typedef struct dagcon_window_keep {
    uint64_t n_segments;                              /* == dagcon_results.n_segments of the same fetch, same order */
    const uint32_t *i0, *i1, *p_first, *p_last;       /* [n_segments] */
} dagcon_window_keep;
int dagcon_fetch_window_keep(dagcon_ctx *ctx, dagcon_window_keep *out);

/*
 * Site link: which sites are carried by the same reads as other sites near them, chosen on the device in front of the
 * split (off by default; a context switch that needs dagcon_set_pileup and dagcon_set_site_reads with phase != 0 on at the
 * same upload).  At thresholds a noisy pile-up needs, most sites are the reads' own errors and outvote the few real ones
 * in rule 4; the reads that carry a real site's minor allele carry the minor allele of the real sites around it too, and
 * an error's do not.  THIS BUILD'S OWN RULE, PARITY UNPINNED, in the terms of rules 1 to 4 of the site reads
 * (tests/site_link_twin.py is its twin).  Everything is per target of the pipeline (with windows: per window).
 * 13. 13.1 For site k let P_k be the taken alignments with M(x, k) = +1 (rule 3) and M_k those with M(x, k) = -1.
 *     13.2 For two sites i != j of one target: pp = |P_i & P_j|, mm = |M_i & M_j|, pm = |P_i & M_j|, mp = |M_i & P_j|;
 *          same = pp + mm, diff = pm + mp, lo = min(same, diff), hi = max(same, diff); cell = min(pp, mm) if same >= diff,
 *          else min(pm, mp).  The two are PARTNERS iff lo * 1000000 <= max_conflict_ppm * (lo + hi) and cell >= min_cell,
 *          in 64-bit integers.  same == diff == 0 gives cell = 0: no partners.
 *     13.3 Only sites whose indices in the target's site list (ascending position, the order of
 *          dagcon_fetch_pileup_sites) differ by at most `reach` are compared.
 *     13.4 partners[k] is the number of partners of k; linked[k] = partners[k] >= min_partners.  A partner need not be
 *          linked itself.
 *     13.5 With the switch on, an entry at a site that is not linked has M = 0 in rule 4 (the split), in rule 6 (the
 *          tally), in rule 9 and in the label counts of rules 8 and 10: everywhere a sign is read.  The entries, the
 *          pile-up, the site list and the consensus do not change; a linked site keeps the sign of rule 3.
 *     13.6 Defaults: max_conflict_ppm 100000, min_cell 3, min_partners 2, reach 256; a 0 in a field means its default
 *          (1 ppm asks for no conflict at all).  They come from one experiment on synthetic reads (1 % substitutions,
 *          10 % inserted and 4 % deleted bases, 40 reads deep, planted sites 1,000 bases apart) and from nothing else.
 *     13.7 A failed target (target_status != DAGCON_OK) has no sites and so no entries in the arrays.
 * dagcon_set_site_link: NULL turns it off; reach > 4096 is DAGCON_ERR_INVALID_ARG (the switch stays as it was).  The
 * switch is read at the upload, whichever entry point makes it.  With any of the three switches off at the upload, or phase
 * == 0, no kernel, buffer, memset, launch or copy differs from a context that never heard of it (k_sr_split tests one kernel
 * argument, NULL then), and dagcon_fetch_site_link is DAGCON_ERR_STATE; the same before a dagcon_fetch, under
 * DAGCON_FLAG_STOP_AFTER_BUILD / _MERGE and for the derived batch of dagcon_upload_haps.  With all on, the kernels of
 * csrc/k_site_link.hip.h run between k_sr_walk and k_sr_split in every execution of the run, re-runs included; two bit
 * rows a site ((deepest target's alignments + 63) / 64 words each) grow with the site arena.
 * dagcon_fetch_site_link: 3 bytes a site, copied when it is called; the sites are those of dagcon_fetch_pileup_sites in
 * their order.  Owned by the context, valid as long as the results of the same fetch.
 */
typedef struct dagcon_site_link_opts { uint32_t max_conflict_ppm, min_cell, min_partners, reach; } dagcon_site_link_opts;   /* 0: that field's default */
int dagcon_set_site_link(dagcon_ctx *ctx, const dagcon_site_link_opts *o);    /* NULL: off (the default) */
typedef struct dagcon_site_link {
    uint64_t n_sites;                                 /* the sites of dagcon_fetch_pileup_sites, same order */
    const uint16_t *partners; const uint8_t *linked;  /* [n_sites] */
} dagcon_site_link;
int dagcon_fetch_site_link(dagcon_ctx *ctx, dagcon_site_link *out);

/*
 * Page-locked host memory for the input blobs (qstr / tstr / backbone): a caller that parses
 * alignment records straight into such a buffer gets its dagcon_upload at link speed instead of
 * through the driver's staging copies.  Optional: any host memory is accepted by dagcon_upload.
 */
int  dagcon_host_alloc(dagcon_ctx *ctx, size_t bytes, void **out);
void dagcon_host_free(dagcon_ctx *ctx, void *p);

/*
 * Unit-level entry point for stage a1 alone: normalizeGaps (Alignment.cpp:
 * 131-217) followed by trimAln (Alignment.cpp:219-242) on n alignments, on
 * the device.  Inputs use the batch blob layout; outputs are written into
 * qout/tout at out_off[a] (capacity 2*aln_len[a] each), with out_len[a] and
 * the trimmed start in out_start[a].  trim = 0 gives normalizeGaps alone;
 * flags = DAGCON_FLAG_RAW_ALIGNMENTS gives trimAln alone (strings as given).
 */
int dagcon_normalize(dagcon_ctx *ctx, uint32_t n, const uint32_t *aln_start,
                     const uint64_t *aln_off, const uint32_t *aln_len,
                     const char *qstr, const char *tstr, uint64_t blob_bytes,
                     uint32_t trim, uint32_t flags, const uint64_t *out_off, char *qout, char *tout,
                     uint32_t *out_len, uint32_t *out_start);

/*
 * The `-a` stage (main.cpp:127-128, SimpleAligner.cpp:25-63): re-aligns n (query, target) pairs of
 * UNALIGNED sequences, as the .pre format carries them (Alignment.cpp:82-112), on the device.
 * Pair a is q_blob[q_off[a] .. +q_len[a]) against t_blob[t_off[a] .. +t_len[a]).  The aligned strings
 * (equal lengths, '-' for gaps) are written to qaln / taln at out_off[a] (room for q_len[a] + t_len[a]
 * columns each), their length to aln_len[a].  By default the alignment is global: in the terms of
 * SimpleAligner.cpp:52-53 GenomicTBegin() = 0 and GenomicTEnd() = t_len[a]; the caller applies
 * SimpleAligner.cpp:51-62 (start / end / reverse complement) itself.
 * blasr_libcpp is not in the reference tree: this stage is pinned to the reference only by its one
 * known-answer test (test/cpp/SimpleAlignerTest.cpp:8-21); everything else is parity-unpinned.
 *
 * Local ends (a context created with DAGCON_FLAG_LOCAL_ALIGN), the reference's SDPAlign(..., Local) in this
 * build's own definition, pinned by the same one known-answer test (which it reproduces with ends 0, 61, 0, 61)
 * and unpinned beyond it.  Same scores, same bands and passes; only the ends change:
 *   - every cell is computed as above (diagonal, insertion, deletion, each only when strictly better); a score
 *     above 0 becomes 0 with "the alignment starts here", so do all cells of row 0;
 *   - the alignment ends at the cell with the smallest score over all rows of the band, a tie going to the larger
 *     i, then the larger j; no cell below 0: no local alignment;
 *   - it runs back from there to a start cell, giving the half-open ends q[q_begin, q_end) and t[t_begin, t_end)
 *     (dagcon_align_ends); the aligned strings cover only those, as CreateAlignmentStrings does;
 *   - a pass stands unless its path comes within 8 cells of an edge of its band or it finds no local alignment;
 *     a pair the last pass finds none for comes back with length 0 and ends 0, 0, 0, 0 and counts in
 *     dagcon_align_dropped.
 * The band is centred as for the global alignment (on j = i * t_len / q_len), so the local ends are found inside it:
 * flanks that move the aligned core off that diagonal by more than the band's half-width put it out of reach, as
 * they do for the global alignment.
 */
int dagcon_align(dagcon_ctx *ctx, uint32_t n, const uint64_t *q_off, const uint32_t *q_len,
                 const uint64_t *t_off, const uint32_t *t_len, const char *q_blob, uint64_t q_bytes,
                 const char *t_blob, uint64_t t_bytes, const uint64_t *out_off, char *qaln, char *taln,
                 uint32_t *aln_len);

/*
 * dazcon --trace-panels: n overlaps of a .las re-aligned inside their trace-point panels, as the reference's
 * Compute_Trace_PTS does (DazAlnProvider.cpp:304-351).  Pair a is q_blob[q_off[a] .. +q_len[a]) (the B interval)
 * against t_blob[t_off[a] .. +t_len[a]) (the A interval), cut into the panels p in [panel_begin[a], panel_begin[a+1]):
 * panel p takes the next panel_t_len[p] bases of t and panel_q_len[p] bases of q.  Each panel is aligned on its own,
 * a unit-cost edit distance with both corners fixed, ties broken per cell diagonal first, then a q base against a gap
 * in t, then a t base against a gap in q; the pair's alignment is its panels' concatenated, written as dagcon_align
 * writes it (qaln / taln at out_off[a], room for q_len[a] + t_len[a] columns, '-' for gaps; length in aln_len[a]).
 * panel_dist (optional) receives each panel's edit distance, -1 for the panels of a pair that was not aligned.
 * A pair with a panel wider or longer than DAGCON_PANEL_MAX_SIDE bases is not aligned: aln_len 0, counted by
 * dagcon_align_dropped.  DAGCON_ERR_INVALID_ARG when a pair's panels do not add up to its t_len / q_len.
 * DALIGNER is not in the reference tree: PARITY UNPINNED, the tie-breaks are this build's own.
 */
#define DAGCON_PANEL_MAX_SIDE 512u
int dagcon_align_panels(dagcon_ctx *ctx, uint32_t n,
                        const uint64_t *q_off, const uint32_t *q_len,
                        const uint64_t *t_off, const uint32_t *t_len,
                        const char *q_blob, uint64_t q_bytes, const char *t_blob, uint64_t t_bytes,
                        const uint64_t *panel_begin,   /* [n + 1] */
                        const uint32_t *panel_t_len,   /* [panel_begin[n]] A bases per panel */
                        const uint32_t *panel_q_len,   /* [panel_begin[n]] B bases per panel */
                        const uint64_t *out_off, char *qaln, char *taln, uint32_t *aln_len,
                        int32_t *panel_dist);          /* [panel_begin[n]] edit distance per panel, or NULL */

/*
 * What main.cpp:117-145 does with -a, in one call: the records of a batch of targets as the .pre format carries
 * them (Alignment.cpp:82-112: tstart is Alignment::start as parsePre leaves it, q / t the unaligned sequences) are
 * re-aligned as by dagcon_align, start / end / strand handled as SimpleAligner.cpp:51-62 does (start = tstart,
 * end = start + t_len; '-': start = tlen - end and both strings reverse-complemented; start += 1), then
 * filtered, normalised, trimmed and threaded as by dagcon_consensus.  The aligned strings stay on the device.
 * Same parity statement as dagcon_align.  With DAGCON_FLAG_LOCAL_ALIGN: start = tstart + t_begin, end =
 * tstart + t_end, then the same '-' and += 1 steps.  This reads SimpleAligner.cpp:53's GenomicTEnd() as the aligned
 * target span (t_end - t_begin) added to the start :52 already moved, a reading blasr's Alignment (not in the tree)
 * cannot confirm; for global alignments and for the known-answer test it agrees with reading it as an absolute end.
 * A '-' record then lies on the forward backbone exactly where its aligned target bases do.  Records without a
 * local alignment (length 0) fall to the min_len filter.
 */
typedef struct dagcon_pre_batch {
    uint32_t n_targets;
    const uint32_t *tlen;        /* [n_targets] */
    const uint64_t *rec_begin;   /* [n_targets + 1]: records of target g are rec_begin[g] .. rec_begin[g + 1] - 1 */
    const uint32_t *tstart;      /* [n_rec] */
    const char *strand;          /* [n_rec] '+' or '-' */
    const uint64_t *q_off;       /* [n_rec] query sequence: q_blob[q_off .. + q_len) */
    const uint32_t *q_len;
    const uint64_t *t_off;       /* [n_rec] target sequence (in the read's orientation): t_blob[t_off .. + t_len) */
    const uint32_t *t_len;
    const char *q_blob;
    uint64_t q_bytes;
    const char *t_blob;
    uint64_t t_bytes;
} dagcon_pre_batch;
int dagcon_consensus_pre(dagcon_ctx *ctx, const dagcon_pre_batch *batch, dagcon_results *results);

/*
 * Alignments as current aligners write them (SAM): one ungapped read, a position and a CIGAR per record, against
 * target bases that are held once per target.  The records are expanded into the pair of gapped strings of
 * dagcon_batch on the device and then take the path of dagcon_consensus: the result is, byte for byte, that of
 * dagcon_consensus on the expanded strings.  The strings never exist on the host.  Expansion of one record, with
 * q its read bases, t its target's bases, qi = 0 and ti = pos - 1:
 *   M, =, X of length L:  L columns (q[qi++], t[ti++]);
 *   I:                    L columns (q[qi++], '-');
 *   D:                    L columns ('-', t[ti++]);
 *   S:                    qi += L, no column;        H, P: nothing.
 * Bytes are copied verbatim (case, N, anything else).  aln_start = pos, aln_len = the number of columns.
 * A record is non-conforming when an op code is above 8 or is N (3), an op has length 0, the ops do not consume
 * exactly q_len read bases, pos == 0, pos - 1 + the target bases consumed > tlen, or one of its three totals
 * (columns, read bases, target bases) does not fit 32 bits.  Its target gets target_status =
 * DAGCON_ERR_NONCONFORMING and no segments whatever its coverage; the rest of the batch is complete and exact, as
 * dagcon_consensus confines a failure.  A sequence that runs past its blob (t_off + tlen > t_bytes, q_off + q_len >
 * q_bytes) or a rec_begin / op_begin that is not monotone is DAGCON_ERR_INVALID_ARG for the call, found on the host
 * before anything is launched.  After the expansion everything is dagcon_consensus: min_cov counts the records of a
 * target, min_len the columns of a record, then normalizeGaps, trimAln, an 'N' backbone filled in by the reads
 * (t_blob feeds the tstr side only; consensus on the real backbone is not offered here).  All flags keep their
 * meaning (RAW_ALIGNMENTS, STOP_AFTER_*, BASE_SUPPORT with dagcon_fetch_support); LOCAL_ALIGN is ignored as
 * dagcon_consensus ignores it.
 */
typedef struct dagcon_cigar_batch {
    uint32_t n_targets;
    const uint32_t *tlen;        /* [n_targets] */
    const uint64_t *t_off;       /* [n_targets] target bases: t_blob[t_off .. + tlen) */
    const char *t_blob;
    uint64_t t_bytes;
    const uint64_t *rec_begin;   /* [n_targets + 1] records of target g, in addAln order */
    const uint32_t *pos;         /* [n_rec] 1-based leftmost target base (SAM POS) = Alignment::start */
    const uint64_t *q_off;       /* [n_rec] read bases as SAM SEQ has them (target orientation); the ranges of several */
                                 /*         records may overlap or coincide (one read, many alignments)               */
    const uint32_t *q_len;
    const char *q_blob;
    uint64_t q_bytes;
    const uint64_t *op_begin;    /* [n_rec + 1] into ops */
    const uint32_t *ops;         /* BAM encoding: len << 4 | op, op 0..8 = M I D N S H P = X */
} dagcon_cigar_batch;
int dagcon_upload_cigar(dagcon_ctx *ctx, const dagcon_cigar_batch *batch);   /* then dagcon_run / _sync / _fetch as ever */
int dagcon_consensus_cigar(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, dagcon_results *results);

/*
 * The same input with its targets cut into windows, for targets of any length and depth (a contig and the reads mapped
 * to it): every window is one target of the pipeline, results.n_targets == n_windows, tlen = end - begin, and the
 * records are cut to the windows they cross on the device.  This build's own definition.  A record covers target bases
 * [s, e), s = pos - 1, e = s + the target bases its ops consume.  For a window [a, b), A = max(a, s), B = min(b, e):
 *   - A >= B: the record has no piece in the window;
 *   - F(x) is the index of the first column of the record's expansion (the rule above) that consumes target base x,
 *     F(s) := 0 and F(e) := the number of columns, so a record's own leading and trailing insertions stay with it;
 *   - the piece is columns [F(A), F(B)) with aln_start = A - a + 1: insertions in front of a cut at A > s are left out,
 *     insertions in front of B < e are kept, so windows that tile a target partition a record's columns;
 *   - pieces of a window keep the order of their records (addAln order).
 * After the cut everything is dagcon_consensus: min_cov counts a window's pieces, min_len a piece's columns, then
 * normalizeGaps, trimAln and an 'N' backbone; all flags keep their meaning.  Per window the result is, byte for byte,
 * that of dagcon_consensus on the piece strings.  With DAGCON_FLAG_BASE_POS a caller joins neighbouring windows at a
 * target coordinate (position + begin); pbdagcon --sam --window does (csrc/host/windows.h).
 * Conformance as for dagcon_consensus_cigar; a non-conforming record fails every window it has a piece in
 * (target_status DAGCON_ERR_NONCONFORMING), the other windows are complete.  The span of a non-conforming record is
 * s = max(pos, 1) - 1 and e = s + its target-base total (32 bits), then s <= tlen - 1 and s + 1 <= e <= tlen.
 * DAGCON_ERR_INVALID_ARG before any launch: end <= begin, end > tlen, a target index out of range, windows out of order.
 * A window longer than the tlen limit of dagcon_consensus or with more than DAGCON_MAX_COVERAGE pieces (after the pick
 * of dagcon_set_record_filter, when a filter is set): DAGCON_ERR_UNSUPPORTED for the call, as there.
 */
typedef struct dagcon_windows {
    uint32_t n_windows;
    const uint32_t *target;   /* [n_windows] index into the cigar batch's targets, ascending */
    const uint32_t *begin;    /* [n_windows] 0-based, half-open [begin, end) in target bases; */
    const uint32_t *end;      /*             ascending begin within a target; windows may overlap */
} dagcon_windows;
int dagcon_upload_cigar_windows(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows);
int dagcon_consensus_cigar_windows(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows,
                                   dagcon_results *results);

/*
 * dagcon_cigar_batch with q_blob in BAM's 4-bit encoding, as a BAM record's seq field has it: q_off[r] is the BYTE
 * offset of record r's first base (every record starts on a byte, as in a BAM record), q_len[r] still counts bases,
 * q_bytes is the size of the packed blob.  Base i of a record is nibble i from q_off: byte i >> 1, the high nibble for
 * even i, decoded by BAM's table "=ACMGRSVTWYHKDBN" on the device (code 0 is the byte '=', copied like any other byte,
 * as the SAM line printed from the record would carry it).  windows may be NULL (then: dagcon_upload_cigar /
 * dagcon_consensus_cigar, else dagcon_upload_cigar_windows / dagcon_consensus_cigar_windows).  t_blob stays one byte a
 * base.  The result is, byte for byte, that of the unpacked call on the same batch with every read decoded to one
 * byte a base by the table: segments, target_status, dagcon_fetch_support, dagcon_fetch_positions, the counts in the
 * timings.  Conformance, confinement of a failure, flags and limits are those of the unpacked calls; the only new
 * refusal is DAGCON_ERR_INVALID_ARG, before any launch, for q_off + (q_len + 1) / 2 > q_bytes.  Letter case is not
 * representable (BAM has none).  The unused low nibble of an odd-length record is ignored, whatever it holds.
 */
int dagcon_upload_cigar_packed(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows);
int dagcon_consensus_cigar_packed(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows,
                                  dagcon_results *results);

/*
 * dagcon_cigar_batch with the read bases as a reads file has them and one strand flag per record (PAF: a line names a
 * slice [qs, qe) of a read that lies once in another file, and for a '-' line the CIGAR is written against the
 * reverse complement of that slice).  q_blob[q_off[r] .. + q_len[r]) is the slice as the file has it, one byte a base
 * (there is no packed form: a reads file is text).  For a record with reverse[r] != 0, read base i of the expansion
 * rule above is comp(q_blob[q_off[r] + q_len[r] - 1 - i]), formed on the device; comp swaps A<->T, C<->G, a<->t, c<->g
 * and leaves every other byte as it is.  (Alignment.cpp:15-26 complements upper case only; reads files carry
 * soft-masked lower case, and the reference reads no PAF: this rule is this build's own, parity unpinned.)
 * Several records may name overlapping or equal ranges of q_blob, on either strand.
 * windows may be NULL (then: dagcon_upload_cigar / dagcon_consensus_cigar, else the _windows calls).  reverse == NULL
 * is the unstranded call.  The result is, byte for byte, that of the unstranded call on the same batch with every
 * reverse record's bases replaced by their reverse complement: segments, target_status, dagcon_fetch_support,
 * dagcon_fetch_positions, the counts in the timings.  Conformance, confinement of a failure, flags, limits and the
 * DAGCON_ERR_INVALID_ARG checks are those of the unstranded calls.
 */
int dagcon_upload_cigar_strand(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows /* or NULL */,
                               const uint8_t *reverse /* [n_rec], or NULL */);
int dagcon_consensus_cigar_strand(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows,
                                  const uint8_t *reverse, dagcon_results *results);

/*
 * Alignments as minimap2 --cs writes them (PAF cs:Z:): the tag's text and the target are the whole alignment, there are
 * no read bases to hand over.  cs_blob[cs_off[r] .. + cs_len[r]) is the text behind "cs:Z:" as the file has it; it goes
 * to the device raw and is decoded there into the ops and the read bases of a dagcon_cigar_batch record (k_cs.hip.h),
 * which then take the path of dagcon_consensus_cigar (windows == NULL) or dagcon_consensus_cigar_windows.  Neither the
 * ops nor the read exist on the host.  The text is in target orientation: a '-' PAF line needs nothing done to it.
 * Decode rule (this build's own: the reference reads no PAF, parity unpinned):
 *   - a byte of  : * + - = ~  starts an op wherever it stands; the op's body runs to the next such byte or to the end
 *     of the text (tokenising is context-free);
 *   - :n     n = 1..9 decimal digits, 1 <= n < 2^28:  op '=' of length n, read bases = the target's bytes at those
 *            positions, verbatim (a soft-masked target passes through);
 *   - =SEQ   one or more ASCII letters:  op '=' of length |SEQ|, read bases SEQ upper-cased;
 *   - *tq    exactly two ASCII letters:  op 'X' of length 1, read base q upper-cased;
 *   - +SEQ   one or more ASCII letters:  op 'I' of length |SEQ|, read bases SEQ upper-cased;
 *   - -SEQ   one or more ASCII letters:  op 'D' of length |SEQ|, no read bases.
 *   Upper-cased: a..z lose the case bit, upper case stays.  The t of *tq and the body of -SEQ are not compared with
 *   the target: the target side always comes from t_blob, as in dagcon_consensus_cigar.  Neighbouring ops are not
 *   merged.
 * The result is, byte for byte, that of dagcon_consensus_cigar (or _windows) on the batch with these ops and these read
 * bases: segments, target_status, dagcon_fetch_support, dagcon_fetch_positions, the counts in the timings.
 * A record is non-conforming (target_status DAGCON_ERR_NONCONFORMING for its target, or for every window it touches;
 * the rest of the batch is complete and exact) when its text breaks the grammar -- a ~ op, a non-empty text whose
 * first byte starts no op, an empty body, a non-letter or a non-digit in a body, :0, more than 9 digits or a number of
 * 2^28 or more, a * body that is not two letters -- or when its read-base total != q_len, its target-base total !=
 * t_span (when t_span is given), or anything holds that makes a CIGAR record non-conforming (pos == 0, pos - 1 + target
 * bases > tlen, a total past 32 bits).  With windows, the span of a non-conforming record is that of the CIGAR calls
 * with its decoded target-base total; a record whose text breaks the grammar has no decoded totals: its total is
 * t_span when that is given, else 0 (the one base at pos).
 * DAGCON_ERR_INVALID_ARG before any launch: cs_off + cs_len > cs_bytes, t_off + tlen > t_bytes, a rec_begin that is not
 * monotone.  Windows errors, limits and flags are those of the CIGAR calls.
 */
typedef struct dagcon_cs_batch {
    uint32_t n_targets;
    const uint32_t *tlen;        /* [n_targets] */
    const uint64_t *t_off;       /* [n_targets] target bases: t_blob[t_off .. + tlen) */
    const char *t_blob;
    uint64_t t_bytes;
    const uint64_t *rec_begin;   /* [n_targets + 1] records of target g, in addAln order */
    const uint32_t *pos;         /* [n_rec] 1-based leftmost target base (PAF ts + 1) */
    const uint32_t *q_len;       /* [n_rec] read bases the record claims (PAF qe - qs) */
    const uint32_t *t_span;      /* [n_rec] target bases it claims (PAF te - ts), or NULL: not checked */
    const uint64_t *cs_off;      /* [n_rec] the text behind "cs:Z:": cs_blob[cs_off .. + cs_len) */
    const uint32_t *cs_len;
    const char *cs_blob;
    uint64_t cs_bytes;
} dagcon_cs_batch;
int dagcon_upload_cs(dagcon_ctx *ctx, const dagcon_cs_batch *batch, const dagcon_windows *windows /* or NULL */);
int dagcon_consensus_cs(dagcon_ctx *ctx, const dagcon_cs_batch *batch, const dagcon_windows *windows /* or NULL */,
                        dagcon_results *results);

/*
 * SAM / BAM records without target bases: a dagcon_cigar_batch (plain reads, or BAM-packed with packed != 0; there is no
 * stranded form) plus one MD:Z text per record.  With CIGAR and SEQ the tag spells every target base a record touches --
 * matches are the read's own bases, mismatches and deleted bases are letters of the text -- so the targets are rebuilt
 * on the device (k_md.hip.h) and the batch then takes the path of dagcon_consensus_cigar / _windows / _packed.
 * batch->t_blob is not read and may be NULL; tlen, t_off and t_bytes lay out a target blob T of t_bytes bytes that the
 * device makes.  md_blob[md_off[r] .. + md_len[r]) is the text behind "MD:Z:" as the file has it.
 * This build's own rule (the reference reads no SAM, parity unpinned):
 * Grammar: a text must match [0-9]+(([A-Za-z]|\^[A-Za-z]+)[0-9]+)* in full.
 *   - A number has 1 to 9 digits and a value below 2^28; 0 and leading zeros are fine.  A number n covers n target bases
 *     as matches.
 *   - A lone letter covers one target base and spells it (a mismatch).
 *   - The letters behind ^ each cover and spell one target base (deleted bases).  They run to the next digit, so ^AC0G is
 *     a deletion of 2 and then a mismatch.
 *   - Letters are stored verbatim; no case is changed.  Offset k of a covered base counts from the record's pos - 1.
 * A record is non-conforming when its text breaks the grammar (an empty text, a first byte that is no digit, ^ followed by
 * a digit or by the end, two letters in a row outside a deletion, any other byte, 10 digits, a value of 2^28 or more),
 * when the bases its text covers do not equal the target bases its CIGAR consumes, or when anything makes it
 * non-conforming for dagcon_consensus_cigar.  It fails its target, or with windows the windows its span meets, exactly as
 * there.  MD and CIGAR are not cross-checked beyond that total: a D op whose bases the text counts as matches deletes
 * whatever T holds there, and a letter under an M op is simply that position's target base.
 * T, from every conforming record of the batch, before dagcon_set_record_filter picks (a record the filter later drops
 * still contributes):
 *   1. a position spelled by a letter of any record holds that letter;
 *   2. otherwise a position under an M / = / X column of any record holds that column's read base, the byte the
 *      expansion would write (decoded from its nibble when the reads are packed);
 *   3. every other byte of the blob is 'N'.
 * There is a conflict when two records spell different letters at one position, or when two records give different read
 * bases at one position no record spells.  Then every record of that target becomes non-conforming ("its target's MD
 * tags disagree"; fate DAGCON_FATE_NONCONFORMING, counts 0): the target fails, or the windows those records meet; the
 * rest of the batch is exact.  A match under one record and a letter from another at the same position is no conflict:
 * the letter wins (step 1).  Whether a conflict exists does not depend on the order the device stores in, so the outcome
 * is deterministic.  The bytes of a failed target in T are unspecified.
 * The result is, byte for byte, that of dagcon_consensus_cigar / _windows / _packed on the same batch with t_blob = T:
 * segments, target_status, dagcon_fetch_support, dagcon_fetch_positions, dagcon_fetch_edits, dagcon_fetch_record_stats
 * and the counts in the timings.
 * DAGCON_ERR_INVALID_ARG before any launch: md NULL while the batch has records, md_off + md_len > md_bytes, target
 * ranges that are not ascending and disjoint (t_off[g] + tlen[g] <= t_off[g + 1]: two targets must not share bytes the
 * device writes), and everything the CIGAR calls refuse.
 * dagcon_fetch_md_targets gives T (t_bytes bytes, owned by the context) after such an upload until the next upload of any
 * kind; DAGCON_ERR_STATE otherwise.
 */
typedef struct dagcon_md_tags {
    const uint64_t *md_off;      /* [n_rec] the text behind "MD:Z:": md_blob[md_off .. + md_len) */
    const uint32_t *md_len;
    const char *md_blob;
    uint64_t md_bytes;
} dagcon_md_tags;
int dagcon_upload_cigar_md(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows /* or NULL */,
                           const dagcon_md_tags *md, int packed);
int dagcon_consensus_cigar_md(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows /* or NULL */,
                              const dagcon_md_tags *md, int packed, dagcon_results *results);
int dagcon_fetch_md_targets(dagcon_ctx *ctx, const char **t_blob, uint64_t *t_bytes);

/*
 * Picking the records (off by default).  The record calls above take every record the aligner wrote; with a filter set
 * on the context they rate every record on the device and leave some out before anything is built.  This build's own
 * rule, PARITY UNPINNED (the reference picks reads upstream, in m4topre.py and dazcon -m).  For a conforming record, over
 * the columns of its expansion (the rule of dagcon_cigar_batch):
 *   match     columns of an M, = or X op whose read byte and target byte are equal after clearing bit 0x20 of both.  The
 *             read byte is the one the expansion writes: decoded from its nibble for packed input, complemented for a
 *             reverse record, the decoded read for cs.  One rule for the three ops: an = or X op is not trusted, the
 *             bases decide.  BAM's '=' base is the byte '=' and matches only '=';
 *   mismatch  the other M / = / X columns;
 *   ins, del  the bases of I ops, of D ops.  S, H and P count nowhere: match + mismatch + ins + del == the columns.
 * err = mismatch + ins + del.  A record passes max_error_ppm iff err * 1000000 <= max_error_ppm * columns, in 64-bit
 * integers; a record of 0 columns passes.  Then max_depth D (0: off), on a target's records that passed -- with windows,
 * on each window's pieces of such records: if more than D remain, the D with the largest match stay, a tie going to the
 * lower record index, and those that stay keep their own order (addAln order).  With windows the key is still the
 * RECORD's match, not the piece's: a record that agrees well overall wins a window it crosses badly.  The cap is taken
 * on every target and window, also on one that then fails or falls below min_cov.  min_cov counts what both steps
 * leave.  The result is, byte for byte, that of the same call without a filter on the batch without the records left
 * out (for a depth cap with windows: window by window): segments, target_status, dagcon_fetch_support,
 * dagcon_fetch_positions, the counts in the timings.  A non-conforming record has no counts and fails its target, or
 * the windows its span meets, exactly as without a filter.  A target or window that the filter brings to at most
 * DAGCON_MAX_COVERAGE records is not refused.
 * The filter holds for every later dagcon_upload_cigar* / dagcon_consensus_cigar* / _packed / _strand / dagcon_upload_cs /
 * dagcon_consensus_cs call on the context, whole targets and windows; dagcon_consensus, dagcon_consensus_pre and
 * dagcon_align ignore it.  NULL switches it off.  {1000000, 0} is legal: nothing is left out, the counts are there.
 * DAGCON_ERR_INVALID_ARG: max_error_ppm > 1000000 or max_depth > DAGCON_MAX_COVERAGE (the filter stays as it was).
 * Without a filter neither kernel of the rating runs.
 */
typedef struct dagcon_record_filter {
    uint32_t max_error_ppm;      /* 1000000: keep all */
    uint32_t max_depth;          /* 0: off */
} dagcon_record_filter;
int dagcon_set_record_filter(dagcon_ctx *ctx, const dagcon_record_filter *f);   /* NULL: off (the default) */

/* What the last record upload under a filter found, record by record (n == rec_begin[n_targets]).  Valid after such an
 * upload (or dagcon_consensus_cigar* / _cs) while the filter is set; DAGCON_ERR_STATE otherwise: no filter, no such
 * upload since the filter was set, or another kind of upload since.  The arrays are owned by the context until the next
 * upload. */
#define DAGCON_FATE_MAX_ERROR 1u      /* over max_error_ppm */
#define DAGCON_FATE_MAX_DEPTH 2u      /* left out of at least one target or window by max_depth */
#define DAGCON_FATE_NONCONFORMING 4u  /* non-conforming: its four counts are 0 */
typedef struct dagcon_record_stats {
    uint64_t n;
    const uint32_t *match, *mismatch, *ins, *del;   /* [n] */
    const uint8_t *fate;                            /* [n] DAGCON_FATE_* bits */
} dagcon_record_stats;
int dagcon_fetch_record_stats(dagcon_ctx *ctx, dagcon_record_stats *out);

/*
 * Debug / parity aid: adjacency of one target's graph as left by the last
 * dagcon_run (after mergeNodes), in list order.  Vertex ids are in backbone
 * position order: the inserted vertices whose _bbMap is p (in read, column
 * order), then backbone vertex p, for p = 0 .. tlen+1.  Node arrays have n_nodes
 * entries; out lists are CSR (out_begin[n_nodes+1], out_dst, out_count), in
 * lists likewise.  Buffers are owned by the context (valid until next call).
 */
typedef struct dagcon_graph_dump {
    uint32_t n_nodes;
    const uint8_t *base;
    const int32_t *weight;
    const int32_t *coverage;     /* meaningful for backbone vertices */
    const uint8_t *deleted;
    const uint8_t *backbone;     /* 1 for enter / backbone / exit vertices */
    const int32_t *bbpos;        /* backbone position (backbone vertices), _bbMap (inserted vertices) */
    const uint32_t *out_begin;
    const int32_t *out_dst;
    const int32_t *out_count;
    const uint32_t *in_begin;
    const int32_t *in_src;
} dagcon_graph_dump;
int dagcon_debug_graph(dagcon_ctx *ctx, uint32_t target, dagcon_graph_dump *out);

/* Kept for ABI 2.  The in-kernel cycle stamps that filled these sixteen counters in a
 * diagnostic build are gone: no build fills them any more, out8[0..15] are set to zero. */
int dagcon_debug_counters(dagcon_ctx *ctx, unsigned long long *out8);

/* Records of the last dagcon_align / dagcon_consensus_pre on this context whose corners the widest band could not
 * connect (sequences of very different lengths, indels of hundreds of bases): their alignment has length 0 and the
 * min_len filter then drops them, where the reference's SDPAlign + GuidedAlign (SimpleAligner.cpp:35-48) always
 * returns something.  On a DAGCON_FLAG_LOCAL_ALIGN context: the pairs without a local alignment in the widest band
 * (no cell scores below 0).  After dagcon_align_panels: the pairs it did not align because a panel was larger than
 * DAGCON_PANEL_MAX_SIDE (length 0 as well).  The calls succeed; a caller that cares asks here (the pbdagcon host
 * warns on stderr, dazcon --trace-panels aligns those pairs again with dagcon_align). */
uint32_t dagcon_align_dropped(dagcon_ctx *ctx);

/* The ends of the last dagcon_align / dagcon_consensus_pre on this context, pair by pair: the aligned strings cover
 * q[q_begin, q_end) and t[t_begin, t_end) of the pair's own sequences.  n must be that call's pair count
 * (DAGCON_ERR_INVALID_ARG otherwise).  Without DAGCON_FLAG_LOCAL_ALIGN: 0, q_len, 0, t_len for aligned pairs; both
 * modes: 0, 0, 0, 0 for pairs left unaligned. */
int dagcon_align_ends(dagcon_ctx *ctx, uint32_t n, uint32_t *q_begin, uint32_t *q_end, uint32_t *t_begin,
                      uint32_t *t_end);

/*
 * q-sense's read placement (the step q-sense.py has blasr do): for n_pairs (query q, target t) pairs over a set of
 * sequences, each pair's strand, its support on each strand and the span of t that q covers, by k-mer votes binned
 * by diagonal.  This build's own definition, parity unpinned: the reference delegates this to blasr.  Sequence s is
 * blob[seq_off[s] .. + seq_len[s]); pair a is q = pair_q[a] against t = pair_t[a].  Exact integer arithmetic
 * (tests/place_twin.py reproduces it bit for bit):
 *   - codes: A/a 0, C/c 1, G/g 2, T/t 3, any other byte invalid.  The k-mer at position i of x is valid if its k bytes
 *     are; its value packs 2 bits a base, the first base in the most significant bits.  8 <= k <= 16 (12 is the
 *     default of qsense).  rc(x) reverses x and complements A<->T, C<->G;
 *   - repeat mask: a k-mer value that occurs more than max_occ times in t is ignored (1 <= max_occ <= 8; qsense: 4);
 *   - votes: for strand '+' x = q, for '-' x = rc(q).  Every (i, j) where x's k-mer at i equals t's unmasked k-mer at
 *     j is one vote on diagonal d = j - i, in bin(d) = floor((d + |q|) / 64) (never negative);
 *   - support: V_s is the largest vote count of any bin of strand s (votes_fwd: V_+, votes_rev: V_-), B_s the smallest
 *     bin that reaches it.  strand is '+' if V_+ >= V_-, else '-'; when both are 0 it is '.' and t0 = t1 = 0;
 *   - span: with the chosen strand's bin B, a vote is consistent if |bin(d) - B| <= R, R = 2 + ceil(|q| / 512); its
 *     quarter is floor(4 i / |q|).  B_head is the most frequent bin among consistent votes of quarter 0, a tie going
 *     to the smaller bin, B if there are none; B_tail likewise for quarter 3.  t0 = clamp(64 B_head + 32 - |q|, 0, |t|)
 *     and t1 = clamp(64 B_tail + 32, 0, |t|): the bin centres as the diagonal at q's first base and just past its last.
 * Size limit: |q|, |t| <= 65,536 (DAGCON_PLACE_MAX_LEN) for every sequence a pair names, else DAGCON_ERR_UNSUPPORTED
 * (q-sense is "not optimized for larger templates"); DAGCON_ERR_INVALID_ARG for k or max_occ out of range or a
 * sequence past the blob.  Outputs are [n_pairs] arrays.
 */
#define DAGCON_PLACE_MAX_LEN 65536u
int dagcon_place(dagcon_ctx *ctx, const uint64_t *seq_off, const uint32_t *seq_len, const char *blob, uint64_t bytes,
                 uint32_t n_pairs, const uint32_t *pair_q, const uint32_t *pair_t, uint32_t k, uint32_t max_occ,
                 uint32_t *votes_fwd, uint32_t *votes_rev, char *strand, uint32_t *t0, uint32_t *t1);

/* Host arithmetic only (no device, no context): the pieces dagcon_upload would cut the merge and bestPath
 * sweeps of a batch of this shape into -- out4 = {pieces per target (merge), shortest stretch worth a
 * piece, 1 when the four-segments-per-wave merge kernel takes the batch, pieces per target (bestPath)}.
 * sum_positions = sum over active targets of tlen + 2 rounded up to a multiple of 4.  Every launch grid
 * derived from these is non-empty: pieces >= 1 for every input (tests/test_abi.py sweeps it). */
int dagcon_debug_plan(uint32_t n_targets, uint64_t n_alignments, uint64_t sum_positions, uint32_t partial_span,
                      uint32_t max_segments, uint32_t min_segment_len, uint32_t out4[4]);

#ifdef __cplusplus
}
#endif
#endif /* DAGCON_H */
