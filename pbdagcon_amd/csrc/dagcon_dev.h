// dagcon_dev.h -- device-side data layout shared by the kernels and the host API.
//
// One batch = T independent targets.  Everything lives in a handful of HBM
// arenas owned by the context; per-target and per-alignment arrays hold
// offsets into them.
//
// Vertex ids are target-local int32, numbered in BACKBONE-POSITION ORDER:
//   for p = 0 .. blen+1:   [inserted vertices whose _bbMap is p, in (read, column) order]
//                          [backbone vertex p]            (p = 0 enter '^', p = blen+1 exit '$')
// so id(backbone p) = bid[p] = gbase[p] + gcount[p], enter = 0, exit = N-1, and every edge of
// the freshly built graph runs from a lower id to a higher id.  Ids are only names: what the
// reference's results depend on is the ORDER of each vertex's out- and in-list (SURVEY
// Appendix A.1/A.2), which is kept exactly.  Position order makes the FIFO sweep of mergeNodes
// and the reverse sweep of bestPath walk memory monotonically (cache lines are reused, not
// re-fetched), which is what a latency-bound pointer chase needs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DG_GAP '-'

// DgParams::flags: bits 0..2 are dagcon_opts.flags; internal bits from 8 up
#define DG_F_RAW      1u
#define DG_F_A1_ONLY  8u   // dagcon_normalize: no graph follows, skip the backbone conformity check
#define DG_F_RESWEEP  16u  // DAGCON_FLAG_DEBUG_RESWEEP

// status bits (DgStatus::err_flags)
#define DG_E_BADCHAR     0x001u  // byte outside printable ASCII in an alignment string
#define DG_E_NONCONF     0x002u  // alignment leaves the backbone (start<1 or runs past tlen)
#define DG_E_NORM_OVF    0x004u  // normalised-column arena too small (rerun with norm_top)
#define DG_E_NODE_OVF    0x008u  // vertex arena too small (rerun with node_need)
#define DG_E_POOL_OVF    0x010u  // adjacency pool arena too small (rerun with pool_need)
#define DG_E_POOL_TGT    0x020u  // one target outgrew its pool share (rerun with larger growth factor)
#define DG_E_STACK       0x040u  // mergeInNodes recursion scratch exhausted
#define DG_E_INTERNAL    0x080u  // invariant violated (empty list dereference, list > 65535)
#define DG_E_OUT_OVF     0x100u  // output arena too small
#define DG_E_TOO_BIG     0x200u  // a target has more than 2^25-2 vertices
#define DG_E_LOG_OVF     0x800u  // a segment appended more entries to enter's / exit's list than its slots hold (rerun with more)
#define DG_E_LIST_OVF    0x400u  // more segments handed to k_merge_list than its worklist holds (rerun with a longer one)
#define DG_E_RUN_WIDE    0x1000u // an insertion run longer than 255 columns met byte-wide matC cells (rerun with 32-bit cells)
#define DG_E_ED_OVF      0x2000u // edit arena too small (dagcon_set_edits; rerun with *DgParams::ed_top)
#define DG_E_SITE_OVF    0x4000u // site arena too small (dagcon_set_pileup; rerun with *DgParams::site_top)
#define DG_E_SR_OVF      0x8000u // entry arena too small (dagcon_set_site_reads; rerun with *DgParams::sr_top)

// failures of one target (its input, or an invariant of its graph): recorded in DgParams::tfail,
// the batch goes on; everything else is a capacity problem of the whole batch (grow and re-run)
#define DG_E_TARGET_MASK (DG_E_BADCHAR | DG_E_NONCONF | DG_E_INTERNAL | DG_E_TOO_BIG)

struct DgStatus {
    uint32_t err_flags;
    uint32_t bad_aln;
    uint32_t bad_target;
    uint32_t n_mseg;               // segments of the merge / bestPath sweeps, all targets (k_cuts)
    unsigned long long norm_top;   // bump cursor into the column arena (uint16 units)
    unsigned long long node_need;  // exact vertex count of the batch (set by carve)
    unsigned long long pool_need;  // exact pool words of the batch (set by carve)
    unsigned long long cns_top;    // bump cursor into the consensus blob
    unsigned long long seg_top;    // bump cursor into the segment arrays
    unsigned long long n_columns;  // normalised, trimmed columns
    unsigned long long ovf_top;    // bump cursor into the re-run region of the chunk scratch (uint16 units)
};

// One 32-byte record per vertex.  The first 16 bytes are what a neighbour needs to know
// about it (one dwordx4 gather); the second 16 bytes say where its own lists live.
// out entry i: pool[out_off + 2i] = dst, pool[out_off + 2i + 1] = count
// in  entry i: pool[in_off + i]   = src          (edge counts live on the out side only)
struct __attribute__((aligned(16))) DgNode {
    uint16_t out_len, in_len;
    uint8_t base, flags;
    uint16_t pad;
    int32_t weight;
    int32_t pending;               // in-edges whose source is not processed yet (merge);
                                   // out-edges whose target is not scored yet (bestPath)
    uint32_t out_off, in_off;
    uint16_t out_cap, in_cap;
    int32_t bbpos;                 // _bbMap: absent key (enter, exit) reads as 0
};
#define DG_NF_BACKBONE 1u
#define DG_NF_DELETED  2u
#define DG_NF_DEFER    8u   // bestPath on partial-span pileups: scored by k_bp_defer, after the segments' sweeps
#define DG_NF_SHARED   4u   // during k_merge_list: a list of this vertex is shared by the segments' workers (DgGraph::sh)

// arrival cell: (target base << 25) | (source id + 1); deletion: id field all ones; DG_CELL_DUP (k_build.hip.h): a match
// whose in-edge an earlier read's folded chain already brings
// departure cell: (target id + 1) | (reads folded into this one's chain << 25)
#define DG_CELL_ID(c)   ((c) & 0x1FFFFFFu)
#define DG_CELL_DEL     0x1FFFFFFu
#define DG_CELL_BASE(c) ((uint8_t)((c) >> 25))
#define DG_MAX_NODES    0x1FFFFFDu
#define DG_EMIT_SEG     512u   // backbone positions per k_emit wave: default of DgParams::emit_shift (1 << 9)
#define DG_CK_NONE      0xFFFFFFFFu
#define DG_DEFER_MAX    64u
#define DG_SH_MAX       8u            // shared out-lists per target (enter + vertices of the prologue that reach into several segments)
#define DG_TOMB         0xFFFFFFFFu   // erased entry of a shared list (enter's out-list, exit's in-list)

struct DgParams {
    // ---- inputs (resident in HBM after dagcon_upload) ----
    const uint8_t *q, *t;
    const uint64_t *aln_off;
    const uint32_t *aln_len, *aln_start, *aln_tgt;
    const uint32_t *tlen;
    const uint64_t *aln_begin;     // [T+1], indices into the (filtered) alignment arrays
    const uint8_t *tactive;        // [T] 1 = build a graph (main.cpp:66-72,118)
    uint32_t *tfail;               // [T] DG_E_* bits of a failure confined to the target (bad input, broken
                                   // invariant): later kernels skip it, the other targets of the batch complete
    const uint8_t *bb;             // optional backbone blob
    const uint64_t *bb_off;
    const uint64_t *mat_base;      // [T] offset into matA/matD/matC: (tlen+2) * K cells
    const uint64_t *bbv_base;      // [T] offset into the per-position arrays: tlen+2 cells
    uint32_t T, A;
    uint32_t trim, min_len;
    int32_t min_weight;
    uint32_t flags;
    uint32_t max_k, max_tlen;
    // ---- per alignment work arrays ----
    uint32_t *nmis;
    uint64_t *norm_off;
    uint32_t *n_lo, *n_hi, *n_start, *n_ins, *n_del;
    uint16_t *norm;                // column arena: low byte q, high byte t
    uint64_t norm_cap;
    // ---- chunked normalizeGaps (k_norm_*): window c of alignment a is chunk ch_base[a] + c ----
    const uint32_t *ch_aln;        // [n_chunks] alignment of the chunk
    const uint32_t *ch_base;       // [A + 1]
    uint32_t n_chunks;
    uint32_t *ch_k0;               // first input column, DG_CH_NONE: no chunk starts in this window
    uint32_t *ch_next;             // window (of the alignment) the next chunk starts in
    uint32_t *ch_w, *ch_tb;        // columns written, of which with a target base
    uint32_t *ch_flag;             // 1 = the alignment goes to k_normalize_slow
    uint64_t *ch_src;              // where the chunk's columns are, in norm_tmp
    uint32_t *ch_out, *ch_adv;     // after k_norm_scan: column index / target bases in front, DG_CH_NONE: no chunk
    uint32_t *n_lb;                // [A] target bases trimAln took off the left end
    uint16_t *norm_tmp;            // chunk scratch: 2 columns per input column, then the re-run region
    // column of alignment a where backbone position s << emit_shift begins (its insertion run first),
    // at ckpt[ck_base[a] + s]; DG_CK_NONE where the read has no column at that position
    uint32_t *ckpt;
    const uint32_t *ck_base;       // [A]
    uint32_t emit_shift;           // log2 of the positions per k_emit wave (>= 4: whole 16-position batches)
    uint64_t tmp_main, tmp_cap;    // uint16 units: start of the re-run region, end of the scratch
    const uint64_t *tmp_off;       // [A] NULL: an alignment's scratch lies at its aln_off; dagcon_upload_haps, whose groups share strings: where it lies
    // ---- per target work arrays ----
    uint64_t *node_base;
    uint32_t *n_nodes;
    uint64_t *pool_base;
    uint32_t *pool_size, *pool_top;
    uint32_t *t_nins;              // inserted vertices of the target
    // ---- per backbone position (bbv_base indexed) ----
    uint32_t *gcount;              // inserted vertices whose _bbMap is p
    uint32_t *gbase;               // id of the first vertex of group p
    uint32_t *bid;                 // id of backbone vertex p
    int32_t *cov;                  // coverage (AlnGraphBoost.cpp:76,87)
    // ---- matrices [position][read] ----
    uint32_t *matA, *matD;         // arrival / departure
    void *matC;                    // [read][position] (row stride matc_stride): insertion run length in front of
                                   // the position, then (k_groups) its exclusive prefix over reads.  Cells are uint8_t
                                   // where p.emit_scan keeps the run lengths themselves (the kernels' <uint8_t>
                                   // instances; a run of more than 255 columns raises DG_E_RUN_WIDE), uint32_t otherwise
    const uint64_t *matc_base;     // [T] offset of the target's K rows, in cells
    const uint32_t *matc_stride;   // [T] (tlen + 2) rounded up to a multiple of 8 cells
    // ---- vertex arena ----
    DgNode *nodes;
    int32_t *best, *queue;
    float2 *score;                 // (best-path score, 1 = final)
    float *bp_tt;                  // per vertex: what an edge into it subtracts (k_bp_terms)
    float *score_b;                // per vertex (p.gcuts): B, best path to exit that does not pass the piece's upper cut
    uint32_t bp_seg_min;           // k_cuts2: shortest bestPath piece, in backbone positions (see fill_params)
    uint32_t bp_lane;              // 1: full-span bestPath with a lane per piece (k_bp_sweep_l); k_bp_sweep then takes the pieces it gave up
    uint32_t bl_stk;               // k_bp_sweep_l: entries of a lane's evaluation stack (<= DG_BL_STK; a test knob below that)
    uint8_t *cns_tmp;
    uint64_t node_cap;
    uint32_t *pool;
    uint64_t pool_cap;
    int32_t *stk;                  // per-target scratch, stk_words each
    uint32_t stk_words;
    uint32_t growth_pct;           // pool growth region as % of the initial adjacency words
    uint32_t emit_scan;            // 1 (every target has at most 64 reads): matC keeps the insertion run lengths, k_gsum adds them up
                                   // per position (gcount) and k_emit takes the prefix over the reads itself (DPP): no k_groups
    uint32_t fold;                 // 1: k_emit folds duplicate insertion chains as it builds (dg_emit_fold); 0 with
                                   // DAGCON_FLAG_STOP_AFTER_BUILD (the dump is then addAln's graph itself) and DAGCON_FOLD=0
    uint32_t q_kmax;               // k_merge_q takes the targets of at most this many reads, k_merge the deeper ones (0: no split)
    uint32_t seg_max;              // most segments a target's merge sweep is split into (k_cuts)
    uint32_t seg_min;              // shortest backbone stretch worth a worker of its own
    uint32_t *cuts;                // [T][seg_max + 2]: segment count, first vertex of each segment
    uint32_t bp_max;               // most segments of a target's bestPath sweep (finer than the merge's:
    uint32_t *cuts_bp;             //   its waves are light), [T][bp_max + 2] like cuts
    float *bp_stat;                // [T][seg_max][2]: largest |score| of the segment, score of its first vertex
    uint32_t *bp_len;              // [T][seg_max]: vertices of the best path inside the segment (enter / exit excluded)
    uint32_t *bp_end;              // [T][bp_max] (p.gcuts): where a piece of the walk ended (k_bp_walk)
    float *bp_ab;                  // [T][bp_max][4] (p.gcuts): A, B of the segment's first vertex, absolute score of its upper cut
    uint32_t *defer;               // [T][DG_DEFER_MAX + 1] (p.gcuts): count, then the vertices k_bp_defer scores
    uint8_t *cns_tmp0;             // (p.gcuts) the walk's first piece, from enter to the first cut it meets
    // ---- cuts for partial-span pileups (k_readspan, k_merge_pro, k_cuts2, k_merge_list, k_merge_fin) ----
    uint32_t gcuts;                // 1: mergeNodes runs as prologue + worklist of segments + epilogue
    uint32_t *rd_s, *rd_e;         // [A] first / last backbone position a read consumes (0 / 0: the read is empty)
    uint32_t *rd_lead, *rd_trail;  // [A] insertion run in front of the first / behind the last position
    int32_t *queue0;               // FIFO of the prologue and of the segment that resumes it (it also holds the vertices
                                   // the prologue visits beyond that segment: a stretch of `queue` would be too short)
    uint32_t *pro_state;           // [T][4]: queue head, queue tail of the prologue, vertices it visited, 1 = no cuts allowed
    uint32_t *sh_cnt;              // [T][2 + 2 * DG_SH_MAX]: shared out-lists n, entries of in[exit], then n x (vertex, entries of its out-list)
    uint32_t *seg_done;            // [worklist_cap][DG_SH_MAX + 1]: slots of its stretches a worklist entry has used (last: in[exit])
    uint32_t sh_log;               // slots a segment has behind either shared list
    uint32_t *worklist;            // [0] entries (k_cuts2), [2] ticket cursor (k_merge_list), then (target, first, last) triples
    uint32_t worklist_cap;
    uint32_t *wl_first;            // [T]: worklist index of the target's first segment
    // ---- outputs ----
    uint8_t *cns;
    uint64_t cns_cap;
    uint64_t *cns_off;
    uint32_t *cns_len;
    uint64_t *seg_first;
    uint32_t *n_seg;
    int32_t *seg_r0, *seg_r1;
    uint64_t seg_cap;
    DgStatus *st;
    // ---- per-base support (DAGCON_FLAG_BASE_SUPPORT only; NULL otherwise).  Last, so that every field above keeps its
    // offset and the flag-off kernels their code ----
    uint32_t *sup_tmp;             // [node_cap] parallel to cns_tmp: weight | depth << 16 of each path base of a walk piece
    uint32_t *sup_tmp0;            // [node_cap] (p.gcuts) parallel to cns_tmp0
    uint16_t *sup_w, *sup_d;       // [cns_cap] each, parallel to cns: weight and depth of each kept consensus base
    // ---- per-base target position (DAGCON_FLAG_BASE_POS only; NULL otherwise) ----
    uint32_t *pos_tmp;             // [node_cap] parallel to cns_tmp: _bbMap of each path base of a walk piece
    uint32_t *pos_tmp0;            // [node_cap] (p.gcuts) parallel to cns_tmp0
    uint32_t *pos_out;             // [cns_cap] parallel to cns: _bbMap of each kept consensus base
    // Bit 31 of a pos_tmp / pos_tmp0 word (DG_POS_BB) says that the base's vertex is a backbone vertex: the walks set it,
    // k_bp_join clears it on the way to pos_out unless the edit kernels are to read it there (ed_seg != NULL)
    // ---- edits (dagcon_set_edits on a record upload; NULL / 0 otherwise): k_edits.hip.h ----
    struct DgEdSeg *ed_seg;        // [seg_cap] one record per segment, in the order of seg_r0 / seg_r1
    struct DgEdit *ed_out;         // [ed_cap] the edits, segments in host order (target, then segment)
    uint64_t ed_cap;
    unsigned long long *ed_top;    // edits of the batch (k_ed_scan; in the status block)
    const uint8_t *ed_t;           // the record intake's target blob
    const uint64_t *ed_tbase;      // [T] where a target's (a window's) first base lies in it
    // ---- read support per edit (dagcon_set_edit_support; NULL otherwise): k_evidence.hip.h ----
    struct DgEvid *evid;           // [ed_cap] parallel to ed_out
    // ---- per-position allele counts (dagcon_set_pileup; NULL / 0 otherwise): k_pileup.hip.h ----
    uint32_t *pile;                // [4 * pile_n] a position's words: A | C << 16, G | T << 16, N | DEL << 16, INS
    const uint64_t *pile_begin;    // [T + 1] where a target's (a window's) first position lies in it
    uint64_t pile_n;               // positions of the batch
    unsigned long long *pile_tile; // [tiles of DG_PILE_TILE positions] sites of the tile, then (k_pile_scan) the sites in front of it
    struct DgSite *pile_site;      // [site_cap] the sites, in the order of the positions
    uint64_t site_cap;
    unsigned long long *site_top;  // sites of the batch (k_pile_scan; in the status block)
    uint32_t pile_min_count, pile_min_ppm;     // dagcon_pileup_opts
    // ---- per-read alleles at the sites and the two-way split (dagcon_set_site_reads; NULL / 0 otherwise): k_site_reads.hip.h ----
    unsigned long long *sr_bits;   // [(pile_n + 63) / 64] a bit per position: it is a site (cleared before every run)
    uint32_t *sr_rank;             // [(pile_n + 63) / 64] the first site of a word that holds one (its index in pile_site)
    uint32_t *sr_cnt;              // [A] entries of the alignment; DG_SR_TAKEN: the graph took it
    unsigned long long *sr_off;    // [A] where its entries begin (k_sr_scan)
    uint32_t *sr_site;             // [sr_cap] an entry's site (index in pile_site)
    uint8_t *sr_code;              // [sr_cap] an entry's code: cls | ins << 3
    uint64_t sr_cap;
    unsigned long long *sr_top;    // entries of the batch (k_sr_scan; in the status block)
    uint32_t sr_phase, sr_rounds;  // dagcon_site_reads_opts (rounds: the default filled in)
    uint8_t *sr_hap;               // [A] 0, 1, 2 (phase on)
    int8_t *sr_sigma;              // [site_cap] a site's phase
    uint8_t *sr_kind;              // [site_cap] what decides an entry's sign at the site (dg_sr_kind)
    int *sr_acc;                   // [site_cap] the sum over a site's entries of a round
    uint32_t *sr_nz;               // [A] entries with a sign
    // ---- the tally of the split (dagcon_set_hap_consensus; NULL / 0 otherwise): k_hap.hip.h ----
    uint32_t *hap_cnt;             // [2 * site_cap] a site's words: P1 | M1 << 16, P2 | M2 << 16 (cleared before every run)
    uint32_t *hap_rec;             // [DG_HAP_REC * T] a target's record: n1 n2 n0 n_sep agree disagree split 0
    uint32_t hap_min_sites, hap_min_reads, hap_min_cov;    // dagcon_hap_opts (the defaults filled in), max(1, min_cov)
    // ---- the alleles at the sites (dagcon_set_site_alleles; NULL / 0 otherwise): k_alleles.hip.h ----
    unsigned long long *al_soff;   // [site_cap] where a site's stretch begins: the depths of the sites in front (k_al_soff)
    uint32_t *al_cur;              // [site_cap + 1] entries a site's stretch holds (cleared before every run); last: the deep sites listed
    unsigned long long *al_srt;    // [sr_cap] a site's stretch: its entries' keys, then (k_al_table) its table's keys at the front
    uint32_t *al_tcnt;             // [sr_cap] parallel to al_srt: the count of a table's allele
    uint32_t *al_thap;             // [sr_cap] parallel to al_srt: c1 | c2 << 16 of a table's allele (phase on)
    uint32_t *al_nd;               // [site_cap] alleles of a site's table
    uint32_t *al_deep;             // [site_cap] the sites of more than 64 entries, in no order
    unsigned long long *al_toff;   // [site_cap] where a site's table begins in the compact arrays (k_al_tscan)
    uint16_t *al_idx;              // [sr_cap] parallel to sr_site / sr_code: an entry's place in its site's stretch (k_al_keys), then its allele's index in the site's table (k_al_index)
    uint16_t *al_map;              // [sr_cap] parallel to al_srt: the allele's index of the entry that holds this place of the stretch
    unsigned long long *al_ckey;   // [*al_top, at the fetch] the tables, site after site: key, count, c1 | c2 << 16
    uint32_t *al_ccnt, *al_chap;
    unsigned long long *al_ent_top, *al_top;   // the sum of the depths; the alleles of the batch (words of their own, fetched when asked)
    uint64_t al_nocap;             // 2^64 - 1: the two scans have no arena of their own to outgrow
    // ---- the windows' labels joined into blocks (dagcon_set_window_phase; NULL / 0 otherwise): k_winlink.hip.h ----
    const uint32_t *wl_rec;        // [A] the record an alignment is a piece of; ascending inside a window
    const uint32_t *wl_tgt;        // [T] the target a window lies on: the window in front is its predecessor iff it has the same
    uint32_t *wl_cnt;              // [2 * T] a window's same, diff (k_wl_pairs)
    uint32_t *wl_block;            // [T] the first window of its block (k_wl_scan)
    uint8_t *wl_flip;              // [T] its orientation
    uint8_t *wl_hap;               // [A] sr_hap, oriented (k_wl_apply)
    int8_t *wl_phase;              // [site_cap] sr_sigma, oriented
    uint32_t wl_min_links, wl_max_ppm;     // dagcon_window_phase_opts (the defaults filled in)
    // ---- adjacent sites joined into runs (dagcon_set_site_join; NULL / 0 otherwise): k_join.hip.h.  Last, so that every
    // field above keeps its offset ----
    uint32_t *jn_run;              // [site_cap] a site's stretch (k_jn_stretch), then its run (k_jn_runs)
    uint32_t *jn_sfirst;           // [site_cap] a stretch's first site
    uint32_t *jn_rbeg;             // [site_cap + 1] a run's first site; one more: the end of the last run
    uint32_t *jn_cur;              // [site_cap + 1] spanning members a run's stretch holds (cleared before every run); last: the deep runs listed
    uint32_t *jn_part;             // [site_cap] a run's partial members (cleared with jn_cur)
    uint32_t *jn_nd;               // [site_cap] joined alleles of a run's table
    uint32_t *jn_deep;             // [site_cap] the runs of more than 64 spanning members, in no order
    unsigned long long *jn_toff;   // [site_cap] where a run's table begins in the compact arrays (k_jn_tscan)
    unsigned long long *jn_key;    // [sr_cap] the stretch of a run's first site (al_soff): its spanning members' keys, then (k_jn_table) its table's keys at the front
    uint32_t *jn_tcnt, *jn_thap;   // [sr_cap] parallel to jn_key: the count and c1 | c2 << 16 of a table's joined allele
    uint16_t *jn_map;              // [sr_cap] parallel to jn_key: the joined allele's index of the member that holds this place
    uint16_t *jn_idx;              // [sr_cap] parallel to sr_site: a spanning member's place (k_jn_keys), then its joined allele's index (k_jn_index); DG_JN_NONE: a partial member's entry
    unsigned long long *jn_ckey;   // [*jn_top, at the fetch] the tables, run after run: key, count, c1 | c2 << 16
    uint32_t *jn_ccnt, *jn_chap;
    unsigned long long *jn_st_top, *jn_run_top, *jn_top;   // the stretches, the runs, the joined alleles of the batch (words of their own, fetched when asked)
    // ---- the two groups' edits paired (dagcon_set_hap_calls on the batch of dagcon_upload_haps; NULL otherwise):
    // k_hap_calls.hip.h.  Last, so that every field above keeps its offset ----
    uint8_t *hc_state;             // [ed_cap] parallel to ed_out: DG_HC_*
    unsigned long long *hc_mate;   // [ed_cap] parallel to ed_out: the partner's edit (index into ed_out), all ones: none
    // ---- the kept part of every segment (dagcon_set_window_keep on a windows upload or on the batch dagcon_upload_haps
    // derives from one; NULL otherwise): k_keep.hip.h.  Last, so that every field above keeps its offset ----
    uint4 *keep_out;               // [seg_cap] in the order of seg_r0 / seg_r1: x = the segment's target (k_bp_join), then i0, i1, p_first, p_last (k_win_keep)
    const uint32_t *keep_lo, *keep_hi;     // [T] a target's (a window's) lo and hi
    // ---- the sites the same reads carry (dagcon_set_site_link, with the split; NULL / 0 otherwise): k_site_link.hip.h.
    // Last, so that every field above keeps its offset ----
    unsigned long long *lk_rows;   // [lk_row_cap] a site's rows: lk_words words P, then lk_words words M; bit x - aln_begin[t] (cleared before every run)
    uint64_t lk_row_cap;           // site_cap * 2 * lk_words
    uint16_t *lk_partners;         // [site_cap] a site's partners
    uint8_t *lk_linked;            // [site_cap] 1: partners >= lk_min_partners; k_sr_split mutes the others
    uint32_t lk_words;             // words of a row: (max_k + 63) / 64, one width for the batch
    uint32_t lk_ppm, lk_min_cell, lk_min_partners, lk_reach;   // dagcon_site_link_opts (the defaults filled in)
};
#define DG_HAP_REC 8u
#define DG_SR_TAKEN 0x80000000u
#define DG_POS_BB 0x80000000u

struct __attribute__((aligned(16))) DgEdSeg {
    uint32_t tgt;                  // the segment's target (k_bp_join)
    uint32_t cnt;                  // its edits, after the trim (k_ed_scan_seg<false>)
    uint32_t t0, t1;               // its target span [t0, t1)
    unsigned long long off;        // its first edit in ed_out (k_ed_scan)
    unsigned long long pad;
};
struct DgEdit {
    unsigned long long c_off;      // into cns
    uint32_t t_pos, t_len, c_len, pad;
};

// one per edit: its group's window, alt allele and counts (k_evidence.hip.h)
struct DgEvid {
    unsigned long long c_lo;       // where the group's alt allele begins, into cns
    uint32_t gL, gR;               // the group's window [gL, gR)
    uint32_t alt_len;              // bytes of the alt allele
    uint32_t back;                 // edits back to the group's first edit (0: this is it, and the counts are added here)
    uint32_t span, alt, ref, pad;
};

// one per site: its position in its target and the position's four words (k_pileup.hip.h)
struct DgSite {
    uint32_t pos, tgt;
    uint32_t w[4];
};

// slots a backbone vertex gets for each of its two lists before it has to move to the
// growth region (K = alignments of the target)
__host__ __device__ inline uint32_t dg_capb(uint32_t k) { return k + 2u < 12u ? k + 2u : 12u; }
