// api_ctx.h -- the context: owning buffers, the named buffer sets, the status block, the optional outputs' records and result
// arrays, Ctx, errors, ensure(), upload() and d2h()
// (one translation unit with dagcon_api.hip, which includes it once).
namespace {

struct Ctx;

// a device buffer and its owner: grown by ensure(), freed with the context
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    template <class X> X *as() const { return static_cast<X *>(p); }
};

// a page-locked host buffer and its owner (cap in bytes): what comes back from the device at PCIe speed
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int reserve(Ctx *c, size_t bytes);              // (at least bytes; what it held is gone when it grows)
    template <class X> X *as() const { return static_cast<X *>(p); }
};

// the device buffers of the record intake, by name
struct CigarBufs {
    DevBuf ops, op_begin, tile_begin, totals, ckpt;                // the records' ops, k_cigar_scan's output
    DevBuf q, t, q_off, t_base;                                    // the blobs and where each record's bases begin
    DevBuf out_off;                                                // whole targets: where each record's strings go
    DevBuf piece, cut, wave_piece, wave_begin, piece_out;          // windows: DgCigarCutParams
    DevBuf rev, q_len;                                             // DgCigarStrand
    DevBuf rate_base, tile_rate, rate;                             // DgCigarRate (a record filter is set)
};
// dagcon_upload_cs: the text and what k_cs_scan / k_cs_write take besides CigarBufs::ops, q and t, which k_cs_write fills
struct CsBufs {
    DevBuf text, cs_off, cs_len, totals, n_ops, op_begin, t_base, t_room, q_off, q_len;
};
// dagcon_upload_cigar_md: the MD texts and what the k_md_* kernels take besides CigarBufs::t, which they fill
struct MdBufs {
    DevBuf text, md_off, md_len, totals, t_base, nt, tgt, mark, conflict;
};
// dagcon_align (align_device): blobs, offsets, outputs, directions, launch order, widths, ends; qaln / taln at out_off are
// what dagcon_consensus_pre hands to the pipeline
struct AlignBufs {
    DevBuf q, t, q_off, t_off, q_len, t_len, out_off, qaln, taln, len, dirs, dir_off, idx, halfw, ends;
};
// dagcon_align_panels: blobs, panels (p_*), scratch, per-panel outputs, launch order, then the pairs' side
struct PanelBufs {
    DevBuf q, t, p_q_off, p_t_off, p_q_len, p_t_len, scr_off, qscr, tscr, p_len, p_dist, idx, panel_begin, out_off, qaln, taln, len, kept;
};
// dagcon_place: blob, sequences, tables, pairs, outputs
struct PlaceBufs {
    DevBuf blob, seq_off, seq_len, tab_seq, tab_base, tab_mask, slots, pq, pt, ptab, pid, votes, span, strand;
};

// The buffers of a batch on its way through the pipeline, by who writes them.
// InBufs: what the host uploads per batch (upload_impl, edits_arm; q / t also by the record intake's expansion)
struct InBufs {
    DevBuf q, t, aln_off, aln_len, aln_start, aln_tgt, tlen, aln_begin, tactive, bb, bb_off, mat_base, bbv_base, matc_base, matc_stride;
    DevBuf norm_off, ch_aln, ch_base, ck_base;
    DevBuf tmp_off;                                 // dagcon_upload_haps: where each alignment's normalisation scratch lies (its groups share strings)
    DevBuf ed_tbase;                                // dagcon_set_edits: where each target's bases begin in cg.t
    DevBuf pile_begin;                              // dagcon_set_pileup: where each target's positions begin in run.pile
    DevBuf wl_rec, wl_tgt;                          // dagcon_set_window_phase: each alignment's record, each window's target
    DevBuf keep_lo, keep_hi;                        // dagcon_set_window_keep: each target's (window's) lo and hi
};
// RunBufs: what the kernels of a run fill and nobody clears.  all() is the set DAGCON_POISON & 8 fills with 0xEE bytes
// before every run (launch_all): a new member goes into it, and the static_assert below says so
struct RunBufs {
    DevBuf nmis, n_lo, n_hi, n_start, n_ins, n_del;
    DevBuf ch_k0, ch_next, ch_w, ch_tb, ch_flag, ch_src, ch_out, ch_adv, n_lb, norm_tmp, ckpt;
    DevBuf node_base, n_nodes, pool_base, pool_size, pool_top, t_nins;
    DevBuf cov, gcount, gbase, bid;
    DevBuf best, queue, score, cns_tmp, bp_tt;
    DevBuf stk, cuts, cuts_bp, bp_stat, bp_len, rd, pro_state, sh_cnt, wl_first, queue0, bp_end, bp_ab, defer, cns_tmp0;
    DevBuf cns;
    DevBuf seg;                                     // seg_r0[seg_cap], then seg_r1 at seg_stride() entries
    DevBuf worklist, seg_done;
    DevBuf sup_tmp, sup_tmp0, sup;                  // DAGCON_FLAG_BASE_SUPPORT: walk scratch (4 B per vertex), output (2 x 2 B per base)
    DevBuf pos_tmp, pos_tmp0, pos;                  // DAGCON_FLAG_BASE_POS: walk scratch (4 B per vertex), output (4 B per base)
    DevBuf ed_seg, ed_out;                          // dagcon_set_edits: a DgEdSeg per segment, a DgEdit per edit
    DevBuf evid;                                    // dagcon_set_edit_support: a DgEvid per edit
    DevBuf pile, pile_tile, pile_site;              // dagcon_set_pileup: 16 B per position (cleared before every run), 8 B per tile, a DgSite per site
    // dagcon_set_site_reads: a bit and a rank word per 64 positions; per alignment its entry count, offset, hap and signed
    // entries; per entry its site and code; per site its phase, sign rule and a round's sum
    DevBuf sr_bits, sr_rank, sr_cnt, sr_off, sr_site, sr_code, sr_hap, sr_sigma, sr_kind, sr_acc, sr_nz;
    DevBuf hap_cnt, hap_rec;                        // dagcon_set_hap_consensus: 8 B per site (cleared before every run), DG_HAP_REC words per target
    DevBuf wl_cnt, wl_block, wl_flip, wl_hap, wl_phase;    // dagcon_set_window_phase: 8 + 4 + 1 B per window, 1 B per alignment, 1 B per site
    // dagcon_set_site_alleles: per entry its place, then its allele's index; per site its stretch's offset, its cursor
    // (cleared before every run), its table's size and offset, the list of the deep sites; the stretches (keys, counts,
    // counts per label, the places' indices); the compact tables (sized and filled at the fetch); the two totals
    DevBuf al_map, al_idx, al_soff, al_cur, al_nd, al_deep, al_toff, al_srt, al_tcnt, al_thap, al_ckey, al_ccnt, al_chap, al_tot;
    // dagcon_set_site_join: per site its run and its stretch's first site; per run its first site, its cursor and partial
    // count (one buffer, cleared before every run), its table's size and offset, the list of the deep runs; per entry its
    // member's place, then its joined allele's index; the stretches (keys, counts, counts per label, the places' indices);
    // the compact tables (sized and filled at the fetch); the three totals
    DevBuf jn_run, jn_sfirst, jn_rbeg, jn_cur, jn_nd, jn_deep, jn_toff, jn_key, jn_tcnt, jn_thap, jn_map, jn_idx, jn_ckey, jn_ccnt, jn_chap, jn_tot;
    DevBuf hc_state, hc_mate;                       // dagcon_set_hap_calls: a state byte and a mate index per edit, parallel to ed_out
    DevBuf keep;                                    // dagcon_set_window_keep: 16 B per segment, parallel to seg
    DevBuf lk_rows, lk_partners, lk_linked;         // dagcon_set_site_link: two bit rows a site (cleared before every run), its partners, its linked byte
    std::array<DevBuf *, 116> all() {
        return {&nmis, &n_lo, &n_hi, &n_start, &n_ins, &n_del, &ch_k0, &ch_next, &ch_w, &ch_tb, &ch_flag, &ch_src, &ch_out, &ch_adv, &n_lb, &norm_tmp, &ckpt,
                &node_base, &n_nodes, &pool_base, &pool_size, &pool_top, &t_nins, &cov, &gcount, &gbase, &bid, &best, &queue, &score, &cns_tmp, &bp_tt,
                &stk, &cuts, &cuts_bp, &bp_stat, &bp_len, &rd, &pro_state, &sh_cnt, &wl_first, &queue0, &bp_end, &bp_ab, &defer, &cns_tmp0, &cns,
                &seg, &worklist, &seg_done, &sup_tmp, &sup_tmp0, &sup, &pos_tmp, &pos_tmp0, &pos, &ed_seg, &ed_out, &evid, &pile, &pile_tile, &pile_site,
                &sr_bits, &sr_rank, &sr_cnt, &sr_off, &sr_site, &sr_code, &sr_hap, &sr_sigma, &sr_kind, &sr_acc, &sr_nz,
                &hap_cnt, &hap_rec, &wl_cnt, &wl_block, &wl_flip, &wl_hap, &wl_phase,
                &al_map, &al_idx, &al_soff, &al_cur, &al_nd, &al_deep, &al_toff, &al_srt, &al_tcnt, &al_thap, &al_ckey, &al_ccnt, &al_chap, &al_tot,
                &jn_run, &jn_sfirst, &jn_rbeg, &jn_cur, &jn_nd, &jn_deep, &jn_toff, &jn_key, &jn_tcnt, &jn_thap, &jn_map, &jn_idx, &jn_ckey, &jn_ccnt, &jn_chap, &jn_tot,
                &hc_state, &hc_mate, &keep, &lk_rows, &lk_partners, &lk_linked};
    }
};
static_assert(sizeof(RunBufs) == 116 * sizeof(DevBuf), "RunBufs::all() must name every member");
// ArenaBufs: the arenas with a treatment of their own -- matC is cleared before every run, the others are filled under
// DAGCON_POISON bits 1 (matA, matD), 2 (nodes, pool) and 4 (score_b, norm)
struct ArenaBufs {
    DevBuf matA, matD, matC, nodes, pool, score_b, norm;
};

// The words the host reads back after every run, as ranges of ONE device buffer (each 16-byte aligned): what a run starts
// from zero first -- DgStatus, tfail[T + 1], cns_len[T], n_seg[T]: one memset -- then cns_off[T] and seg_first[T].  The whole
// block comes back in one copy into `host`, its page-locked mirror (dagcon_fetch reads the mirror in place).
struct StatBlock {
    DevBuf dev;
    PinBuf host;
    size_t o_tfail = 0, o_cns_len = 0, o_n_seg = 0, o_cns_off = 0, o_seg_first = 0;     // (DgStatus at 0)
    size_t zero_bytes = 0, bytes = 0;               // (behind seg_first: the totals of the growing arenas, GrowArena::o_top)
    template <typename X> X *d(size_t off) const { return reinterpret_cast<X *>(static_cast<char *>(dev.p) + off); }
    template <typename X> const X *h(size_t off) const { return reinterpret_cast<const X *>(host.as<char>() + off); }
};

// An arena of an optional output whose size only a run tells: the run's scan (k_scan.hip.h) stores the total in a word of
// the status block and raises `ovf` when it exceeds `cap`; dagcon_fetch then sets cap = total + 1024 and runs the batch
// again.  Ctx::growing() lists them; ensure_stat (the words' layout), fill_params, the re-run and arena_total walk that list.
struct GrowArena {
    const char *what;                               // what it holds, for messages
    uint32_t ovf;                                   // DG_E_*_OVF
    bool own_word;                                  // false: its word is the second of the 16 bytes of the arena in front of it
    unsigned long long *DgParams::*p_top;           // the kernels' names for the word and the capacity
    uint64_t DgParams::*p_cap;
    uint64_t cap = 0;                               // entries (first guess at the upload; DAGCON_EDITS_CAP: the edits')
    size_t o_top = 0;                               // the word's offset in the status block of this batch; 0: the output is off
};
struct GrowRef { GrowArena *g; bool on; };          // an arena, and whether the batch on the device was uploaded with its output on

enum class Fresh { FETCH, RUN, UPLOAD };            // what is new when results stop being valid (Ctx::drop_results)
enum class Intake { STRINGS, RECORDS, WINDOWS, HAPS };    // how a batch comes to upload_impl: as strings, from the record intake (whole targets, windows), from dagcon_upload_haps

// One optional output of a run (api_outputs.hip.h): the text its fetches fail with; the switch (dagcon_set_*); whether the
// batch on the device was uploaded under it and under everything it rests on (latch_outputs); whether the last fetch
// brought its results; whether the copies that fetch left out have been made (the output's own fetch makes them when asked)
struct Output {
    const char *missing;
    bool on = false, batch = false, valid = false, fetched = false;
};

// What the outputs' fetches return, by output: host arrays the context owns, valid as long as the results of the same fetch.
// dagcon_fetch_edits: per segment its target range and where its edits begin, per edit its place and length in the target
// and in seq_blob; dagcon_fetch_edit_support: per edit its window and the alignments that span it, carry the consensus'
// allele, the target's
struct EditsOut {
    std::vector<uint32_t> t0, t1, tpos, tlen, clen, w_begin, w_end, span, alt, ref;
    std::vector<uint64_t> begin, coff;
    // dagcon_set_hap_calls only: each listed edit's index on the device, where each target's listed edits begin [T + 1],
    // and the edits of the device
    std::vector<uint64_t> dev_idx, tgt_begin;
    uint64_t n_dev = 0;
};
// dagcon_fetch_hap_calls: per edit of dagcon_fetch_edits its state and its mate
struct HapCallsOut {
    std::vector<uint8_t> state;
    std::vector<uint64_t> mate;
};
// dagcon_fetch_pileup_sites: where a target's sites begin, each site's position and counts; and the site map of the other
// fetches -- where a target's sites begin in the device's list (begin: in the host's), and that list's length
struct SitesOut {
    std::vector<uint64_t> begin, dev_begin;         // [T + 1]
    std::vector<uint32_t> pos;
    std::vector<uint16_t> counts;
    uint64_t n_dev = 0;
};
// dagcon_fetch_site_reads: per kept alignment its target, the caller's index, where its entries begin and its label; per
// entry its site and code; per site its phase.  n_dev_ent: the entries of the device, kept or not
struct SiteReadsOut {
    uint64_t n_dev_ent = 0;
    std::vector<uint32_t> tgt;
    std::vector<uint64_t> src, begin, site;
    std::vector<uint8_t> code, hap;
    std::vector<int8_t> phase;
};
// dagcon_fetch_site_alleles: where a site's alleles begin; per allele its key, count and counts per label; per entry its allele
struct AllelesOut {
    std::vector<uint64_t> begin, key;
    std::vector<uint32_t> count;
    std::vector<uint16_t> hap, ent;
};
// dagcon_fetch_joined_sites: where a run's sites and its joined alleles begin; per run its spanning and partial members; per
// joined allele its key, count and counts per label; per entry its joined allele
struct JoinedOut {
    std::vector<uint64_t> run_begin, begin, key;
    std::vector<uint32_t> spanning, partial, count;
    std::vector<uint16_t> hap, ent;
};
// dagcon_fetch_hap_tally: two lazy parts -- the per-target records (Output::fetched; dagcon_upload_haps reads them too),
// zeros for a failed target, and the site counters in the host's order of the sites (sites_fetched)
struct HapOut {
    bool sites_fetched = false;
    std::vector<uint32_t> rec;          // [6][T]: n1, n2, n0, n_sep, agree, disagree
    std::vector<uint8_t> split;         // [T]
    std::vector<uint16_t> counts;       // [4 * sites] P1 M1 P2 M2
};
// dagcon_fetch_window_phase: per window, per kept alignment, per site, in the host's order
struct WinPhaseOut {
    std::vector<uint32_t> same, diff, block;
    std::vector<uint8_t> flip, hap;
    std::vector<int8_t> phase;
};
// dagcon_fetch_hap_map: the batch on the device is dagcon_upload_haps' (valid), and what it holds
struct HapMapOut {
    bool valid = false;
    std::vector<uint32_t> src_target;
    std::vector<uint8_t> label;
    std::vector<uint64_t> aln_begin, aln_src;
};
// dagcon_fetch_window_keep: per segment of the last results, in their order
struct KeepOut {
    std::vector<uint32_t> i0, i1, p_first, p_last;
};
// dagcon_fetch_site_link: per site of dagcon_fetch_pileup_sites, in the host's order
struct SiteLinkOut {
    std::vector<uint16_t> partners;
    std::vector<uint8_t> linked;
};
// The kept alignments of a fetched run in the device's order (host_order builds it at the first fetch that needs it): each
// one's index on the device and its stretch of the device's entry arrays.  Its target and the caller's index are
// h_aln_tgt / h_aln_src at that index
struct HostOrder {
    bool built = false;
    std::vector<uint32_t> aln, ent_n;
    std::vector<uint64_t> ent_begin;
};

struct Ctx {
    dagcon_opts opts;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::string err;
    bool uploaded = false, ran = false, fetched = false;

    // host copy of the filtered batch
    uint32_t T = 0, A = 0;
    int bp_lane = 1, bl_stk = -1;                  // full-span bestPath: a row of eight lanes per piece (k_bp_sweep_l; DAGCON_BP_LANE=0: a wave per piece, k_bp_sweep; 2: rows whatever the batch size); DAGCON_BP_LANE_STACK: test knob
    uint32_t align_dropped = 0;                    // records of the last dagcon_align / dagcon_consensus_pre the band could not align
    uint32_t align_n = 0;                          // pairs of the last dagcon_align / dagcon_consensus_pre
    std::vector<uint32_t> h_ends;                  // their ends (dagcon_align_ends): q_begin, q_end, t_begin, t_end per pair
    int poison = 0;                                // DAGCON_POISON (tests): arenas nobody clears are filled with 0xEE bytes before every run (bits 1, 2, 4); 8: every buffer the kernels fill
    int fold = 1;                                  // duplicate insertion chains folded by k_emit (DAGCON_FOLD=0: never)
    int merge_q = 1, use_q = 0;                    // k_merge_q: eight segments per wave (DAGCON_MERGE_Q=0: never); this batch
    uint32_t max_k = 0, max_tlen = 0;
    uint64_t sum_len = 0, sum_bb = 0, mat_cells = 0, blob_bytes = 0;
    bool have_bb = false;
    std::vector<uint32_t> h_tlen, h_aln_len, h_aln_start, h_aln_tgt;
    std::vector<uint64_t> h_aln_begin, h_aln_off, h_mat_base, h_bbv_base, h_bb_off, h_matc_base;
    std::vector<uint32_t> h_matc_stride;
    uint64_t matc_cells = 0;
    bool wide_cells = false;                        // an insertion run of more than 255 columns: 32-bit matC cells (met by this upload's run, or by the one before and in this batch's strings)
    std::vector<uint8_t> h_tactive;
    std::vector<uint32_t> h_ch_base, h_ch_aln;      // chunk tables of k_norm_*
    std::vector<uint64_t> h_norm_off;               // column buffer of each alignment
    std::vector<uint32_t> h_ck_base;                // first k_emit checkpoint of each alignment
    uint64_t n_ckpt = 0;
    uint32_t emit_shift = 9;                        // 512 backbone positions per k_emit wave
    uint32_t n_chunks = 0;
    uint64_t tmp_main = 0, tmp_cap = 0;
    bool tmp_shared = false;                        // the batch on the device is dagcon_upload_haps': in.tmp_off holds its scratch offsets

    // device buffers (each frees itself with the context)
    InBufs in;
    RunBufs run;
    ArenaBufs arena;
    AlignBufs al;                                   // dagcon_align
    PanelBufs pn;                                   // dagcon_align_panels
    PlaceBufs pl;                                   // dagcon_place
    CsBufs cs;                                      // dagcon_upload_cs
    CigarBufs cg;                                   // dagcon_upload_cigar and its kin
    MdBufs md;                                      // dagcon_upload_cigar_md
    bool md_valid = false, md_fetched = false;      // cg.t holds the targets such an upload rebuilt; h_md_t holds them too (dagcon_fetch_md_targets)
    uint64_t md_bytes = 0;
    std::vector<char> h_md_t;
    std::vector<uint8_t> h_cig_bad;                 // dagcon_upload_cigar: targets with a non-conforming record (empty: another upload)
    std::string cig_err;                            // the first of them, for dagcon_last_error
    bool filter_on = false;                         // dagcon_set_record_filter: the record intake rates and picks its records
    dagcon_record_filter filter = {1000000u, 0u};
    bool rs_valid = false;                          // the record stats below are those of the last upload (dagcon_fetch_record_stats)
    std::vector<uint32_t> rs_match, rs_mismatch, rs_ins, rs_del;
    std::vector<uint8_t> rs_fate;
    StatBlock sb;                                   // DgStatus, tfail, cns_len, n_seg, cns_off, seg_first
    // The optional outputs (api_outputs.hip.h), one record each, and beside it its options as set and as latched for the
    // batch on the device (latch_outputs holds the rule, and fills the defaults in).  outputs() lists them: whatever
    // happens to all of them walks that list.
    // dagcon_set_edits (its buffers: run.ed_seg, run.ed_out, in.ed_tbase) and dagcon_set_edit_support (on only while edits are)
    Output o_ed{"without the results of a record upload made with dagcon_set_edits on (edits off, another kind of upload, no fetch yet, or stopped before bestPath)"};
    Output o_evid{"without the results of a record upload made with dagcon_set_edit_support on (switch off at the upload, edits off, another kind of upload, "
                  "no fetch yet, or stopped before bestPath)"};
    std::vector<uint64_t> h_ed_tbase;
    // dagcon_set_pileup and its thresholds (its buffers: in.pile_begin, run.pile, run.pile_tile, run.pile_site)
    Output o_pile{"without the results of an upload made with dagcon_set_pileup on (switch off at the upload, no fetch yet, or stopped before bestPath)"};
    dagcon_pileup_opts pile_opts = {0u, 0u}, pile_batch_opts = {0u, 0u};
    std::vector<uint64_t> h_pile_begin;             // [T + 1]
    // dagcon_set_site_reads; per alignment of the device the index the caller knows it by
    Output o_sr{"without the results of an upload made with dagcon_set_pileup and dagcon_set_site_reads on (a switch off at the upload, no fetch yet, or "
                "stopped before bestPath)"};
    dagcon_site_reads_opts sr_opts = {0u, 0u}, sr_batch_opts = {0u, 0u};
    std::vector<uint64_t> h_aln_src;                // [A]
    // dagcon_set_site_alleles
    Output o_al{"without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads and dagcon_set_site_alleles on (a switch off at the "
                "upload, no fetch yet, or stopped before bestPath)"};
    // dagcon_set_site_join
    Output o_jn{"without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads, dagcon_set_site_alleles and dagcon_set_site_join on (a "
                "switch off at the upload, no fetch yet, or stopped before bestPath)"};
    // dagcon_set_hap_consensus
    Output o_hap{"without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads (phase on) and dagcon_set_hap_consensus on (a switch "
                 "off at the upload, no fetch yet, stopped before bestPath, or the batch is dagcon_upload_haps' own)"};
    dagcon_hap_opts hap_opts = {0u, 0u}, hap_batch_opts = {0u, 0u};
    // dagcon_set_window_phase
    Output o_wl{"without the results of a windows upload made with dagcon_set_pileup, dagcon_set_site_reads (phase on) and dagcon_set_window_phase on (a "
                "switch off at the upload, no windows, no fetch yet, or stopped before bestPath)"};
    dagcon_window_phase_opts wl_opts = {0u, 0u}, wl_batch_opts = {0u, 0u};
    // dagcon_set_hap_calls (on only while edits are; latched for the batch of dagcon_upload_haps alone)
    Output o_hc{"without the results of a dagcon_upload_haps made with dagcon_set_hap_calls on behind a record upload that ran with dagcon_set_edits on (a "
                "switch off, another kind of first upload, no fetch yet, or stopped before bestPath)"};
    // dagcon_set_window_keep (its buffers: in.keep_lo, in.keep_hi, run.keep): lo / hi as set, one pair per window of a first
    // batch; latched for a windows upload and for the batch dagcon_upload_haps derives from one.  win_first / win_n: the
    // first batch on the device (the one a dagcon_upload_haps derives from) was a windows upload, and of how many windows
    Output o_keep{"without the results of a windows upload, or of a dagcon_upload_haps behind one, made with dagcon_set_window_keep on (switch off at the upload, "
                  "no windows, no fetch yet, or stopped before bestPath)"};
    std::vector<uint32_t> keep_lo, keep_hi;
    bool win_first = false;
    uint32_t win_n = 0;
    // dagcon_set_site_link (its buffers: run.lk_rows, run.lk_partners, run.lk_linked)
    Output o_lk{"without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads (phase on) and dagcon_set_site_link on (a switch "
                "off at the upload, no fetch yet, stopped before bestPath, or the batch is dagcon_upload_haps' own)"};
    dagcon_site_link_opts lk_opts = {0u, 0u, 0u, 0u}, lk_batch_opts = {0u, 0u, 0u, 0u};
    std::array<Output *, 11> outputs() { return {&o_ed, &o_evid, &o_pile, &o_sr, &o_al, &o_jn, &o_hap, &o_wl, &o_hc, &o_keep, &o_lk}; }
    // the growing arenas: run.ed_out (and run.evid beside it), run.pile_site, run.sr_site / sr_code.  The status block
    // holds 16 bytes for the edits' total, then 16 for the sites', whose second word is the entries'
    GrowArena ed_arena{"edits", DG_E_ED_OVF, true, &DgParams::ed_top, &DgParams::ed_cap};
    GrowArena site_arena{"sites", DG_E_SITE_OVF, true, &DgParams::site_top, &DgParams::site_cap};
    GrowArena sr_arena{"site entries", DG_E_SR_OVF, false, &DgParams::sr_top, &DgParams::sr_cap};
    std::array<GrowRef, 3> growing() { return {{{&ed_arena, o_ed.batch}, {&site_arena, o_pile.batch}, {&sr_arena, o_sr.batch}}}; }
    long ed_cap_env = 0;                            // DAGCON_EDITS_CAP (tests): first size of the edit arena, so that the re-run is met

    uint64_t norm_cap = 0, node_cap = 0, pool_cap = 0, cns_cap = 0, seg_cap = 0;
    uint32_t stk_words = 4096, growth_pct = 100, seg_max = 8, bp_max = 16, seg_env = 0, seg_min = 768;    // (scratch per target and segment: grown x4 and re-run on DG_E_STACK)
    uint32_t sh_log = 16;                           // slots per segment behind enter's / exit's list (x2 on DG_E_LOG_OVF)
    bool full_span = false;                         // (nearly) every alignment of the batch covers its whole target
    uint32_t gcuts = 1;                             // partial-span cuts: prologue + worklist + epilogue (DAGCON_GCUTS=0: off)
    uint32_t worklist_cap = 0, list_grid = 8192;    // partial-span worklist: entries, and the waves of k_merge_list

    DgStatus h_st;
    dagcon_timings tm;

    // results (host)
    std::vector<uint64_t> r_seg_begin, r_seq_off;
    std::vector<int32_t> r_range0, r_range1;
    std::vector<uint32_t> r_seq_len;
    PinBuf r_seg;                       // int32_t, grown with the segment arena: seg_r0's first seg_top entries, then seg_r1's
    std::vector<int32_t> r_status;
    PinBuf r_blob;                      // char: the consensus blob
    PinBuf r_sup;                       // uint16_t, DAGCON_FLAG_BASE_SUPPORT: [seq_bytes] weights, then [seq_bytes] depths
    uint64_t r_sup_n = 0;
    std::vector<uint32_t> r_pos;        // DAGCON_FLAG_BASE_POS: [seq_bytes] _bbMap of every consensus base
    bool pos_valid = false;
    bool pos_pending = false;           // edits or the kept parts on: the positions stay on the device until dagcon_fetch_positions asks for them
    uint64_t r_nb = 0;                  // seq_bytes of the last fetch
    PinBuf r_ed;                        // the DgEdSeg records of the last fetch, then its DgEdit records
    PinBuf r_site;                      // the DgSite records of the last fetch
    PinBuf r_pile;                      // uint16_t, eight per position (o_pile.fetched: of the same run; dagcon_fetch_pileup copies them when asked)
    EditsOut r_edits;
    SitesOut r_sites;
    SiteReadsOut r_reads;
    AllelesOut r_alleles;
    JoinedOut r_joined;
    HapOut r_haps;
    WinPhaseOut r_winphase;
    HapCallsOut r_hc;
    HapMapOut r_hapmap;
    KeepOut r_keep;
    SiteLinkOut r_link;
    HostOrder order;
    bool sup_valid = false;             // r_sup holds the support of the results of the last fetch

    // The one place where results stop being valid.  A fetch drops what the fetch before it left; a run drops that and
    // `fetched`; an upload drops that and `uploaded`, `ran` and the rebuilt targets.  One exception to upload > run > fetch:
    // a run alone leaves sup_valid and pos_valid -- r_sup and r_pos are host copies that still hold what the last fetch
    // brought, and stay readable until the next fetch replaces them.  (The outputs' `batch` latches are the upload's own
    // business: latch_outputs.)
    void drop_results(const Fresh lv) {
        for (Output *o : outputs()) o->valid = o->fetched = false;
        pos_pending = r_haps.sites_fetched = order.built = false;
        if (lv != Fresh::RUN) sup_valid = pos_valid = false;
        if (lv != Fresh::FETCH) fetched = false;
        if (lv == Fresh::UPLOAD) uploaded = ran = md_valid = md_fetched = r_hapmap.valid = false;
    }

    // debug dump storage
    std::vector<uint8_t> g_base, g_deleted, g_backbone;
    std::vector<int32_t> g_weight, g_cov, g_bbpos, g_out_dst, g_out_cnt, g_in_src;
    std::vector<uint32_t> g_out_begin, g_in_begin;

    // (the body runs before the members free themselves: nothing of this context is in flight any more when they do)
    ~Ctx() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int fail(Ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, call)                                                                    \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess)                                                              \
            return fail((c), DAGCON_ERR_HIP, "%s failed: %s (%s:%d)", #call,               \
                        hipGetErrorString(_e), __FILE__, __LINE__);                        \
    } while (0)

int ensure(Ctx *c, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return DAGCON_OK;
    b.release();
    size_t want = bytes + bytes / 16 + 256;
    const bool dbg = getenv("DAGCON_ALLOC_TIMING") != nullptr;
    const double t0 = dbg ? std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() : 0;
    hipError_t e = hipMalloc(&b.p, want);
    if (dbg) {
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
        if (dt > 0.005) fprintf(stderr, "dagcon: hipMalloc(%.1f MB) took %.1f ms\n", want / 1e6, dt * 1e3);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, DAGCON_ERR_WORKSPACE, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return DAGCON_OK;
}

#define ENSURE(c, buf, bytes)                                \
    do {                                                     \
        int _r = ensure((c), (buf), (size_t)(bytes));        \
        if (_r != DAGCON_OK) return _r;                      \
    } while (0)

// room for n entries, then the host's n entries on their way there on the context's stream (n == 0: no copy)
template <typename X>
int upload(Ctx *c, DevBuf &b, const X *host, size_t n) {
    ENSURE(c, b, n * sizeof(X));
    if (n) HIPCHK(c, hipMemcpyAsync(b.p, host, n * sizeof(X), hipMemcpyHostToDevice, c->stream));
    return DAGCON_OK;
}
template <typename X>
int upload(Ctx *c, DevBuf &b, const std::vector<X> &v) { return upload(c, b, v.data(), v.size()); }

// device -> host on the context's own stream.  (hipMemcpy would go through the null stream, and the stream is
// non-blocking so that a second context on the same GPU is not serialised against this one's copies.)
hipError_t d2h(Ctx *c, void *dst, const void *src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

#define UPLOAD(c, buf, ...)                                  \
    do {                                                     \
        int _r = upload((c), (buf), __VA_ARGS__);            \
        if (_r != DAGCON_OK) return _r;                      \
    } while (0)

// one headroom for every page-locked buffer, in bytes: not below any of the five it replaces (the largest was the
// support's, 4 x (n + n / 8 + 4096))
int PinBuf::reserve(Ctx *c, size_t bytes) {
    if (cap >= bytes) return DAGCON_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 8 + 16384;
    HIPCHK(c, hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
    return DAGCON_OK;
}
}  // namespace
