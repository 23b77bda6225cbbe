// dagcon_api.hip -- host side of the C ABI (include/dagcon.h).
//
// Owns the HIP stream, the HBM arenas and the launch sequence of the hot path
//   a1 k_norm_*             | a2 k_carve, k_groups, k_emit, k_lists |
//   b  k_merge              | c  k_bestpath
// There is no CPU fallback anywhere in this file: without a HIP device
// dagcon_create fails with DAGCON_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <array>
#include <vector>

#include "../../include/dagcon.h"
#include "dagcon_dev.h"
#include "k_build.hip.h"
#include "k_merge.hip.h"
#include "k_merge_q.hip.h"
#include "k_bestpath.hip.h"
#include "k_align.hip.h"
#include "k_align_panels.hip.h"
#include "k_place.hip.h"
#include "k_cigar.hip.h"
#include "k_rate.hip.h"
#include "k_cs.hip.h"
#include "k_edits.hip.h"

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// the device buffers of the record intake, by name; all() is what dagcon_destroy frees
struct CigarBufs {
    DevBuf ops, op_begin, tile_begin, totals, ckpt;                // the records' ops, k_cigar_scan's output
    DevBuf q, t, q_off, t_base;                                    // the blobs and where each record's bases begin
    DevBuf out_off;                                                // whole targets: where each record's strings go
    DevBuf piece, cut, wave_piece, wave_begin, piece_out;          // windows: DgCigarCutParams
    DevBuf rev, q_len;                                             // DgCigarStrand
    DevBuf rate_base, tile_rate, rate;                             // DgCigarRate (a record filter is set)
    std::array<DevBuf *, 20> all() {
        return {&ops, &op_begin, &tile_begin, &totals, &ckpt, &q, &t, &q_off, &t_base, &out_off, &piece, &cut, &wave_piece, &wave_begin, &piece_out, &rev, &q_len,
                &rate_base, &tile_rate, &rate};
    }
};
static_assert(sizeof(CigarBufs) == 20 * sizeof(DevBuf), "CigarBufs::all() must name every member");
// dagcon_upload_cs: the text and what k_cs_scan / k_cs_write take besides CigarBufs::ops, q and t, which k_cs_write fills
struct CsBufs {
    DevBuf text, cs_off, cs_len, totals, n_ops, op_begin, t_base, t_room, q_off, q_len;
    std::array<DevBuf *, 10> all() { return {&text, &cs_off, &cs_len, &totals, &n_ops, &op_begin, &t_base, &t_room, &q_off, &q_len}; }
};
static_assert(sizeof(CsBufs) == 10 * sizeof(DevBuf), "CsBufs::all() must name every member");

// ---- how many pieces the merge / bestPath sweeps of a batch are cut into (host arithmetic only: exported as
// dagcon_debug_plan so that a CPU test can sweep it; every grid size derived from it is > 0) ----
#define DQ_KMAX 52u      // reads per target up to which the row sweep (k_merge_q, rows of 8 lanes) beats the wave sweep (k_merge):
                         // 600 targets x 6 kb at 40x / 50x / 60x / 70x: 6.5 / 8.4 / 11.6 / 20.0 ms against 7.1 / 8.4 / 9.7 / 11.2 (tools/kmax_probe.py)
struct DgPlanIn { uint32_t T; uint64_t n_alns, sum_bb; uint32_t gcuts, max_segments, min_segment_len, seg_env, merge_q; };
struct DgPlan { uint32_t seg_max, seg_min, use_q, bp_max; };
static DgPlan dg_plan_pieces(const DgPlanIn &in) {
    DgPlan pl;
    const uint32_t T = in.T;
    // shortest stretch worth a worker: 768 positions when that already fills the chip, shorter (down to 192)
    // for small batches, whose waves would otherwise be few and long
    pl.seg_min = in.min_segment_len;
    if (!pl.seg_min) pl.seg_min = (uint32_t)std::min<uint64_t>(768, std::max<uint64_t>(192, in.sum_bb / 8192));
    // merge workers per target: about one chip's worth of resident waves (8 per SIMD x 1024
    // SIMDs) over the batch, never fewer than 8 nor more than 256 per target
    if (in.max_segments) pl.seg_max = in.max_segments > 64u ? 64u : in.max_segments;
    else if (in.seg_env) pl.seg_max = in.seg_env;
    else if (in.gcuts) pl.seg_max = 64;      // the worklist of k_cuts2 is taken by ticket: the finer its entries the better
                                             // the balance (config-5 shape, 1,000 targets: 8 / 32 / 64 pieces 54 / 34 / 31 ms)
    else { uint32_t sm = T ? 8192u / T : 8u; pl.seg_max = sm < 8u ? 8u : sm > 256u ? 256u : sm; }
    if (in.gcuts && !in.min_segment_len) pl.seg_min = 256;
    // k_merge_q (DQ_ROWS segments per wave, DQ_WAVES waves per SIMD) for full-span batches big enough to fill the chip with
    // it: as many pieces as go (<= 256 per target) with its waves filling the chip a whole number of times -- a last round
    // that is a third full costs as much as a full one (configs[1]: 36 / 49 / 56 / 64 pieces 20.6 / 17.4 / 19.2 / 18.3 ms)
    pl.use_q = 0;
    if (in.merge_q && !in.gcuts && pl.seg_max != 1) {
        const uint32_t slots = 1024u * DQ_WAVES;
        if (in.max_segments || in.seg_env) pl.use_q = 1;                            // (the caller's number of pieces)
        // a row holds 4 + 4 list entries in its one-look path and 8 in the generic one: past ~50 reads per target
        // too many visits outgrow it (DQ_KMAX)
        else if (T && in.n_alns <= (uint64_t)DQ_KMAX * T) {
            // pieces a target can give: up to 256, one per 128 positions of the average backbone
            const uint64_t avail = std::min<uint64_t>(256, std::max<uint64_t>(1, in.sum_bb / T / 128));
            const uint64_t k = (uint64_t)T * avail / DQ_ROWS / slots;                     // whole rounds at that many pieces
            if (k >= 1 || (uint64_t)T * avail / DQ_ROWS * 10u >= 6u * slots) {            // (or one round six tenths full)
                // (very many short targets -- more targets than a round has rows: unless every target gets at
                // least two pieces the wave-per-segment kernel keeps the batch)
                const uint64_t sm = std::min<uint64_t>(avail, std::max<uint64_t>(k, 1) * slots * DQ_ROWS / T);
                if (sm >= 2) { pl.seg_max = (uint32_t)sm; pl.use_q = 1; }
            }
        }
    }
    if (pl.seg_max < 1) pl.seg_max = 1;
    if (pl.use_q && !in.min_segment_len) pl.seg_min = 128;                         // (its pieces are a quarter of a wave's work)
    // bestPath is swept in three times as many pieces: its waves are light (one piece = one
    // sequential sweep when that is asked for)
    // (more than 64 of them only where 64 per target leave the chip short of waves; never on the partial-span path)
    pl.bp_max = pl.seg_max == 1 ? 1u : std::min(in.gcuts || T >= 256u ? 64u : (uint32_t)DG_BP_PIECES, 3u * pl.seg_max);
    if (pl.bp_max < 1) pl.bp_max = 1;
    return pl;
}

// The words the host reads back after every run, as ranges of ONE device buffer (each 16-byte aligned): what a run starts
// from zero first -- DgStatus, tfail[T + 1], cns_len[T], n_seg[T]: one memset -- then cns_off[T] and seg_first[T].  The whole
// block comes back in one copy into `host`, its page-locked mirror (dagcon_fetch reads the mirror in place).
struct StatBlock {
    DevBuf dev;
    char *host = nullptr;
    size_t host_cap = 0;
    size_t o_tfail = 0, o_cns_len = 0, o_n_seg = 0, o_cns_off = 0, o_seg_first = 0;     // (DgStatus at 0)
    size_t o_ed_top = 0;                            // edits of the batch, behind seg_first (a batch with edits on only; 0: none)
    size_t zero_bytes = 0, bytes = 0;
    template <typename X> X *d(size_t off) const { return reinterpret_cast<X *>(static_cast<char *>(dev.p) + off); }
    template <typename X> const X *h(size_t off) const { return reinterpret_cast<const X *>(host + off); }
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
    bool wide_cells = false;                        // this upload met an insertion run of more than 255 columns: 32-bit matC cells
    std::vector<uint8_t> h_tactive;
    std::vector<uint32_t> h_ch_base, h_ch_aln;      // chunk tables of k_norm_*
    std::vector<uint64_t> h_norm_off;               // column buffer of each alignment
    std::vector<uint32_t> h_ck_base;                // first k_emit checkpoint of each alignment
    uint64_t n_ckpt = 0;
    uint32_t emit_shift = 9;                        // 512 backbone positions per k_emit wave
    uint32_t n_chunks = 0;
    uint64_t tmp_main = 0, tmp_cap = 0;

    // device buffers
    DevBuf d_q, d_t, d_aln_off, d_aln_len, d_aln_start, d_aln_tgt, d_tlen, d_aln_begin, d_tactive,
        d_bb, d_bb_off, d_mat_base, d_bbv_base, d_matc_base, d_matc_stride;
    DevBuf d_nmis, d_norm_off, d_n_lo, d_n_hi, d_n_start, d_n_ins, d_n_del, d_norm;
    DevBuf d_ch_aln, d_ch_base, d_ch_k0, d_ch_next, d_ch_w, d_ch_tb, d_ch_flag, d_ch_src, d_ch_out, d_ch_adv,
        d_n_lb, d_norm_tmp, d_ckpt, d_ck_base;
    DevBuf d_node_base, d_n_nodes, d_pool_base, d_pool_size, d_pool_top, d_t_nins;
    DevBuf d_matA, d_matD, d_matC, d_cov, d_gcount, d_gbase, d_bid;
    DevBuf d_nodes, d_best, d_queue, d_score, d_cns_tmp, d_bp_tt, d_score_b;
    DevBuf d_pool, d_stk, d_cuts, d_cuts_bp, d_bp_stat, d_bp_len, d_worklist, d_rd, d_pro_state, d_sh_cnt, d_seg_done, d_wl_first, d_queue0, d_bp_end, d_bp_ab, d_defer, d_cns_tmp0;
    DevBuf d_al[15];                                // dagcon_align: blobs, offsets, outputs, directions, launch order, widths, ends
    DevBuf d_pn[18];                                // dagcon_align_panels: blobs, panels, scratch, outputs, launch order
    DevBuf d_pl[14];                                // dagcon_place: blob, sequences, tables, pairs, outputs
    CsBufs cs;                                      // dagcon_upload_cs
    CigarBufs cg;                                   // dagcon_upload_cigar and its kin
    std::vector<uint8_t> h_cig_bad;                 // dagcon_upload_cigar: targets with a non-conforming record (empty: another upload)
    std::string cig_err;                            // the first of them, for dagcon_last_error
    bool filter_on = false;                         // dagcon_set_record_filter: the record intake rates and picks its records
    dagcon_record_filter filter = {1000000u, 0u};
    bool rs_valid = false;                          // the record stats below are those of the last upload (dagcon_fetch_record_stats)
    std::vector<uint32_t> rs_match, rs_mismatch, rs_ins, rs_del;
    std::vector<uint8_t> rs_fate;
    DevBuf d_cns;
    StatBlock sb;                                   // DgStatus, tfail, cns_len, n_seg, cns_off, seg_first
    DevBuf d_seg;                                   // seg_r0[seg_cap], then seg_r1 at seg_stride() entries
    DevBuf d_pos_tmp, d_pos_tmp0, d_pos;           // DAGCON_FLAG_BASE_POS: walk scratch (4 B per vertex), output (4 B per base)
    DevBuf d_sup_tmp, d_sup_tmp0, d_sup;           // DAGCON_FLAG_BASE_SUPPORT: walk scratch (4 B per vertex), output (2 x 2 B per base)
    // dagcon_set_edits: the switch; whether the batch on the device is a record upload made under it; its buffers
    // (a DgEdSeg per segment, a DgEdit per edit, where each target's bases begin in cg.t)
    bool edits_on = false, ed_batch = false;
    DevBuf d_ed_seg, d_ed_out, d_ed_tbase;
    std::vector<uint64_t> h_ed_tbase;
    uint64_t ed_cap = 0;
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
    int32_t *r_seg = nullptr;           // page-locked, grown with the segment arena: seg_r0's first seg_top entries, then seg_r1's
    size_t r_seg_cap = 0;               // (entries of each half)
    std::vector<int32_t> r_status;
    char *r_blob = nullptr;             // page-locked: the consensus blob comes back at PCIe speed
    size_t r_blob_cap = 0;
    uint16_t *r_sup = nullptr;          // page-locked, DAGCON_FLAG_BASE_SUPPORT: [seq_bytes] weights, then [seq_bytes] depths
    size_t r_sup_cap = 0;               // (entries of each half)
    uint64_t r_sup_n = 0;
    std::vector<uint32_t> r_pos;        // DAGCON_FLAG_BASE_POS: [seq_bytes] _bbMap of every consensus base
    bool pos_valid = false;
    bool pos_pending = false;           // edits on: the positions stay on the device until dagcon_fetch_positions asks for them
    uint64_t r_nb = 0;                  // seq_bytes of the last fetch
    char *r_ed = nullptr;               // page-locked: the DgEdSeg records of the last fetch, then its DgEdit records
    size_t r_ed_cap = 0;
    bool ed_valid = false;              // the arrays below are those of the last fetch (dagcon_fetch_edits)
    std::vector<uint32_t> e_t0, e_t1, e_tpos, e_tlen, e_clen;
    std::vector<uint64_t> e_begin, e_coff;
    bool sup_valid = false;             // r_sup holds the support of the results of the last fetch

    // debug dump storage
    std::vector<uint8_t> g_base, g_deleted, g_backbone;
    std::vector<int32_t> g_weight, g_cov, g_bbpos, g_out_dst, g_out_cnt, g_in_src;
    std::vector<uint32_t> g_out_begin, g_in_begin;
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
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
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

template <typename T>
int upload_vec(Ctx *c, DevBuf &b, const std::vector<T> &v) {
    ENSURE(c, b, v.size() * sizeof(T));
    if (!v.empty()) HIPCHK(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return DAGCON_OK;
}

void free_buf(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

size_t seg_stride(const Ctx *c) { return ((size_t)c->seg_cap + 3) & ~(size_t)3; }      // entries between seg_r0 and seg_r1 (16-byte aligned)

// bytes of a matC cell: a byte where the cells stay run lengths (p.emit_scan) and no run of this upload has outgrown it
bool matc_wide(const Ctx *c) { return c->max_k > 64u || c->wide_cells; }
size_t matc_bytes(const Ctx *c) { return (size_t)c->matc_cells * (matc_wide(c) ? 4u : 1u); }

// the status block of a batch of T targets and its mirror
int ensure_stat(Ctx *c, uint32_t T) {
    StatBlock &b = c->sb;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    b.o_tfail = up16(sizeof(DgStatus));
    b.o_cns_len = b.o_tfail + up16(((size_t)T + 1) * 4);
    b.o_n_seg = b.o_cns_len + up16((size_t)T * 4);
    b.zero_bytes = b.o_n_seg + up16((size_t)T * 4);
    b.o_cns_off = b.zero_bytes;
    b.o_seg_first = b.o_cns_off + up16((size_t)T * 8);
    b.bytes = b.o_seg_first + up16((size_t)T * 8);
    b.o_ed_top = 0;
    if (c->ed_batch) { b.o_ed_top = b.bytes; b.bytes += 16; }
    ENSURE(c, b.dev, b.bytes);
    if (b.host_cap < b.bytes) {
        if (b.host) (void)hipHostFree(b.host);
        b.host = nullptr; b.host_cap = 0;
        const size_t want = b.bytes + b.bytes / 8 + 4096;
        HIPCHK(c, hipHostMalloc((void **)&b.host, want, hipHostMallocDefault));
        b.host_cap = want;
    }
    return DAGCON_OK;
}

int ensure_arenas(Ctx *c) {
    ENSURE(c, c->d_norm, c->norm_cap * sizeof(uint16_t));
    ENSURE(c, c->d_nodes, c->node_cap * sizeof(DgNode));
    ENSURE(c, c->d_best, c->node_cap * 4);
    ENSURE(c, c->d_queue, c->node_cap * 4);
    ENSURE(c, c->d_score, c->node_cap * 8);
    ENSURE(c, c->d_bp_tt, c->node_cap * 4);
    if (c->gcuts) ENSURE(c, c->d_score_b, c->node_cap * 4);
    ENSURE(c, c->d_cns_tmp, c->node_cap);
    ENSURE(c, c->d_pool, c->pool_cap * 4);
    ENSURE(c, c->d_stk, std::max<uint64_t>((uint64_t)c->T * std::max(c->bp_max, c->seg_max), c->gcuts ? c->list_grid : 0) * c->stk_words * 4);
    if (c->gcuts) {
        ENSURE(c, c->d_worklist, (4ull + 3ull * c->worklist_cap) * 4);
        ENSURE(c, c->d_rd, (uint64_t)c->A * 16 + 16);
        ENSURE(c, c->d_pro_state, (uint64_t)c->T * 16 + 16);
        ENSURE(c, c->d_sh_cnt, (uint64_t)c->T * (2 + 2 * DG_SH_MAX) * 4 + 16);
        ENSURE(c, c->d_seg_done, (uint64_t)c->worklist_cap * (DG_SH_MAX + 1) * 4 + 16);
        ENSURE(c, c->d_wl_first, (uint64_t)c->T * 4 + 16);
        ENSURE(c, c->d_queue0, c->node_cap * 4);
        ENSURE(c, c->d_bp_end, (uint64_t)c->T * c->bp_max * 4 + 16);
        ENSURE(c, c->d_bp_ab, (uint64_t)c->T * c->bp_max * 16 + 16);
        ENSURE(c, c->d_defer, (uint64_t)c->T * (DG_DEFER_MAX + 1) * 4 + 16);
        ENSURE(c, c->d_cns_tmp0, c->node_cap);
    }
    ENSURE(c, c->d_cuts, (uint64_t)c->T * (c->seg_max + 2) * 4);
    ENSURE(c, c->d_cuts_bp, (uint64_t)c->T * (c->bp_max + 2) * 4);
    ENSURE(c, c->d_bp_stat, (uint64_t)c->T * c->bp_max * 8);
    ENSURE(c, c->d_bp_len, (uint64_t)c->T * c->bp_max * 4);
    ENSURE(c, c->d_cns, c->cns_cap);
    if (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT) {
        ENSURE(c, c->d_sup_tmp, c->node_cap * 4);
        if (c->gcuts) ENSURE(c, c->d_sup_tmp0, c->node_cap * 4);
        ENSURE(c, c->d_sup, c->cns_cap * 4);
    }
    if (c->opts.flags & DAGCON_FLAG_BASE_POS) {
        ENSURE(c, c->d_pos_tmp, c->node_cap * 4);
        if (c->gcuts) ENSURE(c, c->d_pos_tmp0, c->node_cap * 4);
        ENSURE(c, c->d_pos, c->cns_cap * 4);
    }
    if (c->ed_batch) {
        ENSURE(c, c->d_ed_seg, c->seg_cap * sizeof(DgEdSeg));
        ENSURE(c, c->d_ed_out, c->ed_cap * sizeof(DgEdit));
    }
    ENSURE(c, c->d_seg, 2 * seg_stride(c) * 4);
    if (c->r_seg_cap < c->seg_cap) {
        if (c->r_seg) (void)hipHostFree(c->r_seg);
        c->r_seg = nullptr; c->r_seg_cap = 0;
        const size_t want = (size_t)c->seg_cap + (size_t)(c->seg_cap / 8) + 1024;
        HIPCHK(c, hipHostMalloc((void **)&c->r_seg, 2 * want * 4, hipHostMallocDefault));
        c->r_seg_cap = want;
    }
    ENSURE(c, c->d_matC, matc_bytes(c) + 256);          // (grows for the re-run with 32-bit cells)
    return DAGCON_OK;
}

void fill_params(Ctx *c, DgParams &p) {
    memset(&p, 0, sizeof p);
    p.q = (const uint8_t *)c->d_q.p; p.t = (const uint8_t *)c->d_t.p;
    p.aln_off = (const uint64_t *)c->d_aln_off.p;
    p.aln_len = (const uint32_t *)c->d_aln_len.p;
    p.aln_start = (const uint32_t *)c->d_aln_start.p;
    p.aln_tgt = (const uint32_t *)c->d_aln_tgt.p;
    p.tlen = (const uint32_t *)c->d_tlen.p;
    p.aln_begin = (const uint64_t *)c->d_aln_begin.p;
    p.tactive = (const uint8_t *)c->d_tactive.p; p.tfail = c->sb.d<uint32_t>(c->sb.o_tfail);
    p.bb = c->have_bb ? (const uint8_t *)c->d_bb.p : nullptr;
    p.bb_off = (const uint64_t *)c->d_bb_off.p;
    p.mat_base = (const uint64_t *)c->d_mat_base.p;
    p.matc_base = (const uint64_t *)c->d_matc_base.p; p.matc_stride = (const uint32_t *)c->d_matc_stride.p;
    p.bbv_base = (const uint64_t *)c->d_bbv_base.p;
    p.T = c->T; p.A = c->A;
    p.trim = c->opts.trim; p.min_len = c->opts.min_len;
    p.min_weight = c->opts.min_weight < 0 ? (int32_t)c->opts.min_cov : c->opts.min_weight;
    p.flags = c->opts.flags;
    p.max_k = c->max_k; p.max_tlen = c->max_tlen;
    p.nmis = (uint32_t *)c->d_nmis.p; p.norm_off = (uint64_t *)c->d_norm_off.p;
    p.n_lo = (uint32_t *)c->d_n_lo.p; p.n_hi = (uint32_t *)c->d_n_hi.p;
    p.n_start = (uint32_t *)c->d_n_start.p; p.n_ins = (uint32_t *)c->d_n_ins.p;
    p.n_del = (uint32_t *)c->d_n_del.p;
    p.norm = (uint16_t *)c->d_norm.p; p.norm_cap = c->norm_cap;
    p.ch_aln = (const uint32_t *)c->d_ch_aln.p; p.ch_base = (const uint32_t *)c->d_ch_base.p;
    p.n_chunks = c->n_chunks;
    p.ch_k0 = (uint32_t *)c->d_ch_k0.p; p.ch_next = (uint32_t *)c->d_ch_next.p;
    p.ch_w = (uint32_t *)c->d_ch_w.p; p.ch_tb = (uint32_t *)c->d_ch_tb.p;
    p.ch_flag = (uint32_t *)c->d_ch_flag.p; p.ch_src = (uint64_t *)c->d_ch_src.p;
    p.ch_out = (uint32_t *)c->d_ch_out.p; p.ch_adv = (uint32_t *)c->d_ch_adv.p;
    p.n_lb = (uint32_t *)c->d_n_lb.p; p.norm_tmp = (uint16_t *)c->d_norm_tmp.p;
    p.tmp_main = c->tmp_main; p.tmp_cap = c->tmp_cap;
    p.ckpt = (uint32_t *)c->d_ckpt.p; p.ck_base = (const uint32_t *)c->d_ck_base.p; p.emit_shift = c->emit_shift;
    p.node_base = (uint64_t *)c->d_node_base.p; p.n_nodes = (uint32_t *)c->d_n_nodes.p;
    p.pool_base = (uint64_t *)c->d_pool_base.p; p.pool_size = (uint32_t *)c->d_pool_size.p;
    p.pool_top = (uint32_t *)c->d_pool_top.p; p.t_nins = (uint32_t *)c->d_t_nins.p;
    p.matA = (uint32_t *)c->d_matA.p; p.matD = (uint32_t *)c->d_matD.p; p.matC = c->d_matC.p;
    p.cov = (int32_t *)c->d_cov.p; p.gcount = (uint32_t *)c->d_gcount.p;
    p.gbase = (uint32_t *)c->d_gbase.p; p.bid = (uint32_t *)c->d_bid.p;
    p.nodes = (DgNode *)c->d_nodes.p; p.best = (int32_t *)c->d_best.p;
    p.queue = (int32_t *)c->d_queue.p; p.score = (float2 *)c->d_score.p; p.bp_tt = (float *)c->d_bp_tt.p;
    p.cns_tmp = (uint8_t *)c->d_cns_tmp.p; p.node_cap = c->node_cap;
    p.pool = (uint32_t *)c->d_pool.p; p.pool_cap = c->pool_cap;
    p.stk = (int32_t *)c->d_stk.p; p.stk_words = c->stk_words; p.growth_pct = c->growth_pct;
    p.score_b = (float *)c->d_score_b.p;
    // (rows pay where there are pieces enough to fill the chip with them, eight to a wave: 64 targets x 50 kb x 60x, 16,384
    // pieces: 2.9 ms by rows against 2.3 by waves; configs[1], 147,000 pieces: 3.8 against 4.7.  DAGCON_BP_LANE=2: always)
    p.bp_lane = c->bp_lane >= 2 || (c->bp_lane && (uint64_t)c->T * c->bp_max >= 32768ull) ? 1u : 0u; p.bl_stk = c->bl_stk >= 0 && c->bl_stk < DG_BL_STK ? (uint32_t)c->bl_stk : (uint32_t)DG_BL_STK;
    p.emit_scan = c->max_k <= 64u ? 1u : 0u;
    p.fold = (c->fold && !(c->opts.flags & DAGCON_FLAG_STOP_AFTER_BUILD)) ? 1u : 0u;
    p.q_kmax = c->use_q && !c->opts.max_segments && !c->seg_env && c->max_k > DQ_KMAX ? DQ_KMAX : 0u;
    p.bp_seg_min = (c->seg_min + 2u) / 3u;
    p.seg_max = c->seg_max; p.seg_min = c->seg_min; p.cuts = (uint32_t *)c->d_cuts.p; p.bp_max = c->bp_max; p.cuts_bp = (uint32_t *)c->d_cuts_bp.p; p.bp_stat = (float *)c->d_bp_stat.p; p.bp_len = (uint32_t *)c->d_bp_len.p;
    p.gcuts = c->gcuts; p.sh_log = c->sh_log;
    p.rd_s = (uint32_t *)c->d_rd.p; p.rd_e = p.rd_s + c->A; p.rd_lead = p.rd_e + c->A; p.rd_trail = p.rd_lead + c->A;
    p.pro_state = (uint32_t *)c->d_pro_state.p; p.sh_cnt = (uint32_t *)c->d_sh_cnt.p;
    p.queue0 = (int32_t *)c->d_queue0.p; p.bp_end = (uint32_t *)c->d_bp_end.p; p.bp_ab = (float *)c->d_bp_ab.p;
    p.defer = (uint32_t *)c->d_defer.p; p.cns_tmp0 = (uint8_t *)c->d_cns_tmp0.p;
    p.seg_done = (uint32_t *)c->d_seg_done.p; p.wl_first = (uint32_t *)c->d_wl_first.p;
    p.worklist = (uint32_t *)c->d_worklist.p; p.worklist_cap = c->worklist_cap;
    p.cns = (uint8_t *)c->d_cns.p; p.cns_cap = c->cns_cap;
    p.cns_off = c->sb.d<uint64_t>(c->sb.o_cns_off); p.cns_len = c->sb.d<uint32_t>(c->sb.o_cns_len);
    p.seg_first = c->sb.d<uint64_t>(c->sb.o_seg_first); p.n_seg = c->sb.d<uint32_t>(c->sb.o_n_seg);
    p.seg_r0 = (int32_t *)c->d_seg.p; p.seg_r1 = p.seg_r0 + seg_stride(c);
    p.seg_cap = c->seg_cap;
    p.st = c->sb.d<DgStatus>(0);
    if (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT) {
        p.sup_tmp = (uint32_t *)c->d_sup_tmp.p; p.sup_tmp0 = (uint32_t *)c->d_sup_tmp0.p;
        p.sup_w = (uint16_t *)c->d_sup.p; p.sup_d = p.sup_w + c->cns_cap;
    }
    if (c->opts.flags & DAGCON_FLAG_BASE_POS) {
        p.pos_tmp = (uint32_t *)c->d_pos_tmp.p; p.pos_tmp0 = (uint32_t *)c->d_pos_tmp0.p; p.pos_out = (uint32_t *)c->d_pos.p;
    }
    if (c->ed_batch) {
        p.ed_seg = (DgEdSeg *)c->d_ed_seg.p; p.ed_out = (DgEdit *)c->d_ed_out.p; p.ed_cap = c->ed_cap;
        p.ed_top = c->sb.d<unsigned long long>(c->sb.o_ed_top);
        p.ed_t = (const uint8_t *)c->cg.t.p; p.ed_tbase = (const uint64_t *)c->d_ed_tbase.p;
    }
}

// stage a1: count, chunked normalizeGaps + trimAln, and the sequential kernel for what is left
// (wide: the matC writers' 32-bit instances)
void launch_normalize(Ctx *c, const DgParams &p, const bool wide) {
    hipStream_t s = c->stream;
    if (c->A == 0) return;
    (void)hipMemsetAsync(c->d_ckpt.p, 0xFF, c->n_ckpt * 4, s);
    hipLaunchKernelGGL((k_norm_chunk<DG_NW, 64, false>), dim3((c->n_chunks + 63) / 64), dim3(64), 0, s, p);
    hipLaunchKernelGGL((k_norm_chunk<DG_NW_BIG, 32, true>), dim3((c->n_chunks + 31) / 32), dim3(32), 0, s, p);
    hipLaunchKernelGGL(k_norm_scan, dim3((c->A + 63) / 64), dim3(64), 0, s, p);
    if (wide) {
        hipLaunchKernelGGL(k_norm_finish2<uint32_t>, dim3((c->n_chunks + 3) / 4), dim3(256), 0, s, p);    // a wave per chunk
        hipLaunchKernelGGL(k_normalize_slow<uint32_t>, dim3((c->A + 63) / 64), dim3(64), 0, s, p);
    } else {
        hipLaunchKernelGGL(k_norm_finish2<uint8_t>, dim3((c->n_chunks + 3) / 4), dim3(256), 0, s, p);
        hipLaunchKernelGGL(k_normalize_slow<uint8_t>, dim3((c->A + 63) / 64), dim3(64), 0, s, p);
    }
}

int launch_all(Ctx *c) {
    int r = ensure_arenas(c);
    if (r != DAGCON_OK) return r;
    DgParams p;
    fill_params(c, p);
    hipStream_t s = c->stream;
    const bool wide = matc_wide(c);                       // (!p.emit_scan, or a run of this upload outgrew a byte)
    if (c->poison & 8) {
        // every buffer the kernels themselves fill (nothing the host uploaded), before the memsets below: whoever reads an
        // entry of them that THIS run has not written finds 0xEE bytes, in a fresh process as in one that re-uses its memory
        DevBuf *work[] = {&c->d_nmis, &c->d_n_lo, &c->d_n_hi, &c->d_n_start, &c->d_n_ins, &c->d_n_del, &c->d_ch_k0, &c->d_ch_next, &c->d_ch_w,
                          &c->d_ch_tb, &c->d_ch_flag, &c->d_ch_src, &c->d_ch_out, &c->d_ch_adv, &c->d_n_lb, &c->d_norm_tmp, &c->d_ckpt,
                          &c->d_node_base, &c->d_n_nodes, &c->d_pool_base, &c->d_pool_size, &c->d_pool_top, &c->d_t_nins, &c->d_cov, &c->d_gcount,
                          &c->d_gbase, &c->d_bid, &c->d_best, &c->d_queue, &c->d_score, &c->d_cns_tmp, &c->d_bp_tt, &c->d_stk, &c->d_cuts,
                          &c->d_cuts_bp, &c->d_bp_stat, &c->d_bp_len, &c->d_rd, &c->d_pro_state, &c->d_sh_cnt, &c->d_wl_first,
                          &c->d_queue0, &c->d_bp_end, &c->d_bp_ab, &c->d_defer, &c->d_cns_tmp0, &c->d_cns,
                          &c->d_seg, &c->d_worklist, &c->d_seg_done, &c->d_sup_tmp, &c->d_sup_tmp0, &c->d_sup, &c->d_pos_tmp, &c->d_pos_tmp0, &c->d_pos,
                          &c->d_ed_seg, &c->d_ed_out};
        for (DevBuf *b : work)
            if (b->p && b->cap) HIPCHK(c, hipMemsetAsync(b->p, 0xEE, b->cap, s));
        // (cns_off and seg_first: the part of the status block that is not cleared below)
        if (c->sb.bytes > c->sb.zero_bytes) HIPCHK(c, hipMemsetAsync(c->sb.d<char>(c->sb.zero_bytes), 0xEE, c->sb.bytes - c->sb.zero_bytes, s));
    }
    HIPCHK(c, hipMemsetAsync(c->sb.dev.p, 0, c->sb.zero_bytes, s));      // DgStatus, tfail, cns_len, n_seg
    if (c->matc_cells) HIPCHK(c, hipMemsetAsync(c->d_matC.p, 0, matc_bytes(c), s));
    if (c->poison) {
        // what no kernel is supposed to read before it has been written in THIS run: a process that re-uses its
        // arenas (another context's freed memory, the batch before) finds old cells there, not the zeros of a fresh one
        if ((c->poison & 1) && c->d_matA.p) { HIPCHK(c, hipMemsetAsync(c->d_matA.p, 0xEE, c->d_matA.cap, s)); HIPCHK(c, hipMemsetAsync(c->d_matD.p, 0xEE, c->d_matD.cap, s)); }
        if ((c->poison & 2) && c->d_nodes.p) { HIPCHK(c, hipMemsetAsync(c->d_nodes.p, 0xEE, c->d_nodes.cap, s)); HIPCHK(c, hipMemsetAsync(c->d_pool.p, 0xEE, c->d_pool.cap, s)); }
        if ((c->poison & 4) && c->d_score_b.p) HIPCHK(c, hipMemsetAsync(c->d_score_b.p, 0xEE, c->d_score_b.cap, s));
        if ((c->poison & 4) && c->d_norm.p) HIPCHK(c, hipMemsetAsync(c->d_norm.p, 0xEE, c->d_norm.cap, s));
    }
    HIPCHK(c, hipEventRecord(c->ev[0], s));
    launch_normalize(c, p, wide);
    HIPCHK(c, hipEventRecord(c->ev[1], s));
    // (matA / matD are not cleared: k_emit writes every cell of every row)
    hipLaunchKernelGGL(k_carve, dim3(1), dim3(1024), 0, s, p);
    if (c->T > 0) {
        const uint32_t rows4 = (c->max_tlen + 2 + 4 * DG_LPW - 1) / (4 * DG_LPW);   // 4 waves x DG_LPW positions per block
        if (c->gcuts && c->A > 0) hipLaunchKernelGGL(k_readspan, dim3((c->A + 63) / 64), dim3(64), 0, s, p);   // (before matC becomes prefix sums)
        if (p.emit_scan && wide) hipLaunchKernelGGL(k_gsum<uint32_t>, dim3(c->T, (c->max_tlen + 2 + 255) / 256), dim3(256), 0, s, p);
        else if (p.emit_scan) hipLaunchKernelGGL(k_gsum<uint8_t>, dim3(c->T, (c->max_tlen + 2 + 1023) / 1024), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(k_groups, dim3(c->T, (c->max_tlen + 2 + 31) / 32), dim3(256), 0, s, p);
        hipLaunchKernelGGL(k_gscan, dim3(c->T), dim3(1024), 0, s, p);
        if (c->A > 0) {
            const dim3 eg(c->T, (c->max_k + DG_ERPW - 1) / DG_ERPW, ((c->max_tlen + 2) >> c->emit_shift) + 1);
            if (wide) hipLaunchKernelGGL(k_emit<uint32_t>, eg, dim3(64), 0, s, p);
            else hipLaunchKernelGGL(k_emit<uint8_t>, eg, dim3(64), 0, s, p);
        }
        const size_t lds = (size_t)4 * 2 * (c->max_k + 2) * sizeof(int32_t);
        if (lds > 65536)
            HIPCHK(c, hipFuncSetAttribute((const void *)k_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_lists, dim3(c->T, rows4), dim3(256), lds, s, p);
    }
    HIPCHK(c, hipEventRecord(c->ev[2], s));
    if (c->T > 0 && !(c->opts.flags & DAGCON_FLAG_STOP_AFTER_BUILD)) {
        if (c->gcuts) {
            // partial-span cuts (k_cuts2 makes its own, bestPath's too): enter and what hangs on it first, then the
            // segments as a worklist, exit last
            HIPCHK(c, hipMemsetAsync(c->d_worklist.p, 0, 16, s));
            HIPCHK(c, hipMemsetAsync(c->d_seg_done.p, 0, (size_t)c->worklist_cap * (DG_SH_MAX + 1) * 4, s));
            hipLaunchKernelGGL(k_merge_pro, dim3(c->T), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_cuts2, dim3(c->T), dim3(64), 0, s, p);
            // the worklist, a wave per entry
            hipLaunchKernelGGL(k_merge_list, dim3(c->list_grid), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_merge_fin, dim3(c->T), dim3(64), 0, s, p);
        } else {
            hipLaunchKernelGGL(k_cuts, dim3(c->T), dim3(64), 0, s, p);
            if (c->use_q) {
                hipLaunchKernelGGL(k_merge_q, dim3((c->T * c->seg_max + DQ_ROWS - 1u) / DQ_ROWS), dim3(64), 0, s, p);
                // (the few deep targets of a shallow batch: the same cuts, a wave per segment)
                if (p.q_kmax) hipLaunchKernelGGL(k_merge, dim3(c->T * c->seg_max), dim3(64), 0, s, p);
            } else hipLaunchKernelGGL(k_merge, dim3(c->T * c->seg_max), dim3(64), 0, s, p);
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[3], s));
    if (c->T > 0 && !(c->opts.flags & (DAGCON_FLAG_STOP_AFTER_BUILD | DAGCON_FLAG_STOP_AFTER_MERGE))) {
        const bool sup = (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT) != 0;   // the walks and the join with per-base support
        const bool pos = (c->opts.flags & DAGCON_FLAG_BASE_POS) != 0;       // ... and with per-base target positions
        // (neither flag: the <false, false> instances, the code of the kernels before either existed)
#define DG_BP_LAUNCH(K, GRID)                                                                          \
        do {                                                                                           \
            if (sup && pos) hipLaunchKernelGGL((K<true, true>), GRID, dim3(64), 0, s, p);              \
            else if (sup) hipLaunchKernelGGL((K<true, false>), GRID, dim3(64), 0, s, p);               \
            else if (pos) hipLaunchKernelGGL((K<false, true>), GRID, dim3(64), 0, s, p);               \
            else hipLaunchKernelGGL((K<false, false>), GRID, dim3(64), 0, s, p);                       \
        } while (0)
        hipLaunchKernelGGL(k_bp_terms, dim3(c->T, 16), dim3(256), 0, s, p);
        if (c->gcuts) {
            // partial-span pileups, on the pieces of k_cuts2: one sweep for (A, B), then vertex-parallel kernels for the
            // absolute scores and the choices; k_bp_sweep_abs_g sweeps whole the targets the pieces do not take
            hipLaunchKernelGGL(k_bp_xtree, dim3(c->T), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_sweep_ab, dim3(c->T * c->bp_max), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_comb, dim3(c->T), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_abs, dim3(c->T * c->bp_max), dim3(256), 0, s, p);
            hipLaunchKernelGGL(k_bp_choose, dim3(c->T * c->bp_max), dim3(256), 0, s, p);
            hipLaunchKernelGGL(k_bp_sweep_abs_g, dim3(c->T * c->bp_max), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_defer, dim3(c->T), dim3(64), 0, s, p);
            DG_BP_LAUNCH(k_bp_walk_g, dim3(c->T * c->bp_max));
        } else {
            // a lane per piece first; the wave-per-piece sweep then takes the pieces a lane gave up (deep recursion)
            if (p.bp_lane) hipLaunchKernelGGL(k_bp_sweep_l, dim3((c->T * c->bp_max + 7u) / 8u), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_sweep, dim3(c->T * c->bp_max), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_check, dim3(c->T), dim3(64), 0, s, p);
            if (p.bp_lane) DG_BP_LAUNCH(k_bp_walk_r, dim3((c->T * c->bp_max + 7u) / 8u));
            else DG_BP_LAUNCH(k_bp_walk, dim3(c->T * c->bp_max));
        }
        DG_BP_LAUNCH(k_bp_join, dim3(c->T));
#undef DG_BP_LAUNCH
        if (c->ed_batch) {
            // the edits (k_edits.hip.h): count, place, write; a wave per segment of the arena (seg_top is the device's)
            const dim3 eg((uint32_t)((c->seg_cap + 3) / 4));
            hipLaunchKernelGGL(k_ed_scan_seg<false>, eg, dim3(256), 0, s, p);
            hipLaunchKernelGGL(k_ed_scan, dim3(1), dim3(1024), 0, s, p);
            hipLaunchKernelGGL(k_ed_scan_seg<true>, eg, dim3(256), 0, s, p);
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[4], s));
    HIPCHK(c, hipGetLastError());
    return DAGCON_OK;
}

}  // namespace

extern "C" {

int dagcon_abi_version(void) { return DAGCON_ABI_VERSION; }

void dagcon_default_opts(dagcon_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_cov = 6; o->min_len = 500; o->trim = 50; o->min_weight = -1; o->device = 0; o->flags = 0;
}

const char *dagcon_last_error(const dagcon_ctx *ctx) {
    return ctx ? reinterpret_cast<const Ctx *>(ctx)->err.c_str() : "null context";
}

int dagcon_create(const dagcon_opts *opts, dagcon_ctx **out) {
    if (!opts || !out) return DAGCON_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DAGCON_ERR_NO_DEVICE;
    if (opts->device < 0 || opts->device >= ndev) return DAGCON_ERR_NO_DEVICE;
    if (opts->flags & ~DAGCON_FLAGS_ALL) return DAGCON_ERR_UNSUPPORTED;   // (internal bits start at 8: never from outside)
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, opts->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return DAGCON_ERR_NO_DEVICE;                      // the code object is gfx950 only
    }
    Ctx *c = new Ctx();
    c->opts = *opts;
    c->device = opts->device;
    if (const char *e = getenv("DAGCON_EMIT_SHIFT")) {      // test knob: k_emit stretches of 1 << v positions
        const int v = atoi(e);
        if (v >= 4 && v <= 20) c->emit_shift = (uint32_t)v;
    }
    if (const char *e = getenv("DAGCON_MERGE_SEGS")) {      // tuning knob: 1 = one worker per target
        const int v = atoi(e);
        if (v >= 1 && v <= 64) c->seg_env = (uint32_t)v;
    }
    if (const char *e = getenv("DAGCON_FOLD")) c->fold = atoi(e) != 0;
    if (const char *e = getenv("DAGCON_POISON")) c->poison = atoi(e);
    if (const char *e = getenv("DAGCON_BP_LANE")) c->bp_lane = atoi(e);
    if (const char *e = getenv("DAGCON_BP_LANE_STACK")) c->bl_stk = atoi(e);
    if (const char *e = getenv("DAGCON_MERGE_Q")) c->merge_q = atoi(e) != 0;     // eight segments per wave (k_merge_q.hip.h)
    if (const char *e = getenv("DAGCON_EDITS_CAP")) c->ed_cap_env = atol(e);
    memset(&c->tm, 0, sizeof c->tm);
    memset(&c->h_st, 0, sizeof c->h_st);
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return DAGCON_ERR_NO_DEVICE;
    }
    for (auto &e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete c; return DAGCON_ERR_HIP; }
    if (ensure_stat(c, 0) != DAGCON_OK) { dagcon_destroy(reinterpret_cast<dagcon_ctx *>(c)); return DAGCON_ERR_WORKSPACE; }
    *out = reinterpret_cast<dagcon_ctx *>(c);
    return DAGCON_OK;
}

void dagcon_destroy(dagcon_ctx *ctx) {
    if (!ctx) return;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->r_blob) (void)hipHostFree(c->r_blob);
    if (c->r_sup) (void)hipHostFree(c->r_sup);
    if (c->r_seg) (void)hipHostFree(c->r_seg);
    if (c->r_ed) (void)hipHostFree(c->r_ed);
    if (c->sb.host) (void)hipHostFree(c->sb.host);
    DevBuf *all[] = {&c->d_q, &c->d_t, &c->d_aln_off, &c->d_aln_len, &c->d_aln_start, &c->d_aln_tgt,
                     &c->d_tlen, &c->d_aln_begin, &c->d_tactive, &c->sb.dev, &c->d_bb, &c->d_bb_off, &c->d_mat_base, &c->d_matc_base, &c->d_matc_stride,
                     &c->d_bbv_base, &c->d_nmis, &c->d_norm_off, &c->d_n_lo, &c->d_n_hi, &c->d_n_start, &c->d_ch_aln, &c->d_ch_base, &c->d_ch_k0, &c->d_ch_next, &c->d_ch_w, &c->d_ch_tb, &c->d_ch_flag, &c->d_ch_src, &c->d_ch_out, &c->d_ch_adv, &c->d_n_lb, &c->d_norm_tmp, &c->d_ckpt, &c->d_ck_base,
                     &c->d_n_ins, &c->d_n_del, &c->d_norm, &c->d_node_base, &c->d_n_nodes,
                     &c->d_pool_base, &c->d_pool_size, &c->d_pool_top, &c->d_t_nins, &c->d_matA, &c->d_matD,
                     &c->d_matC, &c->d_cov, &c->d_gcount, &c->d_gbase, &c->d_bid, &c->d_nodes,
                     &c->d_best, &c->d_queue, &c->d_score, &c->d_cns_tmp, &c->d_bp_tt, &c->d_score_b, &c->d_pool, &c->d_stk, &c->d_cuts, &c->d_cuts_bp, &c->d_bp_stat, &c->d_bp_len, &c->d_worklist, &c->d_rd, &c->d_pro_state, &c->d_sh_cnt, &c->d_seg_done, &c->d_wl_first, &c->d_queue0, &c->d_bp_end, &c->d_bp_ab, &c->d_defer, &c->d_cns_tmp0, &c->d_cns,
                     &c->d_seg, &c->d_sup_tmp, &c->d_sup_tmp0, &c->d_sup, &c->d_pos_tmp, &c->d_pos_tmp0, &c->d_pos,
                     &c->d_ed_seg, &c->d_ed_out, &c->d_ed_tbase};
    for (DevBuf *b : all) free_buf(*b);
    for (DevBuf &b : c->d_al) free_buf(b);
    for (DevBuf &b : c->d_pn) free_buf(b);
    for (DevBuf &b : c->d_pl) free_buf(b);
    for (DevBuf *b : c->cg.all()) free_buf(*b);
    for (DevBuf *b : c->cs.all()) free_buf(*b);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// dev_q / dev_t: the blobs are on the device already (dagcon_consensus_pre: the aligner's output), b->qstr / tstr unused
static int upload_impl(dagcon_ctx *ctx, const dagcon_batch *b, const void *dev_q, const void *dev_t) {
    if (!ctx || !b) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->uploaded = c->ran = c->fetched = false;
    c->sup_valid = c->pos_valid = false;
    c->ed_batch = c->ed_valid = c->pos_pending = false;     // (a record upload with edits on says so after the hand-over)
    c->h_cig_bad.clear();
    c->rs_valid = false;
    c->wide_cells = false;                             // (one batch with a very long insertion run does not slow the ones after it)
    const uint32_t T = b->n_targets;
    if (T && (!b->tlen || !b->aln_begin)) return fail(c, DAGCON_ERR_INVALID_ARG, "tlen/aln_begin is NULL");
    const uint64_t A_all = T ? b->aln_begin[T] : 0;
    if (A_all && (!b->aln_start || !b->aln_off || !b->aln_len || ((!b->qstr || !b->tstr) && !(dev_q && dev_t))))
        return fail(c, DAGCON_ERR_INVALID_ARG, "alignment arrays are NULL");
    if (b->backbone && !b->backbone_off) return fail(c, DAGCON_ERR_INVALID_ARG, "backbone_off is NULL");
    HIPCHK(c, hipSetDevice(c->device));

    c->T = T;
    c->h_tlen.assign(b->tlen, b->tlen + T);
    c->h_aln_begin.assign(T + 1, 0);
    c->h_tactive.assign(T, 0);
    c->h_mat_base.assign(T, 0);
    c->h_matc_base.assign(T, 0); c->h_matc_stride.assign(T, 0); c->matc_cells = 0;
    c->h_bbv_base.assign(T, 0);
    c->h_bb_off.assign(T, 0);
    c->h_aln_len.clear(); c->h_aln_start.clear(); c->h_aln_tgt.clear(); c->h_aln_off.clear();
    c->max_k = 0; c->max_tlen = 0; c->sum_len = 0; c->sum_bb = 0; c->mat_cells = 0;
    c->have_bb = b->backbone != nullptr;
    uint64_t bb_bytes = 0, n_whole = 0;
    const uint64_t min_cov = c->opts.min_cov;
    for (uint32_t t = 0; t < T; t++) {
        const uint64_t ab = b->aln_begin[t], ae = b->aln_begin[t + 1];
        if (ae < ab) return fail(c, DAGCON_ERR_INVALID_ARG, "aln_begin not monotone at target %u", t);
        const uint64_t k_all = ae - ab;
        // main.cpp:66-72 (Reader) and :118 (Consensus): groups below min_cov are dropped
        const bool active = k_all > 0 && k_all >= min_cov;
        c->h_aln_begin[t] = c->h_aln_len.size();
        if (!active) continue;
        if (b->tlen[t] > 0x3FFFFFFFu) return fail(c, DAGCON_ERR_UNSUPPORTED, "tlen of target %u too large", t);
        c->h_tactive[t] = 1;
        for (uint64_t a = ab; a < ae; a++) {
            const uint32_t len = b->aln_len[a];
            if (b->aln_off[a] > b->blob_bytes || len > b->blob_bytes - b->aln_off[a])
                return fail(c, DAGCON_ERR_INVALID_ARG, "alignment %llu runs past the blob", (unsigned long long)a);
            if (len < c->opts.min_len) continue;       // main.cpp:132
            c->h_aln_len.push_back(len);
            c->h_aln_start.push_back(b->aln_start[a]);
            c->h_aln_off.push_back(b->aln_off[a]);
            c->h_aln_tgt.push_back(t);
            c->sum_len += len;
            // (a read that spans the target begins at its first base and has a column per target base; necessary, not
            // sufficient -- a read that ends early and inserts a lot passes too: the batch is then exact all the same, with
            // fewer cuts than it could have)
            n_whole += len >= b->tlen[t] && b->aln_start[a] == 1u;
        }
        const uint64_t k = c->h_aln_len.size() - c->h_aln_begin[t];
        if (k > DAGCON_MAX_COVERAGE)
            return fail(c, DAGCON_ERR_UNSUPPORTED, "target %u has %llu alignments (max %u)", t,
                        (unsigned long long)k, DAGCON_MAX_COVERAGE);
        c->max_k = std::max<uint32_t>(c->max_k, (uint32_t)k);
        c->max_tlen = std::max(c->max_tlen, b->tlen[t]);
        if ((uint64_t)b->tlen[t] + 2 > 4ull * 65535ull)
            return fail(c, DAGCON_ERR_UNSUPPORTED, "tlen of target %u exceeds %u", t, 4u * 65535u - 2u);
        c->h_mat_base[t] = c->mat_cells;
        c->mat_cells += ((uint64_t)b->tlen[t] + 2) * k;
        c->h_matc_stride[t] = (b->tlen[t] + 2 + 7) & ~7u;      // matC is [read][position], rows 32-byte aligned
        c->h_matc_base[t] = c->matc_cells;
        c->matc_cells += (uint64_t)c->h_matc_stride[t] * k;
        c->h_bbv_base[t] = c->sum_bb;                      // multiple of 4: 16-byte loads of bid[]
        c->sum_bb += ((uint64_t)b->tlen[t] + 2 + 3) & ~3ull;
        if (c->have_bb) {
            c->h_bb_off[t] = b->backbone_off[t];
            bb_bytes = std::max<uint64_t>(bb_bytes, b->backbone_off[t] + b->tlen[t]);
        }
    }
    // cuts for partial-span pileups (prologue + worklist + epilogue): where the reads are full-span the cut
    // vertices every read passes through are the same ones, found without that machinery
    c->full_span = n_whole == (uint64_t)c->h_aln_len.size();
    // shortest stretch worth a worker: 768 positions when that already fills the chip, shorter (down to 192)
    // for small batches, whose waves would otherwise be few and long
    c->gcuts = c->full_span ? 0u : 1u;
    if (const char *e = getenv("DAGCON_GCUTS")) c->gcuts = atoi(e) ? 1u : 0u;
    {
        DgPlanIn pi;
        pi.T = T; pi.n_alns = c->h_aln_len.size(); pi.sum_bb = c->sum_bb; pi.gcuts = c->gcuts;
        pi.max_segments = c->opts.max_segments; pi.min_segment_len = c->opts.min_segment_len;
        pi.seg_env = c->seg_env; pi.merge_q = c->merge_q ? 1u : 0u;
        const DgPlan pl = dg_plan_pieces(pi);
        c->seg_max = pl.seg_max; c->seg_min = pl.seg_min; c->use_q = (int)pl.use_q; c->bp_max = pl.bp_max;
    }
    if (const char *e = getenv("DAGCON_BP_SEGS")) { const int v = atoi(e); if (v >= 1 && v <= 64) c->bp_max = (uint32_t)v; }
    // scratch per (target, piece): 4096 words where that is cheap, less for batches of very many
    // targets (2 GB in all at most; a piece that needs more raises DG_E_STACK: grown x4, re-run)
    {
        const uint64_t pieces = std::max<uint64_t>(1, (uint64_t)T * std::max(c->bp_max, c->seg_max));
        const uint32_t fit = (uint32_t)std::min<uint64_t>(4096, (512ull << 20) / pieces);
        const uint32_t base = std::max(256u, fit);
        if (c->stk_words < base || (uint64_t)c->stk_words * pieces > (1024ull << 20)) c->stk_words = base;
    }
    if (c->gcuts) c->worklist_cap = std::max<uint32_t>(c->worklist_cap, (uint32_t)std::min<uint64_t>((uint64_t)T * c->seg_max + 64, 0x0FFFFFFFull));
    c->h_aln_begin[T] = c->h_aln_len.size();
    if (c->h_aln_len.size() > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many alignments");
    c->A = (uint32_t)c->h_aln_len.size();
    c->blob_bytes = b->blob_bytes;
    // windows of DG_NCH input columns: the units of the chunked normalizeGaps
    c->h_ch_base.assign((size_t)c->A + 1, 0);
    c->h_ch_aln.clear();
    for (uint32_t a = 0; a < c->A; a++) {
        const uint32_t nw = std::max<uint32_t>(1u, (c->h_aln_len[a] + DG_NCH - 1) / DG_NCH);
        c->h_ch_base[a] = (uint32_t)c->h_ch_aln.size();
        if (c->h_ch_aln.size() + nw > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many alignment columns");
        c->h_ch_aln.insert(c->h_ch_aln.end(), nw, a);
    }
    // column buffers: an alignment normalises to at most 2 columns per input column (every mismatch
    // becomes two); offsets are multiples of 8 columns (16-byte pieces)
    c->h_norm_off.assign((size_t)c->A, 0);
    {
        uint64_t top = 0;
        for (uint32_t a = 0; a < c->A; a++) { c->h_norm_off[a] = top; top += (2ull * c->h_aln_len[a] + 7ull) & ~7ull; }
        c->norm_cap = std::max<uint64_t>(c->norm_cap, top + 64);
    }
    c->h_ck_base.assign((size_t)c->A, 0);
    c->n_ckpt = 0;
    for (uint32_t a = 0; a < c->A; a++) {
        c->h_ck_base[a] = (uint32_t)c->n_ckpt;
        c->n_ckpt += (((uint64_t)c->h_tlen[c->h_aln_tgt[a]] + 2) >> c->emit_shift) + 1;
        if (c->n_ckpt > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many alignment columns");
    }
    c->h_ch_base[c->A] = (uint32_t)c->h_ch_aln.size();
    c->n_chunks = (uint32_t)c->h_ch_aln.size();
    c->tmp_main = (2ull * b->blob_bytes + 8ull * c->n_chunks + 15ull) & ~7ull;
    c->tmp_cap = c->tmp_main + std::max<uint64_t>(c->tmp_main / 16, 1ull << 20);

    // inputs -> HBM
    ENSURE(c, c->d_q, b->blob_bytes);
    ENSURE(c, c->d_t, b->blob_bytes);
    if (b->blob_bytes && !(dev_q == c->d_q.p && dev_t == c->d_t.p)) {     // (dagcon_upload_cigar expands into d_q / d_t themselves)
        HIPCHK(c, hipMemcpyAsync(c->d_q.p, dev_q ? dev_q : b->qstr, b->blob_bytes, dev_q ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_t.p, dev_t ? dev_t : b->tstr, b->blob_bytes, dev_t ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    if (c->have_bb) {
        ENSURE(c, c->d_bb, bb_bytes);
        if (bb_bytes) HIPCHK(c, hipMemcpyAsync(c->d_bb.p, b->backbone, bb_bytes, hipMemcpyHostToDevice, c->stream));
    }
    int r;
    if ((r = upload_vec(c, c->d_aln_off, c->h_aln_off))) return r;
    if ((r = upload_vec(c, c->d_aln_len, c->h_aln_len))) return r;
    if ((r = upload_vec(c, c->d_aln_start, c->h_aln_start))) return r;
    if ((r = upload_vec(c, c->d_aln_tgt, c->h_aln_tgt))) return r;
    if ((r = upload_vec(c, c->d_tlen, c->h_tlen))) return r;
    if ((r = upload_vec(c, c->d_aln_begin, c->h_aln_begin))) return r;
    if ((r = upload_vec(c, c->d_tactive, c->h_tactive))) return r;
    if ((r = upload_vec(c, c->d_bb_off, c->h_bb_off))) return r;
    if ((r = upload_vec(c, c->d_mat_base, c->h_mat_base))) return r;
    if ((r = upload_vec(c, c->d_matc_base, c->h_matc_base))) return r;
    if ((r = upload_vec(c, c->d_matc_stride, c->h_matc_stride))) return r;
    if ((r = upload_vec(c, c->d_bbv_base, c->h_bbv_base))) return r;
    if ((r = upload_vec(c, c->d_ch_base, c->h_ch_base))) return r;
    if ((r = upload_vec(c, c->d_ch_aln, c->h_ch_aln))) return r;
    if ((r = upload_vec(c, c->d_ck_base, c->h_ck_base))) return r;
    if ((r = upload_vec(c, c->d_norm_off, c->h_norm_off))) return r;
    ENSURE(c, c->d_ckpt, c->n_ckpt * 4);

    // work arrays whose size the host knows
    const size_t A4 = (size_t)c->A * 4, T4 = (size_t)T * 4;
    ENSURE(c, c->d_nmis, A4);
    ENSURE(c, c->d_n_lo, A4); ENSURE(c, c->d_n_hi, A4); ENSURE(c, c->d_n_start, A4);
    ENSURE(c, c->d_n_ins, A4); ENSURE(c, c->d_n_del, A4); ENSURE(c, c->d_n_lb, A4);
    {
        const size_t C4 = (size_t)c->n_chunks * 4;
        ENSURE(c, c->d_ch_k0, C4); ENSURE(c, c->d_ch_next, C4); ENSURE(c, c->d_ch_w, C4); ENSURE(c, c->d_ch_tb, C4);
        ENSURE(c, c->d_ch_flag, C4); ENSURE(c, c->d_ch_src, 2 * C4); ENSURE(c, c->d_ch_out, C4); ENSURE(c, c->d_ch_adv, C4);
        ENSURE(c, c->d_norm_tmp, c->tmp_cap * sizeof(uint16_t));
    }
    ENSURE(c, c->d_node_base, (size_t)T * 8); ENSURE(c, c->d_n_nodes, T4);
    ENSURE(c, c->d_pool_base, (size_t)T * 8); ENSURE(c, c->d_pool_size, T4); ENSURE(c, c->d_pool_top, T4);
    ENSURE(c, c->d_t_nins, T4);
    ENSURE(c, c->d_matA, c->mat_cells * 4); ENSURE(c, c->d_matD, c->mat_cells * 4);
    ENSURE(c, c->d_cov, c->sum_bb * 4); ENSURE(c, c->d_gcount, c->sum_bb * 4);
    ENSURE(c, c->d_gbase, c->sum_bb * 4); ENSURE(c, c->d_bid, c->sum_bb * 4);
    if ((r = ensure_stat(c, T))) return r;

    // first guesses for the data-dependent arenas; a run that finds them too
    // small records the exact need on the device and is repeated once.
    c->node_cap = std::max<uint64_t>(c->node_cap, c->sum_bb + c->sum_len / 7 + 1024);
    c->pool_cap = std::max<uint64_t>(c->pool_cap, 8ull * c->node_cap + 80ull * c->sum_bb + 1024ull * T);
    c->cns_cap = std::max<uint64_t>(c->cns_cap, c->sum_bb + c->sum_bb / 4 + 1024);
    c->seg_cap = std::max<uint64_t>(c->seg_cap, (uint64_t)T * 4 + 1024);
    if ((r = ensure_arenas(c))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->uploaded = true;
    c->tm.reruns = 0;
    return DAGCON_OK;
}

int dagcon_upload(dagcon_ctx *ctx, const dagcon_batch *b) { return upload_impl(ctx, b, nullptr, nullptr); }

int dagcon_run(dagcon_ctx *ctx) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->uploaded) return fail(c, DAGCON_ERR_STATE, "dagcon_run before dagcon_upload");
    HIPCHK(c, hipSetDevice(c->device));
    int r = launch_all(c);
    if (r != DAGCON_OK) return r;
    c->ran = true; c->fetched = false;
    c->ed_valid = c->pos_pending = false;
    // debugging aid (tools/bp_pieces.py): DAGCON_DUMP=<target>:<path> leaves that target's merged graph, its bestPath cuts,
    // scores and choices in a file -- N, bp_max, pool words, then cuts row, records, pool, (score, final) pairs, best[]
    if (const char *e = getenv("DAGCON_DUMP")) {
        const uint32_t t = (uint32_t)atoi(e);
        const char *path = strchr(e, ':');
        if (path && t < c->T) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            uint64_t nb = 0, pb = 0;
            uint32_t hdr[4] = {0, c->bp_max, 0, c->seg_max};
            (void)hipMemcpy(&nb, (uint64_t *)c->d_node_base.p + t, 8, hipMemcpyDeviceToHost);
            (void)hipMemcpy(&pb, (uint64_t *)c->d_pool_base.p + t, 8, hipMemcpyDeviceToHost);
            (void)hipMemcpy(&hdr[0], (uint32_t *)c->d_n_nodes.p + t, 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(&hdr[2], (uint32_t *)c->d_pool_top.p + t, 4, hipMemcpyDeviceToHost);
            std::vector<uint32_t> cuts(c->bp_max + 2), pool(hdr[2]), best(hdr[0]);
            std::vector<DgNode> nd(hdr[0]);
            std::vector<float> sc(2 * (size_t)hdr[0]);
            (void)hipMemcpy(cuts.data(), (uint32_t *)c->d_cuts_bp.p + (uint64_t)t * (c->bp_max + 2), cuts.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(nd.data(), (DgNode *)c->d_nodes.p + nb, nd.size() * sizeof(DgNode), hipMemcpyDeviceToHost);
            (void)hipMemcpy(pool.data(), (uint32_t *)c->d_pool.p + pb, pool.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(sc.data(), (float *)c->d_score.p + 2 * nb, sc.size() * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(best.data(), (uint32_t *)c->d_best.p + nb, best.size() * 4, hipMemcpyDeviceToHost);
            if (FILE *f = fopen(path + 1, "wb")) {
                fwrite(hdr, 4, 4, f); fwrite(cuts.data(), 4, cuts.size(), f); fwrite(nd.data(), sizeof(DgNode), nd.size(), f);
                fwrite(pool.data(), 4, pool.size(), f); fwrite(sc.data(), 4, sc.size(), f); fwrite(best.data(), 4, best.size(), f);
                // (partial-span batches: the merge's worklist -- (target, first vertex, last vertex) triples -- behind it)
                uint32_t nl = 0;
                std::vector<uint32_t> wl;
                if (c->gcuts && c->d_worklist.p) {
                    (void)hipMemcpy(&nl, c->d_worklist.p, 4, hipMemcpyDeviceToHost);
                    if (nl > c->worklist_cap) nl = c->worklist_cap;
                    wl.resize(3 * (size_t)nl);
                    if (nl) (void)hipMemcpy(wl.data(), (uint32_t *)c->d_worklist.p + 4, wl.size() * 4, hipMemcpyDeviceToHost);
                }
                fwrite(&nl, 4, 1, f);
                if (nl) fwrite(wl.data(), 4, wl.size(), f);
                fclose(f);
            }
        }
    }
    return DAGCON_OK;
}

int dagcon_sync(dagcon_ctx *ctx) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DAGCON_OK;
}

// device -> host on the context's own stream.  (hipMemcpy would go through the null stream, and the stream is
// non-blocking so that a second context on the same GPU is not serialised against this one's copies.)
static hipError_t d2h(Ctx *c, void *dst, const void *src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

static int read_status(Ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, d2h(c, &c->h_st, c->sb.dev.p, sizeof(DgStatus)));
    return DAGCON_OK;
}

int dagcon_fetch(dagcon_ctx *ctx, dagcon_results *res) {
    if (!ctx || !res) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->ran) return fail(c, DAGCON_ERR_STATE, "dagcon_fetch before dagcon_run");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    const StatBlock &sb = c->sb;
    for (int attempt = 0;; attempt++) {
        // round 1: the whole status block in one copy -- the status, and with it everything whose size the host knows
        HIPCHK(c, d2h(c, sb.host, sb.dev.p, sb.bytes));
        memcpy(&c->h_st, sb.host, sizeof(DgStatus));
        const uint32_t f = c->h_st.err_flags;
        if (f == 0) break;
        if (f & DG_E_TARGET_MASK)       // (target-level failures never set the batch flag: see DgParams::tfail)
            return fail(c, DAGCON_ERR_INTERNAL, "unexpected batch-level flag 0x%x", f);
        if (attempt >= 6) return fail(c, DAGCON_ERR_WORKSPACE, "workspace still too small after %d re-runs (flags 0x%x)", attempt, f);
        if (f & DG_E_NORM_OVF) c->norm_cap = c->h_st.norm_top + 1024;
        if (f & DG_E_NODE_OVF) c->node_cap = c->h_st.node_need + 1024;
        if (f & DG_E_POOL_OVF) c->pool_cap = c->h_st.pool_need + 1024;
        if (f & DG_E_POOL_TGT) c->growth_pct *= 3;
        if (f & DG_E_STACK) c->stk_words *= 4;
        if (f & DG_E_LIST_OVF) c->worklist_cap *= 4;
        if (f & DG_E_LOG_OVF) c->sh_log *= 2;
        if (f & DG_E_RUN_WIDE) c->wide_cells = true;       // (until the next upload)
        if ((f & DG_E_ED_OVF) && sb.o_ed_top) c->ed_cap = *sb.h<uint64_t>(sb.o_ed_top) + 1024;
        if (f & DG_E_OUT_OVF) {
            c->cns_cap = std::max<uint64_t>(c->cns_cap, c->h_st.cns_top + 1024);
            c->seg_cap = std::max<uint64_t>(c->seg_cap, c->h_st.seg_top + 1024);
        }
        c->tm.reruns++;
        if ((r = launch_all(c))) return r;
    }
    // timings
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[4])); c->tm.ms_total = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->tm.ms_normalize = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->tm.ms_build = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); c->tm.ms_merge = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[4])); c->tm.ms_bestpath = ms;

    const uint32_t T = c->T;
    // per-target outcome (ABI 2): a failure is confined to its target
    const uint32_t *m_tfail = sb.h<uint32_t>(sb.o_tfail), *m_n_seg = sb.h<uint32_t>(sb.o_n_seg);
    const uint64_t *m_cns_off = sb.h<uint64_t>(sb.o_cns_off), *m_seg_first = sb.h<uint64_t>(sb.o_seg_first);
    c->r_status.assign(T, DAGCON_OK);
    uint32_t n_failed = 0;
    c->err.clear();
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t f = m_tfail[t];
        if (!f) continue;
        const int code = (f & (DG_E_BADCHAR | DG_E_NONCONF)) ? DAGCON_ERR_NONCONFORMING
                       : (f & DG_E_TOO_BIG) ? DAGCON_ERR_UNSUPPORTED : DAGCON_ERR_INTERNAL;
        c->r_status[t] = code;
        if (!n_failed++) {
            if (f & DG_E_BADCHAR) fail(c, code, "target %u: an alignment holds a byte outside printable ASCII", t);
            else if (f & DG_E_NONCONF) fail(c, code, "target %u: an alignment (after the min_len filter) leaves the backbone: start < 1 or target bases past tlen", t);
            else if (f & DG_E_TOO_BIG) fail(c, code, "target %u too large (more than 2^25 - 3 vertices or 2^30 pool words)", t);
            else fail(c, code, "device invariant violated in target %u", t);
        }
    }
    // dagcon_upload_cigar: a target with a non-conforming record had none of its records expanded
    for (uint32_t t = 0; t < T && !c->h_cig_bad.empty(); t++) {
        if (!c->h_cig_bad[t] || c->r_status[t] != DAGCON_OK) continue;
        c->r_status[t] = DAGCON_ERR_NONCONFORMING;
        if (!n_failed++) c->err = c->cig_err;
    }
    const uint64_t nseg = c->h_st.seg_top, nb = c->h_st.cns_top;
    if (nseg > c->r_seg_cap || nseg > c->seg_cap) return fail(c, DAGCON_ERR_INTERNAL, "%llu segments in an arena of %llu", (unsigned long long)nseg, (unsigned long long)c->seg_cap);
    if (c->r_blob_cap < nb + 1) {
        if (c->r_blob) (void)hipHostFree(c->r_blob);
        c->r_blob = nullptr; c->r_blob_cap = 0;
        const size_t want = (size_t)(nb + 1) + (size_t)(nb / 8) + 4096;
        HIPCHK(c, hipHostMalloc((void **)&c->r_blob, want, hipHostMallocDefault));
        c->r_blob_cap = want;
    }
    c->r_blob[nb] = 0;
    const bool full = !(c->opts.flags & (DAGCON_FLAG_STOP_AFTER_BUILD | DAGCON_FLAG_STOP_AFTER_MERGE));
    const bool want_sup = full && (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT), want_pos = full && (c->opts.flags & DAGCON_FLAG_BASE_POS);
    // edits on: the edits come instead of the positions, which stay on the device for dagcon_fetch_positions to ask for
    const bool want_ed = full && c->ed_batch, lazy_pos = want_pos && want_ed;
    const uint64_t n_ed = want_ed && T ? *sb.h<uint64_t>(sb.o_ed_top) : 0;
    if (n_ed > c->ed_cap) return fail(c, DAGCON_ERR_INTERNAL, "%llu edits in an arena of %llu", (unsigned long long)n_ed, (unsigned long long)c->ed_cap);
    c->sup_valid = c->pos_valid = false;
    c->ed_valid = c->pos_pending = false;
    c->r_nb = nb;
    const size_t ed_seg_bytes = (size_t)nseg * sizeof(DgEdSeg), ed_bytes = ed_seg_bytes + (size_t)n_ed * sizeof(DgEdit);
    if (want_ed && c->r_ed_cap < ed_bytes + 1) {
        if (c->r_ed) (void)hipHostFree(c->r_ed);
        c->r_ed = nullptr; c->r_ed_cap = 0;
        const size_t want = ed_bytes + ed_bytes / 8 + 4096;
        HIPCHK(c, hipHostMalloc((void **)&c->r_ed, want, hipHostMallocDefault));
        c->r_ed_cap = want;
    }
    if (want_sup && c->r_sup_cap < nb + 1) {
        if (c->r_sup) (void)hipHostFree(c->r_sup);
        c->r_sup = nullptr; c->r_sup_cap = 0;
        const size_t want = (size_t)(nb + 1) + (size_t)(nb / 8) + 4096;
        HIPCHK(c, hipHostMalloc((void **)&c->r_sup, want * 4, hipHostMallocDefault));
        c->r_sup_cap = want;
    }
    if (want_pos && !lazy_pos) c->r_pos.resize(nb + 1);
    // round 2: what the status sizes -- the segments' ranges (the first seg_top entries of either array), the blob, the
    // support (weights then depths: the device keeps them apart, no host pass over them) and the positions -- enqueued
    // together, one wait
    int32_t *m_r0 = c->r_seg, *m_r1 = c->r_seg + nseg;
    bool queued = false;
    if (T && full && nseg) {
        HIPCHK(c, hipMemcpyAsync(m_r0, c->d_seg.p, nseg * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(m_r1, (const int32_t *)c->d_seg.p + seg_stride(c), nseg * 4, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (T && full && nb) { HIPCHK(c, hipMemcpyAsync(c->r_blob, c->d_cns.p, nb, hipMemcpyDeviceToHost, c->stream)); queued = true; }
    if (want_sup && nb) {
        HIPCHK(c, hipMemcpyAsync(c->r_sup, c->d_sup.p, nb * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->r_sup + nb, (const uint16_t *)c->d_sup.p + c->cns_cap, nb * 2, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (want_pos && !lazy_pos && nb) { HIPCHK(c, hipMemcpyAsync(c->r_pos.data(), c->d_pos.p, nb * 4, hipMemcpyDeviceToHost, c->stream)); queued = true; }
    if (want_ed && T && nseg) {
        HIPCHK(c, hipMemcpyAsync(c->r_ed, c->d_ed_seg.p, ed_seg_bytes, hipMemcpyDeviceToHost, c->stream));
        if (n_ed) HIPCHK(c, hipMemcpyAsync(c->r_ed + ed_seg_bytes, c->d_ed_out.p, (size_t)n_ed * sizeof(DgEdit), hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (queued) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (want_sup) { c->r_sup_n = nb; c->sup_valid = true; }
    if (want_pos && !lazy_pos) c->pos_valid = true;
    c->pos_pending = lazy_pos;
    const DgEdSeg *m_es = reinterpret_cast<const DgEdSeg *>(c->r_ed);
    const DgEdit *m_ed = reinterpret_cast<const DgEdit *>(c->r_ed + ed_seg_bytes);
    if (want_ed) {
        c->e_t0.clear(); c->e_t1.clear(); c->e_begin.clear();
        c->e_tpos.clear(); c->e_tlen.clear(); c->e_clen.clear(); c->e_coff.clear();
    }
    c->r_seg_begin.assign(T + 1, 0);
    c->r_range0.clear(); c->r_range1.clear(); c->r_seq_off.clear(); c->r_seq_len.clear();
    uint64_t bases = 0;
    for (uint32_t t = 0; t < T; t++) {
        c->r_seg_begin[t] = c->r_range0.size();
        if (!full || !c->h_tactive[t] || m_tfail[t]) continue;
        for (uint32_t i = 0; i < m_n_seg[t]; i++) {
            const uint64_t s = m_seg_first[t] + i;
            const int32_t r0 = m_r0[s], r1 = m_r1[s];
            c->r_range0.push_back(r0); c->r_range1.push_back(r1);
            c->r_seq_off.push_back(m_cns_off[t] + (uint64_t)r0);
            c->r_seq_len.push_back((uint32_t)(r1 - r0));
            bases += (uint64_t)(r1 - r0);
            if (want_ed) {
                // the segment's record and its edits, from the device's order into the host's
                const DgEdSeg &es = m_es[s];
                if (es.tgt != t || es.off > n_ed || es.cnt > n_ed - es.off)
                    return fail(c, DAGCON_ERR_INTERNAL, "k_ed_scan: segment %llu of target %u has edits [%llu, + %u) of %llu, target %u",
                                (unsigned long long)s, t, (unsigned long long)es.off, es.cnt, (unsigned long long)n_ed, es.tgt);
                c->e_t0.push_back(es.t0); c->e_t1.push_back(es.t1); c->e_begin.push_back(c->e_tpos.size());
                for (uint32_t k = 0; k < es.cnt; k++) {
                    const DgEdit &e = m_ed[es.off + k];
                    c->e_tpos.push_back(e.t_pos); c->e_tlen.push_back(e.t_len); c->e_coff.push_back(e.c_off); c->e_clen.push_back(e.c_len);
                }
            }
        }
    }
    if (want_ed) { c->e_begin.push_back(c->e_tpos.size()); c->ed_valid = true; }
    c->r_seg_begin[T] = c->r_range0.size();
    c->tm.consensus_bases = bases;
    c->tm.algorithmic_bytes = 2ull * c->sum_len + bases;
    c->tm.n_alignments = c->A;
    c->tm.n_columns = c->h_st.n_columns;
    c->tm.n_nodes = c->h_st.node_need;
    c->tm.merge_segments = c->h_st.n_mseg;
    res->n_targets = T;
    res->n_segments = c->r_range0.size();
    res->seg_begin = c->r_seg_begin.data();
    res->range0 = c->r_range0.data(); res->range1 = c->r_range1.data();
    res->seq_off = c->r_seq_off.data(); res->seq_len = c->r_seq_len.data();
    res->seq_blob = c->r_blob; res->seq_bytes = nb;
    res->target_status = c->r_status.data(); res->n_failed = n_failed;
    c->fetched = true;
    return DAGCON_OK;
}

int dagcon_fetch_support(dagcon_ctx *ctx, dagcon_support *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_SUPPORT))
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_support on a context created without DAGCON_FLAG_BASE_SUPPORT");
    if (!c->sup_valid)
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_support without the results of a consensus (no fetch yet, or stopped before bestPath)");
    out->n = c->r_sup_n;
    out->weight = c->r_sup;
    out->depth = c->r_sup + c->r_sup_n;
    return DAGCON_OK;
}

int dagcon_fetch_positions(dagcon_ctx *ctx, const uint32_t **pos, uint64_t *n) {
    if (!ctx || !pos || !n) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_POS))
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_positions on a context created without DAGCON_FLAG_BASE_POS");
    if (c->pos_pending) {
        // edits on: the copy dagcon_fetch left out; the kind bit the edit kernels read stays on the device
        HIPCHK(c, hipSetDevice(c->device));
        c->r_pos.resize(c->r_nb + 1);
        if (c->r_nb) HIPCHK(c, d2h(c, c->r_pos.data(), c->d_pos.p, c->r_nb * 4));
        for (uint64_t i = 0; i < c->r_nb; i++) c->r_pos[i] &= ~DG_POS_BB;
        c->pos_pending = false; c->pos_valid = true;
    }
    if (!c->pos_valid)
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_positions without the results of a consensus (no fetch yet, or stopped before bestPath)");
    *pos = c->r_pos.data();
    *n = c->r_pos.size() - 1;
    return DAGCON_OK;
}

int dagcon_set_edits(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_POS))
        return fail(c, DAGCON_ERR_STATE, "dagcon_set_edits on a context created without DAGCON_FLAG_BASE_POS");
    c->edits_on = on != 0;
    return DAGCON_OK;
}

int dagcon_fetch_edits(dagcon_ctx *ctx, dagcon_edits *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->edits_on || !c->ed_valid)
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_edits without the results of a record upload made with dagcon_set_edits on (edits off, "
                                         "another kind of upload, no fetch yet, or stopped before bestPath)");
    out->n_segments = c->e_t0.size(); out->n = c->e_tpos.size();
    out->seg_t0 = c->e_t0.data(); out->seg_t1 = c->e_t1.data(); out->edit_begin = c->e_begin.data();
    out->t_pos = c->e_tpos.data(); out->t_len = c->e_tlen.data(); out->c_off = c->e_coff.data(); out->c_len = c->e_clen.data();
    return DAGCON_OK;
}

// diagnostic builds (-DDG_STAMPS) only: raw device counters of the last run
int dagcon_debug_counters(dagcon_ctx *ctx, unsigned long long *out8) {
    if (!ctx || !out8) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DgStatus st;
    HIPCHK(c, d2h(c, &st, c->sb.dev.p, sizeof st));
    for (int i = 0; i < 16; i++) out8[i] = st.dbg[i];
    return DAGCON_OK;
}

uint32_t dagcon_align_dropped(dagcon_ctx *ctx) {
    return ctx ? reinterpret_cast<Ctx *>(ctx)->align_dropped : 0u;
}

// host arithmetic only (no device, no context): the pieces a batch of that shape would be cut into
int dagcon_debug_plan(uint32_t n_targets, uint64_t n_alignments, uint64_t sum_positions, uint32_t partial_span,
                      uint32_t max_segments, uint32_t min_segment_len, uint32_t out4[4]) {
    if (!out4) return DAGCON_ERR_INVALID_ARG;
    DgPlanIn pi;
    pi.T = n_targets; pi.n_alns = n_alignments; pi.sum_bb = sum_positions; pi.gcuts = partial_span ? 1u : 0u;
    pi.max_segments = max_segments; pi.min_segment_len = min_segment_len; pi.seg_env = 0; pi.merge_q = 1;
    const DgPlan pl = dg_plan_pieces(pi);
    out4[0] = pl.seg_max; out4[1] = pl.seg_min; out4[2] = pl.use_q; out4[3] = pl.bp_max;
    return DAGCON_OK;
}

int dagcon_get_timings(dagcon_ctx *ctx, dagcon_timings *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->ran) return fail(c, DAGCON_ERR_STATE, "no run to report");
    if (!c->fetched) {
        // timings of a run that has been synchronised but not fetched
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[4])); c->tm.ms_total = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->tm.ms_normalize = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->tm.ms_build = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); c->tm.ms_merge = ms;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[4])); c->tm.ms_bestpath = ms;
    }
    *out = c->tm;
    return DAGCON_OK;
}

int dagcon_consensus(dagcon_ctx *ctx, const dagcon_batch *batch, dagcon_results *results) {
    int r = dagcon_upload(ctx, batch);
    if (r != DAGCON_OK) return r;
    if ((r = dagcon_run(ctx)) != DAGCON_OK) return r;
    return dagcon_fetch(ctx, results);
}

static int normalize_impl(Ctx *c, dagcon_ctx *ctx, uint32_t n, const uint32_t *aln_start,
                          const uint64_t *aln_off, const uint32_t *aln_len, const char *qstr,
                          const char *tstr, uint64_t blob_bytes, const uint64_t *out_off, char *qout,
                          char *tout, uint32_t *out_len, uint32_t *out_start) {
    // one pseudo target (tlen 0) that holds every alignment; only the a1
    // kernels run, with the graph stage's conformity check switched off
    std::vector<uint32_t> tl(1, 0u);
    std::vector<uint64_t> ab = {0, n};
    dagcon_batch b;
    memset(&b, 0, sizeof b);
    b.n_targets = 1; b.tlen = tl.data(); b.aln_begin = ab.data();
    b.aln_start = aln_start; b.aln_off = aln_off; b.aln_len = aln_len;
    b.qstr = qstr; b.tstr = tstr; b.blob_bytes = blob_bytes;
    int r = dagcon_upload(ctx, &b);
    if (r != DAGCON_OK) return r;
    for (int attempt = 0;; attempt++) {
        DgParams p;
        fill_params(c, p);
        p.flags |= DG_F_A1_ONLY;
        HIPCHK(c, hipMemsetAsync(c->sb.dev.p, 0, c->sb.zero_bytes, c->stream));     // DgStatus and tfail among them
        launch_normalize(c, p, true);                      // (no graph follows: nothing is written to matC)
        HIPCHK(c, hipGetLastError());
        if ((r = read_status(c))) return r;
        if ((c->h_st.err_flags & DG_E_NORM_OVF) && attempt < 3) {
            c->norm_cap = c->h_st.norm_top + 1024;
            if ((r = ensure_arenas(c))) return r;
            continue;
        }
        break;
    }
    if (c->h_st.err_flags & DG_E_BADCHAR)
        return fail(c, DAGCON_ERR_NONCONFORMING, "alignment %u holds a byte outside printable ASCII", c->h_st.bad_aln);
    if (c->h_st.err_flags) return fail(c, DAGCON_ERR_INTERNAL, "normalize failed (flags 0x%x)", c->h_st.err_flags);
    std::vector<uint64_t> noff(n);
    std::vector<uint32_t> lo(n), hi(n), st(n);
    if (n) {
        HIPCHK(c, d2h(c, noff.data(), c->d_norm_off.p, (size_t)n * 8));
        HIPCHK(c, d2h(c, lo.data(), c->d_n_lo.p, (size_t)n * 4));
        HIPCHK(c, d2h(c, hi.data(), c->d_n_hi.p, (size_t)n * 4));
        HIPCHK(c, d2h(c, st.data(), c->d_n_start.p, (size_t)n * 4));
    }
    std::vector<uint16_t> cols;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t m = hi[a] - lo[a];
        cols.resize(m);
        if (m) HIPCHK(c, d2h(c, cols.data(), (const uint16_t *)c->d_norm.p + noff[a] + lo[a], (size_t)m * 2));
        for (uint32_t i = 0; i < m; i++) {
            qout[out_off[a] + i] = (char)(cols[i] & 0xff);
            tout[out_off[a] + i] = (char)(cols[i] >> 8);
        }
        out_len[a] = m;
        out_start[a] = st[a];
    }
    return DAGCON_OK;
}

int dagcon_normalize(dagcon_ctx *ctx, uint32_t n, const uint32_t *aln_start, const uint64_t *aln_off,
                     const uint32_t *aln_len, const char *qstr, const char *tstr, uint64_t blob_bytes,
                     uint32_t trim, uint32_t flags, const uint64_t *out_off, char *qout, char *tout,
                     uint32_t *out_len, uint32_t *out_start) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n && (!aln_start || !aln_off || !aln_len || !qstr || !tstr || !out_off || !qout || !tout || !out_len || !out_start))
        return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    if (n > DAGCON_MAX_COVERAGE)
        return fail(c, DAGCON_ERR_UNSUPPORTED, "dagcon_normalize takes at most %u alignments per call", DAGCON_MAX_COVERAGE);
    const dagcon_opts saved = c->opts;
    c->opts.min_cov = 0; c->opts.min_len = 0; c->opts.trim = trim;
    c->opts.flags = flags & DAGCON_FLAG_RAW_ALIGNMENTS;
    const int r = normalize_impl(c, ctx, n, aln_start, aln_off, aln_len, qstr, tstr, blob_bytes, out_off,
                                 qout, tout, out_len, out_start);
    c->opts = saved;
    c->uploaded = false; c->ran = false;
    return r;
}

extern "C++" {
template <bool LOCAL>
static void launch_align_band(uint32_t cells, uint32_t nk, hipStream_t s, const DgAlignParams &ap) {
    switch (cells) {
        case 2: hipLaunchKernelGGL((k_align_band<2, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
        case 4: hipLaunchKernelGGL((k_align_band<4, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
        case 6: hipLaunchKernelGGL((k_align_band<6, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
        case 8: hipLaunchKernelGGL((k_align_band<8, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
        case 12: hipLaunchKernelGGL((k_align_band<12, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
        default: hipLaunchKernelGGL((k_align_band<16, LOCAL>), dim3(nk), dim3(64), 0, s, ap); break;
    }
}
}

// the -a stage on the device: aligned strings left in c->d_al[7] / [8] at out_off[a], their lengths in aln_len (host),
// the ends of every pair in c->h_ends (DAGCON_FLAG_LOCAL_ALIGN: the local-end instances of the kernels)
static int align_device(Ctx *c, uint32_t n, const uint64_t *q_off, const uint32_t *q_len,
                        const uint64_t *t_off, const uint32_t *t_len, const char *q_blob, uint64_t q_bytes,
                        const char *t_blob, uint64_t t_bytes, const uint64_t *out_off, uint32_t *aln_len, uint64_t *out_bytes_ret) {
    HIPCHK(c, hipSetDevice(c->device));
    const bool local = (c->opts.flags & DAGCON_FLAG_LOCAL_ALIGN) != 0;
    c->align_n = 0;
    uint64_t out_bytes = 0;
    std::vector<uint64_t> dir_off(n);
    for (uint32_t a = 0; a < n; a++) {
        if (q_off[a] > q_bytes || q_len[a] > q_bytes - q_off[a] || t_off[a] > t_bytes || t_len[a] > t_bytes - t_off[a])
            return fail(c, DAGCON_ERR_INVALID_ARG, "pair %u runs past its blob", a);
        if ((uint64_t)q_len[a] + t_len[a] > 0x7FFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "pair %u too long", a);
        out_bytes = std::max<uint64_t>(out_bytes, out_off[a] + (uint64_t)q_len[a] + t_len[a]);
    }
    DevBuf &dq = c->d_al[0], &dt = c->d_al[1], &dqo = c->d_al[2], &dto = c->d_al[3], &dql = c->d_al[4], &dtl = c->d_al[5],
           &doo = c->d_al[6], &dqa = c->d_al[7], &dta = c->d_al[8], &dlen = c->d_al[9], &ddir = c->d_al[10], &ddo = c->d_al[11];
    ENSURE(c, dq, q_bytes); ENSURE(c, dt, t_bytes);
    ENSURE(c, dqo, (size_t)n * 8); ENSURE(c, dto, (size_t)n * 8); ENSURE(c, dql, (size_t)n * 4); ENSURE(c, dtl, (size_t)n * 4);
    ENSURE(c, doo, (size_t)n * 8); ENSURE(c, dqa, out_bytes); ENSURE(c, dta, out_bytes); ENSURE(c, dlen, (size_t)n * 4);
    ENSURE(c, ddo, (size_t)n * 8);
    DevBuf &dend = c->d_al[14];
    if (local) ENSURE(c, dend, (size_t)n * 16);
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(dq.p, q_blob, q_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dt.p, t_blob, t_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dqo.p, q_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dto.p, t_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dql.p, q_len, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dtl.p, t_len, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(doo.p, out_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
    // Two passes (k_align.hip.h): every pair in the narrow band first; the pairs whose path came near an edge of it
    // (DG_AL_RETRY) again in the full band.  Inside a pass: groups of as many pairs as fit the direction budget
    // (one wave per pair and ~1 us per row: what counts is how many pairs are in flight; but a hipMalloc of tens
    // of GB takes seconds on this platform, so 32 GB at most, a quarter of the free memory), and inside a group
    // one launch per kernel instance (cells per lane).
    uint64_t budget_rows = (6ull << 30) / 256ull;
    {
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) {
            const uint64_t have = (uint64_t)mfree + (uint64_t)ddir.cap;      // (the buffer of the last call is ours to reuse)
            budget_rows = std::min<uint64_t>(16ull << 30, std::max<uint64_t>(1ull << 30, have / 4)) / 256ull;
        }
    }
    if (const char *e = getenv("DAGCON_ALIGN_GB")) { const long long v = atoll(e); if (v >= 1 && v <= 200) budget_rows = ((uint64_t)v << 30) / 256ull; }
    if (const char *e = getenv("DAGCON_ALIGN_ROWS")) { const long long v = atoll(e); if (v >= 1) budget_rows = (uint64_t)v; }   // test knob
    const bool t_dbg = getenv("DAGCON_ALIGN_TIMING") != nullptr;
    if (t_dbg) HIPCHK(c, hipStreamSynchronize(s));
    double t_grp = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    DevBuf &didx = c->d_al[12], &dhw = c->d_al[13];
    ENSURE(c, didx, (size_t)n * 4); ENSURE(c, dhw, (size_t)n * 4);
    std::vector<uint32_t> todo(n), halfw(n), order(n);
    for (uint32_t a = 0; a < n; a++) todo[a] = a;
    DgAlignParams ap;
    ap.q = (const uint8_t *)dq.p; ap.t = (const uint8_t *)dt.p;
    ap.q_off = (const uint64_t *)dqo.p; ap.t_off = (const uint64_t *)dto.p;
    ap.q_len = (const uint32_t *)dql.p; ap.t_len = (const uint32_t *)dtl.p;
    ap.out_off = (const uint64_t *)doo.p; ap.qaln = (uint8_t *)dqa.p; ap.taln = (uint8_t *)dta.p;
    ap.aln_len = (uint32_t *)dlen.p; ap.dir_off = (const uint64_t *)ddo.p; ap.halfw = (const uint32_t *)dhw.p;
    ap.ends = local ? (uint32_t *)dend.p : nullptr;
    // the band that follows the alignment first (k_align_adapt): every pair long enough for a static band wider than it
    {
        std::vector<uint32_t> ad, rest;
        for (uint32_t a = 0; a < n; a++) (dg_align_halfwidth_first(q_len[a], t_len[a]) > DG_AL_WA ? ad : rest).push_back(a);
        if (getenv("DAGCON_ALIGN_STATIC")) { rest.insert(rest.end(), ad.begin(), ad.end()); ad.clear(); }      // test knob
        std::stable_sort(ad.begin(), ad.end(), [&](uint32_t x, uint32_t y) { return q_len[x] > q_len[y]; });
        // groups of equal size (a small last one would run at the latency of its longest pair)
        uint64_t all_rows = 0;
        for (uint32_t a : ad) all_rows += dg_align_rows_adapt(q_len[a], t_len[a]);
        const uint64_t ngrp = std::max<uint64_t>(1, (all_rows + budget_rows - 1) / budget_rows);
        const uint64_t grp_rows = std::min<uint64_t>(budget_rows, all_rows / ngrp + 1 + (all_rows / ngrp) / 64);
        size_t first = 0;
        while (first < ad.size()) {
            uint64_t rows = 0;
            size_t cnt = 0;
            while (first + cnt < ad.size()) {
                const uint32_t a = ad[first + cnt];
                const uint64_t r = dg_align_rows_adapt(q_len[a], t_len[a]);
                if (cnt && rows + r > grp_rows) break;
                dir_off[a] = rows;
                rows += r; cnt++;
            }
            ENSURE(c, ddir, rows * 256ull);
            ap.dirs = (uint32_t *)ddir.p;
            HIPCHK(c, hipMemcpyAsync(ddo.p, dir_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync((uint32_t *)didx.p + first, ad.data() + first, cnt * 4, hipMemcpyHostToDevice, s));
            ap.idx = (const uint32_t *)didx.p + first; ap.n = (uint32_t)cnt; ap.first_pass = 1u;
            if (local) hipLaunchKernelGGL(k_align_adapt<true>, dim3((uint32_t)cnt), dim3(64), 0, s, ap);
            else hipLaunchKernelGGL(k_align_adapt<false>, dim3((uint32_t)cnt), dim3(64), 0, s, ap);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(s));
            if (t_dbg) {
                const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
                fprintf(stderr, "dagcon_align: following band, group of %zu pairs, %.1f MB of directions: %.2f ms\n", cnt, rows * 256.0 / 1e6, (now - t_grp) * 1e3);
                t_grp = now;
            }
            first += cnt;
        }
        if (!ad.empty()) {
            HIPCHK(c, d2h(c, aln_len, dlen.p, (size_t)n * 4));
            size_t back = 0;
            for (uint32_t a : ad) if (aln_len[a] == DG_AL_RETRY) { rest.push_back(a); back++; }
            if (t_dbg) fprintf(stderr, "dagcon_align: %zu of %zu pairs go on to the static bands\n", back, ad.size());
        }
        std::sort(rest.begin(), rest.end());
        todo.swap(rest);
    }
    for (int pass = 0; pass < 2 && !todo.empty(); pass++) {
        // (a pair whose first band is the full one already is final in the first pass: its width says so)
        for (uint32_t a : todo) halfw[a] = pass == 0 ? dg_align_halfwidth_first(q_len[a], t_len[a]) : dg_align_halfwidth(q_len[a], t_len[a]);
        HIPCHK(c, hipMemcpyAsync(dhw.p, halfw.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        static const uint32_t kinds[6] = {2, 4, 6, 8, 12, 16};
        size_t first = 0;
        while (first < todo.size()) {
            uint64_t rows = 0;
            size_t cnt = 0;
            while (first + cnt < todo.size()) {
                const uint32_t a = todo[first + cnt];
                const uint64_t r = dg_align_rows(q_len[a], t_len[a], dg_align_cells(halfw[a]));
                if (cnt && rows + r > budget_rows) break;
                dir_off[a] = rows;
                rows += r; cnt++;
            }
            ENSURE(c, ddir, rows * 256ull);
            ap.dirs = (uint32_t *)ddir.p;
            HIPCHK(c, hipMemcpyAsync(ddo.p, dir_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            // the group's pairs by kernel instance, the long ones first inside each; two launches per instance when the
            // pass is the first one: pairs whose narrow band IS the full band are final at once
            size_t fill = 0;
            for (int k = 0; k < 6; k++) {
                for (int fin = 0; fin < 2; fin++) {
                    const size_t k0 = fill;
                    for (size_t x = 0; x < cnt; x++) {
                        const uint32_t a = todo[first + x];
                        const bool is_final = pass == 1 || halfw[a] == dg_align_halfwidth(q_len[a], t_len[a]);
                        if (dg_align_cells(halfw[a]) == kinds[k] && (int)is_final == fin) order[first + fill++] = a;
                    }
                    const uint32_t nk = (uint32_t)(fill - k0);
                    if (!nk) continue;
                    std::stable_sort(order.begin() + first + k0, order.begin() + first + fill,
                                     [&](uint32_t x, uint32_t y) { return q_len[x] > q_len[y]; });
                    HIPCHK(c, hipMemcpyAsync((uint32_t *)didx.p + first + k0, order.data() + first + k0, (size_t)nk * 4, hipMemcpyHostToDevice, s));
                    ap.idx = (const uint32_t *)didx.p + first + k0; ap.n = nk; ap.first_pass = fin ? 0u : 1u;
                    if (local) launch_align_band<true>(kinds[k], nk, s, ap);
                    else launch_align_band<false>(kinds[k], nk, s, ap);
                    HIPCHK(c, hipGetLastError());
                }
            }
            HIPCHK(c, hipStreamSynchronize(s));       // (the direction buffer and the offsets are reused by the next group)
            if (t_dbg) {
                const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
                fprintf(stderr, "dagcon_align: pass %d, group of %zu pairs, %.1f MB of directions: %.2f ms\n", pass, cnt, rows * 256.0 / 1e6, (now - t_grp) * 1e3);
                t_grp = now;
            }
            first += cnt;
        }
        if (pass == 0) {
            HIPCHK(c, d2h(c, aln_len, dlen.p, (size_t)n * 4));
            std::vector<uint32_t> again;
            for (uint32_t a : todo) if (aln_len[a] == DG_AL_RETRY) again.push_back(a);
            if (t_dbg) fprintf(stderr, "dagcon_align: %zu of %u pairs go to the full band\n", again.size(), n);
            todo.swap(again);
        }
    }
    HIPCHK(c, d2h(c, aln_len, dlen.p, (size_t)n * 4));
    uint32_t dropped = 0;
    for (uint32_t a = 0; a < n; a++) {
        if ((uint64_t)aln_len[a] > (uint64_t)q_len[a] + t_len[a]) return fail(c, DAGCON_ERR_INTERNAL, "pair %u: alignment longer than its room", a);
        // the band could not connect the corners (sequences of very different lengths, indels beyond the widest band):
        // length 0, and the record then falls to the min_len filter -- the reference's SDPAlign always returns something
        dropped += aln_len[a] == 0 && (q_len[a] || t_len[a]);
    }
    c->h_ends.resize((size_t)n * 4);
    if (local) HIPCHK(c, d2h(c, c->h_ends.data(), dend.p, (size_t)n * 16));    // (16 B a pair; the strings stay)
    else
        for (uint32_t a = 0; a < n; a++) {                // global: the whole of both, or nothing
            const bool ok = aln_len[a] != 0;
            uint32_t *e = &c->h_ends[(size_t)a * 4];
            e[0] = 0; e[1] = ok ? q_len[a] : 0u; e[2] = 0; e[3] = ok ? t_len[a] : 0u;
        }
    c->align_n = n;
    c->align_dropped = dropped;                   // (the call succeeds: dagcon_align_dropped reports them)
    *out_bytes_ret = out_bytes;
    return DAGCON_OK;
}

int dagcon_align(dagcon_ctx *ctx, uint32_t n, const uint64_t *q_off, const uint32_t *q_len,
                 const uint64_t *t_off, const uint32_t *t_len, const char *q_blob, uint64_t q_bytes,
                 const char *t_blob, uint64_t t_bytes, const uint64_t *out_off, char *qaln, char *taln,
                 uint32_t *aln_len) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->align_n = 0;
    if (n == 0) return DAGCON_OK;
    if (!q_off || !q_len || !t_off || !t_len || !q_blob || !t_blob || !out_off || !qaln || !taln || !aln_len)
        return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    uint64_t out_bytes = 0;
    int r = align_device(c, n, q_off, q_len, t_off, t_len, q_blob, q_bytes, t_blob, t_bytes, out_off, aln_len, &out_bytes);
    if (r != DAGCON_OK) return r;
    HIPCHK(c, d2h(c, qaln, c->d_al[7].p, out_bytes));
    HIPCHK(c, d2h(c, taln, c->d_al[8].p, out_bytes));
    return DAGCON_OK;
}

int dagcon_align_ends(dagcon_ctx *ctx, uint32_t n, uint32_t *q_begin, uint32_t *q_end, uint32_t *t_begin, uint32_t *t_end) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n != c->align_n) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_align_ends: %u pairs asked, the last alignment had %u", n, c->align_n);
    if (n && (!q_begin || !q_end || !t_begin || !t_end)) return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t *e = &c->h_ends[(size_t)a * 4];
        q_begin[a] = e[0]; q_end[a] = e[1]; t_begin[a] = e[2]; t_end[a] = e[3];
    }
    return DAGCON_OK;
}

// dazcon --trace-panels (k_align_panels.hip.h).  A kernel instance per panel size: C cells a lane (n <= 64 C), R rows of
// directions in LDS (m <= R); as many waves a workgroup as keep its LDS at 64 KiB or less, four at most.
extern "C++" {
template <int C, int R>
static void launch_panels(hipStream_t s, const DgPanelParams &pp) {
    constexpr int per_wave = R * 64 * (C <= 4 ? 1 : 2);
    constexpr int WPB = per_wave >= 65536 ? 1 : 65536 / per_wave > 4 ? 4 : 65536 / per_wave;
    hipLaunchKernelGGL((k_align_panel<C, R, WPB>), dim3((pp.n + WPB - 1) / WPB), dim3(64 * WPB), 0, s, pp);
}
}

int dagcon_align_panels(dagcon_ctx *ctx, uint32_t n, const uint64_t *q_off, const uint32_t *q_len, const uint64_t *t_off,
                        const uint32_t *t_len, const char *q_blob, uint64_t q_bytes, const char *t_blob, uint64_t t_bytes,
                        const uint64_t *panel_begin, const uint32_t *panel_t_len, const uint32_t *panel_q_len,
                        const uint64_t *out_off, char *qaln, char *taln, uint32_t *aln_len, int32_t *panel_dist) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->align_dropped = 0;
    if (n == 0) return DAGCON_OK;
    if (!q_off || !q_len || !t_off || !t_len || !q_blob || !t_blob || !panel_begin || !out_off || !qaln || !taln || !aln_len)
        return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    const uint64_t np = panel_begin[n];
    if (np && (!panel_t_len || !panel_q_len)) return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    if (np > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many panels");
    HIPCHK(c, hipSetDevice(c->device));
    // checks, then every panel's place: its first bases in the blobs, its room of m + n columns in the scratch buffer
    std::vector<uint64_t> p_qoff(np), p_toff(np), p_scr(np);
    std::vector<uint32_t> kept, cls[9];
    std::vector<uint8_t> drop(n, 0);
    uint64_t out_bytes = 0, scr_bytes = 0;
    uint32_t dropped = 0;
    for (uint32_t a = 0; a < n; a++) {
        if (q_off[a] > q_bytes || q_len[a] > q_bytes - q_off[a] || t_off[a] > t_bytes || t_len[a] > t_bytes - t_off[a])
            return fail(c, DAGCON_ERR_INVALID_ARG, "pair %u runs past its blob", a);
        if ((uint64_t)q_len[a] + t_len[a] > 0x7FFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "pair %u too long", a);
        if (panel_begin[a] > panel_begin[a + 1] || panel_begin[a + 1] > np)
            return fail(c, DAGCON_ERR_INVALID_ARG, "panel_begin is not ascending at pair %u", a);
        uint64_t st = 0, sq = 0;
        bool big = false;
        for (uint64_t p = panel_begin[a]; p < panel_begin[a + 1]; p++) {
            p_toff[p] = t_off[a] + st; p_qoff[p] = q_off[a] + sq;
            st += panel_t_len[p]; sq += panel_q_len[p];
            big |= panel_t_len[p] > DAGCON_PANEL_MAX_SIDE || panel_q_len[p] > DAGCON_PANEL_MAX_SIDE;
        }
        if (st != t_len[a] || sq != q_len[a])
            return fail(c, DAGCON_ERR_INVALID_ARG, "pair %u: its panels hold %llu A and %llu B bases, not %u and %u", a,
                        (unsigned long long)st, (unsigned long long)sq, t_len[a], q_len[a]);
        out_bytes = std::max<uint64_t>(out_bytes, out_off[a] + (uint64_t)q_len[a] + t_len[a]);
        if (big) { drop[a] = 1; dropped++; continue; }
        kept.push_back(a);
        for (uint64_t p = panel_begin[a]; p < panel_begin[a + 1]; p++) {
            p_scr[p] = scr_bytes;
            scr_bytes += (uint64_t)panel_t_len[p] + panel_q_len[p];
            const uint32_t m = panel_t_len[p], w = panel_q_len[p];
            const int ci = w <= 128 ? 0 : w <= 256 ? 1 : 2, ri = m <= 128 ? 0 : m <= 256 ? 1 : 2;
            cls[ci * 3 + ri].push_back((uint32_t)p);
        }
    }
    DevBuf &dq = c->d_pn[0], &dt = c->d_pn[1], &dpq = c->d_pn[2], &dpt = c->d_pn[3], &dpql = c->d_pn[4], &dptl = c->d_pn[5],
           &dscr = c->d_pn[6], &dqs = c->d_pn[7], &dts = c->d_pn[8], &dplen = c->d_pn[9], &dpdist = c->d_pn[10],
           &didx = c->d_pn[11], &dpb = c->d_pn[12], &doo = c->d_pn[13], &dqa = c->d_pn[14], &dta = c->d_pn[15],
           &dlen = c->d_pn[16], &dkept = c->d_pn[17];
    hipStream_t s = c->stream;
    ENSURE(c, dlen, (size_t)n * 4); ENSURE(c, dqa, out_bytes); ENSURE(c, dta, out_bytes);
    HIPCHK(c, hipMemsetAsync(dlen.p, 0, (size_t)n * 4, s));
    if (!kept.empty()) {
        ENSURE(c, dq, q_bytes); ENSURE(c, dt, t_bytes);
        ENSURE(c, dpq, np * 8); ENSURE(c, dpt, np * 8); ENSURE(c, dpql, np * 4); ENSURE(c, dptl, np * 4); ENSURE(c, dscr, np * 8);
        ENSURE(c, dqs, scr_bytes); ENSURE(c, dts, scr_bytes); ENSURE(c, dplen, np * 4); ENSURE(c, dpdist, np * 4);
        ENSURE(c, didx, np * 4); ENSURE(c, dpb, ((size_t)n + 1) * 8); ENSURE(c, doo, (size_t)n * 8); ENSURE(c, dkept, kept.size() * 4);
        HIPCHK(c, hipMemcpyAsync(dq.p, q_blob, q_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dt.p, t_blob, t_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dpq.p, p_qoff.data(), np * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dpt.p, p_toff.data(), np * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dpql.p, panel_q_len, np * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dptl.p, panel_t_len, np * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dscr.p, p_scr.data(), np * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dpb.p, panel_begin, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(doo.p, out_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(dkept.p, kept.data(), kept.size() * 4, hipMemcpyHostToDevice, s));
        std::vector<uint32_t> order;
        order.reserve(np);
        for (const auto &v : cls) order.insert(order.end(), v.begin(), v.end());
        HIPCHK(c, hipMemcpyAsync(didx.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
        DgPanelParams pp;
        pp.q = (const uint8_t *)dq.p; pp.t = (const uint8_t *)dt.p;
        pp.q_off = (const uint64_t *)dpq.p; pp.t_off = (const uint64_t *)dpt.p;
        pp.q_len = (const uint32_t *)dpql.p; pp.t_len = (const uint32_t *)dptl.p;
        pp.scr_off = (const uint64_t *)dscr.p; pp.qscr = (uint8_t *)dqs.p; pp.tscr = (uint8_t *)dts.p;
        pp.len = (uint32_t *)dplen.p; pp.dist = (int32_t *)dpdist.p;
        size_t first = 0;
        for (int k = 0; k < 9; k++) {
            if (cls[k].empty()) continue;
            pp.idx = (const uint32_t *)didx.p + first; pp.n = (uint32_t)cls[k].size();
            switch (k) {
                case 0: launch_panels<2, 128>(s, pp); break;
                case 1: launch_panels<2, 256>(s, pp); break;
                case 2: launch_panels<2, 512>(s, pp); break;
                case 3: launch_panels<4, 128>(s, pp); break;
                case 4: launch_panels<4, 256>(s, pp); break;
                case 5: launch_panels<4, 512>(s, pp); break;
                case 6: launch_panels<8, 128>(s, pp); break;
                case 7: launch_panels<8, 256>(s, pp); break;
                default: launch_panels<8, 512>(s, pp); break;
            }
            HIPCHK(c, hipGetLastError());
            first += cls[k].size();
        }
        hipLaunchKernelGGL(k_align_panel_compact, dim3((uint32_t)kept.size()), dim3(DG_PANEL_COMPACT_THREADS), 0, s,
                           (const uint64_t *)dpb.p, (const uint64_t *)dscr.p, (const uint32_t *)dptl.p, (const uint32_t *)dpql.p,
                           (const uint32_t *)dplen.p, (const uint8_t *)dqs.p, (const uint8_t *)dts.p, (const uint64_t *)doo.p,
                           (uint8_t *)dqa.p, (uint8_t *)dta.p, (uint32_t *)dlen.p, (const uint32_t *)dkept.p);
        HIPCHK(c, hipGetLastError());
        if (panel_dist) HIPCHK(c, d2h(c, panel_dist, dpdist.p, np * 4));
    }
    HIPCHK(c, d2h(c, aln_len, dlen.p, (size_t)n * 4));
    if (!kept.empty()) {
        HIPCHK(c, d2h(c, qaln, dqa.p, out_bytes));
        HIPCHK(c, d2h(c, taln, dta.p, out_bytes));
    }
    for (uint32_t a = 0; a < n; a++) {
        if ((uint64_t)aln_len[a] > (uint64_t)q_len[a] + t_len[a]) return fail(c, DAGCON_ERR_INTERNAL, "pair %u: alignment longer than its room", a);
        if (drop[a] && panel_dist) for (uint64_t p = panel_begin[a]; p < panel_begin[a + 1]; p++) panel_dist[p] = -1;
    }
    c->align_dropped = dropped;
    return DAGCON_OK;
}

// dagcon_place (k_place.hip.h).  Pairs are taken in target order; the distinct targets are cut into groups whose tables
// fit in DG_PLACE_SLOT_BUDGET slots, and each group is one memset, one k_place_index and one k_place_vote launch.
#define DG_PLACE_SLOT_BUDGET (8u << 20)     // 256 MB of tables at a time
int dagcon_place(dagcon_ctx *ctx, const uint64_t *seq_off, const uint32_t *seq_len, const char *blob, uint64_t bytes,
                 uint32_t n_pairs, const uint32_t *pair_q, const uint32_t *pair_t, uint32_t k, uint32_t max_occ,
                 uint32_t *votes_fwd, uint32_t *votes_rev, char *strand, uint32_t *t0, uint32_t *t1) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n_pairs == 0) return DAGCON_OK;
    if (!seq_off || !seq_len || !blob || !pair_q || !pair_t || !votes_fwd || !votes_rev || !strand || !t0 || !t1)
        return fail(c, DAGCON_ERR_INVALID_ARG, "NULL argument");
    if (k < 8 || k > DG_PLACE_KMAX) return fail(c, DAGCON_ERR_INVALID_ARG, "k = %u is outside 8 .. 16", k);
    if (max_occ < 1 || max_occ > DG_PLACE_MAX_OCC) return fail(c, DAGCON_ERR_INVALID_ARG, "max_occ = %u is outside 1 .. 8", max_occ);
    uint64_t n_seq = 0;
    for (uint32_t a = 0; a < n_pairs; a++) {
        for (const uint32_t s : {pair_q[a], pair_t[a]}) {
            if (seq_off[s] > bytes || seq_len[s] > bytes - seq_off[s])
                return fail(c, DAGCON_ERR_INVALID_ARG, "pair %u: sequence %u runs past the blob", a, s);
            if (seq_len[s] > DG_PLACE_MAX_LEN)
                return fail(c, DAGCON_ERR_UNSUPPORTED, "pair %u: sequence %u has %u bases, more than %u", a, s, seq_len[s], DG_PLACE_MAX_LEN);
            n_seq = std::max<uint64_t>(n_seq, (uint64_t)s + 1);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    // pairs in target order (counting sort), a table per distinct target, groups of tables
    std::vector<uint32_t> first(n_seq + 1, 0);
    for (uint32_t a = 0; a < n_pairs; a++) first[pair_t[a] + 1]++;
    for (uint64_t s = 0; s < n_seq; s++) first[s + 1] += first[s];
    std::vector<uint32_t> pid(n_pairs), pq(n_pairs), pt(n_pairs), ptab(n_pairs);
    {
        std::vector<uint32_t> fill(first.begin(), first.end() - 1);
        for (uint32_t a = 0; a < n_pairs; a++) pid[fill[pair_t[a]]++] = a;
    }
    std::vector<uint32_t> tab_seq, tab_mask;
    std::vector<uint64_t> tab_base;                 // counted from its group's first slot
    struct Group { uint32_t tab0, tab1, pair0, pair1, nb; uint64_t slots; };
    std::vector<Group> groups;
    Group g{0, 0, 0, 0, 1, 0};
    uint64_t max_slots = 0;
    for (uint64_t s = 0; s < n_seq; s++) {
        if (first[s] == first[s + 1]) continue;
        const uint32_t lt = seq_len[s];
        const uint64_t nk = lt >= k ? lt - k + 1 : 0;
        uint64_t slots = 64;
        while (slots < 2 * nk) slots <<= 1;
        if (g.slots + slots > DG_PLACE_SLOT_BUDGET && g.tab1 > g.tab0) {
            groups.push_back(g);
            max_slots = std::max(max_slots, g.slots);
            g = Group{g.tab1, g.tab1, g.pair1, g.pair1, 1, 0};
        }
        const uint32_t tb = (uint32_t)tab_seq.size();
        tab_seq.push_back((uint32_t)s); tab_base.push_back(g.slots); tab_mask.push_back((uint32_t)(slots - 1));
        g.slots += slots;
        g.tab1 = tb + 1;
        for (uint32_t x = first[s]; x < first[s + 1]; x++) {
            const uint32_t a = pid[x];
            pq[x] = pair_q[a]; pt[x] = pair_t[a]; ptab[x] = tb - g.tab0;
            const uint32_t lq = seq_len[pair_q[a]];
            if (lq >= k && lt >= k) g.nb = std::max(g.nb, ((lt - k + lq) >> DG_PLACE_BIN_SHIFT) + 1);
        }
        g.pair1 = first[s + 1];
    }
    groups.push_back(g);
    max_slots = std::max(max_slots, g.slots);

    DevBuf &dblob = c->d_pl[0], &doff = c->d_pl[1], &dlen = c->d_pl[2], &dtseq = c->d_pl[3], &dtbase = c->d_pl[4],
           &dtmask = c->d_pl[5], &dslots = c->d_pl[6], &dpq = c->d_pl[7], &dpt = c->d_pl[8], &dptab = c->d_pl[9],
           &dpid = c->d_pl[10], &dvotes = c->d_pl[11], &dspan = c->d_pl[12], &dstrand = c->d_pl[13];
    hipStream_t st = c->stream;
    const uint32_t n_tab = (uint32_t)tab_seq.size();
    ENSURE(c, dblob, bytes); ENSURE(c, doff, n_seq * 8); ENSURE(c, dlen, n_seq * 4);
    ENSURE(c, dtseq, (size_t)n_tab * 4); ENSURE(c, dtbase, (size_t)n_tab * 8); ENSURE(c, dtmask, (size_t)n_tab * 4);
    ENSURE(c, dslots, max_slots * sizeof(DgPlaceSlot));
    ENSURE(c, dpq, (size_t)n_pairs * 4); ENSURE(c, dpt, (size_t)n_pairs * 4); ENSURE(c, dptab, (size_t)n_pairs * 4);
    ENSURE(c, dpid, (size_t)n_pairs * 4); ENSURE(c, dvotes, (size_t)n_pairs * 8); ENSURE(c, dspan, (size_t)n_pairs * 8);
    ENSURE(c, dstrand, n_pairs);
    if (bytes) HIPCHK(c, hipMemcpyAsync(dblob.p, blob, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(doff.p, seq_off, n_seq * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dlen.p, seq_len, n_seq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dtseq.p, tab_seq.data(), (size_t)n_tab * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dtbase.p, tab_base.data(), (size_t)n_tab * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dtmask.p, tab_mask.data(), (size_t)n_tab * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dpq.p, pq.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dpt.p, pt.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dptab.p, ptab.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dpid.p, pid.data(), (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
    DgPlaceParams pp;
    pp.blob = (const uint8_t *)dblob.p; pp.seq_off = (const uint64_t *)doff.p; pp.seq_len = (const uint32_t *)dlen.p;
    pp.slots = (DgPlaceSlot *)dslots.p;
    pp.votes_fwd = (uint32_t *)dvotes.p; pp.votes_rev = (uint32_t *)dvotes.p + n_pairs;
    pp.t0 = (uint32_t *)dspan.p; pp.t1 = (uint32_t *)dspan.p + n_pairs; pp.strand = (uint8_t *)dstrand.p;
    pp.k = k; pp.max_occ = max_occ;
    for (const Group &gr : groups) {
        HIPCHK(c, hipMemsetAsync(dslots.p, 0, gr.slots * sizeof(DgPlaceSlot), st));
        pp.tab_seq = (const uint32_t *)dtseq.p + gr.tab0; pp.tab_base = (const uint64_t *)dtbase.p + gr.tab0;
        pp.tab_mask = (const uint32_t *)dtmask.p + gr.tab0;
        pp.pq = (const uint32_t *)dpq.p + gr.pair0; pp.pt = (const uint32_t *)dpt.p + gr.pair0;
        pp.ptab = (const uint32_t *)dptab.p + gr.pair0; pp.pid = (const uint32_t *)dpid.p + gr.pair0;
        hipLaunchKernelGGL(k_place_index, dim3(gr.tab1 - gr.tab0), dim3(DG_PLACE_THREADS), 0, st, pp);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_place_vote, dim3(gr.pair1 - gr.pair0), dim3(DG_PLACE_THREADS), (size_t)6 * gr.nb * 4, st, pp);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, d2h(c, votes_fwd, dvotes.p, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, votes_rev, (const uint32_t *)dvotes.p + n_pairs, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, t0, dspan.p, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, t1, (const uint32_t *)dspan.p + n_pairs, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, strand, dstrand.p, n_pairs));
    return DAGCON_OK;
}

// main.cpp:117-145 with -a in one call: every record re-aligned (SimpleAligner.cpp:25-63), start / end / strand as
// SimpleAligner.cpp:51-62, then the usual path; the aligned strings never leave the device
int dagcon_consensus_pre(dagcon_ctx *ctx, const dagcon_pre_batch *b, dagcon_results *results) {
    if (!ctx || !b || !results) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    const uint32_t T = b->n_targets;
    if (T && (!b->tlen || !b->rec_begin)) return fail(c, DAGCON_ERR_INVALID_ARG, "tlen/rec_begin is NULL");
    const uint64_t n64 = T ? b->rec_begin[T] : 0;
    if (n64 > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many records");
    const uint32_t n = (uint32_t)n64;
    if (n && (!b->tstart || !b->strand || !b->q_off || !b->q_len || !b->t_off || !b->t_len || !b->q_blob || !b->t_blob))
        return fail(c, DAGCON_ERR_INVALID_ARG, "record arrays are NULL");
    c->align_n = 0;
    std::vector<uint64_t> out_off(n);
    std::vector<uint32_t> alen(n, 0), start(n);
    uint64_t tot = 0;
    for (uint32_t a = 0; a < n; a++) { out_off[a] = tot; tot += ((uint64_t)b->q_len[a] + b->t_len[a] + 15ull) & ~15ull; }
    uint64_t out_bytes = 0;
    if (n) {
        int r = align_device(c, n, b->q_off, b->q_len, b->t_off, b->t_len, b->q_blob, b->q_bytes, b->t_blob, b->t_bytes,
                             out_off.data(), alen.data(), &out_bytes);
        if (r != DAGCON_OK) return r;
    }
    // SimpleAligner.cpp:51-62: start = tstart + GenomicTBegin(), end = start + the aligned target span (global:
    // GenomicTBegin() = 0, the span |tseq|; DAGCON_FLAG_LOCAL_ALIGN: t_begin, t_end - t_begin)
    const bool local = (c->opts.flags & DAGCON_FLAG_LOCAL_ALIGN) != 0;
    std::vector<uint32_t> rc_list;
    for (uint32_t g = 0; g < T; g++) {
        if (b->rec_begin[g + 1] < b->rec_begin[g] || b->rec_begin[g + 1] > n64) return fail(c, DAGCON_ERR_INVALID_ARG, "rec_begin not monotone at target %u", g);
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            uint32_t st = b->tstart[a];
            uint32_t en = st + b->t_len[a];
            if (local) { en = st + c->h_ends[a * 4 + 3]; st += c->h_ends[a * 4 + 2]; }
            if (b->strand[a] == '-') { st = b->tlen[g] - en; if (alen[a]) rc_list.push_back((uint32_t)a); }
            start[a] = st + 1u;
        }
    }
    if (!rc_list.empty()) {
        DevBuf &didx = c->d_al[12];
        HIPCHK(c, hipMemcpyAsync(didx.p, rc_list.data(), rc_list.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_align_revcomp, dim3((uint32_t)rc_list.size()), dim3(64), 0, c->stream,
                           (uint8_t *)c->d_al[7].p, (uint8_t *)c->d_al[8].p, (const uint64_t *)c->d_al[6].p,
                           (const uint32_t *)c->d_al[9].p, (const uint32_t *)didx.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));       // (rc_list is a local)
    }
    dagcon_batch db;
    memset(&db, 0, sizeof db);
    db.n_targets = T; db.tlen = b->tlen; db.aln_begin = b->rec_begin;
    db.aln_start = start.data(); db.aln_off = out_off.data(); db.aln_len = alen.data();
    db.blob_bytes = n ? out_bytes : 0;
    int r = upload_impl(ctx, &db, n ? c->d_al[7].p : nullptr, n ? c->d_al[8].p : nullptr);
    if (r != DAGCON_OK) return r;
    if ((r = dagcon_run(ctx)) != DAGCON_OK) return r;
    return dagcon_fetch(ctx, results);
}

}  // extern "C"
namespace {
// ---- record intake: dagcon_upload_cigar, _windows, _packed, _strand and dagcon_upload_cs ------------------------------
// One path, upload_records: reset, scan, judge, rate, pick, plan, expand, hand-over.  Whole targets and windows differ in
// the plan alone (plan_whole / plan_windows); the input kinds differ in what cigar_scan uploads and in the kernels
// cigar_rate and cigar_expand pick, both read off a RecordSource.  rate runs only when a record filter is set.

// what dagcon_upload_cs leaves for the path: every record judged and sized from its text
struct CsDecoded {
    std::vector<const char *> why;                                 // per record: nullptr: conforming
    std::vector<uint32_t> tot;                                     // per record, as CigarScan::tot
};

// Where a batch's read bases and ops come from: a kind and what that kind alone carries; no other pairing can be built.
//   PLAIN / PACKED  q_blob holds one base a byte / two (a record takes (q_len + 1) / 2 bytes from q_off)
//   STRANDED        one base a byte and a flag per record: != 0, the ops are written against the reverse complement
//   DECODED         dagcon_upload_cs: ops, reads and targets are on the device already (CigarBufs::ops, q, t, made by
//                   k_cs_write), b->ops and b->q_blob are NULL, b->q_off is the host's prefix sum of q_len; the scan's totals
//                   must be k_cs_scan's for every conforming record, and the path goes on with k_cs_scan's
class RecordSource {
  public:
    enum Kind { PLAIN, PACKED, STRANDED, DECODED };
    static RecordSource plain() { return RecordSource(PLAIN, nullptr); }
    static RecordSource packed() { return RecordSource(PACKED, nullptr); }
    static RecordSource stranded(const uint8_t *reverse) { return reverse ? RecordSource(STRANDED, reverse) : plain(); }
    static RecordSource decoded(const CsDecoded &cs) { return RecordSource(DECODED, &cs); }
    Kind kind() const { return kind_; }
    const uint8_t *reverse() const { return kind_ == STRANDED ? static_cast<const uint8_t *>(carried_) : nullptr; }
    const CsDecoded *cs() const { return kind_ == DECODED ? static_cast<const CsDecoded *>(carried_) : nullptr; }

  private:
    RecordSource(Kind k, const void *carried) : kind_(k), carried_(carried) {}
    Kind kind_;
    const void *carried_;
};

// reset: what any upload does to the context's state first
Ctx *intake_reset(dagcon_ctx *ctx) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->uploaded = c->ran = c->fetched = false;
    c->sup_valid = c->pos_valid = false;
    c->ed_batch = c->ed_valid = c->pos_pending = false;
    return c;
}

// the checks a dagcon_cigar_batch and a dagcon_cs_batch share: the targets, their records' ranges, and the record count
int check_targets(Ctx *c, uint32_t T, const uint32_t *tlen, const uint64_t *t_off, const uint64_t *rec_begin, const char *t_blob, uint64_t t_bytes,
                  bool have_record_arrays, uint32_t &n) {
    if (T && (!tlen || !rec_begin || !t_off)) return fail(c, DAGCON_ERR_INVALID_ARG, "tlen/t_off/rec_begin is NULL");
    const uint64_t n64 = T ? rec_begin[T] : 0;
    if (n64 > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many records");
    n = (uint32_t)n64;
    if (n && !have_record_arrays) return fail(c, DAGCON_ERR_INVALID_ARG, "record arrays are NULL");
    if (T && rec_begin[0] != 0) return fail(c, DAGCON_ERR_INVALID_ARG, "rec_begin does not start at 0");
    for (uint32_t g = 0; g < T; g++) {
        if (rec_begin[g + 1] < rec_begin[g] || rec_begin[g + 1] > n64) return fail(c, DAGCON_ERR_INVALID_ARG, "rec_begin not monotone at target %u", g);
        if (t_off[g] > t_bytes || tlen[g] > t_bytes - t_off[g]) return fail(c, DAGCON_ERR_INVALID_ARG, "target %u runs past t_blob", g);
        if (tlen[g] && !t_blob) return fail(c, DAGCON_ERR_INVALID_ARG, "t_blob is NULL");
    }
    return DAGCON_OK;
}

// scan: the checks of the batch, its upload, k_cigar_scan and the totals back on the host; p is left ready for an
// expansion but for what the plan decides (t_base, the offsets)
struct CigarScan {
    uint32_t n = 0;                                                // records
    DgCigarParams p;
    std::vector<uint64_t> tile_begin;                              // [n + 1]
    std::vector<uint32_t> tot;                                     // per record: columns, read bases, target bases, DG_CG_* flags
    DgCigarStrand st = {nullptr, nullptr};                         // cigar_strand: the strand kernels' own arguments
};
int cigar_scan(Ctx *c, const dagcon_cigar_batch *b, const RecordSource &src, CigarScan &sc) {
    const CsDecoded *cs = src.cs();
    const bool packed = src.kind() == RecordSource::PACKED;
    uint32_t n = 0;
    int r = check_targets(c, b->n_targets, b->tlen, b->t_off, b->rec_begin, b->t_blob, b->t_bytes, b->pos && b->q_off && b->q_len && b->op_begin, n);
    if (r != DAGCON_OK) return r;
    std::vector<uint64_t> &tile_begin = sc.tile_begin;
    tile_begin.assign((size_t)n + 1, 0);
    for (uint32_t a = 0; a < n; a++) {
        if (b->op_begin[a + 1] < b->op_begin[a]) return fail(c, DAGCON_ERR_INVALID_ARG, "op_begin not monotone at record %u", a);
        const uint64_t qb = packed ? ((uint64_t)b->q_len[a] + 1u) / 2u : b->q_len[a];
        if (b->q_off[a] > b->q_bytes || qb > b->q_bytes - b->q_off[a]) return fail(c, DAGCON_ERR_INVALID_ARG, "record %u runs past q_blob", a);
        if (b->q_len[a] && !b->q_blob && !cs) return fail(c, DAGCON_ERR_INVALID_ARG, "q_blob is NULL");
        tile_begin[a + 1] = tile_begin[a] + (b->op_begin[a + 1] - b->op_begin[a] + 63u) / 64u;
    }
    const uint64_t n_ops = n ? b->op_begin[n] - b->op_begin[0] : 0, n_tiles = tile_begin[n];
    if (n_ops && !b->ops && !cs) return fail(c, DAGCON_ERR_INVALID_ARG, "ops is NULL");
    if (n_tiles > 0x7FFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many CIGAR ops");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    CigarBufs &d = c->cg;
    // op_begin as the caller has it, less its first entry (ops are uploaded from there)
    std::vector<uint64_t> opb((size_t)n + 1, 0);
    for (uint32_t a = 0; a <= n && n; a++) opb[a] = b->op_begin[a] - b->op_begin[0];
    ENSURE(c, d.ops, n_ops * 4); ENSURE(c, d.totals, (size_t)n * 16); ENSURE(c, d.ckpt, n_tiles * 16);
    ENSURE(c, d.q, b->q_bytes); ENSURE(c, d.t, b->t_bytes); ENSURE(c, d.q_off, (size_t)n * 8);
    if (n_ops && !cs) HIPCHK(c, hipMemcpyAsync(d.ops.p, b->ops + b->op_begin[0], n_ops * 4, hipMemcpyHostToDevice, s));
    if (b->q_bytes && b->q_blob) HIPCHK(c, hipMemcpyAsync(d.q.p, b->q_blob, b->q_bytes, hipMemcpyHostToDevice, s));
    if (b->t_bytes && b->t_blob && !cs) HIPCHK(c, hipMemcpyAsync(d.t.p, b->t_blob, b->t_bytes, hipMemcpyHostToDevice, s));
    if (n) HIPCHK(c, hipMemcpyAsync(d.q_off.p, b->q_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if ((r = upload_vec(c, d.op_begin, opb))) return r;
    if ((r = upload_vec(c, d.tile_begin, tile_begin))) return r;
    DgCigarParams &p = sc.p;
    memset(&p, 0, sizeof p);
    p.ops = (const uint32_t *)d.ops.p; p.op_begin = (const uint64_t *)d.op_begin.p; p.tile_begin = (const uint64_t *)d.tile_begin.p;
    p.n = n; p.n_tiles = (uint32_t)n_tiles;
    p.totals = (uint4 *)d.totals.p; p.ckpt = (uint4 *)d.ckpt.p;
    p.q = (const uint8_t *)d.q.p; p.t = (const uint8_t *)d.t.p; p.q_off = (const uint64_t *)d.q_off.p;
    std::vector<uint32_t> &tot = sc.tot;
    tot.assign((size_t)n * 4, 0);
    if (n) {
        hipLaunchKernelGGL(k_cigar_scan, dim3((n + 3u) / 4u), dim3(256), 0, s, p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, d2h(c, tot.data(), d.totals.p, (size_t)n * 16));
    }
    if (cs) {
        for (uint32_t a = 0; a < n; a++)
            if (!cs->why[a] && memcmp(&tot[(size_t)a * 4], &cs->tot[(size_t)a * 4], 16) != 0)
                return fail(c, DAGCON_ERR_INTERNAL, "k_cs_write: the ops of record %u sum to %u columns, %u read bases, %u target bases, flags %u; k_cs_scan said %u, %u, %u", a,
                            tot[(size_t)a * 4], tot[(size_t)a * 4 + 1], tot[(size_t)a * 4 + 2], tot[(size_t)a * 4 + 3], cs->tot[(size_t)a * 4], cs->tot[(size_t)a * 4 + 1], cs->tot[(size_t)a * 4 + 2]);
        tot = cs->tot;
    }
    sc.n = n;
    return DAGCON_OK;
}

// judge: why each record is non-conforming (include/dagcon.h; nullptr: it conforms), and the text of the first that is
struct CigarVerdict {
    std::vector<const char *> why;                                 // [n]
    std::string first_err;
};
CigarVerdict cigar_judge(const dagcon_cigar_batch *b, const RecordSource &src, const CigarScan &sc) {
    CigarVerdict v;
    v.why.assign((size_t)sc.n, nullptr);
    for (uint32_t g = 0; g < b->n_targets; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            const uint32_t nq = sc.tot[a * 4 + 1], nt = sc.tot[a * 4 + 2], fl = sc.tot[a * 4 + 3];
            const char *why = src.cs() ? src.cs()->why[a]
                            : (fl & DG_CG_BAD_OP) ? "an op code above 8 or N"
                            : (fl & DG_CG_ZERO_LEN) ? "an op of length 0"
                            : (fl & DG_CG_OVERFLOW) ? "a total past 32 bits"
                            : b->pos[a] == 0 ? "pos is 0"
                            : nq != b->q_len[a] ? "the ops do not consume exactly q_len read bases"
                            : (uint64_t)b->pos[a] - 1u + nt > b->tlen[g] ? "target bases past tlen" : nullptr;
            v.why[a] = why;
            if (why && v.first_err.empty()) {
                char buf[256];
                snprintf(buf, sizeof buf, "target %u: record %llu is non-conforming (%s)", g, (unsigned long long)a, why);
                v.first_err = buf;
            }
        }
    return v;
}

// the strand kernels' own arguments, one flag and q_len per record: uploaded once, by whichever stage asks first
int cigar_strand(Ctx *c, const dagcon_cigar_batch *b, const RecordSource &src, CigarScan &sc) {
    if (src.kind() != RecordSource::STRANDED || sc.st.rev) return DAGCON_OK;
    ENSURE(c, c->cg.rev, (size_t)sc.n); ENSURE(c, c->cg.q_len, (size_t)sc.n * 4);
    if (sc.n) {
        HIPCHK(c, hipMemcpyAsync(c->cg.rev.p, src.reverse(), (size_t)sc.n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->cg.q_len.p, b->q_len, (size_t)sc.n * 4, hipMemcpyHostToDevice, c->stream));
    }
    sc.st.rev = (const uint8_t *)c->cg.rev.p; sc.st.q_len = (const uint32_t *)c->cg.q_len.p;
    return DAGCON_OK;
}

// rate and pick (dagcon_set_record_filter; include/dagcon.h has the rule): which records the plan is to see.  Without a
// filter every record is kept and nothing is launched.
struct CigarPick {
    std::vector<uint8_t> keep;                                     // [n] 0: over max_error (a non-conforming record stays: it fails its target as ever)
    uint32_t max_depth = 0;                                        // 0: off
    std::vector<uint32_t> rate;                                    // [n] x4 match, mismatch, ins, del (a filter is set)
    std::vector<uint8_t> fate;                                     // [n] DAGCON_FATE_* (a filter is set)
};

// rate: k_cigar_rate over the tiles of the conforming records, k_cigar_rate_sum over the records, the counts back on the
// host and checked against the scan's column totals before anything is decided from them
int cigar_rate(Ctx *c, const dagcon_cigar_batch *b, const RecordSource &src, CigarScan &sc, const CigarVerdict &v, CigarPick &pk) {
    const uint32_t n = sc.n;
    pk.rate.assign((size_t)n * 4, 0);
    if (!n) return DAGCON_OK;
    std::vector<uint64_t> base((size_t)n, DG_CG_SKIP);
    for (uint32_t g = 0; g < b->n_targets; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++)
            if (!v.why[a]) base[a] = b->t_off[g] + b->pos[a] - 1u;
    CigarBufs &d = c->cg;
    int r;
    if ((r = upload_vec(c, d.rate_base, base))) return r;
    if ((r = cigar_strand(c, b, src, sc))) return r;
    ENSURE(c, d.tile_rate, (size_t)sc.p.n_tiles * 16); ENSURE(c, d.rate, (size_t)n * 16);
    DgCigarRate rt;
    rt.base = (const uint64_t *)d.rate_base.p; rt.tile_rate = (uint4 *)d.tile_rate.p; rt.rate = (uint4 *)d.rate.p;
    hipStream_t s = c->stream;
    if (sc.p.n_tiles) {
        const dim3 grid(sc.p.n_tiles), block(64);
        switch (src.kind()) {
        case RecordSource::STRANDED: hipLaunchKernelGGL(k_cigar_rate_strand, grid, block, 0, s, sc.p, rt, sc.st); break;
        case RecordSource::PACKED: hipLaunchKernelGGL(k_cigar_rate_packed, grid, block, 0, s, sc.p, rt); break;
        case RecordSource::PLAIN:
        case RecordSource::DECODED: hipLaunchKernelGGL(k_cigar_rate, grid, block, 0, s, sc.p, rt); break;
        }
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cigar_rate_sum, dim3((n + 3u) / 4u), dim3(256), 0, s, sc.p, rt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, d2h(c, pk.rate.data(), d.rate.p, (size_t)n * 16));
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t *k = &pk.rate[(size_t)a * 4];
        const uint64_t sum = (uint64_t)k[0] + k[1] + k[2] + k[3];
        if (sum != (v.why[a] ? 0u : sc.tot[(size_t)a * 4]))
            return fail(c, DAGCON_ERR_INTERNAL, "k_cigar_rate: record %u has %u + %u + %u + %u of %u columns", a, k[0], k[1], k[2], k[3], sc.tot[(size_t)a * 4]);
    }
    return DAGCON_OK;
}

// pick, first step: the error threshold, record by record
void cigar_pick(const dagcon_record_filter &f, const CigarVerdict &v, CigarPick &pk) {
    const size_t n = v.why.size();
    pk.fate.assign(n, 0);
    pk.max_depth = f.max_depth;
    for (size_t a = 0; a < n; a++) {
        if (v.why[a]) { pk.fate[a] = DAGCON_FATE_NONCONFORMING; continue; }
        const uint32_t *k = &pk.rate[a * 4];
        const uint64_t err = (uint64_t)k[1] + k[2] + k[3], col = err + k[0];
        if (err * 1000000ull > (uint64_t)f.max_error_ppm * col) { pk.fate[a] = DAGCON_FATE_MAX_ERROR; pk.keep[a] = 0; }
    }
}

// pick, second step: the depth cap on one target's or one window's records, recs in their own order.  More than
// max_depth: the max_depth with the largest match stay (a tie goes to the lower record index), in their own order;
// take[i] says whether recs[i] does.  Empty: all stay
std::vector<uint8_t> cap_depth(CigarPick &pk, const std::vector<uint32_t> &recs) {
    std::vector<uint8_t> take;
    if (!pk.max_depth || recs.size() <= pk.max_depth) return take;
    std::vector<uint32_t> by_match(recs.size());
    for (uint32_t i = 0; i < by_match.size(); i++) by_match[i] = i;
    std::stable_sort(by_match.begin(), by_match.end(), [&](uint32_t x, uint32_t y) { return pk.rate[(size_t)recs[x] * 4] > pk.rate[(size_t)recs[y] * 4]; });
    take.assign(recs.size(), 0);
    for (uint32_t i = 0; i < pk.max_depth; i++) take[by_match[i]] = 1;
    for (size_t i = 0; i < recs.size(); i++)
        if (!take[i]) pk.fate[recs[i]] |= DAGCON_FATE_MAX_DEPTH;
    return take;
}

// plan: what upload_impl is to see (a dagcon_batch of strings, planned as dagcon_consensus_pre plans them), where the
// expansion writes them (set in sc.p, and cw for pieces), and how many waves it takes (0: nothing to expand)
struct CigarPlan {
    std::vector<uint8_t> bad;                                      // per target of the pipeline: it holds a non-conforming record
    std::vector<uint32_t> tlen;                                    // windows: the pipeline's targets (whole: the batch's own)
    std::vector<uint64_t> beg, off;                                // aln_begin, aln_off
    std::vector<uint32_t> start, len;                              // aln_start, aln_len
    uint64_t bytes = 0;                                            // of each string blob
    bool pieces = false;                                           // the expansion is k_cigar_expand_cut's, over cw
    DgCigarCutParams cw;
    uint32_t waves = 0;
};

// whole targets: one record, one string; the targets with a non-conforming record lose all their records (a target below
// min_cov is skipped whatever it holds: it goes in without records, and nothing of it is expanded).  min_cov counts the
// records the pick left
int plan_whole(Ctx *c, const dagcon_cigar_batch *b, CigarScan &sc, const CigarVerdict &v, CigarPick &pk, CigarPlan &pl) {
    const uint32_t T = b->n_targets, n = sc.n;
    pl.bad.assign(T, 0);
    for (uint32_t g = 0; g < T; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++)
            if (v.why[a]) pl.bad[g] = 1;
    std::vector<uint64_t> out_off((size_t)n, DG_CG_SKIP), t_base((size_t)n, 0);
    pl.beg.assign((size_t)T + 1, 0);
    std::vector<uint32_t> recs;
    for (uint32_t g = 0; g < T; g++) {
        pl.beg[g] = pl.start.size();
        recs.clear();
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++)
            if (pk.keep[a] && !v.why[a]) recs.push_back((uint32_t)a);
        const std::vector<uint8_t> take = cap_depth(pk, recs);
        if (!take.empty()) {
            size_t to = 0;
            for (size_t i = 0; i < recs.size(); i++)
                if (take[i]) recs[to++] = recs[i];
            recs.resize(to);
        }
        const uint64_t k = recs.size();
        if (pl.bad[g] || k == 0 || k < c->opts.min_cov) continue;
        for (const uint32_t a : recs) {
            out_off[a] = pl.bytes; t_base[a] = b->t_off[g] + b->pos[a] - 1u;
            pl.start.push_back(b->pos[a]); pl.off.push_back(pl.bytes); pl.len.push_back(sc.tot[a * 4]);
            pl.bytes += ((uint64_t)sc.tot[a * 4] + 15ull) & ~15ull;
        }
    }
    pl.beg[T] = pl.start.size();
    int r;
    if ((r = upload_vec(c, c->cg.t_base, t_base))) return r;
    if ((r = upload_vec(c, c->cg.out_off, out_off))) return r;
    sc.p.t_base = (const uint64_t *)c->cg.t_base.p; sc.p.out_off = (const uint64_t *)c->cg.out_off.p;
    pl.waves = pl.bytes ? sc.p.n_tiles : 0u;
    return DAGCON_OK;
}

int check_windows(Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    const uint32_t T = b->n_targets, W = wn->n_windows;
    if (W && (!wn->target || !wn->begin || !wn->end)) return fail(c, DAGCON_ERR_INVALID_ARG, "window arrays are NULL");
    if (T && !b->tlen) return fail(c, DAGCON_ERR_INVALID_ARG, "tlen/t_off/rec_begin is NULL");
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t g = wn->target[w];
        if (g >= T) return fail(c, DAGCON_ERR_INVALID_ARG, "window %u: target %u out of range", w, g);
        if (wn->end[w] <= wn->begin[w] || wn->end[w] > b->tlen[g])
            return fail(c, DAGCON_ERR_INVALID_ARG, "window %u: [%u, %u) is empty or runs past tlen %u", w, wn->begin[w], wn->end[w], b->tlen[g]);
        if (w && (g < wn->target[w - 1] || (g == wn->target[w - 1] && wn->begin[w] < wn->begin[w - 1])))
            return fail(c, DAGCON_ERR_INVALID_ARG, "window %u is out of order (targets ascending, begins ascending inside a target)", w);
    }
    return DAGCON_OK;
}

// windows: every target cut into windows, each window a target of the pipeline (include/dagcon.h has the cut).  After
// the scan's totals the host knows every record's [s, e) and lists the (record, window) pieces; k_cigar_cut turns each
// piece's two target coordinates into columns and tiles, the host plans the output from those, and k_cigar_expand_cut
// writes every piece from the one device copy of the record's ops and bases.
int plan_windows(Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn, CigarScan &sc, const CigarVerdict &v, CigarPick &pk, CigarPlan &pl) {
    const uint32_t T = b->n_targets, W = wn->n_windows, n = sc.n;
    const std::vector<uint32_t> &tot = sc.tot;
    CigarBufs &d = c->cg;
    // every record's [s, e) in target bases.  A non-conforming record has whatever span its pos and its target-base
    // total give, clipped to the target and at least one base long: it fails the windows that span meets
    std::vector<uint32_t> rs((size_t)n), re((size_t)n);
    std::vector<uint64_t> t_base((size_t)n, 0);
    for (uint32_t g = 0; g < T; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            const uint64_t tl = b->tlen[g];
            uint64_t s0 = b->pos[a] ? b->pos[a] - 1u : 0u, e0 = s0 + tot[a * 4 + 2];
            if (v.why[a]) {
                if (tl && s0 > tl - 1) s0 = tl - 1;
                if (e0 < s0 + 1) e0 = s0 + 1;
                if (e0 > tl) e0 = tl;
            }
            rs[a] = (uint32_t)s0; re[a] = (uint32_t)e0;
            t_base[a] = b->t_off[g] + s0;
        }
    // the pieces, window by window, records in their own order (addAln order); a window with a non-conforming piece, or
    // with fewer pieces than min_cov after the pick, keeps none
    pl.bad.assign(W, 0);
    std::vector<uint32_t> recs;
    pl.beg.assign((size_t)W + 1, 0);
    std::vector<uint32_t> piece;                                   // x4: record, a_rel, b_rel, window
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t g = wn->target[w], wa = wn->begin[w], wb = wn->end[w];
        const size_t first = piece.size();
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            const uint32_t A = std::max(wa, rs[a]), B = std::min(wb, re[a]);
            if (A >= B) continue;
            if (v.why[a]) { pl.bad[w] = 1; continue; }
            if (!pk.keep[a]) continue;
            piece.push_back((uint32_t)a); piece.push_back(A - rs[a]); piece.push_back(B - rs[a]); piece.push_back(w);
        }
        size_t k = (piece.size() - first) / 4;
        recs.resize(k);
        for (size_t i = 0; i < k; i++) recs[i] = piece[first + i * 4];
        const std::vector<uint8_t> take = cap_depth(pk, recs);
        if (!take.empty()) {                                       // the pieces that stay, moved up in their own order
            size_t to = first;
            for (size_t i = 0; i < k; i++)
                if (take[i]) { std::copy_n(&piece[first + i * 4], 4, &piece[to]); to += 4; }
            piece.resize(to);
            k = (to - first) / 4;
        }
        if (pl.bad[w] || k < c->opts.min_cov) piece.resize(first);
    }
    const uint64_t np64 = piece.size() / 4;
    if (np64 > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many alignments");
    const uint32_t np = (uint32_t)np64;
    DgCigarCutParams &cw = pl.cw;
    memset(&cw, 0, sizeof cw);
    pl.pieces = true;
    std::vector<uint32_t> cut((size_t)np * 4);
    int r;
    if (np) {
        if ((r = upload_vec(c, d.piece, piece))) return r;
        ENSURE(c, d.cut, (size_t)np * 16);
        cw.piece = (const uint4 *)d.piece.p; cw.cut = (uint4 *)d.cut.p; cw.n_pieces = np;
        hipLaunchKernelGGL(k_cigar_cut, dim3((np + 3u) / 4u), dim3(256), 0, c->stream, sc.p, cw);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, d2h(c, cut.data(), d.cut.p, (size_t)np * 16));
    }
    // the output plan: nothing the device said is used before it has been checked against the record's own sizes
    std::vector<uint64_t> pout((size_t)np);
    std::vector<uint32_t> wbegin((size_t)np), wpiece;
    pl.off.resize(np); pl.start.resize(np); pl.len.resize(np);
    uint32_t cur = 0;
    for (uint32_t i = 0; i < np; i++) {
        const uint32_t a = piece[i * 4], w = piece[i * 4 + 3];
        const uint32_t ca = cut[i * 4], cb = cut[i * 4 + 1], ta = cut[i * 4 + 2], tb = cut[i * 4 + 3];
        const uint64_t ntile = sc.tile_begin[a + 1] - sc.tile_begin[a];
        if (ca > cb || cb > tot[a * 4] || ta > tb || tb >= ntile)
            return fail(c, DAGCON_ERR_INTERNAL, "k_cigar_cut: piece %u of record %u has columns [%u, %u), tiles [%u, %u] of %llu", i, a, ca, cb, ta, tb, (unsigned long long)ntile);
        while (cur < w) pl.beg[++cur] = i;
        pl.off[i] = pout[i] = pl.bytes;
        pl.len[i] = cb - ca;
        pl.start[i] = rs[a] + piece[i * 4 + 1] - wn->begin[w] + 1u;
        pl.bytes += ((uint64_t)(cb - ca) + 15ull) & ~15ull;
        if (wpiece.size() + (tb - ta + 1u) > 0x7FFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many CIGAR ops");
        wbegin[i] = (uint32_t)wpiece.size();
        wpiece.insert(wpiece.end(), tb - ta + 1u, i);
    }
    while (cur < W) pl.beg[++cur] = np;
    pl.tlen.resize(W);
    for (uint32_t w = 0; w < W; w++) pl.tlen[w] = wn->end[w] - wn->begin[w];
    if (np && pl.bytes) {
        if ((r = upload_vec(c, d.t_base, t_base))) return r;
        if ((r = upload_vec(c, d.wave_piece, wpiece))) return r;
        if ((r = upload_vec(c, d.wave_begin, wbegin))) return r;
        if ((r = upload_vec(c, d.piece_out, pout))) return r;
        sc.p.t_base = (const uint64_t *)d.t_base.p;
        cw.wave_piece = (const uint32_t *)d.wave_piece.p; cw.wave_begin = (const uint32_t *)d.wave_begin.p;
        cw.piece_out = (const uint64_t *)d.piece_out.p; cw.n_waves = (uint32_t)wpiece.size();
        pl.waves = cw.n_waves;
    }
    return DAGCON_OK;
}

// expand: the strings into d_q / d_t, a wave per tile (of a record, or of a piece), by the kernel of the source's kind
int cigar_expand(Ctx *c, const dagcon_cigar_batch *b, const RecordSource &src, CigarScan &sc, const CigarPlan &pl) {
    ENSURE(c, c->d_q, pl.bytes); ENSURE(c, c->d_t, pl.bytes);
    if (!pl.waves) return DAGCON_OK;
    DgCigarParams &p = sc.p;
    p.out_q = (uint8_t *)c->d_q.p; p.out_t = (uint8_t *)c->d_t.p;
    const dim3 grid(pl.waves), block(64);
    hipStream_t s = c->stream;
    switch (src.kind()) {
    case RecordSource::STRANDED: {
        const int r = cigar_strand(c, b, src, sc);
        if (r != DAGCON_OK) return r;
        if (pl.pieces) hipLaunchKernelGGL(k_cigar_expand_cut_strand, grid, block, 0, s, p, pl.cw, sc.st);
        else hipLaunchKernelGGL(k_cigar_expand_strand, grid, block, 0, s, p, sc.st);
        break;
    }
    case RecordSource::PACKED:
        if (pl.pieces) hipLaunchKernelGGL(k_cigar_expand_cut_packed, grid, block, 0, s, p, pl.cw);
        else hipLaunchKernelGGL(k_cigar_expand_packed, grid, block, 0, s, p);
        break;
    case RecordSource::PLAIN:
    case RecordSource::DECODED:
        if (pl.pieces) hipLaunchKernelGGL(k_cigar_expand_cut, grid, block, 0, s, p, pl.cw);
        else hipLaunchKernelGGL(k_cigar_expand, grid, block, 0, s, p);
        break;
    }
    HIPCHK(c, hipGetLastError());
    return DAGCON_OK;
}

// hand-over: the planned strings go in by the door dagcon_consensus_pre uses; the context remembers which of the
// pipeline's targets fail for a record, and why
int cigar_hand_over(dagcon_ctx *ctx, Ctx *c, const dagcon_cigar_batch *b, const CigarPlan &pl, const CigarVerdict &v, const CigarPick &pk) {
    dagcon_batch db;
    memset(&db, 0, sizeof db);
    db.n_targets = (uint32_t)pl.bad.size(); db.tlen = pl.pieces ? pl.tlen.data() : b->tlen; db.aln_begin = pl.beg.data();
    db.aln_start = pl.start.data(); db.aln_off = pl.off.data(); db.aln_len = pl.len.data();
    db.blob_bytes = pl.bytes;
    const int r = upload_impl(ctx, &db, c->d_q.p, c->d_t.p);       // (synchronises the stream: the caller's locals may go)
    if (r != DAGCON_OK) { (void)hipStreamSynchronize(c->stream); return r; }
    c->h_cig_bad = pl.bad;
    c->cig_err = v.first_err;
    if (c->filter_on) {                                            // dagcon_fetch_record_stats: one array per count
        const size_t n = pk.fate.size();
        c->rs_match.resize(n); c->rs_mismatch.resize(n); c->rs_ins.resize(n); c->rs_del.resize(n);
        for (size_t a = 0; a < n; a++) {
            c->rs_match[a] = pk.rate[a * 4]; c->rs_mismatch[a] = pk.rate[a * 4 + 1];
            c->rs_ins[a] = pk.rate[a * 4 + 2]; c->rs_del[a] = pk.rate[a * 4 + 3];
        }
        c->rs_fate = pk.fate;
        c->rs_valid = true;
    }
    return DAGCON_OK;
}

// dagcon_set_edits: the batch the hand-over left is one whose edits the run is to report.  Each of the pipeline's targets
// gets the place of its first base in cg.t (a window's: its target's, plus its begin), the status block a word for the
// edit count, the arena a first size (grown by the re-run when DG_E_ED_OVF says so)
int edits_arm(Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    const uint32_t T = c->T;
    c->h_ed_tbase.assign(T, 0);
    for (uint32_t t = 0; t < T; t++) c->h_ed_tbase[t] = wn ? b->t_off[wn->target[t]] + wn->begin[t] : b->t_off[t];
    c->ed_batch = true;
    c->ed_cap = c->ed_cap_env > 0 ? (uint64_t)c->ed_cap_env : std::max<uint64_t>(c->ed_cap, c->sum_bb / 8 + 1024);
    int r;
    if ((r = upload_vec(c, c->d_ed_tbase, c->h_ed_tbase))) return r;
    if ((r = ensure_stat(c, T))) return r;
    if ((r = ensure_arenas(c))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DAGCON_OK;
}

// SAM-style input: position + ungapped read + CIGAR per record, target bases once per target.  k_cigar_scan sizes every
// record, the host plans the string blobs as for any batch, the expansion writes them into d_q / d_t, and upload_impl
// takes them from there.  wn NULL: whole targets.  The strings never exist on the host.
int upload_records(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn, const RecordSource &src) {
    if (!ctx || !b) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = intake_reset(ctx);
    int r;
    if (wn && (r = check_windows(c, b, wn))) return r;
    CigarScan sc;
    if ((r = cigar_scan(c, b, src, sc))) return r;
    const CigarVerdict v = cigar_judge(b, src, sc);
    CigarPick pk;
    pk.keep.assign((size_t)sc.n, 1);
    if (c->filter_on) {
        if ((r = cigar_rate(c, b, src, sc, v, pk))) return r;
        cigar_pick(c->filter, v, pk);
    }
    CigarPlan pl;
    if ((r = wn ? plan_windows(c, b, wn, sc, v, pk, pl) : plan_whole(c, b, sc, v, pk, pl))) return r;
    if ((r = cigar_expand(c, b, src, sc, pl))) return r;
    if ((r = cigar_hand_over(ctx, c, b, pl, v, pk))) return r;
    return c->edits_on ? edits_arm(c, b, wn) : DAGCON_OK;
}

// minimap2's cs:Z: text per record, the target's bases once per target (include/dagcon.h has the rule).  k_cs_scan sizes
// and judges every record from the raw text; the host lays the conforming records' ops out without gaps and gives every
// record its q_len bytes of the read buffer; k_cs_write fills both on the device; from there the batch is a
// dagcon_cigar_batch whose ops, reads and targets are device-resident (upload_records with RecordSource::decoded)
int upload_cs(dagcon_ctx *ctx, const dagcon_cs_batch *b, const dagcon_windows *wn) {
    if (!ctx || !b) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = intake_reset(ctx);
    const uint32_t T = b->n_targets;
    uint32_t n = 0;
    int r = check_targets(c, T, b->tlen, b->t_off, b->rec_begin, b->t_blob, b->t_bytes, b->pos && b->q_len && b->cs_off && b->cs_len, n);
    if (r != DAGCON_OK) return r;
    std::vector<uint64_t> q_off((size_t)n + 1, 0);
    for (uint32_t a = 0; a < n; a++) {
        if (b->cs_off[a] > b->cs_bytes || b->cs_len[a] > b->cs_bytes - b->cs_off[a]) return fail(c, DAGCON_ERR_INVALID_ARG, "record %u runs past cs_blob", a);
        if (b->cs_len[a] && !b->cs_blob) return fail(c, DAGCON_ERR_INVALID_ARG, "cs_blob is NULL");
        q_off[a + 1] = q_off[a] + b->q_len[a];
    }
    const uint64_t q_bytes = q_off[n];
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    CsBufs &d = c->cs;
    CigarBufs &cg = c->cg;                                         // ops, q and t: what k_cs_write makes for cigar_scan
    ENSURE(c, d.text, b->cs_bytes); ENSURE(c, d.cs_off, (size_t)n * 8); ENSURE(c, d.cs_len, (size_t)n * 4);
    ENSURE(c, d.totals, (size_t)n * 16); ENSURE(c, d.n_ops, (size_t)n * 4); ENSURE(c, cg.t, b->t_bytes); ENSURE(c, cg.q, q_bytes);
    if (b->cs_bytes && b->cs_blob) HIPCHK(c, hipMemcpyAsync(d.text.p, b->cs_blob, b->cs_bytes, hipMemcpyHostToDevice, s));
    if (b->t_bytes && b->t_blob) HIPCHK(c, hipMemcpyAsync(cg.t.p, b->t_blob, b->t_bytes, hipMemcpyHostToDevice, s));
    DgCsParams p;
    memset(&p, 0, sizeof p);
    CsDecoded cs;
    cs.why.assign((size_t)n, nullptr);
    cs.tot.assign((size_t)n * 4, 0);
    std::vector<uint32_t> nops((size_t)n, 0);
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d.cs_off.p, b->cs_off, (size_t)n * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d.cs_len.p, b->cs_len, (size_t)n * 4, hipMemcpyHostToDevice, s));
        p.cs = (const uint8_t *)d.text.p; p.cs_off = (const uint64_t *)d.cs_off.p; p.cs_len = (const uint32_t *)d.cs_len.p; p.n = n;
        p.totals = (uint4 *)d.totals.p; p.n_ops = (uint32_t *)d.n_ops.p;
        hipLaunchKernelGGL(k_cs_scan, dim3((n + 3u) / 4u), dim3(256), 0, s, p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, d2h(c, cs.tot.data(), d.totals.p, (size_t)n * 16));
        HIPCHK(c, d2h(c, nops.data(), d.n_ops.p, (size_t)n * 4));
    }
    // what every record is; the ops of the conforming ones back to back, a read of q_len bytes each
    std::vector<uint64_t> opb((size_t)n + 1, 0), t_base((size_t)n, 0);
    std::vector<uint32_t> t_room((size_t)n, 0);
    for (uint32_t g = 0; g < T; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            uint32_t *tt = &cs.tot[a * 4];
            const uint32_t nq = tt[1], nt = tt[2], fl = tt[3];
            const uint32_t pos = b->pos[a], tl = b->tlen[g];
            const char *why = (fl & DG_CS_BAD_OP) ? "cs: a ~ op, or a first byte that starts no op"
                            : (fl & DG_CS_BAD_BODY) ? "cs: an op's body is empty, holds a byte that is no letter (no digit for :), is :0, has more than 9 digits or is 2^28 or more, or a * body is not two letters"
                            : (fl & DG_CG_OVERFLOW) ? "a total past 32 bits"
                            : pos == 0 ? "pos is 0"
                            : nq != b->q_len[a] ? "the cs ops do not produce exactly q_len read bases"
                            : (b->t_span && nt != b->t_span[a]) ? "the cs ops do not consume exactly t_span target bases"
                            : (uint64_t)pos - 1u + nt > tl ? "target bases past tlen" : nullptr;
            if (!why && nops[a] > b->cs_len[a] / 2u)
                return fail(c, DAGCON_ERR_INTERNAL, "k_cs_scan: record %llu has %u ops in %u bytes of text", (unsigned long long)a, nops[a], b->cs_len[a]);
            cs.why[a] = why;
            if (fl & (DG_CS_BAD_OP | DG_CS_BAD_BODY)) { tt[0] = 0; tt[1] = 0; tt[2] = b->t_span ? b->t_span[a] : 0u; }   // (no decoded totals: include/dagcon.h)
            opb[a + 1] = opb[a] + (why ? 0u : nops[a]);
            if (pos >= 1u && pos - 1u <= tl) { t_room[a] = tl - (pos - 1u); t_base[a] = b->t_off[g] + pos - 1u; }
        }
    const uint64_t n_ops = opb[n];
    ENSURE(c, cg.ops, n_ops * 4);
    if (n_ops) {
        if ((r = upload_vec(c, d.op_begin, opb))) return r;
        if ((r = upload_vec(c, d.t_base, t_base))) return r;
        if ((r = upload_vec(c, d.t_room, t_room))) return r;
        if ((r = upload_vec(c, d.q_off, q_off))) return r;
        ENSURE(c, d.q_len, (size_t)n * 4);
        HIPCHK(c, hipMemcpyAsync(d.q_len.p, b->q_len, (size_t)n * 4, hipMemcpyHostToDevice, s));
        p.op_begin = (const uint64_t *)d.op_begin.p; p.ops = (uint32_t *)cg.ops.p;
        p.t = (const uint8_t *)cg.t.p; p.t_base = (const uint64_t *)d.t_base.p; p.t_room = (const uint32_t *)d.t_room.p;
        p.q_off = (const uint64_t *)d.q_off.p; p.q_len = (const uint32_t *)d.q_len.p; p.q = (uint8_t *)cg.q.p;
        hipLaunchKernelGGL(k_cs_write, dim3((n + 3u) / 4u), dim3(256), 0, s, p);
        HIPCHK(c, hipGetLastError());
    }
    dagcon_cigar_batch cb;
    memset(&cb, 0, sizeof cb);
    cb.n_targets = T; cb.tlen = b->tlen; cb.t_off = b->t_off; cb.t_blob = b->t_blob; cb.t_bytes = b->t_bytes;
    cb.rec_begin = b->rec_begin; cb.pos = b->pos; cb.q_off = q_off.data(); cb.q_len = b->q_len; cb.q_bytes = q_bytes;
    cb.op_begin = opb.data();
    r = upload_records(ctx, &cb, wn, RecordSource::decoded(cs));
    if (r != DAGCON_OK) (void)hipStreamSynchronize(s);            // (the locals above may go)
    return r;
}

// what every dagcon_consensus_* of this intake is: upload, run, fetch
template <typename Upload>
int upload_run_fetch(dagcon_ctx *ctx, dagcon_results *results, Upload upload) {
    if (!results) return DAGCON_ERR_INVALID_ARG;
    int r = upload();
    if (r != DAGCON_OK) return r;
    if ((r = dagcon_run(ctx)) != DAGCON_OK) return r;
    return dagcon_fetch(ctx, results);
}
}  // namespace
extern "C" {

int dagcon_set_record_filter(dagcon_ctx *ctx, const dagcon_record_filter *f) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (f && f->max_error_ppm > 1000000u) return fail(c, DAGCON_ERR_INVALID_ARG, "max_error_ppm %u is above 1000000", f->max_error_ppm);
    if (f && f->max_depth > DAGCON_MAX_COVERAGE) return fail(c, DAGCON_ERR_INVALID_ARG, "max_depth %u is above %u", f->max_depth, DAGCON_MAX_COVERAGE);
    c->filter_on = f != nullptr;
    if (f) c->filter = *f;
    c->rs_valid = false;                                           // (the stats belong to an upload under the filter that is set)
    return DAGCON_OK;
}
int dagcon_fetch_record_stats(dagcon_ctx *ctx, dagcon_record_stats *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->filter_on || !c->rs_valid) return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_record_stats: no record upload under a record filter");
    out->n = c->rs_fate.size();
    out->match = c->rs_match.data(); out->mismatch = c->rs_mismatch.data(); out->ins = c->rs_ins.data(); out->del = c->rs_del.data();
    out->fate = c->rs_fate.data();
    return DAGCON_OK;
}
int dagcon_upload_cs(dagcon_ctx *ctx, const dagcon_cs_batch *b, const dagcon_windows *wn) { return upload_cs(ctx, b, wn); }
int dagcon_upload_cigar(dagcon_ctx *ctx, const dagcon_cigar_batch *b) { return upload_records(ctx, b, nullptr, RecordSource::plain()); }
int dagcon_upload_cigar_windows(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    return wn ? upload_records(ctx, b, wn, RecordSource::plain()) : DAGCON_ERR_INVALID_ARG;
}
// q_blob as a BAM record's seq field has it, two bases a byte (k_cigar.hip.h); windows may be NULL
int dagcon_upload_cigar_packed(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    return upload_records(ctx, b, wn, RecordSource::packed());
}
// q_blob as the reads file has it, reverse[r] != 0: the ops are written against the reverse complement (k_cigar.hip.h);
// windows and reverse may be NULL
int dagcon_upload_cigar_strand(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn, const uint8_t *reverse) {
    return upload_records(ctx, b, wn, RecordSource::stranded(reverse));
}

int dagcon_consensus_cs(dagcon_ctx *ctx, const dagcon_cs_batch *batch, const dagcon_windows *windows, dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cs(ctx, batch, windows); });
}
int dagcon_consensus_cigar(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cigar(ctx, batch); });
}
int dagcon_consensus_cigar_windows(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows, dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cigar_windows(ctx, batch, windows); });
}
int dagcon_consensus_cigar_packed(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows, dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cigar_packed(ctx, batch, windows); });
}
int dagcon_consensus_cigar_strand(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows, const uint8_t *reverse,
                                  dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cigar_strand(ctx, batch, windows, reverse); });
}

int dagcon_host_alloc(dagcon_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return DAGCON_OK;
}

void dagcon_host_free(dagcon_ctx *ctx, void *p) {
    if (!ctx || !p) return;
    (void)hipSetDevice(reinterpret_cast<Ctx *>(ctx)->device);
    (void)hipHostFree(p);
}

int dagcon_debug_graph(dagcon_ctx *ctx, uint32_t target, dagcon_graph_dump *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->ran) return fail(c, DAGCON_ERR_STATE, "dagcon_debug_graph before dagcon_run");
    if (target >= c->T) return fail(c, DAGCON_ERR_INVALID_ARG, "target out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t nb = 0, pb = 0;
    uint32_t N = 0, psz = 0;
    HIPCHK(c, d2h(c, &nb, (uint64_t *)c->d_node_base.p + target, 8));
    HIPCHK(c, d2h(c, &pb, (uint64_t *)c->d_pool_base.p + target, 8));
    HIPCHK(c, d2h(c, &N, (uint32_t *)c->d_n_nodes.p + target, 4));
    HIPCHK(c, d2h(c, &psz, (uint32_t *)c->d_pool_top.p + target, 4));
    if (!c->h_tactive[target]) N = 0;
    std::vector<DgNode> nd(N);
    std::vector<uint32_t> pool(psz);
    std::vector<int32_t> cov(c->h_tlen[target] + 2, 0);
    c->g_weight.assign(N, 0); c->g_cov.assign(N, 0);
    if (N) {
        HIPCHK(c, d2h(c, nd.data(), (DgNode *)c->d_nodes.p + nb, (size_t)N * sizeof(DgNode)));
        const uint32_t nbb = c->h_tlen[target] + 2;
        HIPCHK(c, d2h(c, cov.data(), (int32_t *)c->d_cov.p + c->h_bbv_base[target], (size_t)nbb * 4));
        if (psz) HIPCHK(c, d2h(c, pool.data(), (uint32_t *)c->d_pool.p + pb, (size_t)psz * 4));
    }
    c->g_base.assign(N, 0); c->g_deleted.assign(N, 0); c->g_backbone.assign(N, 0); c->g_bbpos.assign(N, 0);
    c->g_out_begin.assign(N + 1, 0); c->g_in_begin.assign(N + 1, 0);
    c->g_out_dst.clear(); c->g_out_cnt.clear(); c->g_in_src.clear();
    uint32_t nbb_seen = 0;
    for (uint32_t v = 0; v < N; v++) {
        c->g_base[v] = nd[v].base;
        c->g_weight[v] = nd[v].weight;
        c->g_deleted[v] = (nd[v].flags & DG_NF_DELETED) ? 1 : 0;
        c->g_backbone[v] = (nd[v].flags & DG_NF_BACKBONE) ? 1 : 0;
        if (c->g_backbone[v]) { c->g_bbpos[v] = (int32_t)nbb_seen; c->g_cov[v] = cov[nbb_seen]; nbb_seen++; }
        else c->g_bbpos[v] = nd[v].bbpos;
        c->g_out_begin[v] = (uint32_t)c->g_out_dst.size();
        c->g_in_begin[v] = (uint32_t)c->g_in_src.size();
        for (uint32_t i = 0; i < nd[v].out_len; i++) {
            c->g_out_dst.push_back((int32_t)pool[nd[v].out_off + 2 * i]);
            c->g_out_cnt.push_back((int32_t)pool[nd[v].out_off + 2 * i + 1]);
        }
        for (uint32_t i = 0; i < nd[v].in_len; i++) c->g_in_src.push_back((int32_t)pool[nd[v].in_off + i]);
    }
    c->g_out_begin[N] = (uint32_t)c->g_out_dst.size();
    c->g_in_begin[N] = (uint32_t)c->g_in_src.size();
    out->n_nodes = N;
    out->base = c->g_base.data(); out->weight = c->g_weight.data(); out->coverage = c->g_cov.data();
    out->deleted = c->g_deleted.data(); out->backbone = c->g_backbone.data(); out->bbpos = c->g_bbpos.data();
    out->out_begin = c->g_out_begin.data(); out->out_dst = c->g_out_dst.data(); out->out_count = c->g_out_cnt.data();
    out->in_begin = c->g_in_begin.data(); out->in_src = c->g_in_src.data();
    return DAGCON_OK;
}

}  // extern "C"
