// api_run.hip.h -- a batch through the pipeline: plan, arenas, parameters, launches; upload, run, fetch of the consensus with
// its support and positions, timings, normalize.  The optional outputs' side of every step is in api_outputs.hip.h
// (one translation unit with dagcon_api.hip, which includes it once).
namespace {

// what this fetch brings back and how much of it: decided once from the status block, read by the steps behind it
struct FetchPlan {
    bool full, want_sup, want_pos, lazy_pos, want_ed, want_evid, want_pile;       // (the outputs' own: outputs_plan)
    uint64_t nseg, nb, n_ed, n_site;
    size_t ed_seg_bytes, ed_bytes, evid_bytes;      // r_ed: the DgEdSeg records, then the DgEdit records, then the DgEvid records (all 8-byte aligned)
};

// the optional outputs' side of every step (api_outputs.hip.h)
void latch_outputs(Ctx *c, Intake kind);
int outputs_room(Ctx *c);
void outputs_params(Ctx *c, DgParams &p);
int outputs_launch(Ctx *c, const DgParams &p);
int outputs_upload(Ctx *c, const dagcon_batch *b);
int outputs_plan(Ctx *c, FetchPlan &f);
int outputs_copies(Ctx *c, const FetchPlan &f, bool &queued);
int outputs_unpack(Ctx *c, const FetchPlan &f);

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
    // the totals of the growing arenas whose output is on: 16 bytes each, or the second word of the arena's in front
    size_t prev = 0;
    for (const GrowRef &r : c->growing()) {
        r.g->o_top = !r.on ? 0 : r.g->own_word ? b.bytes : prev + 8;
        if (r.on && r.g->own_word) b.bytes += 16;
        prev = r.g->o_top;
    }
    ENSURE(c, b.dev, b.bytes);
    return b.host.reserve(c, b.bytes);
}

int ensure_arenas(Ctx *c) {
    ENSURE(c, c->arena.norm, c->norm_cap * sizeof(uint16_t));
    ENSURE(c, c->arena.nodes, c->node_cap * sizeof(DgNode));
    ENSURE(c, c->run.best, c->node_cap * 4);
    ENSURE(c, c->run.queue, c->node_cap * 4);
    ENSURE(c, c->run.score, c->node_cap * 8);
    ENSURE(c, c->run.bp_tt, c->node_cap * 4);
    if (c->gcuts) ENSURE(c, c->arena.score_b, c->node_cap * 4);
    ENSURE(c, c->run.cns_tmp, c->node_cap);
    ENSURE(c, c->arena.pool, c->pool_cap * 4);
    ENSURE(c, c->run.stk, std::max<uint64_t>((uint64_t)c->T * std::max(c->bp_max, c->seg_max), c->gcuts ? c->list_grid : 0) * c->stk_words * 4);
    if (c->gcuts) {
        ENSURE(c, c->run.worklist, (4ull + 3ull * c->worklist_cap) * 4);
        ENSURE(c, c->run.rd, (uint64_t)c->A * 16 + 16);
        ENSURE(c, c->run.pro_state, (uint64_t)c->T * 16 + 16);
        ENSURE(c, c->run.sh_cnt, (uint64_t)c->T * (2 + 2 * DG_SH_MAX) * 4 + 16);
        ENSURE(c, c->run.seg_done, (uint64_t)c->worklist_cap * (DG_SH_MAX + 1) * 4 + 16);
        ENSURE(c, c->run.wl_first, (uint64_t)c->T * 4 + 16);
        ENSURE(c, c->run.queue0, c->node_cap * 4);
        ENSURE(c, c->run.bp_end, (uint64_t)c->T * c->bp_max * 4 + 16);
        ENSURE(c, c->run.bp_ab, (uint64_t)c->T * c->bp_max * 16 + 16);
        ENSURE(c, c->run.defer, (uint64_t)c->T * (DG_DEFER_MAX + 1) * 4 + 16);
        ENSURE(c, c->run.cns_tmp0, c->node_cap);
    }
    ENSURE(c, c->run.cuts, (uint64_t)c->T * (c->seg_max + 2) * 4);
    ENSURE(c, c->run.cuts_bp, (uint64_t)c->T * (c->bp_max + 2) * 4);
    ENSURE(c, c->run.bp_stat, (uint64_t)c->T * c->bp_max * 8);
    ENSURE(c, c->run.bp_len, (uint64_t)c->T * c->bp_max * 4);
    ENSURE(c, c->run.cns, c->cns_cap);
    if (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT) {
        ENSURE(c, c->run.sup_tmp, c->node_cap * 4);
        if (c->gcuts) ENSURE(c, c->run.sup_tmp0, c->node_cap * 4);
        ENSURE(c, c->run.sup, c->cns_cap * 4);
    }
    if (c->opts.flags & DAGCON_FLAG_BASE_POS) {
        ENSURE(c, c->run.pos_tmp, c->node_cap * 4);
        if (c->gcuts) ENSURE(c, c->run.pos_tmp0, c->node_cap * 4);
        ENSURE(c, c->run.pos, c->cns_cap * 4);
    }
    if (int r = outputs_room(c)) return r;
    ENSURE(c, c->run.seg, 2 * seg_stride(c) * 4);
    if (int r = c->r_seg.reserve(c, 2 * (size_t)c->seg_cap * 4)) return r;
    ENSURE(c, c->arena.matC, matc_bytes(c) + 256);          // (grows for the re-run with 32-bit cells)
    return DAGCON_OK;
}

void fill_params(Ctx *c, DgParams &p) {
    memset(&p, 0, sizeof p);
    p.q = c->in.q.as<const uint8_t>(); p.t = c->in.t.as<const uint8_t>();
    p.aln_off = c->in.aln_off.as<const uint64_t>();
    p.aln_len = c->in.aln_len.as<const uint32_t>();
    p.aln_start = c->in.aln_start.as<const uint32_t>();
    p.aln_tgt = c->in.aln_tgt.as<const uint32_t>();
    p.tlen = c->in.tlen.as<const uint32_t>();
    p.aln_begin = c->in.aln_begin.as<const uint64_t>();
    p.tactive = c->in.tactive.as<const uint8_t>(); p.tfail = c->sb.d<uint32_t>(c->sb.o_tfail);
    p.bb = c->have_bb ? c->in.bb.as<const uint8_t>() : nullptr;
    p.bb_off = c->in.bb_off.as<const uint64_t>();
    p.mat_base = c->in.mat_base.as<const uint64_t>();
    p.matc_base = c->in.matc_base.as<const uint64_t>(); p.matc_stride = c->in.matc_stride.as<const uint32_t>();
    p.bbv_base = c->in.bbv_base.as<const uint64_t>();
    p.T = c->T; p.A = c->A;
    p.trim = c->opts.trim; p.min_len = c->opts.min_len;
    p.min_weight = c->opts.min_weight < 0 ? (int32_t)c->opts.min_cov : c->opts.min_weight;
    p.flags = c->opts.flags;
    p.max_k = c->max_k; p.max_tlen = c->max_tlen;
    p.nmis = c->run.nmis.as<uint32_t>(); p.norm_off = c->in.norm_off.as<uint64_t>();
    p.n_lo = c->run.n_lo.as<uint32_t>(); p.n_hi = c->run.n_hi.as<uint32_t>();
    p.n_start = c->run.n_start.as<uint32_t>(); p.n_ins = c->run.n_ins.as<uint32_t>();
    p.n_del = c->run.n_del.as<uint32_t>();
    p.norm = c->arena.norm.as<uint16_t>(); p.norm_cap = c->norm_cap;
    p.ch_aln = c->in.ch_aln.as<const uint32_t>(); p.ch_base = c->in.ch_base.as<const uint32_t>();
    p.n_chunks = c->n_chunks;
    p.ch_k0 = c->run.ch_k0.as<uint32_t>(); p.ch_next = c->run.ch_next.as<uint32_t>();
    p.ch_w = c->run.ch_w.as<uint32_t>(); p.ch_tb = c->run.ch_tb.as<uint32_t>();
    p.ch_flag = c->run.ch_flag.as<uint32_t>(); p.ch_src = c->run.ch_src.as<uint64_t>();
    p.ch_out = c->run.ch_out.as<uint32_t>(); p.ch_adv = c->run.ch_adv.as<uint32_t>();
    p.n_lb = c->run.n_lb.as<uint32_t>(); p.norm_tmp = c->run.norm_tmp.as<uint16_t>();
    p.tmp_main = c->tmp_main; p.tmp_cap = c->tmp_cap; p.tmp_off = c->tmp_shared ? c->in.tmp_off.as<const uint64_t>() : nullptr;
    p.ckpt = c->run.ckpt.as<uint32_t>(); p.ck_base = c->in.ck_base.as<const uint32_t>(); p.emit_shift = c->emit_shift;
    p.node_base = c->run.node_base.as<uint64_t>(); p.n_nodes = c->run.n_nodes.as<uint32_t>();
    p.pool_base = c->run.pool_base.as<uint64_t>(); p.pool_size = c->run.pool_size.as<uint32_t>();
    p.pool_top = c->run.pool_top.as<uint32_t>(); p.t_nins = c->run.t_nins.as<uint32_t>();
    p.matA = c->arena.matA.as<uint32_t>(); p.matD = c->arena.matD.as<uint32_t>(); p.matC = c->arena.matC.p;
    p.cov = c->run.cov.as<int32_t>(); p.gcount = c->run.gcount.as<uint32_t>();
    p.gbase = c->run.gbase.as<uint32_t>(); p.bid = c->run.bid.as<uint32_t>();
    p.nodes = c->arena.nodes.as<DgNode>(); p.best = c->run.best.as<int32_t>();
    p.queue = c->run.queue.as<int32_t>(); p.score = c->run.score.as<float2>(); p.bp_tt = c->run.bp_tt.as<float>();
    p.cns_tmp = c->run.cns_tmp.as<uint8_t>(); p.node_cap = c->node_cap;
    p.pool = c->arena.pool.as<uint32_t>(); p.pool_cap = c->pool_cap;
    p.stk = c->run.stk.as<int32_t>(); p.stk_words = c->stk_words; p.growth_pct = c->growth_pct;
    p.score_b = c->arena.score_b.as<float>();
    // (rows pay where there are pieces enough to fill the chip with them, eight to a wave: 64 targets x 50 kb x 60x, 16,384
    // pieces: 2.9 ms by rows against 2.3 by waves; configs[1], 147,000 pieces: 3.8 against 4.7.  DAGCON_BP_LANE=2: always)
    p.bp_lane = c->bp_lane >= 2 || (c->bp_lane && (uint64_t)c->T * c->bp_max >= 32768ull) ? 1u : 0u; p.bl_stk = c->bl_stk >= 0 && c->bl_stk < DG_BL_STK ? (uint32_t)c->bl_stk : (uint32_t)DG_BL_STK;
    p.emit_scan = c->max_k <= 64u ? 1u : 0u;
    p.fold = (c->fold && !(c->opts.flags & DAGCON_FLAG_STOP_AFTER_BUILD)) ? 1u : 0u;
    p.q_kmax = c->use_q && !c->opts.max_segments && !c->seg_env && c->max_k > DQ_KMAX ? DQ_KMAX : 0u;
    p.bp_seg_min = (c->seg_min + 2u) / 3u;
    p.seg_max = c->seg_max; p.seg_min = c->seg_min; p.cuts = c->run.cuts.as<uint32_t>(); p.bp_max = c->bp_max; p.cuts_bp = c->run.cuts_bp.as<uint32_t>(); p.bp_stat = c->run.bp_stat.as<float>(); p.bp_len = c->run.bp_len.as<uint32_t>();
    p.gcuts = c->gcuts; p.sh_log = c->sh_log;
    p.rd_s = c->run.rd.as<uint32_t>(); p.rd_e = p.rd_s + c->A; p.rd_lead = p.rd_e + c->A; p.rd_trail = p.rd_lead + c->A;
    p.pro_state = c->run.pro_state.as<uint32_t>(); p.sh_cnt = c->run.sh_cnt.as<uint32_t>();
    p.queue0 = c->run.queue0.as<int32_t>(); p.bp_end = c->run.bp_end.as<uint32_t>(); p.bp_ab = c->run.bp_ab.as<float>();
    p.defer = c->run.defer.as<uint32_t>(); p.cns_tmp0 = c->run.cns_tmp0.as<uint8_t>();
    p.seg_done = c->run.seg_done.as<uint32_t>(); p.wl_first = c->run.wl_first.as<uint32_t>();
    p.worklist = c->run.worklist.as<uint32_t>(); p.worklist_cap = c->worklist_cap;
    p.cns = c->run.cns.as<uint8_t>(); p.cns_cap = c->cns_cap;
    p.cns_off = c->sb.d<uint64_t>(c->sb.o_cns_off); p.cns_len = c->sb.d<uint32_t>(c->sb.o_cns_len);
    p.seg_first = c->sb.d<uint64_t>(c->sb.o_seg_first); p.n_seg = c->sb.d<uint32_t>(c->sb.o_n_seg);
    p.seg_r0 = c->run.seg.as<int32_t>(); p.seg_r1 = p.seg_r0 + seg_stride(c);
    p.seg_cap = c->seg_cap;
    p.st = c->sb.d<DgStatus>(0);
    if (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT) {
        p.sup_tmp = c->run.sup_tmp.as<uint32_t>(); p.sup_tmp0 = c->run.sup_tmp0.as<uint32_t>();
        p.sup_w = c->run.sup.as<uint16_t>(); p.sup_d = p.sup_w + c->cns_cap;
    }
    if (c->opts.flags & DAGCON_FLAG_BASE_POS) {
        p.pos_tmp = c->run.pos_tmp.as<uint32_t>(); p.pos_tmp0 = c->run.pos_tmp0.as<uint32_t>(); p.pos_out = c->run.pos.as<uint32_t>();
    }
    for (const GrowRef &r : c->growing())                   // ed_top / ed_cap, site_top / site_cap, sr_top / sr_cap
        if (r.on) { p.*(r.g->p_top) = c->sb.d<unsigned long long>(r.g->o_top); p.*(r.g->p_cap) = r.g->cap; }
    outputs_params(c, p);
}

// stage a1: count, chunked normalizeGaps + trimAln, and the sequential kernel for what is left
// (wide: the matC writers' 32-bit instances)
void launch_normalize(Ctx *c, const DgParams &p, const bool wide) {
    hipStream_t s = c->stream;
    if (c->A == 0) return;
    (void)hipMemsetAsync(c->run.ckpt.p, 0xFF, c->n_ckpt * 4, s);
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
        for (DevBuf *b : c->run.all())
            if (b->p && b->cap) HIPCHK(c, hipMemsetAsync(b->p, 0xEE, b->cap, s));
        // (cns_off and seg_first: the part of the status block that is not cleared below)
        if (c->sb.bytes > c->sb.zero_bytes) HIPCHK(c, hipMemsetAsync(c->sb.d<char>(c->sb.zero_bytes), 0xEE, c->sb.bytes - c->sb.zero_bytes, s));
    }
    HIPCHK(c, hipMemsetAsync(c->sb.dev.p, 0, c->sb.zero_bytes, s));      // DgStatus, tfail, cns_len, n_seg
    if (c->matc_cells) HIPCHK(c, hipMemsetAsync(c->arena.matC.p, 0, matc_bytes(c), s));
    if (c->poison) {
        // what no kernel is supposed to read before it has been written in THIS run: a process that re-uses its
        // arenas (another context's freed memory, the batch before) finds old cells there, not the zeros of a fresh one
        if ((c->poison & 1) && c->arena.matA.p) { HIPCHK(c, hipMemsetAsync(c->arena.matA.p, 0xEE, c->arena.matA.cap, s)); HIPCHK(c, hipMemsetAsync(c->arena.matD.p, 0xEE, c->arena.matD.cap, s)); }
        if ((c->poison & 2) && c->arena.nodes.p) { HIPCHK(c, hipMemsetAsync(c->arena.nodes.p, 0xEE, c->arena.nodes.cap, s)); HIPCHK(c, hipMemsetAsync(c->arena.pool.p, 0xEE, c->arena.pool.cap, s)); }
        if ((c->poison & 4) && c->arena.score_b.p) HIPCHK(c, hipMemsetAsync(c->arena.score_b.p, 0xEE, c->arena.score_b.cap, s));
        if ((c->poison & 4) && c->arena.norm.p) HIPCHK(c, hipMemsetAsync(c->arena.norm.p, 0xEE, c->arena.norm.cap, s));
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
        // targets of up to 64 reads: a lane per position, a wave's 64 rows in LDS (33,280 bytes a block at the most)
        const size_t lds_lanes = (size_t)DG_LL_WAVES * DG_WAVE * (std::min<uint32_t>(c->max_k, DG_WAVE) | 1u) * sizeof(uint32_t);
        hipLaunchKernelGGL(k_lists_lanes, dim3(c->T, (c->max_tlen + 2 + DG_LL_WAVES * DG_WAVE - 1) / (DG_LL_WAVES * DG_WAVE)),
                           dim3(DG_LL_WAVES * DG_WAVE), lds_lanes, s, p);
        if (c->max_k > DG_WAVE) {
            // (the deep targets of the batch: a wave per position)
            const size_t lds = (size_t)4 * 2 * (c->max_k + 2) * sizeof(int32_t);
            if (lds > 65536)
                HIPCHK(c, hipFuncSetAttribute((const void *)k_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_lists, dim3(c->T, rows4), dim3(256), lds, s, p);
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[2], s));
    if (c->T > 0 && !(c->opts.flags & DAGCON_FLAG_STOP_AFTER_BUILD)) {
        if (c->gcuts) {
            // partial-span cuts (k_cuts2 makes its own, bestPath's too): enter and what hangs on it first, then the
            // segments as a worklist, exit last
            HIPCHK(c, hipMemsetAsync(c->run.worklist.p, 0, 16, s));
            HIPCHK(c, hipMemsetAsync(c->run.seg_done.p, 0, (size_t)c->worklist_cap * (DG_SH_MAX + 1) * 4, s));
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
            // a row of eight lanes per piece first; the wave-per-piece sweep then takes the pieces a row gave up (deep recursion)
            if (p.bp_lane) hipLaunchKernelGGL(k_bp_sweep_l, dim3((c->T * c->bp_max + 7u) / 8u), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_sweep, dim3(c->T * c->bp_max), dim3(64), 0, s, p);
            hipLaunchKernelGGL(k_bp_check, dim3(c->T), dim3(64), 0, s, p);
            if (p.bp_lane) DG_BP_LAUNCH(k_bp_walk_r, dim3((c->T * c->bp_max + 7u) / 8u));
            else DG_BP_LAUNCH(k_bp_walk, dim3(c->T * c->bp_max));
        }
        DG_BP_LAUNCH(k_bp_join, dim3(c->T));
#undef DG_BP_LAUNCH
        if ((r = outputs_launch(c, p))) return r;
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
    if (ensure_stat(c, 0) != DAGCON_OK) { delete c; return DAGCON_ERR_WORKSPACE; }
    *out = reinterpret_cast<dagcon_ctx *>(c);
    return DAGCON_OK;
}

// ~Ctx: the device, the wait for the stream, the events and the stream; then every buffer frees itself
void dagcon_destroy(dagcon_ctx *ctx) { delete reinterpret_cast<Ctx *>(ctx); }

// whether a target string of the batch holds more than 255 gap columns in a row: the batch that follows one that needed
// 32-bit run cells (DG_E_RUN_WIDE) and is of its kind starts with them, instead of paying the same re-run at every upload.
// The raw strings decide: a run that only normalizeGaps makes that long still costs its re-run, as in any other batch
static bool has_long_gap_run(const char *tstr, const std::vector<uint64_t> &off, const std::vector<uint32_t> &len) {
    for (size_t a = 0; a < len.size(); a++) {
        const char *s = tstr + off[a];
        uint32_t run = 0;
        for (uint32_t i = 0; i < len[a]; i++) {
            run = s[i] == '-' || s[i] == '.' ? run + 1 : 0;
            if (run > 255u) return true;
        }
    }
    return false;
}

// dev_q / dev_t: the blobs are on the device already (dagcon_consensus_pre: the aligner's output), b->qstr / tstr unused
// kind: where the batch comes from, which says what it may run with (latch_outputs); dagcon_upload_haps': its alignments
// may name the same strings
static int upload_impl(dagcon_ctx *ctx, const dagcon_batch *b, const void *dev_q, const void *dev_t, const Intake kind = Intake::STRINGS) {
    if (!ctx || !b) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->drop_results(Fresh::UPLOAD);
    latch_outputs(c, kind);
    if (kind != Intake::HAPS) { c->win_first = kind == Intake::WINDOWS; c->win_n = b->n_targets; }     // (the batch a dagcon_upload_haps derives from)
    c->h_aln_src.clear();
    c->h_cig_bad.clear();
    c->rs_valid = false;
    // one batch with a very long insertion run does not slow the ones after it: the mark is dropped here, and kept below only
    // for a batch that shows such a run itself (has_long_gap_run: looked for in that state alone)
    const bool was_wide = c->wide_cells;
    c->wide_cells = false;
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
            if (c->o_sr.batch) c->h_aln_src.push_back(a);
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
    if (was_wide && !dev_t && b->tstr) c->wide_cells = has_long_gap_run(b->tstr, c->h_aln_off, c->h_aln_len);
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
    // the scratch of the chunked normalizeGaps: two columns per input column at the alignment's own offset in the blob;
    // where alignments share strings, at the columns in front of it in the batch instead
    const bool shared = kind == Intake::HAPS;
    c->tmp_shared = shared;
    uint64_t tmp_cols = b->blob_bytes;
    std::vector<uint64_t> tmp_off;
    if (shared) {
        tmp_off.resize(c->A);
        tmp_cols = 0;
        for (uint32_t a = 0; a < c->A; a++) { tmp_off[a] = tmp_cols; tmp_cols += c->h_aln_len[a]; }
    }
    c->tmp_main = dg_tmp_main(tmp_cols, c->n_chunks);
    c->tmp_cap = dg_tmp_cap(c->tmp_main);

    // inputs -> HBM
    ENSURE(c, c->in.q, b->blob_bytes);
    ENSURE(c, c->in.t, b->blob_bytes);
    if (b->blob_bytes && !(dev_q == c->in.q.p && dev_t == c->in.t.p)) {     // (dagcon_upload_cigar expands into d_q / d_t themselves)
        HIPCHK(c, hipMemcpyAsync(c->in.q.p, dev_q ? dev_q : b->qstr, b->blob_bytes, dev_q ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->in.t.p, dev_t ? dev_t : b->tstr, b->blob_bytes, dev_t ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    if (c->have_bb && (const void *)b->backbone != c->in.bb.p) {             // (dagcon_upload_haps: the backbones are there already)
        UPLOAD(c, c->in.bb, b->backbone, bb_bytes);
    }
    int r;
    UPLOAD(c, c->in.aln_off, c->h_aln_off);
    UPLOAD(c, c->in.aln_len, c->h_aln_len);
    UPLOAD(c, c->in.aln_start, c->h_aln_start);
    UPLOAD(c, c->in.aln_tgt, c->h_aln_tgt);
    UPLOAD(c, c->in.tlen, c->h_tlen);
    UPLOAD(c, c->in.aln_begin, c->h_aln_begin);
    UPLOAD(c, c->in.tactive, c->h_tactive);
    UPLOAD(c, c->in.bb_off, c->h_bb_off);
    UPLOAD(c, c->in.mat_base, c->h_mat_base);
    UPLOAD(c, c->in.matc_base, c->h_matc_base);
    UPLOAD(c, c->in.matc_stride, c->h_matc_stride);
    UPLOAD(c, c->in.bbv_base, c->h_bbv_base);
    UPLOAD(c, c->in.ch_base, c->h_ch_base);
    UPLOAD(c, c->in.ch_aln, c->h_ch_aln);
    UPLOAD(c, c->in.ck_base, c->h_ck_base);
    UPLOAD(c, c->in.norm_off, c->h_norm_off);
    if (shared) UPLOAD(c, c->in.tmp_off, tmp_off);          // (a local: upload_impl waits for the stream before it returns)
    if ((r = outputs_upload(c, b))) return r;
    ENSURE(c, c->run.ckpt, c->n_ckpt * 4);

    // work arrays whose size the host knows
    const size_t A4 = (size_t)c->A * 4, T4 = (size_t)T * 4;
    ENSURE(c, c->run.nmis, A4);
    ENSURE(c, c->run.n_lo, A4); ENSURE(c, c->run.n_hi, A4); ENSURE(c, c->run.n_start, A4);
    ENSURE(c, c->run.n_ins, A4); ENSURE(c, c->run.n_del, A4); ENSURE(c, c->run.n_lb, A4);
    {
        const size_t C4 = (size_t)c->n_chunks * 4;
        ENSURE(c, c->run.ch_k0, C4); ENSURE(c, c->run.ch_next, C4); ENSURE(c, c->run.ch_w, C4); ENSURE(c, c->run.ch_tb, C4);
        ENSURE(c, c->run.ch_flag, C4); ENSURE(c, c->run.ch_src, 2 * C4); ENSURE(c, c->run.ch_out, C4); ENSURE(c, c->run.ch_adv, C4);
        ENSURE(c, c->run.norm_tmp, c->tmp_cap * sizeof(uint16_t));
    }
    ENSURE(c, c->run.node_base, (size_t)T * 8); ENSURE(c, c->run.n_nodes, T4);
    ENSURE(c, c->run.pool_base, (size_t)T * 8); ENSURE(c, c->run.pool_size, T4); ENSURE(c, c->run.pool_top, T4);
    ENSURE(c, c->run.t_nins, T4);
    ENSURE(c, c->arena.matA, c->mat_cells * 4); ENSURE(c, c->arena.matD, c->mat_cells * 4);
    ENSURE(c, c->run.cov, c->sum_bb * 4); ENSURE(c, c->run.gcount, c->sum_bb * 4);
    ENSURE(c, c->run.gbase, c->sum_bb * 4); ENSURE(c, c->run.bid, c->sum_bb * 4);
    if ((r = ensure_stat(c, T))) return r;

    // first guesses for the data-dependent arenas; a run that finds them too
    // small records the exact need on the device and is repeated once.
    // (tests/norm_limit_cases.py, arenas_fit, restates node_cap and pool_cap to keep its batches inside them: change it
    // with them)
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

static int dump_target(Ctx *c, const char *e);      // DAGCON_DUMP (debugging aid, next to dagcon_debug_graph)

int dagcon_run(dagcon_ctx *ctx) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->uploaded) return fail(c, DAGCON_ERR_STATE, "dagcon_run before dagcon_upload");
    HIPCHK(c, hipSetDevice(c->device));
    int r = launch_all(c);
    if (r != DAGCON_OK) return r;
    c->drop_results(Fresh::RUN);
    c->ran = true;
    if (const char *e = getenv("DAGCON_DUMP")) return dump_target(c, e);
    return DAGCON_OK;
}

int dagcon_sync(dagcon_ctx *ctx) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DAGCON_OK;
}

// the stages' times of a run the stream has finished, from its events
static int read_timings(Ctx *c) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[4])); c->tm.ms_total = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->tm.ms_normalize = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[1], c->ev[2])); c->tm.ms_build = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3])); c->tm.ms_merge = ms;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[4])); c->tm.ms_bestpath = ms;
    return DAGCON_OK;
}

static int read_status(Ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, d2h(c, &c->h_st, c->sb.dev.p, sizeof(DgStatus)));
    return DAGCON_OK;
}

// ---- dagcon_fetch: status and re-runs, outcomes, sizes, the second round of copies, two unpack passes ----

// round 1, until no batch-level flag is left: the whole status block in one copy -- the status, and with it everything whose
// size the host knows; an arena that was too small is grown to what the device asked for and the batch runs again
static int fetch_status(Ctx *c) {
    const StatBlock &sb = c->sb;
    for (int attempt = 0;; attempt++) {
        HIPCHK(c, d2h(c, sb.host.p, sb.dev.p, sb.bytes));
        memcpy(&c->h_st, sb.host.p, sizeof(DgStatus));
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
        if (f & DG_E_RUN_WIDE) c->wide_cells = true;       // (until the upload of a batch without such a run)
        for (const GrowRef &r : c->growing())
            if ((f & r.g->ovf) && r.g->o_top) r.g->cap = *sb.h<uint64_t>(r.g->o_top) + 1024;
        if (f & DG_E_OUT_OVF) {
            c->cns_cap = std::max<uint64_t>(c->cns_cap, c->h_st.cns_top + 1024);
            c->seg_cap = std::max<uint64_t>(c->seg_cap, c->h_st.seg_top + 1024);
        }
        c->tm.reruns++;
        if (int r = launch_all(c)) return r;
    }
    return read_timings(c);
}

// per-target outcome (ABI 2): a failure is confined to its target.  Returns the number of failed targets
static uint32_t fetch_outcomes(Ctx *c) {
    const uint32_t T = c->T;
    const uint32_t *m_tfail = c->sb.h<uint32_t>(c->sb.o_tfail);
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
    return n_failed;
}

// the total of a growing arena in the status block's mirror; ran false: its scan did not run in this batch
static int arena_total(Ctx *c, const GrowArena &g, const bool ran, uint64_t &n) {
    n = ran && g.o_top ? *c->sb.h<uint64_t>(g.o_top) : 0;
    if (n > g.cap) return fail(c, DAGCON_ERR_INTERNAL, "%llu %s in an arena of %llu", (unsigned long long)n, g.what, (unsigned long long)g.cap);
    return DAGCON_OK;
}

// the sizes, each checked against its arena; the results of the fetch before stop being valid; room for the copies
static int fetch_plan(Ctx *c, FetchPlan &f) {
    int r;
    f.nseg = c->h_st.seg_top; f.nb = c->h_st.cns_top;
    if (2 * f.nseg * 4 > c->r_seg.cap || f.nseg > c->seg_cap) return fail(c, DAGCON_ERR_INTERNAL, "%llu segments in an arena of %llu", (unsigned long long)f.nseg, (unsigned long long)c->seg_cap);
    if ((r = c->r_blob.reserve(c, f.nb + 1))) return r;
    c->r_blob.as<char>()[f.nb] = 0;
    f.full = !(c->opts.flags & (DAGCON_FLAG_STOP_AFTER_BUILD | DAGCON_FLAG_STOP_AFTER_MERGE));
    f.want_sup = f.full && (c->opts.flags & DAGCON_FLAG_BASE_SUPPORT); f.want_pos = f.full && (c->opts.flags & DAGCON_FLAG_BASE_POS);
    if ((r = outputs_plan(c, f))) return r;
    // edits on: the edits come instead of the positions, which stay on the device for dagcon_fetch_positions to ask for; so
    // they do where the kept parts are in effect (dagcon_set_window_keep): 16 bytes a segment stand in for 4 a base
    f.lazy_pos = f.want_pos && (f.want_ed || c->o_keep.batch);
    c->drop_results(Fresh::FETCH);
    c->r_nb = f.nb;
    if (f.want_sup && (r = c->r_sup.reserve(c, 2 * (size_t)(f.nb + 1) * 2))) return r;     // (two halves of nb + 1 entries)
    if (f.want_pos && !f.lazy_pos) c->r_pos.resize(f.nb + 1);
    return DAGCON_OK;
}

// round 2: what the status sizes -- the segments' ranges (the first seg_top entries of either array), the blob, the
// support (weights then depths: the device keeps them apart, no host pass over them), the positions, and what the optional
// outputs bring (the edit records, the sites) -- enqueued together, one wait
static int fetch_copies(Ctx *c, const FetchPlan &f) {
    const uint32_t T = c->T;
    const uint64_t nseg = f.nseg, nb = f.nb;
    int32_t *m_r0 = c->r_seg.as<int32_t>(), *m_r1 = m_r0 + nseg;
    uint16_t *const m_sup = c->r_sup.as<uint16_t>();
    bool queued = false;
    if (T && f.full && nseg) {
        HIPCHK(c, hipMemcpyAsync(m_r0, c->run.seg.p, nseg * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(m_r1, c->run.seg.as<const int32_t>() + seg_stride(c), nseg * 4, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (T && f.full && nb) { HIPCHK(c, hipMemcpyAsync(c->r_blob.p, c->run.cns.p, nb, hipMemcpyDeviceToHost, c->stream)); queued = true; }
    if (f.want_sup && nb) {
        HIPCHK(c, hipMemcpyAsync(m_sup, c->run.sup.p, nb * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(m_sup + nb, c->run.sup.as<const uint16_t>() + c->cns_cap, nb * 2, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (f.want_pos && !f.lazy_pos && nb) { HIPCHK(c, hipMemcpyAsync(c->r_pos.data(), c->run.pos.p, nb * 4, hipMemcpyDeviceToHost, c->stream)); queued = true; }
    if (int r = outputs_copies(c, f, queued)) return r;
    if (queued) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (f.want_sup) { c->r_sup_n = nb; c->sup_valid = true; }
    if (f.want_pos && !f.lazy_pos) c->pos_valid = true;
    c->pos_pending = f.lazy_pos;
    return DAGCON_OK;
}

// the segments of every target that came through, in the host's order.  bases: the consensus bases of the batch
static void unpack_segments(Ctx *c, const FetchPlan &f, uint64_t &bases) {
    const StatBlock &sb = c->sb;
    const uint32_t T = c->T;
    const uint32_t *m_tfail = sb.h<uint32_t>(sb.o_tfail), *m_n_seg = sb.h<uint32_t>(sb.o_n_seg);
    const uint64_t *m_cns_off = sb.h<uint64_t>(sb.o_cns_off), *m_seg_first = sb.h<uint64_t>(sb.o_seg_first);
    const int32_t *m_r0 = c->r_seg.as<int32_t>(), *m_r1 = m_r0 + f.nseg;
    c->r_seg_begin.assign(T + 1, 0);
    c->r_range0.clear(); c->r_range1.clear(); c->r_seq_off.clear(); c->r_seq_len.clear();
    bases = 0;
    for (uint32_t t = 0; t < T; t++) {
        c->r_seg_begin[t] = c->r_range0.size();
        if (!f.full || !c->h_tactive[t] || m_tfail[t]) continue;
        for (uint32_t i = 0; i < m_n_seg[t]; i++) {
            const uint64_t s = m_seg_first[t] + i;
            const int32_t r0 = m_r0[s], r1 = m_r1[s];
            c->r_range0.push_back(r0); c->r_range1.push_back(r1);
            c->r_seq_off.push_back(m_cns_off[t] + (uint64_t)r0);
            c->r_seq_len.push_back((uint32_t)(r1 - r0));
            bases += (uint64_t)(r1 - r0);
        }
    }
    c->r_seg_begin[T] = c->r_range0.size();
}

int dagcon_fetch(dagcon_ctx *ctx, dagcon_results *res) {
    if (!ctx || !res) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->ran) return fail(c, DAGCON_ERR_STATE, "dagcon_fetch before dagcon_run");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = fetch_status(c))) return r;
    const uint32_t n_failed = fetch_outcomes(c);
    FetchPlan f;
    uint64_t bases = 0;
    if ((r = fetch_plan(c, f))) return r;
    if ((r = fetch_copies(c, f))) return r;
    unpack_segments(c, f, bases);
    if ((r = outputs_unpack(c, f))) return r;
    c->tm.consensus_bases = bases;
    c->tm.algorithmic_bytes = 2ull * c->sum_len + bases;
    c->tm.n_alignments = c->A;
    c->tm.n_columns = c->h_st.n_columns;
    c->tm.n_nodes = c->h_st.node_need;
    c->tm.merge_segments = c->h_st.n_mseg;
    res->n_targets = c->T;
    res->n_segments = c->r_range0.size();
    res->seg_begin = c->r_seg_begin.data();
    res->range0 = c->r_range0.data(); res->range1 = c->r_range1.data();
    res->seq_off = c->r_seq_off.data(); res->seq_len = c->r_seq_len.data();
    res->seq_blob = c->r_blob.as<char>(); res->seq_bytes = f.nb;
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
    out->weight = c->r_sup.as<uint16_t>();
    out->depth = out->weight + c->r_sup_n;
    return DAGCON_OK;
}

int dagcon_fetch_positions(dagcon_ctx *ctx, const uint32_t **pos, uint64_t *n) {
    if (!ctx || !pos || !n) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_POS))
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_positions on a context created without DAGCON_FLAG_BASE_POS");
    if (c->pos_pending) {
        // edits or the kept parts on: the copy dagcon_fetch left out; the kind bit the edit kernels read stays on the device
        HIPCHK(c, hipSetDevice(c->device));
        c->r_pos.resize(c->r_nb + 1);
        if (c->r_nb) HIPCHK(c, d2h(c, c->r_pos.data(), c->run.pos.p, c->r_nb * 4));
        for (uint64_t i = 0; i < c->r_nb; i++) c->r_pos[i] &= ~DG_POS_BB;
        c->pos_pending = false; c->pos_valid = true;
    }
    if (!c->pos_valid)
        return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_positions without the results of a consensus (no fetch yet, or stopped before bestPath)");
    *pos = c->r_pos.data();
    *n = c->r_pos.size() - 1;
    return DAGCON_OK;
}

// kept for ABI 2: no build fills the counters any more, sixteen zeros
int dagcon_debug_counters(dagcon_ctx *ctx, unsigned long long *out8) {
    if (!ctx || !out8) return DAGCON_ERR_INVALID_ARG;
    for (int i = 0; i < 16; i++) out8[i] = 0;
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
        if (int r = read_timings(c)) return r;
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
        HIPCHK(c, d2h(c, noff.data(), c->in.norm_off.p, (size_t)n * 8));
        HIPCHK(c, d2h(c, lo.data(), c->run.n_lo.p, (size_t)n * 4));
        HIPCHK(c, d2h(c, hi.data(), c->run.n_hi.p, (size_t)n * 4));
        HIPCHK(c, d2h(c, st.data(), c->run.n_start.p, (size_t)n * 4));
    }
    std::vector<uint16_t> cols;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t m = hi[a] - lo[a];
        cols.resize(m);
        if (m) HIPCHK(c, d2h(c, cols.data(), c->arena.norm.as<const uint16_t>() + noff[a] + lo[a], (size_t)m * 2));
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
}  // extern "C"
