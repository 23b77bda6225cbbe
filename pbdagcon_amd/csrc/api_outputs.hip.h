// api_outputs.hip.h -- the optional outputs of a run (edits and their support, the pile-up and its sites, the reads at the
// sites, the window phase, the alleles, the joined sites, the haplotype tally, the hap calls, the kept parts, the site link), each one's host side in one place: its room, its kernel
// parameters, its launches, its part of the fetch and its dagcon_set_* / dagcon_fetch_* entry points.  The pipeline
// (api_run.hip.h) calls outputs_room, outputs_params, outputs_launch, outputs_upload and the outputs_plan / _copies /
// _unpack steps of dagcon_fetch, at the end of this file; DESIGN.md says how to add an output.  (The entry points stand
// outside the namespace, next to their output: their linkage is that of their declarations in include/dagcon.h.)
// (one translation unit with dagcon_api.hip, which includes it once).
namespace {

// ---- what the outputs share: the dependency rule, "did the kernels run", the fetches' precondition, the host's order ----

// The dependency rule, once: which outputs the batch being uploaded runs with, and with which options (defaults filled
// in).  Edits need a record upload and their support needs edits; the sites need the pile-up; the reads at the sites need
// the sites; the alleles, the tally, the site link and the window phase need those reads, the last three with phase on; the window phase
// needs a windows upload; the joined sites need the alleles.  The batch of dagcon_upload_haps runs with none, whatever the
// switches say (but for the kept parts, which need a windows upload or the batch derived from one and nothing else) --
// unless dagcon_set_hap_calls is on and the batch it derives from ran with the edits latched (a record
// upload, then: cg.t still holds its targets): then it runs with the edits, with their support iff that batch did, and
// with the pairing of the two groups' edits.
void latch_outputs(Ctx *c, const Intake kind) {
    const bool had_ed = c->o_ed.batch, had_evid = c->o_evid.batch;
    for (Output *o : c->outputs()) o->batch = false;
    if (kind == Intake::HAPS) {
        c->o_hc.batch = c->o_hc.on && c->o_ed.on && had_ed;
        c->o_ed.batch = c->o_hc.batch;
        c->o_evid.batch = c->o_hc.batch && had_evid;
        c->o_keep.batch = c->o_keep.on && c->win_first;
        return;
    }
    c->o_ed.batch = c->o_ed.on && kind != Intake::STRINGS;
    c->o_evid.batch = c->o_evid.on && c->o_ed.batch;
    c->o_pile.batch = c->o_pile.on;
    c->o_sr.batch = c->o_sr.on && c->o_pile.batch;
    const bool phased = c->o_sr.batch && c->sr_opts.phase != 0;
    c->o_al.batch = c->o_al.on && c->o_sr.batch;
    c->o_jn.batch = c->o_jn.on && c->o_al.batch;
    c->o_hap.batch = c->o_hap.on && phased;
    c->o_wl.batch = c->o_wl.on && phased && kind == Intake::WINDOWS;
    c->o_keep.batch = c->o_keep.on && kind == Intake::WINDOWS;
    c->pile_batch_opts = c->pile_opts;
    c->sr_batch_opts = c->sr_opts;
    c->hap_batch_opts = {c->hap_opts.min_sites ? c->hap_opts.min_sites : 2u, c->hap_opts.min_reads ? c->hap_opts.min_reads : 3u};
    c->wl_batch_opts = {c->wl_opts.min_links ? c->wl_opts.min_links : 3u, c->wl_opts.max_conflict_ppm ? c->wl_opts.max_conflict_ppm : 250000u};
    c->o_lk.batch = c->o_lk.on && phased;
    const dagcon_site_link_opts &lk = c->lk_opts;
    c->lk_batch_opts = {lk.max_conflict_ppm ? lk.max_conflict_ppm : 100000u, lk.min_cell ? lk.min_cell : 3u, lk.min_partners ? lk.min_partners : 2u, lk.reach ? lk.reach : 256u};
}

// Whether the kernels behind the consensus ran in this batch: the launches below and every fetch ask here.  The sites'
// kernels need a target position to work on; the kernels with a wave or a thread per alignment need an alignment too
// (without one k_sr_mark and k_sr_scan still run)
bool sites_ran(const Ctx *c) { return c->o_pile.batch && c->T && c->h_pile_begin.back(); }
bool reads_ran(const Ctx *c) { return sites_ran(c) && c->A; }

// The precondition of every fetch: the last dagcon_fetch brought this output's results.  (latch_outputs latches an output
// only together with everything it rests on, and outputs_unpack marks what was latched: one record answers.)
int need(Ctx *c, const Output &o, const char *who, const bool also = true) {
    return o.valid && also ? DAGCON_OK : fail(c, DAGCON_ERR_STATE, "%s %s", who, o.missing);
}

// one entry more than an array holds, so that data() of an empty one is no NULL
template <class... V> void pad(V &...v) { (v.emplace_back(), ...); }

// a per-site array of the device (`per` values a site) in the host's order of the sites: a failed target's sites go
template <typename X>
void gather_sites(const Ctx *c, const X *dev, X *host, const size_t per = 1) {
    const SitesOut &s = c->r_sites;
    for (uint32_t t = 0; t < c->T; t++) {
        const uint64_t n = s.begin[t + 1] - s.begin[t];
        if (c->r_status[t] == DAGCON_OK && n) memcpy(host + s.begin[t] * per, dev + s.dev_begin[t] * per, (size_t)n * per * sizeof(X));
    }
}

// The alignments in the host's terms, once per fetched run: those of a failed target and the ones the graph did not take
// go; each of the others keeps its index on the device and its stretch of the device's entry arrays
int host_order(Ctx *c) {
    HostOrder &h = c->order;
    if (h.built) return DAGCON_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t A = c->A;
    const uint64_t ne = c->r_reads.n_dev_ent;
    std::vector<uint32_t> cnt((size_t)A, 0);
    if (reads_ran(c)) HIPCHK(c, d2h(c, cnt.data(), c->run.sr_cnt.p, (size_t)A * 4));
    h.aln.clear(); h.ent_begin.clear(); h.ent_n.clear();
    uint64_t e = 0;
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t n = cnt[a] & ~DG_SR_TAKEN;
        const uint64_t e0 = e;
        e += n;
        if (e > ne) return fail(c, DAGCON_ERR_INTERNAL, "k_sr_walk: the alignments hold more than the %llu entries of the batch (alignment %u)", (unsigned long long)ne, a);
        if (c->r_status[c->h_aln_tgt[a]] != DAGCON_OK || !(cnt[a] & DG_SR_TAKEN)) continue;
        h.aln.push_back(a); h.ent_begin.push_back(e0); h.ent_n.push_back(n);
    }
    if (e != ne) return fail(c, DAGCON_ERR_INTERNAL, "k_sr_walk: the alignments hold %llu entries, the batch %llu", (unsigned long long)e, (unsigned long long)ne);
    h.built = true;
    return DAGCON_OK;
}

}  // namespace

// ---- edits and their read support (k_edits.hip.h, k_evidence.hip.h) ----
namespace {

int edits_room(Ctx *c) {
    if (!c->o_ed.batch) return DAGCON_OK;
    ENSURE(c, c->run.ed_seg, c->seg_cap * sizeof(DgEdSeg));
    ENSURE(c, c->run.ed_out, c->ed_arena.cap * sizeof(DgEdit));
    if (c->o_evid.batch) ENSURE(c, c->run.evid, c->ed_arena.cap * sizeof(DgEvid));
    return DAGCON_OK;
}

void edits_params(Ctx *c, DgParams &p) {
    if (!c->o_ed.batch) return;
    p.ed_seg = c->run.ed_seg.as<DgEdSeg>(); p.ed_out = c->run.ed_out.as<DgEdit>();
    p.ed_t = c->cg.t.as<const uint8_t>(); p.ed_tbase = c->in.ed_tbase.as<const uint64_t>();
    if (c->o_evid.batch) p.evid = c->run.evid.as<DgEvid>();
}

void edits_launch(Ctx *c, const DgParams &p) {
    if (!c->o_ed.batch) return;
    hipStream_t s = c->stream;
    // the edits (k_edits.hip.h): count, place, write; a wave per segment of the arena (seg_top is the device's)
    const dim3 eg((uint32_t)((c->seg_cap + 3) / 4));
    hipLaunchKernelGGL(k_ed_scan_seg<false>, eg, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_ed_scan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_ed_scan_seg<true>, eg, dim3(256), 0, s, p);
    if (c->o_evid.batch) {
        // read support per edit (k_evidence.hip.h): windows and groups per segment, a wave per alignment, the copy
        hipLaunchKernelGGL(k_ev_windows, eg, dim3(256), 0, s, p);
        if (c->A > 0) hipLaunchKernelGGL(k_ev_count, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
        hipLaunchKernelGGL(k_ev_spread, eg, dim3(256), 0, s, p);
    }
}

// each segment's edit record, its edits and their support, from the device's order into the host's: the segments of
// every target that came through, as unpack_segments lists them
int edits_unpack(Ctx *c, const FetchPlan &f) {
    if (!f.want_ed) return DAGCON_OK;
    const StatBlock &sb = c->sb;
    const uint32_t *m_tfail = sb.h<uint32_t>(sb.o_tfail), *m_n_seg = sb.h<uint32_t>(sb.o_n_seg);
    const uint64_t *m_seg_first = sb.h<uint64_t>(sb.o_seg_first);
    const char *const m_edb = c->r_ed.as<char>();
    const DgEdSeg *m_es = reinterpret_cast<const DgEdSeg *>(m_edb);
    const DgEdit *m_ed = reinterpret_cast<const DgEdit *>(m_edb + f.ed_seg_bytes);
    const DgEvid *m_evid = reinterpret_cast<const DgEvid *>(m_edb + f.ed_bytes);
    EditsOut &o = c->r_edits;
    o = EditsOut();
    const bool calls = c->o_hc.batch;                 // dagcon_fetch_hap_calls brings its arrays into this order
    o.n_dev = f.n_ed;
    for (uint32_t t = 0; t < c->T; t++) {
        if (calls) o.tgt_begin.push_back(o.tpos.size());
        if (!c->h_tactive[t] || m_tfail[t]) continue;
        for (uint32_t i = 0; i < m_n_seg[t]; i++) {
            const uint64_t s = m_seg_first[t] + i;
            const DgEdSeg &es = m_es[s];
            if (es.tgt != t || es.off > f.n_ed || es.cnt > f.n_ed - es.off)
                return fail(c, DAGCON_ERR_INTERNAL, "k_ed_scan: segment %llu of target %u has edits [%llu, + %u) of %llu, target %u",
                            (unsigned long long)s, t, (unsigned long long)es.off, es.cnt, (unsigned long long)f.n_ed, es.tgt);
            o.t0.push_back(es.t0); o.t1.push_back(es.t1); o.begin.push_back(o.tpos.size());
            for (uint32_t k = 0; k < es.cnt; k++) {
                const DgEdit &e = m_ed[es.off + k];
                o.tpos.push_back(e.t_pos); o.tlen.push_back(e.t_len); o.coff.push_back(e.c_off); o.clen.push_back(e.c_len);
                if (calls) o.dev_idx.push_back(es.off + k);
                if (f.want_evid) {
                    const DgEvid &v = m_evid[es.off + k];
                    o.w_begin.push_back(v.gL); o.w_end.push_back(v.gR);
                    o.span.push_back(v.span); o.alt.push_back(v.alt); o.ref.push_back(v.ref);
                }
            }
        }
    }
    o.begin.push_back(o.tpos.size());
    if (calls) o.tgt_begin.push_back(o.tpos.size());
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_edits(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_POS))
        return fail(c, DAGCON_ERR_STATE, "dagcon_set_edits on a context created without DAGCON_FLAG_BASE_POS");
    c->o_ed.on = on != 0;
    if (!c->o_ed.on) c->o_evid.on = c->o_hc.on = false;
    return DAGCON_OK;
}

int dagcon_fetch_edits(dagcon_ctx *ctx, dagcon_edits *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_ed, "dagcon_fetch_edits", c->o_ed.on)) return r;
    const EditsOut &o = c->r_edits;
    out->n_segments = o.t0.size(); out->n = o.tpos.size();
    out->seg_t0 = o.t0.data(); out->seg_t1 = o.t1.data(); out->edit_begin = o.begin.data();
    out->t_pos = o.tpos.data(); out->t_len = o.tlen.data(); out->c_off = o.coff.data(); out->c_len = o.clen.data();
    return DAGCON_OK;
}

int dagcon_set_edit_support(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->o_ed.on) return fail(c, DAGCON_ERR_STATE, "dagcon_set_edit_support without dagcon_set_edits on");
    c->o_evid.on = on != 0;
    return DAGCON_OK;
}

int dagcon_fetch_edit_support(dagcon_ctx *ctx, dagcon_edit_support *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_evid, "dagcon_fetch_edit_support", c->o_ed.on)) return r;
    const EditsOut &o = c->r_edits;
    out->n = o.w_begin.size();
    out->w_begin = o.w_begin.data(); out->w_end = o.w_end.data();
    out->span = o.span.data(); out->alt = o.alt.data(); out->ref = o.ref.data();
    return DAGCON_OK;
}

// ---- the pile-up and its sites (k_pileup.hip.h) ----
namespace {

int pile_room(Ctx *c) {
    if (!c->o_pile.batch) return DAGCON_OK;
    const uint64_t pn = c->h_pile_begin.back();
    ENSURE(c, c->run.pile, pn * 16);
    ENSURE(c, c->run.pile_tile, (pn + DG_PILE_TILE - 1) / DG_PILE_TILE * 8);
    ENSURE(c, c->run.pile_site, c->site_arena.cap * sizeof(DgSite));
    return DAGCON_OK;
}

void pile_params(Ctx *c, DgParams &p) {
    if (!c->o_pile.batch) return;
    p.pile = c->run.pile.as<uint32_t>(); p.pile_begin = c->in.pile_begin.as<const uint64_t>(); p.pile_n = c->h_pile_begin.back();
    p.pile_tile = c->run.pile_tile.as<unsigned long long>();
    p.pile_site = c->run.pile_site.as<DgSite>();
    p.pile_min_count = c->pile_batch_opts.min_count; p.pile_min_ppm = c->pile_batch_opts.min_frac_ppm;
}

int pile_launch(Ctx *c, const DgParams &p) {
    if (!sites_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    // the counters start from zero in every execution, a re-run included; a wave per alignment; then the sites: mark and
    // count per tile, one scan, write
    HIPCHK(c, hipMemsetAsync(c->run.pile.p, 0, p.pile_n * 16, s));
    if (reads_ran(c)) hipLaunchKernelGGL(k_pile_count, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
    const dim3 tg((uint32_t)((p.pile_n + DG_PILE_TILE - 1) / DG_PILE_TILE));
    hipLaunchKernelGGL(k_pile_sites<false>, tg, dim3(DG_PILE_TILE), 0, s, p);
    hipLaunchKernelGGL(k_pile_scan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_pile_sites<true>, tg, dim3(DG_PILE_TILE), 0, s, p);
    return DAGCON_OK;
}

// The device lists the sites in the order of the positions: a target's are one stretch, the targets ascend.  A target the
// host reports as failed has none (one that failed on the device has none there either); dev_begin keeps where each
// target's begin in the device's list
int pile_unpack(Ctx *c, const FetchPlan &f) {
    if (!f.want_pile) return DAGCON_OK;
    const uint32_t T = c->T;
    const uint64_t n_site = f.n_site;
    const DgSite *m_site = c->r_site.as<const DgSite>();
    SitesOut &o = c->r_sites;
    o.begin.assign((size_t)T + 1, 0); o.dev_begin.assign((size_t)T + 1, n_site); o.pos.clear(); o.counts.clear();
    uint64_t k = 0;
    for (uint32_t t = 0; t < T; t++) {
        o.begin[t] = o.pos.size();
        o.dev_begin[t] = k;
        for (; k < n_site && m_site[k].tgt == t; k++) {
            const DgSite &x = m_site[k];
            if (x.pos >= c->h_tlen[t]) return fail(c, DAGCON_ERR_INTERNAL, "k_pile_sites: site %llu of target %u at position %u of %u", (unsigned long long)k, t, x.pos, c->h_tlen[t]);
            if (c->r_status[t] != DAGCON_OK) continue;
            o.pos.push_back(x.pos);
            for (int j = 0; j < 4; j++) { o.counts.push_back((uint16_t)(x.w[j] & 0xFFFFu)); o.counts.push_back((uint16_t)(x.w[j] >> 16)); }
        }
    }
    if (k != n_site) return fail(c, DAGCON_ERR_INTERNAL, "k_pile_sites: site %llu of %llu is out of order (target %u)", (unsigned long long)k, (unsigned long long)n_site, m_site[k].tgt);
    o.begin[T] = o.pos.size();
    o.n_dev = n_site;
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_pileup(dagcon_ctx *ctx, const dagcon_pileup_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!o) { c->o_pile.on = false; return DAGCON_OK; }
    if (o->min_frac_ppm > 1000000u) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_pileup: min_frac_ppm %u is more than 1000000", o->min_frac_ppm);
    c->pile_opts = *o;
    c->o_pile.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_pileup_sites(dagcon_ctx *ctx, dagcon_pileup_sites *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_pile, "dagcon_fetch_pileup_sites")) return r;
    out->n_targets = c->T;
    out->site_begin = c->r_sites.begin.data(); out->pos = c->r_sites.pos.data(); out->counts = c->r_sites.counts.data();
    return DAGCON_OK;
}

int dagcon_fetch_pileup(dagcon_ctx *ctx, dagcon_pileup *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_pile, "dagcon_fetch_pileup")) return r;
    if (!c->o_pile.fetched) {
        // the copy dagcon_fetch left out: 16 bytes a position, only when asked for
        HIPCHK(c, hipSetDevice(c->device));
        const uint64_t pn = c->h_pile_begin.back();
        if (int r = c->r_pile.reserve(c, (size_t)pn * 16 + 16)) return r;
        if (pn) HIPCHK(c, d2h(c, c->r_pile.p, c->run.pile.p, (size_t)pn * 16));
        // a failed target: all zero, whatever was counted before it failed
        for (uint32_t t = 0; t < c->T; t++)
            if (c->r_status[t] != DAGCON_OK) memset(c->r_pile.as<char>() + 16 * c->h_pile_begin[t], 0, (size_t)16 * c->h_tlen[t]);
        c->o_pile.fetched = true;
    }
    out->n_targets = c->T;
    out->pos_begin = c->h_pile_begin.data(); out->counts = c->r_pile.as<uint16_t>();
    return DAGCON_OK;
}

// ---- the sites the same reads carry (k_site_link.hip.h): latched only with the split, whose launches it sits between ----
namespace {

int link_room(Ctx *c) {
    if (!c->o_lk.batch) return DAGCON_OK;
    const uint64_t words = (c->max_k + 63u) / 64u;
    ENSURE(c, c->run.lk_rows, c->site_arena.cap * 2 * words * 8); ENSURE(c, c->run.lk_partners, c->site_arena.cap * 2); ENSURE(c, c->run.lk_linked, c->site_arena.cap);
    return DAGCON_OK;
}

void link_params(Ctx *c, DgParams &p) {
    if (!c->o_lk.batch) return;
    p.lk_words = (c->max_k + 63u) / 64u; p.lk_row_cap = c->site_arena.cap * 2 * p.lk_words;
    p.lk_rows = c->run.lk_rows.as<unsigned long long>(); p.lk_partners = c->run.lk_partners.as<uint16_t>(); p.lk_linked = c->run.lk_linked.as<uint8_t>();
    p.lk_ppm = c->lk_batch_opts.max_conflict_ppm; p.lk_min_cell = c->lk_batch_opts.min_cell;
    p.lk_min_partners = c->lk_batch_opts.min_partners; p.lk_reach = c->lk_batch_opts.reach;
}

// between k_sr_walk<true> and k_sr_split (reads_launch calls it there): the sites' kinds, the bit rows, the pairs.  The
// rows start from zero in every execution, a re-run included; partners and linked are written for every site
int link_launch(Ctx *c, const DgParams &p) {
    if (!c->o_lk.batch || !reads_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->run.lk_rows.p, 0, p.lk_row_cap * 8, s));
    hipLaunchKernelGGL(k_lk_kind, dim3((uint32_t)((p.site_cap + 255) / 256)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_lk_bits, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_lk_pairs, dim3((uint32_t)((p.site_cap + 3) / 4)), dim3(256), 0, s, p);
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_site_link(dagcon_ctx *ctx, const dagcon_site_link_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!o) { c->o_lk.on = false; return DAGCON_OK; }
    if (o->reach > DG_LK_MAX_REACH) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_site_link: a reach of %u is more than %u", o->reach, DG_LK_MAX_REACH);
    c->lk_opts = *o;
    c->o_lk.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_site_link(dagcon_ctx *ctx, dagcon_site_link *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_lk, "dagcon_fetch_site_link")) return r;
    SiteLinkOut &o = c->r_link;
    if (!c->o_lk.fetched) {
        // the copies dagcon_fetch left out, 3 bytes a site, into the host's order of the sites: a failed target's go
        HIPCHK(c, hipSetDevice(c->device));
        const SitesOut &s = c->r_sites;
        const uint64_t ns = s.n_dev;
        std::vector<uint16_t> partners((size_t)ns + 1, 0);
        std::vector<uint8_t> linked((size_t)ns + 1, 0);
        if (ns && reads_ran(c)) { HIPCHK(c, d2h(c, partners.data(), c->run.lk_partners.p, (size_t)ns * 2)); HIPCHK(c, d2h(c, linked.data(), c->run.lk_linked.p, (size_t)ns)); }
        o.partners.assign(s.pos.size() + 1, 0); o.linked.assign(s.pos.size() + 1, 0);
        gather_sites(c, partners.data(), o.partners.data());
        gather_sites(c, linked.data(), o.linked.data());
        for (size_t k = 0; k < s.pos.size(); k++)
            if (o.linked[k] > 1u || o.partners[k] > 2u * DG_LK_MAX_REACH || (o.linked[k] != 0) != (o.partners[k] >= c->lk_batch_opts.min_partners))
                return fail(c, DAGCON_ERR_INTERNAL, "k_lk_pairs: site %zu has %u partners and linked %u", k, o.partners[k], o.linked[k]);
        c->o_lk.fetched = true;
    }
    out->n_sites = c->r_sites.pos.size();
    out->partners = o.partners.data(); out->linked = o.linked.data();
    return DAGCON_OK;
}

// ---- the reads at the sites and the split (k_site_reads.hip.h) ----
namespace {

int reads_room(Ctx *c) {
    if (!c->o_sr.batch) return DAGCON_OK;
    const uint64_t words = (c->h_pile_begin.back() + 63) / 64;
    const size_t A4 = (size_t)c->A * 4;
    ENSURE(c, c->run.sr_bits, words * 8); ENSURE(c, c->run.sr_rank, words * 4);
    ENSURE(c, c->run.sr_cnt, A4); ENSURE(c, c->run.sr_off, 2 * A4);
    ENSURE(c, c->run.sr_site, c->sr_arena.cap * 4); ENSURE(c, c->run.sr_code, c->sr_arena.cap);
    if (c->sr_batch_opts.phase) {
        ENSURE(c, c->run.sr_hap, (size_t)c->A); ENSURE(c, c->run.sr_nz, A4);
        ENSURE(c, c->run.sr_sigma, c->site_arena.cap); ENSURE(c, c->run.sr_kind, c->site_arena.cap); ENSURE(c, c->run.sr_acc, c->site_arena.cap * 4);
    }
    return DAGCON_OK;
}

void reads_params(Ctx *c, DgParams &p) {
    if (!c->o_sr.batch) return;
    p.sr_bits = c->run.sr_bits.as<unsigned long long>(); p.sr_rank = c->run.sr_rank.as<uint32_t>();
    p.sr_cnt = c->run.sr_cnt.as<uint32_t>(); p.sr_off = c->run.sr_off.as<unsigned long long>();
    p.sr_site = c->run.sr_site.as<uint32_t>(); p.sr_code = c->run.sr_code.as<uint8_t>();
    p.sr_phase = c->sr_batch_opts.phase; p.sr_rounds = c->sr_batch_opts.rounds ? c->sr_batch_opts.rounds : 8u;
    if (p.sr_phase) {
        p.sr_hap = c->run.sr_hap.as<uint8_t>(); p.sr_nz = c->run.sr_nz.as<uint32_t>();
        p.sr_sigma = c->run.sr_sigma.as<int8_t>(); p.sr_kind = c->run.sr_kind.as<uint8_t>(); p.sr_acc = c->run.sr_acc.as<int>();
    }
}

int reads_launch(Ctx *c, const DgParams &p) {
    if (!c->o_sr.batch || !sites_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    const bool reads = reads_ran(c);
    // a bit per site position, count, scan, write; then the split
    HIPCHK(c, hipMemsetAsync(c->run.sr_bits.p, 0, (p.pile_n + 63) / 64 * 8, s));
    hipLaunchKernelGGL(k_sr_mark, dim3((uint32_t)((p.site_cap + 255) / 256)), dim3(256), 0, s, p);
    if (reads) hipLaunchKernelGGL(k_sr_walk<false>, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_sr_scan, dim3(1), dim3(1024), 0, s, p);
    if (reads) hipLaunchKernelGGL(k_sr_walk<true>, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
    if (int r = link_launch(c, p)) return r;
    if (p.sr_phase && reads) hipLaunchKernelGGL(k_sr_split, dim3(c->T), dim3(256), 0, s, p);
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_site_reads(dagcon_ctx *ctx, const dagcon_site_reads_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!o) { c->o_sr.on = false; return DAGCON_OK; }
    if (o->rounds > 64u) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_site_reads: %u rounds are more than 64", o->rounds);
    c->sr_opts = *o;
    c->o_sr.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_site_reads(dagcon_ctx *ctx, dagcon_site_reads *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_sr, "dagcon_fetch_site_reads")) return r;
    const bool phase = c->sr_batch_opts.phase != 0;
    SiteReadsOut &o = c->r_reads;
    if (!c->o_sr.fetched) {
        // the copies dagcon_fetch left out, and the device's arrays in the host's terms: the alignments go into the host's
        // order (host_order), a site's index becomes the one dagcon_fetch_pileup_sites lists it under
        if (int r = host_order(c)) return r;
        const HostOrder &h = c->order;
        const SitesOut &s = c->r_sites;
        const uint64_t ne = o.n_dev_ent, ns = s.n_dev;
        std::vector<uint32_t> site((size_t)ne);
        std::vector<uint8_t> code((size_t)ne), hap((size_t)c->A, 0);
        std::vector<int8_t> sigma((size_t)ns, 0);
        if (ne) { HIPCHK(c, d2h(c, site.data(), c->run.sr_site.p, (size_t)ne * 4)); HIPCHK(c, d2h(c, code.data(), c->run.sr_code.p, (size_t)ne)); }
        if (phase && reads_ran(c)) HIPCHK(c, d2h(c, hap.data(), c->run.sr_hap.p, (size_t)c->A));
        if (phase && ns) HIPCHK(c, d2h(c, sigma.data(), c->run.sr_sigma.p, (size_t)ns));
        o.tgt.clear(); o.src.clear(); o.begin.assign(1, 0); o.site.clear(); o.code.clear(); o.hap.clear();
        for (size_t x = 0; x < h.aln.size(); x++) {
            const uint32_t a = h.aln[x], t = c->h_aln_tgt[a];
            const uint64_t e0 = h.ent_begin[x], d0 = s.dev_begin[t], d1 = s.dev_begin[t + 1];
            for (uint64_t j = e0; j < e0 + h.ent_n[x]; j++) {
                if (site[j] < d0 || site[j] >= d1 || (code[j] & 7u) > 5u || (code[j] >> 4))
                    return fail(c, DAGCON_ERR_INTERNAL, "k_sr_walk: entry %llu of alignment %u: site %u, code %u (target %u has sites [%llu, %llu))", (unsigned long long)(j - e0), a,
                                site[j], code[j], t, (unsigned long long)d0, (unsigned long long)d1);
                o.site.push_back(site[j] - d0 + s.begin[t]);
                o.code.push_back(code[j]);
            }
            o.tgt.push_back(t); o.src.push_back(c->h_aln_src[a]); o.begin.push_back(o.site.size());
            if (hap[a] > 2u) return fail(c, DAGCON_ERR_INTERNAL, "k_sr_split: alignment %u has hap %u", a, hap[a]);
            o.hap.push_back(hap[a]);
        }
        o.phase.assign(s.pos.size() + 1, 0);
        if (phase) gather_sites(c, sigma.data(), o.phase.data());
        pad(o.site, o.code, o.tgt, o.src, o.hap);
        c->o_sr.fetched = true;
    }
    out->n_aln = o.begin.size() - 1;
    out->aln_tgt = o.tgt.data(); out->aln_src = o.src.data(); out->ent_begin = o.begin.data();
    out->ent_site = o.site.data(); out->ent_code = o.code.data();
    out->hap = phase ? o.hap.data() : nullptr; out->phase = phase ? o.phase.data() : nullptr;
    return DAGCON_OK;
}

// ---- the window phase (k_winlink.hip.h) ----
namespace {

int winphase_room(Ctx *c) {
    if (!c->o_wl.batch) return DAGCON_OK;
    ENSURE(c, c->run.wl_cnt, (size_t)c->T * 8); ENSURE(c, c->run.wl_block, (size_t)c->T * 4); ENSURE(c, c->run.wl_flip, (size_t)c->T);
    ENSURE(c, c->run.wl_hap, (size_t)c->A); ENSURE(c, c->run.wl_phase, c->site_arena.cap);
    return DAGCON_OK;
}

void winphase_params(Ctx *c, DgParams &p) {
    if (!c->o_wl.batch) return;
    p.wl_rec = c->in.wl_rec.as<const uint32_t>(); p.wl_tgt = c->in.wl_tgt.as<const uint32_t>();
    p.wl_cnt = c->run.wl_cnt.as<uint32_t>(); p.wl_block = c->run.wl_block.as<uint32_t>(); p.wl_flip = c->run.wl_flip.as<uint8_t>();
    p.wl_hap = c->run.wl_hap.as<uint8_t>(); p.wl_phase = c->run.wl_phase.as<int8_t>();
    p.wl_min_links = c->wl_batch_opts.min_links; p.wl_max_ppm = c->wl_batch_opts.max_conflict_ppm;
}

void winphase_launch(Ctx *c, const DgParams &p) {
    if (!c->o_wl.batch || !reads_ran(c)) return;
    hipStream_t s = c->stream;
    // the windows' labels joined into blocks: a wave per window, one scan, a thread per alignment and site.  Every word
    // they leave is written in every execution: nothing to clear
    hipLaunchKernelGGL(k_wl_pairs, dim3((c->T + 3) / 4), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_wl_scan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_wl_apply, dim3((uint32_t)((std::max<uint64_t>(c->A, p.site_cap) + 255) / 256)), dim3(256), 0, s, p);
}

}  // namespace

int dagcon_set_window_phase(dagcon_ctx *ctx, const dagcon_window_phase_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!o) { c->o_wl.on = false; return DAGCON_OK; }
    if (o->max_conflict_ppm > 1000000u) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_window_phase: max_conflict_ppm %u is more than 1000000", o->max_conflict_ppm);
    c->wl_opts = *o;
    c->o_wl.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_window_phase(dagcon_ctx *ctx, dagcon_window_phase *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_wl, "dagcon_fetch_window_phase")) return r;
    const uint32_t T = c->T;
    WinPhaseOut &o = c->r_winphase;
    if (!c->o_wl.fetched) {
        // the alignments and the sites go into the host's order as in dagcon_fetch_site_reads
        if (int r = host_order(c)) return r;
        const HostOrder &h = c->order;
        const uint32_t A = c->A;
        const uint64_t ns = c->r_sites.n_dev;
        const bool ran = reads_ran(c);
        std::vector<uint32_t> cnt((size_t)T * 2, 0u);
        std::vector<uint8_t> hap((size_t)A, 0);
        std::vector<int8_t> sigma((size_t)ns, 0);
        o.block.assign((size_t)T + 1, 0u); o.flip.assign((size_t)T + 1, 0);
        for (uint32_t t = 0; t < T; t++) o.block[t] = t;
        if (ran) {
            HIPCHK(c, d2h(c, cnt.data(), c->run.wl_cnt.p, (size_t)T * 8));
            HIPCHK(c, d2h(c, o.block.data(), c->run.wl_block.p, (size_t)T * 4));
            HIPCHK(c, d2h(c, o.flip.data(), c->run.wl_flip.p, (size_t)T));
            HIPCHK(c, d2h(c, hap.data(), c->run.wl_hap.p, (size_t)A));
            if (ns) HIPCHK(c, d2h(c, sigma.data(), c->run.wl_phase.p, (size_t)ns));
        }
        o.same.assign((size_t)T + 1, 0u); o.diff.assign((size_t)T + 1, 0u);
        for (uint32_t t = 0; t < T; t++) {
            o.same[t] = cnt[2 * (size_t)t]; o.diff[t] = cnt[2 * (size_t)t + 1];
            if (o.block[t] > t || o.flip[t] > 1u || (o.block[t] == t && o.flip[t]))
                return fail(c, DAGCON_ERR_INTERNAL, "k_wl_scan: window %u has block %u, flip %u", t, o.block[t], o.flip[t]);
        }
        const size_t nx = h.aln.size();
        o.hap.assign(nx + 1, 0);
        for (size_t x = 0; x < nx; x++) {
            const uint8_t hp = hap[h.aln[x]];
            if (hp > 2u) return fail(c, DAGCON_ERR_INTERNAL, "k_wl_apply: alignment %u has hap %u", h.aln[x], hp);
            o.hap[x] = hp;
        }
        o.phase.assign(c->r_sites.pos.size() + 1, 0);
        gather_sites(c, sigma.data(), o.phase.data());
        c->o_wl.fetched = true;
    }
    out->n_windows = T;
    out->same = o.same.data(); out->diff = o.diff.data(); out->block = o.block.data(); out->flip = o.flip.data();
    out->n_aln = c->order.aln.size(); out->hap = o.hap.data();
    out->n_sites = c->r_sites.pos.size(); out->phase = o.phase.data();
    return DAGCON_OK;
}

// ---- the alleles at the sites (k_alleles.hip.h) ----
namespace {

int alleles_room(Ctx *c) {
    if (!c->o_al.batch) return DAGCON_OK;
    const size_t ne = c->sr_arena.cap, ns = c->site_arena.cap;
    // (20 bytes an entry and 28 a site; the compact tables wait for dagcon_fetch_site_alleles, which knows their size)
    ENSURE(c, c->run.al_map, ne * 2); ENSURE(c, c->run.al_idx, ne * 2);
    ENSURE(c, c->run.al_soff, ns * 8); ENSURE(c, c->run.al_cur, (ns + 1) * 4); ENSURE(c, c->run.al_nd, ns * 4);
    ENSURE(c, c->run.al_deep, ns * 4); ENSURE(c, c->run.al_toff, ns * 8);
    ENSURE(c, c->run.al_srt, ne * 8); ENSURE(c, c->run.al_tcnt, ne * 4); ENSURE(c, c->run.al_thap, ne * 4);
    ENSURE(c, c->run.al_tot, 16);
    return DAGCON_OK;
}

void alleles_params(Ctx *c, DgParams &p) {
    if (!c->o_al.batch) return;
    p.al_map = c->run.al_map.as<uint16_t>(); p.al_idx = c->run.al_idx.as<uint16_t>();
    p.al_soff = c->run.al_soff.as<unsigned long long>(); p.al_cur = c->run.al_cur.as<uint32_t>(); p.al_nd = c->run.al_nd.as<uint32_t>();
    p.al_deep = c->run.al_deep.as<uint32_t>(); p.al_toff = c->run.al_toff.as<unsigned long long>();
    p.al_srt = c->run.al_srt.as<unsigned long long>(); p.al_tcnt = c->run.al_tcnt.as<uint32_t>(); p.al_thap = c->run.al_thap.as<uint32_t>();
    p.al_ckey = c->run.al_ckey.as<unsigned long long>(); p.al_ccnt = c->run.al_ccnt.as<uint32_t>(); p.al_chap = c->run.al_chap.as<uint32_t>();
    p.al_ent_top = c->run.al_tot.as<unsigned long long>(); p.al_top = p.al_ent_top + 1;
    p.al_nocap = ~0ull;
}

int alleles_launch(Ctx *c, const DgParams &p) {
    if (!c->o_al.batch || !reads_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    // a stretch per site, the keys, a table per site, the tables' places, an index per entry (and the counts per label,
    // behind the split).  The sites' cursors start from zero in every execution, a re-run included
    const dim3 sg((uint32_t)((p.site_cap + 3) / 4)), ag((c->A + 3) / 4);
    HIPCHK(c, hipMemsetAsync(c->run.al_cur.p, 0, (p.site_cap + 1) * 4, s));
    hipLaunchKernelGGL(k_al_soff, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_al_keys, ag, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_al_table, sg, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_al_table_deep, dim3(1024), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_al_tscan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_al_index, ag, dim3(256), 0, s, p);
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_site_alleles(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    reinterpret_cast<Ctx *>(ctx)->o_al.on = on != 0;
    return DAGCON_OK;
}

int dagcon_fetch_site_alleles(dagcon_ctx *ctx, dagcon_site_alleles *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_al, "dagcon_fetch_site_alleles")) return r;
    const bool phase = c->sr_batch_opts.phase != 0;
    AllelesOut &o = c->r_alleles;
    if (!c->o_al.fetched) {
        // the entries in the host's terms first (which of the device's survive, and each one's site); then the copies
        // dagcon_fetch left out: the tables' places, the compact tables, an index per entry.  A failed target's sites and
        // entries go, as in dagcon_fetch_site_reads
        dagcon_site_reads sr;
        if (int r = dagcon_fetch_site_reads(ctx, &sr)) return r;
        HIPCHK(c, hipSetDevice(c->device));
        const HostOrder &h = c->order;
        const SitesOut &s = c->r_sites;
        const std::vector<uint64_t> &x_site = c->r_reads.site;
        const uint32_t T = c->T;
        const uint64_t ne = c->r_reads.n_dev_ent, ns = s.n_dev;
        const bool ran = reads_ran(c);
        unsigned long long tot[2] = {0ull, 0ull};
        if (ran) HIPCHK(c, d2h(c, tot, c->run.al_tot.p, sizeof tot));
        const uint64_t na = tot[1];
        if (na > c->sr_arena.cap || (!ran && (ne || ns)))
            return fail(c, DAGCON_ERR_INTERNAL, "k_al_tscan: %llu alleles in an arena of %llu", (unsigned long long)na, (unsigned long long)c->sr_arena.cap);
        std::vector<uint64_t> toff((size_t)ns), key((size_t)na);
        std::vector<uint32_t> nd((size_t)ns), count((size_t)na), hapw((size_t)na);
        std::vector<uint16_t> idx((size_t)ne);
        if (ns) { HIPCHK(c, d2h(c, toff.data(), c->run.al_toff.p, (size_t)ns * 8)); HIPCHK(c, d2h(c, nd.data(), c->run.al_nd.p, (size_t)ns * 4)); }
        if (na) {
            // the compact copy, now that its size is known: room, zeros (a table k_al_pack refuses stays empty and fails
            // the checks below), the copy on the stream
            ENSURE(c, c->run.al_ckey, (size_t)na * 8); ENSURE(c, c->run.al_ccnt, (size_t)na * 4); ENSURE(c, c->run.al_chap, (size_t)na * 4);
            HIPCHK(c, hipMemsetAsync(c->run.al_ckey.p, 0, (size_t)na * 8, c->stream));
            HIPCHK(c, hipMemsetAsync(c->run.al_ccnt.p, 0, (size_t)na * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(c->run.al_chap.p, 0, (size_t)na * 4, c->stream));
            DgParams p;
            fill_params(c, p);
            hipLaunchKernelGGL(k_al_pack, dim3((uint32_t)((p.site_cap + 3) / 4)), dim3(256), 0, c->stream, p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, d2h(c, key.data(), c->run.al_ckey.p, (size_t)na * 8)); HIPCHK(c, d2h(c, count.data(), c->run.al_ccnt.p, (size_t)na * 4));
            HIPCHK(c, d2h(c, hapw.data(), c->run.al_chap.p, (size_t)na * 4));
        }
        if (ne) HIPCHK(c, d2h(c, idx.data(), c->run.al_idx.p, (size_t)ne * 2));
        o.begin.assign(1, 0); o.key.clear(); o.count.clear(); o.hap.clear(); o.ent.clear();
        for (uint32_t t = 0; t < T; t++) {
            if (c->r_status[t] != DAGCON_OK) continue;
            for (uint64_t j = s.begin[t]; j < s.begin[t + 1]; j++) {
                const uint64_t d = s.dev_begin[t] + (j - s.begin[t]);
                uint64_t depth = 0, sum = 0;
                for (int q = 0; q < 6; q++) depth += s.counts[j * 8 + q];
                if (d >= ns || toff[d] > na || nd[d] > na - toff[d] || !nd[d])
                    return fail(c, DAGCON_ERR_INTERNAL, "k_al_table: site %llu of target %u has alleles [%llu, + %u) of %llu", (unsigned long long)d, t,
                                (unsigned long long)(d < ns ? toff[d] : 0), d < ns ? nd[d] : 0u, (unsigned long long)na);
                for (uint64_t i = toff[d]; i < toff[d] + nd[d]; i++) {
                    const uint32_t c1 = hapw[i] & 0xFFFFu, c2 = hapw[i] >> 16;
                    sum += count[i];
                    if ((key[i] >> 61) || !count[i] || (uint64_t)c1 + c2 > count[i])
                        return fail(c, DAGCON_ERR_INTERNAL, "k_al_table: allele %llu of site %llu: key %llx, count %u, c1 %u, c2 %u", (unsigned long long)(i - toff[d]),
                                    (unsigned long long)d, (unsigned long long)key[i], count[i], c1, c2);
                    o.key.push_back(key[i]); o.count.push_back(count[i]);
                    o.hap.push_back((uint16_t)c1); o.hap.push_back((uint16_t)c2); o.hap.push_back((uint16_t)(count[i] - c1 - c2));
                }
                if (sum != depth) return fail(c, DAGCON_ERR_INTERNAL, "k_al_table: the alleles of site %llu count %llu entries, its depth is %llu", (unsigned long long)d,
                                              (unsigned long long)sum, (unsigned long long)depth);
                o.begin.push_back(o.key.size());
            }
        }
        // the entries, in the order of dagcon_fetch_site_reads (x_site: each one's site there)
        for (size_t k = 0; k < h.aln.size(); k++) {
            const uint64_t e0 = h.ent_begin[k];
            for (uint64_t j = e0; j < e0 + h.ent_n[k]; j++) {
                const uint64_t x = o.ent.size();
                if (x + 1 >= x_site.size() || idx[j] >= o.begin[x_site[x] + 1] - o.begin[x_site[x]])
                    return fail(c, DAGCON_ERR_INTERNAL, "k_al_index: entry %llu of alignment %u has allele %u", (unsigned long long)(j - e0), h.aln[k], idx[j]);
                o.ent.push_back(idx[j]);
            }
        }
        if (o.ent.size() + 1 != x_site.size())
            return fail(c, DAGCON_ERR_INTERNAL, "k_al_index: %llu entries with an allele, %llu entries", (unsigned long long)o.ent.size(), (unsigned long long)(x_site.size() - 1));
        pad(o.key, o.count, o.ent, o.hap, o.hap, o.hap);
        c->o_al.fetched = true;
    }
    out->n_sites = o.begin.size() - 1;
    out->al_begin = o.begin.data(); out->key = o.key.data(); out->count = o.count.data();
    out->hap_count = phase ? o.hap.data() : nullptr;
    out->n_ent = o.ent.size() - 1; out->ent_allele = o.ent.data();
    return DAGCON_OK;
}

// host only: the one implementation is the command line's (host/alleles.h)
int dagcon_allele_text(uint64_t key, char *out, size_t cap) { return dg_allele_text(key, out, cap); }

// ---- adjacent sites joined into runs (k_join.hip.h) ----
namespace {

int join_room(Ctx *c) {
    if (!c->o_jn.batch) return DAGCON_OK;
    const size_t ne = c->sr_arena.cap, ns = c->site_arena.cap;
    // (20 bytes an entry and 36 a site; the compact tables wait for dagcon_fetch_joined_sites, which knows their size)
    ENSURE(c, c->run.jn_run, ns * 4); ENSURE(c, c->run.jn_sfirst, ns * 4); ENSURE(c, c->run.jn_rbeg, (ns + 1) * 4);
    ENSURE(c, c->run.jn_cur, (2 * ns + 1) * 4); ENSURE(c, c->run.jn_nd, ns * 4); ENSURE(c, c->run.jn_deep, ns * 4); ENSURE(c, c->run.jn_toff, ns * 8);
    ENSURE(c, c->run.jn_key, ne * 8); ENSURE(c, c->run.jn_tcnt, ne * 4); ENSURE(c, c->run.jn_thap, ne * 4);
    ENSURE(c, c->run.jn_map, ne * 2); ENSURE(c, c->run.jn_idx, ne * 2);
    ENSURE(c, c->run.jn_tot, 32);
    return DAGCON_OK;
}

void join_params(Ctx *c, DgParams &p) {
    if (!c->o_jn.batch) return;
    p.jn_run = c->run.jn_run.as<uint32_t>(); p.jn_sfirst = c->run.jn_sfirst.as<uint32_t>(); p.jn_rbeg = c->run.jn_rbeg.as<uint32_t>();
    p.jn_cur = c->run.jn_cur.as<uint32_t>(); p.jn_part = p.jn_cur + c->site_arena.cap + 1;
    p.jn_nd = c->run.jn_nd.as<uint32_t>(); p.jn_deep = c->run.jn_deep.as<uint32_t>(); p.jn_toff = c->run.jn_toff.as<unsigned long long>();
    p.jn_key = c->run.jn_key.as<unsigned long long>(); p.jn_tcnt = c->run.jn_tcnt.as<uint32_t>(); p.jn_thap = c->run.jn_thap.as<uint32_t>();
    p.jn_map = c->run.jn_map.as<uint16_t>(); p.jn_idx = c->run.jn_idx.as<uint16_t>();
    p.jn_ckey = c->run.jn_ckey.as<unsigned long long>(); p.jn_ccnt = c->run.jn_ccnt.as<uint32_t>(); p.jn_chap = c->run.jn_chap.as<uint32_t>();
    p.jn_st_top = c->run.jn_tot.as<unsigned long long>(); p.jn_run_top = p.jn_st_top + 1; p.jn_top = p.jn_st_top + 2;
}

int join_launch(Ctx *c, const DgParams &p) {
    if (!c->o_jn.batch || !reads_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    // the runs, the spanning members' keys, a table per run, the tables' places, an index per entry (and the counts per
    // label).  The runs' cursors and partial counts start from zero in every execution, a re-run included
    const dim3 rg((uint32_t)((p.site_cap + 3) / 4)), ag((c->A + 3) / 4);
    HIPCHK(c, hipMemsetAsync(c->run.jn_cur.p, 0, (2 * p.site_cap + 1) * 4, s));
    hipLaunchKernelGGL(k_jn_stretch, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_jn_runs, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_jn_keys, ag, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_jn_table, rg, dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_jn_table_deep, dim3(1024), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_jn_tscan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(k_jn_index, ag, dim3(256), 0, s, p);
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_site_join(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    reinterpret_cast<Ctx *>(ctx)->o_jn.on = on != 0;
    return DAGCON_OK;
}

int dagcon_fetch_joined_sites(dagcon_ctx *ctx, dagcon_joined_sites *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_jn, "dagcon_fetch_joined_sites")) return r;
    const bool phase = c->sr_batch_opts.phase != 0;
    JoinedOut &o = c->r_joined;
    if (!c->o_jn.fetched) {
        // the sites, the entries and the alleles in the host's terms first; then the copies dagcon_fetch left out: the
        // runs, their members' counts, the tables' places, the compact tables, an index per entry.  A failed target's
        // sites, runs and entries go, as in dagcon_fetch_site_alleles
        dagcon_site_alleles sa;
        if (int r = dagcon_fetch_site_alleles(ctx, &sa)) return r;
        HIPCHK(c, hipSetDevice(c->device));
        const HostOrder &h = c->order;
        const SitesOut &s = c->r_sites;
        const std::vector<uint64_t> &x_site = c->r_reads.site;
        const uint32_t T = c->T;
        const uint64_t ne = c->r_reads.n_dev_ent, ns = s.n_dev;
        const bool ran = reads_ran(c);
        unsigned long long tot[3] = {0ull, 0ull, 0ull};
        if (ran) HIPCHK(c, d2h(c, tot, c->run.jn_tot.p, sizeof tot));
        const uint64_t nr = tot[1], nj = tot[2];
        if (nr > ns || nj > c->sr_arena.cap || (ns && ran && !nr))
            return fail(c, DAGCON_ERR_INTERNAL, "k_jn_runs: %llu runs of %llu sites, %llu joined alleles in an arena of %llu", (unsigned long long)nr, (unsigned long long)ns,
                        (unsigned long long)nj, (unsigned long long)c->sr_arena.cap);
        std::vector<uint32_t> rbeg((size_t)nr + 1, 0u), span((size_t)nr), part((size_t)nr), nd((size_t)nr), count((size_t)nj), hapw((size_t)nj);
        std::vector<uint64_t> toff((size_t)nr), key((size_t)nj);
        std::vector<uint16_t> idx((size_t)ne);
        if (nr) {
            HIPCHK(c, d2h(c, rbeg.data(), c->run.jn_rbeg.p, ((size_t)nr + 1) * 4)); HIPCHK(c, d2h(c, span.data(), c->run.jn_cur.p, (size_t)nr * 4));
            HIPCHK(c, d2h(c, part.data(), c->run.jn_cur.as<uint32_t>() + c->site_arena.cap + 1, (size_t)nr * 4));
            HIPCHK(c, d2h(c, nd.data(), c->run.jn_nd.p, (size_t)nr * 4)); HIPCHK(c, d2h(c, toff.data(), c->run.jn_toff.p, (size_t)nr * 8));
        }
        if (nj) {
            // the compact copy, now that its size is known: room, zeros (a table k_jn_pack refuses stays empty and fails
            // the checks below), the copy on the stream
            ENSURE(c, c->run.jn_ckey, (size_t)nj * 8); ENSURE(c, c->run.jn_ccnt, (size_t)nj * 4); ENSURE(c, c->run.jn_chap, (size_t)nj * 4);
            HIPCHK(c, hipMemsetAsync(c->run.jn_ckey.p, 0, (size_t)nj * 8, c->stream));
            HIPCHK(c, hipMemsetAsync(c->run.jn_ccnt.p, 0, (size_t)nj * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(c->run.jn_chap.p, 0, (size_t)nj * 4, c->stream));
            DgParams p;
            fill_params(c, p);
            hipLaunchKernelGGL(k_jn_pack, dim3((uint32_t)((p.site_cap + 3) / 4)), dim3(256), 0, c->stream, p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, d2h(c, key.data(), c->run.jn_ckey.p, (size_t)nj * 8)); HIPCHK(c, d2h(c, count.data(), c->run.jn_ccnt.p, (size_t)nj * 4));
            HIPCHK(c, d2h(c, hapw.data(), c->run.jn_chap.p, (size_t)nj * 4));
        }
        if (ne) HIPCHK(c, d2h(c, idx.data(), c->run.jn_idx.p, (size_t)ne * 2));
        o.run_begin.clear(); o.spanning.clear(); o.partial.clear(); o.begin.assign(1, 0); o.key.clear(); o.count.clear(); o.hap.clear(); o.ent.clear();
        std::vector<uint32_t> run_of((size_t)s.pos.size() + 1, 0u);           // a host site's run
        uint64_t r = 0;                                                       // the device's runs ascend with its sites
        for (uint32_t t = 0; t < T; t++) {
            const uint64_t d0 = s.dev_begin[t], d1 = s.dev_begin[t + 1];
            while (r < nr && rbeg[r] < d0) r++;
            if (c->r_status[t] != DAGCON_OK) continue;
            uint64_t first = 0;                                               // of the stretch, in the host's list
            for (uint64_t j = s.begin[t]; j < s.begin[t + 1]; j++) {
                // rule 10.1 on the host's list; the device's run must begin exactly where the rule says
                const bool cont = j > s.begin[t] && s.pos[j] == s.pos[j - 1] + 1u;
                if (!cont) first = j;
                const bool head = !cont || (j - first) % 16u == 0u;
                const uint64_t d = d0 + (j - s.begin[t]);
                const bool dev_head = r < nr && rbeg[r] == d;
                if (head != dev_head || d >= d1)
                    return fail(c, DAGCON_ERR_INTERNAL, "k_jn_runs: site %llu of target %u: a run head by the rule %d, on the device %d", (unsigned long long)d, t, (int)head, (int)dev_head);
                if (head) {
                    uint64_t depth = 0, sum = 0;
                    for (int q = 0; q < 6; q++) depth += s.counts[j * 8 + q];
                    if (toff[r] > nj || nd[r] > nj - toff[r] || span[r] > depth || (uint64_t)span[r] + part[r] < depth || (!nd[r]) != (!span[r]))
                        return fail(c, DAGCON_ERR_INTERNAL, "k_jn_table: run %llu of target %u has joined alleles [%llu, + %u) of %llu, %u spanning and %u partial members, depth %llu",
                                    (unsigned long long)r, t, (unsigned long long)toff[r], nd[r], (unsigned long long)nj, span[r], part[r], (unsigned long long)depth);
                    for (uint64_t i = toff[r]; i < toff[r] + nd[r]; i++) {
                        const uint32_t c1 = hapw[i] & 0xFFFFu, c2 = hapw[i] >> 16;
                        sum += count[i];
                        if (!count[i] || (uint64_t)c1 + c2 > count[i])
                            return fail(c, DAGCON_ERR_INTERNAL, "k_jn_table: joined allele %llu of run %llu: key %llx, count %u, c1 %u, c2 %u", (unsigned long long)(i - toff[r]),
                                        (unsigned long long)r, (unsigned long long)key[i], count[i], c1, c2);
                        o.key.push_back(key[i]); o.count.push_back(count[i]);
                        o.hap.push_back((uint16_t)c1); o.hap.push_back((uint16_t)c2); o.hap.push_back((uint16_t)(count[i] - c1 - c2));
                    }
                    if (sum != span[r]) return fail(c, DAGCON_ERR_INTERNAL, "k_jn_table: the joined alleles of run %llu count %llu members, %u span it", (unsigned long long)r,
                                                    (unsigned long long)sum, span[r]);
                    o.run_begin.push_back(j); o.spanning.push_back(span[r]); o.partial.push_back(part[r]); o.begin.push_back(o.key.size());
                    r++;
                }
                run_of[j] = (uint32_t)(o.spanning.size() - 1);
            }
        }
        o.run_begin.push_back(s.pos.size());
        // the entries, in the order of dagcon_fetch_site_reads (x_site: each one's site there)
        for (size_t k = 0; k < h.aln.size(); k++) {
            const uint64_t e0 = h.ent_begin[k];
            for (uint64_t j = e0; j < e0 + h.ent_n[k]; j++) {
                const uint64_t x = o.ent.size();
                if (x + 1 >= x_site.size()) return fail(c, DAGCON_ERR_INTERNAL, "k_jn_index: more than %llu entries", (unsigned long long)(x_site.size() - 1));
                const uint32_t rr = run_of[x_site[x]];
                if (idx[j] != 0xFFFFu && idx[j] >= o.begin[rr + 1] - o.begin[rr])
                    return fail(c, DAGCON_ERR_INTERNAL, "k_jn_index: entry %llu of alignment %u has joined allele %u", (unsigned long long)(j - e0), h.aln[k], idx[j]);
                o.ent.push_back(idx[j]);
            }
        }
        if (o.ent.size() + 1 != x_site.size())
            return fail(c, DAGCON_ERR_INTERNAL, "k_jn_index: %llu entries with a joined allele, %llu entries", (unsigned long long)o.ent.size(), (unsigned long long)(x_site.size() - 1));
        pad(o.key, o.count, o.ent, o.hap, o.hap, o.hap, o.spanning, o.partial);
        c->o_jn.fetched = true;
    }
    out->n_runs = o.run_begin.size() - 1;
    out->run_begin = o.run_begin.data(); out->spanning = o.spanning.data(); out->partial = o.partial.data();
    out->jal_begin = o.begin.data(); out->key = o.key.data(); out->count = o.count.data();
    out->hap_count = phase ? o.hap.data() : nullptr;
    out->n_ent = o.ent.size() - 1; out->ent_joined = o.ent.data();
    return DAGCON_OK;
}

// ---- the tally of the split, and the batch of the groups (k_hap.hip.h) ----
namespace {

int calls_arm(Ctx *c, const std::vector<uint32_t> &src_target);      // dagcon_set_hap_calls, below: its part of dagcon_upload_haps
int keep_check(Ctx *c, bool windows, uint32_t n_windows);            // dagcon_set_window_keep, below: its parts
int keep_arm(Ctx *c, const std::vector<uint32_t> *src_target);

int hap_room(Ctx *c) {
    if (!c->o_hap.batch) return DAGCON_OK;
    ENSURE(c, c->run.hap_cnt, c->site_arena.cap * 8); ENSURE(c, c->run.hap_rec, (size_t)c->T * DG_HAP_REC * 4);
    return DAGCON_OK;
}

void hap_params(Ctx *c, DgParams &p) {
    if (!c->o_hap.batch) return;
    p.hap_cnt = c->run.hap_cnt.as<uint32_t>(); p.hap_rec = c->run.hap_rec.as<uint32_t>();
    p.hap_min_sites = c->hap_batch_opts.min_sites; p.hap_min_reads = c->hap_batch_opts.min_reads;
    p.hap_min_cov = std::max<uint32_t>(1u, c->opts.min_cov);
}

int hap_launch(Ctx *c, const DgParams &p) {
    if (!c->o_hap.batch || !reads_ran(c)) return DAGCON_OK;
    hipStream_t s = c->stream;
    // the sites' counters start from zero in every execution, a re-run included; a wave per alignment, then a block per target
    HIPCHK(c, hipMemsetAsync(c->run.hap_cnt.p, 0, p.site_cap * 8, s));
    hipLaunchKernelGGL(k_hap_tally, dim3((c->A + 3) / 4), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_hap_targets, dim3(c->T), dim3(256), 0, s, p);
    return DAGCON_OK;
}

// the per-target records of the tally, once a fetch: n1 n2 n0 n_sep agree disagree and the split bit; a failed target has zeros
int hap_records(Ctx *c) {
    if (c->o_hap.fetched) return DAGCON_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t T = c->T;
    HapOut &o = c->r_haps;
    std::vector<uint32_t> rec((size_t)T * DG_HAP_REC, 0u);
    if (reads_ran(c)) HIPCHK(c, d2h(c, rec.data(), c->run.hap_rec.p, rec.size() * 4));
    o.rec.assign((size_t)6 * T + 1, 0u); o.split.assign((size_t)T + 1, 0);
    for (uint32_t t = 0; t < T; t++) {
        if (c->r_status[t] != DAGCON_OK) continue;
        const uint32_t *r = &rec[(size_t)t * DG_HAP_REC];
        const uint64_t K = c->h_aln_begin[t + 1] - c->h_aln_begin[t];
        if (r[6] > 1u || r[7] || (uint64_t)r[0] + r[1] + r[2] > K)
            return fail(c, DAGCON_ERR_INTERNAL, "k_hap_targets: target %u of %llu alignments has n1 %u, n2 %u, n0 %u, split %u", t, (unsigned long long)K, r[0], r[1], r[2], r[6]);
        for (int i = 0; i < 6; i++) o.rec[(size_t)i * T + t] = r[i];
        o.split[t] = (uint8_t)r[6];
    }
    c->o_hap.fetched = true;
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_hap_consensus(dagcon_ctx *ctx, const dagcon_hap_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!o) { c->o_hap.on = false; return DAGCON_OK; }
    c->hap_opts = *o;
    c->o_hap.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_hap_tally(dagcon_ctx *ctx, dagcon_hap_tally *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    int r;
    if ((r = need(c, c->o_hap, "dagcon_fetch_hap_tally")) || (r = hap_records(c))) return r;
    const uint32_t T = c->T;
    HapOut &o = c->r_haps;
    if (!o.sites_fetched) {
        // 8 bytes a site, in the device's order; the host's list leaves out the sites of failed targets
        const SitesOut &s = c->r_sites;
        const uint64_t ns = s.n_dev;
        std::vector<uint16_t> dev((size_t)ns * 4 + 4, 0);
        if (ns && c->A) HIPCHK(c, d2h(c, dev.data(), c->run.hap_cnt.p, (size_t)ns * 8));
        o.counts.assign(s.pos.size() * 4 + 4, 0);
        for (uint32_t t = 0; t < T; t++) {
            const uint64_t n = s.begin[t + 1] - s.begin[t];
            if (c->r_status[t] == DAGCON_OK && s.dev_begin[t] + n > ns) return fail(c, DAGCON_ERR_INTERNAL, "k_hap_tally: target %u has sites [%llu, + %llu) of %llu", t, (unsigned long long)s.dev_begin[t], (unsigned long long)n, (unsigned long long)ns);
        }
        gather_sites(c, dev.data(), o.counts.data(), 4);
        o.sites_fetched = true;
    }
    out->n_targets = T;
    out->n1 = o.rec.data(); out->n2 = out->n1 + T; out->n0 = out->n2 + T;
    out->n_sep = out->n0 + T; out->agree = out->n_sep + T; out->disagree = out->agree + T;
    out->split = o.split.data(); out->site_counts = o.counts.data();
    return DAGCON_OK;
}

int dagcon_upload_haps(dagcon_ctx *ctx) { return dagcon_upload_haps_swapped(ctx, nullptr); }

// swap[t] != 0: the two groups of split target t change names (the caller's orientation of its labels); NULL: none does
int dagcon_upload_haps_swapped(dagcon_ctx *ctx, const uint8_t *swap) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    int r;
    if ((r = need(c, c->o_hap, "dagcon_upload_haps")) || (r = hap_records(c))) return r;
    if ((r = keep_check(c, c->win_first, c->win_n))) { c->drop_results(Fresh::UPLOAD); return r; }     // (before any launch; as after any failed upload)
    const uint32_t T = c->T, A = c->A;
    std::vector<uint8_t> hap((size_t)A, 0);
    if (reads_ran(c)) HIPCHK(c, d2h(c, hap.data(), c->run.sr_hap.p, (size_t)A));
    // the plan, on the host: one byte an alignment and one record a target say everything upload_impl needs.  Group g of a
    // split target: its alignments of the device batch with hap g or 0 (the ones the graph did not take are 0 too); under
    // swap[t] the group the caller names g is the device's 3 - g
    std::vector<uint32_t> tlen, start, len, src_target;
    std::vector<uint64_t> begin(1, 0), off, bb_off, src;
    std::vector<uint8_t> label;
    for (uint32_t t = 0; t < T; t++) {
        if (!c->r_haps.split[t]) continue;
        for (uint8_t g = 1; g <= 2; g++) {
            const uint8_t dg = swap && swap[t] ? (uint8_t)(3u - g) : g;
            for (uint64_t a = c->h_aln_begin[t]; a < c->h_aln_begin[t + 1]; a++) {
                if (hap[a] > 2u) return fail(c, DAGCON_ERR_INTERNAL, "k_sr_split: alignment %llu has hap %u", (unsigned long long)a, hap[a]);
                if (hap[a] && hap[a] != dg) continue;
                off.push_back(c->h_aln_off[a]); len.push_back(c->h_aln_len[a]); start.push_back(c->h_aln_start[a]);
                src.push_back(c->h_aln_src[a]);
            }
            tlen.push_back(c->h_tlen[t]); bb_off.push_back(c->h_bb_off[t]);
            src_target.push_back(t); label.push_back(g); begin.push_back(off.size());
        }
    }
    dagcon_batch db;
    memset(&db, 0, sizeof db);
    db.n_targets = (uint32_t)tlen.size(); db.tlen = tlen.data(); db.aln_begin = begin.data();
    db.aln_start = start.data(); db.aln_off = off.data(); db.aln_len = len.data();
    db.blob_bytes = c->blob_bytes;
    if (c->have_bb) { db.backbone = c->in.bb.as<const char>(); db.backbone_off = bb_off.data(); }    // (in.bb itself: nothing is copied)
    // an upload like any other, but one that latches no optional output (Intake::HAPS); the switches stay as the caller set them
    if ((r = upload_impl(ctx, &db, c->in.q.p, c->in.t.p, Intake::HAPS))) return r;   // (as after any failed upload: the first batch's results are gone)
    if ((r = calls_arm(c, src_target)) || (r = keep_arm(c, &src_target))) return r;
    pad(src_target, label, src);
    HapMapOut &m = c->r_hapmap;
    m.src_target.swap(src_target); m.label.swap(label); m.aln_begin.swap(begin); m.aln_src.swap(src);
    m.valid = true;
    return DAGCON_OK;
}

int dagcon_fetch_hap_map(dagcon_ctx *ctx, dagcon_hap_map *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    const HapMapOut &m = c->r_hapmap;
    if (!m.valid) return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_hap_map without a dagcon_upload_haps as the last upload");
    out->n_targets = (uint32_t)(m.aln_begin.size() - 1);
    out->src_target = m.src_target.data(); out->label = m.label.data();
    out->aln_begin = m.aln_begin.data(); out->aln_src = m.aln_src.data();
    return DAGCON_OK;
}

// ---- the two groups' edits paired (k_hap_calls.hip.h) ----
namespace {

int calls_room(Ctx *c) {
    if (!c->o_hc.batch) return DAGCON_OK;
    ENSURE(c, c->run.hc_state, c->ed_arena.cap); ENSURE(c, c->run.hc_mate, c->ed_arena.cap * 8);
    return DAGCON_OK;
}

void calls_params(Ctx *c, DgParams &p) {
    if (!c->o_hc.batch) return;
    p.hc_state = c->run.hc_state.as<uint8_t>(); p.hc_mate = c->run.hc_mate.as<unsigned long long>();
}

// behind the edit kernels, in every execution of the run (a re-run after DG_E_ED_OVF included): a wave per derived target
void calls_launch(Ctx *c, const DgParams &p) {
    if (!c->o_hc.batch || !c->T) return;
    hipLaunchKernelGGL(k_hap_calls, dim3((c->T + 3) / 4), dim3(256), 0, c->stream, p);
}

// dagcon_upload_haps, behind its upload_impl: a derived target's bases are its source target's (a window's) in cg.t
int calls_arm(Ctx *c, const std::vector<uint32_t> &src_target) {
    if (!c->o_ed.batch) return DAGCON_OK;
    std::vector<uint64_t> tbase(src_target.size());
    for (size_t d = 0; d < tbase.size(); d++) tbase[d] = c->h_ed_tbase[src_target[d]];
    c->h_ed_tbase.swap(tbase);
    UPLOAD(c, c->in.ed_tbase, c->h_ed_tbase);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_hap_calls(dagcon_ctx *ctx, int on) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->o_ed.on) return fail(c, DAGCON_ERR_STATE, "dagcon_set_hap_calls without dagcon_set_edits on");
    c->o_hc.on = on != 0;
    return DAGCON_OK;
}

int dagcon_fetch_hap_calls(dagcon_ctx *ctx, dagcon_hap_calls *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_hc, "dagcon_fetch_hap_calls", c->o_ed.on)) return r;
    HapCallsOut &o = c->r_hc;
    if (!c->o_hc.fetched) {
        // the copies dagcon_fetch left out (9 bytes an edit), and the device's arrays in the order of dagcon_fetch_edits: a
        // failed target's edits go, as in edits_unpack, and a mate becomes an index into the listed edits
        HIPCHK(c, hipSetDevice(c->device));
        const EditsOut &e = c->r_edits;
        const uint64_t nd = e.n_dev, n = e.dev_idx.size();
        const uint32_t T = c->T;
        std::vector<uint8_t> state((size_t)nd);
        std::vector<uint64_t> mate((size_t)nd), host_of((size_t)nd, UINT64_MAX);
        if (nd) { HIPCHK(c, d2h(c, state.data(), c->run.hc_state.p, (size_t)nd)); HIPCHK(c, d2h(c, mate.data(), c->run.hc_mate.p, (size_t)nd * 8)); }
        for (uint64_t i = 0; i < n; i++) host_of[e.dev_idx[i]] = i;
        o.state.assign((size_t)n + 1, 0); o.mate.assign((size_t)n + 1, UINT64_MAX);
        for (uint32_t d = 0; d < T; d++) {
            // the partner's stretch of the listed edits: empty when it failed or there is none
            const uint32_t dp = d ^ 1u;
            const uint64_t q0 = dp < T ? e.tgt_begin[dp] : 0, q1 = dp < T ? e.tgt_begin[dp + 1] : 0;
            for (uint64_t i = e.tgt_begin[d]; i < e.tgt_begin[d + 1]; i++) {
                const uint64_t x = e.dev_idx[i];
                const uint64_t m = mate[x] < nd ? host_of[mate[x]] : UINT64_MAX;
                const bool paired = state[x] == DAGCON_HC_CLASH || state[x] == DAGCON_HC_HOM;
                if (state[x] > DAGCON_HC_HOM || (mate[x] != UINT64_MAX && (m < q0 || m >= q1)) || paired != (m != UINT64_MAX))
                    return fail(c, DAGCON_ERR_INTERNAL, "k_hap_calls: edit %llu of derived target %u has state %u and mate %llu (the partner's edits are [%llu, %llu))",
                                (unsigned long long)(i - e.tgt_begin[d]), d, state[x], (unsigned long long)m, (unsigned long long)q0, (unsigned long long)q1);
                o.state[i] = state[x]; o.mate[i] = m;
            }
        }
        c->o_hc.fetched = true;
    }
    out->n = o.state.size() - 1;
    out->state = o.state.data(); out->mate = o.mate.data();
    return DAGCON_OK;
}

// ---- the kept part of every segment of a window (k_keep.hip.h) ----
namespace {

// before any launch of an upload the switch would take effect for (a windows upload of n_windows windows, or the batch
// dagcon_upload_haps derives from one): one lo / hi pair per window of the first batch
int keep_check(Ctx *c, const bool windows, const uint32_t n_windows) {
    if (!c->o_keep.on || !windows || c->keep_lo.size() == n_windows) return DAGCON_OK;
    return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_window_keep: lo / hi for %zu windows, the first batch has %u", c->keep_lo.size(), n_windows);
}

int keep_room(Ctx *c) {
    if (!c->o_keep.batch) return DAGCON_OK;
    ENSURE(c, c->run.keep, c->seg_cap * sizeof(uint4));
    return DAGCON_OK;
}

void keep_params(Ctx *c, DgParams &p) {
    if (!c->o_keep.batch) return;
    p.keep_out = c->run.keep.as<uint4>();
    p.keep_lo = c->in.keep_lo.as<const uint32_t>(); p.keep_hi = c->in.keep_hi.as<const uint32_t>();
}

// behind k_bp_join and the edit kernels, in every execution of the run: a wave per segment of the arena (seg_top is the device's)
void keep_launch(Ctx *c, const DgParams &p) {
    if (!c->o_keep.batch) return;
    hipLaunchKernelGGL(k_win_keep, dim3((uint32_t)((c->seg_cap + 3) / 4)), dim3(256), 0, c->stream, p);
}

// behind upload_impl: each target's lo and hi.  A windows upload: target t is window t; dagcon_upload_haps: derived target
// d takes those of src_target[d]
int keep_arm(Ctx *c, const std::vector<uint32_t> *src_target) {
    if (!c->o_keep.batch) return DAGCON_OK;
    const uint32_t T = c->T;
    std::vector<uint32_t> lo((size_t)T), hi((size_t)T);
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t w = src_target ? (*src_target)[t] : t;
        if (w >= c->keep_lo.size()) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_window_keep: lo / hi for %zu windows, target %u is window %u", c->keep_lo.size(), t, w);
        lo[t] = c->keep_lo[w]; hi[t] = c->keep_hi[w];
    }
    UPLOAD(c, c->in.keep_lo, lo);
    UPLOAD(c, c->in.keep_hi, hi);
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // (lo and hi are locals)
    return DAGCON_OK;
}

}  // namespace

int dagcon_set_window_keep(dagcon_ctx *ctx, const dagcon_window_keep_opts *o) {
    if (!ctx) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!(c->opts.flags & DAGCON_FLAG_BASE_POS))
        return fail(c, DAGCON_ERR_STATE, "dagcon_set_window_keep on a context created without DAGCON_FLAG_BASE_POS");
    if (!o) { c->o_keep.on = false; return DAGCON_OK; }
    if (o->n && (!o->lo || !o->hi)) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_window_keep: lo / hi is NULL");
    for (uint32_t t = 0; t < o->n; t++)
        if (o->lo[t] > o->hi[t]) return fail(c, DAGCON_ERR_INVALID_ARG, "dagcon_set_window_keep: window %u has lo %u above hi %u", t, o->lo[t], o->hi[t]);
    c->keep_lo.assign(o->lo, o->lo + o->n); c->keep_hi.assign(o->hi, o->hi + o->n);
    c->o_keep.on = true;
    return DAGCON_OK;
}

int dagcon_fetch_window_keep(dagcon_ctx *ctx, dagcon_window_keep *out) {
    if (!ctx || !out) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (int r = need(c, c->o_keep, "dagcon_fetch_window_keep")) return r;
    KeepOut &o = c->r_keep;
    if (!c->o_keep.fetched) {
        // the copy dagcon_fetch left out, 16 bytes a segment, and the records from the device's segment order into that of
        // dagcon_results: the segments of every target that came through, as unpack_segments lists them
        HIPCHK(c, hipSetDevice(c->device));
        const StatBlock &sb = c->sb;
        const uint32_t *m_tfail = sb.h<uint32_t>(sb.o_tfail), *m_n_seg = sb.h<uint32_t>(sb.o_n_seg);
        const uint64_t *m_seg_first = sb.h<uint64_t>(sb.o_seg_first);
        const uint64_t nseg = c->h_st.seg_top;
        std::vector<uint32_t> rec((size_t)nseg * 4);
        if (c->T && nseg) HIPCHK(c, d2h(c, rec.data(), c->run.keep.p, (size_t)nseg * 16));
        o.i0.clear(); o.i1.clear(); o.p_first.clear(); o.p_last.clear();
        for (uint32_t t = 0; t < c->T; t++) {
            if (!c->h_tactive[t] || m_tfail[t]) continue;
            for (uint32_t i = 0; i < m_n_seg[t]; i++) {
                const uint64_t s = m_seg_first[t] + i, x = o.i0.size();
                if (s >= nseg || x >= c->r_seq_len.size()) return fail(c, DAGCON_ERR_INTERNAL, "k_win_keep: segment %llu of target %u of %llu segments", (unsigned long long)s, t, (unsigned long long)nseg);
                const uint32_t *r = &rec[(size_t)s * 4];
                if (r[0] > r[1] || r[1] > c->r_seq_len[x] || (r[0] == r[1] && (r[0] | r[2] | r[3])))
                    return fail(c, DAGCON_ERR_INTERNAL, "k_win_keep: segment %u of target %u has the part [%u, %u) of %u bases, positions %u and %u", i, t, r[0], r[1], c->r_seq_len[x], r[2], r[3]);
                o.i0.push_back(r[0]); o.i1.push_back(r[1]); o.p_first.push_back(r[2]); o.p_last.push_back(r[3]);
            }
        }
        if (o.i0.size() != c->r_seq_len.size())
            return fail(c, DAGCON_ERR_INTERNAL, "k_win_keep: %zu records for %zu segments", o.i0.size(), c->r_seq_len.size());
        pad(o.i0, o.i1, o.p_first, o.p_last);
        c->o_keep.fetched = true;
    }
    out->n_segments = o.i0.size() - 1;
    out->i0 = o.i0.data(); out->i1 = o.i1.data(); out->p_first = o.p_first.data(); out->p_last = o.p_last.data();
    return DAGCON_OK;
}

// ---- the pipeline's calls: every output in the order of its launches ----
namespace {

int outputs_room(Ctx *c) {
    int r;
    if ((r = edits_room(c)) || (r = pile_room(c)) || (r = reads_room(c)) || (r = hap_room(c)) || (r = winphase_room(c))) return r;
    if ((r = alleles_room(c)) || (r = calls_room(c)) || (r = keep_room(c)) || (r = link_room(c))) return r;
    return join_room(c);
}

void outputs_params(Ctx *c, DgParams &p) {
    edits_params(c, p); pile_params(c, p); reads_params(c, p); hap_params(c, p); winphase_params(c, p); alleles_params(c, p); join_params(c, p); calls_params(c, p); keep_params(c, p); link_params(c, p);
}

// between k_bp_join and the last event of a run that goes as far as bestPath (T > 0)
int outputs_launch(Ctx *c, const DgParams &p) {
    int r;
    edits_launch(c, p);
    calls_launch(c, p);
    keep_launch(c, p);
    if ((r = pile_launch(c, p)) || (r = reads_launch(c, p))) return r;
    winphase_launch(c, p);
    if ((r = alleles_launch(c, p)) || (r = join_launch(c, p))) return r;
    return hap_launch(c, p);
}

// upload_impl, once the batch is planned: what the outputs upload themselves and the first guesses of their arenas; a run
// with more records their number and is repeated (DG_E_ED_OVF, DG_E_SITE_OVF, DG_E_SR_OVF)
int outputs_upload(Ctx *c, const dagcon_batch *b) {
    const uint32_t T = c->T;
    if (c->o_ed.batch) c->ed_arena.cap = c->ed_cap_env > 0 ? (uint64_t)c->ed_cap_env : std::max<uint64_t>(c->ed_arena.cap, c->sum_bb / 8 + 1024);
    if (!c->o_pile.batch) return DAGCON_OK;
    // a target's positions [pile_begin[t], + tlen): every target has them, the ones no graph is built for too (all zero)
    c->h_pile_begin.assign((size_t)T + 1, 0);
    for (uint32_t t = 0; t < T; t++) c->h_pile_begin[t + 1] = c->h_pile_begin[t] + b->tlen[t];
    UPLOAD(c, c->in.pile_begin, c->h_pile_begin);
    c->site_arena.cap = std::max<uint64_t>(c->site_arena.cap, c->h_pile_begin[T] / 8 + 1024);
    if (!c->o_sr.batch) return DAGCON_OK;
    // a site index is 32 bits wide in an entry; the first guess is one column in 64 an entry
    if (c->h_pile_begin[T] > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "dagcon_set_site_reads: more than 2^32 - 16 target positions in a batch");
    c->sr_arena.cap = std::max<uint64_t>(c->sr_arena.cap, c->sum_len / 64 + 4096);
    return DAGCON_OK;
}

// dagcon_fetch: the sizes, each checked against its arena, and room for the copies.  The edit records come back in the
// fetch's second round, instead of the positions: the DgEdSeg records of the segments, then the DgEdit records, then
// the DgEvid records (all 8-byte aligned).  So do the sites; the pile-up's counts, 16 bytes a position, and the sites'
// entries stay on the device until their own fetch asks for them
int outputs_plan(Ctx *c, FetchPlan &f) {
    int r;
    f.want_ed = f.full && c->o_ed.batch;
    if ((r = arena_total(c, c->ed_arena, f.want_ed && c->T, f.n_ed))) return r;
    f.want_evid = f.want_ed && c->o_evid.batch;
    f.ed_seg_bytes = (size_t)f.nseg * sizeof(DgEdSeg); f.ed_bytes = f.ed_seg_bytes + (size_t)f.n_ed * sizeof(DgEdit);
    f.evid_bytes = f.want_evid ? (size_t)f.n_ed * sizeof(DgEvid) : 0;
    if (f.want_ed && (r = c->r_ed.reserve(c, f.ed_bytes + f.evid_bytes + 1))) return r;
    f.want_pile = f.full && c->o_pile.batch;
    if ((r = arena_total(c, c->site_arena, f.want_pile && sites_ran(c), f.n_site))) return r;
    return f.want_pile ? c->r_site.reserve(c, (size_t)f.n_site * sizeof(DgSite) + 1) : DAGCON_OK;
}

// their copies of the second round, behind the pipeline's own
int outputs_copies(Ctx *c, const FetchPlan &f, bool &queued) {
    char *const m_edb = c->r_ed.as<char>();
    if (f.want_ed && c->T && f.nseg) {
        HIPCHK(c, hipMemcpyAsync(m_edb, c->run.ed_seg.p, f.ed_seg_bytes, hipMemcpyDeviceToHost, c->stream));
        if (f.n_ed) HIPCHK(c, hipMemcpyAsync(m_edb + f.ed_seg_bytes, c->run.ed_out.p, (size_t)f.n_ed * sizeof(DgEdit), hipMemcpyDeviceToHost, c->stream));
        if (f.evid_bytes) HIPCHK(c, hipMemcpyAsync(m_edb + f.ed_bytes, c->run.evid.p, f.evid_bytes, hipMemcpyDeviceToHost, c->stream));
        queued = true;
    }
    if (f.n_site) { HIPCHK(c, hipMemcpyAsync(c->r_site.p, c->run.pile_site.p, (size_t)f.n_site * sizeof(DgSite), hipMemcpyDeviceToHost, c->stream)); queued = true; }
    return DAGCON_OK;
}

// the device's records in the host's terms (the number of the sites' entries came with the status block); what this
// step leaves marks every latched output's results as there
int outputs_unpack(Ctx *c, const FetchPlan &f) {
    int r;
    if ((r = edits_unpack(c, f)) || (r = pile_unpack(c, f))) return r;
    if (f.want_pile && c->o_sr.batch && (r = arena_total(c, c->sr_arena, sites_ran(c), c->r_reads.n_dev_ent))) return r;
    for (Output *o : c->outputs()) o->valid = f.full && o->batch;
    return DAGCON_OK;
}

}  // namespace
