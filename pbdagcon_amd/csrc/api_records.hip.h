// api_records.hip.h -- the record intake (SAM, BAM, PAF, cs:Z:, MD:Z:), its filter, the callers' page-locked memory, debugging aids
// (one translation unit with dagcon_api.hip, which includes it once).
namespace {
// ---- record intake: dagcon_upload_cigar, _windows, _packed, _strand, dagcon_upload_cs and dagcon_upload_cigar_md -------
// One path, upload_records: reset, scan, judge, then records_finish: rate, pick, plan, expand, hand-over (upload_md makes
// the targets between the scan and a judgement of its own, and joins at records_finish).  Whole targets and windows differ in
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
//   rebuilt()       PLAIN or PACKED from dagcon_upload_cigar_md: the targets are made on the device (CigarBufs::t, by the
//                   k_md_* kernels); b->t_blob is not read and may be NULL
class RecordSource {
  public:
    enum Kind { PLAIN, PACKED, STRANDED, DECODED };
    static RecordSource plain() { return RecordSource(PLAIN, nullptr); }
    static RecordSource packed() { return RecordSource(PACKED, nullptr); }
    static RecordSource stranded(const uint8_t *reverse) { return reverse ? RecordSource(STRANDED, reverse) : plain(); }
    static RecordSource decoded(const CsDecoded &cs) { return RecordSource(DECODED, &cs); }
    static RecordSource rebuilt(bool packed) { RecordSource s(packed ? PACKED : PLAIN, nullptr); s.rebuilt_ = true; return s; }
    Kind kind() const { return kind_; }
    bool rebuilt() const { return rebuilt_; }
    const uint8_t *reverse() const { return kind_ == STRANDED ? static_cast<const uint8_t *>(carried_) : nullptr; }
    const CsDecoded *cs() const { return kind_ == DECODED ? static_cast<const CsDecoded *>(carried_) : nullptr; }

  private:
    RecordSource(Kind k, const void *carried) : kind_(k), carried_(carried) {}
    Kind kind_;
    const void *carried_;
    bool rebuilt_ = false;
};

// reset: what any upload does to the context's state first
Ctx *intake_reset(dagcon_ctx *ctx) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    c->drop_results(Fresh::UPLOAD);
    for (Output *o : c->outputs()) o->batch = false;               // (upload_impl latches them: latch_outputs)
    return c;
}

// the checks a dagcon_cigar_batch and a dagcon_cs_batch share: the targets, their records' ranges, and the record count
int check_targets(Ctx *c, uint32_t T, const uint32_t *tlen, const uint64_t *t_off, const uint64_t *rec_begin, const char *t_blob, uint64_t t_bytes,
                  bool have_record_arrays, uint32_t &n, bool need_t_blob = true) {
    if (T && (!tlen || !rec_begin || !t_off)) return fail(c, DAGCON_ERR_INVALID_ARG, "tlen/t_off/rec_begin is NULL");
    const uint64_t n64 = T ? rec_begin[T] : 0;
    if (n64 > 0xFFFFFFF0ull) return fail(c, DAGCON_ERR_UNSUPPORTED, "too many records");
    n = (uint32_t)n64;
    if (n && !have_record_arrays) return fail(c, DAGCON_ERR_INVALID_ARG, "record arrays are NULL");
    if (T && rec_begin[0] != 0) return fail(c, DAGCON_ERR_INVALID_ARG, "rec_begin does not start at 0");
    for (uint32_t g = 0; g < T; g++) {
        if (rec_begin[g + 1] < rec_begin[g] || rec_begin[g + 1] > n64) return fail(c, DAGCON_ERR_INVALID_ARG, "rec_begin not monotone at target %u", g);
        if (t_off[g] > t_bytes || tlen[g] > t_bytes - t_off[g]) return fail(c, DAGCON_ERR_INVALID_ARG, "target %u runs past t_blob", g);
        if (tlen[g] && !t_blob && need_t_blob) return fail(c, DAGCON_ERR_INVALID_ARG, "t_blob is NULL");
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
    int r = check_targets(c, b->n_targets, b->tlen, b->t_off, b->rec_begin, b->t_blob, b->t_bytes, b->pos && b->q_off && b->q_len && b->op_begin, n, !src.rebuilt());
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
    ENSURE(c, d.q, b->q_bytes); ENSURE(c, d.t, b->t_bytes);
    if (n_ops && !cs) HIPCHK(c, hipMemcpyAsync(d.ops.p, b->ops + b->op_begin[0], n_ops * 4, hipMemcpyHostToDevice, s));
    if (b->q_bytes && b->q_blob) HIPCHK(c, hipMemcpyAsync(d.q.p, b->q_blob, b->q_bytes, hipMemcpyHostToDevice, s));
    if (b->t_bytes && b->t_blob && !cs && !src.rebuilt()) HIPCHK(c, hipMemcpyAsync(d.t.p, b->t_blob, b->t_bytes, hipMemcpyHostToDevice, s));
    UPLOAD(c, d.q_off, b->q_off, n);
    UPLOAD(c, d.op_begin, opb);
    UPLOAD(c, d.tile_begin, tile_begin);
    DgCigarParams &p = sc.p;
    memset(&p, 0, sizeof p);
    p.ops = d.ops.as<const uint32_t>(); p.op_begin = d.op_begin.as<const uint64_t>(); p.tile_begin = d.tile_begin.as<const uint64_t>();
    p.n = n; p.n_tiles = (uint32_t)n_tiles;
    p.totals = d.totals.as<uint4>(); p.ckpt = d.ckpt.as<uint4>();
    p.q = d.q.as<const uint8_t>(); p.t = d.t.as<const uint8_t>(); p.q_off = d.q_off.as<const uint64_t>();
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
// (more: per record what its MD text adds to the reasons below, dagcon_upload_cigar_md; nullptr: nothing)
CigarVerdict cigar_judge(const dagcon_cigar_batch *b, const RecordSource &src, const CigarScan &sc, const std::vector<const char *> *more = nullptr) {
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
                            : (uint64_t)b->pos[a] - 1u + nt > b->tlen[g] ? "target bases past tlen"
                            : more ? (*more)[a] : nullptr;
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
    UPLOAD(c, c->cg.rev, src.reverse(), sc.n); UPLOAD(c, c->cg.q_len, b->q_len, sc.n);
    sc.st.rev = c->cg.rev.as<const uint8_t>(); sc.st.q_len = c->cg.q_len.as<const uint32_t>();
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
    UPLOAD(c, d.rate_base, base);
    if ((r = cigar_strand(c, b, src, sc))) return r;
    ENSURE(c, d.tile_rate, (size_t)sc.p.n_tiles * 16); ENSURE(c, d.rate, (size_t)n * 16);
    DgCigarRate rt;
    rt.base = d.rate_base.as<const uint64_t>(); rt.tile_rate = d.tile_rate.as<uint4>(); rt.rate = d.rate.as<uint4>();
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
    std::vector<uint32_t> rec;                                     // the record each of them comes from (dagcon_site_reads::aln_src)
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
            pl.start.push_back(b->pos[a]); pl.off.push_back(pl.bytes); pl.len.push_back(sc.tot[a * 4]); pl.rec.push_back(a);
            pl.bytes += ((uint64_t)sc.tot[a * 4] + 15ull) & ~15ull;
        }
    }
    pl.beg[T] = pl.start.size();
    UPLOAD(c, c->cg.t_base, t_base);
    UPLOAD(c, c->cg.out_off, out_off);
    sc.p.t_base = c->cg.t_base.as<const uint64_t>(); sc.p.out_off = c->cg.out_off.as<const uint64_t>();
    pl.waves = pl.bytes ? sc.p.n_tiles : 0u;
    return DAGCON_OK;
}

int check_windows(Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    const uint32_t T = b->n_targets, W = wn->n_windows;
    if (int r = keep_check(c, true, W)) return r;                 // (dagcon_set_window_keep: before any launch)
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
    if (np) {
        UPLOAD(c, d.piece, piece);
        ENSURE(c, d.cut, (size_t)np * 16);
        cw.piece = d.piece.as<const uint4>(); cw.cut = d.cut.as<uint4>(); cw.n_pieces = np;
        hipLaunchKernelGGL(k_cigar_cut, dim3((np + 3u) / 4u), dim3(256), 0, c->stream, sc.p, cw);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, d2h(c, cut.data(), d.cut.p, (size_t)np * 16));
    }
    // the output plan: nothing the device said is used before it has been checked against the record's own sizes
    std::vector<uint64_t> pout((size_t)np);
    std::vector<uint32_t> wbegin((size_t)np), wpiece;
    pl.off.resize(np); pl.start.resize(np); pl.len.resize(np); pl.rec.resize(np);
    uint32_t cur = 0;
    for (uint32_t i = 0; i < np; i++) {
        const uint32_t a = piece[i * 4], w = piece[i * 4 + 3];
        const uint32_t ca = cut[i * 4], cb = cut[i * 4 + 1], ta = cut[i * 4 + 2], tb = cut[i * 4 + 3];
        const uint64_t ntile = sc.tile_begin[a + 1] - sc.tile_begin[a];
        if (ca > cb || cb > tot[a * 4] || ta > tb || tb >= ntile)
            return fail(c, DAGCON_ERR_INTERNAL, "k_cigar_cut: piece %u of record %u has columns [%u, %u), tiles [%u, %u] of %llu", i, a, ca, cb, ta, tb, (unsigned long long)ntile);
        while (cur < w) pl.beg[++cur] = i;
        pl.off[i] = pout[i] = pl.bytes; pl.rec[i] = a;
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
        UPLOAD(c, d.t_base, t_base);
        UPLOAD(c, d.wave_piece, wpiece);
        UPLOAD(c, d.wave_begin, wbegin);
        UPLOAD(c, d.piece_out, pout);
        sc.p.t_base = d.t_base.as<const uint64_t>();
        cw.wave_piece = d.wave_piece.as<const uint32_t>(); cw.wave_begin = d.wave_begin.as<const uint32_t>();
        cw.piece_out = d.piece_out.as<const uint64_t>(); cw.n_waves = (uint32_t)wpiece.size();
        pl.waves = cw.n_waves;
    }
    return DAGCON_OK;
}

// expand: the strings into d_q / d_t, a wave per tile (of a record, or of a piece), by the kernel of the source's kind
int cigar_expand(Ctx *c, const dagcon_cigar_batch *b, const RecordSource &src, CigarScan &sc, const CigarPlan &pl) {
    ENSURE(c, c->in.q, pl.bytes); ENSURE(c, c->in.t, pl.bytes);
    if (!pl.waves) return DAGCON_OK;
    DgCigarParams &p = sc.p;
    p.out_q = c->in.q.as<uint8_t>(); p.out_t = c->in.t.as<uint8_t>();
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
    const int r = upload_impl(ctx, &db, c->in.q.p, c->in.t.p, pl.pieces ? Intake::WINDOWS : Intake::RECORDS);   // (synchronises the stream: the caller's locals may go)
    if (r != DAGCON_OK) { (void)hipStreamSynchronize(c->stream); return r; }
    c->h_cig_bad = pl.bad;
    for (uint64_t &x : c->h_aln_src) x = pl.rec[x];                // (dagcon_set_site_reads: upload_impl left the index into pl's arrays)
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

// dagcon_set_edits: the batch the hand-over left is one whose edits the run is to report (latched, with its room, by
// upload_impl).  What only the intake knows: the place of each pipeline target's first base in cg.t (a window's: its
// target's, plus its begin)
int edits_arm(Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn) {
    const uint32_t T = c->T;
    c->h_ed_tbase.assign(T, 0);
    for (uint32_t t = 0; t < T; t++) c->h_ed_tbase[t] = wn ? b->t_off[wn->target[t]] + wn->begin[t] : b->t_off[t];
    UPLOAD(c, c->in.ed_tbase, c->h_ed_tbase);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DAGCON_OK;
}

// dagcon_set_window_phase: the batch the hand-over left is a windows upload whose labels the run is to join (latched, with
// its room, by upload_impl).  What only the intake knows: each alignment's record (4 bytes; h_aln_src holds it) and each
// window's target
int window_phase_arm(Ctx *c, const dagcon_windows *wn) {
    std::vector<uint32_t> rec(c->h_aln_src.size());
    for (size_t a = 0; a < rec.size(); a++) rec[a] = (uint32_t)c->h_aln_src[a];
    UPLOAD(c, c->in.wl_rec, rec);
    UPLOAD(c, c->in.wl_tgt, wn->target, (size_t)c->T);
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // (rec is a local)
    return DAGCON_OK;
}

// what follows the scan and the judgement of every record intake: rate, pick, plan, expand, hand-over
int records_finish(dagcon_ctx *ctx, Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn, const RecordSource &src, CigarScan &sc, const CigarVerdict &v) {
    int r;
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
    if (c->o_wl.batch && (r = window_phase_arm(c, wn))) return r;
    if ((r = keep_arm(c, nullptr))) return r;
    return c->o_ed.batch ? edits_arm(c, b, wn) : DAGCON_OK;
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
    return records_finish(ctx, c, b, wn, src, sc, cigar_judge(b, src, sc));
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
    if (wn && (r = keep_check(c, true, wn->n_windows))) return r;   // (before k_cs_scan: check_windows comes behind it)
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
    ENSURE(c, d.text, b->cs_bytes);
    ENSURE(c, d.totals, (size_t)n * 16); ENSURE(c, d.n_ops, (size_t)n * 4); ENSURE(c, cg.t, b->t_bytes); ENSURE(c, cg.q, q_bytes);
    if (b->cs_bytes && b->cs_blob) HIPCHK(c, hipMemcpyAsync(d.text.p, b->cs_blob, b->cs_bytes, hipMemcpyHostToDevice, s));
    if (b->t_bytes && b->t_blob) HIPCHK(c, hipMemcpyAsync(cg.t.p, b->t_blob, b->t_bytes, hipMemcpyHostToDevice, s));
    UPLOAD(c, d.cs_off, b->cs_off, n); UPLOAD(c, d.cs_len, b->cs_len, n);
    DgCsParams p;
    memset(&p, 0, sizeof p);
    CsDecoded cs;
    cs.why.assign((size_t)n, nullptr);
    cs.tot.assign((size_t)n * 4, 0);
    std::vector<uint32_t> nops((size_t)n, 0);
    if (n) {
        p.cs = d.text.as<const uint8_t>(); p.cs_off = d.cs_off.as<const uint64_t>(); p.cs_len = d.cs_len.as<const uint32_t>(); p.n = n;
        p.totals = d.totals.as<uint4>(); p.n_ops = d.n_ops.as<uint32_t>();
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
        UPLOAD(c, d.op_begin, opb);
        UPLOAD(c, d.t_base, t_base);
        UPLOAD(c, d.t_room, t_room);
        UPLOAD(c, d.q_off, q_off);
        UPLOAD(c, d.q_len, b->q_len, n);
        p.op_begin = d.op_begin.as<const uint64_t>(); p.ops = cg.ops.as<uint32_t>();
        p.t = cg.t.as<const uint8_t>(); p.t_base = d.t_base.as<const uint64_t>(); p.t_room = d.t_room.as<const uint32_t>();
        p.q_off = d.q_off.as<const uint64_t>(); p.q_len = d.q_len.as<const uint32_t>(); p.q = cg.q.as<uint8_t>();
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

const char *const MD_DISAGREE = "its target's MD tags disagree";

// SAM / BAM records with one MD:Z text each and no target bases (include/dagcon.h has the rule).  The targets are rebuilt
// in cg.t before the intake above runs on them: T is set to 'N', k_cigar_scan and k_md_scan size every record, the host
// judges them, k_md_write / k_md_check store and compare the letters of the conforming ones, k_md_fill / k_md_fill_check
// their read bases under M / = / X at positions no letter spells; a target whose tags disagree loses all its records.
int upload_md_records(dagcon_ctx *ctx, Ctx *c, const dagcon_cigar_batch *b, const dagcon_windows *wn, const dagcon_md_tags *md, bool packed) {
    int r;
    if (wn && (r = check_windows(c, b, wn))) return r;
    const uint32_t T = b->n_targets;
    uint32_t n = 0;
    if ((r = check_targets(c, T, b->tlen, b->t_off, b->rec_begin, nullptr, b->t_bytes, b->pos && b->q_off && b->q_len && b->op_begin, n, false))) return r;
    if (n && (!md || !md->md_off || !md->md_len)) return fail(c, DAGCON_ERR_INVALID_ARG, "md is NULL");
    for (uint32_t g = 0; g + 1 < T; g++)
        if (b->t_off[g] + b->tlen[g] > b->t_off[g + 1])
            return fail(c, DAGCON_ERR_INVALID_ARG, "targets %u and %u are not ascending and disjoint in the target blob", g, g + 1);
    for (uint32_t a = 0; a < n; a++) {
        if (md->md_off[a] > md->md_bytes || md->md_len[a] > md->md_bytes - md->md_off[a]) return fail(c, DAGCON_ERR_INVALID_ARG, "record %u runs past md_blob", a);
        if (md->md_len[a] && !md->md_blob) return fail(c, DAGCON_ERR_INVALID_ARG, "md_blob is NULL");
    }
    const uint64_t md_bytes = n ? md->md_bytes : 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    MdBufs &d = c->md;
    CigarBufs &cg = c->cg;
    ENSURE(c, cg.t, b->t_bytes); ENSURE(c, d.mark, b->t_bytes); ENSURE(c, d.conflict, T);
    if (b->t_bytes) {
        HIPCHK(c, hipMemsetAsync(cg.t.p, 'N', b->t_bytes, s));
        HIPCHK(c, hipMemsetAsync(d.mark.p, 0, b->t_bytes, s));
    }
    if (T) HIPCHK(c, hipMemsetAsync(d.conflict.p, 0, T, s));
    const RecordSource src = RecordSource::rebuilt(packed);
    CigarScan sc;
    if ((r = cigar_scan(c, b, src, sc))) return r;
    ENSURE(c, d.text, md_bytes); ENSURE(c, d.totals, (size_t)n * 16);
    std::vector<const char *> more((size_t)n, nullptr);
    if (!n) return records_finish(ctx, c, b, wn, src, sc, cigar_judge(b, src, sc));
    if (md_bytes && md->md_blob) HIPCHK(c, hipMemcpyAsync(d.text.p, md->md_blob, md_bytes, hipMemcpyHostToDevice, s));
    UPLOAD(c, d.md_off, md->md_off, n); UPLOAD(c, d.md_len, md->md_len, n);
    DgMdParams p;
    memset(&p, 0, sizeof p);
    p.md = d.text.as<const uint8_t>(); p.md_off = d.md_off.as<const uint64_t>(); p.md_len = d.md_len.as<const uint32_t>(); p.n = n;
    p.totals = d.totals.as<uint4>();
    const dim3 rec_grid((n + 3u) / 4u), rec_block(256);
    hipLaunchKernelGGL(k_md_scan, rec_grid, rec_block, 0, s, p);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> mtot((size_t)n * 4, 0);
    HIPCHK(c, d2h(c, mtot.data(), d.totals.p, (size_t)n * 16));
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t covered = mtot[(size_t)a * 4], fl = mtot[(size_t)a * 4 + 2];
        more[a] = (fl & DG_MD_BAD) ? "MD: the text is empty, does not begin and end with a number, holds a byte that is no digit, letter or ^, a ^ that follows no number or "
                                     "has no letter behind it, two letters in a row outside a deletion, more than 9 digits or a number of 2^28 or more"
                : (fl & DG_CG_OVERFLOW) ? "MD: the bases covered do not fit 32 bits"
                : covered != sc.tot[(size_t)a * 4 + 2] ? "MD: the text does not cover exactly the target bases the CIGAR consumes" : nullptr;
    }
    CigarVerdict v = cigar_judge(b, src, sc, &more);
    // the conforming records: where each begins in T, how far it goes, whose it is
    std::vector<uint64_t> t_base((size_t)n, DG_CG_SKIP);
    std::vector<uint32_t> nt((size_t)n, 0), tgt((size_t)n, 0);
    bool any = false;
    for (uint32_t g = 0; g < T; g++)
        for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) {
            tgt[a] = g;
            if (v.why[a]) continue;
            t_base[a] = b->t_off[g] + b->pos[a] - 1u; nt[a] = sc.tot[a * 4 + 2];
            any = true;
        }
    if (any) {
        UPLOAD(c, d.t_base, t_base); UPLOAD(c, d.nt, nt); UPLOAD(c, d.tgt, tgt);
        p.t = cg.t.as<uint8_t>(); p.mark = d.mark.as<uint8_t>(); p.t_base = d.t_base.as<const uint64_t>(); p.nt = d.nt.as<const uint32_t>();
        p.tgt = d.tgt.as<const uint32_t>(); p.conflict = d.conflict.as<uint8_t>();
        hipLaunchKernelGGL(k_md_write, rec_grid, rec_block, 0, s, p);
        hipLaunchKernelGGL(k_md_check, rec_grid, rec_block, 0, s, p);
        if (sc.p.n_tiles) {
            const dim3 grid(sc.p.n_tiles), block(64);
            if (packed) {
                hipLaunchKernelGGL(k_md_fill_packed, grid, block, 0, s, sc.p, p);
                hipLaunchKernelGGL(k_md_fill_check_packed, grid, block, 0, s, sc.p, p);
            } else {
                hipLaunchKernelGGL(k_md_fill, grid, block, 0, s, sc.p, p);
                hipLaunchKernelGGL(k_md_fill_check, grid, block, 0, s, sc.p, p);
            }
        }
        HIPCHK(c, hipGetLastError());
        std::vector<uint8_t> conflict(T, 0);
        HIPCHK(c, d2h(c, conflict.data(), d.conflict.p, T));
        bool again = false;
        for (uint32_t g = 0; g < T; g++)
            if (conflict[g]) {
                for (uint64_t a = b->rec_begin[g]; a < b->rec_begin[g + 1]; a++) more[a] = MD_DISAGREE;
                again = true;
            }
        if (again) v = cigar_judge(b, src, sc, &more);
    }
    return records_finish(ctx, c, b, wn, src, sc, v);
}
int upload_md(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn, const dagcon_md_tags *md, bool packed) {
    if (!ctx || !b) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = intake_reset(ctx);
    const int r = upload_md_records(ctx, c, b, wn, md, packed);
    if (r != DAGCON_OK) { (void)hipStreamSynchronize(c->stream); return r; }    // (the locals above may go)
    c->md_valid = true;                                            // (cg.t holds the targets until the next upload)
    c->md_bytes = b->t_bytes;
    return DAGCON_OK;
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

int dagcon_upload_cigar_md(dagcon_ctx *ctx, const dagcon_cigar_batch *b, const dagcon_windows *wn, const dagcon_md_tags *md, int packed) {
    return upload_md(ctx, b, wn, md, packed != 0);
}
int dagcon_consensus_cigar_md(dagcon_ctx *ctx, const dagcon_cigar_batch *batch, const dagcon_windows *windows, const dagcon_md_tags *md, int packed,
                              dagcon_results *results) {
    return upload_run_fetch(ctx, results, [&] { return dagcon_upload_cigar_md(ctx, batch, windows, md, packed); });
}
// the targets the last dagcon_upload_cigar_md rebuilt: copied from the device when first asked for
int dagcon_fetch_md_targets(dagcon_ctx *ctx, const char **t_blob, uint64_t *t_bytes) {
    if (!ctx || !t_blob || !t_bytes) return DAGCON_ERR_INVALID_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c->md_valid) return fail(c, DAGCON_ERR_STATE, "dagcon_fetch_md_targets: the last upload was not a dagcon_upload_cigar_md");
    if (!c->md_fetched) {
        c->h_md_t.resize(c->md_bytes + 1);
        HIPCHK(c, hipSetDevice(c->device));
        if (c->md_bytes) HIPCHK(c, d2h(c, c->h_md_t.data(), c->cg.t.p, c->md_bytes));
        c->h_md_t[c->md_bytes] = 0;
        c->md_fetched = true;
    }
    *t_blob = c->h_md_t.data(); *t_bytes = c->md_bytes;
    return DAGCON_OK;
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

// debugging aid (tools/bp_pieces.py): DAGCON_DUMP=<target>:<path> leaves that target's merged graph, its bestPath cuts,
// scores and choices in a file -- N, bp_max, pool words, then cuts row, records, pool, (score, final) pairs, best[]
static int dump_target(Ctx *c, const char *e) {
    const uint32_t t = (uint32_t)atoi(e);
    const char *path = strchr(e, ':');
    if (path && t < c->T) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint64_t nb = 0, pb = 0;
        uint32_t hdr[4] = {0, c->bp_max, 0, c->seg_max};
        (void)hipMemcpy(&nb, c->run.node_base.as<uint64_t>() + t, 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&pb, c->run.pool_base.as<uint64_t>() + t, 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&hdr[0], c->run.n_nodes.as<uint32_t>() + t, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&hdr[2], c->run.pool_top.as<uint32_t>() + t, 4, hipMemcpyDeviceToHost);
        std::vector<uint32_t> cuts(c->bp_max + 2), pool(hdr[2]), best(hdr[0]);
        std::vector<DgNode> nd(hdr[0]);
        std::vector<float> sc(2 * (size_t)hdr[0]);
        (void)hipMemcpy(cuts.data(), c->run.cuts_bp.as<uint32_t>() + (uint64_t)t * (c->bp_max + 2), cuts.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(nd.data(), c->arena.nodes.as<DgNode>() + nb, nd.size() * sizeof(DgNode), hipMemcpyDeviceToHost);
        (void)hipMemcpy(pool.data(), c->arena.pool.as<uint32_t>() + pb, pool.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(sc.data(), c->run.score.as<float>() + 2 * nb, sc.size() * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(best.data(), c->run.best.as<uint32_t>() + nb, best.size() * 4, hipMemcpyDeviceToHost);
        if (FILE *f = fopen(path + 1, "wb")) {
            fwrite(hdr, 4, 4, f); fwrite(cuts.data(), 4, cuts.size(), f); fwrite(nd.data(), sizeof(DgNode), nd.size(), f);
            fwrite(pool.data(), 4, pool.size(), f); fwrite(sc.data(), 4, sc.size(), f); fwrite(best.data(), 4, best.size(), f);
            // (partial-span batches: the merge's worklist -- (target, first vertex, last vertex) triples -- behind it)
            uint32_t nl = 0;
            std::vector<uint32_t> wl;
            if (c->gcuts && c->run.worklist.p) {
                (void)hipMemcpy(&nl, c->run.worklist.p, 4, hipMemcpyDeviceToHost);
                if (nl > c->worklist_cap) nl = c->worklist_cap;
                wl.resize(3 * (size_t)nl);
                if (nl) (void)hipMemcpy(wl.data(), c->run.worklist.as<uint32_t>() + 4, wl.size() * 4, hipMemcpyDeviceToHost);
            }
            fwrite(&nl, 4, 1, f);
            if (nl) fwrite(wl.data(), 4, wl.size(), f);
            // (... and, for tests/test_cut_limits.py, what the cuts were decided on: the target's sh_cnt row, its defer
            // row, pro_state[4t .. 4t + 3], its reads K, then rd_s, rd_e, rd_lead, rd_trail of each)
            if (c->gcuts && c->run.sh_cnt.p && c->run.defer.p && c->run.pro_state.p && c->run.rd.p) {
                const uint64_t ab = c->h_aln_begin[t];
                const uint32_t K = (uint32_t)(c->h_aln_begin[t + 1] - ab);
                std::vector<uint32_t> sh(2 + 2 * DG_SH_MAX), df(DG_DEFER_MAX + 1), ps(4), rd(4 * (size_t)K);
                (void)hipMemcpy(sh.data(), c->run.sh_cnt.as<uint32_t>() + (uint64_t)t * sh.size(), sh.size() * 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(df.data(), c->run.defer.as<uint32_t>() + (uint64_t)t * df.size(), df.size() * 4, hipMemcpyDeviceToHost);
                (void)hipMemcpy(ps.data(), c->run.pro_state.as<uint32_t>() + 4ull * t, 16, hipMemcpyDeviceToHost);
                for (int j = 0; j < 4 && K; j++)
                    (void)hipMemcpy(rd.data() + (size_t)j * K, c->run.rd.as<uint32_t>() + (uint64_t)j * c->A + ab, (size_t)K * 4, hipMemcpyDeviceToHost);
                fwrite(sh.data(), 4, sh.size(), f); fwrite(df.data(), 4, df.size(), f); fwrite(ps.data(), 4, 4, f);
                fwrite(&K, 4, 1, f);
                if (K) fwrite(rd.data(), 4, rd.size(), f);
            }
            fclose(f);
        }
    }
    return DAGCON_OK;
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
    HIPCHK(c, d2h(c, &nb, c->run.node_base.as<uint64_t>() + target, 8));
    HIPCHK(c, d2h(c, &pb, c->run.pool_base.as<uint64_t>() + target, 8));
    HIPCHK(c, d2h(c, &N, c->run.n_nodes.as<uint32_t>() + target, 4));
    HIPCHK(c, d2h(c, &psz, c->run.pool_top.as<uint32_t>() + target, 4));
    if (!c->h_tactive[target]) N = 0;
    std::vector<DgNode> nd(N);
    std::vector<uint32_t> pool(psz);
    std::vector<int32_t> cov(c->h_tlen[target] + 2, 0);
    c->g_weight.assign(N, 0); c->g_cov.assign(N, 0);
    if (N) {
        HIPCHK(c, d2h(c, nd.data(), c->arena.nodes.as<DgNode>() + nb, (size_t)N * sizeof(DgNode)));
        const uint32_t nbb = c->h_tlen[target] + 2;
        HIPCHK(c, d2h(c, cov.data(), c->run.cov.as<int32_t>() + c->h_bbv_base[target], (size_t)nbb * 4));
        if (psz) HIPCHK(c, d2h(c, pool.data(), c->arena.pool.as<uint32_t>() + pb, (size_t)psz * 4));
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
