// api_align.hip.h -- in front of the pipeline: dagcon_align, dagcon_align_panels, dagcon_place, dagcon_consensus_pre
// (one translation unit with dagcon_api.hip, which includes it once).
extern "C" {

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

// the -a stage on the device: aligned strings left in c->al.qaln / taln at out_off[a], their lengths in aln_len (host),
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
    AlignBufs &d = c->al;
    ENSURE(c, d.qaln, out_bytes); ENSURE(c, d.taln, out_bytes); ENSURE(c, d.len, (size_t)n * 4);
    ENSURE(c, d.dir_off, (size_t)n * 8);
    if (local) ENSURE(c, d.ends, (size_t)n * 16);
    hipStream_t s = c->stream;
    UPLOAD(c, d.q, q_blob, q_bytes); UPLOAD(c, d.t, t_blob, t_bytes);
    UPLOAD(c, d.q_off, q_off, n); UPLOAD(c, d.t_off, t_off, n); UPLOAD(c, d.q_len, q_len, n); UPLOAD(c, d.t_len, t_len, n);
    UPLOAD(c, d.out_off, out_off, n);
    // Two passes (k_align.hip.h): every pair in the narrow band first; the pairs whose path came near an edge of it
    // (DG_AL_RETRY) again in the full band.  Inside a pass: groups of as many pairs as fit the direction budget
    // (one wave per pair and ~1 us per row: what counts is how many pairs are in flight; but a hipMalloc of tens
    // of GB takes seconds on this platform, so 32 GB at most, a quarter of the free memory), and inside a group
    // one launch per kernel instance (cells per lane).
    uint64_t budget_rows = (6ull << 30) / 256ull;
    {
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) {
            const uint64_t have = (uint64_t)mfree + (uint64_t)d.dirs.cap;      // (the buffer of the last call is ours to reuse)
            budget_rows = std::min<uint64_t>(16ull << 30, std::max<uint64_t>(1ull << 30, have / 4)) / 256ull;
        }
    }
    if (const char *e = getenv("DAGCON_ALIGN_GB")) { const long long v = atoll(e); if (v >= 1 && v <= 200) budget_rows = ((uint64_t)v << 30) / 256ull; }
    if (const char *e = getenv("DAGCON_ALIGN_ROWS")) { const long long v = atoll(e); if (v >= 1) budget_rows = (uint64_t)v; }   // test knob
    const bool t_dbg = getenv("DAGCON_ALIGN_TIMING") != nullptr;
    if (t_dbg) HIPCHK(c, hipStreamSynchronize(s));
    double t_grp = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    ENSURE(c, d.idx, (size_t)n * 4); ENSURE(c, d.halfw, (size_t)n * 4);
    std::vector<uint32_t> todo(n), halfw(n), order(n);
    for (uint32_t a = 0; a < n; a++) todo[a] = a;
    DgAlignParams ap;
    ap.q = d.q.as<const uint8_t>(); ap.t = d.t.as<const uint8_t>();
    ap.q_off = d.q_off.as<const uint64_t>(); ap.t_off = d.t_off.as<const uint64_t>();
    ap.q_len = d.q_len.as<const uint32_t>(); ap.t_len = d.t_len.as<const uint32_t>();
    ap.out_off = d.out_off.as<const uint64_t>(); ap.qaln = d.qaln.as<uint8_t>(); ap.taln = d.taln.as<uint8_t>();
    ap.aln_len = d.len.as<uint32_t>(); ap.dir_off = d.dir_off.as<const uint64_t>(); ap.halfw = d.halfw.as<const uint32_t>();
    ap.ends = local ? d.ends.as<uint32_t>() : nullptr;
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
            ENSURE(c, d.dirs, rows * 256ull);
            ap.dirs = d.dirs.as<uint32_t>();
            HIPCHK(c, hipMemcpyAsync(d.dir_off.p, dir_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipMemcpyAsync(d.idx.as<uint32_t>() + first, ad.data() + first, cnt * 4, hipMemcpyHostToDevice, s));
            ap.idx = d.idx.as<const uint32_t>() + first; ap.n = (uint32_t)cnt; ap.first_pass = 1u;
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
            HIPCHK(c, d2h(c, aln_len, d.len.p, (size_t)n * 4));
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
        HIPCHK(c, hipMemcpyAsync(d.halfw.p, halfw.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
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
            ENSURE(c, d.dirs, rows * 256ull);
            ap.dirs = d.dirs.as<uint32_t>();
            HIPCHK(c, hipMemcpyAsync(d.dir_off.p, dir_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
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
                    HIPCHK(c, hipMemcpyAsync(d.idx.as<uint32_t>() + first + k0, order.data() + first + k0, (size_t)nk * 4, hipMemcpyHostToDevice, s));
                    ap.idx = d.idx.as<const uint32_t>() + first + k0; ap.n = nk; ap.first_pass = fin ? 0u : 1u;
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
            HIPCHK(c, d2h(c, aln_len, d.len.p, (size_t)n * 4));
            std::vector<uint32_t> again;
            for (uint32_t a : todo) if (aln_len[a] == DG_AL_RETRY) again.push_back(a);
            if (t_dbg) fprintf(stderr, "dagcon_align: %zu of %u pairs go to the full band\n", again.size(), n);
            todo.swap(again);
        }
    }
    HIPCHK(c, d2h(c, aln_len, d.len.p, (size_t)n * 4));
    uint32_t dropped = 0;
    for (uint32_t a = 0; a < n; a++) {
        if ((uint64_t)aln_len[a] > (uint64_t)q_len[a] + t_len[a]) return fail(c, DAGCON_ERR_INTERNAL, "pair %u: alignment longer than its room", a);
        // the band could not connect the corners (sequences of very different lengths, indels beyond the widest band):
        // length 0, and the record then falls to the min_len filter -- the reference's SDPAlign always returns something
        dropped += aln_len[a] == 0 && (q_len[a] || t_len[a]);
    }
    c->h_ends.resize((size_t)n * 4);
    if (local) HIPCHK(c, d2h(c, c->h_ends.data(), d.ends.p, (size_t)n * 16));    // (16 B a pair; the strings stay)
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
    HIPCHK(c, d2h(c, qaln, c->al.qaln.p, out_bytes));
    HIPCHK(c, d2h(c, taln, c->al.taln.p, out_bytes));
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
    PanelBufs &d = c->pn;
    hipStream_t s = c->stream;
    ENSURE(c, d.len, (size_t)n * 4); ENSURE(c, d.qaln, out_bytes); ENSURE(c, d.taln, out_bytes);
    HIPCHK(c, hipMemsetAsync(d.len.p, 0, (size_t)n * 4, s));
    if (!kept.empty()) {
        ENSURE(c, d.qscr, scr_bytes); ENSURE(c, d.tscr, scr_bytes); ENSURE(c, d.p_len, np * 4); ENSURE(c, d.p_dist, np * 4);
        ENSURE(c, d.idx, np * 4);
        UPLOAD(c, d.q, q_blob, q_bytes); UPLOAD(c, d.t, t_blob, t_bytes);
        UPLOAD(c, d.p_q_off, p_qoff); UPLOAD(c, d.p_t_off, p_toff); UPLOAD(c, d.p_q_len, panel_q_len, np); UPLOAD(c, d.p_t_len, panel_t_len, np);
        UPLOAD(c, d.scr_off, p_scr); UPLOAD(c, d.panel_begin, panel_begin, (size_t)n + 1); UPLOAD(c, d.out_off, out_off, n); UPLOAD(c, d.kept, kept);
        std::vector<uint32_t> order;
        order.reserve(np);
        for (const auto &v : cls) order.insert(order.end(), v.begin(), v.end());
        HIPCHK(c, hipMemcpyAsync(d.idx.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
        DgPanelParams pp;
        pp.q = d.q.as<const uint8_t>(); pp.t = d.t.as<const uint8_t>();
        pp.q_off = d.p_q_off.as<const uint64_t>(); pp.t_off = d.p_t_off.as<const uint64_t>();
        pp.q_len = d.p_q_len.as<const uint32_t>(); pp.t_len = d.p_t_len.as<const uint32_t>();
        pp.scr_off = d.scr_off.as<const uint64_t>(); pp.qscr = d.qscr.as<uint8_t>(); pp.tscr = d.tscr.as<uint8_t>();
        pp.len = d.p_len.as<uint32_t>(); pp.dist = d.p_dist.as<int32_t>();
        size_t first = 0;
        for (int k = 0; k < 9; k++) {
            if (cls[k].empty()) continue;
            pp.idx = d.idx.as<const uint32_t>() + first; pp.n = (uint32_t)cls[k].size();
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
                           d.panel_begin.as<const uint64_t>(), d.scr_off.as<const uint64_t>(), d.p_t_len.as<const uint32_t>(), d.p_q_len.as<const uint32_t>(),
                           d.p_len.as<const uint32_t>(), d.qscr.as<const uint8_t>(), d.tscr.as<const uint8_t>(), d.out_off.as<const uint64_t>(),
                           d.qaln.as<uint8_t>(), d.taln.as<uint8_t>(), d.len.as<uint32_t>(), d.kept.as<const uint32_t>());
        HIPCHK(c, hipGetLastError());
        if (panel_dist) HIPCHK(c, d2h(c, panel_dist, d.p_dist.p, np * 4));
    }
    HIPCHK(c, d2h(c, aln_len, d.len.p, (size_t)n * 4));
    if (!kept.empty()) {
        HIPCHK(c, d2h(c, qaln, d.qaln.p, out_bytes));
        HIPCHK(c, d2h(c, taln, d.taln.p, out_bytes));
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

    PlaceBufs &d = c->pl;
    hipStream_t st = c->stream;
    ENSURE(c, d.slots, max_slots * sizeof(DgPlaceSlot));
    ENSURE(c, d.votes, (size_t)n_pairs * 8); ENSURE(c, d.span, (size_t)n_pairs * 8); ENSURE(c, d.strand, n_pairs);
    UPLOAD(c, d.blob, blob, bytes); UPLOAD(c, d.seq_off, seq_off, n_seq); UPLOAD(c, d.seq_len, seq_len, n_seq);
    UPLOAD(c, d.tab_seq, tab_seq); UPLOAD(c, d.tab_base, tab_base); UPLOAD(c, d.tab_mask, tab_mask);
    UPLOAD(c, d.pq, pq); UPLOAD(c, d.pt, pt); UPLOAD(c, d.ptab, ptab); UPLOAD(c, d.pid, pid);
    DgPlaceParams pp;
    pp.blob = d.blob.as<const uint8_t>(); pp.seq_off = d.seq_off.as<const uint64_t>(); pp.seq_len = d.seq_len.as<const uint32_t>();
    pp.slots = d.slots.as<DgPlaceSlot>();
    pp.votes_fwd = d.votes.as<uint32_t>(); pp.votes_rev = d.votes.as<uint32_t>() + n_pairs;
    pp.t0 = d.span.as<uint32_t>(); pp.t1 = d.span.as<uint32_t>() + n_pairs; pp.strand = d.strand.as<uint8_t>();
    pp.k = k; pp.max_occ = max_occ;
    for (const Group &gr : groups) {
        HIPCHK(c, hipMemsetAsync(d.slots.p, 0, gr.slots * sizeof(DgPlaceSlot), st));
        pp.tab_seq = d.tab_seq.as<const uint32_t>() + gr.tab0; pp.tab_base = d.tab_base.as<const uint64_t>() + gr.tab0;
        pp.tab_mask = d.tab_mask.as<const uint32_t>() + gr.tab0;
        pp.pq = d.pq.as<const uint32_t>() + gr.pair0; pp.pt = d.pt.as<const uint32_t>() + gr.pair0;
        pp.ptab = d.ptab.as<const uint32_t>() + gr.pair0; pp.pid = d.pid.as<const uint32_t>() + gr.pair0;
        hipLaunchKernelGGL(k_place_index, dim3(gr.tab1 - gr.tab0), dim3(DG_PLACE_THREADS), 0, st, pp);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_place_vote, dim3(gr.pair1 - gr.pair0), dim3(DG_PLACE_THREADS), (size_t)6 * gr.nb * 4, st, pp);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, d2h(c, votes_fwd, d.votes.p, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, votes_rev, d.votes.as<const uint32_t>() + n_pairs, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, t0, d.span.p, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, t1, d.span.as<const uint32_t>() + n_pairs, (size_t)n_pairs * 4));
    HIPCHK(c, d2h(c, strand, d.strand.p, n_pairs));
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
        const AlignBufs &d = c->al;                       // (align_device left room for n entries in idx)
        HIPCHK(c, hipMemcpyAsync(d.idx.p, rc_list.data(), rc_list.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_align_revcomp, dim3((uint32_t)rc_list.size()), dim3(64), 0, c->stream,
                           d.qaln.as<uint8_t>(), d.taln.as<uint8_t>(), d.out_off.as<const uint64_t>(),
                           d.len.as<const uint32_t>(), d.idx.as<const uint32_t>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));       // (rc_list is a local)
    }
    dagcon_batch db;
    memset(&db, 0, sizeof db);
    db.n_targets = T; db.tlen = b->tlen; db.aln_begin = b->rec_begin;
    db.aln_start = start.data(); db.aln_off = out_off.data(); db.aln_len = alen.data();
    db.blob_bytes = n ? out_bytes : 0;
    int r = upload_impl(ctx, &db, n ? c->al.qaln.p : nullptr, n ? c->al.taln.p : nullptr);
    if (r != DAGCON_OK) return r;
    if ((r = dagcon_run(ctx)) != DAGCON_OK) return r;
    return dagcon_fetch(ctx, results);
}

}  // extern "C"
