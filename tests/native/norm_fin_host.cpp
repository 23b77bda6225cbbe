// norm_fin_host.cpp -- csrc/k_norm_fin.hip.h on the CPU: what a lane of k_norm_finish2 derives from its bit masks,
// against the literal column loop of dg_finish_alignment (DG_FIN_COL, k_build.hip.h) with the rules at a chunk's edges.
// A program of its own (tests/test_norm_fin_host.py builds it with the host compiler and the sanitizers and runs it);
// it makes its cases itself and prints one line per set: "<set> cases <n> mismatches <m> ...".  Every comparison is exact.
//
//   pieces   all 4^8 class patterns of an 8-column piece x run_in x (window edges | positions around a checkpoint
//            multiple, the conformity limit and tlen + 1)
//   combine  dg_seg_combine: associativity on a small domain; the 64-lane scan network against the serial run length
//   chunks   whole chunks of 1 .. 2,300 columns through an emulation of the wave: lanes in order, the same functions
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../pbdagcon_amd/csrc/k_norm_fin.hip.h"

static const uint32_t E_SHIFTS[3] = {4, 7, 9};

// ---- what a chunk writes ----
struct Sink {
    std::vector<std::pair<uint32_t, uint32_t>> cells, ck;          // (position, run), (slot, column)
    bool wide = false, nonconf = false;
    uint32_t n_ins = 0, n_del = 0, adv = 0, run = 0;
    void clear() { cells.clear(); ck.clear(); wide = nonconf = false; n_ins = n_del = adv = run = 0; }
    void store_run(bool byte_cells, uint32_t pos, uint32_t r) {
        if (byte_cells && r > 255u) { wide = true; return; }        // dg_store_run: nothing stored, the flag raised
        cells.push_back({pos, r});
    }
    bool unique_sorted() {
        std::sort(cells.begin(), cells.end()); std::sort(ck.begin(), ck.end());
        for (size_t i = 1; i < cells.size(); i++) if (cells[i].first == cells[i - 1].first) return false;
        for (size_t i = 1; i < ck.size(); i++) if (ck[i].first == ck[i - 1].first) return false;
        return true;
    }
    bool same(const Sink &b) const {
        return cells == b.cells && ck == b.ck && wide == b.wide && nonconf == b.nonconf && n_ins == b.n_ins && n_del == b.n_del &&
               adv == b.adv && run == b.run;
    }
};

struct Chunk {
    std::vector<uint16_t> cols;    // w columns, then whatever lies behind them up to the end of the last 16-byte piece
    uint32_t w, o, lo, hi, start, tlen, emit_shift, adv_init;
    bool has_cm, graph, byte_cells;
};

// ---- the reference: DG_FIN_COL, literally, on the columns [xa, xb) of the chunk ----
static bool ref_conf(uint32_t start, uint32_t tlen, uint32_t A) { return start >= 1u && (A == 0u || (uint64_t)start - 1u + A <= (uint64_t)tlen); }

static void ref_cols(const Chunk &c, uint32_t xa, uint32_t xb, uint32_t &adv, uint32_t &run, Sink &s) {
    const uint32_t start = c.start, tlen = c.tlen, ck_mask = (1u << c.emit_shift) - 1u;
    for (uint32_t x = xa; x < xb; x++) {
        const uint8_t qb = DG_Q(c.cols[x]), tb = DG_T(c.cols[x]);
        if (qb == tb || qb == DG_GAP) {
            const bool conf = ref_conf(start, tlen, adv);
            if (c.has_cm && conf && ((start + adv) & ck_mask) == 0 && start + adv <= tlen + 1 && !(x == 0 && c.o > c.lo))
                s.ck.push_back({(start + adv) >> c.emit_shift, c.o + x - run});
            if (run) { if (c.has_cm && conf && start + adv <= tlen + 1) s.store_run(c.byte_cells, start + adv, run); run = 0; }
            adv++; s.n_del += (qb != tb);
        } else if (tb == DG_GAP) { s.n_ins++; run++; }
    }
}

static void window_of(const Chunk &c, uint32_t &f0, uint32_t &f1, bool &any) {
    f0 = c.lo > c.o ? c.lo - c.o : 0u;
    f1 = c.hi > c.o ? (c.hi - c.o < c.w ? c.hi - c.o : c.w) : 0u;
    any = f1 > f0;
}

// the end of a chunk: the column behind it is a match (the next chunk's first) or the end of the window
static void chunk_end(const Chunk &c, bool conf, uint32_t adv, uint32_t run, Sink &s) {
    uint32_t f0, f1; bool any;
    window_of(c, f0, f1, any);
    const uint32_t start = c.start, tlen = c.tlen, ck_mask = (1u << c.emit_shift) - 1u;
    if (any && c.has_cm && conf && ((start + adv) & ck_mask) == 0 && start + adv <= tlen + 1 && (c.o + f1 < c.hi || run))
        s.ck.push_back({(start + adv) >> c.emit_shift, c.o + f1 - run});
    if (run && c.has_cm && conf && start + adv <= tlen + 1) s.store_run(c.byte_cells, start + adv, run);
    if (c.graph && any && !conf) s.nonconf = true;
    s.adv = adv; s.run = run;
}

static void ref_chunk(const Chunk &c, Sink &s) {
    uint32_t f0, f1; bool any;
    window_of(c, f0, f1, any);
    uint32_t adv = c.adv_init, run = 0;
    if (any) ref_cols(c, f0, f1, adv, run, s);
    chunk_end(c, ref_conf(c.start, c.tlen, adv), adv, run, s);
}

// ---- the lane, as the kernel has it: run ends first, then checkpoints ----
static void lane_events(const DgFinChunk &u, uint32_t advm, uint32_t insm, uint32_t run_in, uint32_t adv_lane, uint32_t c0,
                        bool byte_cells, Sink &s) {
    uint32_t ends = dg_fin_run_ends(advm, insm, run_in);
    while (ends) {
        const uint32_t k = (uint32_t)__builtin_ctz(ends);
        ends &= ends - 1u;
        const DgFinEvent e = dg_fin_event(u, advm, insm, run_in, adv_lane, k);
        if (e.writes) s.store_run(byte_cells, e.pos, e.run);
    }
    const uint32_t nadv = (uint32_t)__builtin_popcount(advm);
    for (uint32_t jc = dg_fin_first_ckpt(u, adv_lane); jc < nadv; jc += u.ck_mask + 1u) {
        const uint32_t k = dg_fin_nth_adv(advm, jc);
        const DgFinEvent e = dg_fin_event(u, advm, insm, run_in, adv_lane, k);
        uint32_t slot, value;
        if (dg_fin_ckpt(u, e, c0 + k, slot, value)) s.ck.push_back({slot, value});
        if (u.ck_mask == 0xFFFFFFFFu) break;
    }
}

// ---- the scan network of dg_wave_seg_incl: DPP row shifts and row broadcasts, lanes without a source get 0 ----
static void wave_seg_incl(uint32_t x[64]) {
    uint32_t s[64];
    for (int n = 1; n <= 8; n <<= 1) {                                 // row_shr:n inside rows of 16 lanes
        for (int l = 0; l < 64; l++) s[l] = (l & 15) >= n ? x[l - n] : 0u;
        for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
    }
    for (int l = 0; l < 64; l++) s[l] = ((l >> 4) & 1) ? x[(l & ~15) - 1] : 0u;      // row_bcast:15 into rows 1 and 3
    for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
    for (int l = 0; l < 64; l++) s[l] = (l >> 5) ? x[31] : 0u;                        // row_bcast:31 into rows 2 and 3
    for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
}

static dg_u4 load_piece(const Chunk &c, uint32_t v, const uint32_t nvec) {
    if (v >= nvec) v = nvec - 1u;                                   // as the kernel: the last piece once more
    uint32_t wd[4];
    memcpy(wd, c.cols.data() + 8u * v, 16);
    return DG_MAKE_U4(wd[0], wd[1], wd[2], wd[3]);
}

// ---- the wave on a chunk: k_norm_finish2 without the copy ----
static void emul_chunk(const Chunk &c, Sink &s) {
    uint32_t f0, f1; bool any;
    window_of(c, f0, f1, any);
    const DgFinChunk u = dg_fin_chunk(c.start, c.tlen, c.emit_shift, c.o, c.lo);
    const uint32_t nvec = (c.w + 7u) / 8u;
    uint32_t adv_tile = c.adv_init, run_tile = 0;
    const bool writes = c.has_cm && u.ok;
    for (uint32_t v0 = 0; v0 < nvec; v0 += 64u * DG_FIN_NP) {
        if (!any || 8u * v0 >= f1) continue;
        uint32_t advm[64], insm[64], nadv[64], seg[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t vl = v0 + DG_FIN_NP * lane;
            uint32_t am = 0, im = 0, dm = 0;
            for (uint32_t j = 0; j < DG_FIN_NP; j++) {
                const DgFinMasks m = dg_fin_piece(load_piece(c, vl + j, nvec));
                am |= m.advm << (8u * j); im |= m.insm << (8u * j); dm |= m.delm << (8u * j);
            }
            const uint32_t win = dg_fin_window(8u * vl, f0, f1);
            am &= win; im &= win; dm &= win;
            advm[lane] = am; insm[lane] = im; nadv[lane] = (uint32_t)__builtin_popcount(am);
            s.n_ins += (uint32_t)__builtin_popcount(im); s.n_del += (uint32_t)__builtin_popcount(dm);
            seg[lane] = dg_seg_pack(am, im);
        }
        wave_seg_incl(seg);
        uint32_t adv_rel = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t seg_front = lane ? seg[lane - 1] : 0u;                   // wave_shr:1
            const uint32_t run_in = dg_seg_value(dg_seg_combine(run_tile, seg_front));
            if (writes) lane_events(u, advm[lane], insm[lane], run_in, adv_tile + adv_rel, 8u * (v0 + DG_FIN_NP * lane), c.byte_cells, s);
            adv_rel += nadv[lane];
        }
        run_tile = dg_seg_value(dg_seg_combine(run_tile, seg[63]));
        adv_tile += adv_rel;
    }
    chunk_end(c, dg_fin_conf(u, adv_tile), adv_tile, run_tile, s);
}

// ---- random numbers (the cases must not depend on the C library) ----
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static uint32_t rnd_in(uint32_t a, uint32_t b) { return a + rnd() % (b - a + 1u); }   // a .. b

static uint16_t column_of(uint32_t cls) {     // 0 match, 1 deletion, 2 insertion, 3 neither
    const uint8_t b = "ACGT"[rnd() & 3u];
    if (cls == 0) return DG_COL(b, b);
    if (cls == 1) return DG_COL(DG_GAP, b);
    if (cls == 2) return DG_COL(b, DG_GAP);
    return DG_COL(b, "ACGT"[((b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : 3) + 1 + (rnd() % 3u)) & 3u]);
}

static int report(const char *set, const Chunk &c, const Sink &a, const Sink &b, unsigned long id) {
    fprintf(stderr, "%s case %lu differs: w %u o %u lo %u hi %u start %u tlen %u shift %u adv_init %u cm %d graph %d byte %d\n"
            "  reference: %zu cells %zu ck wide %d nonconf %d ins %u del %u adv %u run %u\n"
            "  lanes:     %zu cells %zu ck wide %d nonconf %d ins %u del %u adv %u run %u\n",
            set, id, c.w, c.o, c.lo, c.hi, c.start, c.tlen, c.emit_shift, c.adv_init, c.has_cm, c.graph, c.byte_cells,
            a.cells.size(), a.ck.size(), a.wide, a.nonconf, a.n_ins, a.n_del, a.adv, a.run,
            b.cells.size(), b.ck.size(), b.wide, b.nonconf, b.n_ins, b.n_del, b.adv, b.run);
    return 1;
}

// ---- set 1: exhaustive 8-column pieces ----
struct Scene { uint32_t shift, start, adv_lane, tlen, o, lo; };

static std::vector<Scene> scenes() {
    std::vector<Scene> v;
    // start + adv_lane steps across a checkpoint multiple: 10 columns before it to 1 behind
    for (uint32_t shift : E_SHIFTS)
        for (uint32_t d = 0; d <= 11; d++) {
            const uint32_t M = 3u << shift;
            v.push_back({shift, 7u, M - 7u + 1u - d, 1u << 20, 64u, 0u});
        }
    // adv_lane steps across the conformity limit (= tlen + 1 - start, so across tlen + 1 as well)
    for (int e = -2; e <= 10; e++) v.push_back({4u, 5u, 100u, (uint32_t)(5 - 1 + 100 + e), 64u, 0u});
    v.push_back({4u, 0u, 16u, 1u << 20, 64u, 0u});              // start 0: never conforming
    v.push_back({4u, 16u, 0u, 1u << 20, 64u, 70u});             // a chunk's first column inside the window, o <= lo
    v.push_back({4u, 16u, 0u, 1u << 20, 64u, 10u});             // the same, o > lo: the chunk in front records it
    v.push_back({0u, 3u, 9u, 1u << 20, 64u, 10u});              // emit_shift 0: every position a checkpoint
    v.push_back({2u, 3u, 9u, 1u << 20, 64u, 10u});
    return v;
}

static int set_pieces() {
    static const uint32_t RUN_IN[5] = {0, 1, 3, 254, 255};
    const std::vector<Scene> sc = scenes();
    unsigned long n = 0, bad = 0;
    Chunk layouts[2][2];           // [the lane is the chunk's first or its sixth][the piece is the lane's lower or upper one]
    for (auto &row : layouts)
        for (Chunk &c : row) { c.cols.assign(96, 0); c.w = 96; c.has_cm = true; c.graph = true; c.adv_init = 0; }
    Sink ref, got;
    uint32_t cur_pat = 0xFFFFFFFFu;
    auto one = [&](uint32_t pat, uint32_t run_in, uint32_t f0, uint32_t f1, const Scene &z, bool upper, bool byte_cells) {
        // the piece as the lane's lower or upper 8 columns (the lane's other 8 are "neither" columns); the lane's first
        // column is chunk column 0 only in the scenes that test that rule (adv_lane 0), else 16 * (some lane)
        const uint32_t base = upper ? 8u : 0u;
        const uint32_t c0 = z.adv_lane == 0 ? 0u : 16u * 5u;
        if (pat != cur_pat) {
            cur_pat = pat;
            for (uint32_t first = 0; first < 2; first++)
                for (uint32_t up = 0; up < 2; up++) {
                    Chunk &l = layouts[first][up];
                    const uint32_t at = first ? 0u : 80u;
                    for (uint32_t k = 0; k < 16; k++) l.cols[at + k] = column_of(3);
                    for (uint32_t k = 0; k < 8; k++) l.cols[at + 8u * up + k] = column_of((pat >> (2 * k)) & 3u);
                }
        }
        Chunk &c = layouts[c0 == 0u][upper];
        c.start = z.start; c.tlen = z.tlen; c.emit_shift = z.shift; c.o = z.o; c.lo = z.lo; c.hi = z.o + 4096u; c.byte_cells = byte_cells;
        // reference: the literal loop over the piece's window columns, entered with (adv_lane, run_in)
        ref.clear(); got.clear();
        {
            uint32_t adv = z.adv_lane, run = run_in;
            ref_cols(c, c0 + base + f0, c0 + base + f1, adv, run, ref);
            ref.adv = adv; ref.run = run;
        }
        // the lane
        uint32_t am = 0, im = 0, dm = 0;
        for (uint32_t j = 0; j < 2; j++) {
            uint32_t wd[4];
            memcpy(wd, c.cols.data() + c0 + 8u * j, 16);
            const DgFinMasks m = dg_fin_piece(DG_MAKE_U4(wd[0], wd[1], wd[2], wd[3]));
            am |= m.advm << (8u * j); im |= m.insm << (8u * j); dm |= m.delm << (8u * j);
        }
        const uint32_t win = dg_fin_window(c0, c0 + base + f0, c0 + base + f1) & DG_FIN_ALL;
        am &= win; im &= win; dm &= win;
        const DgFinChunk u = dg_fin_chunk(c.start, c.tlen, c.emit_shift, c.o, c.lo);
        if (u.ok) lane_events(u, am, im, run_in, z.adv_lane, c0, byte_cells, got);
        got.n_ins = (uint32_t)__builtin_popcount(im); got.n_del = (uint32_t)__builtin_popcount(dm);
        got.adv = z.adv_lane + (uint32_t)__builtin_popcount(am);
        got.run = dg_seg_value(dg_seg_combine(run_in, dg_seg_pack(am, im)));
        n++;
        if (!got.unique_sorted() || !ref.unique_sorted() || !ref.same(got)) {
            if (bad++ < 5) {
                fprintf(stderr, "pattern %#x run_in %u window %u..%u upper %d adv_lane %u: ", pat, run_in, f0, f1, upper, z.adv_lane);
                report("pieces", c, ref, got, n);
            }
        }
    };
    if (DG_FIN_COLS < 16u) { fprintf(stderr, "set pieces needs two pieces a lane\n"); return 1; }
    for (uint32_t pat = 0; pat < 65536u; pat++)
        for (uint32_t ri = 0; ri < 5; ri++) {
            // every scene on the whole piece
            for (size_t z = 0; z < sc.size(); z++) one(pat, RUN_IN[ri], 0, 8, sc[z], ((pat ^ z) & 1u) != 0, ((pat >> 3) ^ z) & 1u);
            // every window edge, the scenes in turn
            uint32_t z = pat * 5u + ri;
            for (uint32_t f0 = 0; f0 <= 8; f0++)
                for (uint32_t f1 = f0; f1 <= 8; f1++, z++) one(pat, RUN_IN[ri], f0, f1, sc[z % sc.size()], (z / sc.size()) & 1u, (z >> 2) & 1u);
        }
    printf("pieces cases %lu mismatches %lu scenes %zu\n", n, bad, sc.size());
    return bad != 0;
}

// ---- set 2: the scan's operator ----
static int set_combine() {
    unsigned long n = 0, bad = 0;
    std::vector<uint32_t> dom;
    for (uint32_t f = 0; f < 2; f++)
        for (uint32_t v : {0u, 1u, 2u, 3u, 5u, 255u, 256u, 70000u}) dom.push_back((f ? DG_SEG_RESET : 0u) | v);
    for (uint32_t a : dom) {
        if (dg_seg_combine(0u, a) != a || dg_seg_combine(a, 0u) != a) bad++;          // 0 is the identity
        for (uint32_t b : dom)
            for (uint32_t c : dom) {
                n++;
                if (dg_seg_combine(dg_seg_combine(a, b), c) != dg_seg_combine(a, dg_seg_combine(b, c))) bad++;
            }
    }
    // the 64-lane network against the run length counted column by column
    unsigned long waves = 0;
    for (int trial = 0; trial < 20000; trial++) {
        uint32_t advm[64], insm[64], seg[64];
        const uint32_t p_adv = rnd() % 100u, p_ins = rnd() % 100u;                     // in percent, per trial
        for (int l = 0; l < 64; l++) {
            uint32_t am = 0, im = 0;
            for (uint32_t k = 0; k < DG_FIN_COLS; k++) {
                if (rnd() % 100u < p_adv) am |= 1u << k;
                else if (rnd() % 100u < p_ins) im |= 1u << k;
            }
            advm[l] = am; insm[l] = im; seg[l] = dg_seg_pack(am, im);
        }
        const uint32_t run_tile = (trial & 1) ? rnd() % 600u : 0u;
        wave_seg_incl(seg);
        uint32_t run = run_tile;
        for (int l = 0; l < 64; l++) {
            const uint32_t run_in = dg_seg_value(dg_seg_combine(run_tile, l ? seg[l - 1] : 0u));
            if (run_in != run) bad++;
            for (uint32_t k = 0; k < DG_FIN_COLS; k++) {
                if ((advm[l] >> k) & 1u) run = 0;
                else if ((insm[l] >> k) & 1u) run++;
            }
        }
        if (dg_seg_value(dg_seg_combine(run_tile, seg[63])) != run) bad++;
        waves++;
    }
    printf("combine cases %lu mismatches %lu waves %lu\n", n, bad, waves);
    return bad != 0;
}

// ---- set 3: whole chunks ----
static int set_chunks(unsigned long n_cases) {
    unsigned long bad = 0, multi_pass = 0, wide = 0, nonconf = 0, empty = 0, o_gt_lo = 0, trailing = 0, raw = 0, cells = 0, cks = 0,
                  edge_piece = 0, edge_pass = 0, edge_chunk = 0, trim_first = 0, trim_last = 0;
    unsigned o7 = 0;
    Sink ref, got;
    for (unsigned long id = 0; id < n_cases; id++) {
        Chunk c;
        const uint32_t kind = (uint32_t)(id % 16u);
        c.w = kind == 0 ? rnd_in(1, 40) : kind < 4 ? rnd_in(1, 2300) : kind < 8 ? rnd_in(1000, 2300) : rnd_in(400, 700);
        const uint32_t nvec = (c.w + 7u) / 8u;
        const uint32_t p_ins = rnd_in(5, 30), p_del = rnd_in(2, 15), p_ext = rnd_in(0, 70);
        const bool with_raw = (id % 5u) == 0;
        raw += with_raw;
        c.cols.resize(8u * nvec);
        for (uint32_t x = 0; x < c.w;) {
            const uint32_t r = rnd() % 100u;
            if (r < p_ins) {                                             // an insertion run
                uint32_t L = 1;
                while (rnd() % 100u < p_ext) L++;
                if (rnd() % 400u == 0) L = rnd_in(200, 300);             // across the 255 of a byte cell
                for (; L && x < c.w; L--) c.cols[x++] = column_of(2);
            } else if (r < p_ins + p_del) c.cols[x++] = column_of(1);
            else if (with_raw && r < p_ins + p_del + 4u) c.cols[x++] = column_of(3);
            else c.cols[x++] = column_of(0);
        }
        // a run of 1 .. 16 insertions that ends exactly on a piece edge, a lane edge, a pass edge or the chunk's edge
        if (id % 3u == 0) {
            const uint32_t L = rnd_in(1, 16), what = (uint32_t)((id / 3u) % 4u);
            uint32_t end = what == 0 ? 8u * rnd_in(1, nvec) : what == 1 ? 16u * rnd_in(1, (nvec + 1u) / 2u) : what == 2 ? 1024u : c.w;
            if (end <= c.w && end >= L) {
                for (uint32_t x = end - L; x < end; x++) c.cols[x] = column_of(2);
                if (end < c.w) c.cols[end] = column_of(0);
                if (end - L > 0) c.cols[end - L - 1u] = column_of(0);
                edge_piece += what == 0; edge_pass += what == 2; edge_chunk += what == 3;
            }
        }
        for (uint32_t x = c.w; x < 8u * nvec; x++) c.cols[x] = (uint16_t)rnd();          // behind the chunk: anything
        c.o = (uint32_t)(id % 8u) + 8u * rnd_in(0, 500);
        o7 |= 1u << (c.o & 7u);
        // the trimmed window: whole chunk inside / lo or hi in the first or last piece / anywhere / empty
        const uint32_t wk = (uint32_t)((id / 16u) % 8u);
        uint32_t f0 = 0, f1 = c.w;
        bool more_behind = rnd() & 1u;                                   // columns of the window behind the chunk
        if (wk == 1) { f0 = rnd_in(0, std::min(c.w, 8u)); trim_first++; }
        else if (wk == 2) { f1 = c.w - rnd_in(0, std::min(c.w, 8u)); more_behind = false; trim_last++; }
        else if (wk == 3) { f0 = rnd_in(0, c.w); f1 = rnd_in(f0, c.w); more_behind = false; }
        else if (wk == 4) { f0 = rnd_in(0, std::min(c.w, 8u)); f1 = rnd_in(f0, std::min(c.w, 8u)); more_behind = false; }
        else if (wk == 5) { f1 = c.w; f0 = c.w - rnd_in(0, std::min(c.w, 8u)); }
        c.lo = f0 ? c.o + f0 : (rnd() & 1u) ? c.o : rnd_in(0, c.o);
        c.hi = f1 < c.w || !more_behind ? c.o + f1 : c.o + c.w + rnd_in(1, 5000);
        if (wk == 6 && (id & 64u)) { c.lo = c.o + c.w + 3u; c.hi = c.lo + 10u; }         // the window behind the chunk
        if (wk == 6 && !(id & 64u)) { c.hi = rnd_in(0, c.o); c.lo = rnd_in(0, c.hi); }   // in front of it
        o_gt_lo += c.o > c.lo;
        c.emit_shift = (uint32_t[]){0u, 2u, 4u, 7u, 9u, 9u, 9u, 4u}[rnd() & 7u];
        c.adv_init = (rnd() & 3u) ? rnd_in(0, 30000) : 0u;
        c.start = (rnd() % 50u == 0) ? 0u : rnd_in(1, 3000);
        c.graph = (id % 11u) != 0;
        c.has_cm = c.graph && (id % 13u) != 0;
        c.byte_cells = (id & 1u) != 0;
        uint32_t nadv_all = 0;
        for (uint32_t x = 0; x < c.w; x++) { const uint8_t q = DG_Q(c.cols[x]), t = DG_T(c.cols[x]); nadv_all += (q == t || q == DG_GAP); }
        const uint32_t tk = rnd() % 4u;                                   // tlen: far away, or the limit inside the chunk
        c.tlen = !c.graph ? 0xFFFFFFFFu : tk ? c.start + c.adv_init + nadv_all + rnd_in(0, 4000)
                                             : (uint32_t)std::max<int64_t>(0, (int64_t)c.start + c.adv_init + (int64_t)rnd_in(0, nadv_all + 2u) - 2);
        ref.clear(); got.clear();
        ref_chunk(c, ref);
        emul_chunk(c, got);
        uint32_t g0, g1; bool any;
        window_of(c, g0, g1, any);
        multi_pass += 8u * nvec > 64u * DG_FIN_COLS; wide += ref.wide; nonconf += ref.nonconf; empty += !any;
        trailing += any && ref.run != 0 && c.o + g1 == c.hi;
        cells += ref.cells.size(); cks += ref.ck.size();
        if (!got.unique_sorted() || !ref.unique_sorted() || !ref.same(got)) {
            if (bad++ < 5) report("chunks", c, ref, got, id);
        }
    }
    printf("chunks cases %lu mismatches %lu multi_pass %lu wide %lu nonconf %lu empty %lu o_gt_lo %lu trailing %lu raw %lu cells %lu "
           "ckpts %lu edge_piece %lu edge_pass %lu edge_chunk %lu trim_first %lu trim_last %lu o_mod8 %#x\n",
           n_cases, bad, multi_pass, wide, nonconf, empty, o_gt_lo, trailing, raw, cells, cks, edge_piece, edge_pass, edge_chunk,
           trim_first, trim_last, o7);
    return bad != 0;
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "all";
    int rc = 0;
    if (!strcmp(what, "pieces") || !strcmp(what, "all")) rc |= set_pieces();
    if (!strcmp(what, "combine") || !strcmp(what, "all")) rc |= set_combine();
    if (!strcmp(what, "chunks") || !strcmp(what, "all")) rc |= set_chunks(argc > 2 ? strtoul(argv[2], nullptr, 10) : 20000ul);
    return rc;
}
