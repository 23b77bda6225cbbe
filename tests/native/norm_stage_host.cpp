// norm_stage_host.cpp -- the normalize stage on the CPU, saying which route every chunk takes: for tests/test_norm_limits.py.
//
// The run loops (csrc/k_norm_run.hip.h) and the lane functions of the finish (csrc/k_norm_fin.hip.h) are the product's
// own text, with the real DG_NCH of 512; restated around them are k_norm_chunk's driver (first pass, RETRY pass for the
// chunks flagged 2, the `dirty` re-run loop, the ovf_top bump with its out-of-room test), k_norm_scan (offsets, swallowed
// and empty windows, the trim by whole chunks) and k_norm_finish2's copy and its pass and lane schedule.  The sizes of
// the scratch come from dg_tmp_main / dg_tmp_cap, which the host API calls too.
//
// Built by the test with the host compiler and -fsanitize=address,undefined.  Every buffer has exactly the size the
// device gives it: the blob, a lane's NW + 2 window row, a chunk's share of the scratch (up to where the next chunk's
// stretch begins, by the device's `src` arithmetic), a re-run's `need` columns, an alignment's 2 * len columns of the
// result.  A read or write past one stops the program.
//
// mode "stage" (argv[1] = stage, argv[2] = file): batches, one after the other:
//   uint32 n_alns, trim, emit_shift, shared, blob_bytes; blob_bytes of q; blob_bytes of t;
//   n_alns x { uint32 off, len, start, tlen }          (shared: the scratch lies at the columns in front in the batch)
// and prints, every line with the batch's number in front:
//   B tmp_main tmp_cap region ovf_top
//   W a c k0 route reruns next w tb span wraps asked        one per window; route: none p1 p2 slow:window slow:scratch;
//                                                            span / wraps: of the second pass, its largest e - i and how often
//                                                            its 512-column ring came round, (e - 1) / 512
//   A a slow lo hi start n_lb m branches n_ins n_del nonconf  branches: L whole chunk skipped from the left, l column by
//                                                            column, R / r the same from the right, x `o >= lo` false
//                                                            for a chunk the right end would else skip whole, m the two
//                                                            ends met; - none
//   F a c o w passes h nb carried ck_first ck_lane0           per chunk of the result: passes entered with a run in flight,
//                                                            checkpoints the x == 0 rule held back, on a later pass's lane 0
//   Q a <q>   T a <t>   C a pos:run ...   K a slot:column ...    the trimmed strings, matC runs, checkpoints ('.': none)
// mode "runs" (argv[2] = file of norm_run_host.cpp's cases): dg_norm_run<512> alone, per case
//   <case> need <n>      the widest look-up a plain restatement finds, over the alignment and every cold start in it
//   <case> whole <flags> <q> <t>  /  <case> chunks <flags> <q> <t>  wrapped <0|1>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

static uint32_t g_span = 0, g_emax = 0;
#define DG_NORM_RUN_PROBE(e, i) do { if ((e) - (i) > g_span) g_span = (e) - (i); if ((e) > g_emax) g_emax = (e); } while (0)
#include "../../pbdagcon_amd/csrc/k_norm_fin.hip.h"

static_assert(DG_NCH == 512u, "the model runs with the device's window");
#define NW_SMALL 64u
#define NW_BIG 512u
#define REDO 0xFFFFFFFFu

static void *exact_alloc(size_t bytes) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
    return p;
}
static void die(const char *what) { std::fprintf(stderr, "model: %s\n", what); std::exit(3); }

template <uint32_t NW>
static DgChunkRun run_one(const uint8_t *q, const uint8_t *t, uint32_t len, uint32_t k0, uint32_t k1, uint16_t *out) {
    uint16_t *win = static_cast<uint16_t *>(exact_alloc((NW + 2u) * sizeof(uint16_t)));      // the lane's LDS row
    std::memset(win, 0xEE, (NW + 2u) * sizeof(uint16_t));
    DgChunkRun r;
    if (NW == NW_SMALL) r = dg_norm_run_gc(q, t, len, k0, k1, win, out);
    else r = dg_norm_run<NW>(q, t, len, k0, k1, win, out);
    std::free(win);
    return r;
}

struct Aln { uint32_t off, len, start, tlen; };
enum Route { R_NONE, R_P1, R_P2, R_SLOW_WIN, R_SLOW_SCRATCH };
static const char *ROUTE[] = {"none", "p1", "p2", "slow:window", "slow:scratch"};
struct Chunk {
    uint32_t a = 0, c = 0, k0 = DG_CH_NONE, next = 0, w = 0, tb = 0, flag = 0, reruns = 0, span = 0, out = DG_CH_NONE, adv = 0;
    uint64_t src = 0, cap = 0, asked = 0;
    uint32_t wraps = 0;
    Route route = R_NONE;
};

struct Batch {
    uint32_t n = 0, trim = 0, emit_shift = 0, shared = 0, blob = 0;
    uint8_t *q = nullptr, *t = nullptr;
    std::vector<Aln> alns;
    std::vector<uint32_t> ch_base;
    std::vector<uint64_t> soff;
    std::vector<Chunk> ch;
    uint64_t tmp_main = 0, tmp_cap = 0, ovf_top = 0;
    uint16_t *tmp = nullptr;
};

// k_norm_chunk, one lane: RETRY false = the first pass (64-column window), true = the second (512)
template <uint32_t NW, bool RETRY>
static void chunk_lane(Batch &b, uint32_t g) {
    Chunk &x = b.ch[g];
    if (RETRY && x.flag != 2u) return;
    const Aln &al = b.alns[x.a];
    const uint32_t c = x.c, nwin = b.ch_base[x.a + 1] - b.ch_base[x.a], len = al.len;
    const uint8_t *q = b.q + al.off, *t = b.t + al.off;
    uint32_t flag = 0, cn = c + 1;
    DgChunkRun r;
    r.w = 0; r.tb = 0; r.dirty = false; r.overflow = false; r.badchar = false;
    const uint32_t k0 = dg_chunk_start(q, t, len, c);
    uint64_t src = 0, cap = 0;
    x.reruns = 0;
    if (k0 != DG_CH_NONE) {
        src = (2ull * (b.soff[x.a] + k0) + 8ull * g + 7ull) & ~7ull;
        // the chunk's share: up to the first stretch of the next window that has a start (the end of the main part if none)
        cap = b.tmp_main - src;
        for (uint32_t y = g + 1; y < b.ch.size(); y++) {
            const Aln &ay = b.alns[b.ch[y].a];
            const uint32_t ky = dg_chunk_start(b.q + ay.off, b.t + ay.off, ay.len, b.ch[y].c);
            if (ky != DG_CH_NONE) { cap = ((2ull * (b.soff[b.ch[y].a] + ky) + 8ull * y + 7ull) & ~7ull) - src; break; }
        }
        x.route = RETRY ? R_P2 : R_P1;
        for (;;) {
            uint32_t k1 = len;
            for (; cn < nwin; cn++) {
                const uint32_t s = dg_chunk_start(q, t, len, cn);
                if (s != DG_CH_NONE) { k1 = s; break; }
            }
            uint16_t *out = static_cast<uint16_t *>(exact_alloc(cap * sizeof(uint16_t)));
            g_span = 0; g_emax = 0;
            r = run_one<NW>(q, t, len, k0, k1, out);
            if (RETRY) { x.span = std::max(x.span, g_span); x.wraps = std::max(x.wraps, g_emax ? (g_emax - 1u) / NW_BIG : 0u); }
            if (!r.overflow) {
                if (src + r.w > b.tmp_cap) die("a run's columns leave the scratch");
                std::memcpy(b.tmp + src, out, (size_t)r.w * sizeof(uint16_t));
            }
            std::free(out);
            if (r.badchar) die("a byte outside 33..126");
            if (r.overflow) { flag = RETRY ? 1u : 2u; if (RETRY) x.route = R_SLOW_WIN; break; }
            if (!r.dirty) break;
            cn++;
            uint32_t k2 = len;
            for (uint32_t y = cn; y < nwin; y++) {
                const uint32_t s = dg_chunk_start(q, t, len, y);
                if (s != DG_CH_NONE) { k2 = s; break; }
            }
            const unsigned long long need = (2ull * (k2 - k0) + 15ull) & ~7ull;
            const unsigned long long o = b.ovf_top;
            b.ovf_top += need;                                             // atomicAdd(&p.st->ovf_top, need)
            x.asked += need;
            if (b.tmp_main + o + need > b.tmp_cap) { flag = 1; x.route = R_SLOW_SCRATCH; break; }      // out of room: slow path
            src = b.tmp_main + o; cap = need;
            x.reruns++;
        }
    }
    x.k0 = k0; x.next = cn; x.w = r.w; x.tb = r.tb; x.flag = flag; x.src = src; x.cap = cap;
}

struct AlnOut {
    bool slow = false, nonconf = false;
    uint32_t lo = 0, hi = 0, start = 0, n_lb = 0, m = 0, n_ins = 0, n_del = 0;
    std::string branches;
    std::vector<std::pair<uint32_t, uint32_t>> cells, ck;
    std::vector<uint16_t> norm;            // (2 * len + 7) & ~7 columns, as norm_off spaces the alignments
};

// k_norm_scan, one lane
static void scan_lane(Batch &b, uint32_t a, AlnOut &o) {
    const uint32_t g0 = b.ch_base[a], g1 = b.ch_base[a + 1];
    bool redo = false;
    uint32_t m = 0, tbt = 0;
    for (uint32_t g = g0; g < g1;) {
        if (b.ch[g].k0 == DG_CH_NONE) { b.ch[g].out = DG_CH_NONE; g++; continue; }
        redo |= b.ch[g].flag != 0;
        b.ch[g].out = m; b.ch[g].adv = tbt;
        m += b.ch[g].w; tbt += b.ch[g].tb;
        uint32_t nx = g0 + b.ch[g].next;
        if (nx > g1) nx = g1;
        for (uint32_t x = g + 1; x < nx; x++) b.ch[x].out = DG_CH_NONE;
        g = nx;
    }
    o.m = m;
    if (redo) { o.slow = true; o.hi = REDO; return; }
    const uint32_t trim = b.trim;
    bool L = false, l = false, R = false, r = false, xf = false;
    uint32_t lbases = 0, rbases = 0, lo = 0, hi = m;
    for (uint32_t g = g0; g < g1 && lbases < trim && lo < m; g++) {
        if (b.ch[g].out == DG_CH_NONE) continue;
        const uint32_t w = b.ch[g].w, tb = b.ch[g].tb;
        if (lbases + tb < trim) { lo += w; lbases += tb; L = true; continue; }
        const uint16_t *src = b.tmp + b.ch[g].src;
        l = true;
        for (uint32_t x = 0; x < w && lbases < trim; x++) {
            if (DG_T(src[x]) != DG_GAP) lbases++;
            lo++;
        }
    }
    for (uint32_t g = g1; g > g0 && rbases < trim && hi > lo;) {
        g--;
        const uint32_t oo = b.ch[g].out;
        if (oo == DG_CH_NONE) continue;
        const uint32_t tb = b.ch[g].tb;
        if (!(oo >= lo) && rbases + tb < trim) xf = true;                  // the left end stopped inside a chunk the right end would skip whole
        if (oo >= lo && rbases + tb < trim) { hi = oo; rbases += tb; R = true; continue; }
        const uint16_t *src = b.tmp + b.ch[g].src;
        r = true;
        while (rbases < trim && hi > lo && hi > oo) {
            if (DG_T(src[--hi - oo]) != DG_GAP) rbases++;
        }
    }
    o.lo = lo; o.hi = hi; o.start = b.alns[a].start + lbases; o.n_lb = lbases;
    if (L) o.branches += 'L';
    if (l) o.branches += 'l';
    if (R) o.branches += 'R';
    if (r) o.branches += 'r';
    if (xf) o.branches += 'x';
    if (trim && hi == lo) o.branches += 'm';
    if (o.branches.empty()) o.branches = "-";
}

// dg_wave_seg_incl's network: DPP row shifts and row broadcasts, lanes without a source get 0
static void wave_seg_incl(uint32_t x[64]) {
    uint32_t s[64];
    for (int n = 1; n <= 8; n <<= 1) {
        for (int l = 0; l < 64; l++) s[l] = (l & 15) >= n ? x[l - n] : 0u;
        for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
    }
    for (int l = 0; l < 64; l++) s[l] = ((l >> 4) & 1) ? x[(l & ~15) - 1] : 0u;
    for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
    for (int l = 0; l < 64; l++) s[l] = (l >> 5) ? x[31] : 0u;
    for (int l = 0; l < 64; l++) x[l] = dg_seg_combine(s[l], x[l]);
}

struct FinOut { uint32_t passes = 0, h = 0, nb = 0, carried = 0, ck_first = 0, ck_lane0 = 0; };

// k_norm_finish2, one wave: the copy (head, funnelled pieces, tail) and the events, lanes in order
static FinOut finish_wave(const Batch &b, const Chunk &x, AlnOut &ao) {
    FinOut f;
    const Aln &al = b.alns[x.a];
    const uint32_t o = x.out, hi = ao.hi, lo = ao.lo, start = ao.start, lb = ao.n_lb, w = x.w, adv0 = x.adv;
    const uint16_t *src = b.tmp + x.src;
    const uint32_t nvec = (w + 7u) / 8u;
    if (8ull * nvec > x.cap) die("the finish reads pieces behind the chunk's share of the scratch");
    if ((size_t)o + w > ao.norm.size()) die("the finish writes behind the alignment's columns");
    uint16_t *dst = ao.norm.data() + o;
    const DgFinChunk u = dg_fin_chunk(start, al.tlen, b.emit_shift, o, lo);
    const uint32_t adv_init = adv0 > lb ? adv0 - lb : 0u;
    const uint32_t f0 = lo > o ? lo - o : 0u;
    const uint32_t f1 = hi > o ? (hi - o < w ? hi - o : w) : 0u;
    const bool any = f1 > f0;
    const uint32_t h0 = (8u - (o & 7u)) & 7u;
    const uint32_t h = h0 < w ? h0 : w;
    const uint32_t nb = (w - h) / 8u;
    f.h = h; f.nb = nb;
    for (uint32_t lane = 0; lane < 64; lane++) {
        if (lane < h) dst[lane] = src[lane];
        const uint32_t xx = h + 8u * nb + lane;
        if (lane < 8 && xx < w) dst[xx] = src[xx];
    }
    uint32_t adv_tile = adv_init, run_tile = 0;
    const bool writes = u.ok;
    for (uint32_t v0 = 0; v0 < nvec; v0 += 64u * DG_FIN_NP) {
        f.passes++;
        uint32_t advm[64], insm[64], nadv[64], seg[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t vl = v0 + DG_FIN_NP * lane;
            dg_u4 pc[DG_FIN_NP + 1u];
            for (uint32_t j = 0; j <= DG_FIN_NP; j++) {
                const uint32_t v = vl + j < nvec ? vl + j : nvec - 1u;
                uint32_t wd[4];
                std::memcpy(wd, src + 8u * v, 16);
                pc[j] = DG_MAKE_U4(wd[0], wd[1], wd[2], wd[3]);
            }
            for (uint32_t j = 0; j < DG_FIN_NP; j++)
                if (vl + j < nb) {
                    // dg_funnel_cols(pc[j], pc[j + 1], h): 8 columns starting h columns into the two pieces
                    uint16_t two[16];
                    std::memcpy(two, &pc[j], 16); std::memcpy(two + 8, &pc[j + 1u], 16);
                    std::memcpy(dst + h + 8u * (vl + j), two + h, 16);
                }
            uint32_t am = 0, im = 0, dm = 0;
            for (uint32_t j = 0; j < DG_FIN_NP; j++) {
                const DgFinMasks mk = dg_fin_piece(pc[j]);
                am |= mk.advm << (8u * j); im |= mk.insm << (8u * j); dm |= mk.delm << (8u * j);
            }
            const uint32_t win = dg_fin_window(8u * vl, f0, f1);
            am &= win; im &= win; dm &= win;
            advm[lane] = am; insm[lane] = im; nadv[lane] = (uint32_t)__builtin_popcount(am);
            if (any && 8u * v0 < f1) { ao.n_ins += (uint32_t)__builtin_popcount(im); ao.n_del += (uint32_t)__builtin_popcount(dm); }
            seg[lane] = dg_seg_pack(am, im);
        }
        if (!any || 8u * v0 >= f1) continue;
        if (v0 && run_tile) f.carried++;
        wave_seg_incl(seg);
        uint32_t adv_rel = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t seg_front = lane ? seg[lane - 1] : 0u;
            const uint32_t run_in = dg_seg_value(dg_seg_combine(run_tile, seg_front));
            const uint32_t adv_lane = adv_tile + adv_rel;
            const uint32_t c0 = 8u * (v0 + DG_FIN_NP * lane);
            if (writes) {
                uint32_t ends = dg_fin_run_ends(advm[lane], insm[lane], run_in);
                while (ends) {
                    const uint32_t k = (uint32_t)__builtin_ctz(ends);
                    ends &= ends - 1u;
                    const DgFinEvent e = dg_fin_event(u, advm[lane], insm[lane], run_in, adv_lane, k);
                    if (e.writes) ao.cells.push_back({e.pos, e.run});
                }
                for (uint32_t jc = dg_fin_first_ckpt(u, adv_lane); jc < nadv[lane]; jc += u.ck_mask + 1u) {
                    const uint32_t k = dg_fin_nth_adv(advm[lane], jc);
                    const DgFinEvent e = dg_fin_event(u, advm[lane], insm[lane], run_in, adv_lane, k);
                    uint32_t slot, value;
                    if (dg_fin_ckpt(u, e, c0 + k, slot, value)) {
                        ao.ck.push_back({slot, value});
                        if (v0 && lane == 0) f.ck_lane0++;
                    } else if (e.writes) f.ck_first++;
                }
            }
            adv_rel += nadv[lane];
        }
        run_tile = dg_seg_value(dg_seg_combine(run_tile, seg[63]));
        adv_tile += adv_rel;
    }
    {
        const uint32_t adv = adv_tile, run = run_tile;
        const bool conf = dg_fin_conf(u, adv);
        if (any && conf && ((start + adv) & u.ck_mask) == 0 && start + adv <= al.tlen + 1 && (o + f1 < hi || run))
            ao.ck.push_back({(start + adv) >> b.emit_shift, o + f1 - run});
        if (run && conf && start + adv <= al.tlen + 1) ao.cells.push_back({start + adv, run});
        if (any && !conf) ao.nonconf = true;
    }
    return f;
}

static void print_pairs(const char *tag, unsigned long bi, uint32_t a, std::vector<std::pair<uint32_t, uint32_t>> &v) {
    std::sort(v.begin(), v.end());
    std::printf("%lu %s %u", bi, tag, a);
    if (v.empty()) std::printf(" .");
    for (auto &p : v) std::printf(" %u:%u", p.first, p.second);
    std::printf("\n");
}

static int mode_stage(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    for (unsigned long bi = 0;; bi++) {
        uint32_t hdr[5];
        if (std::fread(hdr, 4, 5, f) != 5) break;
        Batch b;
        b.n = hdr[0]; b.trim = hdr[1]; b.emit_shift = hdr[2]; b.shared = hdr[3]; b.blob = hdr[4];
        b.q = static_cast<uint8_t *>(exact_alloc(b.blob)); b.t = static_cast<uint8_t *>(exact_alloc(b.blob));
        if (b.blob && (std::fread(b.q, 1, b.blob, f) != b.blob || std::fread(b.t, 1, b.blob, f) != b.blob)) die("short blob");
        b.alns.resize(b.n);
        if (b.n && std::fread(b.alns.data(), sizeof(Aln), b.n, f) != b.n) die("short table");
        // the host's tables (upload_impl): windows of DG_NCH input columns, the scratch offsets and sizes
        b.ch_base.assign(b.n + 1u, 0);
        uint64_t cols = 0;
        b.soff.resize(b.n);
        for (uint32_t a = 0; a < b.n; a++) {
            const Aln &al = b.alns[a];
            if ((uint64_t)al.off + al.len > b.blob) die("an alignment leaves the blob");
            const uint32_t nw = std::max<uint32_t>(1u, (al.len + DG_NCH - 1) / DG_NCH);
            b.ch_base[a] = (uint32_t)b.ch.size();
            for (uint32_t c = 0; c < nw; c++) { Chunk x; x.a = a; x.c = c; b.ch.push_back(x); }
            b.soff[a] = b.shared ? cols : al.off;
            cols += al.len;
        }
        b.ch_base[b.n] = (uint32_t)b.ch.size();
        b.tmp_main = dg_tmp_main(b.shared ? cols : b.blob, b.ch.size());
        b.tmp_cap = dg_tmp_cap(b.tmp_main);
        b.tmp = static_cast<uint16_t *>(exact_alloc(b.tmp_cap * sizeof(uint16_t)));
        std::memset(b.tmp, 0xEE, b.tmp_cap * sizeof(uint16_t));
        for (uint32_t g = 0; g < b.ch.size(); g++) chunk_lane<NW_SMALL, false>(b, g);
        for (uint32_t g = 0; g < b.ch.size(); g++) chunk_lane<NW_BIG, true>(b, g);
        std::printf("%lu B %llu %llu %llu %llu\n", bi, (unsigned long long)b.tmp_main, (unsigned long long)b.tmp_cap,
                    (unsigned long long)(b.tmp_cap - b.tmp_main), (unsigned long long)b.ovf_top);
        for (uint32_t a = 0; a < b.n; a++) {
            AlnOut ao;
            ao.norm.assign((2ull * b.alns[a].len + 7ull) & ~7ull, 0xEEEE);
            scan_lane(b, a, ao);
            for (uint32_t g = b.ch_base[a]; g < b.ch_base[a + 1]; g++) {
                const Chunk &x = b.ch[g];
                std::printf("%lu W %u %u %d %s %u %u %u %u %u %d %llu\n", bi, a, x.c, x.k0 == DG_CH_NONE ? -1 : (int)x.k0, ROUTE[x.route],
                            x.reruns, x.next, x.w, x.tb, x.span, (int)x.wraps, (unsigned long long)x.asked);
            }
            if (!ao.slow)
                for (uint32_t g = b.ch_base[a]; g < b.ch_base[a + 1]; g++) {
                    const Chunk &x = b.ch[g];
                    if (x.out == DG_CH_NONE) continue;
                    const FinOut fo = finish_wave(b, x, ao);
                    std::printf("%lu F %u %u %u %u %u %u %u %u %u %u\n", bi, a, x.c, x.out, x.w, fo.passes, fo.h, fo.nb, fo.carried,
                                fo.ck_first, fo.ck_lane0);
                }
            std::printf("%lu A %u %d %u %u %u %u %u %s %u %u %d\n", bi, a, (int)ao.slow, ao.lo, ao.hi, ao.start, ao.n_lb, ao.m,
                        ao.slow ? "-" : ao.branches.c_str(), ao.n_ins, ao.n_del, (int)ao.nonconf);
            if (!ao.slow) {
                std::string qs, ts;
                for (uint32_t x = ao.lo; x < ao.hi; x++) { qs.push_back((char)DG_Q(ao.norm[x])); ts.push_back((char)DG_T(ao.norm[x])); }
                std::printf("%lu Q %u %s\n%lu T %u %s\n", bi, a, qs.empty() ? "." : qs.c_str(), bi, a, ts.empty() ? "." : ts.c_str());
                print_pairs("C", bi, a, ao.cells);
                print_pairs("K", bi, a, ao.ck);
            }
        }
        std::free(b.q); std::free(b.t); std::free(b.tmp);
    }
    std::fclose(f);
    return 0;
}

// ---- mode "runs": dg_norm_run<512> alone ----
// normalizeGaps (Alignment.cpp:131-217) written down plainly on the columns from input column k0 on, to say how wide its
// look-ups are.  The second pass holds the columns [i, e) and no finished ones (they leave through a register), so a
// step at column g whose partner is p needs e - i = p - g + 1 (p = the end if there is no partner).  It refills while
// (e - i) + 32 <= 512; a step that waits has e - i below what it needs: with need <= 480 every refill is granted.
static uint32_t plain_need(const uint8_t *q0, const uint8_t *t0, uint32_t len, uint32_t k0) {
    std::vector<uint8_t> q, t;
    for (uint32_t k = k0; k < len; k++) {
        uint8_t a = q0[k], b = t0[k];
        if (a == '.') a = '-';
        if (b == '.') b = '-';
        if (a != b && a != '-' && b != '-') { q.push_back('-'); t.push_back(b); q.push_back(a); t.push_back('-'); }
        else { q.push_back(a); t.push_back(b); }
    }
    const size_t n = q.size();
    uint32_t need = 0;
    for (size_t g = 0; g + 1 < n; g++) {
        if (t[g] == '-') {
            size_t p = g + 1;
            while (p < n && t[p] == '-') p++;
            need = std::max<uint32_t>(need, (uint32_t)(p - g + 1));
            if (p < n && t[p] == q[g]) { t[g] = t[p]; t[p] = '-'; }
        }
        if (q[g] == '-') {
            size_t p = g + 1;
            while (p < n && q[p] == '-') p++;
            need = std::max<uint32_t>(need, (uint32_t)(p - g + 1));
            if (p < n && q[p] == t[g]) { q[g] = q[p]; q[p] = '-'; }
        }
    }
    return need;
}

struct Result { bool overflow = false, wrapped = false; std::string q, t; };
static void append(Result &res, const uint16_t *out, uint32_t w) {
    for (uint32_t x = 0; x < w; x++) { res.q.push_back((char)DG_Q(out[x])); res.t.push_back((char)DG_T(out[x])); }
}
static Result run_whole(const uint8_t *q, const uint8_t *t, uint32_t len) {
    Result res;
    const size_t cap = (2ull * len + 7ull) & ~7ull;
    uint16_t *out = static_cast<uint16_t *>(exact_alloc(cap * sizeof(uint16_t)));
    g_span = g_emax = 0;
    const DgChunkRun r = run_one<NW_BIG>(q, t, len, 0, len, out);
    res.overflow = r.overflow; res.wrapped = g_emax > NW_BIG;
    if (!r.overflow) append(res, out, r.w);
    std::free(out);
    return res;
}
static Result run_chunks(const uint8_t *q, const uint8_t *t, uint32_t len) {
    Result res;
    const uint32_t nwin = len ? (len + DG_NCH - 1u) / DG_NCH : 1u;
    std::vector<uint32_t> k0s(nwin), next(nwin);
    std::vector<std::vector<uint16_t>> outs(nwin);
    for (uint32_t c = 0; c < nwin; c++) {
        const uint32_t k0 = dg_chunk_start(q, t, len, c);
        k0s[c] = k0; next[c] = c + 1;
        if (k0 == DG_CH_NONE) continue;
        uint32_t cn = c + 1;
        for (;;) {
            uint32_t k1 = len;
            for (; cn < nwin; cn++) {
                const uint32_t s = dg_chunk_start(q, t, len, cn);
                if (s != DG_CH_NONE) { k1 = s; break; }
            }
            const size_t cap = (2ull * (k1 - k0) + 7ull) & ~7ull;
            uint16_t *out = static_cast<uint16_t *>(exact_alloc(cap * sizeof(uint16_t)));
            g_span = g_emax = 0;
            const DgChunkRun r = run_one<NW_BIG>(q, t, len, k0, k1, out);
            res.wrapped |= g_emax > NW_BIG;
            if (r.overflow) { res.overflow = true; std::free(out); break; }
            outs[c].assign(out, out + r.w);
            std::free(out);
            if (!r.dirty) break;
            cn++;
        }
        next[c] = cn;
        if (res.overflow) return res;
    }
    for (uint32_t c = 0; c < nwin;) {
        if (k0s[c] == DG_CH_NONE) { c++; continue; }
        append(res, outs[c].data(), (uint32_t)outs[c].size());
        c = next[c] < nwin ? next[c] : nwin;
    }
    return res;
}
static void print_run(size_t idx, const char *mode, const Result &r) {
    std::printf("%zu %s %s %s %s %d\n", idx, mode, r.overflow ? "o" : "-", r.overflow || r.q.empty() ? "." : r.q.c_str(),
                r.overflow || r.t.empty() ? "." : r.t.c_str(), (int)r.wrapped);
}

static int mode_runs(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    for (size_t idx = 0;; idx++) {
        uint32_t hdr[2];
        if (std::fread(hdr, sizeof(uint32_t), 2, f) != 2) break;
        const uint32_t len = hdr[0], phase = hdr[1] & 15u;
        uint8_t *qbuf = static_cast<uint8_t *>(exact_alloc((size_t)phase + len));
        uint8_t *tbuf = static_cast<uint8_t *>(exact_alloc((size_t)phase + len));
        std::memset(qbuf, 'N', phase); std::memset(tbuf, 'N', phase);
        if (len && (std::fread(qbuf + phase, 1, len, f) != len || std::fread(tbuf + phase, 1, len, f) != len)) die("short case");
        const uint8_t *q = qbuf + phase, *t = tbuf + phase;
        uint32_t need = plain_need(q, t, len, 0);
        const uint32_t nwin = len ? (len + DG_NCH - 1u) / DG_NCH : 1u;
        for (uint32_t c = 1; c < nwin; c++) {
            const uint32_t k0 = dg_chunk_start(q, t, len, c);
            if (k0 != DG_CH_NONE) need = std::max(need, plain_need(q, t, len, k0));
        }
        std::printf("%zu need %u\n", idx, need);
        print_run(idx, "whole", run_whole(q, t, len));
        print_run(idx, "chunks", run_chunks(q, t, len));
        std::free(qbuf); std::free(tbuf);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "stage")) return mode_stage(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "runs")) return mode_runs(argv[2]);
    std::fprintf(stderr, "usage: norm_stage_host stage|runs FILE\n");
    return 2;
}
