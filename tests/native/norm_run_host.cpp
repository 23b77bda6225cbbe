// norm_run_host.cpp -- the run loops of k_norm_chunk (csrc/k_norm_run.hip.h) on the CPU, for tests/test_norm_run_host.py.
//
// Built by the test with the host compiler, -fsanitize=address,undefined and -DDG_NCH=32 (chunk edges every 32 input
// columns).  Every buffer has exactly the size the kernel gives it, so a read or write past it stops the program.
//
// Input (argv[1], binary): per case  uint32 len, uint32 phase, len bytes of q, len bytes of t.  The strings are placed
// `phase` bytes behind a 16-byte boundary, as an alignment at offset `phase` of the device's string buffers is.
// Output (stdout), five lines a case:
//   <case> need <n>                    what the plain restatement below says the window has to span (see plain_need)
//   <case> gc whole <flags> <q> <t>    first-pass form (64-column window), the alignment as one chunk
//   <case> gc chunks <flags> <q> <t>   first-pass form, cut at dg_chunk_start's columns, with the kernel's re-run driver
//   <case> big whole / big chunks      the same with the second-pass form (512-column window)
// flags: 'o' overflow, 'b' a byte outside 33..126, '-' neither; <q> <t> are the output strings, '.' when empty or when
// a flag is set.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pbdagcon_amd/csrc/k_norm_run.hip.h"

static void *exact_alloc(size_t bytes) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
    return p;
}

struct Result { bool overflow = false, badchar = false; std::string q, t; };

template <bool GC>
static DgChunkRun run_one(const uint8_t *q, const uint8_t *t, uint32_t len, uint32_t k0, uint32_t k1, uint16_t *out) {
    constexpr uint32_t NW = GC ? 64u : 512u;
    uint16_t *win = static_cast<uint16_t *>(exact_alloc((NW + 2u) * sizeof(uint16_t)));      // the lane's LDS row
    std::memset(win, 0, (NW + 2u) * sizeof(uint16_t));
    DgChunkRun r;
    if (GC) r = dg_norm_run_gc(q, t, len, k0, k1, win, out);
    else r = dg_norm_run<NW>(q, t, len, k0, k1, win, out);
    std::free(win);
    return r;
}

static void append(Result &res, const uint16_t *out, uint32_t w) {
    for (uint32_t x = 0; x < w; x++) { res.q.push_back((char)DG_Q(out[x])); res.t.push_back((char)DG_T(out[x])); }
}

// the alignment as one chunk [0, len)
template <bool GC>
static Result run_whole(const uint8_t *q, const uint8_t *t, uint32_t len) {
    Result res;
    const size_t cap = (2ull * len + 7ull) & ~7ull;
    uint16_t *out = static_cast<uint16_t *>(exact_alloc(cap * sizeof(uint16_t)));
    const DgChunkRun r = run_one<GC>(q, t, len, 0, len, out);
    res.overflow = r.overflow; res.badchar = r.badchar;
    if (!r.overflow) append(res, out, r.w);
    std::free(out);
    return res;
}

// k_norm_chunk's driver and k_norm_scan's walk over the chunks, restated: every window of DG_NCH input columns that
// has a start column runs cold from there to the next start; a run that reports `dirty` is done again with the next
// chunk taken in, and the chunks it swallowed are skipped when the pieces are put together.
template <bool GC>
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
            const DgChunkRun r = run_one<GC>(q, t, len, k0, k1, out);
            res.badchar |= r.badchar;
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

// normalizeGaps (Alignment.cpp:131-217) written down plainly, to say how long a stretch of columns its look-ups span.
// A push at column g looks for its partner p, the next column with a base in that string (the end of the alignment
// if there is none).  The first pass holds, in front of g, the final columns that still wait for their group of 8
// output columns: at most 7 of them besides (-, -) columns, so never more than the columns behind the 8th earlier
// column that is no (-, -).  With lo the column behind that one, `need` is the largest p - lo over all look-ups, and
// the largest g + 1 - lo over all columns g (the waiting columns alone, with the (-, -) columns among them).  The
// first pass refills as long as its window spans at most 32 columns, so an alignment with need <= 32 never makes it
// report `overflow`, as one chunk or cut into chunks.
static uint32_t plain_need(const uint8_t *q0, const uint8_t *t0, uint32_t len) {
    std::vector<uint8_t> q, t;
    for (uint32_t k = 0; k < len; k++) {
        uint8_t a = q0[k], b = t0[k];
        if (a == '.') a = '-';
        if (b == '.') b = '-';
        if (a != b && a != '-' && b != '-') { q.push_back('-'); t.push_back(b); q.push_back(a); t.push_back('-'); }
        else { q.push_back(a); t.push_back(b); }
    }
    const size_t n = q.size();
    std::vector<size_t> kept;            // positions of the final columns that are no (-, -), in order
    uint32_t need = 0;
    for (size_t g = 0; g + 1 < n; g++) {
        const size_t lo = kept.size() >= 8 ? kept[kept.size() - 8] + 1 : 0;
        if (g + 1 - lo > need) need = (uint32_t)(g + 1 - lo);        // the waiting columns themselves, with their (-, -)
        if (t[g] == '-') {
            size_t p = g + 1;
            while (p < n && t[p] == '-') p++;
            if (p - lo > need) need = (uint32_t)(p - lo);
            if (p < n && t[p] == q[g]) { t[g] = t[p]; t[p] = '-'; }
        }
        if (q[g] == '-') {
            size_t p = g + 1;
            while (p < n && q[p] == '-') p++;
            if (p - lo > need) need = (uint32_t)(p - lo);
            if (p < n && q[p] == t[g]) { q[g] = q[p]; q[p] = '-'; }
        }
        if (q[g] != '-' || t[g] != '-') kept.push_back(g);
    }
    return need;
}

static void print(size_t idx, const char *form, const char *mode, const Result &r) {
    const bool flagged = r.overflow || r.badchar;
    std::printf("%zu %s %s %s%s %s %s\n", idx, form, mode, r.overflow ? "o" : "", r.badchar ? "b" : (r.overflow ? "" : "-"),
                flagged || r.q.empty() ? "." : r.q.c_str(), flagged || r.t.empty() ? "." : r.t.c_str());
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: norm_run_host CASES\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    size_t idx = 0;
    for (;; idx++) {
        uint32_t hdr[2];
        if (std::fread(hdr, sizeof(uint32_t), 2, f) != 2) break;
        const uint32_t len = hdr[0], phase = hdr[1] & 15u;
        uint8_t *qbuf = static_cast<uint8_t *>(exact_alloc((size_t)phase + len));
        uint8_t *tbuf = static_cast<uint8_t *>(exact_alloc((size_t)phase + len));
        std::memset(qbuf, 'N', phase); std::memset(tbuf, 'N', phase);
        if (len && (std::fread(qbuf + phase, 1, len, f) != len || std::fread(tbuf + phase, 1, len, f) != len)) {
            std::fprintf(stderr, "case %zu: short read\n", idx);
            return 2;
        }
        const uint8_t *q = qbuf + phase, *t = tbuf + phase;
        std::printf("%zu need %u\n", idx, plain_need(q, t, len));
        print(idx, "gc", "whole", run_whole<true>(q, t, len));
        print(idx, "gc", "chunks", run_chunks<true>(q, t, len));
        print(idx, "big", "whole", run_whole<false>(q, t, len));
        print(idx, "big", "chunks", run_chunks<false>(q, t, len));
        std::free(qbuf); std::free(tbuf);
    }
    std::fclose(f);
    return 0;
}
