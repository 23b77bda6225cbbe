// k_pileup.hip.h -- what the alignments show at every target position (dagcon_set_pileup; include/dagcon.h has the rule).
// Everything read here is resident after a run: the normalised, trimmed columns the graph was built from (norm) and
// where each alignment's lie (norm_off, n_lo, n_hi, n_start, aln_tgt).
//
//   k_pile_count        a wave per alignment: walks its columns 64 a step (k_walk.hip.h: the alignment's header, the
//                       step, the target coordinate of a column).  A column with a
//                       target base adds 1 to one of the six counters of its position; an inserted column whose
//                       neighbour in front holds a target base (bit lane - 1 of the same ballot, bit 63 of the step
//                       before for lane 0) begins a run and adds 1 to INS of that neighbour's position.  A position is
//                       four 32-bit words of two counters each; an add is one integer atomicAdd of 1 or 1 << 16 straight
//                       to memory, nothing comes back.  A counter stays below 4095 (DAGCON_MAX_COVERAGE alignments, each
//                       at most once per counter and position), so no half carries into the other.  The host clears the
//                       words on the stream before every execution.
//   k_pile_sites<false> a thread per position, a block per tile of 256: marks the sites (the rule in integers), counts
//                       them per tile.
//   k_pile_scan         one block (k_scan.hip.h): the exclusive prefix over the tiles; the total; DG_E_SITE_OVF when the
//                       arena is too small (the batch is re-run with a larger one, as for every other arena).
//   k_pile_sites<true>  the same marks again, every site stored at its place: tile offset, waves in front, lanes in
//                       front.  The order is that of the positions; no atomic decides it.
//
// Every index is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_scan.hip.h"
#include "k_walk.hip.h"

#define DG_PILE_TILE 256u

__global__ __launch_bounds__(256) void k_pile_count(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    DgWalk wk;
    if (dg_walk_open(p, a, lane, wk) != DG_WALK_GO) return;
    const uint32_t t = wk.t, tlen = wk.tlen;
    const uint64_t pb = p.pile_begin[t];
    if (pb > p.pile_n || tlen > p.pile_n - pb) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    uint32_t *cnt = p.pile + 4ull * pb;
    uint32_t tc0 = wk.s0;
    bool carry = false, bad = false;                                    // carry: the column in front of this step holds a target base
    for (uint32_t c0 = wk.lo; c0 < wk.hi; c0 += 64u) {
        const DgWalkStep s = dg_walk_step(wk, c0, tc0, lane);
        const uint8_t qb = s.qb;
        const unsigned long long mT = s.mT;
        const uint32_t tc = s.tc;
        const bool prevT = lane ? ((mT >> (lane - 1)) & 1ull) != 0ull : carry;
        if (s.isT) {
            if (tc >= tlen) bad = true;
            else {
                uint32_t w = 2u, inc = 1u;                              // N
                if (qb == DG_GAP) inc = 1u << 16;                       // DEL
                else switch (qb & 0xDFu) {
                    case 'A': w = 0u; break;
                    case 'C': w = 0u; inc = 1u << 16; break;
                    case 'G': w = 1u; break;
                    case 'T': w = 1u; inc = 1u << 16; break;
                    default: break;
                }
                atomicAdd(&cnt[4ull * tc + w], inc);
            }
        } else if (s.v && qb != DG_GAP && prevT) {
            // the first column of an insertion run: it belongs to the base in front, tc - 1 (prevT: tc >= 1 + the start)
            if (tc == 0u || tc - 1u >= tlen) bad = true;
            else atomicAdd(&cnt[4ull * (tc - 1u) + 3u], 1u);
        }
        tc0 += (uint32_t)__popcll(mT);
        carry = (mT >> 63) != 0ull;
    }
    if (__ballot(bad)) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); }
}

// the rule of dagcon_pileup_opts on the four words of a position
__device__ __forceinline__ bool dg_pile_is_site(const uint4 w, const uint32_t min_count, const uint32_t min_ppm) {
    const uint32_t n[6] = {w.x & 0xFFFFu, w.x >> 16, w.y & 0xFFFFu, w.y >> 16, w.z & 0xFFFFu, w.z >> 16};
    const uint32_t ins = w.w & 0xFFFFu;
    uint32_t depth = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        depth += n[k];
        if (n[k] > s1) { s2 = s1; s1 = n[k]; }
        else if (n[k] > s2) s2 = n[k];
    }
    if (!depth) return false;
    const uint32_t rest = depth >= ins ? depth - ins : 0u;
    const uint32_t mi = ins < rest ? ins : rest, m = s2 > mi ? s2 : mi;
    return m >= min_count && (unsigned long long)m * 1000000ull >= (unsigned long long)min_ppm * depth;
}

template <bool WRITE>
__global__ __launch_bounds__(DG_PILE_TILE) void k_pile_sites(DgParams p) {
    if (dg_failed(p)) return;
    __shared__ uint32_t s_wave[DG_PILE_TILE / 64u];
    const uint64_t g = (uint64_t)blockIdx.x * DG_PILE_TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool site = false;
    uint32_t t = 0;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (g < p.pile_n) {
        // the target of position g: the last one that begins at or in front of it (targets without a base begin where the next does)
        uint32_t l = 0, r = p.T;
        while (l < r) { const uint32_t m = l + (r - l) / 2u; if (p.pile_begin[m] <= g) l = m + 1u; else r = m; }
        t = l ? l - 1u : 0u;
        if (l && !dg_tskip(p, t)) {
            w = reinterpret_cast<const uint4 *>(p.pile)[g];
            site = dg_pile_is_site(w, p.pile_min_count, p.pile_min_ppm);
        }
    }
    const unsigned long long m = __ballot(site);
    if (lane == 0) s_wave[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) p.pile_tile[blockIdx.x] = (unsigned long long)s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    } else {
        if (!site) return;
        unsigned long long at = p.pile_tile[blockIdx.x] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; k++) at += s_wave[k];
        if (at >= p.site_cap || at >= *p.site_top) { dg_fail_target(p, t, DG_E_INTERNAL); return; }
        DgSite s;
        s.pos = (uint32_t)(g - p.pile_begin[t]); s.tgt = t; s.w[0] = w.x; s.w[1] = w.y; s.w[2] = w.z; s.w[3] = w.w;
        p.pile_site[at] = s;
    }
}

// the exclusive prefix of the tiles' site counts, one block
struct DgPileScanItem {
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return (p.pile_n + DG_PILE_TILE - 1u) / DG_PILE_TILE; }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t b) const { return p.pile_tile[b]; }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t b, const unsigned long long off) const { p.pile_tile[b] = off; }
    static constexpr auto top = &DgParams::site_top; static constexpr auto cap = &DgParams::site_cap;
    static constexpr uint32_t ovf = DG_E_SITE_OVF;
};
__global__ __launch_bounds__(1024) void k_pile_scan(DgParams p) { dg_block_scan<DgPileScanItem>(p); }
