// k_site_link.hip.h -- which sites of a target are carried by the same reads as other sites near them (dagcon_set_site_link;
// include/dagcon.h, rule 13, has the definition).  A heterozygous site and a collapsed repeat copy split the reads the same
// way at every site; a read error does not.  The kernels run between k_sr_walk<true> and k_sr_split, which then mutes the
// sites that are not linked: their entries get the sign 0 in the split and in everything behind it.
//
//   k_lk_kind    a thread per site: what decides an entry's sign at the site (dg_sr_kind, the one copy of that rule), into
//                sr_kind, where k_sr_split would write the same byte later.
//   k_lk_bits    a wave per alignment, a lane per entry: the entry's sign sets bit (x - aln_begin[t]) of its site's row P
//                (M = +1) or row M (M = -1) with a 64-bit atomicOr.  The rows are cleared on the stream before every
//                execution; an OR does not depend on the order.  A site's rows are 2 * lk_words words, P then M, the
//                sites one behind the other: one width for the batch, that of its deepest target.
//   k_lk_pairs   a wave per site i, a lane per candidate j of [i - reach, i + reach], 64 candidates a step.  A candidate
//                counts when it is a site of the same target: pile_site is in the order of the targets, so that test
//                clips the range to the target's own sites without a search.  Four ANDs and population counts a word; the
//                rows of neighbouring candidates are neighbours in memory, so a step's loads coalesce.  The partners of a
//                step are a ballot and a population count.  No atomics, no LDS: every site looks both ways and writes only
//                its own count.
//
// dg_lk_pair and dg_lk_rows are the rule's arithmetic, with no kernel and no device-only construct in them, so that a host
// compiler takes them as well (tests/native/site_link_host.cpp runs them on the CPU; define DG_LK_HOST_ONLY in front).
// Every index is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include <stdint.h>

#ifndef DG_HD_INLINE
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DG_HD_INLINE __host__ __device__ __forceinline__
#else
#define DG_HD_INLINE inline __attribute__((always_inline))
#endif
#endif

#define DG_LK_MAX_REACH 4096u

// Rule 13.2 on the four counts of a pair of sites: partners or not.  All of it in 64-bit integers.
DG_HD_INLINE bool dg_lk_pair(const uint32_t pp, const uint32_t mm, const uint32_t pm, const uint32_t mp, const uint32_t max_conflict_ppm, const uint32_t min_cell) {
    const uint64_t same = (uint64_t)pp + mm, diff = (uint64_t)pm + mp;
    const uint64_t lo = same < diff ? same : diff, hi = same < diff ? diff : same;
    const uint32_t cell = same >= diff ? (pp < mm ? pp : mm) : (pm < mp ? pm : mp);
    return lo * 1000000ull <= (uint64_t)max_conflict_ppm * (lo + hi) && cell >= min_cell;
}

// the four counts pp mm pm mp from two sites' rows of `words` words each
DG_HD_INLINE void dg_lk_cells(const unsigned long long *Pi, const unsigned long long *Mi, const unsigned long long *Pj, const unsigned long long *Mj, const uint32_t words,
                              uint32_t c[4]) {
    uint32_t pp = 0u, mm = 0u, pm = 0u, mp = 0u;
    for (uint32_t w = 0; w < words; w++) {
        const unsigned long long a = Pi[w], b = Mi[w], x = Pj[w], y = Mj[w];
        pp += (uint32_t)__builtin_popcountll(a & x); mm += (uint32_t)__builtin_popcountll(b & y);
        pm += (uint32_t)__builtin_popcountll(a & y); mp += (uint32_t)__builtin_popcountll(b & x);
    }
    c[0] = pp; c[1] = mm; c[2] = pm; c[3] = mp;
}

// the counts, then the test
DG_HD_INLINE bool dg_lk_rows(const unsigned long long *Pi, const unsigned long long *Mi, const unsigned long long *Pj, const unsigned long long *Mj, const uint32_t words,
                             const uint32_t max_conflict_ppm, const uint32_t min_cell) {
    uint32_t c[4];
    dg_lk_cells(Pi, Mi, Pj, Mj, words, c);
    return dg_lk_pair(c[0], c[1], c[2], c[3], max_conflict_ppm, min_cell);
}

#ifndef DG_LK_HOST_ONLY
#include "dagcon_dev.h"
#include "k_site_reads.hip.h"

__global__ __launch_bounds__(256) void k_lk_kind(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k >= dg_sr_nsite(p)) return;
    p.sr_kind[k] = (uint8_t)dg_sr_kind(p.pile_site[k]);
}

__global__ __launch_bounds__(256) void k_lk_bits(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64, lane = threadIdx.x & 63u;
    const uint32_t t = p.aln_tgt[a];
    if (t >= p.T || dg_tskip(p, t)) return;
    const uint32_t raw = p.sr_cnt[a], cnt = raw & ~DG_SR_TAKEN;
    if (!(raw & DG_SR_TAKEN) || !cnt) return;
    const uint64_t b0 = p.aln_begin[t];
    const unsigned long long e0 = p.sr_off[a];
    const uint64_t W = p.lk_words;
    // the alignment's bit lies inside a row, and its entries inside the arena
    if (a64 < b0 || a64 - b0 >= W * 64u || e0 > p.sr_cap || cnt > p.sr_cap - e0) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const uint32_t x = (uint32_t)(a64 - b0);
    const unsigned long long bit = 1ull << (x & 63u);
    const unsigned long long n_site = dg_sr_nsite(p);
    bool bad = false;
    for (uint32_t j = lane; j < cnt; j += 64u) {
        const unsigned long long k = p.sr_site[e0 + j];
        if (k >= n_site || (k + 1ull) * 2ull * W > p.lk_row_cap) { bad = true; continue; }
        const int m = dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]);
        if (m) atomicOr(&p.lk_rows[k * 2ull * W + (m < 0 ? W : 0ull) + (x >> 6)], bit);
    }
    if (__ballot(bad) && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

__global__ __launch_bounds__(256) void k_lk_pairs(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long n_site = dg_sr_nsite(p);
    const unsigned long long i = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_site) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = p.pile_site[i].tgt;
    if (t >= p.T) return;                                              // (k_pile_sites wrote it: never)
    const uint64_t W = p.lk_words;
    if (dg_tskip(p, t) || (i + 1ull) * 2ull * W > p.lk_row_cap) {
        if (lane == 0) {
            if (!dg_tskip(p, t)) dg_fail_target(p, t, DG_E_INTERNAL);
            p.lk_partners[i] = 0u; p.lk_linked[i] = 0u;
        }
        return;
    }
    const unsigned long long *ri = p.lk_rows + i * 2ull * W;
    const unsigned long long j0 = i > p.lk_reach ? i - p.lk_reach : 0ull;
    const unsigned long long j1 = n_site - i > (unsigned long long)p.lk_reach + 1ull ? i + p.lk_reach + 1ull : n_site;
    uint32_t partners = 0u;
    for (unsigned long long base = j0; base < j1; base += 64u) {
        const unsigned long long j = base + lane;
        // a site of the same target, and its rows inside the arena (j < n_site <= site_cap: they are)
        bool is = false;
        if (j < j1 && j != i && (j + 1ull) * 2ull * W <= p.lk_row_cap && p.pile_site[j].tgt == t)
            is = dg_lk_rows(ri, ri + W, p.lk_rows + j * 2ull * W, p.lk_rows + j * 2ull * W + W, (uint32_t)W, p.lk_ppm, p.lk_min_cell);
        partners += (uint32_t)__popcll(__ballot(is));
    }
    if (lane == 0) {
        p.lk_partners[i] = (uint16_t)partners;                         // (at most 2 * DG_LK_MAX_REACH)
        p.lk_linked[i] = partners >= p.lk_min_partners ? 1u : 0u;
    }
}
#endif
