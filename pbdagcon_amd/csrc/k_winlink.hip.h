// k_winlink.hip.h -- the read labels of neighbouring windows joined into blocks (dagcon_set_window_phase; include/dagcon.h
// has the rule, 9).  It runs right behind k_sr_split and reads what that left: sr_cnt (DG_SR_TAKEN), sr_hap, sr_sigma.  A
// window is a target of the pipeline, its alignments are [aln_begin[w], aln_begin[w + 1]) and, being the pieces of
// plan_windows, ascend in their record (wl_rec).
//
//   k_wl_pairs          a wave per window.  A window with a predecessor (the same wl_tgt as the window in front) takes its
//                       alignments 64 at a time; a lane whose alignment is taken and labelled looks its record up in the
//                       predecessor's range by binary search and classes the pair as same or differ when the piece found
//                       is taken and labelled too.  The two counts are summed by ballot and population count, lane 0
//                       stores them: no atomics.  A window without a predecessor stores 0, 0.
//   k_wl_scan           one block, rounds of 1,024 windows as in k_scan.hip.h, but a segmented scan: a window's item is
//                       (head, flip) -- an unlinked window (w + 1, 0), a linked one (0, diff > same) -- and
//                       a (+) b = b.head ? b : (a.head, a.flip ^ b.flip), which is associative.  The inclusive prefix of
//                       window w holds its block (the nearest unlinked window in front, or itself) and its orientation.
//                       The link test of rule 9.3 is evaluated here, in 64-bit integers.
//   k_wl_apply          a thread per alignment and per site: the oriented hap and phase.
//
// Every index is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_site_reads.hip.h"

__global__ __launch_bounds__(256) void k_wl_pairs(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t w64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w64 >= p.T) return;
    const uint32_t w = (uint32_t)w64;
    const int lane = threadIdx.x & 63;
    uint32_t same = 0u, diff = 0u;
    if (w > 0u && p.wl_tgt[w] == p.wl_tgt[w - 1u] && !dg_tskip(p, w) && !dg_tskip(p, w - 1u)) {
        const uint64_t p0 = p.aln_begin[w - 1u], b0 = p.aln_begin[w], b1 = p.aln_begin[w + 1u];
        if (p0 > b0 || b0 > b1 || b1 > p.A) { if (lane == 0) dg_fail_target(p, w, DG_E_INTERNAL); }
        else {
            bool bad = false;
            for (uint64_t a0 = b0; a0 < b1; a0 += 64u) {
                const uint64_t a = a0 + (uint32_t)lane;
                bool s = false, d = false;
                if (a < b1 && (p.sr_cnt[a] & DG_SR_TAKEN)) {
                    const uint32_t h = p.sr_hap[a];
                    if (h > 2u) bad = true;
                    else if (h) {
                        const uint32_t r = p.wl_rec[a];
                        uint64_t l = p0, e = b0;
                        while (l < e) { const uint64_t m = l + (e - l) / 2u; if (p.wl_rec[m] < r) l = m + 1u; else e = m; }
                        if (l < b0 && p.wl_rec[l] == r && (p.sr_cnt[l] & DG_SR_TAKEN)) {
                            const uint32_t g = p.sr_hap[l];
                            if (g > 2u) bad = true;
                            else if (g) { s = g == h; d = g != h; }
                        }
                    }
                }
                same += (uint32_t)__popcll(__ballot(s));
                diff += (uint32_t)__popcll(__ballot(d));
            }
            if (__ballot(bad)) { if (lane == 0) dg_fail_target(p, w, DG_E_INTERNAL); same = diff = 0u; }
        }
    }
    if (lane == 0) { p.wl_cnt[2ull * w] = same; p.wl_cnt[2ull * w + 1u] = diff; }
}

// rule 9.3 on a window's two counts
__device__ __forceinline__ bool dg_wl_linked(const DgParams &p, const uint32_t same, const uint32_t diff) {
    const unsigned long long hi = same > diff ? same : diff, lo = same > diff ? diff : same;
    return hi >= p.wl_min_links && hi > lo && lo * 1000000ull <= (unsigned long long)p.wl_max_ppm * (hi + lo);
}

// a (+) b of the segmented scan: head << 1 | flip
__device__ __forceinline__ unsigned long long dg_wl_join(const unsigned long long a, const unsigned long long b) {
    return (b >> 1) ? b : (a ^ (b & 1ull));
}

__global__ __launch_bounds__(1024) void k_wl_scan(DgParams p) {
    if (dg_failed(p)) return;
    __shared__ unsigned long long s_part[16], s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    const uint64_t n = p.T;
    for (uint64_t i0 = 0; i0 < n; i0 += 1024u) {
        const uint64_t i = i0 + threadIdx.x;
        unsigned long long incl = 0ull;                                // (past the end: the identity)
        if (i < n) {
            const uint32_t same = p.wl_cnt[2ull * i], diff = p.wl_cnt[2ull * i + 1u];
            incl = i > 0u && dg_wl_linked(p, same, diff) ? (diff > same ? 1ull : 0ull) : (i + 1ull) << 1;
        }
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long up = __shfl_up(incl, o); if (lane >= o) incl = dg_wl_join(up, incl); }
        if (lane == 63) s_part[wv] = incl;
        __syncthreads();
        unsigned long long acc = s_carry;
        for (int k = 0; k < wv; k++) acc = dg_wl_join(acc, s_part[k]);
        acc = dg_wl_join(acc, incl);
        if (i < n) {
            const unsigned long long head = acc >> 1;
            if (head == 0ull || head > i + 1ull) dg_fail_target(p, (uint32_t)i, DG_E_INTERNAL);   // (window 0 is a head: never)
            p.wl_block[i] = head ? (uint32_t)(head - 1ull) : (uint32_t)i;
            p.wl_flip[i] = (uint8_t)(acc & 1ull);
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = acc;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_wl_apply(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i < p.A) {
        const uint32_t t = p.aln_tgt[i];
        if (t < p.T) {
            const uint8_t h = p.sr_hap[i];
            p.wl_hap[i] = h == 0u || h > 2u || !p.wl_flip[t] ? h : (uint8_t)(3u - h);
        } else p.wl_hap[i] = 0u;
    }
    if (i < dg_sr_nsite(p)) {
        const uint32_t t = p.pile_site[i].tgt;
        const int8_t s = p.sr_sigma[i];
        p.wl_phase[i] = t < p.T && p.wl_flip[t] ? (int8_t)-s : s;
    }
}
