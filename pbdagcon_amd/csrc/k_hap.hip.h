// k_hap.hip.h -- the tally of the two-way split (dagcon_set_hap_consensus; include/dagcon.h has the rule): per site how
// often each label shows each of the site's two alleles, per target how well the labels separate and whether the target
// is worth a consensus per label.  It runs right behind k_sr_split and reads what that left: sr_hap, sr_sigma, sr_kind
// and the entries of k_sr_walk<true>.
//
//   k_hap_tally         a wave per alignment (k_sr_walk's grid), the entry loop of the split's step 1: a signed entry of an
//                       alignment with hap 1 or 2 is one 32-bit integer atomicAdd on its site's words in hap_cnt (cleared
//                       on the stream before every execution) -- word 0 is P1 | M1 << 16, word 1 is P2 | M2 << 16, two
//                       16-bit counters a word as in k_pile_count.  A count is at most DAGCON_MAX_COVERAGE = 4094 < 65536:
//                       no half carries into the other.  A deep target is spread over as many waves as it has reads.
//   k_hap_targets       a block per target: the slice of pile_site by k_sr_split's search, the sites' agree / disagree /
//                       separating and the alignments' labels summed by one block reduction (4 x 6 words of LDS), one
//                       record of DG_HAP_REC words per target, zeros for a target without a graph.
//
// Integer sums only: nothing depends on an order.  Every index is checked before it is used; a violation fails the target
// with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_site_reads.hip.h"

__global__ __launch_bounds__(256) void k_hap_tally(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    const uint32_t t = p.aln_tgt[a];
    if (t >= p.T || dg_tskip(p, t)) return;
    const uint32_t raw = p.sr_cnt[a], cnt = raw & ~DG_SR_TAKEN;
    if (!(raw & DG_SR_TAKEN)) return;
    const uint32_t hv = p.sr_hap[a];
    if (hv == 0u) return;                                              // unassigned: it is counted in n0 alone
    const unsigned long long e0 = p.sr_off[a];
    if (hv > 2u || e0 > p.sr_cap || cnt > p.sr_cap - e0) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const unsigned long long n_site = dg_sr_nsite(p);
    bool bad = false;
    for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
        const unsigned long long k = p.sr_site[e0 + j];
        if (k >= n_site || p.pile_site[k].tgt != t) { bad = true; continue; }
        const int m = dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]);
        if (m) atomicAdd(&p.hap_cnt[2ull * k + (hv - 1u)], m > 0 ? 1u : 1u << 16);
    }
    if (__ballot(bad) && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

__global__ __launch_bounds__(256) void k_hap_targets(DgParams p) {
    if (dg_failed(p)) return;
    const uint32_t t = blockIdx.x;
    if (t >= p.T) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *rec = p.hap_rec + (size_t)DG_HAP_REC * t;
    if (threadIdx.x < DG_HAP_REC) rec[threadIdx.x] = 0u;               // what a target without a graph keeps
    const uint64_t b0 = p.aln_begin[t], b1 = p.aln_begin[t + 1];
    if (b0 > b1 || b1 > p.A) { if (threadIdx.x == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    if (dg_tskip(p, t)) return;
    const uint32_t a0 = (uint32_t)b0, a1 = (uint32_t)b1;
    // the target's sites: pile_site is in the order of the targets (k_sr_split's search)
    const unsigned long long n_site = dg_sr_nsite(p);
    unsigned long long s0, s1;
    {
        unsigned long long l = 0, r = n_site;
        while (l < r) { const unsigned long long m = l + (r - l) / 2u; if (p.pile_site[m].tgt < t) l = m + 1u; else r = m; }
        s0 = l; r = n_site;
        while (l < r) { const unsigned long long m = l + (r - l) / 2u; if (p.pile_site[m].tgt <= t) l = m + 1u; else r = m; }
        s1 = l;
    }
    // v: n1 n2 n0 n_sep agree disagree
    uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    bool bad = false;
    for (unsigned long long k = s0 + threadIdx.x; k < s1; k += 256u) {
        const uint32_t w0 = p.hap_cnt[2ull * k], w1 = p.hap_cnt[2ull * k + 1u];
        const uint32_t P1 = w0 & 0xFFFFu, M1 = w0 >> 16, P2 = w1 & 0xFFFFu, M2 = w1 >> 16;
        const int sg = p.sr_sigma[k];
        if (sg > 0) { v[3] += P1 >= 1u && M2 >= 1u; v[4] += P1 + M2; v[5] += M1 + P2; }
        else if (sg < 0) { v[3] += M1 >= 1u && P2 >= 1u; v[4] += M1 + P2; v[5] += P1 + M2; }
    }
    for (uint64_t a = (uint64_t)a0 + threadIdx.x; a < a1; a += 256u) {
        if (!(p.sr_cnt[a] & DG_SR_TAKEN)) continue;
        const uint32_t hv = p.sr_hap[a];
        if (hv > 2u) { bad = true; continue; }
        v[hv == 1u ? 0 : hv == 2u ? 1 : 2]++;
    }
    __shared__ uint32_t s_v[4][6];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; i++) {
        uint32_t x = v[i];
        for (int o = 32; o; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
        if (lane == 0) s_v[wv][i] = x;
    }
    if (__ballot(bad) && lane == 0) s_bad = 1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (s_bad) { dg_fail_target(p, t, DG_E_INTERNAL); return; }
    uint32_t s[6];
#pragma unroll
    for (int i = 0; i < 6; i++) s[i] = s_v[0][i] + s_v[1][i] + s_v[2][i] + s_v[3][i];
    const uint32_t K = a1 - a0;
    // (a failure after the test above leaves a record behind; the host reports a failed target's as zeros)
    const bool split = s[0] <= K && s[1] <= K && s[3] >= p.hap_min_sites && s[0] >= p.hap_min_reads && s[1] >= p.hap_min_reads &&
                       K - s[1] >= p.hap_min_cov && K - s[0] >= p.hap_min_cov;
#pragma unroll
    for (int i = 0; i < 6; i++) rec[i] = s[i];
    rec[6] = split ? 1u : 0u;
}
