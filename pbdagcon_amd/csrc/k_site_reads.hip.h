// k_site_reads.hip.h -- which alignment shows which allele at each site of the pile-up, and a two-way split of the
// alignments of a target (dagcon_set_site_reads; include/dagcon.h has the rule).  It runs right behind k_pile_sites<true>
// and reads what that left: the site list (pile_site, *site_top) and, as k_pile_count does, the normalised, trimmed columns.
//
//   k_sr_mark           a thread per site: sets the bit of its position in sr_bits (cleared on the stream before every
//                       execution), and the first site of a 64-position word stores its own index in sr_rank of that word.
//                       The site of a position whose bit is set is then sr_rank[word] + popcount(bits below): no search.
//                       A word without a site is never asked, so sr_rank needs no clearing.
//   k_sr_walk<false>    a wave per alignment, k_pile_count's walk (k_walk.hip.h): 64 columns a step, the coordinate from a
//                       ballot and a population count.  A column with a target base whose position has its bit set is an entry; the
//                       wave counts them, sr_cnt[a] (DG_SR_TAKEN: the alignment is one the graph took).  A column whose
//                       bit is clear costs the walk one test of a word that the 64 lanes share.
//   k_sr_scan           one block (k_scan.hip.h): the exclusive prefix of the alignments' entry counts; the total; DG_E_SR_OVF when the
//                       arena is too small (the batch is re-run with a larger one).
//   k_sr_walk<true>     the same walk, every entry stored at its place: the alignment's offset, the entries of the steps
//                       before, the lanes in front.  The code is cls | ins << 3: cls by k_pile_count's classification, ins
//                       when the column behind is the first of an insertion run (that column's own lane would count INS
//                       for the same position; here the lane of the base looks one column ahead, lane 63 with a load).
//   k_sr_split          phase on: a block per target.  A site's sign rule (k1, k2 or the insertion rule) goes to sr_kind
//                       (DG_SR_MUTED for a site that dagcon_set_site_link found no partners for: k_site_link.hip.h);
//                       the seed is the alignment with the most signed entries; then rounds of two steps, a wave per
//                       alignment summing M * sigma over its entries (no atomics), and a wave per alignment adding M * h
//                       to its sites' sums with integer atomicAdd (an integer sum does not depend on the order).  A round
//                       that changes nothing ends the loop: the rounds after it would change nothing either.
//
// Every index is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_scan.hip.h"
#include "k_walk.hip.h"

// sites of the batch the kernels may index: *site_top, never more than the arena
__device__ __forceinline__ unsigned long long dg_sr_nsite(const DgParams &p) {
    const unsigned long long n = *p.site_top;
    return n < p.site_cap ? n : p.site_cap;
}

__global__ __launch_bounds__(256) void k_sr_mark(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long n = dg_sr_nsite(p);
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const DgSite s = p.pile_site[k];
    if (s.tgt >= p.T) return;                                          // (k_pile_sites wrote it: never; the walk finds no bit for it)
    const uint64_t pb = p.pile_begin[s.tgt];
    if (s.pos >= p.tlen[s.tgt] || pb > p.pile_n || s.pos >= p.pile_n - pb) { dg_fail_target(p, s.tgt, DG_E_INTERNAL); return; }
    const uint64_t g = pb + s.pos;
    atomicOr(&p.sr_bits[g >> 6], 1ull << (g & 63u));
    bool first = k == 0;
    if (!first) {
        const DgSite q = p.pile_site[k - 1];
        first = q.tgt >= p.T || ((p.pile_begin[q.tgt] + q.pos) >> 6) != (g >> 6);
    }
    if (first) p.sr_rank[g >> 6] = (uint32_t)k;
}

// k_pile_count's classification of a column with a target base: 0..5 for A C G T N DEL
__device__ __forceinline__ uint32_t dg_sr_cls(const uint8_t qb) {
    if (qb == DG_GAP) return 5u;
    switch (qb & 0xDFu) {
        case 'A': return 0u;
        case 'C': return 1u;
        case 'G': return 2u;
        case 'T': return 3u;
        default: return 4u;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_sr_walk(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    DgWalk wk;
    if (dg_walk_open(p, a, lane, wk) != DG_WALK_GO) {                  // (<false>: every early way out leaves a count of 0)
        if (!WRITE && lane == 0) p.sr_cnt[a] = 0u;
        return;
    }
    const uint32_t t = wk.t, tlen = wk.tlen, hi = wk.hi;
    const uint64_t pb = p.pile_begin[t];
    if (pb > p.pile_n || tlen > p.pile_n - pb) {
        if (lane == 0) { dg_fail_target(p, t, DG_E_INTERNAL); if (!WRITE) p.sr_cnt[a] = 0u; }
        return;
    }
    const unsigned long long n_site = dg_sr_nsite(p);
    unsigned long long at = 0ull, end = 0ull;
    if (WRITE) {
        at = p.sr_off[a];
        const uint32_t cnt = p.sr_cnt[a] & ~DG_SR_TAKEN;
        if (at > p.sr_cap || cnt > p.sr_cap - at) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
        end = at + cnt;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t tc0 = wk.s0, total = 0u;
    bool bad = false;
    for (uint32_t c0 = wk.lo; c0 < hi; c0 += 64u) {
        const DgWalkStep ws = dg_walk_step(wk, c0, tc0, lane);
        const uint32_t i = ws.i, tc = ws.tc;
        bool ent = false;
        unsigned long long word = 0ull;
        uint64_t g = 0;
        if (ws.isT) {
            if (tc >= tlen) bad = true;
            else { g = pb + tc; word = p.sr_bits[g >> 6]; ent = ((word >> (g & 63u)) & 1ull) != 0ull; }
        }
        const unsigned long long mE = __ballot(ent);
        if (WRITE && mE) {
            // the column behind: the next lane's, lane 63's from memory
            uint32_t nx = (uint32_t)__shfl_down((int)ws.c, 1);
            if (lane == 63) nx = i + 1u < hi ? wk.col[i + 1u] : (uint32_t)(DG_GAP | (DG_GAP << 8));
            if (ent) {
                const bool ins = i + 1u < hi && (uint8_t)(nx >> 8) == DG_GAP && (uint8_t)(nx & 0xff) != DG_GAP;
                const unsigned long long k = (unsigned long long)p.sr_rank[g >> 6] + (unsigned long long)__popcll(word & ((1ull << (g & 63u)) - 1ull));
                const unsigned long long to = at + (unsigned long long)total + (unsigned long long)__popcll(mE & lt);
                if (k >= n_site || to >= end) bad = true;
                else {
                    const DgSite s = p.pile_site[k];
                    if (s.tgt != t || s.pos != tc) bad = true;
                    else { p.sr_site[to] = (uint32_t)k; p.sr_code[to] = (uint8_t)(dg_sr_cls(ws.qb) | (ins ? 8u : 0u)); }
                }
            }
        }
        total += (uint32_t)__popcll(mE);
        tc0 += (uint32_t)__popcll(ws.mT);
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (WRITE && at + total != end) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    if (any_bad) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); }
    if (!WRITE && lane == 0) p.sr_cnt[a] = any_bad ? 0u : (total | DG_SR_TAKEN);
}

// the exclusive prefix of the alignments' entry counts, one block
struct DgSrScanItem {
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return p.A; }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t a) const { return p.sr_cnt[a] & ~DG_SR_TAKEN; }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t a, const unsigned long long off) const { p.sr_off[a] = off; }
    static constexpr auto top = &DgParams::sr_top; static constexpr auto cap = &DgParams::sr_cap;
    static constexpr uint32_t ovf = DG_E_SR_OVF;
};
__global__ __launch_bounds__(1024) void k_sr_scan(DgParams p) { dg_block_scan<DgSrScanItem>(p); }

// what decides an entry's sign at a site: 0x80 an insertion site; otherwise k1 | k2 << 3, k2 == 7: no second class.
// DG_SR_MUTED, both class fields 7, matches no class (a class is 0 .. 5): every entry's sign is 0 there
#define DG_SR_MUTED 0x3Fu
__host__ __device__ __forceinline__ uint32_t dg_sr_kind(const DgSite &s) {
    const uint32_t n[6] = {s.w[0] & 0xFFFFu, s.w[0] >> 16, s.w[1] & 0xFFFFu, s.w[1] >> 16, s.w[2] & 0xFFFFu, s.w[2] >> 16};
    const uint32_t ins = s.w[3] & 0xFFFFu;
    uint32_t depth = 0, k1 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) { depth += n[k]; if (n[k] > n[k1]) k1 = (uint32_t)k; }
    uint32_t k2 = 7u, c2 = 0u;
#pragma unroll
    for (int k = 0; k < 6; k++)
        if ((uint32_t)k != k1 && n[k] > c2) { c2 = n[k]; k2 = (uint32_t)k; }
    // (c2 is the pile-up's s2: the largest of the others is the second largest of the six, ties as they fall)
    const uint32_t rest = depth >= ins ? depth - ins : 0u;
    if ((ins < rest ? ins : rest) > c2) return 0x80u;
    return k1 | (k2 << 3);
}
__host__ __device__ __forceinline__ int dg_sr_sign(const uint32_t code, const uint32_t kind) {
    if (kind & 0x80u) return (code & 8u) ? -1 : 1;
    const uint32_t cls = code & 7u;
    return cls == (kind & 7u) ? 1 : cls == ((kind >> 3) & 7u) ? -1 : 0;
}

__global__ __launch_bounds__(256) void k_sr_split(DgParams p) {
    if (dg_failed(p)) return;
    const uint32_t t = blockIdx.x;
    if (t >= p.T) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t b0 = p.aln_begin[t], b1 = p.aln_begin[t + 1];
    if (b0 > b1 || b1 > p.A) { if (threadIdx.x == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const uint32_t a0 = (uint32_t)b0, a1 = (uint32_t)b1;
    for (uint64_t a = (uint64_t)a0 + threadIdx.x; a < a1; a += 256u) p.sr_hap[a] = 0u;
    if (dg_tskip(p, t)) return;
    // the target's sites: pile_site is in the order of the targets
    const unsigned long long n_site = dg_sr_nsite(p);
    unsigned long long s0, s1;
    {
        unsigned long long l = 0, r = n_site;
        while (l < r) { const unsigned long long m = l + (r - l) / 2u; if (p.pile_site[m].tgt < t) l = m + 1u; else r = m; }
        s0 = l; r = n_site;
        while (l < r) { const unsigned long long m = l + (r - l) / 2u; if (p.pile_site[m].tgt <= t) l = m + 1u; else r = m; }
        s1 = l;
    }
    __shared__ uint32_t s_best[4], s_besta[4], s_seed;
    __shared__ int s_changed, s_bad;
    if (threadIdx.x == 0) { s_changed = 0; s_bad = 0; }
    for (unsigned long long k = s0 + threadIdx.x; k < s1; k += 256u) {
        // (dagcon_set_site_link: a site that is not linked gets the kind under which every entry's sign is 0)
        p.sr_kind[k] = p.lk_linked && !p.lk_linked[k] ? (uint8_t)DG_SR_MUTED : (uint8_t)dg_sr_kind(p.pile_site[k]);
        p.sr_sigma[k] = 0;
        p.sr_acc[k] = 0;
    }
    __syncthreads();
    // signed entries per alignment, and the seed: the most of them, ties to the lowest alignment
    uint32_t best = 0u, best_a = 0xFFFFFFFFu;
    bool bad = false;
    for (uint64_t a = (uint64_t)a0 + (uint32_t)wv; a < a1; a += 4u) {
        const uint32_t raw = p.sr_cnt[a], cnt = raw & ~DG_SR_TAKEN;
        const unsigned long long e0 = p.sr_off[a];
        uint32_t nz = 0u;
        if (e0 > p.sr_cap || cnt > p.sr_cap - e0) bad = true;
        else
            for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
                const unsigned long long k = p.sr_site[e0 + j];
                if (k < s0 || k >= s1) { bad = true; continue; }
                nz += dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]) != 0;
            }
        for (int o = 32; o; o >>= 1) nz += (uint32_t)__shfl_xor((int)nz, o);
        if (lane == 0) p.sr_nz[a] = nz;
        if (nz > best) { best = nz; best_a = (uint32_t)a; }                     // (a ascends in a wave: the first of the largest stays)
    }
    if (__ballot(bad)) { if (lane == 0) s_bad = 1; }
    if (lane == 0) { s_best[wv] = best; s_besta[wv] = best_a; }
    __syncthreads();
    if (s_bad) { if (threadIdx.x == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    if (threadIdx.x == 0) {
        uint32_t b = 0u, ba = 0xFFFFFFFFu;
        for (int k = 0; k < 4; k++)
            if (s_best[k] > b || (s_best[k] == b && b && s_besta[k] < ba)) { b = s_best[k]; ba = s_besta[k]; }
        s_seed = ba;
    }
    __syncthreads();
    const uint32_t seed = s_seed;
    if (seed == 0xFFFFFFFFu) return;                                   // no alignment has a signed entry: everything stays 0
    {
        const uint32_t cnt = p.sr_cnt[seed] & ~DG_SR_TAKEN;
        const unsigned long long e0 = p.sr_off[seed];
        for (uint32_t j = threadIdx.x; j < cnt; j += 256u) {
            const unsigned long long k = p.sr_site[e0 + j];
            p.sr_sigma[k] = (int8_t)dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]);
        }
    }
    __syncthreads();
    for (uint32_t round = 0; round < p.sr_rounds; round++) {
        // step 1: h[x] = sgn(sum_k M(x, k) sigma[k]); step 2's sums right behind it, from the same wave
        bool changed = false;
        for (uint64_t a = (uint64_t)a0 + (uint32_t)wv; a < a1; a += 4u) {
            if (!p.sr_nz[a]) continue;
            const uint32_t cnt = p.sr_cnt[a] & ~DG_SR_TAKEN;
            const unsigned long long e0 = p.sr_off[a];
            int sum = 0;
            for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
                const unsigned long long k = p.sr_site[e0 + j];
                sum += dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]) * (int)p.sr_sigma[k];
            }
            for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
            const int h = sum > 0 ? 1 : sum < 0 ? -1 : 0;
            const uint8_t hv = h > 0 ? 1u : h < 0 ? 2u : 0u;
            if (lane == 0) {
                if (p.sr_hap[a] != hv) changed = true;
                p.sr_hap[a] = hv;
            }
            if (h)
                for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
                    const unsigned long long k = p.sr_site[e0 + j];
                    const int m = dg_sr_sign(p.sr_code[e0 + j], p.sr_kind[k]);
                    if (m) atomicAdd(&p.sr_acc[k], m * h);
                }
        }
        if (changed && lane == 0) s_changed = 1;
        __syncthreads();                                               // every h is read before a sigma changes: the sums above used the old ones
        // step 2: sigma[k] = sgn(sum_x M(x, k) h[x]); the sum is taken and cleared in one atomic
        bool changed2 = false;
        for (unsigned long long k = s0 + threadIdx.x; k < s1; k += 256u) {
            const int sum = atomicExch(&p.sr_acc[k], 0);
            const int8_t sg = sum > 0 ? 1 : sum < 0 ? -1 : 0;
            if (p.sr_sigma[k] != sg) { changed2 = true; p.sr_sigma[k] = sg; }
        }
        if (changed2) s_changed = 1;
        __syncthreads();
        const int any = s_changed;
        __syncthreads();
        if (!any) break;
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
    }
}
