// k_join.hip.h -- adjacent sites joined into runs, and per run the table of what its spanning alignments show at all of
// its sites at once (dagcon_set_site_join; include/dagcon.h has the rule, 10).  It runs right behind k_al_index and reads
// what the site reads and the alleles left: the site list, the entries (sr_off, sr_cnt, sr_site), every entry's allele
// index (al_idx), the sites' stretches (al_soff) and sr_hap.
//
//   k_jn_stretch        one block (k_scan.hip.h): site k continues site k - 1 iff same target and position + 1.  The prefix
//                       of "does not continue" numbers the stretches; a stretch's first site is stored under its number.
//   k_jn_runs           one block: site k is a run head iff it does not continue or lies a multiple of DG_JN_SITES behind
//                       its stretch's first site.  The prefix of the heads numbers the runs (jn_run) and stores where each
//                       begins (jn_rbeg, one more for the end of the last).
//   k_jn_keys           a wave per alignment, k_al_index's entry loop, a lane per entry.  The lane of an alignment's first
//                       entry inside a run decides whether the alignment spans the run: the next m - 1 entries must exist
//                       and be the run's next sites.  A spanning member's key, a nibble per site, goes into the stretch of
//                       the run's first site (the spanning members of a run number at most that site's depth, so al_soff
//                       addresses arrays as long as the entry arena: no arena of its own, no overflow path), at a place
//                       claimed with an integer atomicAdd on the run's cursor; its entries keep the place (jn_idx, for
//                       now).  Otherwise the lane adds 1 to the run's partial members.  Cursors and partial counts are
//                       cleared on the stream before every execution.  Look-ahead is by loads: a run may lie anywhere in
//                       the loop's 64 entries.
//   k_jn_table          a wave per run of at most 64 spanning members: the two sorts of k_al_table (dg_al_wave_sort).
//   k_jn_table_deep     a block per deeper run: the two sorts of k_al_table_deep in LDS (dg_al_block_sort).
//   k_jn_tscan          one block: the exclusive prefix of the runs' table lengths, the total.
//   k_jn_index          a wave per alignment: every entry of a spanning member takes its index from the map at its place,
//                       every other entry 0xFFFF; phase on: the lane of the member's first entry adds 1 or 1 << 16 to the
//                       allele's word, once per member.
//   k_jn_pack           a wave per run, launched by dagcon_fetch_joined_sites: the table to its place in the compact arrays.
//
// Integer sums and sorts of whole multisets only: nothing that is fetched depends on an order of execution.  Every index
// is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_alleles.hip.h"
#include "k_scan.hip.h"
#include "k_site_reads.hip.h"

#ifndef DG_JN_SITES
#define DG_JN_SITES 16u                 // sites a run holds at most: a nibble each in a 64-bit key (include/dagcon.h has it too)
#endif
#define DG_JN_NONE 0xFFFFu              // jn_idx of an entry of a partial member

// runs of the batch the kernels may index
__device__ __forceinline__ unsigned long long dg_jn_nrun(const DgParams &p) {
    const unsigned long long n = *p.jn_run_top, ns = dg_sr_nsite(p);
    return n < ns ? n : ns;
}

struct DgJnStretchItem {
    uint32_t nc;
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return dg_sr_nsite(p); }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t k) {
        nc = 1u;
        if (k > 0) {
            const DgSite s = p.pile_site[k], b = p.pile_site[k - 1];
            nc = s.tgt == b.tgt && s.pos == b.pos + 1u ? 0u : 1u;
        }
        return nc;
    }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t k, const unsigned long long off) const {
        const unsigned long long s = off + nc - 1ull;                      // (site 0 does not continue: off + nc >= 1)
        p.jn_run[k] = (uint32_t)s;
        if (nc) p.jn_sfirst[s] = (uint32_t)k;
    }
    static constexpr auto top = &DgParams::jn_st_top; static constexpr auto cap = &DgParams::al_nocap;
    static constexpr uint32_t ovf = DG_E_INTERNAL;          // (never raised: al_nocap is 2^64 - 1)
};
__global__ __launch_bounds__(1024) void k_jn_stretch(DgParams p) { dg_block_scan<DgJnStretchItem>(p); }

struct DgJnRunItem {
    uint32_t head;
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return dg_sr_nsite(p); }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t k) {
        const uint32_t s = p.jn_run[k];                                    // the stretch, until store puts the run there
        const uint64_t f = s <= k ? p.jn_sfirst[s] : k;
        head = f > k || (k - f) % DG_JN_SITES == 0u ? 1u : 0u;
        return head;
    }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t k, const unsigned long long off) const {
        const unsigned long long r = off + head - 1ull;
        p.jn_run[k] = (uint32_t)r;
        if (head) p.jn_rbeg[r] = (uint32_t)k;
        if (k + 1u == n(p)) p.jn_rbeg[r + 1ull] = (uint32_t)(k + 1u);
    }
    static constexpr auto top = &DgParams::jn_run_top; static constexpr auto cap = &DgParams::al_nocap;
    static constexpr uint32_t ovf = DG_E_INTERNAL;
};
__global__ __launch_bounds__(1024) void k_jn_runs(DgParams p) { dg_block_scan<DgJnRunItem>(p); }

struct DgJnTableItem {
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return dg_jn_nrun(p); }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t r) const { return p.jn_nd[r]; }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t r, const unsigned long long off) const { p.jn_toff[r] = off; }
    static constexpr auto top = &DgParams::jn_top; static constexpr auto cap = &DgParams::al_nocap;
    static constexpr uint32_t ovf = DG_E_INTERNAL;
};
__global__ __launch_bounds__(1024) void k_jn_tscan(DgParams p) { dg_block_scan<DgJnTableItem>(p); }

// an entry's run: the run of site k, its sites [b, b + m).  false: an index is out of its range
__device__ __forceinline__ bool dg_jn_run_of(const DgParams &p, const unsigned long long k, const unsigned long long n_site, const unsigned long long n_run,
                                             uint32_t &r, uint32_t &b, uint32_t &m) {
    if (k >= n_site) return false;
    r = p.jn_run[k];
    if (r >= n_run) return false;
    b = p.jn_rbeg[r];
    const uint32_t e = p.jn_rbeg[r + 1u];
    if (b > k || e <= k || e > n_site || e - b > DG_JN_SITES) return false;
    m = e - b;
    return true;
}

// the header of an alignment for the two entry loops; false: nothing to do
__device__ __forceinline__ bool dg_jn_aln_open(const DgParams &p, const uint32_t a, const int lane, uint32_t &t, uint32_t &cnt, unsigned long long &e0, uint32_t &hv) {
    t = p.aln_tgt[a];
    if (t >= p.T || dg_tskip(p, t)) return false;
    const uint32_t raw = p.sr_cnt[a];
    cnt = raw & ~DG_SR_TAKEN;
    if (!(raw & DG_SR_TAKEN)) return false;
    e0 = p.sr_off[a];
    hv = p.sr_phase ? p.sr_hap[a] : 0u;
    if (hv > 2u || e0 > p.sr_cap || cnt > p.sr_cap - e0) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return false; }
    return true;
}

__global__ __launch_bounds__(256) void k_jn_keys(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const int lane = threadIdx.x & 63;
    uint32_t t = 0u, cnt = 0u, hv = 0u;
    unsigned long long e0 = 0ull;
    if (!dg_jn_aln_open(p, (uint32_t)a64, lane, t, cnt, e0, hv)) return;
    const unsigned long long n_site = dg_sr_nsite(p), n_run = dg_jn_nrun(p);
    bool bad = false;
    for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
        const unsigned long long k = p.sr_site[e0 + j];
        uint32_t r = 0u, b = 0u, m = 0u;
        if (!dg_jn_run_of(p, k, n_site, n_run, r, b, m)) { bad = true; continue; }
        // one lane per alignment and run: the one of the alignment's first entry inside the run
        if (k != b && j != 0u) continue;
        bool spans = k == b && m <= cnt - j;
        unsigned long long key = 0ull;
        if (spans) {
            // an alignment's entries are consecutive positions: with m entries left, they are the run's sites
            for (uint32_t i = 0; i < m; i++) {
                const unsigned long long ki = p.sr_site[e0 + j + i];
                if (ki != (unsigned long long)b + i) { spans = false; bad = true; break; }
                const uint32_t ai = p.al_idx[e0 + j + i];
                if (ai >= p.al_nd[ki]) { spans = false; bad = true; break; }
                key |= (unsigned long long)(ai < 15u ? ai : 15u) << (4u * (15u - i));
            }
            if (!spans) continue;
            const DgSite s = p.pile_site[b];
            const unsigned long long off = p.al_soff[b];
            const uint32_t depth = dg_al_depth(s);
            if (s.tgt != t || off > p.sr_cap || depth > p.sr_cap - off) { bad = true; continue; }
            const uint32_t c = atomicAdd(&p.jn_cur[r], 1u);
            if (c >= depth) { bad = true; continue; }
            p.jn_key[off + c] = key;
            for (uint32_t i = 0; i < m; i++) p.jn_idx[e0 + j + i] = (uint16_t)c;
        } else atomicAdd(&p.jn_part[r], 1u);
    }
    if (__ballot(bad) && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

// The two tables.  The sorts, their order and their items are the sites' own (dg_al_wave_sort, dg_al_block_sort, dg_al_less,
// DgAlItem: k_alleles.hip.h).  The steps between the sorts stand here a second time: with k_al_table and k_al_table_deep
// calling these two functions instead of their own bodies the compiler gave those kernels other registers (30 -> 27 and
// 122 -> 106 VGPRs, profiles/site_join/resource_usage.txt), and the kernels of an output that is not asked for stay as they are.
// The table of up to 64 keys, a key a lane, as k_al_table builds a site's: the `depth` keys at srt[off ..] become
// the table at the front of the same stretch (key, count, the counts per label from 0), every place of the stretch learns
// the index of its allele (map).  Returns the table's length
__device__ __forceinline__ uint32_t dg_jn_wave_table(unsigned long long *srt, uint32_t *tcnt, uint32_t *thap, uint16_t *map, const unsigned long long off,
                                                     const uint32_t depth, const int lane) {
    DgAlItem v;
    const bool have = (uint32_t)lane < depth;
    v.w = have ? 0u : DG_AL_PAD;
    v.key = have ? srt[off + (uint32_t)lane] : ~0ull;
    v.lo = (uint32_t)lane;                                              // the place in the stretch: what the entry knows itself by
    v = dg_al_wave_sort(v, lane);
    const uint32_t slot = v.lo;
    const unsigned long long prev = __shfl_up(v.key, 1);
    const bool head = have && (lane == 0 || prev != v.key);
    const unsigned long long mH = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : mH >> (lane + 1);
    const uint32_t next = above ? (uint32_t)lane + 1u + (uint32_t)__builtin_ctzll(above) : depth;
    const uint32_t nd = (uint32_t)__popcll(mH);
    // the head of this lane's run: the highest head at or below the lane
    const unsigned long long below = mH & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
    const uint32_t mine = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
    v.w = head ? DG_AL_DEEP - (next - (uint32_t)lane) : DG_AL_PAD;
    if (!head) v.key = ~0ull;
    v.lo = (uint32_t)lane;                                              // where the head stood
    v = dg_al_wave_sort(v, lane);
    if ((uint32_t)lane < nd) {
        srt[off + (uint32_t)lane] = v.key;
        tcnt[off + (uint32_t)lane] = DG_AL_DEEP - v.w;
        thap[off + (uint32_t)lane] = 0u;
    }
    // allele i of the table came from the head at v.lo of lane i: every entry of that head's run gets i
    uint32_t index = 0u;
    for (uint32_t i = 0; i < nd; i++)
        if ((uint32_t)__shfl((int)v.lo, (int)i) == mine) index = i;
    if (have) map[off + slot] = (uint16_t)index;
    return nd;
}

// The same for up to DG_AL_DEEP keys, a block in LDS, as k_al_table_deep builds a deep site's.  Every thread of the block calls it with the same arguments; *s_nd is 0
// and the block is in step when it begins; the caller puts a barrier in front of the arrays' next use
struct DgJnLds { unsigned long long *key; uint32_t *w; uint16_t *lo, *slot, *head, *inv; };
__device__ __forceinline__ uint32_t dg_jn_block_table(unsigned long long *srt, uint32_t *tcnt, uint32_t *thap, uint16_t *map, const unsigned long long off,
                                                      const uint32_t depth, const DgJnLds l, uint32_t *s_nd) {
    unsigned long long *const s_key = l.key;
    uint32_t *const s_w = l.w;
    uint16_t *const s_lo = l.lo, *const s_slot = l.slot, *const s_head = l.head, *const s_inv = l.inv;
    uint32_t n2 = 128u;
    while (n2 < depth) n2 <<= 1;
    for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
        const bool have = i < depth;
        s_w[i] = have ? 0u : DG_AL_PAD;
        s_key[i] = have ? srt[off + i] : ~0ull;
        s_lo[i] = (uint16_t)i;
    }
    __syncthreads();
    dg_al_block_sort(s_key, s_w, s_lo, n2);
    // the heads and their runs: every thread reads, then every thread writes
    uint32_t run[DG_AL_DEEP / 256u], heads = 0u;
#pragma unroll
    for (uint32_t r = 0; r < DG_AL_DEEP / 256u; r++) {
        const uint32_t i = threadIdx.x + 256u * r;
        run[r] = 0u;
        if (i < depth) s_slot[i] = s_lo[i];
        if (i < depth && (i == 0u || s_key[i - 1u] != s_key[i])) {
            uint32_t e = i;
            do s_head[e++] = (uint16_t)i; while (e < depth && s_key[e] == s_key[i]);
            run[r] = e - i;
            heads++;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < DG_AL_DEEP / 256u; r++) {
        const uint32_t i = threadIdx.x + 256u * r;
        if (i >= n2) continue;
        if (run[r]) s_w[i] = DG_AL_DEEP - run[r];
        else { s_w[i] = DG_AL_PAD; s_key[i] = ~0ull; }
        s_lo[i] = (uint16_t)i;                                         // where the head stood
    }
    if (heads) atomicAdd(s_nd, heads);
    __syncthreads();
    dg_al_block_sort(s_key, s_w, s_lo, n2);
    const uint32_t nd = *s_nd;
    for (uint32_t i = threadIdx.x; i < nd; i += 256u) {
        srt[off + i] = s_key[i];
        tcnt[off + i] = DG_AL_DEEP - s_w[i];
        thap[off + i] = 0u;
        s_inv[s_lo[i]] = (uint16_t)i;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < depth; i += 256u) map[off + s_slot[i]] = s_inv[s_head[i]];
    return nd;
}

// a run's header for the table kernels: false: nothing to build (nd is written)
__device__ __forceinline__ bool dg_jn_run_open(const DgParams &p, const unsigned long long r, const bool first, uint32_t &t, uint32_t &n, unsigned long long &off) {
    const unsigned long long n_site = dg_sr_nsite(p);
    const uint32_t b = p.jn_rbeg[r];
    if (b >= n_site) { if (first) p.jn_nd[r] = 0u; return false; }
    const DgSite s = p.pile_site[b];
    t = s.tgt;
    if (t >= p.T || dg_tskip(p, t)) { if (first) p.jn_nd[r] = 0u; return false; }
    const uint32_t depth = dg_al_depth(s);
    off = p.al_soff[b];
    n = p.jn_cur[r];
    if (off > p.sr_cap || depth > p.sr_cap - off || depth > DG_AL_DEEP || n > depth) {
        if (first) { dg_fail_target(p, t, DG_E_INTERNAL); p.jn_nd[r] = 0u; }
        return false;
    }
    if (!n) { if (first) p.jn_nd[r] = 0u; return false; }
    return true;
}

__global__ __launch_bounds__(256) void k_jn_table(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long r = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= dg_jn_nrun(p)) return;
    const int lane = threadIdx.x & 63;
    uint32_t t = 0u, n = 0u;
    unsigned long long off = 0ull;
    // the header as lane 0 read it: every lane of the wave takes the same way
    const bool go = dg_jn_run_open(p, r, lane == 0, t, n, off);
    if (!__shfl((int)go, 0)) return;
    t = (uint32_t)__shfl((int)t, 0); n = (uint32_t)__shfl((int)n, 0); off = __shfl(off, 0);
    if (n > 64u) {
        if (lane == 0) {
            const uint32_t at = atomicAdd(&p.jn_cur[p.site_cap], 1u);
            if (at < p.site_cap) p.jn_deep[at] = (uint32_t)r;
            else { dg_fail_target(p, t, DG_E_INTERNAL); p.jn_nd[r] = 0u; }
        }
        return;
    }
    const uint32_t nd = dg_jn_wave_table(p.jn_key, p.jn_tcnt, p.jn_thap, p.jn_map, off, n, lane);
    if (lane == 0) p.jn_nd[r] = nd;
}

__global__ __launch_bounds__(256) void k_jn_table_deep(DgParams p) {
    if (dg_failed(p)) return;
    __shared__ unsigned long long s_key[DG_AL_DEEP];
    __shared__ uint32_t s_w[DG_AL_DEEP];
    __shared__ uint16_t s_lo[DG_AL_DEEP], s_slot[DG_AL_DEEP], s_head[DG_AL_DEEP], s_inv[DG_AL_DEEP];
    __shared__ uint32_t s_nd, s_n;
    __shared__ unsigned long long s_off;
    const uint32_t listed = p.jn_cur[p.site_cap], n_deep = listed < p.site_cap ? listed : (uint32_t)p.site_cap;
    const unsigned long long n_run = dg_jn_nrun(p);
    for (uint32_t w = blockIdx.x; w < n_deep; w += gridDim.x) {
        const unsigned long long r = p.jn_deep[w];
        // the header, read by one thread: every thread of the block takes the same way
        if (threadIdx.x == 0) {
            uint32_t t = 0u, n = 0u;
            unsigned long long o = 0ull;
            s_n = r < n_run && dg_jn_run_open(p, r, true, t, n, o) ? n : 0u;
            s_off = o;
            s_nd = 0u;
        }
        __syncthreads();
        const uint32_t n = s_n;
        const unsigned long long off = s_off;
        if (!n) { __syncthreads(); continue; }
        const uint32_t nd = dg_jn_block_table(p.jn_key, p.jn_tcnt, p.jn_thap, p.jn_map, off, n, {s_key, s_w, s_lo, s_slot, s_head, s_inv}, &s_nd);
        if (threadIdx.x == 0) p.jn_nd[r] = nd;
        __syncthreads();                                                   // (s_nd and the arrays are the next run's)
    }
}

__global__ __launch_bounds__(256) void k_jn_index(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const int lane = threadIdx.x & 63;
    uint32_t t = 0u, cnt = 0u, hv = 0u;
    unsigned long long e0 = 0ull;
    if (!dg_jn_aln_open(p, (uint32_t)a64, lane, t, cnt, e0, hv)) return;
    const unsigned long long n_site = dg_sr_nsite(p), n_run = dg_jn_nrun(p);
    bool bad = false;
    for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
        const unsigned long long k = p.sr_site[e0 + j];
        uint32_t r = 0u, b = 0u, m = 0u;
        if (!dg_jn_run_of(p, k, n_site, n_run, r, b, m)) { bad = true; continue; }
        // the member spans the run iff its entry at the run's first site and the one at its last both exist (k_jn_keys
        // checked the ones between)
        const uint32_t jj = (uint32_t)(k - b);
        const bool spans = jj <= j && m <= cnt - (j - jj) && p.sr_site[e0 + j - jj] == b && p.sr_site[e0 + j - jj + m - 1u] == b + m - 1u;
        if (!spans) { p.jn_idx[e0 + j] = DG_JN_NONE; continue; }
        const DgSite s = p.pile_site[b];
        const unsigned long long off = p.al_soff[b];
        const uint32_t depth = dg_al_depth(s), slot = p.jn_idx[e0 + j], n = p.jn_cur[r], nd = p.jn_nd[r];
        if (s.tgt != t || off > p.sr_cap || depth > p.sr_cap - off || n > depth || slot >= n) { bad = true; continue; }
        const uint32_t i = p.jn_map[off + slot];
        if (i >= nd) { bad = true; continue; }
        p.jn_idx[e0 + j] = (uint16_t)i;
        if (hv && jj == 0u) atomicAdd(&p.jn_thap[off + i], hv == 1u ? 1u : 1u << 16);
    }
    if (__ballot(bad) && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

__global__ __launch_bounds__(256) void k_jn_pack(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long r = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= dg_jn_nrun(p)) return;
    const int lane = threadIdx.x & 63;
    const uint32_t nd = p.jn_nd[r];
    if (!nd) return;
    const uint32_t b = p.jn_rbeg[r];
    if (b >= dg_sr_nsite(p)) return;
    const uint32_t t = p.pile_site[b].tgt;
    if (t >= p.T) return;
    const unsigned long long off = p.al_soff[b], to = p.jn_toff[r], n = *p.jn_top;
    if (off > p.sr_cap || nd > p.sr_cap - off || n > p.sr_cap || to > n || nd > n - to) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    for (uint32_t i = (uint32_t)lane; i < nd; i += 64u) {
        p.jn_ckey[to + i] = p.jn_key[off + i];
        p.jn_ccnt[to + i] = p.jn_tcnt[off + i];
        p.jn_chap[to + i] = p.jn_thap[off + i];
    }
}
