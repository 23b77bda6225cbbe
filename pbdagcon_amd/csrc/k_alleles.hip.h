// k_alleles.hip.h -- the alleles at the sites: what each alignment's bases between target base p and target base p + 1 are,
// grouped and counted per site, and per entry the index of its allele (dagcon_set_site_alleles; include/dagcon.h has the
// rule, 8).  It runs right behind k_sr_walk<true>, and behind k_sr_split for the counts per label, and reads what those
// left: the site list, the entries (sr_off, sr_cnt, sr_site), sr_hap and, as k_sr_walk does, the normalised, trimmed columns.
//
//   k_al_soff           one block (k_scan.hip.h): the exclusive prefix of the sites' depths.  The entries of a site number
//                       exactly its depth, so the prefix gives every site a stretch of an array as long as the entry arena:
//                       no arena of its own, no overflow path.  A site of a target that is out has a stretch of 0.
//   k_al_keys           a wave per alignment, k_sr_walk<true>'s walk and slot arithmetic.  The lane of an entry reads ahead
//                       through the columns of its insertion run, at most 21 of them (a run may cross the 64-column step
//                       and is cut by hi), and builds the key.  The key goes into the site's stretch at a place
//                       claimed with an integer atomicAdd on the site's cursor (cleared on the stream before every
//                       execution), and the entry keeps that place (al_idx, for now).  Which place an entry gets depends
//                       on the order of execution; nothing that is fetched does: only the multiset of a stretch is used.
//   k_al_table          a wave per site of depth <= 64, a key a lane: a bitonic sort by key in registers, the heads of the
//                       runs from one ballot, a run's length from the next head; then the same network again on
//                       (count descending, key ascending) with every lane that is no head sent to the end.  Lane i < nd
//                       holds allele i of the table: key and count go to the head of the site's own stretch (the table
//                       cannot be longer than the stretch), the counts per label start from 0.  Both sorts carry a tag:
//                       the first the key's place in the stretch, the second where the run's head stood; so every place
//                       of the stretch learns the index of its allele (al_map), with no search.  A deeper site goes on
//                       a list (one integer atomicAdd; the list's order is never read as an order).
//   k_al_table_deep     a block per listed site, the same two sorts in LDS: 4,096 keys, words and tags, and three more
//                       arrays of 4,096 x 2 B for the map (80 KB: two blocks a CU).
//   k_al_tscan          one block: the exclusive prefix of the sites' allele counts, the total.
//   k_al_index          a wave per alignment (k_hap_tally's entry loop): an entry reads the index of its allele from al_map
//                       at its place in the stretch and stores it over the place; phase on: one integer atomicAdd of 1 or 1 << 16 on the allele's word c1 | c2 << 16
//                       (a count is at most DAGCON_MAX_COVERAGE = 4094: no half carries into the other; c0 is the rest).
//   k_al_pack           a wave per site: the table from the site's stretch to its place in the compact arrays.  It is
//                       launched by dagcon_fetch_site_alleles, not by the run: the compact arrays are sized by the total
//                       k_al_tscan left, and a run that nobody asks pays nothing for them.
//
// Integer sums and sorts of whole multisets only: nothing depends on an order of execution.  Every index is checked before
// it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_scan.hip.h"
#include "k_site_reads.hip.h"
#include "k_walk.hip.h"

#define DG_AL_BASES 20u                 // bases a key holds; bit 60: the allele is longer
#define DG_AL_LONG (1ull << 60)
#define DG_AL_DEEP 4096u                // keys a block sorts: a site has at most DAGCON_MAX_COVERAGE = 4094 entries
#define DG_AL_PAD 0xFFFFFFFFu           // the sort word of what is no allele: behind every count

__device__ __forceinline__ uint32_t dg_al_depth(const DgSite &s) {
    return (s.w[0] & 0xFFFFu) + (s.w[0] >> 16) + (s.w[1] & 0xFFFFu) + (s.w[1] >> 16) + (s.w[2] & 0xFFFFu) + (s.w[2] >> 16);
}

// the exclusive prefix of the sites' depths, one block
struct DgAlDepthItem {
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return dg_sr_nsite(p); }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t k) const {
        const DgSite s = p.pile_site[k];
        return s.tgt >= p.T || dg_tskip(p, s.tgt) ? 0ull : dg_al_depth(s);
    }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t k, const unsigned long long off) const { p.al_soff[k] = off; }
    static constexpr auto top = &DgParams::al_ent_top; static constexpr auto cap = &DgParams::al_nocap;
    static constexpr uint32_t ovf = DG_E_INTERNAL;          // (never raised: al_nocap is 2^64 - 1; the users check every slot against sr_cap)
};
__global__ __launch_bounds__(1024) void k_al_soff(DgParams p) { dg_block_scan<DgAlDepthItem>(p); }

// the exclusive prefix of the sites' allele counts, one block
struct DgAlTableItem {
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return dg_sr_nsite(p); }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t k) const { return p.al_nd[k]; }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t k, const unsigned long long off) const { p.al_toff[k] = off; }
    static constexpr auto top = &DgParams::al_top; static constexpr auto cap = &DgParams::al_nocap;
    static constexpr uint32_t ovf = DG_E_INTERNAL;
};
__global__ __launch_bounds__(1024) void k_al_tscan(DgParams p) { dg_block_scan<DgAlTableItem>(p); }

__global__ __launch_bounds__(256) void k_al_keys(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    DgWalk wk;
    if (dg_walk_open(p, a, lane, wk) != DG_WALK_GO) return;
    const uint32_t t = wk.t, tlen = wk.tlen, hi = wk.hi;
    const uint64_t pb = p.pile_begin[t];
    if (pb > p.pile_n || tlen > p.pile_n - pb) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const unsigned long long n_site = dg_sr_nsite(p);
    const unsigned long long at = p.sr_off[a];
    const uint32_t cnt = p.sr_cnt[a] & ~DG_SR_TAKEN;
    if (at > p.sr_cap || cnt > p.sr_cap - at) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const unsigned long long end = at + cnt;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t tc0 = wk.s0, total = 0u;
    bool bad = false;
    for (uint32_t c0 = wk.lo; c0 < hi; c0 += 64u) {
        const DgWalkStep ws = dg_walk_step(wk, c0, tc0, lane);
        bool ent = false;
        if (ws.isT) {
            if (ws.tc >= tlen) bad = true;
            else { const uint64_t g = pb + ws.tc; ent = ((p.sr_bits[g >> 6] >> (g & 63u)) & 1ull) != 0ull; }
        }
        const unsigned long long mE = __ballot(ent);
        if (ent) {
            // the allele: the base of the column, then the inserted bases behind it
            unsigned long long key = 0ull;
            uint32_t L = 0u;
            if (ws.qb != DG_GAP) { key = (unsigned long long)(dg_sr_cls(ws.qb) + 1u) << (3u * (DG_AL_BASES - 1u)); L = 1u; }
            for (uint32_t j = ws.i + 1u; j < hi; j++) {
                const uint32_t c = wk.col[j];
                const uint8_t qb = (uint8_t)(c & 0xff);
                if ((uint8_t)(c >> 8) != DG_GAP || qb == DG_GAP) break;
                if (L == DG_AL_BASES) { key |= DG_AL_LONG; break; }
                key |= (unsigned long long)(dg_sr_cls(qb) + 1u) << (3u * (DG_AL_BASES - 1u - L));
                L++;
            }
            const unsigned long long to = at + (unsigned long long)total + (unsigned long long)__popcll(mE & lt);
            if (to >= end) bad = true;
            else {
                const unsigned long long k = p.sr_site[to];
                if (k >= n_site) bad = true;
                else {
                    const DgSite s = p.pile_site[k];
                    const unsigned long long off = p.al_soff[k];
                    const uint32_t depth = dg_al_depth(s);
                    if (s.tgt != t || s.pos != ws.tc || off > p.sr_cap || depth > p.sr_cap - off) bad = true;
                    else {
                        const uint32_t c = atomicAdd(&p.al_cur[k], 1u);
                        if (c >= depth) bad = true;
                        else { p.al_idx[to] = (uint16_t)c; p.al_srt[off + c] = key; }
                    }
                }
            }
        }
        total += (uint32_t)__popcll(mE);
        tc0 += (uint32_t)__popcll(ws.mT);
    }
    if (__ballot(bad) != 0ull || at + total != end) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); }
}

// what the two sorts order: the word first, then the key, then the tag (the tag only rides along: where an item came from)
struct DgAlItem { uint32_t w; unsigned long long key; uint32_t lo; };
__device__ __forceinline__ bool dg_al_less(const DgAlItem &x, const DgAlItem &y) {
    return x.w < y.w || (x.w == y.w && (x.key < y.key || (x.key == y.key && x.lo < y.lo)));
}

// 64 items, one a lane, ascending over the lanes
__device__ __forceinline__ DgAlItem dg_al_wave_sort(DgAlItem v, const int lane) {
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            DgAlItem o;
            o.w = (uint32_t)__shfl_xor((int)v.w, j);
            o.key = __shfl_xor(v.key, j);
            o.lo = (uint32_t)__shfl_xor((int)v.lo, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            if (dg_al_less(o, v) == keep_min) v = o;
        }
    return v;
}

// a site's header for the table kernels: false: nothing to build (nd is written)
__device__ __forceinline__ bool dg_al_site_open(const DgParams &p, const unsigned long long k, const bool first, uint32_t &t, uint32_t &depth, unsigned long long &off) {
    const DgSite s = p.pile_site[k];
    t = s.tgt;
    if (t >= p.T || dg_tskip(p, t)) { if (first) p.al_nd[k] = 0u; return false; }
    depth = dg_al_depth(s);
    off = p.al_soff[k];
    if (off > p.sr_cap || depth > p.sr_cap - off || depth > DG_AL_DEEP || p.al_cur[k] != depth) {
        if (first) { dg_fail_target(p, t, DG_E_INTERNAL); p.al_nd[k] = 0u; }
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_al_table(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long k = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= dg_sr_nsite(p)) return;
    const int lane = threadIdx.x & 63;
    uint32_t t = 0u, depth = 0u;
    unsigned long long off = 0ull;
    // the header as lane 0 read it: every lane of the wave takes the same way
    const bool go = dg_al_site_open(p, k, lane == 0, t, depth, off);
    if (!__shfl((int)go, 0)) return;
    t = (uint32_t)__shfl((int)t, 0); depth = (uint32_t)__shfl((int)depth, 0); off = __shfl(off, 0);
    if (depth > 64u) {
        if (lane == 0) {
            const uint32_t at = atomicAdd(&p.al_cur[p.site_cap], 1u);
            if (at < p.site_cap) p.al_deep[at] = (uint32_t)k;
            else { dg_fail_target(p, t, DG_E_INTERNAL); p.al_nd[k] = 0u; }
        }
        return;
    }
    DgAlItem v;
    const bool have = (uint32_t)lane < depth;
    v.w = have ? 0u : DG_AL_PAD;
    v.key = have ? p.al_srt[off + (uint32_t)lane] : ~0ull;
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
        p.al_srt[off + (uint32_t)lane] = v.key;
        p.al_tcnt[off + (uint32_t)lane] = DG_AL_DEEP - v.w;
        p.al_thap[off + (uint32_t)lane] = 0u;
    }
    // allele i of the table came from the head at v.lo of lane i: every entry of that head's run gets i
    uint32_t index = 0u;
    for (uint32_t i = 0; i < nd; i++)
        if ((uint32_t)__shfl((int)v.lo, (int)i) == mine) index = i;
    if (have) p.al_map[off + slot] = (uint16_t)index;
    if (lane == 0) p.al_nd[k] = nd;
}

// n2 items in LDS, a power of two, ascending
__device__ __forceinline__ void dg_al_block_sort(unsigned long long *s_key, uint32_t *s_w, uint16_t *s_lo, const uint32_t n2) {
    for (uint32_t k = 2u; k <= n2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
                const uint32_t x = i ^ j;
                if (x <= i) continue;
                const DgAlItem lo = {s_w[i], s_key[i], s_lo[i]}, hi = {s_w[x], s_key[x], s_lo[x]};
                if (dg_al_less(hi, lo) == ((i & k) == 0u)) {
                    s_w[i] = hi.w; s_key[i] = hi.key; s_lo[i] = (uint16_t)hi.lo; s_w[x] = lo.w; s_key[x] = lo.key; s_lo[x] = (uint16_t)lo.lo;
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(256) void k_al_table_deep(DgParams p) {
    if (dg_failed(p)) return;
    __shared__ unsigned long long s_key[DG_AL_DEEP];
    __shared__ uint32_t s_w[DG_AL_DEEP];
    __shared__ uint16_t s_lo[DG_AL_DEEP], s_slot[DG_AL_DEEP], s_head[DG_AL_DEEP], s_inv[DG_AL_DEEP];   // the tag; an entry's place in the stretch; its run's head; the head's allele
    __shared__ uint32_t s_nd, s_depth;
    __shared__ unsigned long long s_off;
    const uint32_t listed = p.al_cur[p.site_cap], n_deep = listed < p.site_cap ? listed : (uint32_t)p.site_cap;
    const unsigned long long n_site = dg_sr_nsite(p);
    for (uint32_t w = blockIdx.x; w < n_deep; w += gridDim.x) {
        const unsigned long long k = p.al_deep[w];
        // the header, read by one thread: every thread of the block takes the same way
        if (threadIdx.x == 0) {
            uint32_t t = 0u, d = 0u;
            unsigned long long o = 0ull;
            s_depth = k < n_site && dg_al_site_open(p, k, true, t, d, o) ? d : 0u;
            s_off = o;
            s_nd = 0u;
        }
        __syncthreads();
        const uint32_t depth = s_depth;
        const unsigned long long off = s_off;
        if (!depth) { __syncthreads(); continue; }
        uint32_t n2 = 128u;
        while (n2 < depth) n2 <<= 1;
        for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
            const bool have = i < depth;
            s_w[i] = have ? 0u : DG_AL_PAD;
            s_key[i] = have ? p.al_srt[off + i] : ~0ull;
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
        if (heads) atomicAdd(&s_nd, heads);
        __syncthreads();
        dg_al_block_sort(s_key, s_w, s_lo, n2);
        const uint32_t nd = s_nd;
        for (uint32_t i = threadIdx.x; i < nd; i += 256u) {
            p.al_srt[off + i] = s_key[i];
            p.al_tcnt[off + i] = DG_AL_DEEP - s_w[i];
            p.al_thap[off + i] = 0u;
            s_inv[s_lo[i]] = (uint16_t)i;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < depth; i += 256u) p.al_map[off + s_slot[i]] = s_inv[s_head[i]];
        if (threadIdx.x == 0) p.al_nd[k] = nd;
        __syncthreads();                                                   // (s_nd and the arrays are the next site's)
    }
}

__global__ __launch_bounds__(256) void k_al_index(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    const uint32_t t = p.aln_tgt[a];
    if (t >= p.T || dg_tskip(p, t)) return;
    const uint32_t raw = p.sr_cnt[a], cnt = raw & ~DG_SR_TAKEN;
    if (!(raw & DG_SR_TAKEN)) return;
    const unsigned long long e0 = p.sr_off[a];
    const uint32_t hv = p.sr_phase ? p.sr_hap[a] : 0u;
    if (hv > 2u || e0 > p.sr_cap || cnt > p.sr_cap - e0) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    const unsigned long long n_site = dg_sr_nsite(p);
    bool bad = false;
    for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
        const unsigned long long k = p.sr_site[e0 + j];
        if (k >= n_site) { bad = true; continue; }
        const DgSite s = p.pile_site[k];
        const unsigned long long off = p.al_soff[k];
        const uint32_t depth = dg_al_depth(s), slot = p.al_idx[e0 + j], nd = p.al_nd[k];
        if (s.tgt != t || off > p.sr_cap || depth > p.sr_cap - off || slot >= depth) { bad = true; continue; }
        const uint32_t i = p.al_map[off + slot];
        if (i >= nd) { bad = true; continue; }
        p.al_idx[e0 + j] = (uint16_t)i;
        if (hv) atomicAdd(&p.al_thap[off + i], hv == 1u ? 1u : 1u << 16);
    }
    if (__ballot(bad) && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

__global__ __launch_bounds__(256) void k_al_pack(DgParams p) {
    if (dg_failed(p)) return;
    const unsigned long long k = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= dg_sr_nsite(p)) return;
    const int lane = threadIdx.x & 63;
    const uint32_t nd = p.al_nd[k];
    if (!nd) return;
    const uint32_t t = p.pile_site[k].tgt;
    if (t >= p.T) return;
    const unsigned long long off = p.al_soff[k], to = p.al_toff[k], n = *p.al_top;
    if (off > p.sr_cap || nd > p.sr_cap - off || n > p.sr_cap || to > n || nd > n - to) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    for (uint32_t i = (uint32_t)lane; i < nd; i += 64u) {
        p.al_ckey[to + i] = p.al_srt[off + i];
        p.al_ccnt[to + i] = p.al_tcnt[off + i];
        p.al_chap[to + i] = p.al_thap[off + i];
    }
}
