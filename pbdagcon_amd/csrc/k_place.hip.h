// k_place.hip.h -- dagcon_place: for (query q, target t) pairs, the strand of q on t, its support on each strand and
// the span of t it covers, from k-mer votes binned by diagonal.  This is the step blasr did for q-sense.py; the contract
// (include/dagcon.h, tests/place_twin.py) is this build's own, exact integer arithmetic.
//
// k_place_index: one workgroup per distinct target.  Every valid k-mer of t goes into the target's open-addressing table
// (DgPlaceSlot: 32 bytes, a tag of key + 1, an occurrence count, the first DG_PLACE_MAX_OCC positions).  The tag is
// claimed by a 64-bit compare-and-swap, the count is an atomic add, and the position goes to the entry the add returned,
// so the order of positions inside a slot depends on timing: the votes below are a multiset and do not.
//
// k_place_vote: one workgroup per pair.  The query is staged through LDS a tile of DG_PLACE_THREADS positions at a time;
// each lane builds the forward k-mer of its position p and, in the same loop, the reverse-complement k-mer of
// q[p, p + k), which is rc(q)'s k-mer at i = |q| - k - p.  Both are probed in t's table, and each stored position j of an
// unmasked k-mer is one vote on diagonal d = j - i, binned as (d + |q|) >> 6.  Integer LDS atomics fill six histograms:
// per strand the total, the votes of quarter 0 and the votes of quarter 3 of the query.  Quarter histograms keep every
// bin; the +-R window around the chosen bin is applied when they are read, which is the same as counting only consistent
// votes.  The argmaxes are block reductions of (count << 32 | ~bin), so the smaller bin wins a tie.  One lane writes
// the outputs with ordinary global stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dagcon.h"

#define DG_PLACE_MAX_LEN DAGCON_PLACE_MAX_LEN
#define DG_PLACE_MAX_OCC 8u         // positions a slot keeps; max_occ is at most this
#define DG_PLACE_THREADS 256
#define DG_PLACE_BIN_SHIFT 6        // 64 diagonals per bin
#define DG_PLACE_KMAX 16u

// two 16-byte loads: {tag, count, positions 0-1}, {positions 2-7, pad}
struct __attribute__((aligned(16))) DgPlaceSlot {
    unsigned long long tag;        // 0: empty, else key + 1
    uint32_t count;                // occurrences of the key in t (may exceed DG_PLACE_MAX_OCC)
    uint16_t pos[DG_PLACE_MAX_OCC];
    uint32_t pad;
};
static_assert(sizeof(DgPlaceSlot) == 32, "DgPlaceSlot is two 16-byte loads");

struct DgPlaceParams {
    const uint8_t *blob;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    // index launch: one entry per table
    const uint32_t *tab_seq;       // sequence id of the table's target
    const uint64_t *tab_base;      // first slot of the table
    const uint32_t *tab_mask;      // slots - 1 (a power of two, at least twice the target's k-mers)
    DgPlaceSlot *slots;
    // vote launch: one entry per pair
    const uint32_t *pq, *pt;       // sequence ids
    const uint32_t *ptab;          // table of pt
    const uint32_t *pid;           // output index
    uint32_t *votes_fwd, *votes_rev, *t0, *t1;
    uint8_t *strand;
    uint32_t k, max_occ;
};

__device__ __forceinline__ uint32_t dg_place_code(uint8_t b) {
    switch (b | 0x20) {            // only 'A' and 'a' become 'a', and so on
        case 'a': return 0;
        case 'c': return 1;
        case 'g': return 2;
        case 't': return 3;
        default: return 4;
    }
}

__device__ __forceinline__ uint32_t dg_place_hash(uint32_t key, uint32_t mask) {
    return (uint32_t)(((unsigned long long)key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// codes of x[base, base + DG_PLACE_THREADS + DG_PLACE_KMAX - 1) into s_code (4 past the end of x); the caller syncs
__device__ __forceinline__ void dg_place_tile(const uint8_t *x, uint32_t len, uint32_t base, uint8_t *s_code) {
    for (uint32_t o = threadIdx.x; o < DG_PLACE_THREADS + DG_PLACE_KMAX - 1; o += DG_PLACE_THREADS)
        s_code[o] = (uint8_t)(base + o < len ? dg_place_code(x[base + o]) : 4u);
}

// the forward k-mer at tile offset o and the reverse complement of the same k bases; false if a base is invalid
__device__ __forceinline__ bool dg_place_kmer(const uint8_t *s_code, uint32_t o, uint32_t k, uint32_t &fwd, uint32_t &rev) {
    uint32_t f = 0, r = 0, bad = 0;
    for (uint32_t m = 0; m < k; m++) {
        const uint32_t c = s_code[o + m];
        bad |= c >> 2;
        f = (f << 2) | (c & 3u);
        r |= (3u - (c & 3u)) << (2u * m);
    }
    fwd = f; rev = r;
    return !bad;
}

__global__ __launch_bounds__(DG_PLACE_THREADS) void k_place_index(DgPlaceParams p) {
    __shared__ uint8_t s_code[DG_PLACE_THREADS + DG_PLACE_KMAX];
    const uint32_t tb = blockIdx.x;
    const uint32_t sid = p.tab_seq[tb];
    const uint32_t len = p.seq_len[sid], k = p.k;
    const uint8_t *t = p.blob + p.seq_off[sid];
    DgPlaceSlot *tab = p.slots + p.tab_base[tb];
    const uint32_t mask = p.tab_mask[tb];
    const uint32_t nk = len >= k ? len - k + 1 : 0;
    for (uint32_t base = 0; base < nk; base += DG_PLACE_THREADS) {
        __syncthreads();
        dg_place_tile(t, len, base, s_code);
        __syncthreads();
        const uint32_t j = base + threadIdx.x;
        uint32_t key, rev;
        if (j >= nk || !dg_place_kmer(s_code, threadIdx.x, k, key, rev)) continue;
        const unsigned long long tag = (unsigned long long)key + 1ull;
        uint32_t h = dg_place_hash(key, mask);
        for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {     // the table is at most half full
            DgPlaceSlot *s = tab + h;
            const unsigned long long old = atomicCAS(&s->tag, 0ull, tag);
            if (old == 0ull || old == tag) {
                const uint32_t c = atomicAdd(&s->count, 1u);
                if (c < DG_PLACE_MAX_OCC) s->pos[c] = (uint16_t)j;
                break;
            }
        }
    }
}

// the largest (count << 32 | ~bin) over h[lo, hi), in every thread.  red: one word per wave
__device__ __forceinline__ unsigned long long dg_place_argmax(const uint32_t *h, int lo, int hi, unsigned long long *red) {
    unsigned long long best = 0;
    for (int b = lo + (int)threadIdx.x; b < hi; b += DG_PLACE_THREADS) {
        const unsigned long long v = ((unsigned long long)h[b] << 32) | (0xFFFFFFFFu - (uint32_t)b);
        best = v > best ? v : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(best, o, 64);
        best = v > best ? v : best;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    for (int w = 0; w < DG_PLACE_THREADS / 64; w++) best = red[w] > best ? red[w] : best;
    return best;
}

__device__ __forceinline__ int dg_place_bin_of(unsigned long long v) { return (int)(0xFFFFFFFFu - (uint32_t)v); }

// dynamic LDS: 6 * nbins words, nbins = (|t| + |q| - k) / 64 + 1 for the largest pair of the launch
__global__ __launch_bounds__(DG_PLACE_THREADS) void k_place_vote(DgPlaceParams p) {
    extern __shared__ uint32_t s_hist[];
    __shared__ uint8_t s_code[DG_PLACE_THREADS + DG_PLACE_KMAX];
    __shared__ unsigned long long s_red[DG_PLACE_THREADS / 64];
    const uint32_t x = blockIdx.x;
    const uint32_t qs = p.pq[x], ts = p.pt[x], k = p.k, max_occ = p.max_occ;
    const uint32_t lq = p.seq_len[qs], lt = p.seq_len[ts];
    const uint8_t *q = p.blob + p.seq_off[qs];
    const DgPlaceSlot *tab = p.slots + p.tab_base[p.ptab[x]];
    const uint32_t mask = p.tab_mask[p.ptab[x]];
    const bool any = lq >= k && lt >= k;
    const uint32_t nb = any ? ((lt - k + lq) >> DG_PLACE_BIN_SHIFT) + 1 : 1;
    // s_hist[(s * 3 + kind) * nb + bin]: s = 0 '+', 1 '-'; kind = 0 all votes, 1 quarter 0, 2 quarter 3
    for (uint32_t o = threadIdx.x; o < 6 * nb; o += DG_PLACE_THREADS) s_hist[o] = 0;
    const uint32_t nk = any ? lq - k + 1 : 0;
    for (uint32_t base = 0; base < nk; base += DG_PLACE_THREADS) {
        __syncthreads();
        dg_place_tile(q, lq, base, s_code);
        __syncthreads();
        const uint32_t pp = base + threadIdx.x;
        uint32_t kf, kr;
        if (pp >= nk || !dg_place_kmer(s_code, threadIdx.x, k, kf, kr)) continue;
        for (uint32_t s = 0; s < 2; s++) {
            const uint32_t key = s ? kr : kf;
            const uint32_t i = s ? lq - k - pp : pp;
            const unsigned long long tag = (unsigned long long)key + 1ull;
            uint32_t h = dg_place_hash(key, mask);
            for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
                const uint4 *sp = reinterpret_cast<const uint4 *>(tab + h);
                const uint4 a = sp[0];
                const unsigned long long tg = ((unsigned long long)a.y << 32) | a.x;
                if (tg == 0ull) break;                                     // not in t
                if (tg != tag) continue;
                const uint32_t cnt = a.z;
                if (cnt > max_occ) break;                                  // a repeat: masked
                const uint4 b = cnt > 2 ? sp[1] : make_uint4(0, 0, 0, 0);
                const uint32_t w[4] = {a.w, b.x, b.y, b.z};                // two positions a word
                const uint32_t quarter = (4u * i) / lq;
                uint32_t *H = s_hist + s * 3u * nb;
                for (uint32_t c = 0; c < cnt; c++) {
                    const uint32_t j = (w[c >> 1] >> ((c & 1u) * 16u)) & 0xFFFFu;
                    const uint32_t bin = (j + lq - i) >> DG_PLACE_BIN_SHIFT;  // j - i + |q| >= k > 0
                    atomicAdd(&H[bin], 1u);
                    if (quarter == 0) atomicAdd(&H[nb + bin], 1u);
                    else if (quarter == 3) atomicAdd(&H[2 * nb + bin], 1u);
                }
                break;
            }
        }
    }
    __syncthreads();
    const unsigned long long bf = dg_place_argmax(s_hist, 0, (int)nb, s_red);
    const unsigned long long br = dg_place_argmax(s_hist + 3 * nb, 0, (int)nb, s_red);
    const uint32_t vf = (uint32_t)(bf >> 32), vr = (uint32_t)(br >> 32);
    const uint32_t sc = vf >= vr ? 0 : 1;
    const int B = dg_place_bin_of(sc ? br : bf);
    const int R = 2 + (int)((lq + 511u) / 512u);
    const int lo = B - R < 0 ? 0 : B - R, hi = B + R + 1 > (int)nb ? (int)nb : B + R + 1;
    const unsigned long long bh = dg_place_argmax(s_hist + (sc * 3 + 1) * nb, lo, hi, s_red);
    const unsigned long long bt = dg_place_argmax(s_hist + (sc * 3 + 2) * nb, lo, hi, s_red);
    if (threadIdx.x == 0) {
        const uint32_t o = p.pid[x];
        p.votes_fwd[o] = vf;
        p.votes_rev[o] = vr;
        if (vf == 0 && vr == 0) {
            p.strand[o] = '.';
            p.t0[o] = 0;
            p.t1[o] = 0;
        } else {
            const long long Bh = (bh >> 32) ? dg_place_bin_of(bh) : B, Bt = (bt >> 32) ? dg_place_bin_of(bt) : B;
            long long a0 = 64ll * Bh + 32 - (long long)lq, a1 = 64ll * Bt + 32;
            a0 = a0 < 0 ? 0 : a0 > (long long)lt ? (long long)lt : a0;
            a1 = a1 < 0 ? 0 : a1 > (long long)lt ? (long long)lt : a1;
            p.strand[o] = sc ? '-' : '+';
            p.t0[o] = (uint32_t)a0;
            p.t1[o] = (uint32_t)a1;
        }
    }
}
