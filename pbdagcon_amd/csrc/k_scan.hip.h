// k_scan.hip.h -- the one-block exclusive prefix behind every growing arena of an optional output: k_ed_scan (k_edits.hip.h),
// k_pile_scan (k_pileup.hip.h) and k_sr_scan (k_site_reads.hip.h) are this text, each with an item of its own.
//
// 1,024 threads take 1,024 items a round: a __shfl_up ladder per wave, the waves' sums in s_part, the rounds before in
// s_carry.  The total goes to the arena's word of the status block, then the overflow flag is raised when it exceeds the
// arena (the host re-runs the batch with total + 1,024).
//
// An item type I is a thread's item of a round; it supplies
//   I::n(p)            how many items there are
//   it.load(p, i)      the count of item i (the item may remember what it read)
//   it.store(p, i, o)  item i's offset o goes where it belongs
//   I::top, I::cap     DgParams' members for the total's word and the arena's capacity (as GrowArena names them on the host)
//   I::ovf             the overflow flag
// load and store are called for i < n only, store after load.
#pragma once
#include "dagcon_dev.h"

template <class I>
__device__ __forceinline__ void dg_block_scan(const DgParams &p) {
    if (dg_failed(p)) return;
    __shared__ unsigned long long s_part[16], s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    const uint64_t n = I::n(p);
    for (uint64_t i0 = 0; i0 < n; i0 += 1024u) {
        const uint64_t i = i0 + threadIdx.x;
        I it;
        const unsigned long long own = i < n ? it.load(p, i) : 0ull;
        unsigned long long incl = own;
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long up = __shfl_up(incl, o); if (lane >= o) incl += up; }
        if (lane == 63) s_part[wv] = incl;
        __syncthreads();
        unsigned long long off = s_carry;
        for (int k = 0; k < wv; k++) off += s_part[k];
        off += incl - own;
        if (i < n) it.store(p, i, off);
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = off + own;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *(p.*I::top) = s_carry;
        if (s_carry > p.*I::cap) dg_fail(p, I::ovf);
    }
}
