// k_keep.hip.h -- the kept part of every segment of a window, cut on the device (dagcon_set_window_keep; include/dagcon.h,
// rule 12, has the definition).
//
// What k_bp_join leaves: for consensus base i of a segment, pos_out[i] = P(i), the 1-based target position of its
// best-path vertex (DG_POS_BB on top where the edit kernels are to read it: masked here).  A window is consensus'd with an
// overlap on either side and only its core is kept: the part of a segment from its first base with P > lo up to its first
// base from there on with P > hi.  The stitch needs no more of a segment than that: 16 bytes instead of 4 a base.
//
//   k_win_keep   a wave per segment of the arena, four waves to a block (as k_ed_scan_seg addresses them).  It steps 64
//                positions at a time from the segment's front, one coalesced 256-byte load a step, two ballots, and
//                leaves the loop at i1: a window with an overlap O on both sides reads about O + core of its positions.
//                Lane 0 stores the record.  No atomics, no LDS, no scratch.
//
// dg_keep_step is the step itself, on the two ballot masks: no kernel and no device-only construct in it, so that a host
// compiler takes it as well (tests/native/keep_host.cpp runs it on the CPU; define DG_KEEP_HOST_ONLY in front).
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

// what a wave carries from step to step: whether i0 has been met, and i0
struct DgKeepState {
    uint32_t have, i0;
};

// One step of 64 bases [base, base + nvalid): m_lo / m_hi have bit l set iff P(base + l) > lo / > hi (bits at or above
// nvalid are ignored).  Only first crossings count: i0 is the lowest set lane of m_lo of the first step that has one; i1
// is the lowest lane of m_hi at or above i0 from that step on -- a base in front of i0 with P > hi does not count.
// Returns true when i1 has been met (i1 is set, the wave is done), false when the next step is to be looked at.
DG_HD_INLINE bool dg_keep_step(unsigned long long m_lo, unsigned long long m_hi, const uint32_t base, const uint32_t nvalid, DgKeepState &s, uint32_t &i1) {
    const unsigned long long vm = nvalid >= 64u ? ~0ull : ((1ull << nvalid) - 1ull);
    m_lo &= vm; m_hi &= vm;
    if (!s.have) {
        if (!m_lo) return false;
        const uint32_t f = (uint32_t)__builtin_ctzll(m_lo);
        s.have = 1u; s.i0 = base + f;
        m_hi &= ~0ull << f;                                  // the lanes in front of i0 in the step that found it
    }
    if (!m_hi) return false;
    i1 = base + (uint32_t)__builtin_ctzll(m_hi);
    return true;
}

#ifndef DG_KEEP_HOST_ONLY
#include "dagcon_dev.h"

__global__ __launch_bounds__(256) void k_win_keep(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t ds = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ds >= p.st->seg_top || ds >= p.seg_cap) return;
    const int lane = threadIdx.x & 63;
    const uint32_t t = p.keep_out[ds].x;                     // (k_bp_join: which target the segment belongs to)
    if (t >= p.T || dg_tskip(p, t)) return;
    const int32_t r0 = p.seg_r0[ds], r1 = p.seg_r1[ds];
    const uint64_t off = p.cns_off[t];
    if (r0 < 0 || r1 < r0 || (uint32_t)r1 > p.cns_len[t] || off > p.cns_cap || (uint64_t)r1 > p.cns_cap - off) {
        if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
        return;
    }
    const uint32_t n = (uint32_t)(r1 - r0);
    const uint32_t *pw = p.pos_out + off + (uint64_t)r0;
    const uint32_t lo = p.keep_lo[t], hi = p.keep_hi[t];
    DgKeepState s = {0u, 0u};
    uint32_t i1 = n;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t i = base + (uint32_t)lane;
        const uint32_t P = i < n ? pw[i] & ~DG_POS_BB : 0u;
        const unsigned long long m_lo = __ballot(i < n && P > lo), m_hi = __ballot(i < n && P > hi);
        if (dg_keep_step(m_lo, m_hi, base, n - base < 64u ? n - base : 64u, s, i1)) break;
    }
    if (lane != 0) return;
    uint4 rec = make_uint4(0u, 0u, 0u, 0u);
    if (s.have && i1 > s.i0) {
        if (i1 > n) { dg_fail_target(p, t, DG_E_INTERNAL); return; }
        rec = make_uint4(s.i0, i1, pw[s.i0] & ~DG_POS_BB, pw[i1 - 1u] & ~DG_POS_BB);
    }
    p.keep_out[ds] = rec;
}
#endif
