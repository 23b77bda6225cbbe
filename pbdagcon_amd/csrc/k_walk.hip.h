// k_walk.hip.h -- a wave walks the normalised, trimmed columns of one alignment: what k_pile_count (k_pileup.hip.h),
// k_sr_walk (k_site_reads.hip.h) and k_ev_count (k_evidence.hip.h) share.  Everything read here is resident after a run:
// norm, norm_off, n_lo, n_hi, n_start, aln_tgt.
//
//   dg_walk_open  the alignment's header.  SKIP: nothing to walk (the target is out, or the alignment is empty after the
//                 trim: the graph did not take it).  FAILED: an index is out of its range; lane 0 has failed the target
//                 with DG_E_INTERNAL.  GO: w is filled.  A kernel's own ranges (pile_begin, the segments, the edits) are
//                 checked by that kernel, behind the open.
//   dg_walk_step  the 64 columns from c0, a lane each: lanes past hi hold the gap / gap pad.  The target coordinate of a
//                 column is tc0, the target bases in front of the step, plus a population count of the ballot of the
//                 target-base columns below the lane; the caller carries tc0 += popcount(mT) to the next step.
#pragma once
#include "dagcon_dev.h"

struct DgWalk {
    uint32_t t, lo, hi, tlen;       // the target; the columns [lo, hi) of col; the target's length
    uint32_t s0;                    // target bases in front of column lo: tc0 of the first step
    const uint16_t *col;
};
enum { DG_WALK_SKIP, DG_WALK_FAILED, DG_WALK_GO };

__device__ __forceinline__ int dg_walk_open(const DgParams &p, const uint32_t a, const int lane, DgWalk &w) {
    w.t = p.aln_tgt[a];
    if (w.t >= p.T || dg_tskip(p, w.t)) return DG_WALK_SKIP;
    w.lo = p.n_lo[a]; w.hi = p.n_hi[a];
    if (w.hi <= w.lo) return DG_WALK_SKIP;
    w.tlen = p.tlen[w.t];
    const uint64_t noff = p.norm_off[a];
    const uint32_t start = p.n_start[a];
    if (w.hi == DG_REDO || noff + w.hi > p.norm_cap || start < 1u) {
        if (lane == 0) dg_fail_target(p, w.t, DG_E_INTERNAL);
        return DG_WALK_FAILED;
    }
    w.s0 = start - 1u;
    w.col = p.norm + noff;
    return DG_WALK_GO;
}

struct DgWalkStep {
    uint32_t i, c;                  // the lane's column and its cell (query byte low, target byte high)
    bool v, isT;                    // the column is one of the alignment's; it holds a target base
    uint8_t qb, tcb;
    unsigned long long mT;          // the lanes with a target base
    uint32_t tc;                    // target bases in front of this column
};

__device__ __forceinline__ DgWalkStep dg_walk_step(const DgWalk &w, const uint32_t c0, const uint32_t tc0, const int lane) {
    DgWalkStep s;
    s.i = c0 + (uint32_t)lane;
    s.v = s.i < w.hi;
    s.c = s.v ? w.col[s.i] : (uint16_t)(DG_GAP | (DG_GAP << 8));
    s.qb = (uint8_t)(s.c & 0xff); s.tcb = (uint8_t)(s.c >> 8);
    s.isT = s.v && s.tcb != DG_GAP;
    s.mT = __ballot(s.isT);
    s.tc = tc0 + (uint32_t)__popcll(s.mT & ((1ull << lane) - 1ull));
    return s;
}
