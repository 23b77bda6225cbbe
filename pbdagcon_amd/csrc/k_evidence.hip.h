// k_evidence.hip.h -- how many alignments stand behind each edit (dagcon_set_edit_support; include/dagcon.h has the
// definition).  Everything read here is resident after a run: the edits (ed_seg, ed_out), the record intake's target
// bytes (ed_t, ed_tbase), the consensus (cns), and the normalised, trimmed columns the graph was built from (norm).
//
//   k_ev_windows  a wave per segment, 64 edits a step.  Forward: a lane extends its edit's window [L, R) (bounded byte
//                 loops), the join flag is L_i <= R_{i-1}, a group's gL and alt begin flow forward from its head (ballot,
//                 highest head lane at or below, one shuffle, a carry across steps).  Backward over the same steps: gR
//                 and the alt end flow back from the group's tail.  A lane reads in the second loop only what it wrote
//                 itself in the first.  Leaves one DgEvid per edit, counts zero.
//   k_ev_count    a wave per alignment: walks its columns 64 a step (k_walk.hip.h: the alignment's header, the step, the
//                 target coordinate of a column); the loop is its own.  The first group it can span is
//                 found by binary search; one group is open at a time (a group
//                 that touches the one before it, across two adjacent segments, is walked from the step of base gR - 1
//                 again), its allele index and its "still equal to alt /
//                 ref" flags are wave-uniform.  A group closes at the column of target base gR (or at the alignment's
//                 end when gR == tlen); lane 0 then adds to the head edit's counters.  The counts are integers: the
//                 order of the adds does not matter.
//   k_ev_spread   a wave per segment: a member edit takes its head's counts.
//
// Every index is checked before it is used; a violation fails the target with DG_E_INTERNAL.
#pragma once
#include "dagcon_dev.h"
#include "k_walk.hip.h"

// k_cigar_rate's comparison: equal after clearing bit 0x20 in both
__device__ __forceinline__ bool dg_ev_eq(const uint8_t a, const uint8_t b) { return ((a ^ b) & 0xDFu) == 0u; }

__global__ __launch_bounds__(256) void k_ev_windows(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t ds = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ds >= p.st->seg_top || ds >= p.seg_cap) return;
    const int lane = threadIdx.x & 63;
    const DgEdSeg sg = p.ed_seg[ds];
    const uint32_t t = sg.tgt;
    if (t >= p.T || dg_tskip(p, t)) return;
    const int32_t r0 = p.seg_r0[ds], r1 = p.seg_r1[ds];
    const uint32_t n = (uint32_t)(r1 - r0), tlen = p.tlen[t];
    const uint64_t co = p.cns_off[t] + (uint64_t)r0;
    const uint8_t *cb = p.cns + co, *tb = p.ed_t + p.ed_tbase[t];
    const uint32_t cnt = sg.cnt, t0 = sg.t0, t1 = sg.t1;
    const uint64_t base = sg.off;
    if (r1 < r0 || co + n > p.cns_cap || t0 > t1 || t1 > tlen || base > p.ed_cap || cnt > p.ed_cap - base) {
        if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
        return;
    }
    if (!cnt) return;
    const DgEdit *ed = p.ed_out + base;
    DgEvid *ev = p.evid + base;
    bool bad = false;
    // forward: windows, join flags, what flows from a group's head
    uint32_t c_R = t0, c_gL = 0, c_cL = 0, c_head = 0;
    for (uint32_t s = 0; s < cnt; s += 64u) {
        const uint32_t i = s + (uint32_t)lane;
        const bool valid = i < cnt;
        uint32_t L = 0, R = 0, cLh = 0, cRt = 0;
        if (valid) {
            const DgEdit e = ed[i];
            uint32_t lo = t0, hi = t1;
            if (i > 0) { const DgEdit b = ed[i - 1]; lo = b.t_pos + b.t_len; }
            if (i + 1u < cnt) hi = ed[i + 1].t_pos;
            const uint32_t tp = e.t_pos, tl = e.t_len, cl = e.c_len;
            const uint64_t crel = e.c_off - co;
            if (e.c_off < co || crel > n || cl > n - (uint32_t)crel || lo < t0 || hi > t1 || tp < lo || tp > hi || tl > hi - tp || !(tl || cl)) bad = true;
            else {
                const uint32_t c = (uint32_t)crel;
                L = tp; R = tp + tl;
                if ((tl == 0u) != (cl == 0u)) {
                    // a pure insertion or deletion: every place the same bytes could stand in a repeat
                    const uint8_t *u = cl ? cb + c : tb + tp;
                    const uint32_t k = cl ? cl : tl;
                    uint32_t x = k - 1u;
                    while (L > lo && dg_ev_eq(tb[L - 1u], u[x])) { L--; x = x ? x - 1u : k - 1u; }
                    x = 0;
                    while (R < hi && dg_ev_eq(tb[R], u[x])) { R++; x = x + 1u < k ? x + 1u : 0u; }
                }
                if (c < tp - L || c + cl + (R - tp - tl) > n) bad = true;     // (the bytes between edits are the same on both sides)
                else { cLh = c - (tp - L); cRt = c + cl + (R - tp - tl); }
            }
        }
        uint32_t Rp = (uint32_t)__shfl_up((int)R, 1);
        if (lane == 0) Rp = c_R;
        const bool head = valid && (i == 0u || L > Rp);
        const unsigned long long hm = __ballot(head);
        const unsigned long long below = hm & (~0ull >> (63 - lane));
        const int hl = below ? 63 - __clzll((long long)below) : lane;
        const uint32_t gL_s = (uint32_t)__shfl((int)L, hl), cL_s = (uint32_t)__shfl((int)cLh, hl);
        const uint32_t myL = below ? gL_s : c_gL, mycL = below ? cL_s : c_cL, myhead = below ? s + (uint32_t)hl : c_head;
        if (valid) {
            DgEvid r;
            r.c_lo = co + mycL; r.gL = myL; r.gR = R; r.alt_len = cRt; r.back = i - myhead;
            r.span = r.alt = r.ref = 0u; r.pad = 0u;
            ev[i] = r;
        }
        const int last = cnt - s >= 64u ? 63 : (int)(cnt - s - 1u);
        c_R = (uint32_t)__shfl((int)R, last); c_gL = (uint32_t)__shfl((int)myL, last);
        c_cL = (uint32_t)__shfl((int)mycL, last); c_head = (uint32_t)__shfl((int)myhead, last);
    }
    if (__ballot(bad)) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    // backward: what flows from a group's tail
    uint32_t c_gR = 0, c_cR = 0;
    int nxt_head = 1;
    for (uint32_t s = (cnt - 1u) & ~63u;; s -= 64u) {
        const uint32_t i = s + (uint32_t)lane;
        const bool valid = i < cnt;
        DgEvid r;
        r.c_lo = co; r.gL = r.gR = r.alt_len = 0u; r.back = 1u;
        if (valid) r = ev[i];
        const int own = valid && r.back == 0u;
        int nh = __shfl_down(own, 1);
        if (lane == 63) nh = nxt_head;
        if (i + 1u == cnt) nh = 1;
        const unsigned long long tm = __ballot(valid && nh);
        const unsigned long long above = tm >> lane;
        const int tl_ = above ? lane + __ffsll((long long)above) - 1 : lane;
        const uint32_t gR_s = (uint32_t)__shfl((int)r.gR, tl_), cR_s = (uint32_t)__shfl((int)r.alt_len, tl_);
        const uint32_t myR = above ? gR_s : c_gR, mycR = above ? cR_s : c_cR;
        if (valid) {
            const uint64_t cL = r.c_lo - co;
            if (myR < r.gL || myR > tlen || mycR < cL || mycR > n) bad = true;
            else { ev[i].gR = myR; ev[i].alt_len = mycR - (uint32_t)cL; }
        }
        c_gR = (uint32_t)__shfl((int)myR, 0); c_cR = (uint32_t)__shfl((int)mycR, 0);
        nxt_head = __shfl(own, 0);
        if (s == 0u) break;
    }
    if (__ballot(bad)) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); }
}

// the head edit of the first group at or behind edit g of [g, ee)
__device__ __forceinline__ uint64_t dg_ev_next_head(const DgParams &p, uint64_t g, const uint64_t ee) {
    while (g < ee && p.evid[g].back != 0u) g++;
    return g;
}

__global__ __launch_bounds__(256) void k_ev_count(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t a64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a64 >= p.A) return;
    const uint32_t a = (uint32_t)a64;
    const int lane = threadIdx.x & 63;
    DgWalk wk;
    if (dg_walk_open(p, a, lane, wk) != DG_WALK_GO) return;
    const uint32_t t = wk.t, lo = wk.lo, hi = wk.hi, tlen = wk.tlen, s0 = wk.s0;
    const uint32_t ns = p.n_seg[t];
    if (!ns) return;
    const uint64_t first = p.seg_first[t];
    bool bad = first + ns > p.seg_cap || first + ns > p.st->seg_top;
    uint64_t g = 0, ee = 0;
    if (!bad) {
        const DgEdSeg sa = p.ed_seg[first], sz = p.ed_seg[first + ns - 1u];
        g = sa.off; ee = sz.off + sz.cnt;
        bad = g > ee || ee > p.ed_cap || ee > *p.ed_top;
    }
    if (bad) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    if (g == ee) return;
    {
        // the first edit whose group begins where this alignment has a left flank (gL >= 1 + s0), or at base 0
        const uint32_t need = s0 ? s0 + 1u : 0u;
        uint64_t l = g, r = ee;
        while (l < r) { const uint64_t m = l + (r - l) / 2u; if (p.evid[m].gL < need) l = m + 1u; else r = m; }
        g = dg_ev_next_head(p, l, ee);
    }
    const uint8_t *tb = p.ed_t + p.ed_tbase[t];
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t tc0 = s0, c0 = lo;
    // where the step began that holds target base gR - 1 of the open group: the first group of the next segment may begin
    // at gR (segments can be adjacent, t1 == t0), and its left flank and leading insertions lie in front of base gR
    uint32_t sv_c0 = lo, sv_tc0 = s0;
    // the open group: wave-uniform
    uint32_t gL = 0, gR = 0, alt_len = 0, ai = 0;
    const uint8_t *alt = p.cns;
    bool eqA = true, eqR = true, lf = false, fresh = true;
    while (c0 < hi && g < ee) {
        bool rewind = false;
        const DgWalkStep s = dg_walk_step(wk, c0, tc0, lane);
        const bool v = s.v, isT = s.isT;
        const uint8_t qb = s.qb, tcb = s.tcb;
        const uint32_t nT = (uint32_t)__popcll(s.mT), tc = s.tc;
        const bool same = isT && dg_ev_eq(qb, tcb);
        while (g < ee) {
            if (fresh) {
                const DgEvid r = p.evid[g];
                if (r.gL > r.gR || r.gR > tlen || r.c_lo > p.cns_cap || r.alt_len > p.cns_cap - r.c_lo) { bad = true; break; }
                gL = r.gL; gR = r.gR; alt_len = r.alt_len; alt = p.cns + r.c_lo;
                ai = 0; eqA = eqR = true; lf = gL == 0u; fresh = false;
                sv_c0 = lo; sv_tc0 = s0;                                // (gR == 0: from the alignment's first column)
            }
            if ((gL ? gL - 1u : 0u) > tc0 + nT) break;                  // nothing of this group in this step
            if (gR && __ballot(isT && tc == gR - 1u)) { sv_c0 = c0; sv_tc0 = tc0; }
            const bool inA = v && qb != DG_GAP && tc >= gL && (tc < gR || (tc == gR && tcb == DG_GAP));
            const unsigned long long mA = __ballot(inA);
            const uint32_t idx = ai + (uint32_t)__popcll(mA & lt);
            const bool noA = inA && !(idx < alt_len && dg_ev_eq(qb, alt[idx]));
            const bool noR = inA && !(idx < gR - gL && dg_ev_eq(qb, tb[gL + idx]));
            if (__ballot(noA)) eqA = false;
            if (__ballot(noR)) eqR = false;
            ai += (uint32_t)__popcll(mA);
            if (gL && __ballot(same && tc == gL - 1u)) lf = true;
            bool rf = true;
            if (gR < tlen) {
                if (!__ballot(isT && tc == gR)) break;                  // base gR lies in a later step, or behind the alignment
                rf = __ballot(same && tc == gR) != 0ull;
            } else {
                if (c0 + 64u < hi) break;                               // gR == tlen: closes at the alignment's end
                if (tc0 + nT != tlen) { g = ee; break; }                // e0 != tlen: neither this group nor a later one
            }
            if (lane == 0) {
                atomicAdd(&p.evid[g].span, 1u);
                if (lf && rf && eqA && ai == alt_len) atomicAdd(&p.evid[g].alt, 1u);
                else if (lf && rf && eqR && ai == gR - gL) atomicAdd(&p.evid[g].ref, 1u);
            }
            g = dg_ev_next_head(p, g + 1u, ee);
            fresh = true;
            // a group that touches the one just closed: walk again from the step of base gR - 1 (every such step back
            // goes with one group forward, so the walk ends)
            if (g < ee && p.evid[g].gL <= gR) { c0 = sv_c0; tc0 = sv_tc0; rewind = true; break; }
        }
        if (bad) break;
        if (rewind) continue;
        tc0 += nT; c0 += 64u;
    }
    if (bad && lane == 0) dg_fail_target(p, t, DG_E_INTERNAL);
}

__global__ __launch_bounds__(256) void k_ev_spread(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t ds = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ds >= p.st->seg_top || ds >= p.seg_cap) return;
    const int lane = threadIdx.x & 63;
    const DgEdSeg sg = p.ed_seg[ds];
    if (sg.tgt >= p.T || dg_tskip(p, sg.tgt)) return;
    if (sg.off > p.ed_cap || sg.cnt > p.ed_cap - sg.off) return;       // (k_ev_windows failed the target already)
    DgEvid *ev = p.evid + sg.off;
    for (uint32_t i = (uint32_t)lane; i < sg.cnt; i += 64u) {
        const uint32_t back = ev[i].back;
        if (!back) continue;
        if (back > i) { dg_fail_target(p, sg.tgt, DG_E_INTERNAL); continue; }
        const DgEvid h = ev[i - back];
        ev[i].span = h.span; ev[i].alt = h.alt; ev[i].ref = h.ref;
    }
}
