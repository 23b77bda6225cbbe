// k_merge_q.hip.h -- mergeNodes (AlnGraphBoost.cpp:129-273) with EIGHT segments per wave (round 2: four).
//
// k_merge (k_merge.hip.h) gives a wave to one segment between two cut vertices and uses, on a typical visit, 2 - 4 of
// its 64 lanes: the kernel is bound by instruction issue, and almost all of the instructions are bookkeeping that
// does not care how many lanes take part.  Here a wave sweeps DQ_ROWS segments at once, one per row of DQ_W lanes (8 x 8 since round 3; 4 x 16 in round 2): the code
// is the same sweep, written for a row -- a list entry per lane of the row, ballots cut down to the row's bits,
// cross-lane reads through the row (ds_bpermute), per-row state in vector registers -- so one instruction serves
// DQ_ROWS visits as long as the rows do the same thing.  When one row merges and the others do not, the others wait
// (the wave executes the union of its rows' paths); lists longer than a row take the reference-literal
// single-lane path (dgg_*), as lists longer than a wave do in k_merge.
//
// Exactness is inherited: every row runs exactly the sweep of dg_merge_segment on its own segment, and segments
// touch disjoint state (the cut argument above k_cuts).  A visit that has something to merge is not written again
// here: it is k_merge.hip.h's dg_visit_merging (with dg_merge_in_group / dg_merge_out_group and dg_release under it),
// instantiated for a row (DgRow) where the wave kernels instantiate it for the wave (DgWave); so are the lane-0
// plumbing (DG_LANE0, dg_fail_lane0) and the fence.  What is this file's own is a different design from the wave's:
// the two-phase loop of dq_merge_segment and its one-look path, 4 + 4 entries with the record carried in the ring.
// Full-span pileups only (p.gcuts == 0).
#pragma once
#include <hip/hip_runtime.h>
#include "dagcon_dev.h"

#ifndef DQ_W
#define DQ_W 8                       // lanes of a row (round 3: 8 rows of 8 lanes; 4 x 16 / 2 x 32 -> merge 13.3 / 18.9 ms against 11.2 at configs[1])
#endif
#define DQ_ROWS (64 / DQ_W)          // rows (segments) of a wave
#define DQ_ALL ((uint32_t)((1ull << DQ_W) - 1ull))
#define DQ_LO ((1u << (DQ_W / 2)) - 1u)   // the lower half of a row: in entries of the one-look path
#ifndef DQ_RING
#define DQ_RING 16                   // the youngest queue entries of a row, in LDS: (id, out_len | in_len << 16, out_off, in_off)
#endif
typedef uint32_t qmask;              // one bit per lane of the row

__device__ __forceinline__ qmask dq_ballot(bool p) { return (qmask)((__ballot(p) >> (threadIdx.x & (64u - DQ_W))) & (unsigned long long)DQ_ALL); }
__device__ __forceinline__ int dq_rl(int v, int l) { return __shfl(v, l, DQ_W); }          // lane l of the caller's row
#define DQ_LT(lane) ((1u << (lane)) - 1u)
// the row as a lane group of the merge rule and of the merging visit (dg_merge_in_group / dg_merge_out_group,
// dg_release, dg_visit_merging: k_merge.hip.h)
struct DgRow {
    typedef qmask mask;
    static constexpr int W = DQ_W;
    static constexpr int IN_W = DQ_W;
    static constexpr bool row_text = true;
    typedef int4 qent;
    static constexpr uint32_t RING = DQ_RING;
    static __device__ __forceinline__ qent ent(int v) { return make_int4(v, -1, 0, 0); }      // (lens = -1: see dq_merge_segment)
    static __device__ __forceinline__ mask ballot(bool p) { return dq_ballot(p); }
    static __device__ __forceinline__ int rl(int v, int l) { return dq_rl(v, l); }
    static __device__ __forceinline__ int ffs(mask m) { return __ffs((int)m); }
    static __device__ __forceinline__ int popc(mask m) { return __popc(m); }
    static __device__ __forceinline__ mask lt(int lane) { return DQ_LT(lane); }
};

// what a row is doing (dq_merge_segment)
#define DQ_ST_RUN 0                  // visits that merge nothing, one after the other
#define DQ_ST_NEED 1                 // its visit has a merge group or a long list: the generic code
#define DQ_ST_END 2                  // the segment is done (or has failed)

// One segment [c_start, c_end] of target t, swept by the calling ROW (dg_merge_segment, mode DG_MM_WORKER).
// c_end = 0x7fffffff: the segment runs to the exit vertex.  Full-span pileups only: no list is shared between segments.
__device__ __forceinline__ void dq_merge_segment(const DgParams &p, const uint32_t t, const int c_start, const int c_end,
                                                 int32_t *stk_base, int *s_stk, int4 *s_ring) {
    const int lane = threadIdx.x & (DQ_W - 1);
    const uint64_t nb = p.node_base[t];
    const uint32_t NT = p.n_nodes[t];
    const bool has_end = c_end != 0x7fffffff;
    const int c_hi = has_end ? c_end : (int)NT - 1;
    DgGraph g;
    g.nd = p.nodes + nb; g.queue = p.queue + nb + c_start;
    g.pool = p.pool + p.pool_base[t]; g.pool_size = p.pool_size[t]; g.pool_top = p.pool_top + t;
    g.stk = stk_base; g.stk_words = p.stk_words;
    g.st = p.st; g.tfail = p.tfail + t; g.t = t; g.err = false;
    g.sh = 0; g.X = -1; g.sh_tab = nullptr; g.seg = 0; g.lg_cap = 0; g.lg_cnt = nullptr;
    const int X = (int)DG_TOMB;                           // (an erased entry is no vertex; none outside shared lists)
    const uint32_t N = (uint32_t)(c_hi - c_start + 1);     // vertices this worker can dequeue
    uint32_t qh = 0, qt = 1;
    // (a ring entry carries what the visit needs of its vertex's record when the one who queued the vertex had it at hand
    // -- lens = -1: not so.  The record of a queued vertex does not change before its visit: whoever could touch its lists
    // is one of its predecessors, or has one of them for a predecessor, and those have all been visited)
    if (lane == 0) { g.queue[0] = c_start; s_ring[0] = make_int4(c_start, -1, 0, 0); }
    DG_WAVE_FENCE();
    // Two phases per round, so that the rows of a wave spend their time on the same code: (A) every row runs
    // through the visits that merge nothing (one look, the FIFO bookkeeping) until it meets a visit that has a merge
    // group, or a list longer than half a row, to deal with -- rows that have met theirs wait; (B) those visits, by
    // the generic code, all rows at once.
    // (What steers a row lives in a vector register, `st`, and the loop of phase A has no way out but its condition:
    // a boolean that differs from row to row is a lane mask to the compiler, and every such mask that lives across a
    // branch costs three scalar instructions at every join behind it -- with five of them and breaks from four levels
    // deep, 115 of the 265 instructions of a visit that merges nothing were mask bookkeeping.)
    int st = DQ_ST_RUN;
    int u = -1;
    for (;;) {
        while (st == DQ_ST_RUN && qh < qt) {
            int4 qe = make_int4(0, -1, 0, 0);
            if (qt - qh <= DQ_RING) qe = s_ring[qh & (DQ_RING - 1)];
            else qe.x = g.queue[qh];
            u = qe.x;
            qh++;
            const bool in_only = u == c_end;               // the next segment's worker does the rest of that visit
            if (u < c_start || u > c_hi || (in_only && qh != qt)) {       // cannot happen (see k_cuts)
                dg_fail_lane0(g, DG_E_INTERNAL, lane);
                st = DQ_ST_END;
            } else {
                const bool skip_in = c_start != 0 && u == c_start;        // the previous segment's worker merges in[u]
                // (k_merge asks for the next vertex's record before this visit's stores go out; here the 8 registers that
                // takes cost more, in waves per SIMD, than the round trip: 17.3 ms with, 16.1 without at configs[1])
                // u's lens and list offsets: from the ring (the visit that queued u had just read them), else from its record
                uint32_t u_lens = (uint32_t)qe.y, u_out = (uint32_t)qe.z, u_inn = (uint32_t)qe.w;
                if (qe.y == -1) {
                    const uint4 ul = dg_lo16(&DG_NV(g, u)), uh = dg_hi16(&DG_NV(g, u));
                    u_lens = ul.x; u_out = DG_H2_OUTOFF(uh); u_inn = DG_H2_INOFF(uh);
                }
                const int eff_in = skip_in ? 0 : (int)(u_lens >> 16), eff_out = in_only ? 0 : (int)(u_lens & 0xffffu);
                if (eff_in > DQ_W / 2 || eff_out > DQ_W / 2) st = DQ_ST_NEED;
                else {
                    const bool is_in = lane < DQ_W / 2;
                    const int idx = lane & (DQ_W / 2 - 1);
                    const bool valid = is_in ? idx < eff_in : idx < eff_out;
                    const uint32_t ea = is_in ? u_inn + (uint32_t)idx : u_out + 2u * (uint32_t)idx;
                    int nbr = 0;
                    if (valid) nbr = (int)DG_PW(g, ea);
                    uint4 h = make_uint4(0, 0, 0, 0);
                    uint2 ho = make_uint2(0, 0);                  // out_off, in_off of an out-neighbour: for the ring, should this visit queue it
                    if (valid) h = dg_lo16(&DG_NV(g, nbr));
                    if (valid && !is_in) ho = *(reinterpret_cast<const uint2 *>(&DG_NV(g, nbr)) + 2);
                    // in lanes: out_len == 1 (low half of h.x), out lanes: in_len == 1 (high half)
                    const qmask cand = dq_ballot(valid && ((h.x >> (is_in ? 0u : 16u)) & 0xffffu) == 1u);
                    // a merge group = two candidates of one side with the same base
                    int work = 0;
                    if (__popc(cand & DQ_LO) >= 2 || __popc(cand & (DQ_ALL & ~DQ_LO)) >= 2) {
                        const int key = ((cand >> lane) & 1u) ? (DG_H_BASE(h) | (is_in ? 0 : 256)) : -1 - lane;
                        qmask m = cand;
                        while (m) {
                            const int kf = dq_rl(key, __ffs((int)m) - 1);
                            const qmask same = dq_ballot(key == kf);
                            if (__popc(same) >= 2) { work = 2; m = 0; }
                            else m &= ~same;
                        }
                    }
                    if (work) st = DQ_ST_NEED;
                    else if (in_only) st = DQ_ST_END;      // nothing to merge in front of the cut: segment done
                    else {
                        // the FIFO bookkeeping; the record of a vertex queued here is at hand, and goes into the ring
                        qt = dg_release<DgRow>(g, valid && !is_in, nbr, DG_H_PEND(h) - 1, qt, N, s_ring, make_int4(nbr, (int)h.x, (int)ho.x, (int)ho.y), lane);
                        if (qt > N) { dg_fail_lane0(g, DG_E_INTERNAL, lane); st = DQ_ST_END; }
                    }
                }
            }
        }
        if (st != DQ_ST_NEED) break;                       // the queue ran dry, the cut was reached, or something failed
        const bool skip_in = c_start != 0 && u == c_start, in_only = u == c_end;
        // (B) the visit that has something to merge: dg_visit_merging, the text the wave kernels run
        qt = dg_visit_merging<DgRow, false>(g, u, X, skip_in, in_only, 0, qt, N, s_stk, s_ring, lane);
        if (in_only) break;                               // the next segment's worker does the rest of this visit
        if (g.err) break;
        st = DQ_ST_RUN;
    }
}

// mergeNodes, DQ_ROWS = 8 (target, segment of p.cuts) pairs per wave: row r of block b sweeps pair DQ_ROWS b + r.  (Rows that take
// their pairs off a ticket counter, one after the other, were 2 - 3 ms slower at configs[1] than this grid with the
// number of pieces chosen so that the waves fill the chip a whole number of times: dagcon_upload.)
#ifndef DQ_WAVES
#define DQ_WAVES 6
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DQ_WAVES, DQ_WAVES))) void k_merge_q(DgParams p) {
    __shared__ int s_stk[DQ_ROWS][2 * DG_IN_STACK];
    __shared__ int4 s_ring[DQ_ROWS][DQ_RING];
    const uint32_t row = threadIdx.x / DQ_W;
    const uint32_t pair = blockIdx.x * DQ_ROWS + row;
    const uint32_t t = pair / p.seg_max, seg = pair % p.seg_max;
    if (t >= p.T) return;
    if (dg_failed(p) || dg_tskip(p, t)) return;
    // a row holds 8 + 8 list entries: a target far deeper than that is swept by k_merge (a wave per segment), launched
    // beside this kernel when the batch has such targets (DgParams::q_kmax; 0: every target is taken here)
    if (p.q_kmax && (uint32_t)(p.aln_begin[t + 1] - p.aln_begin[t]) > p.q_kmax) return;
    const uint32_t *crow = p.cuts + (uint64_t)t * (p.seg_max + 2u);
    const uint32_t nseg = crow[0];
    if (seg >= nseg) return;
    const int c_start = (int)crow[1 + seg];
    const int c_end = seg + 1 < nseg ? (int)crow[2 + seg] : 0x7fffffff;
    dq_merge_segment(p, t, c_start, c_end, p.stk + (uint64_t)pair * p.stk_words, s_stk[row], s_ring[row]);
}
