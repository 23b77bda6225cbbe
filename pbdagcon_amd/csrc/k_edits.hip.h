// k_edits.hip.h -- where the consensus differs from its target (dagcon_set_edits; include/dagcon.h has the definition).
//
// What the walks and k_bp_join leave: for consensus base i of a segment, pos_out[i] = _bbMap of its best-path vertex,
// DG_POS_BB set when that vertex is a backbone vertex.  A backbone base is a target base kept, an inserted base is a base
// added, a target position between two consecutive backbone bases that neither carries is a base dropped: the gaps
// between consecutive backbone bases are the edits, and nothing is aligned.
//
//   k_ed_scan_seg<false>  a wave per segment: counts the segment's edits after the trim, writes its span [t0, t1)
//   k_ed_scan             one block (k_scan.hip.h, the scan of every growing arena): the exclusive prefix of the counts,
//                         targets in their own order, then a target's segments in theirs (the order the host lists them
//                         in); the total; DG_E_ED_OVF when the arena is too small (the batch is re-run with a larger one)
//   k_ed_scan_seg<true>   the same scan again, every surviving edit stored at its place: the order is that of the
//                         target, no atomic decides it
//
// The scan runs from the segment's end, 64 bases a step.  A lane that holds a backbone base owns the gap behind it, up to
// the next backbone base: that one is the lowest backbone lane above it in the step (a ballot), else the one the steps
// before it met, carried in (nxt_i, nxt_p) -- so an insertion run or a deletion of any length is one edit of the lane in
// front of it, whatever number of steps it crosses.  The run behind the last backbone base is that lane's too (no next
// one: an insertion at t1); the run in front of the first, and a segment without a backbone base, are lane 0's after the
// last step.  The trim is per lane, against the target's bytes in the record intake's blob and the consensus where
// k_bp_join wrote it.
#pragma once
#include "dagcon_dev.h"
#include "k_scan.hip.h"

// equal leading bytes off both sides, then equal trailing ones (exact bytes); c is relative to the segment
__device__ __forceinline__ void dg_ed_trim(const uint8_t *tb, const uint8_t *cb, uint32_t &t_pos, uint32_t &t_len, uint32_t &c, uint32_t &c_len) {
    while (t_len && c_len && tb[t_pos] == cb[c]) { t_pos++; c++; t_len--; c_len--; }
    while (t_len && c_len && tb[t_pos + t_len - 1u] == cb[c + c_len - 1u]) { t_len--; c_len--; }
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_ed_scan_seg(DgParams p) {
    if (dg_failed(p)) return;
    const uint64_t ds = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ds >= p.st->seg_top || ds >= p.seg_cap) return;
    const int lane = threadIdx.x & 63;
    const uint32_t t = p.ed_seg[ds].tgt;
    if (t >= p.T || dg_tskip(p, t)) return;
    const int32_t r0 = p.seg_r0[ds], r1 = p.seg_r1[ds];
    const uint32_t n = (uint32_t)(r1 - r0), tlen = p.tlen[t];
    const uint64_t co = p.cns_off[t] + (uint64_t)r0;
    const uint32_t *pw = p.pos_out + co;
    const uint8_t *cb = p.cns + co, *tb = p.ed_t + p.ed_tbase[t];
    const uint32_t total = WRITE ? p.ed_seg[ds].cnt : 0u;
    const uint64_t base = WRITE ? p.ed_seg[ds].off : 0ull;
    DgEdit *out = p.ed_out;
    bool have_nxt = false, bad = false;
    uint32_t nxt_i = 0, nxt_p = 0, last_p = 0, after = 0;
    for (uint32_t hi = n; hi > 0; hi = hi > 64u ? hi - 64u : 0u) {
        const uint32_t lo = hi > 64u ? hi - 64u : 0u;               // the step is bases [lo, hi), lane l holds lo + l
        const uint32_t i = lo + (uint32_t)lane;
        const uint32_t w = i < hi ? pw[i] : 0u;
        const bool bb = i < hi && (w & DG_POS_BB);
        const uint32_t P = w & ~DG_POS_BB;
        const unsigned long long m = __ballot(bb);
        const unsigned long long above = lane == 63 ? 0ull : m >> (lane + 1);
        const int nl = above ? lane + __ffsll((long long)above) : -1;   // the next backbone lane of this step
        const uint32_t np_in = (uint32_t)__shfl((int)P, nl < 0 ? lane : nl);
        const bool has_n = nl >= 0 || have_nxt;
        const uint32_t ni = nl >= 0 ? lo + (uint32_t)nl : nxt_i, np = nl >= 0 ? np_in : nxt_p;
        uint32_t t_pos = P, t_len = 0, c = i + 1u, c_len = 0;
        bool has = false;
        if (bb) {
            if (P < 1u || P > tlen || (has_n && (np <= P || np > tlen))) bad = true;   // (backbone positions rise strictly along a path)
            else {
                if (has_n) { c_len = ni - i - 1u; t_len = np - 1u - P; }
                else c_len = n - 1u - i;                                // the run behind the last backbone base: at t1
                if (t_len && c_len) dg_ed_trim(tb, cb, t_pos, t_len, c, c_len);
                has = t_len || c_len;
            }
        }
        const unsigned long long hm = __ballot(has);
        if constexpr (WRITE) {
            if (has) {
                // ascending target order: the edits of later steps and of higher lanes come behind this one
                const uint32_t behind = after + (uint32_t)__popcll(hm >> lane);
                const uint64_t at = base + total - behind;
                if (behind > total || at >= p.ed_cap) bad = true;
                else { DgEdit e; e.c_off = co + c; e.t_pos = t_pos; e.t_len = t_len; e.c_len = c_len; e.pad = 0; out[at] = e; }
            }
        }
        after += (uint32_t)__popcll(hm);
        if (m) {
            if (!have_nxt) last_p = (uint32_t)__shfl((int)P, 63 - __clzll((long long)m));
            const int f = __ffsll((long long)m) - 1;
            nxt_i = lo + (uint32_t)f; nxt_p = (uint32_t)__shfl((int)P, f);
            have_nxt = true;
        }
    }
    // in front of the first backbone base; a segment without one is one insertion at t0 = t1 = _bbMap of its first base - 1
    uint32_t t0 = 0, t1 = 0, lead = 0;
    if (have_nxt) { t0 = nxt_p - 1u; t1 = last_p; lead = nxt_i; }
    else if (n) {
        const uint32_t P = pw[0] & ~DG_POS_BB;
        if (P < 1u || P > tlen + 1u) bad = true;
        else { t0 = t1 = P - 1u; lead = n; }
    }
    if (lead) {
        after++;
        if constexpr (WRITE) {
            if (after != total || base >= p.ed_cap) bad = true;
            else if (lane == 0 && !bad) { DgEdit e; e.c_off = co; e.t_pos = t0; e.t_len = 0; e.c_len = lead; e.pad = 0; out[base] = e; }
        }
    }
    if constexpr (WRITE) { if (after != total) bad = true; }
    if (__ballot(bad)) { if (lane == 0) dg_fail_target(p, t, DG_E_INTERNAL); return; }
    if constexpr (!WRITE) {
        if (lane == 0) { p.ed_seg[ds].cnt = after; p.ed_seg[ds].t0 = t0; p.ed_seg[ds].t1 = t1; }
    }
}

// the exclusive prefix of the segments' counts in host order, one block; a failed target's segments count nothing (the
// host does not list them).  A thread takes a target and goes through its segments one by one, reading and writing
// 32-byte records: a batch of many targets with a few segments each is what this is shaped for.  One target with
// thousands of segments runs on one lane here; that case has not been measured (a prefix per segment would be the cure)
struct DgEdScanItem {
    uint64_t first;
    uint32_t ns;
    static __device__ __forceinline__ uint64_t n(const DgParams &p) { return p.T; }
    __device__ __forceinline__ unsigned long long load(const DgParams &p, const uint64_t t) {
        const bool live = !dg_tskip(p, (uint32_t)t);
        first = live ? p.seg_first[t] : 0ull;
        ns = live ? p.n_seg[t] : 0u;
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < ns; k++) sum += p.ed_seg[first + k].cnt;
        return sum;
    }
    __device__ __forceinline__ void store(const DgParams &p, const uint64_t, unsigned long long off) const {
        for (uint32_t k = 0; k < ns; k++) { p.ed_seg[first + k].off = off; off += p.ed_seg[first + k].cnt; }
    }
    static constexpr auto top = &DgParams::ed_top; static constexpr auto cap = &DgParams::ed_cap;
    static constexpr uint32_t ovf = DG_E_ED_OVF;
};
__global__ __launch_bounds__(1024) void k_ed_scan(DgParams p) { dg_block_scan<DgEdScanItem>(p); }
