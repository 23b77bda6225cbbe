// k_hap_calls.hip.h -- the edits of the two groups of a split target, paired (dagcon_set_hap_calls; include/dagcon.h has
// the definition, rule 11).  Runs behind the edit kernels of the batch dagcon_upload_haps derives: label 1 of a split
// target is derived target d (even), label 2 is d ^ 1, and both carry their edits against the same source target.
//
//   k_hap_calls   a wave per derived target, 64 of its edits a step, a lane per edit.  The target's edits are one stretch
//                 of ed_out (k_ed_scan places a target's segments one behind the other), the partner's the stretch next to
//                 it.  Inside a target the occupied intervals [t_pos, t_pos + max(t_len, 1)) are disjoint and rise, so a
//                 lane finds the one partner edit that can touch its own by binary search on the intervals' ends; equal
//                 place, lengths and alt bytes make it the HOM mate, any overlap a CLASH; without one the partner's
//                 segment spans say whether its consensus covers the edit (HET) or not (NOCOVER).
//
// A lane writes one state byte and one 64-bit mate (an index into ed_out, all ones: none) at its own edit's index: no
// atomics, no LDS, nothing two lanes store.  The kernel fails no target (its partner's wave reads tfail): what it finds
// out of bounds it reports as state DG_HC_BAD, which the fetch turns into DAGCON_ERR_INTERNAL.
#pragma once
#include "dagcon_dev.h"

#define DG_HC_NOCOVER 0u
#define DG_HC_HET     1u
#define DG_HC_CLASH   2u
#define DG_HC_HOM     3u
#define DG_HC_BAD     0xFFu
#define DG_HC_NONE    (~0ull)

// the stretch [e0, e1) of ed_out that holds the edits of target t's ns segments from sf on; false: out of bounds
__device__ __forceinline__ bool dg_hc_stretch(const DgParams &p, const uint64_t sf, const uint32_t ns, const uint64_t n_ed, uint64_t &e0, uint64_t &e1) {
    if (sf >= p.seg_cap || ns > p.seg_cap - sf) return false;
    const DgEdSeg &a = p.ed_seg[sf], &b = p.ed_seg[sf + ns - 1u];
    e0 = a.off; e1 = b.off + b.cnt;
    return e0 <= e1 && e1 <= n_ed;
}

__global__ __launch_bounds__(256) void k_hap_calls(DgParams p) {
    if (dg_failed(p)) return;
    const uint32_t d = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (d >= p.T || dg_tskip(p, d)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ns = p.n_seg[d];
    if (!ns) return;
    const uint64_t n_ed = *p.ed_top < p.ed_cap ? *p.ed_top : p.ed_cap;
    uint64_t e0 = 0, e1 = 0;
    if (!dg_hc_stretch(p, p.seg_first[d], ns, n_ed, e0, e1)) return;       // (no index to report at: the host's own check of the records fails the fetch)
    // the partner: its segments and its stretch; none when it failed, was not built or left no segment
    const uint32_t dp = d ^ 1u;
    uint32_t pns = dp < p.T && !dg_tskip(p, dp) ? p.n_seg[dp] : 0u;
    const uint64_t psf = pns ? p.seg_first[dp] : 0ull;
    uint64_t q0 = 0, q1 = 0;
    bool pbad = false;
    if (pns && !dg_hc_stretch(p, psf, pns, n_ed, q0, q1)) { pbad = true; pns = 0; q0 = q1 = 0; }
    const DgEdit *ed = p.ed_out;
    for (uint64_t i = e0 + lane; i < e1; i += 64u) {
        const DgEdit e = ed[i];
        const uint32_t lo = e.t_pos, hi = e.t_pos + (e.t_len ? e.t_len : 1u);
        uint32_t state = DG_HC_NOCOVER;
        uint64_t mate = DG_HC_NONE;
        // the first partner edit whose occupied interval ends behind lo: the only one that can hold lo, and the lowest
        // that can reach into [lo, hi)
        uint64_t a = q0, b = q1;
        while (a < b) {
            const uint64_t m = a + ((b - a) >> 1);
            const DgEdit x = ed[m];
            if (x.t_pos + (x.t_len ? x.t_len : 1u) > lo) b = m; else a = m + 1u;
        }
        bool bad = pbad || e.c_off > p.cns_cap || e.c_len > p.cns_cap - e.c_off;
        if (!bad && a < q1) {
            const DgEdit x = ed[a];
            if (x.t_pos < hi) {
                mate = a;
                state = DG_HC_CLASH;
                if (x.c_off > p.cns_cap || x.c_len > p.cns_cap - x.c_off) bad = true;
                else if (x.t_pos == e.t_pos && x.t_len == e.t_len && x.c_len == e.c_len) {
                    const uint8_t *u = p.cns + e.c_off, *v = p.cns + x.c_off;
                    uint32_t k = 0;
                    while (k < e.c_len && u[k] == v[k]) k++;
                    if (k == e.c_len) state = DG_HC_HOM;
                }
            }
        }
        if (!bad && mate == DG_HC_NONE) {
            // no partner edit touches it: a partner segment whose span holds the edit shows the target there
            for (uint32_t s = 0; s < pns; s++) {
                const DgEdSeg &g = p.ed_seg[psf + s];
                if (g.t0 <= e.t_pos && e.t_pos + e.t_len <= g.t1) { state = DG_HC_HET; break; }
            }
        }
        p.hc_state[i] = (uint8_t)(bad ? DG_HC_BAD : state);
        p.hc_mate[i] = bad ? DG_HC_NONE : mate;
    }
}
