// k_align_panels.hip.h -- dazcon --trace-panels: every overlap of a .las re-aligned inside its trace-point panels.
//
// DALIGNER cuts an overlap's A interval into panels of tspace bases (the first and the last may be shorter) and records,
// per panel, how many B bases go with it (the trace).  The reference re-aligns each panel (Compute_Trace_PTS,
// DazAlnProvider.cpp:349); DALIGNER is not in the tree, so the tie-breaks are this build's own: PARITY UNPINNED.  What
// is computed, per panel of t (A bases, m rows) against q (B bases, n columns): the unit-cost edit distance with both
// corners fixed,
//
//     D[0][j] = j,  D[i][0] = i,
//     D[i][j] = min(D[i-1][j-1] + (t[i-1] != q[j-1]), D[i][j-1] + 1, D[i-1][j] + 1),
//
// ties broken per cell in k_align.hip.h's order: diagonal, then a q base against a gap in t (D[i][j-1]), then a t base
// against a gap in q (D[i-1][j]); row 0 always moves left, column 0 always up.  The walk back from (m, n) gives the
// panel's columns, '-' for gaps; an overlap's alignment is its panels' concatenated.  tests/panel_twin.py is the CPU twin.
//
// k_align_panel: one wave per panel, WPB panels per workgroup.  The B side is on the lanes, C cells a lane (lane l owns
// columns j = l C + 1 .. l C + C; columns past n are computed and never read), the row loop runs over A.  The in-row
// dependency is the running minimum of k_align_band, D[i][j] = min(E[j], min_{k < j}(E[k] - k) + j) with
// E = min(diagonal, up) and E[0] = i, through dg_al_scan_min.  Two bits of direction per cell stay in LDS (R rows of
// 64 lane words): the walk back reads them there, and nothing but the aligned characters goes to HBM.  The walk is
// uniform, one code per step in a lane register; every 64 steps the characters are filled in by all lanes (ballot
// prefix counts give each step its i and j) and written backwards from the end of the panel's room in the scratch
// buffer, which holds m + n columns for every panel.
//
// k_align_panel_compact: one workgroup per overlap.  Scans its panels' lengths and copies their columns, in order, to
// the overlap's output room.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "k_align.hip.h"

struct DgPanelParams {
    const uint8_t *q, *t;          // sequence blobs
    const uint64_t *q_off, *t_off; // per panel: first B base, first A base
    const uint32_t *q_len, *t_len; // per panel: n, m (each at most the R of the kernel instance, and DAGCON_PANEL_MAX_SIDE)
    const uint64_t *scr_off;       // per panel: its room of m + n columns in qscr / tscr
    uint8_t *qscr, *tscr;          // a panel's columns end at scr_off + m + n
    uint32_t *len;                 // per panel: columns
    int32_t *dist;                 // per panel: edit distance
    const uint32_t *idx;           // the panels of this launch
    uint32_t n;
};

template <int C, int R, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_align_panel(DgPanelParams p) {
    typedef typename std::conditional<(C <= 4), uint8_t, uint16_t>::type DirT;      // 2 bits per cell
    __shared__ DirT s_dir[WPB][R * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * WPB + (uint32_t)wave;
    if (x >= p.n) return;
    const uint32_t pi = p.idx[x];
    const uint32_t m = p.t_len[pi], n = p.q_len[pi];          // host: m <= R, n <= 64 C
    const uint8_t *t = p.t + p.t_off[pi], *q = p.q + p.q_off[pi];
    DirT *dir = s_dir[wave];
    const int kb = lane * C;                                  // the lane's cells are columns kb + 1 .. kb + C
    int P[C], Q[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t j = (uint32_t)(kb + c) + 1u;
        P[c] = (int)j;                                        // row 0
        Q[c] = j <= n ? (int)q[j - 1u] : -1;
    }
    int tch = 0;                                              // t[i0 + lane]: 64 rows' characters
    for (uint32_t i = 1; i <= m; i++) {
        if (((i - 1u) & 63u) == 0) tch = i - 1u + (uint32_t)lane < m ? (int)t[i - 1u + (uint32_t)lane] : 0;
        const int tc = __builtin_amdgcn_readlane(tch, (int)((i - 1u) & 63u));
        const int left = dg_al_dpp<DG_DPP_WAVE_SHR1, 0xf>((int)i - 1, P[C - 1]);   // D[i-1][kb] (lane 0: column 0)
        int dg[C], E[C];
        int lm = 0x7fffffff;
#pragma unroll
        for (int c = 0; c < C; c++) {
            dg[c] = (c == 0 ? left : P[c - 1]) + (Q[c] != tc ? 1 : 0);
            const int up = P[c] + 1;
            E[c] = dg[c] < up ? dg[c] : up;
            const int xv = E[c] - (kb + c + 1);
            lm = xv < lm ? xv : lm;
        }
        // min over the columns in front of the lane, D[i][0] - 0 = i included
        int pm = dg_al_dpp<DG_DPP_WAVE_SHR1, 0xf>((int)i, dg_al_scan_min(lm));
        uint32_t word = 0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int j = kb + c + 1;
            const int lf = pm + j;                            // D[i][j-1] + 1
            const int up = P[c] + 1;
            const int d = E[c] < lf ? E[c] : lf;
            const uint32_t code = dg[c] == d ? 0u : lf <= up ? 1u : 2u;
            const int xv = E[c] - j;
            pm = xv < pm ? xv : pm;
            P[c] = d;
            word |= code << (2 * c);
        }
        dir[(i - 1u) * 64u + (uint32_t)lane] = (DirT)word;
    }
    int dist = (int)m;                                        // D[m][0]
    if (n > 0) {
        const uint32_t k = n - 1u;
        int v = 0;
#pragma unroll
        for (int c = 0; c < C; c++) if (k % C == (uint32_t)c) v = P[c];
        dist = __builtin_amdgcn_readlane(v, (int)(k / C));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- walk back from (m, n): codes 0 diagonal, 1 q against a gap, 2 t against a gap ----
    uint8_t *qo = p.qscr + p.scr_off[pi], *to = p.tscr + p.scr_off[pi];
    const uint32_t room = m + n;
    uint32_t i = m, j = n, len = 0, iq = m, jq = n;           // (iq, jq): where the unfilled steps begin
    int codes = 0;
    // steps s0 .. s0 + cnt - 1 (cnt <= 64) from the lane registers to the room, backwards from its end
    auto fill = [&](uint32_t s0, uint32_t cnt) {
        const bool on = (uint32_t)lane < cnt;
        const uint32_t d = on ? (uint32_t)codes : 3u;
        const bool ut = on && d != 1u, uq = on && d != 2u;
        const unsigned long long mt = __ballot(ut), mq = __ballot(uq);
        const unsigned long long lt = (1ull << lane) - 1ull;
        const uint32_t myi = iq - (uint32_t)__popcll(mt & lt), myj = jq - (uint32_t)__popcll(mq & lt);
        if (on) {
            const uint32_t at = room - 1u - (s0 + (uint32_t)lane);
            to[at] = ut ? t[myi - 1u] : (uint8_t)'-';
            qo[at] = uq ? q[myj - 1u] : (uint8_t)'-';
        }
        iq -= (uint32_t)__popcll(mt); jq -= (uint32_t)__popcll(mq);
    };
    while (i > 0 || j > 0) {
        uint32_t d;
        if (i == 0) d = 1u;
        else if (j == 0) d = 2u;
        else {
            const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)dir[(i - 1u) * 64u + (j - 1u) / C]);
            d = (w >> (2u * ((j - 1u) % C))) & 3u;
            if (d == 3u) d = 0u;                              // (never written; keeps every step inside the panel)
        }
        codes = (uint32_t)lane == (len & 63u) ? (int)d : codes;
        len++;
        if (d != 1u) i--;
        if (d != 2u) j--;
        if ((len & 63u) == 0) fill(len - 64u, 64u);
    }
    if (len & 63u) fill(len & ~63u, len & 63u);
    if (lane == 0) { p.len[pi] = len; p.dist[pi] = dist; }
}

// pass 2: overlap a's panels pb[a] .. pb[a+1]-1, their columns one after the other from out_off[a]
#define DG_PANEL_COMPACT_THREADS 256
__global__ __launch_bounds__(DG_PANEL_COMPACT_THREADS) void k_align_panel_compact(
        const uint64_t *pb, const uint64_t *scr_off, const uint32_t *p_tlen, const uint32_t *p_qlen, const uint32_t *p_len,
        const uint8_t *qscr, const uint8_t *tscr, const uint64_t *out_off, uint8_t *qaln, uint8_t *taln, uint32_t *aln_len,
        const uint32_t *idx) {
    constexpr int T = DG_PANEL_COMPACT_THREADS;
    __shared__ uint32_t s_len[T], s_pos[T];
    __shared__ uint64_t s_src[T];
    const uint32_t a = idx[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t p0 = pb[a], p1 = pb[a + 1];
    uint8_t *qo = qaln + out_off[a], *to = taln + out_off[a];
    uint64_t base = 0;
    for (uint64_t c0 = p0; c0 < p1; c0 += T) {
        const uint64_t pp = c0 + (uint64_t)tid;
        const uint32_t l = pp < p1 ? p_len[pp] : 0u;
        s_len[tid] = l; s_pos[tid] = l;
        if (pp < p1) s_src[tid] = scr_off[pp] + (uint64_t)p_tlen[pp] + p_qlen[pp] - l;     // the panel's columns end its room
        __syncthreads();
        for (int o = 1; o < T; o <<= 1) {                      // inclusive scan of the chunk's lengths
            const uint32_t v = tid >= o ? s_pos[tid - o] : 0u;
            __syncthreads();
            s_pos[tid] += v;
            __syncthreads();
        }
        const uint32_t cn = (uint32_t)(p1 - c0 < (uint64_t)T ? p1 - c0 : (uint64_t)T);
        for (uint32_t k = 0; k < cn; k++) {
            const uint32_t l = s_len[k];
            const uint64_t dst = base + s_pos[k] - l, src = s_src[k];
            for (uint32_t e = (uint32_t)tid; e < l; e += T) { qo[dst + e] = qscr[src + e]; to[dst + e] = tscr[src + e]; }
        }
        base += s_pos[cn - 1u];
        __syncthreads();
    }
    if (tid == 0) aln_len[a] = (uint32_t)base;
}
