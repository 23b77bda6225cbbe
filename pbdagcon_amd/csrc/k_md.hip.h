// k_md.hip.h -- dagcon_upload_cigar_md: SAM / BAM records that carry an MD:Z tag need no reference.  With CIGAR and SEQ
// the tag spells every target base a record touches: matches are the read's own bases, mismatches and deleted bases are
// letters of the text.  The kernels here rebuild the target blob T on the device (include/dagcon.h has the rule) before
// the record intake of k_cigar.hip.h runs on it unchanged; T never exists on the host unless dagcon_fetch_md_targets asks.
//
// k_md_scan, k_md_write, k_md_check: one body (dg_md_record, MODE a template parameter), one wave per record.  The
// record's text is taken 64 bytes at a time (a step), a lane a byte.  Three ballots give the digit, letter and ^ classes
// of the step.  Every byte is judged against the class of the byte in front of it (the bit below it in the ballots; for
// lane 0 a wave-uniform carry): a digit may not follow ^, a letter may follow a digit, a ^, or a letter of a deletion,
// a ^ follows a digit only, any other byte is refused; the text begins and ends with a digit.  A letter belongs to a
// deletion iff the nearest non-letter at or below it is ^: the highest set bit of the non-letter mask below the lane,
// looked up in the ^ ballot; when the step has no non-letter below the lane, a wave-uniform flag carried from the steps
// before says so.  A number is not walked: a digit lane multiplies its digit by 10^(bytes to the end of its run), an
// inclusive wave prefix sum (k_cigar.hip.h's DPP scan) runs over these products, and the lane at the run's start takes
// the difference of the sums at the run's end and in front of itself.  A run the step cuts is carried (its value and its
// digit count, wave-uniform); the step it ends in multiplies the value by 10^(its leading digits) and adds their sum.
// A second prefix sum, over the numbers at their first digits and 1 at every letter, gives every letter its target
// offset k, counted from the record's pos - 1.
//   k_md_scan stores per record the bases covered, the letters and the flags, nothing else.  The host takes these back
//   and judges every record (include/dagcon.h): the grammar, and covered == the target bases the CIGAR consumes.
//   k_md_write tokenises the conforming records again and stores every letter to T[t_base + k] and a 1 to mark[t_base +
//   k], one mark byte per target base.  Two records that spell different letters at one position race; one store wins.
//   k_md_check tokenises once more and compares every letter with T: a loser of that race finds a difference and stores
//   1 to conflict[target of r].  Whether a difference exists does not depend on who won.
//
// k_md_fill, k_md_fill_check: a wave per 64-op tile of a conforming record, on dg_cg_tile and the walk of
// dg_cg_expand_tile over the tile's columns (PACKED a template parameter, through dg_cg_qbase).  Fill: for every M / = /
// X column whose mark is 0, T[ti] = the read base.  Check: where T[ti] differs from the read base at an unmarked
// position, conflict[target of r] = 1 (again the loser of a race of plain stores sees it).  A marked position is left
// alone by both: the letter wins.
// Only plain vector loads and stores, no atomics.
//
// Out-of-bounds safety.  The text is not trusted; nothing it says becomes an index unguarded.
//   - text: the host admits a batch only after md_off + md_len <= md_bytes (64 bits); a lane reads byte base + lane only
//     when that is below md_len.
//   - k_md_scan stores totals[r], r < n, nothing else.
//   - k_md_write and k_md_check run a record only when the host gave it a t_base other than DG_CG_SKIP, which it does
//     for records whose scan totals conform: no flag, covered == the CIGAR's target total nt, pos >= 1 and pos - 1 + nt <=
//     tlen (so t_base + nt <= t_off + tlen <= t_bytes, the size of T and of mark).  The later passes read the same device
//     copy of the text, so they form the same sums; on top of that every store and every load of T and mark is guarded
//     on its own by k < nt[r], the CIGAR's total the host passes.
//   - k_md_fill and k_md_fill_check skip a tile whose record has t_base == DG_CG_SKIP.  For the others the sums
//     recomputed from the device copy of the ops are the scan's (k_cigar.hip.h): a read-base index lies inside [0, q_len),
//     a target-base index ti inside [0, nt); the accesses of T and mark are guarded by ti < nt[r] all the same.
//   - conflict has one byte per target and tgt[r] < n_targets comes from the host's rec_begin.
//   The host refuses target ranges that are not ascending and disjoint, so no two targets share a byte of T.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_cigar.hip.h"
#include "k_cs.hip.h"

#define DG_MD_BAD 8u          // the text breaks the grammar   (beside DG_CG_OVERFLOW in totals[].z)

struct DgMdParams {
    const uint8_t *md;             // the text blob
    const uint64_t *md_off;        // [n]
    const uint32_t *md_len;        // [n]
    uint32_t n;                    // records
    uint4 *totals;                 // [n] bases covered, letters, flags, 0 (k_md_scan)
    // k_md_write, k_md_check, k_md_fill, k_md_fill_check
    uint8_t *t;                    // the target blob, made here
    uint8_t *mark;                 // one byte per byte of t: 1: a letter of some record spells it
    const uint64_t *t_base;        // [n] t_off of the record's target + pos - 1; DG_CG_SKIP: leave the record alone
    const uint32_t *nt;            // [n] the target bases the record's CIGAR consumes
    const uint32_t *tgt;           // [n] the record's target
    uint8_t *conflict;             // [n_targets]
};

enum { DG_MD_SCAN = 0, DG_MD_WRITE = 1, DG_MD_CHECK = 2 };
// the class of a byte, as the byte behind it sees it
enum { DG_MD_START = 0, DG_MD_DIGIT = 1, DG_MD_LETTER = 2, DG_MD_CARET = 3, DG_MD_OTHER = 4 };

template <int MODE>
__device__ __forceinline__ void dg_md_record(const DgMdParams &p, uint32_t r, uint32_t lane) {
    const uint32_t len = p.md_len[r];
    const uint8_t *txt = p.md + p.md_off[r];
    uint64_t tb = 0;
    uint32_t room = 0;
    if constexpr (MODE != DG_MD_SCAN) {
        tb = p.t_base[r];
        if (tb == DG_CG_SKIP) return;                             // (wave-uniform) not conforming
        room = p.nt[r];
    }
    // what crosses a step (wave-uniform)
    uint32_t c_prev = DG_MD_START;                                // the class of the last byte
    bool c_del = false;                                           // the nearest non-letter so far is ^
    uint32_t c_num = 0, c_dig = 0;                                // a number the step cut: its value (below 10^9), its digits (capped at 10)
    uint32_t flags = 0, n_let = 0;
    uint64_t s_t = 0;                                             // target bases covered so far
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t lm1 = lane ? lane - 1u : 0u;
    for (uint64_t base = 0; base < len; base += 64u) {
        const uint64_t left = (uint64_t)len - base;
        const uint32_t nv = left < 64u ? (uint32_t)left : 64u;    // bytes of this step
        const bool last_step = left <= 64u;
        const bool valid = lane < nv;
        const uint32_t b = valid ? txt[base + lane] : 0u;
        const bool digit = valid && (b - (uint32_t)'0') < 10u;
        const bool letter = valid && ((b & 0xDFu) - (uint32_t)'A') < 26u;
        const bool caret = valid && b == (uint32_t)'^';
        const unsigned long long Vm = ~0ull >> (64u - nv);
        const unsigned long long Dm = __ballot(digit), Lm = __ballot(letter), Cm = __ballot(caret);
        const unsigned long long NL = Vm & ~Lm, ND = Vm & ~Dm;
        // ---- every byte against the byte in front of it
        const uint32_t pc = lane == 0u ? c_prev
                          : ((Dm >> lm1) & 1ull) ? DG_MD_DIGIT : ((Lm >> lm1) & 1ull) ? DG_MD_LETTER : ((Cm >> lm1) & 1ull) ? DG_MD_CARET : DG_MD_OTHER;
        const unsigned long long nl_below = NL & below;
        const bool in_del = nl_below ? ((Cm >> (63u - (uint32_t)__clzll((long long)nl_below))) & 1ull) != 0ull : c_del;
        bool bad = false;
        if (digit) bad = pc == DG_MD_CARET;
        else if (letter) bad = pc == DG_MD_START || (pc == DG_MD_LETTER && !in_del);
        else if (caret) bad = pc != DG_MD_DIGIT;
        else if (valid) bad = true;
        // ---- the numbers: digit * 10^(bytes to the end of its run), summed by a prefix sum
        const unsigned long long gt = ND & (~1ull << lane);       // non-digits above this lane
        const uint32_t e = gt ? (uint32_t)__ffsll((long long)gt) - 1u : nv;    // where the lane's run ends in this step
        const uint32_t place = e - 1u - lane;
        const uint32_t contrib = (digit && place <= 8u) ? (b - (uint32_t)'0') * dg_cs_pow10(place) : 0u;
        const uint64_t P = dg_cg_scan64(contrib);
        const unsigned long long nd_below = ND & below;
        const uint32_t s = nd_below ? 64u - (uint32_t)__clzll((long long)nd_below) : 0u;    // where the lane's run starts in this step
        const bool from_carry = nd_below == 0ull && c_prev == DG_MD_DIGIT;                // ... or that it began in a step before
        if (digit && lane - s + (from_carry ? c_dig : 0u) > 8u) bad = true;               // a tenth digit
        const bool complete = gt != 0ull || last_step;            // the lane's run ends in this step
        const uint32_t num = (uint32_t)(dg_cs_shfl64(P, e - 1u) - P) + contrib;           // at a run's first digit: its value (below 10^9)
        uint32_t i_t = letter ? 1u : 0u;
        if (digit && lane == s && !from_carry && complete) {
            if (num >= (1u << 28)) bad = true;
            i_t = num;
        }
        // ---- the number the step before cut
        const uint32_t fe = ND ? (uint32_t)__ffsll((long long)ND) - 1u : nv;              // its digits in this step
        uint64_t c_val = 0;
        uint32_t c_cnt = 0;
        if (c_prev == DG_MD_DIGIT) {
            c_cnt = c_dig + fe > 10u ? 10u : c_dig + fe;
            const uint32_t part = fe ? (uint32_t)dg_cs_shfl64(P, fe - 1u) : 0u;
            if (c_cnt <= 9u) c_val = (uint64_t)c_num * dg_cs_pow10(fe) + part;            // (more: flagged above by the lanes past place 9)
            if (fe < nv || last_step) {                           // it ends here, in front of every letter of the step
                if (c_val >= (1ull << 28)) flags |= DG_MD_BAD;
                s_t += c_val;
            }
        }
        if (__ballot(bad)) flags |= DG_MD_BAD;
        const uint64_t p_t = dg_cg_scan64(i_t);
        if constexpr (MODE != DG_MD_SCAN) {
            const uint64_t k = s_t + p_t - 1u;                    // a letter's own target base
            if (letter && k < room) {
                if constexpr (MODE == DG_MD_WRITE) {
                    p.t[tb + k] = (uint8_t)b;
                    p.mark[tb + k] = 1u;
                } else {
                    if (p.t[tb + k] != (uint8_t)b) p.conflict[p.tgt[r]] = 1u;
                }
            }
        }
        s_t += dg_cg_last64(p_t);
        n_let += (uint32_t)__popcll(Lm);
        // ---- what the next step needs
        const unsigned long long top = 1ull << (nv - 1u);
        if (ND != 0ull) {
            const uint32_t jl = 63u - (uint32_t)__clzll((long long)ND);
            c_num = (uint32_t)(dg_cg_last64(P) - dg_cs_shfl64(P, jl));
            c_dig = nv - 1u - jl;
        } else if (c_prev == DG_MD_DIGIT) {
            c_num = (uint32_t)c_val;
            c_dig = c_cnt;
        } else {
            c_num = (uint32_t)dg_cg_last64(P);
            c_dig = 10u;                                          // (a whole step of digits: flagged above)
        }
        if (NL != 0ull) c_del = ((Cm >> (63u - (uint32_t)__clzll((long long)NL))) & 1ull) != 0ull;
        c_prev = (Dm & top) ? DG_MD_DIGIT : (Lm & top) ? DG_MD_LETTER : (Cm & top) ? DG_MD_CARET : DG_MD_OTHER;
    }
    if constexpr (MODE == DG_MD_SCAN) {
        if (c_prev != DG_MD_DIGIT) flags |= DG_MD_BAD;            // an empty text, or one that does not end with a number
        if (s_t >> 32) flags |= DG_CG_OVERFLOW;
        if (lane == 0u) p.totals[r] = make_uint4((uint32_t)s_t, n_let, flags, 0u);
    }
}

// a wave per record (four to a workgroup)
__global__ __launch_bounds__(256) void k_md_scan(DgMdParams p) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.n) return;
    dg_md_record<DG_MD_SCAN>(p, r, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void k_md_write(DgMdParams p) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= p.n) return;
    dg_md_record<DG_MD_WRITE>(p, r, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void k_md_check(DgMdParams p) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= p.n) return;
    dg_md_record<DG_MD_CHECK>(p, r, threadIdx.x & 63u);
}

#define DG_MD_MATCH_MASK 0x181u   // M = X: a column with a read base and a target base

// a wave per tile of 64 ops: the tile's M / = / X columns at unmarked positions (k_cigar_expand's table and search)
template <bool PACKED, bool CHECK>
__device__ __forceinline__ void dg_md_fill(const DgCigarParams &p, const DgMdParams &m) {
    __shared__ uint32_t s_end[64], s_q0[64], s_t0[64], s_code[64];
    const uint32_t tile = blockIdx.x;
    if (tile >= p.n_tiles) return;
    const uint4 ck = p.ckpt[tile];
    const uint32_t r = ck.w;
    const uint64_t tb = m.t_base[r];
    if (tb == DG_CG_SKIP) return;                                 // (wave-uniform: nobody reaches the barrier)
    const uint32_t room = m.nt[r];
    const uint32_t lane = threadIdx.x;
    const DgCgTile tl = dg_cg_tile(p, r, tile - p.tile_begin[r], lane);
    s_end[lane] = tl.e_col;
    s_q0[lane] = ck.y + tl.e_q - tl.i_q;                          // the op's first read base
    s_t0[lane] = ck.z + tl.e_t - tl.i_t;                          // its first target base, from pos - 1
    s_code[lane] = tl.code;
    __syncthreads();
    const uint32_t n_col = (uint32_t)__builtin_amdgcn_readlane((int)tl.e_col, 63);
    const uint8_t *q = p.q + p.q_off[r];
    for (uint32_t c = lane; c < n_col; c += 64u) {
        // the first op whose columns end past c
        uint32_t lo = 0;
#pragma unroll
        for (uint32_t step = 32u; step; step >>= 1)
            if (s_end[lo + step - 1u] <= c) lo += step;
        const uint32_t kk = c - (lo ? s_end[lo - 1u] : 0u);
        if (!((1u << s_code[lo]) & DG_MD_MATCH_MASK)) continue;
        const uint32_t ti = s_t0[lo] + kk;
        if (ti >= room || m.mark[tb + ti] != 0u) continue;
        const uint8_t qb = dg_cg_qbase<PACKED>(q, s_q0[lo] + kk);
        if constexpr (CHECK) {
            if (m.t[tb + ti] != qb) m.conflict[m.tgt[r]] = 1u;
        } else {
            m.t[tb + ti] = qb;
        }
    }
}
__global__ __launch_bounds__(64) void k_md_fill(DgCigarParams p, DgMdParams m) { dg_md_fill<false, false>(p, m); }
__global__ __launch_bounds__(64) void k_md_fill_packed(DgCigarParams p, DgMdParams m) { dg_md_fill<true, false>(p, m); }
__global__ __launch_bounds__(64) void k_md_fill_check(DgCigarParams p, DgMdParams m) { dg_md_fill<false, true>(p, m); }
__global__ __launch_bounds__(64) void k_md_fill_check_packed(DgCigarParams p, DgMdParams m) { dg_md_fill<true, true>(p, m); }
