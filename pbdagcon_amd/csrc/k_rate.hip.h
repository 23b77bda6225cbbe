// k_rate.hip.h -- dagcon_set_record_filter: how well every record's read agrees with its target over its alignment, counted
// on the device from the ops, the read bases and the target k_cigar_scan has left there (include/dagcon.h has the rule).
// The host never looks at a base; it gets four counts per record and picks the records from those.
//
// k_cigar_rate (_packed, _strand): one wave per tile of 64 ops, launched over n_tiles as k_cigar_expand is, and of its
// shape: the wave rebuilds the tile's prefix sums (dg_cg_tile), leaves per op the end of its columns, its first read /
// target base and its code in LDS, and walks the tile's columns 64 at a time with the same binary search over the 64
// ends.  Where the expansion stores a byte of each string, a lane here compares the two bytes of an M / = / X column
// (equal after clearing bit 0x20 of both: one XOR and one AND); matches and mismatches are summed per step by a ballot
// and a population count, which are wave-uniform (scalar registers).  ins and del are the tile's I and D lengths, summed
// from the ops by the DPP scan.  Lane 0 stores the tile's uint4 {match, mismatch, ins, del} with one plain vector store.
// The read base is the one the expansion would write: dg_cg_qbase<PACKED> or dg_cg_qbase_strand.
//
// k_cigar_rate_sum: one wave per record, four to a workgroup like k_cigar_scan.  The record's tile entries are taken 64
// at a time, a lane one uint4, each of the four words summed over the wave by dg_cg_scan32 and carried across rounds.  No
// atomics: a record's counts are a fixed-order sum and do not depend on scheduling.  A record that is not rated gets
// four zeros.  32 bits are enough: the four counts add up to the record's columns, which fit (only such records are rated).
//
// Out-of-bounds safety: base[r] is DG_CG_SKIP unless the host found record r conforming after cigar_judge (its ops
// consume exactly q_len read bases, pos >= 1, pos - 1 + target bases <= tlen, all totals fit 32 bits, and q_off + q_len,
// t_off + tlen lie inside the blobs); otherwise it is t_off + pos - 1, what k_cigar_expand gets as t_base.  For such a
// record the sums recomputed here from the same device copy of the ops are the scan's, so a read-base index lies in
// [0, q_len) (byte i >> 1 < (q_len + 1) / 2 packed; q_len - 1 - i mirrored), a target-base index in [pos - 1, pos - 1 +
// target bases), exactly the argument of dg_cg_expand_tile.  No base of any other record is read.  base[r] depends on the
// record alone, a wave works on one record, so the test is wave-uniform, and it stands before the kernel's one barrier:
// either all 64 lanes reach it or none.  Lanes past the tile's last column form no index.  tile_rate has n_tiles entries
// and the wave of tile i writes entry i; k_cigar_rate_sum reads a record's entries [tile_begin[r], tile_begin[r + 1])
// only when the same base[r] says they were written, and writes rate[r], r < n.
#pragma once
#include "k_cigar.hip.h"

#define DG_CG_MATCH_MASK 0x181u   // M = X: columns with a base on both sides

struct DgCigarRate {
    const uint64_t *base;          // [n] t_off of the record's target + pos - 1; DG_CG_SKIP: the record is not rated
    uint4 *tile_rate;              // [n_tiles] match, mismatch, ins, del of the tile
    uint4 *rate;                   // [n] the same of the record
};

// a wave per tile of 64 ops
template <bool PACKED, bool STRAND>
__device__ __forceinline__ void dg_cg_rate(const DgCigarParams &p, const DgCigarStrand &st, const DgCigarRate &rt) {
    static_assert(!(PACKED && STRAND), "packed bases carry no strand");
    __shared__ uint32_t s_end[64], s_q0[64], s_t0[64], s_code[64];
    const uint32_t tile = blockIdx.x;
    if (tile >= p.n_tiles) return;
    const uint4 ck = p.ckpt[tile];
    const uint32_t r = ck.w;
    const uint64_t base = rt.base[r];
    if (base == DG_CG_SKIP) return;                               // (wave-uniform: nobody reaches the barrier)
    const uint32_t lane = threadIdx.x;
    const DgCgTile tl = dg_cg_tile(p, r, tile - p.tile_begin[r], lane);
    s_end[lane] = tl.e_col;
    s_q0[lane] = ck.y + tl.e_q - tl.i_q;                          // the op's first read base
    s_t0[lane] = ck.z + tl.e_t - tl.i_t;                          // its first target base, from pos - 1
    s_code[lane] = tl.code;
    __syncthreads();
    const uint32_t n_col = (uint32_t)__builtin_amdgcn_readlane((int)tl.e_col, 63);
    const uint32_t n_ins = (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(tl.code == 1u ? tl.i_col : 0u), 63);
    const uint32_t n_del = (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(tl.code == 2u ? tl.i_col : 0u), 63);
    const uint8_t *q = p.q + p.q_off[r];
    const uint8_t *t = p.t + base;
    bool rev = false;
    uint32_t last = 0;
    if constexpr (STRAND) {                                       // (r is wave-uniform: scalar loads, once per wave)
        rev = st.rev[r] != 0;
        last = st.q_len[r] - 1u;                                  // (read only for a base index below q_len >= 1)
    }
    uint32_t n_match = 0, n_mis = 0;
    for (uint32_t c0 = 0; c0 < n_col; c0 += 64u) {                // (wave-uniform trip count: every lane reaches the ballots)
        const uint32_t c = c0 + lane;
        bool both = false, eq = false;
        if (c < n_col) {
            // the first op whose columns end past c
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t step = 32u; step; step >>= 1)
                if (s_end[lo + step - 1u] <= c) lo += step;
            const uint32_t first = lo ? s_end[lo - 1u] : 0u;
            const uint32_t kk = c - first;
            both = ((1u << s_code[lo]) & DG_CG_MATCH_MASK) != 0u;
            if (both) {
                uint8_t qb;
                if constexpr (STRAND) qb = dg_cg_qbase_strand(q, s_q0[lo] + kk, rev, last);
                else qb = dg_cg_qbase<PACKED>(q, s_q0[lo] + kk);
                eq = (((uint32_t)qb ^ (uint32_t)t[s_t0[lo] + kk]) & 0xDFu) == 0u;
            }
        }
        n_match += (uint32_t)__popcll(__ballot(both && eq));
        n_mis += (uint32_t)__popcll(__ballot(both && !eq));
    }
    if (lane == 0) rt.tile_rate[tile] = make_uint4(n_match, n_mis, n_ins, n_del);
}
__global__ __launch_bounds__(64) void k_cigar_rate(DgCigarParams p, DgCigarRate rt) { dg_cg_rate<false, false>(p, DgCigarStrand{}, rt); }
__global__ __launch_bounds__(64) void k_cigar_rate_packed(DgCigarParams p, DgCigarRate rt) { dg_cg_rate<true, false>(p, DgCigarStrand{}, rt); }
__global__ __launch_bounds__(64) void k_cigar_rate_strand(DgCigarParams p, DgCigarRate rt, DgCigarStrand st) { dg_cg_rate<false, true>(p, st, rt); }

// a wave per record (four to a workgroup)
__global__ __launch_bounds__(256) void k_cigar_rate_sum(DgCigarParams p, DgCigarRate rt) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.n) return;
    uint32_t c_m = 0, c_x = 0, c_i = 0, c_d = 0;                  // carried across rounds
    if (rt.base[r] != DG_CG_SKIP) {
        const uint64_t t0 = p.tile_begin[r], t1 = p.tile_begin[r + 1];
        for (uint64_t k = t0; k < t1; k += 64) {
            const uint4 v = k + lane < t1 ? rt.tile_rate[k + lane] : make_uint4(0u, 0u, 0u, 0u);
            c_m += (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(v.x), 63);
            c_x += (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(v.y), 63);
            c_i += (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(v.z), 63);
            c_d += (uint32_t)__builtin_amdgcn_readlane((int)dg_cg_scan32(v.w), 63);
        }
    }
    if (lane == 0) rt.rate[r] = make_uint4(c_m, c_x, c_i, c_d);
}
