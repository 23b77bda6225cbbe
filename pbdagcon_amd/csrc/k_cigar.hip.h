// k_cigar.hip.h -- dagcon_upload_cigar: alignments given as (position, ungapped read, CIGAR) against target bases held
// once are expanded into the pair of gapped strings dagcon_upload takes, on the device (include/dagcon.h has the rule).
// The strings never exist on the host.
//
// k_cigar_scan: one wave per record.  The record's ops are taken 64 at a time (a tile); every lane turns its op into
// three increments -- columns, read bases, target bases -- and an inclusive wave prefix sum (DPP, 64-bit: a tile of
// 64 ops of 2^28 - 1 does not fit 32 bits) plus a carry across tiles gives the tile's checkpoint (columns, read
// bases, target bases in front of it, and the record it belongs to: the map the expansion is launched over) and, at
// the end, the record's three totals and its flags.  No lane loops over a record's ops one by one.
//
// k_cigar_expand: one wave per tile.  The tile's columns are one contiguous range of the record's strings: the wave
// recomputes the tile's prefix sums (32 bits are enough here: only records whose totals fit are expanded), leaves
// per op the end of its columns, its first read / target base and its code in LDS, and walks the range 64 columns at
// a time; a lane finds the op of its column by a binary search over the 64 ends and stores one byte of each string.
// A wave's stores are contiguous 64-byte runs; the reads of q and t are gathers that move forward with the columns.
// Only plain vector loads and stores.
//
// Out-of-bounds safety: the host expands a record only when the scan's totals say that its ops consume exactly q_len
// read bases and stay inside the target, after it has checked q_off + q_len and t_off + tlen against the blobs; the
// expansion recomputes the same sums from the same device copy of the ops, so every index it forms lies inside
// [0, q_len), [pos - 1, tlen) and [0, columns).
//
// Packed read bases (dagcon_upload_cigar_packed; k_cigar_expand_packed, k_cigar_expand_cut_packed): q holds BAM's seq
// field as it lies, two bases a byte.  Read base i of a record is nibble i of q + q_off[r]: byte i >> 1, the high
// nibble for even i, decoded by BAM's table =ACMGRSVTWYHKDBN (dg_cg_nt16: the 16 letters are two 64-bit immediates and
// a shift, no table in memory).  A record starts on a byte; the first base an op uses falls on either nibble (a soft
// clip of odd length), so every lane takes its own byte and its own nibble.  The packed kernels are the unpacked ones
// but for that one load (one body, PACKED a template parameter); scan and cut read no bases and serve both.
// Out-of-bounds safety, packed: the host admits a record only after q_off + (q_len + 1) / 2 <= q_bytes (in 64 bits)
// and, as above, after the scan's totals say that its ops consume exactly q_len read bases; a base index i formed here
// is then below q_len, and the byte index i >> 1 below (q_len + 1) / 2.
//
// Read strand (dagcon_upload_cigar_strand; k_cigar_expand_strand, k_cigar_expand_cut_strand): q holds a record's bases as
// the reads file has them and rev one byte per record; for rev[r] != 0 the ops are written against the reverse
// complement, so read base i is comp(q[q_len - 1 - i]).  A wave works on one record, so the flag is wave-uniform: it is
// loaded once per wave (a scalar load) next to the record's q_len, which is its read-base total (ckpt and totals hold
// it only per tile; the host passes q_len[]).  comp swaps A<->T, C<->G in either case and keeps every other byte: four
// compares on the byte with its case bit cleared and an XOR by the pair's difference (A^T = 0x15, C^G = 0x04), no table
// in memory.  The strand kernels are the unpacked ones but for that index and those few ALU ops (one body, STRAND a
// template parameter); scan and cut read no bases and serve all.
// Out-of-bounds safety, strand: as above a base index i formed here is below q_len, the q_len the host checked against
// the blob and passes to the kernel unchanged; 0 <= i < q_len implies 0 <= q_len - 1 - i < q_len, so the mirrored
// index stays inside the same q_off .. + q_len range.  rev and q_len have one entry per record, and r < n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DG_CG_BAD_OP 1u       // an op code above 8, or N (3)
#define DG_CG_ZERO_LEN 2u     // an op of length 0
#define DG_CG_OVERFLOW 4u     // a total past 2^32 - 1
#define DG_CG_SKIP (~0ull)    // out_off of a record that is not expanded

// BAM op codes: M 0, I 1, D 2, N 3, S 4, H 5, P 6, = 7, X 8
#define DG_CG_COL_MASK 0x187u   // M I D = X make columns
#define DG_CG_Q_MASK 0x193u     // M I S = X consume read bases
#define DG_CG_T_MASK 0x185u     // M D = X consume target bases

struct DgCigarParams {
    const uint32_t *ops;
    const uint64_t *op_begin;      // [n + 1]
    const uint64_t *tile_begin;    // [n + 1]: first tile (64 ops) of each record
    uint32_t n;                    // records
    uint32_t n_tiles;
    uint4 *totals;                 // [n] columns, read bases, target bases, DG_CG_* flags
    uint4 *ckpt;                   // [n_tiles] columns, read bases, target bases in front of the tile; its record
    // expansion
    const uint8_t *q, *t;          // the blobs
    const uint64_t *q_off;         // [n]
    const uint64_t *t_base;        // [n] t_off of the record's target + pos - 1
    const uint64_t *out_off;       // [n] DG_CG_SKIP: leave the record alone
    uint8_t *out_q, *out_t;
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dg_cg_dpp64(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}
// inclusive prefix sum over the 64 lanes (the scheme of dg_al_scan_min: four shifts inside a row, two row broadcasts)
__device__ __forceinline__ uint64_t dg_cg_scan64(uint64_t incl) {
    incl += dg_cg_dpp64<0x111, 0xf>(incl);     // row_shr:1
    incl += dg_cg_dpp64<0x112, 0xf>(incl);     // row_shr:2
    incl += dg_cg_dpp64<0x114, 0xf>(incl);     // row_shr:4
    incl += dg_cg_dpp64<0x118, 0xf>(incl);     // row_shr:8
    incl += dg_cg_dpp64<0x142, 0xa>(incl);     // row_bcast:15 into rows 1 and 3
    incl += dg_cg_dpp64<0x143, 0xc>(incl);     // row_bcast:31 into rows 2 and 3
    return incl;
}
__device__ __forceinline__ uint32_t dg_cg_scan32(uint32_t incl) {
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xa, 0xf, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xc, 0xf, false);
    return incl;
}
__device__ __forceinline__ uint64_t dg_cg_last64(uint64_t x) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}

// a wave per record (four to a workgroup)
__global__ __launch_bounds__(256) void k_cigar_scan(DgCigarParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.n) return;
    const uint64_t ob = p.op_begin[r], oe = p.op_begin[r + 1];
    const uint64_t tile0 = p.tile_begin[r];
    uint64_t c_col = 0, c_q = 0, c_t = 0;                         // carried across tiles
    uint32_t flags = 0;
    uint64_t tile = 0;
    for (uint64_t o = ob; o < oe; o += 64, tile++) {
        const bool have = o + lane < oe;
        const uint32_t op = have ? p.ops[o + lane] : 0u;
        const uint32_t code = op & 15u, len = op >> 4;
        const uint32_t bit = 1u << code;
        const bool bad = have && (code > 8u || code == 3u), zero = have && len == 0u;
        if (__ballot(bad)) flags |= DG_CG_BAD_OP;
        if (__ballot(zero)) flags |= DG_CG_ZERO_LEN;
        const uint64_t s_col = dg_cg_scan64((have && (bit & DG_CG_COL_MASK)) ? len : 0u);
        const uint64_t s_q = dg_cg_scan64((have && (bit & DG_CG_Q_MASK)) ? len : 0u);
        const uint64_t s_t = dg_cg_scan64((have && (bit & DG_CG_T_MASK)) ? len : 0u);
        if (lane == 0) p.ckpt[tile0 + tile] = make_uint4((uint32_t)c_col, (uint32_t)c_q, (uint32_t)c_t, r);
        c_col += dg_cg_last64(s_col); c_q += dg_cg_last64(s_q); c_t += dg_cg_last64(s_t);
    }
    if ((c_col | c_q | c_t) >> 32) flags |= DG_CG_OVERFLOW;
    if (lane == 0) p.totals[r] = make_uint4((uint32_t)c_col, (uint32_t)c_q, (uint32_t)c_t, flags);
}

// BAM's 4-bit base codes: "=ACMGRSV" and "TWYHKDBN", first letter in the lowest byte
__device__ __forceinline__ uint8_t dg_cg_nt16(uint32_t code) {
    const uint64_t w = (code & 8u) ? 0x4E42444B48595754ull : 0x565352474D43413Dull;
    return (uint8_t)(w >> ((code & 7u) * 8u));
}
// read base i of a record whose bases begin at q
template <bool PACKED>
__device__ __forceinline__ uint8_t dg_cg_qbase(const uint8_t *q, uint32_t i) {
    if constexpr (PACKED) return dg_cg_nt16(((uint32_t)q[i >> 1] >> ((~i & 1u) * 4u)) & 15u);
    else return q[i];
}
// the complement: A<->T, C<->G, a<->t, c<->g, any other byte as it is
__device__ __forceinline__ uint8_t dg_cg_comp(uint8_t b) {
    const uint32_t u = b & 0xDFu;                                  // case bit cleared (only letters compare equal below)
    const uint32_t x = (u == 'A' || u == 'T') ? 0x15u : (u == 'C' || u == 'G') ? 0x04u : 0u;
    return (uint8_t)(b ^ x);
}
// what the strand kernels know of a record beyond DgCigarParams (kernel arguments of their own: the struct, and with it
// the four kernels without strand, stay as they are)
struct DgCigarStrand {
    const uint8_t *rev;            // [n] != 0: the ops are written against the reverse complement of the bases
    const uint32_t *q_len;         // [n]
};
// read base i of a record of the strand kernels: last = q_len - 1 for a reverse record (wave-uniform), else unused
__device__ __forceinline__ uint8_t dg_cg_qbase_strand(const uint8_t *q, uint32_t i, bool rev, uint32_t last) {
    const uint8_t b = q[rev ? last - i : i];
    return rev ? dg_cg_comp(b) : b;
}

// The one definition of "a tile's ops, decoded and summed": lane l of the wave takes op l of the k-th tile of record r
// (nothing past the record's last op), turns it into its three increments and takes their inclusive prefix sums over
// the wave.  What a caller leaves unused (dg_cg_find: the read bases) costs nothing: the body is inlined
struct DgCgTile {
    uint32_t code;                 // BAM op code (0 for a lane past the record's ops: no increments)
    uint32_t i_col, i_q, i_t;      // the op's columns, read bases, target bases
    uint32_t e_col, e_q, e_t;      // the same summed over lanes 0 .. l
};
__device__ __forceinline__ DgCgTile dg_cg_tile(const DgCigarParams &p, uint32_t r, uint64_t k, uint32_t lane) {
    const uint64_t o = p.op_begin[r] + k * 64u, oe = p.op_begin[r + 1];
    const bool have = o + lane < oe;
    const uint32_t op = have ? p.ops[o + lane] : 0u;
    const uint32_t len = op >> 4;
    DgCgTile t;
    t.code = op & 15u;
    const uint32_t bit = have ? 1u << t.code : 0u;
    t.i_col = (bit & DG_CG_COL_MASK) ? len : 0u;
    t.i_q = (bit & DG_CG_Q_MASK) ? len : 0u;
    t.i_t = (bit & DG_CG_T_MASK) ? len : 0u;
    t.e_col = dg_cg_scan32(t.i_col);
    t.e_q = dg_cg_scan32(t.i_q); t.e_t = dg_cg_scan32(t.i_t);
    return t;
}

// The one expand body: a wave writes the columns of the k-th tile of record r (ck its checkpoint) that lie inside the
// record's columns [c0, c1), column c at oq / ot + c - c0.  k_cigar_expand asks for all of a record (c0 = 0, c1 past any
// column), k_cigar_expand_cut for a piece ([F(A), F(B)) below).
// Out-of-bounds safety, for every caller: r is a conforming record (above), so the sums recomputed here from the same
// device copy of the ops are the scan's: a read-base index lies inside [0, q_len), a target-base index inside
// [pos - 1, pos - 1 + target bases), a tile's columns inside [0, columns); a store goes to c - c0 with c0 <= c < c1 and
// c < columns, so inside the min(c1, columns) - c0 bytes the host gave the caller at oq / ot.
template <bool PACKED, bool STRAND>
__device__ __forceinline__ void dg_cg_expand_tile(const DgCigarParams &p, const DgCigarStrand &st, uint32_t r, uint64_t k, const uint4 ck,
                                                  uint32_t c0, uint32_t c1, uint8_t *oq, uint8_t *ot) {
    static_assert(!(PACKED && STRAND), "packed bases carry no strand");
    __shared__ uint32_t s_end[64], s_q0[64], s_t0[64], s_code[64];
    const uint32_t lane = threadIdx.x;
    const DgCgTile tl = dg_cg_tile(p, r, k, lane);
    s_end[lane] = tl.e_col;
    s_q0[lane] = ck.y + tl.e_q - tl.i_q;                          // the op's first read base
    s_t0[lane] = ck.z + tl.e_t - tl.i_t;                          // its first target base, from pos - 1
    s_code[lane] = tl.code;
    __syncthreads();
    const uint32_t n_col = (uint32_t)__builtin_amdgcn_readlane((int)tl.e_col, 63);
    // the tile's columns are [ck.x, ck.x + n_col) of the record: those inside [c0, c1), tile-relative
    const uint32_t c_lo = c0 > ck.x ? c0 - ck.x : 0u;
    const uint32_t c_hi = c1 > ck.x ? (c1 - ck.x < n_col ? c1 - ck.x : n_col) : 0u;
    const uint8_t *q = p.q + p.q_off[r];
    const uint8_t *t = p.t + p.t_base[r];
    bool rev = false;
    uint32_t last = 0;
    if constexpr (STRAND) {                                       // (r is wave-uniform: scalar loads, once per wave)
        rev = st.rev[r] != 0;
        last = st.q_len[r] - 1u;                                  // (read only for a base index below q_len >= 1)
    }
    for (uint32_t c = c_lo + lane; c < c_hi; c += 64u) {
        // the first op whose columns end past c
        uint32_t lo = 0;
#pragma unroll
        for (uint32_t step = 32u; step; step >>= 1)
            if (s_end[lo + step - 1u] <= c) lo += step;
        const uint32_t first = lo ? s_end[lo - 1u] : 0u;          // (an op without columns ends where it begins: never found)
        const uint32_t kk = c - first;
        const uint32_t b = 1u << s_code[lo];
        const uint32_t at = ck.x + c - c0;                        // (ck.x + c >= c0: c >= c_lo)
        if constexpr (STRAND) oq[at] = (b & DG_CG_Q_MASK) ? dg_cg_qbase_strand(q, s_q0[lo] + kk, rev, last) : (uint8_t)'-';
        else oq[at] = (b & DG_CG_Q_MASK) ? dg_cg_qbase<PACKED>(q, s_q0[lo] + kk) : (uint8_t)'-';
        ot[at] = (b & DG_CG_T_MASK) ? t[s_t0[lo] + kk] : (uint8_t)'-';
    }
}

// a wave per tile of 64 ops: all of the tile's columns, at the record's own offset
template <bool PACKED, bool STRAND>
__device__ __forceinline__ void dg_cg_expand(const DgCigarParams &p, const DgCigarStrand &st) {
    const uint32_t tile = blockIdx.x;
    if (tile >= p.n_tiles) return;
    const uint4 ck = p.ckpt[tile];
    const uint32_t r = ck.w;
    const uint64_t out = p.out_off[r];
    if (out == DG_CG_SKIP) return;                                // (wave-uniform: nobody reaches the barrier)
    dg_cg_expand_tile<PACKED, STRAND>(p, st, r, tile - p.tile_begin[r], ck, 0u, ~0u, p.out_q + out, p.out_t + out);
}
__global__ __launch_bounds__(64) void k_cigar_expand(DgCigarParams p) { dg_cg_expand<false, false>(p, DgCigarStrand{}); }
__global__ __launch_bounds__(64) void k_cigar_expand_packed(DgCigarParams p) { dg_cg_expand<true, false>(p, DgCigarStrand{}); }
__global__ __launch_bounds__(64) void k_cigar_expand_strand(DgCigarParams p, DgCigarStrand st) { dg_cg_expand<false, true>(p, st); }

// ---- records cut to windows (dagcon_upload_cigar_windows; include/dagcon.h has the rule) ----------------------------
// A piece is one (record, window) pair: the record's columns [F(A), F(B)), F(x) the first column that consumes target
// base x, F(s) = 0 and F(e) = the record's column count.  The host lists the pieces from the scan's totals (it knows
// s = pos - 1 and e = s + target bases) and gives each the two bounds relative to s: 0 <= a_rel < b_rel <= target bases.
//
// k_cigar_cut: a wave per piece.  For a bound x strictly inside the record, the tile that consumes base x is the last
// one whose checkpoint has at most x target bases in front (ckpt[].z is monotone over a record's tiles): a 64-ary
// search, every lane one checkpoint per round and a ballot.  Then one 64-lane load of that tile's ops, the prefix sums
// of k_cigar_expand, and a ballot for the op whose target bases hold x; the column follows from that lane's sums.
// No lane walks ops one by one.  Output per piece: F(A), F(B), the tile of F(A), the tile of F(B) (record-relative).
//
// k_cigar_expand_cut: a wave per (piece, tile), k_cigar_expand's table and search on the columns of the tile that lie
// inside [F(A), F(B)), written at the piece's own offset less F(A).  A record that crosses k windows is expanded k
// times from the one copy of its ops and bases.
//
// Out-of-bounds safety: pieces are listed only for conforming records (their sums fit 32 bits, consume q_len read bases
// and stay inside the target).  The host takes k_cigar_cut's four words back and refuses anything but
// F(A) <= F(B) <= columns and first tile <= last tile < the record's tiles before it plans the output: a piece's room
// is F(B) - F(A) bytes rounded up to 16, and the expansion writes column c only when F(A) <= c < F(B), at c - F(A).
// Its reads are those of k_cigar_expand: inside [0, q_len) and [pos - 1, pos - 1 + target bases).
#define DG_CG_NO_COL 0xFFFFFFFFu   // k_cigar_cut found no op for a bound (the host fails the call: never expanded)

struct DgCigarCutParams {
    const uint4 *piece;            // [n_pieces] record, a_rel, b_rel, -
    uint4 *cut;                    // [n_pieces] F(A), F(B), tile of F(A), tile of F(B)
    uint32_t n_pieces;
    // expansion
    const uint32_t *wave_piece;    // [n_waves] the piece of each wave
    const uint32_t *wave_begin;    // [n_pieces] the piece's first wave
    const uint64_t *piece_out;     // [n_pieces] where the piece's strings go
    uint32_t n_waves;
};

// the column and the tile of bound x (0 < x < the record's target bases); wave-uniform in and out
__device__ __forceinline__ void dg_cg_find(const DgCigarParams &p, uint32_t r, uint64_t tile0, uint32_t ntile, uint32_t x,
                                           uint32_t lane, uint32_t &col, uint32_t &tile) {
    uint32_t lo = 0, n = ntile;
    for (;;) {                                                    // z of tile lo is at most x throughout
        const uint32_t stride = (n + 63u) / 64u;
        const bool le = lane * stride < n && p.ckpt[tile0 + lo + lane * stride].z <= x;
        uint32_t cnt = (uint32_t)__popcll(__ballot(le));
        if (cnt == 0) cnt = 1;
        const uint32_t end = lo + n;
        lo += (cnt - 1u) * stride;
        n = end - lo < stride ? end - lo : stride;
        if (stride <= 1u) break;
    }
    tile = lo;
    const uint4 ck = p.ckpt[tile0 + lo];
    const DgCgTile tl = dg_cg_tile(p, r, lo, lane);
    const uint32_t t0 = ck.z + tl.e_t - tl.i_t;                   // the op's first target base
    const unsigned long long hit = __ballot(tl.i_t != 0u && t0 <= x && x - t0 < tl.i_t);
    const uint32_t mine = ck.x + tl.e_col - tl.i_col + (x - t0);        // (an op with target bases has a column for each)
    col = hit ? (uint32_t)__shfl((int)mine, __ffsll((long long)hit) - 1) : DG_CG_NO_COL;
}

// a wave per piece (four to a workgroup)
__global__ __launch_bounds__(256) void k_cigar_cut(DgCigarParams p, DgCigarCutParams w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pc = blockIdx.x * 4u + (threadIdx.x >> 6);     // wave-uniform
    if (pc >= w.n_pieces) return;
    const uint4 pi = w.piece[pc];
    const uint32_t r = pi.x;
    const uint4 tot = p.totals[r];
    const uint64_t tile0 = p.tile_begin[r];
    const uint32_t ntile = (uint32_t)(p.tile_begin[r + 1] - tile0);
    uint32_t ca = 0, ta = 0, cb = tot.x, tb = ntile ? ntile - 1u : 0u;
    if (ntile) {
        if (pi.y != 0u && pi.y < tot.z) dg_cg_find(p, r, tile0, ntile, pi.y, lane, ca, ta);
        if (pi.z < tot.z) dg_cg_find(p, r, tile0, ntile, pi.z, lane, cb, tb);
    }
    if (lane == 0) w.cut[pc] = make_uint4(ca, cb, ta, tb);
}

// a wave per (piece, tile of 64 ops): the tile's columns inside [F(A), F(B)), at the piece's own offset
template <bool PACKED, bool STRAND>
__device__ __forceinline__ void dg_cg_expand_cut(const DgCigarParams &p, const DgCigarCutParams &w, const DgCigarStrand &st) {
    if (blockIdx.x >= w.n_waves) return;
    const uint32_t pc = w.wave_piece[blockIdx.x];
    const uint32_t r = w.piece[pc].x;
    const uint4 cut = w.cut[pc];
    const uint32_t k = cut.z + (blockIdx.x - w.wave_begin[pc]);   // the record's k-th tile
    const uint64_t out = w.piece_out[pc];
    dg_cg_expand_tile<PACKED, STRAND>(p, st, r, k, p.ckpt[p.tile_begin[r] + k], cut.x, cut.y, p.out_q + out, p.out_t + out);
}
__global__ __launch_bounds__(64) void k_cigar_expand_cut(DgCigarParams p, DgCigarCutParams w) { dg_cg_expand_cut<false, false>(p, w, DgCigarStrand{}); }
__global__ __launch_bounds__(64) void k_cigar_expand_cut_packed(DgCigarParams p, DgCigarCutParams w) { dg_cg_expand_cut<true, false>(p, w, DgCigarStrand{}); }
__global__ __launch_bounds__(64) void k_cigar_expand_cut_strand(DgCigarParams p, DgCigarCutParams w, DgCigarStrand st) {
    dg_cg_expand_cut<false, true>(p, w, st);
}
