// k_cs.hip.h -- dagcon_upload_cs: alignments given as minimap2's cs:Z: text against target bases held once are decoded,
// on the device, into what k_cigar.hip.h takes: BAM-encoded ops and one ungapped read per record (include/dagcon.h has
// the rule).  The text is uploaded as the file has it; neither the ops nor the read exist on the host.
//
// k_cs_scan, k_cs_write: one body (dg_cs_record, WRITE a template parameter), one wave per record.  The record's text is
// taken 64 bytes at a time (a step), a lane a byte.  A ballot of the bytes  : * + - = ~  gives the op starts of the
// step; from it every lane has, in a few bit operations, the start of the op it lies in (the highest start at or below
// it, else the op left open by the step before), its place in that op's body, and the op's end inside the step (the
// lowest start above it, else the end of the step).  Bodies are judged per byte (letter, digit, place), lengths per op
// start.  A number is not walked: a digit lane multiplies its digit by 10^(bytes to the op's end), an inclusive wave
// prefix sum (k_cigar.hip.h's DPP scan) runs over these products, and the op-start lane takes the difference of the
// sums at its end and at itself.  What crosses a step is wave-uniform: the open op's byte, its body bytes so far, the
// value of its digits so far (a later step multiplies it by 10^(its digits) and adds its own sum), and the running
// counts of ops, columns, read bases and target bases.  Read bases and target bases are counted per byte where the byte
// is one (a letter of =SEQ / +SEQ / -SEQ, the * and its second letter) and per op for :n, so that a second prefix sum
// gives every lane the read index of its own byte and every :n op the read and target index it copies from.
//   k_cs_scan (WRITE = false) stores nothing but the record's totals (columns, read bases, target bases, flags: the
//   uint4 of k_cigar_scan) and its number of ops.  The host takes these back, judges every record (include/dagcon.h) and
//   lays the ops of the conforming ones out without gaps: op_begin as k_cigar_scan reads it.
//   k_cs_write (WRITE = true) tokenises the conforming records again and stores: per op start the op (lane j of the
//   step, at the record's running op count plus the starts before j), per letter of =SEQ / +SEQ / *tq the upper-cased
//   byte at its read index, and per :n op, the whole wave together, n target bytes at its read index.
// From there k_cigar_scan, k_cigar_cut, k_cigar_expand and k_cigar_expand_cut run unchanged on the device-resident ops
// and read (measured: DESIGN.md, "cs input").  Only plain vector loads and stores.
//
// Out-of-bounds safety.  The text is not trusted; nothing it says becomes an index unguarded.
//   - text: the host admits a batch only after cs_off + cs_len <= cs_bytes (64 bits); a lane reads byte base + lane only
//     when that is below cs_len.
//   - k_cs_scan stores totals[r] and n_ops[r], r < n, nothing else.
//   - k_cs_write runs a record only when the host gave it ops to write (op_begin[r + 1] > op_begin[r]), which it does
//     for records whose scan totals conform: no flag, exactly q_len read bases, pos >= 1 and pos - 1 + target bases <=
//     tlen.  The second pass reads the same device copy of the text, so it forms the same sums; on top of that every
//     store is guarded on its own: an op goes to slot i only for i < op_begin[r + 1] - op_begin[r], a read byte to index
//     i only for i < q_len[r] (the host's prefix sum of q_len gives every record its own q_len bytes of the buffer: no
//     lane writes past them), and a :n copy is cut to min(n, q_len - read index, t_room - target index), t_room = tlen -
//     (pos - 1) from the host, so target bytes are read inside [pos - 1, tlen) only.  All indexes are 64-bit sums of
//     32-bit terms over at most 2^32 bytes of text: they do not wrap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_cigar.hip.h"

#define DG_CS_BAD_OP 8u       // a ~ op, or a first byte that starts no op   (beside the DG_CG_* flags in totals[].w)
#define DG_CS_BAD_BODY 16u    // an empty body, a non-letter, a non-digit, :0, a number of 2^28 or more, a * body not of two letters

struct DgCsParams {
    const uint8_t *cs;             // the text blob
    const uint64_t *cs_off;        // [n]
    const uint32_t *cs_len;        // [n]
    uint32_t n;                    // records
    uint4 *totals;                 // [n] columns, read bases, target bases, flags (k_cs_scan)
    uint32_t *n_ops;               // [n] (k_cs_scan)
    // k_cs_write
    const uint64_t *op_begin;      // [n + 1]: where the record's ops go; an empty range: the record is left alone
    uint32_t *ops;
    const uint8_t *t;              // the target blob
    const uint64_t *t_base;        // [n] t_off of the record's target + pos - 1
    const uint32_t *t_room;        // [n] tlen - (pos - 1)
    const uint64_t *q_off;         // [n] prefix sum of q_len
    const uint32_t *q_len;         // [n]
    uint8_t *q;                    // the reads, made here
};

__device__ __forceinline__ bool dg_cs_isop(uint32_t b) {
    return b == ':' || b == '*' || b == '+' || b == '-' || b == '=' || b == '~';
}
// 10^e, e <= 9
__device__ __forceinline__ uint32_t dg_cs_pow10(uint32_t e) {
    uint32_t w = (e & 1u) ? 10u : 1u;
    if (e & 2u) w *= 100u;
    if (e & 4u) w *= 10000u;
    if (e & 8u) w *= 100000000u;
    return w;
}
__device__ __forceinline__ uint64_t dg_cs_shfl64(uint64_t x, uint32_t src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, (int)src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}
// the op of a cs token: type its first byte, len its body length, num the value of a :n
__device__ __forceinline__ uint32_t dg_cs_op(uint32_t type, uint32_t len, uint32_t num) {
    return type == ':' ? (num << 4) | 7u : type == '=' ? (len << 4) | 7u : type == '*' ? (1u << 4) | 8u
         : type == '+' ? (len << 4) | 1u : (len << 4) | 2u;
}
// q[qpos .. + n) = t[tpos .. + n), the whole wave, cut to the record's read and to its target
__device__ __forceinline__ void dg_cs_copy(uint8_t *q, const uint8_t *t, uint64_t qpos, uint64_t tpos, uint32_t n, uint32_t qlen,
                                           uint32_t troom, uint32_t lane) {
    uint64_t cnt = n;
    cnt = qpos < qlen ? (cnt < qlen - qpos ? cnt : qlen - qpos) : 0u;
    cnt = tpos < troom ? (cnt < troom - tpos ? cnt : troom - tpos) : 0u;
    for (uint64_t i = lane; i < cnt; i += 64u) q[qpos + i] = t[tpos + i];
}

template <bool WRITE>
__device__ __forceinline__ void dg_cs_record(const DgCsParams &p, uint32_t r, uint32_t lane) {
    const uint32_t len = p.cs_len[r];
    const uint8_t *txt = p.cs + p.cs_off[r];
    uint64_t ob = 0;
    uint32_t slots = 0, qlen = 0, troom = 0;
    const uint8_t *t = nullptr;
    uint8_t *q = nullptr;
    if constexpr (WRITE) {
        ob = p.op_begin[r];
        slots = (uint32_t)(p.op_begin[r + 1] - ob);
        if (slots == 0u) return;                                  // (wave-uniform) not conforming, or nothing to write
        qlen = p.q_len[r]; troom = p.t_room[r];
        t = p.t + p.t_base[r]; q = p.q + p.q_off[r];
    }
    // what crosses a step (wave-uniform)
    uint32_t c_type = 0;                                          // the open op's first byte; 0: no op yet
    uint32_t c_len = 0;                                           // its body bytes so far
    uint32_t c_num = 0;                                           // a ':' op: the value of its digits so far (below 10^9)
    uint32_t flags = 0, n_op = 0;
    uint64_t s_col = 0, s_q = 0, s_t = 0;
    for (uint64_t base = 0; base < len; base += 64u) {
        const uint64_t left = (uint64_t)len - base;
        const uint32_t nv = left < 64u ? (uint32_t)left : 64u;    // bytes of this step
        const bool last_step = left <= 64u;
        const bool valid = lane < nv;
        const uint32_t b = valid ? txt[base + lane] : 0u;
        const bool isop = valid && dg_cs_isop(b);
        const unsigned long long S = __ballot(isop);
        const unsigned long long le = S & (~0ull >> (63u - lane));    // starts at or below this lane
        const bool own = le != 0ull;                              // the lane's op starts in this step, at lane j
        const uint32_t j = own ? 63u - (uint32_t)__clzll((long long)le) : 0u;
        const uint32_t jt = (uint32_t)__shfl((int)b, (int)j);
        const uint32_t type = own ? jt : c_type;
        const uint32_t k = own ? lane - j : c_len + lane + 1u;    // place in the op: 0 its first byte, the body from 1
        const unsigned long long gt = S & (~1ull << lane);        // starts above this lane
        const uint32_t e = gt ? (uint32_t)__ffsll((long long)gt) - 1u : nv;    // where the lane's op ends in this step
        const bool complete = gt != 0ull || last_step;            // ... and whether that is the op's end
        const uint32_t fe = S ? (uint32_t)__ffsll((long long)S) - 1u : nv;     // bytes of the open op in this step
        const bool letter = ((b & 0xDFu) - (uint32_t)'A') < 26u, digit = (b - (uint32_t)'0') < 10u;
        // ---- the numbers: digit * 10^(bytes to the op's end), summed by a prefix sum
        const uint32_t place = e - 1u - lane;
        const uint32_t contrib = (valid && !isop && type == ':' && digit && place <= 8u) ? (b - (uint32_t)'0') * dg_cs_pow10(place) : 0u;
        const uint64_t P = dg_cg_scan64(contrib);
        const uint32_t num = (uint32_t)(dg_cs_shfl64(P, e - 1u) - P);         // at an op start: its digits in this step (below 10^9)
        // ---- the op left open by the step before
        const bool cc = c_type != 0u && (S != 0ull || last_step);             // it ends in this step
        uint64_t c_val = 0;
        if (c_type == ':') {
            const uint32_t part = fe ? (uint32_t)dg_cs_shfl64(P, fe - 1u) : 0u;
            c_val = (uint64_t)c_num * dg_cs_pow10(fe < 9u ? fe : 9u) + part;
            if ((uint64_t)c_len + fe > 9u) c_val = 0;             // (flagged below by the lanes past place 9)
        }
        if (cc) {
            const uint64_t lc = (uint64_t)c_len + fe;
            if (lc == 0u || (c_type == '*' && lc != 2u)) flags |= DG_CS_BAD_BODY;
            if (c_type == ':' && (lc > 9u || c_val == 0u || c_val >= (1ull << 28))) flags |= DG_CS_BAD_BODY;
            if constexpr (WRITE) {
                if (lane == 0u && n_op < slots) p.ops[ob + n_op] = dg_cs_op(c_type, (uint32_t)lc, (uint32_t)c_val);
                if (c_type == ':') dg_cs_copy(q, t, s_q, s_t, (uint32_t)c_val, qlen, troom, lane);
            }
            if (c_type == ':') { s_col += c_val; s_q += c_val; s_t += c_val; }
        }
        // ---- this step's bytes
        bool bad_op = valid && (b == '~' || (!isop && type == 0u));
        bool bad_body = false;
        uint32_t i_q = 0, i_t = 0, i_col = 0;
        if (isop) {
            const uint32_t l = e - lane - 1u;
            if (complete) {
                if (l == 0u || (b == '*' && l != 2u)) bad_body = true;
                if (b == ':') {
                    if (num == 0u || num >= (1u << 28)) bad_body = true;
                    i_q = i_t = i_col = num;
                }
            }
            if (b == '*') i_t = i_col = 1u;
        } else if (valid) {
            if (type == ':') bad_body = !digit || k > 9u;
            else if (type == '*') { bad_body = !letter || k > 2u; i_q = k == 2u ? 1u : 0u; }
            else if (type == '=') { bad_body = !letter; i_q = i_t = i_col = 1u; }
            else if (type == '+') { bad_body = !letter; i_q = i_col = 1u; }
            else if (type == '-') { bad_body = !letter; i_t = i_col = 1u; }
        }
        if (__ballot(bad_op)) flags |= DG_CS_BAD_OP;
        if (__ballot(bad_body)) flags |= DG_CS_BAD_BODY;
        const uint64_t p_col = dg_cg_scan64(i_col), p_q = dg_cg_scan64(i_q), p_t = dg_cg_scan64(i_t);
        if constexpr (WRITE) {
            if (isop && complete) {
                const uint32_t idx = n_op + (cc ? 1u : 0u) + (uint32_t)__popcll(S & ((1ull << lane) - 1ull));
                if (idx < slots) p.ops[ob + idx] = dg_cs_op(b, e - lane - 1u, num);
            }
            if (valid && !isop && i_q) {                          // a letter of =SEQ, +SEQ or the q of *tq
                const uint64_t at = s_q + p_q - 1u;
                if (at < qlen) q[at] = (uint8_t)((b - (uint32_t)'a') < 26u ? b - 32u : b);
            }
            unsigned long long C = __ballot(isop && complete && b == ':');
            while (C) {                                           // (wave-uniform) every :n of the step, the wave together
                const uint32_t jj = (uint32_t)__ffsll((long long)C) - 1u;
                C &= C - 1ull;
                const uint32_t n_j = (uint32_t)__shfl((int)num, (int)jj);
                const uint64_t q_j = s_q + dg_cs_shfl64(p_q - i_q, jj), t_j = s_t + dg_cs_shfl64(p_t - i_t, jj);
                dg_cs_copy(q, t, q_j, t_j, n_j, qlen, troom, lane);
            }
        }
        s_col += dg_cg_last64(p_col); s_q += dg_cg_last64(p_q); s_t += dg_cg_last64(p_t);
        const bool open = S != 0ull && !last_step;                // the step's last op goes on
        n_op += (cc ? 1u : 0u) + (uint32_t)__popcll(S) - (open ? 1u : 0u);
        if (S != 0ull) {
            const uint32_t jl = 63u - (uint32_t)__clzll((long long)S);
            c_type = (uint32_t)__shfl((int)b, (int)jl);
            c_len = nv - 1u - jl;
            c_num = (uint32_t)(dg_cg_last64(P) - dg_cs_shfl64(P, jl));
        } else {
            c_len += nv;
            c_num = (uint32_t)c_val;
        }
    }
    if constexpr (!WRITE) {
        if ((s_col | s_q | s_t) >> 32) flags |= DG_CG_OVERFLOW;
        if (lane == 0u) {
            p.totals[r] = make_uint4((uint32_t)s_col, (uint32_t)s_q, (uint32_t)s_t, flags);
            p.n_ops[r] = n_op;
        }
    }
}

// a wave per record (four to a workgroup)
__global__ __launch_bounds__(256) void k_cs_scan(DgCsParams p) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);      // wave-uniform
    if (r >= p.n) return;
    dg_cs_record<false>(p, r, threadIdx.x & 63u);
}
__global__ __launch_bounds__(256) void k_cs_write(DgCsParams p) {
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= p.n) return;
    dg_cs_record<true>(p, r, threadIdx.x & 63u);
}
