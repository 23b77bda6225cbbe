// k_norm_run.hip.h -- normalizeGaps (Alignment.cpp:131-217) on one chunk of an alignment: the loop a lane of
// k_norm_chunk runs.  No kernel and no device-only construct in here, so that a host compiler takes the file as
// well (tests/native/norm_run_host.cpp runs both forms on the CPU).
//
//   dg_norm_run<NW>   the column-by-column push loop on a window of NW columns: the second pass (NW = 512)
//   dg_norm_run_gc    the first pass, 64-column window: visits only the gap columns, found with two bit masks
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DG_HD __host__ __device__
#define DG_HD_INLINE __host__ __device__ __forceinline__
typedef uint4 dg_u4;
#define DG_MAKE_U4(a, b, c, d) make_uint4((a), (b), (c), (d))
#else
#define DG_HD
#define DG_HD_INLINE inline __attribute__((always_inline))
struct __attribute__((may_alias, aligned(16))) dg_u4 { uint32_t x, y, z, w; };
static inline dg_u4 DG_MAKE_U4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { dg_u4 v; v.x = a; v.y = b; v.z = c; v.w = d; return v; }
#endif
#ifndef DG_GAP
#define DG_GAP '-'
#endif

// a column: low byte = query char, high byte = target char
#define DG_COL(qb, tb) ((uint16_t)((uint16_t)(qb) | ((uint16_t)(tb) << 8)))
#define DG_Q(c) ((uint8_t)((c) & 0xff))
#define DG_T(c) ((uint8_t)((c) >> 8))

#ifndef DG_NCH
#define DG_NCH 512u            // input columns per window (1024: +1.4 ms at configs[1], 256: the same, 128: +1.3 ms)
#endif
#define DG_CH_NONE 0xFFFFFFFFu

DG_HD_INLINE bool dg_match_col(uint8_t qb, uint8_t tb) { return qb == tb && qb != DG_GAP && qb != '.'; }

// column a chunk starts at inside window c of the alignment, DG_CH_NONE if there is none
DG_HD inline uint32_t dg_chunk_start(const uint8_t *q, const uint8_t *t, uint32_t len, uint32_t c) {
    if (c == 0) return 0;
    const uint64_t w0 = (uint64_t)c * DG_NCH;
    if (w0 >= len) return DG_CH_NONE;
    const uint32_t hi = (uint64_t)len < w0 + DG_NCH ? len : (uint32_t)(w0 + DG_NCH);
    for (uint32_t k = (uint32_t)w0; k < hi; k++) {
        const uint8_t b = q[k];
        if (dg_match_col(b, t[k]) && b != q[k - 1] && dg_match_col(q[k - 1], t[k - 1]) && dg_match_col(q[k - 2], t[k - 2]))
            return k;
    }
    return DG_CH_NONE;
}

// The chunk scratch, in uint16 columns.  Main part: two columns per input column of the batch (tmp_cols) at the
// chunk's own place, 8 more per window so that every chunk's stretch starts on a 16-byte boundary; behind it the
// re-run region, a sixteenth of that and no less than 2^20 columns (k_norm_chunk's ovf_top counts into it).
DG_HD_INLINE uint64_t dg_tmp_main(const uint64_t tmp_cols, const uint64_t n_chunks) {
    return (2ull * tmp_cols + 8ull * n_chunks + 15ull) & ~7ull;
}
DG_HD_INLINE uint64_t dg_tmp_region(const uint64_t tmp_main) {
    return tmp_main / 16 > (1ull << 20) ? tmp_main / 16 : 1ull << 20;
}
DG_HD_INLINE uint64_t dg_tmp_cap(const uint64_t tmp_main) { return tmp_main + dg_tmp_region(tmp_main); }

// A seam for the CPU model of the stage (tests/native/norm_stage_host.cpp), which defines this macro before it includes
// the header to read dg_norm_run's window cursors after every refill: the largest e - i and how often the ring came
// round.  Nobody else defines it: here, and in every build of the library, it expands to nothing and the loop is unchanged.
#ifndef DG_NORM_RUN_PROBE
#define DG_NORM_RUN_PROBE(e, i)
#endif

struct DgChunkRun { uint32_t w, tb; bool dirty, overflow, badchar; };

// normalizeGaps (Alignment.cpp:142-214) on the input columns [k0, k1) of an alignment, started
// cold; the look-ahead may read (and, reported as `dirty`, write) beyond k1.
template <uint32_t NW>
DG_HD inline DgChunkRun dg_norm_run(const uint8_t *q, const uint8_t *t, const uint32_t len, const uint32_t k0,
                                    const uint32_t k1, uint16_t *win, uint16_t *out) {
#define DG_W(x) win[(x) & (NW - 1u)]
    DgChunkRun r;
    r.w = 0; r.tb = 0; r.dirty = false; r.overflow = false; r.badchar = false;
    if (k0 >= k1) return r;
    uint32_t badw = 0;                                     // bit 7 of a byte set: a byte outside 33..126 was read
    uint32_t ip = k0, e = 0, i = 0, w = 0, tb = 0, jt = 0, jq = 0;
    uint32_t e_end = 0xFFFFFFFFu;                          // window index of input column k1, once known
    // finished columns collect in a 128-bit shift register and leave 8 at a time (out is
    // 16-byte aligned): one store request instead of eight
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    // (flags that differ from lane to lane are kept as integers in vector registers, not as booleans: see k_emit)
    uint32_t in_done = 0, dirty = 0, overflow = 0;
    for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(in_done), "+v"(dirty));
#endif
        // ---- refill: Alignment.cpp:142-159 on the next (up to) 16 input columns ----
        if (!in_done && (e - i) + 32u > NW) { overflow = 1; break; }
        if (!in_done) {
            uint32_t take = len - ip;
            if (take > 16u) take = 16u;
            if (ip < k1 && take > k1 - ip) take = k1 - ip;  // land on the chunk's end exactly
#define DG_EXPAND(QB, TB)                                                      \
            do {                                                               \
                uint8_t qb_ = (QB), tb_ = (TB);                                \
                if (qb_ == '.') qb_ = DG_GAP;                                  \
                if (tb_ == '.') tb_ = DG_GAP;                                  \
                /* a mismatch becomes (-, t) (q, -): no branch -- the second slot is written whatever the column is */ \
                /* (the next column overwrites it; the refill has 32 free slots for its 16 columns) */                   \
                const bool mm_ = qb_ != tb_ && qb_ != DG_GAP && tb_ != DG_GAP; \
                DG_W(e) = mm_ ? DG_COL(DG_GAP, tb_) : DG_COL(qb_, tb_);        \
                DG_W(e + 1u) = DG_COL(qb_, DG_GAP);                            \
                e += mm_ ? 2u : 1u;                                            \
            } while (0)
            if (take == 16u && (((uintptr_t)(q + ip)) & 15u) == 0) {
                // the common case, unrolled: bytes come out of the two 16-byte registers with
                // constant shifts
                const dg_u4 qv = *reinterpret_cast<const dg_u4 *>(q + ip);
                const dg_u4 tv = *reinterpret_cast<const dg_u4 *>(t + ip);
                const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w}, tw[4] = {tv.x, tv.y, tv.z, tv.w};
                // every byte has to be printable ASCII (33..126): four at a time
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    badw |= ((qw[k] - 0x21212121u) & ~qw[k]) | ((qw[k] + 0x01010101u) | qw[k]);
                    badw |= ((tw[k] - 0x21212121u) & ~tw[k]) | ((tw[k] + 0x01010101u) | tw[k]);
                }
#pragma unroll
                for (int k = 0; k < 16; k++)
                    DG_EXPAND((uint8_t)(qw[k >> 2] >> (8 * (k & 3))), (uint8_t)(tw[k >> 2] >> (8 * (k & 3))));
            } else {
                // head (up to the next 16-byte boundary) and tail: byte loads
                const uint32_t to_align = (uint32_t)((16u - (((uintptr_t)(q + ip)) & 15u)) & 15u);
                if (to_align && take > to_align) take = to_align;
                for (uint32_t k = 0; k < take; k++) {
                    const uint8_t qb0 = q[ip + k], tb0 = t[ip + k];
                    if (qb0 < 33 || qb0 > 126 || tb0 < 33 || tb0 > 126) badw = 0x80u;
                    DG_EXPAND(qb0, tb0);
                }
            }
#undef DG_EXPAND
            ip += take;
            if (ip == k1) e_end = e;
            if (ip == len) in_done = 1;
        }
        DG_NORM_RUN_PROBE(e, i);
        // ---- Alignment.cpp:165-198 push gaps to the right, as far as the window reaches.
        // jt / jq only move forward (a column left of a cursor is never turned back into
        // a base).  A step that runs out of window stores what it has done to column i
        // and is restarted after the refill: the t-pass of a restarted step either finds
        // its column already filled or repeats the same fruitless look-up. ----
        while (i < e && i < e_end) {
            if (i + 1 == e && !in_done) break;
            const uint16_t c = DG_W(i);
            uint8_t qi = DG_Q(c), ti = DG_T(c);
            uint32_t more = 0;
            if (i + 1 < e) {
                if (ti == DG_GAP) {
                    if (jt <= i) jt = i + 1;
                    while (jt < e && DG_T(DG_W(jt)) == DG_GAP) jt++;
                    if (jt < e) {
                        const uint16_t cj = DG_W(jt);
                        if (DG_T(cj) == qi) { ti = qi; DG_W(jt) = DG_COL(DG_Q(cj), DG_GAP); dirty |= (uint32_t)(jt >= e_end); }
                    } else if (!in_done) more = 2;
                }
                if (!more && qi == DG_GAP) {
                    if (jq <= i) jq = i + 1;
                    while (jq < e && DG_Q(DG_W(jq)) == DG_GAP) jq++;
                    if (jq < e) {
                        const uint16_t cj = DG_W(jq);
                        if (DG_Q(cj) == ti) { qi = ti; DG_W(jq) = DG_COL(DG_GAP, DG_T(cj)); dirty |= (uint32_t)(jq >= e_end); }
                    } else if (!in_done) more = 2;
                }
            }
            if (more) { DG_W(i) = DG_COL(qi, ti); break; }
            if (qi != DG_GAP || ti != DG_GAP) {                                // :209-214
                o0 = (o0 >> 16) | (o1 << 16); o1 = (o1 >> 16) | (o2 << 16); o2 = (o2 >> 16) | (o3 << 16);
                o3 = (o3 >> 16) | ((uint32_t)DG_COL(qi, ti) << 16);
                w++;
                tb += (ti != DG_GAP);
                if ((w & 7u) == 0) *reinterpret_cast<dg_u4 *>(out + w - 8) = DG_MAKE_U4(o0, o1, o2, o3);
            }
            i++;
        }
        if (i == e_end) break;
    }
#undef DG_W
    // the last, partial group: its columns sit at the top of the register
    for (uint32_t k = w & 7u, x = w - (w & 7u); k > 0; k--, x++) {
        const uint32_t sh = 8u - k;                        // column x is sh places from the bottom
        const uint32_t word = sh >> 1;
        const uint32_t v = word == 0 ? o0 : word == 1 ? o1 : word == 2 ? o2 : o3;
        out[x] = (uint16_t)((sh & 1u) ? v >> 16 : v & 0xffffu);
    }
    r.w = w; r.tb = tb; r.dirty = dirty != 0; r.overflow = overflow != 0; r.badchar = (badw & 0x80808080u) != 0;
    return r;
}

// bit 7 of every byte of x that equals the same byte of y (exact for all byte values: no carry crosses a byte)
DG_HD_INLINE uint32_t dg_eq_bytes(const uint32_t x, const uint32_t y) {
    const uint32_t d = x ^ y;
    return ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
}

// The same contract on a 64-column window (win: 64 columns of the lane's own), for the first pass.
//
// normalizeGaps acts only at a column that holds a gap, and it finds the partner column by skipping gaps.  Both are
// read off two masks over the live window columns [o, e): TG (the target is a gap) and QG (the query is a gap), bit
// x - o for window column x.  Columns with a base in both strings -- most of the input -- are never looked at:
//   refill  as in dg_norm_run; every expanded column also sets its two bits
//   visits  the first set bit of TG | QG at or after i is the next column with anything to do.  Its partner is the
//           first clear bit of TG (t-pass) or QG (q-pass) behind it; a push rewrites both columns in LDS and flips
//           their two bits.  At most one of the two passes writes (the t-pass only where the query holds a base),
//           so a visit whose partner is not in the window yet has written nothing: it is repeated after the refill.
//           A column a push has emptied lies to the right of the visit that did it and is met in its turn.
//   output  columns in front of i are final and leave in groups of 8, one 16-byte store a group, read back from
//           LDS; a (-, -) column (TG & QG) is dropped, by a column-by-column path for the groups that hold one.
// The window holds up to 7 final columns that wait for their group, so the look-ahead it serves is the few columns
// shorter; what it cannot serve is reported as `overflow`, as before.
DG_HD inline DgChunkRun dg_norm_run_gc(const uint8_t *q, const uint8_t *t, const uint32_t len, const uint32_t k0,
                                       const uint32_t k1, uint16_t *win, uint16_t *out) {
#define DG_W(x) win[(x) & 63u]
    DgChunkRun r;
    r.w = 0; r.tb = 0; r.dirty = false; r.overflow = false; r.badchar = false;
    if (k0 >= k1) return r;
    uint32_t badw = 0;                                     // bit 7 of a byte set: a byte outside 33..126 was read
    // window columns: [0, o) written out, [o, i) final, [i, e) still to visit; e - o <= 64
    uint32_t ip = k0, e = 0, i = 0, o = 0, w = 0, tb = 0;
    uint32_t e_end = 0xFFFFFFFFu;                          // window index of input column k1, once known
    uint64_t TG = 0, QG = 0;                               // bits at and above e - o are clear
    // (flags that differ from lane to lane are kept as integers in vector registers, not as booleans: see k_emit)
    uint32_t in_done = 0, dirty = 0, overflow = 0;
    for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(in_done), "+v"(dirty));
#endif
        // ---- refill: Alignment.cpp:142-159 on the next (up to) 16 input columns ----
        if (!in_done && (e - o) + 32u > 64u) { overflow = 1; break; }
        if (!in_done) {
            uint32_t take = len - ip;
            if (take > 16u) take = 16u;
            if (ip < k1 && take > k1 - ip) take = k1 - ip;  // land on the chunk's end exactly
            // this refill's mask bits, bit l for column e0 + l (16 columns expand to at most 32)
            uint32_t tgl = 0, qgl = 0, l = 0;
            const uint32_t e0 = e, re0 = e - o;
            // Four columns at a time, as flags in bit 7 of their bytes: '.' becomes '-', then "is a gap" for either
            // string and "is a mismatch".  X holds (target is a gap) + 2 * (mismatch) per byte, Y holds (query is a gap
            // or mismatch): the bits the column(s) of that byte add to TG and QG.
#define DG_FLAGS(QW, TW)                                                       \
            const uint32_t qd_ = (QW) - (dg_eq_bytes((QW), 0x2E2E2E2Eu) >> 7), td_ = (TW) - (dg_eq_bytes((TW), 0x2E2E2E2Eu) >> 7); \
            const uint32_t gq_ = dg_eq_bytes(qd_, 0x2D2D2D2Du), gt_ = dg_eq_bytes(td_, 0x2D2D2D2Du);                                  \
            const uint32_t mmw_ = ~(dg_eq_bytes(qd_, td_) | gq_ | gt_) & 0x80808080u;                                                 \
            const uint32_t X_ = (gt_ >> 7) | (mmw_ >> 6), Y_ = (gq_ | mmw_) >> 7
            // a mismatch becomes (-, t) (q, -): no branch -- the second slot is written whatever the column is
            // (the next column overwrites it; the refill has 32 free slots for its 16 columns)
#define DG_EXPAND(SH)                                                          \
            do {                                                               \
                const uint32_t qb_ = (qd_ >> (SH)) & 0xffu, tb_ = (td_ >> (SH)) & 0xffu;          \
                const uint32_t nm_ = (uint32_t)((int32_t)(mmw_ << (24u - (SH))) >> 31);   /* all ones: a mismatch */ \
                const uint32_t x_ = e0 + l;                                    \
                DG_W(x_) = (uint16_t)(((qb_ & ~nm_) | ((uint32_t)DG_GAP & nm_)) | (tb_ << 8));    \
                DG_W(x_ + 1u) = (uint16_t)(qb_ | ((uint32_t)DG_GAP << 8));     \
                tgl |= ((X_ >> (SH)) & 3u) << l;                               \
                qgl |= ((Y_ >> (SH)) & 1u) << l;                               \
                l += 1u - nm_;                                                 \
            } while (0)
            if (take == 16u && (((uintptr_t)(q + ip)) & 15u) == 0) {
                // the common case, unrolled: bytes come out of the two 16-byte registers with
                // constant shifts
                const dg_u4 qv = *reinterpret_cast<const dg_u4 *>(q + ip);
                const dg_u4 tv = *reinterpret_cast<const dg_u4 *>(t + ip);
                const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w}, tw[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    // every byte has to be printable ASCII (33..126): four at a time
                    badw |= ((qw[k] - 0x21212121u) & ~qw[k]) | ((qw[k] + 0x01010101u) | qw[k]);
                    badw |= ((tw[k] - 0x21212121u) & ~tw[k]) | ((tw[k] + 0x01010101u) | tw[k]);
                    DG_FLAGS(qw[k], tw[k]);
                    DG_EXPAND(0u); DG_EXPAND(8u); DG_EXPAND(16u); DG_EXPAND(24u);
                }
            } else {
                // head (up to the next 16-byte boundary) and tail: byte loads
                const uint32_t to_align = (uint32_t)((16u - (((uintptr_t)(q + ip)) & 15u)) & 15u);
                if (to_align && take > to_align) take = to_align;
                for (uint32_t k = 0; k < take; k++) {
                    const uint32_t qb0 = q[ip + k], tb0 = t[ip + k];
                    if (qb0 < 33 || qb0 > 126 || tb0 < 33 || tb0 > 126) badw = 0x80u;
                    DG_FLAGS(qb0, tb0);
                    DG_EXPAND(0u);
                }
            }
#undef DG_EXPAND
#undef DG_FLAGS
            e = e0 + l;
            TG |= (uint64_t)tgl << re0;                     // re0 <= 32
            QG |= (uint64_t)qgl << re0;
            ip += take;
            if (ip == k1) e_end = e;
            if (ip == len) in_done = 1;
        }
        // ---- Alignment.cpp:165-198 push gaps to the right, at the gap columns only ----
        const uint32_t lim = e < e_end ? e : e_end;
        while (i < lim) {
            // the next column at or after i that holds a gap (i - o < 64: i < e <= o + 64)
            const uint64_t m = ((TG | QG) >> (i - o)) & (~0ull >> (64u - (lim - i)));
            if (!m) { i = lim; break; }                    // none: every column up to lim is final
            const uint32_t g = i + (uint32_t)__builtin_ctzll(m);
            i = g;
            if (g + 1u == e) {                             // the last column present:
                if (in_done) i = g + 1u;                   // the alignment's last column is never visited (:165),
                break;                                     // any other waits for the refill
            }
            const uint32_t rg = g - o;
            const uint16_t c = DG_W(g);
            uint8_t qi = DG_Q(c), ti = DG_T(c);
            const uint64_t ahead = ~0ull >> (64u - ((e - o) - rg - 1u));      // the columns (g, e), from bit 0
            uint32_t more = 0;
            if (ti == DG_GAP) {
                const uint64_t nt = (~TG >> (rg + 1u)) & ahead;               // (rg + 1 < e - o <= 64)
                if (nt) {
                    const uint32_t d = rg + 1u + (uint32_t)__builtin_ctzll(nt);
                    const uint16_t cj = DG_W(o + d);
                    if (DG_T(cj) == qi) {
                        ti = qi;
                        DG_W(o + d) = DG_COL(DG_Q(cj), DG_GAP);
                        DG_W(g) = DG_COL(qi, ti);
                        TG ^= (1ull << rg) | (1ull << d);
                        dirty |= (uint32_t)(o + d >= e_end);
                    }
                } else if (!in_done) more = 1;
            }
            if (!more && qi == DG_GAP) {
                const uint64_t nq = (~QG >> (rg + 1u)) & ahead;
                if (nq) {
                    const uint32_t d = rg + 1u + (uint32_t)__builtin_ctzll(nq);
                    const uint16_t cj = DG_W(o + d);
                    if (DG_Q(cj) == ti) {
                        qi = ti;
                        DG_W(o + d) = DG_COL(DG_GAP, DG_T(cj));
                        DG_W(g) = DG_COL(qi, ti);
                        QG ^= (1ull << rg) | (1ull << d);
                        dirty |= (uint32_t)(o + d >= e_end);
                    }
                } else if (!in_done) more = 1;
            }
            if (more) break;                               // nothing written: the visit is repeated after the refill
            i = g + 1u;
        }
        // ---- :209-214 final columns leave 8 at a time (out is 16-byte aligned, w a multiple of 8) ----
        while (i - o >= 8u) {
            if ((((uint32_t)TG & (uint32_t)QG) & 0xffu) == 0) {
                uint32_t v[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) v[k] = (uint32_t)DG_W(o + 2u * k) | ((uint32_t)DG_W(o + 2u * k + 1u) << 16);
                *reinterpret_cast<dg_u4 *>(out + w) = DG_MAKE_U4(v[0], v[1], v[2], v[3]);
                tb += (uint32_t)__builtin_popcount(~(uint32_t)TG & 0xffu);
                w += 8u; o += 8u;
                TG >>= 8; QG >>= 8;
            } else {
                // a (-, -) column among them: the next 8 columns that are none, if that many are final
                uint64_t nd = ~(TG & QG) & (~0ull >> (64u - (i - o)));
                if (__builtin_popcountll(nd) < 8) break;
                uint32_t d = 0;
                for (uint32_t k = 0; k < 8u; k++) {
                    d = (uint32_t)__builtin_ctzll(nd);
                    nd &= nd - 1u;
                    const uint16_t c = DG_W(o + d);
                    out[w + k] = c;
                    tb += (DG_T(c) != DG_GAP);
                }
                w += 8u; o += d + 1u;
                TG = d + 1u < 64u ? TG >> (d + 1u) : 0;
                QG = d + 1u < 64u ? QG >> (d + 1u) : 0;
            }
        }
        if (i == e_end) break;
    }
    // the last, partial group, column by column
    if (!overflow) {
        for (uint32_t x = o; x < i; x++) {
            const uint16_t c = DG_W(x);
            if (c == DG_COL(DG_GAP, DG_GAP)) continue;
            out[w++] = c;
            tb += (DG_T(c) != DG_GAP);
        }
    }
#undef DG_W
    r.w = w; r.tb = tb; r.dirty = dirty != 0; r.overflow = overflow != 0; r.badchar = (badw & 0x80808080u) != 0;
    return r;
}
