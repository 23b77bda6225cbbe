// k_norm_fin.hip.h -- what a lane of k_norm_finish2 computes on its columns of a chunk: the classes of the columns
// by 32-bit words, the operator of the segmented scan that carries insertion runs from lane to lane, and the EVENTS
// among a lane's columns (an insertion run ends, a checkpoint position is reached) with their target position and
// run length -- by bit masks and popcounts, so that the kernel visits the events and not every column.  No kernel
// and no device-only construct in here, so that a host compiler takes the file as well
// (tests/native/norm_fin_host.cpp runs it on the CPU against the literal loop of dg_finish_alignment).
//
// A lane holds DG_FIN_NP adjacent 16-byte pieces of 8 columns; bit k of its masks is its column k:
//   advm  the column advances the backbone cursor (a match or a deletion: q == t or q is a gap)
//   insm  the column is an insertion (not advancing, t is a gap)
//   delm  the column is a deletion (advancing, q != t)
// all three cleared outside the trimmed window.  A column that is neither (raw columns: two different bases) does not
// reset an insertion run, so a run is a popcount of insm between two advancing columns, not a stretch of set bits.
#pragma once
#include "k_norm_run.hip.h"

#ifndef DG_FIN_NP
#define DG_FIN_NP 2u           // 16-byte pieces per lane and pass (1: see DESIGN.md section 5, round 8)
#endif
#define DG_FIN_COLS (8u * DG_FIN_NP)                       // columns per lane and pass
#define DG_FIN_ALL ((1u << DG_FIN_COLS) - 1u)

// Two columns of a word (bytes q0 t0 q1 t1), flags in bits 7 and 23 (K: advancing) and 15 and 31 (K: insertion),
// D: deletion in bits 7 and 23.
DG_HD_INLINE void dg_fin_word(const uint32_t w, uint32_t &K, uint32_t &D) {
    const uint32_t G = dg_eq_bytes(w, 0x2D2D2D2Du);        // is a gap, all four bytes
    const uint32_t E = dg_eq_bytes(w, w >> 8);             // q == t in bits 7 and 23
    const uint32_t A = (E | G) & 0x00800080u;
    const uint32_t I = ~A & (G >> 8) & 0x00800080u;
    K = A | (I << 8);
    D = A & ~E;
}

struct DgFinMasks { uint32_t advm, insm, delm; };          // 8 bits each

// the four words of a piece: word j's flags go to bits 2j (its first column) and 2j + 1
DG_HD_INLINE DgFinMasks dg_fin_piece(const dg_u4 pc) {
    uint32_t K0, K1, K2, K3, D0, D1, D2, D3;
    dg_fin_word(pc.x, K0, D0); dg_fin_word(pc.y, K1, D1); dg_fin_word(pc.z, K2, D2); dg_fin_word(pc.w, K3, D3);
    uint32_t k = (K0 >> 7) | (K1 >> 5) | (K2 >> 3) | (K3 >> 1);      // even columns: bits 0..6 / 8..14, odd: 16 higher
    uint32_t d = (D0 >> 7) | (D1 >> 5) | (D2 >> 3) | (D3 >> 1);
    k |= k >> 15; d |= d >> 15;
    DgFinMasks m;
    m.advm = k & 0xFFu; m.insm = (k >> 8) & 0xFFu; m.delm = d & 0xFFu;
    return m;
}

// bit k: column c0 + k of the chunk lies in the trimmed window [f0, f1), k < DG_FIN_COLS
DG_HD_INLINE uint32_t dg_fin_window(const uint32_t c0, const uint32_t f0, const uint32_t f1) {
    const uint32_t a = f0 > c0 ? (f0 - c0 < DG_FIN_COLS ? f0 - c0 : DG_FIN_COLS) : 0u;
    const uint32_t b = f1 > c0 ? (f1 - c0 < DG_FIN_COLS ? f1 - c0 : DG_FIN_COLS) : 0u;
    return b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
}

// ---- the segmented scan: insertion columns since the last advancing column ----
// A (reset, value) pair in one word: bit 31 = the stretch holds an advancing column, the rest = insertion columns
// behind its last advancing column (all of them if it holds none).  0 is the identity.
#define DG_SEG_RESET 0x80000000u
DG_HD_INLINE uint32_t dg_seg_pack(const uint32_t advm, const uint32_t insm) {
    if (!advm) return (uint32_t)__builtin_popcount(insm);
    const uint32_t upto = (2u << (31 - __builtin_clz(advm))) - 1u;                   // up to its last advancing column
    return DG_SEG_RESET | (uint32_t)__builtin_popcount(insm & ~upto);
}
// a: the stretch in front, b: the stretch behind it
DG_HD_INLINE uint32_t dg_seg_combine(const uint32_t a, const uint32_t b) { return (b & DG_SEG_RESET) ? b : a + b; }
DG_HD_INLINE uint32_t dg_seg_value(const uint32_t x) { return x & ~DG_SEG_RESET; }

// ---- events ----
// The advancing columns at which an insertion run ends: an insertion column lies between the advancing column in
// front (in the lane) and this one, or none is in front and run_in (the run that arrives at the lane) is not 0.
// With everything moved up a bit and run_in as bit 0: every advancing column closes a segment of insertion bits
// below it, advm - insm borrows from exactly the advancing bits whose segment is not empty, and no borrow leaves
// its segment (the segment's insertion bits sum to less than its advancing bit).
DG_HD_INLINE uint32_t dg_fin_run_ends(const uint32_t advm, const uint32_t insm, const uint32_t run_in) {
    const uint32_t a = advm << 1, b = (insm << 1) | (run_in ? 1u : 0u);
    return (a & ~(a - b)) >> 1;
}

// the insertion run that ends at the lane's advancing column k
DG_HD_INLINE uint32_t dg_fin_run_at(const uint32_t advm, const uint32_t insm, const uint32_t run_in, const uint32_t k) {
    // no branch: with a bit in front of bit 0 the highest advancing column below k is always there, and the columns
    // behind it are those from its own bit number on in the mask that is a bit up
    const uint32_t below = (1u << k) - 1u, prev = advm & below;
    const uint32_t behind = ~0u << (31 - __builtin_clz((prev << 1) | 1u));
    return (prev ? 0u : run_in) + (uint32_t)__builtin_popcount(insm & below & behind);
}

// column of the lane's j-th advancing column (j < popcount(advm))
DG_HD_INLINE uint32_t dg_fin_nth_adv(uint32_t advm, uint32_t j) {
    while (j--) advm &= advm - 1u;
    return (uint32_t)__builtin_ctz(advm);
}

// What is the same for all columns of a chunk.  Conformity (dg_finish_alignment: start >= 1 and, once a target base
// is behind, start - 1 + adv <= tlen) only ever turns false as adv grows: it is adv <= lim.
struct DgFinChunk {
    uint32_t start, tlen, lim, ck_mask, ck_shift;
    uint32_t o, lo;                // the chunk's first column in the alignment, the trimmed window's first
    bool ok;                       // start >= 1
};
DG_HD_INLINE DgFinChunk dg_fin_chunk(const uint32_t start, const uint32_t tlen, const uint32_t emit_shift, const uint32_t o,
                                     const uint32_t lo) {
    DgFinChunk u;
    u.start = start; u.tlen = tlen; u.ck_shift = emit_shift; u.ck_mask = (1u << emit_shift) - 1u; u.o = o; u.lo = lo;
    u.ok = start >= 1u;
    const uint64_t room = (uint64_t)tlen + 1u;             // start - 1 + adv <= tlen  <=>  adv <= tlen + 1 - start
    u.lim = !u.ok ? 0u : room >= start ? (uint32_t)(room - start) : 0u;
    return u;
}
DG_HD_INLINE bool dg_fin_conf(const DgFinChunk &u, const uint32_t adv) { return u.ok && adv <= u.lim; }
// may the position start + adv be written to (matC cell, checkpoint)
DG_HD_INLINE bool dg_fin_writes(const DgFinChunk &u, const uint32_t adv) {
    return dg_fin_conf(u, adv) && u.start + adv <= u.tlen + 1u;
}

// An event at the lane's advancing column k; adv_lane: target bases in front of the lane's columns.
// pos = start + adv as dg_finish_alignment has it at that column, run = the insertion run that ends there.
struct DgFinEvent { uint32_t pos, run; bool writes; };
DG_HD_INLINE DgFinEvent dg_fin_event(const DgFinChunk &u, const uint32_t advm, const uint32_t insm, const uint32_t run_in,
                                     const uint32_t adv_lane, const uint32_t k) {
    DgFinEvent e;
    const uint32_t adv = adv_lane + (uint32_t)__builtin_popcount(advm & ((1u << k) - 1u));
    e.pos = u.start + adv;
    e.run = dg_fin_run_at(advm, insm, run_in, k);
    e.writes = dg_fin_writes(u, adv);
    return e;
}

// Checkpoints: the lane's advancing columns whose position start + adv is a multiple of 1 << emit_shift are its
// j-th ones, j = first, first + (ck_mask + 1), ... below popcount(advm).
DG_HD_INLINE uint32_t dg_fin_first_ckpt(const DgFinChunk &u, const uint32_t adv_lane) {
    return (0u - (u.start + adv_lane)) & u.ck_mask;
}
// the checkpoint at the lane's advancing column k = column x of the chunk: does this chunk record it, and what
// (the first column of a chunk inside the window is recorded by the chunk in front, whose last columns may be the
// insertion run that belongs to this position)
DG_HD_INLINE bool dg_fin_ckpt(const DgFinChunk &u, const DgFinEvent &e, const uint32_t x, uint32_t &slot, uint32_t &value) {
    slot = e.pos >> u.ck_shift;
    value = u.o + x - e.run;
    return e.writes && !(x == 0u && u.o > u.lo);
}
