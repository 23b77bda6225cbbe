// k_lists_row.hip.h -- one arrival / departure row of a backbone position -> the entries of one adjacency list, the
// whole row on ONE lane: the loop a lane of k_lists_lanes runs (dg_list_row of k_build.hip.h is the same rule with a
// read per lane).  No kernel and no device-only construct in here, so that a host compiler takes the file as well
// (tests/native/lists_row_host.cpp runs it on the CPU).
//
//   Entry 0 is the adjacent backbone vertex (`chain`, id + 1), there even with no read on it.
//   A cell with an id in [ulo, uhi) is a vertex of the adjacent insertion group: one read only, appended as it is met.
//   Any other non-zero id is another backbone vertex (deletion jump, enter, exit): appended at its first read, counted
//   in a table of DG_LTAB slots (reads; the `extra` of the first read stays in the staged cell); a row with more
//   distinct ones is marked `overflow` and left to the wave-wide routine.
//
// The entries after entry 0 are staged in place: entry j (j >= 1) lands in row[j - 1] as id | extra << 25, which the
// scan has passed by then (at most one entry per cell).
#pragma once
#include <stdint.h>

#ifndef DG_HD_INLINE
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DG_HD_INLINE __host__ __device__ __forceinline__
#else
#define DG_HD_INLINE inline __attribute__((always_inline))
#endif
#endif
#ifndef DG_CELL_ID
#define DG_CELL_ID(c)   ((c) & 0x1FFFFFFu)
#define DG_CELL_DEL     0x1FFFFFFu
#endif
#ifndef DG_CELL_DUP
#define DG_CELL_DUP 0x1FFFFFEu
#endif

#define DG_LTAB 4u             // other backbone neighbours a lane keeps count of (profiles/lists_lanes/row_stats.txt)

struct DgLaneRow {
    uint32_t n;                // entries, entry 0 included
    uint32_t c0;               // reads on entry 0
    uint32_t tv[DG_LTAB];      // other backbone neighbours, the latest in slot 0: id + 1 (0: free slot),
    uint32_t tc[DG_LTAB];      //   reads that hold it
    uint32_t overflow;         // non-zero: a distinct neighbour beyond the table, the lists of this row are not valid
    uint32_t n_cov, n_match, last_base;   // arrival rows: covering reads, those that are no deletion, base of the last one
};

// (written without branches but the one around the store: the lanes of a wave execute the union of their paths)
template <bool ARRIVAL>
DG_HD_INLINE void dg_lane_cell(DgLaneRow &s, const uint32_t cell, uint32_t *row, const uint32_t chain,
                               const uint32_t ulo, const uint32_t uspan) {
    uint32_t val = DG_CELL_ID(cell);
    if (ARRIVAL) {
        s.n_cov += cell != 0u;
        s.n_match += (cell != 0u) & (val != DG_CELL_DEL);
        s.last_base = cell != 0u ? cell >> 25 : s.last_base;
        val = ((val == DG_CELL_DEL) | (val == DG_CELL_DUP)) ? 0u : val;
    }
    s.c0 += val == chain;
    const bool uniq = val - ulo < uspan;                       // ulo <= val < uhi
    bool newo = !uniq & (val != 0u) & (val != chain);
#pragma unroll
    for (uint32_t k = 0; k < DG_LTAB; k++) {
        const bool h = s.tv[k] == val;                         // (a free slot counts the empty cells: nobody reads that)
        s.tc[k] += h;
        newo &= !h;
    }
    // a new one moves the table up by a slot; what falls out of the last slot was a fifth
    s.overflow |= newo ? s.tv[DG_LTAB - 1u] : 0u;
#pragma unroll
    for (uint32_t k = DG_LTAB - 1u; k > 0; k--) {
        s.tv[k] = newo ? s.tv[k - 1u] : s.tv[k];
        s.tc[k] = newo ? s.tc[k - 1u] : s.tc[k];
    }
    s.tv[0] = newo ? val : s.tv[0];
    s.tc[0] = newo ? 1u : s.tc[0];
    if (uniq | newo) { row[s.n - 1u] = ARRIVAL ? val : cell; s.n++; }
}

// the row of K cells at row[0 .. K), scanned once in read order
template <bool ARRIVAL>
DG_HD_INLINE DgLaneRow dg_lane_row(uint32_t *row, const uint32_t K, const uint32_t chain, const uint32_t ulo,
                                   const uint32_t uhi) {
    DgLaneRow s = {};
    s.n = 1u;
    const uint32_t uspan = uhi > ulo ? uhi - ulo : 0u;
    uint32_t r = 0;
    // (four cells fetched ahead of the stores they cannot meet: the staged entries stay behind the scan)
    for (; r + 4u <= K; r += 4u) {
        const uint32_t c0 = row[r], c1 = row[r + 1u], c2 = row[r + 2u], c3 = row[r + 3u];
        dg_lane_cell<ARRIVAL>(s, c0, row, chain, ulo, uspan);
        dg_lane_cell<ARRIVAL>(s, c1, row, chain, ulo, uspan);
        dg_lane_cell<ARRIVAL>(s, c2, row, chain, ulo, uspan);
        dg_lane_cell<ARRIVAL>(s, c3, row, chain, ulo, uspan);
    }
    for (; r < K; r++) dg_lane_cell<ARRIVAL>(s, row[r], row, chain, ulo, uspan);
    return s;
}

// count of a staged entry (out-lists): `e` = row[j - 1], j >= 1
DG_HD_INLINE uint32_t dg_lane_count(const DgLaneRow &s, const uint32_t e) {
    const uint32_t id = DG_CELL_ID(e), extra = e >> 25;
    uint32_t cnt = 1u;
#pragma unroll
    for (uint32_t k = 0; k < DG_LTAB; k++) cnt = s.tv[k] == id ? s.tc[k] : cnt;
    return cnt + extra;
}
