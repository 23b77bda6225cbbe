"""Bit-exact CPU twin of the local-end mode of the -a aligner (k_align.hip.h, LOCAL instances; dagcon_align on a context
created with DAGCON_FLAG_LOCAL_ALIGN).  The global twin is oracle/dagcon_oracle.c (og_banded_align and its two band
kinds); this restates it with the local ends and the same choices:
  - scores match -5, mismatch +6, insertion 4, deletion 5; a cell takes the diagonal, then an insertion (gap in t), then
    a deletion (gap in q), each only when strictly better; a score above 0 becomes 0 with code 3 ("starts here"), and
    so does every cell of row 0;
  - the end cell has the smallest score below 0 over all rows of the band, a tie going to the larger i, then the larger
    j; the walk runs back from it to a code-3 cell;
  - the band that follows the alignment (56 cells a side, shift clamp(a + 1 - 56, 0, 2), a = the row's first smallest
    cell) for pairs whose first static band is wider than 56; then the static band of dg_align_halfwidth_first, then the
    full one; a pass stands unless its path (the start cell included) comes within 8 cells of an edge or it finds no
    local alignment, and the last pass stands.
One numpy row at a time: the in-row deletion term through np.minimum.accumulate, unclamped, the clamp after it (exact:
min(0, min(A, S + 5)) = min(0, min(A, min(0, S) + 5))), as the kernels compute it.  The walk back is scalar."""
import math

import numpy as np

MATCH, MISMATCH, INS, DEL = -5, 6, 4, 5
BIG = 1 << 28            # the kernels' unreachable score: every candidate built on it stays far above 0
MAXW, WA, MARGIN = 480, 56, 8
RC = bytes.maketrans(b"ACGT", b"TGCA")


def halfwidth(n, m):
    L = max(n, m)
    return min(32 + 4 * math.isqrt((15 * L + 99) // 100), MAXW)


def halfwidth_first(n, m):
    L = max(n, m)
    return min(32 + 2 * math.isqrt((15 * L + 99) // 100), halfwidth(n, m))


def _row(prev_d, prev_u, qc, tv, j, m):
    """One row of cells at columns j (consecutive), from the previous row's scores at the diagonal / upper neighbours
    (BIG where there is none) -> (scores, codes), BIG on the cells outside [0, m]."""
    B = len(j)
    k = np.arange(B, dtype=np.int64)
    valid = (j >= 0) & (j <= m)
    tc = np.where((j >= 1) & (j <= m), tv[np.clip(j - 1, 0, max(m - 1, 0))] if m else 0, -1)
    dg = prev_d + np.where(tc == qc, MATCH, MISMATCH)
    up = prev_u + INS
    ins = up < dg
    A = np.where(valid, np.where(ins, up, dg), BIG)
    x = A - DEL * k
    pm = np.empty(B, np.int64)
    pm[0] = np.iinfo(np.int64).max
    pm[1:] = np.minimum.accumulate(x)[:-1]
    dl = (j > 0) & (pm < x)
    sc = np.where(dl, pm + DEL * k, A)
    d = np.where(dl, 2, ins.astype(np.int64))
    st = sc > 0
    sc = np.where(st, 0, sc)
    d = np.where(st, 3, d)
    return np.where(valid, sc, BIG), d.astype(np.uint8)


def _walk(q, t, dirs, i, j, kof, step_i, margin_b):
    """Walk back from (i, j) to a code-3 cell.  kof(i) = column of row i's cell 0; step_i(i): called as a step leaves
    row i.  -> (qaln, taln, (q_begin, q_end, t_begin, t_end), touched)."""
    ie, je = i, j
    qa, ta = bytearray(), bytearray()
    touched = False
    while True:
        kk = j - kof(i)
        if margin_b is not None and (kk < MARGIN or kk > margin_b - 1 - MARGIN):
            touched = True
        d = int(dirs[i][kk])
        if d == 3:
            break
        if d == 0:
            qa.append(q[i - 1]); ta.append(t[j - 1]); step_i(i); i -= 1; j -= 1
        elif d == 1:
            qa.append(q[i - 1]); ta.append(ord("-")); step_i(i); i -= 1
        else:
            qa.append(ord("-")); ta.append(t[j - 1]); j -= 1
    return bytes(qa[::-1]), bytes(ta[::-1]), (i, ie, j, je), touched


def static_band(q, t, W):
    """The static band of half-width W around j = i m / n -> (qaln, taln, ends, touched), or None: no cell below 0."""
    n, m = len(q), len(t)
    B = 2 * W + 1
    qv, tv = np.frombuffer(q, np.uint8).astype(np.int64), np.frombuffer(t, np.uint8).astype(np.int64)
    k = np.arange(B, dtype=np.int64)
    dirs = np.empty((n + 1, B), np.uint8)
    j = -W + k
    prev = np.where((j >= 0) & (j <= m), 0, BIG)
    dirs[0] = 3
    best, bi, bk = 0, -1, -1
    pad = np.full(B + 2, BIG, np.int64)
    for i in range(1, n + 1):
        ci, cp = i * m // n, (i - 1) * m // n
        s = ci - cp
        j = ci - W + k
        if s > B:
            pd = pu = np.full(B, BIG, np.int64)
        else:
            ext = np.concatenate((pad[:1], prev, np.full(s + 1, BIG, np.int64)))     # ext[x + 1] = prev[x]
            pd, pu = ext[k + s], ext[k + s + 1]                                        # prev[k + s - 1], prev[k + s]
        prev, dirs[i] = _row(pd, pu, int(qv[i - 1]), tv, j, m)
        rmin = int(prev.min())
        if rmin < 0 and rmin <= best:
            best, bi, bk = rmin, i, int(np.flatnonzero(prev == rmin)[-1])
    if best >= 0:
        return None
    kof = lambda i: i * m // n - W                               # noqa: E731
    return _walk(q, t, dirs, bi, kof(bi) + bk, kof, lambda i: None, B)


def following_band(q, t):
    """The band that follows the alignment -> (qaln, taln, ends), or None: fall back to the static bands."""
    n, m = len(q), len(t)
    W = WA
    B = 2 * W + 1
    qv, tv = np.frombuffer(q, np.uint8).astype(np.int64), np.frombuffer(t, np.uint8).astype(np.int64)
    k = np.arange(B, dtype=np.int64)
    dirs = np.empty((n + 1, B), np.uint8)
    sh = np.zeros(n + 1, np.int64)
    los = np.zeros(n + 1, np.int64)
    lo = -W
    j = lo + k
    prev = np.where((j >= 0) & (j <= m), 0, BIG)
    dirs[0] = 3
    best, bi, bk = 0, -1, -1
    for i in range(1, n + 1):
        a = int(np.argmin(prev))
        if prev[a] >= BIG:
            return None
        s = min(max(a + 1 - W, 0), 2)
        lo += s
        sh[i], los[i] = s, lo
        ext = np.concatenate((prev, np.full(2, BIG, np.int64)))
        pd = np.concatenate(([BIG], ext))[k + s] if s == 0 else ext[k + s - 1]
        pu = ext[k + s]
        prev, dirs[i] = _row(pd, pu, int(qv[i - 1]), tv, lo + k, m)
        rmin = int(prev.min())
        if rmin < 0 and rmin <= best:
            best, bi, bk = rmin, i, int(np.flatnonzero(prev == rmin)[-1])
    if best >= 0:
        return None
    los[0] = -W
    cur = {"lo": int(los[bi])}

    def step(i):
        cur["lo"] -= int(sh[i])
    # (the rows' lo: the walk moves it back by the row's shift as it leaves the row, as the kernel does)
    qa, ta, ends, touched = _walk(q, t, dirs, bi, int(los[bi]) + bk, lambda i: cur["lo"], step, B)
    return None if touched else (qa, ta, ends)


STAGE_NONE, STAGE_FOLLOWING, STAGE_FIRST, STAGE_FULL = 0, 1, 2, 3     # oracle.STAGE_*: the pass whose answer stands


def align(q: bytes, t: bytes, static_only: bool = False, stage: bool = False):
    """The pass structure of dagcon_align in local mode -> (qaln, taln, (q_begin, q_end, t_begin, t_end)); a pair
    without a local alignment -> (b"", b"", (0, 0, 0, 0)).  static_only: DAGCON_ALIGN_STATIC=1.  stage: a fourth
    element says which pass produced the answer (STAGE_*: the following band, the first static band, the full band;
    none when no pass finds a local alignment)."""
    n, m = len(q), len(t)
    none = (b"", b"", (0, 0, 0, 0))
    if n == 0 or m == 0:
        return none + (STAGE_NONE,) if stage else none
    w1, w2 = halfwidth_first(n, m), halfwidth(n, m)
    if w1 > WA and not static_only:
        r = following_band(q, t)
        if r is not None:
            return r + (STAGE_FOLLOWING,) if stage else r
    r, st = static_band(q, t, w1), STAGE_FIRST
    if w1 < w2 and (r is None or r[3]):
        r, st = static_band(q, t, w2), STAGE_FULL
    if r is None:
        return none + (STAGE_NONE,) if stage else none
    return r[:3] + (st,) if stage else r[:3]


def full_matrix(q: bytes, t: bytes):
    """A plain scalar local DP over the whole matrix, cell by cell, with the same rules (the clamp inside the
    recurrence, the same tie-breaks and end cell) -> (qaln, taln, ends), or the empty result."""
    n, m = len(q), len(t)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    D = [[3] * (m + 1) for _ in range(n + 1)]
    best, bi, bj = 0, -1, -1
    for i in range(1, n + 1):
        for j in range(m + 1):
            v, d = BIG, 3
            if j > 0:
                v, d = H[i - 1][j - 1] + (MATCH if q[i - 1] == t[j - 1] else MISMATCH), 0
            if H[i - 1][j] + INS < v:
                v, d = H[i - 1][j] + INS, 1
            if j > 0 and H[i][j - 1] + DEL < v:
                v, d = H[i][j - 1] + DEL, 2
            if v > 0:
                v, d = 0, 3
            H[i][j], D[i][j] = v, d
            if v < 0 and v <= best:
                best, bi, bj = v, i, j
    if best >= 0:
        return b"", b"", (0, 0, 0, 0)
    qa, ta, ends, _ = _walk(q, t, D, bi, bj, lambda i: 0, lambda i: None, None)
    return qa, ta, ends


def finish(tstart: int, tlen: int, strand: bytes, qa: bytes, ta: bytes, ends):
    """SimpleAligner.cpp:51-62 in local mode: start = tstart + t_begin, end = tstart + t_end ('GenomicTEnd()' read as
    the aligned target span added to the moved start); '-': start = tlen - end, both strings reverse-complemented;
    start += 1.  -> (start, end, qaln, taln)."""
    start, end = tstart + ends[2], tstart + ends[3]
    if strand[:1] == b"-":
        start = tlen - end
        qa, ta = qa.translate(RC)[::-1], ta.translate(RC)[::-1]
    return start + 1, end, qa, ta
