"""Bit-exact CPU twin of k_align_panels.hip.h (dagcon_align_panels, dazcon --trace-panels): every trace-point panel
aligned on its own, unit-cost edit distance with both corners fixed, ties diagonal first, then a q base against a gap
in t (D[i][j-1]), then a t base against a gap in q (D[i-1][j]); row 0 always moves left, column 0 always up.
Parity unpinned: DALIGNER is not in the reference tree, the tie-breaks are this build's own.  One numpy row at a time
(the in-row term through np.minimum.accumulate, as the kernel's running minimum), the walk back scalar."""
import numpy as np

DIAG, LEFT, UP = 0, 1, 2


def align_panel(t: bytes, q: bytes):
    """A-panel t (rows) against B-panel q (columns) -> (qaln, taln, distance)."""
    m, n = len(t), len(q)
    tv = np.frombuffer(t, np.uint8)
    qv = np.frombuffer(q, np.uint8)
    jj = np.arange(n + 1, dtype=np.int64)
    prev = jj.copy()                                          # row 0
    dirs = np.zeros((m + 1, n + 1), np.uint8)
    for i in range(1, m + 1):
        diag = prev[:-1] + (qv != tv[i - 1])
        up = prev[1:] + 1
        e = np.empty(n + 1, np.int64)
        e[0] = i
        e[1:] = np.minimum(diag, up)
        lf = np.minimum.accumulate(e - jj)[:-1] + jj[1:]      # D[i][j-1] + 1
        d = np.minimum(e[1:], lf)
        dirs[i, 1:] = np.where(diag == d, DIAG, np.where(lf <= up, LEFT, UP))
        prev = np.concatenate(([i], d))
    dist = int(prev[n])
    qa, ta = bytearray(), bytearray()
    i, j = m, n
    while i > 0 or j > 0:
        k = LEFT if i == 0 else UP if j == 0 else int(dirs[i, j])
        if k == DIAG:
            qa.append(q[j - 1]); ta.append(t[i - 1]); i -= 1; j -= 1
        elif k == LEFT:
            qa.append(q[j - 1]); ta.append(ord("-")); j -= 1
        else:
            qa.append(ord("-")); ta.append(t[i - 1]); i -= 1
    return bytes(qa[::-1]), bytes(ta[::-1]), dist


def align_overlap(q: bytes, t: bytes, panels):
    """q (B interval) against t (A interval) cut into panels [(A bases, B bases)] -> (qaln, taln, [distance])."""
    qa, ta, dists = [], [], []
    a = b = 0
    for tl, ql in panels:
        x, y, d = align_panel(t[a:a + tl], q[b:b + ql])
        qa.append(x); ta.append(y); dists.append(d)
        a += tl; b += ql
    assert a == len(t) and b == len(q)
    return b"".join(qa), b"".join(ta), dists


def trace_panels(abpos, aepos, trace, tspace):
    """A .las record's trace -> its panels [(A bases, B bases)]: panel 0 is A[abpos, min(aepos, (abpos // tspace + 1)
    tspace)), the middle ones tspace, the last ends at aepos; panel i takes trace[2 i + 1] B bases."""
    bounds, a = [], abpos
    while a < aepos:
        e = min(aepos, (a // tspace + 1) * tspace)
        bounds.append(e - a)
        a = e
    assert len(trace) == 2 * len(bounds)
    return [(bounds[i], trace[2 * i + 1]) for i in range(len(bounds))]
