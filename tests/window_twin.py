"""CPU twin of the windowed CIGAR input (include/dagcon.h, dagcon_windows) and the rule by which the results of
neighbouring windows are joined at a target coordinate, on top of cigar_twin.  numpy / Python only; the oracle is
imported by the two functions that read per-base positions off its graph, nowhere else.

    span(pos, tlen, ops)                -> (s, e): the target bases [s, e) a record covers
    first_col(tstr, s, x)               -> F(x): the first column of the expansion that consumes target base x
    cut(pos, q, t, ops, a, b)           -> None | (aln_start, qstr, tstr, c0, c1): the record's piece in window [a, b)
    window_targets(targets, windows)    -> per window (tlen, [(start, q, t)], failed)
    tiled(tlen, W, O)                   -> [(begin, end, core begin, core end)]
    stitch(windows, min_len)            -> [(t0, t1, seq, extra)]: the joined pieces of one target
    positions(...)                      -> per segment the _bbMap of its bases (the oracle's graph)
"""
import ctypes as C

import numpy as np

import cigar_twin as ct

GAP = ct.GAP


def span(pos, tlen, ops):
    """[s, e) of a record.  A conforming record: s = pos - 1, e = s + the target bases its ops consume.  Any other
    record: the same arithmetic on what it has (codes above 8 and N consume nothing; the total kept to 32 bits), then
    s <= tlen - 1 and s + 1 <= e <= tlen, the rule of include/dagcon.h."""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1)
    code, ln = ops & 15, ops >> 4
    nt = int(ln[np.isin(code, ct._TGT)].sum())
    s = max(int(pos), 1) - 1
    if ct.conforming(pos, int(ln[np.isin(code, ct._QRY)].sum()), tlen, ops):
        return s, s + nt
    e = s + (nt & 0xFFFFFFFF)
    s = min(s, tlen - 1)
    return s, min(max(e, s + 1), tlen)


def first_col(tstr, s, e, x):
    """F(x) for s <= x <= e over the target side of a record's expansion: F(s) = 0, F(e) = the number of columns,
    otherwise the first column that consumes target base x."""
    ts = np.frombuffer(bytes(tstr), np.uint8)
    if x == s:
        return 0
    if x == e:
        return int(ts.size)
    cons = ts != GAP
    tidx = s + np.cumsum(cons) - 1                     # the target base a consuming column holds
    hit = np.flatnonzero(cons & (tidx == x))
    assert hit.size == 1
    return int(hit[0])


def cut(pos, q, t, ops, a, b):
    """The piece of a conforming record in window [a, b) of its target t (bytes): None, or (aln_start, qstr, tstr,
    first column, end column)."""
    start, qs, ts = ct.expand(pos, q, t, ops)
    s = pos - 1
    e = s + sum(1 for ch in ts if ch != GAP)
    A, B = max(a, s), min(b, e)
    if A >= B:
        return None
    c0, c1 = first_col(ts, s, e, A), first_col(ts, s, e, B)
    return A - a + 1, qs[c0:c1], ts[c0:c1], c0, c1


def window_targets(targets, windows):
    """targets = [(target bases, [(pos, read, ops)])], windows = [(target index, begin, end)]: per window
    (tlen, [(aln_start, qstr, tstr)], failed) -- failed: a non-conforming record has a piece in it (its pieces list is
    then empty).  Pieces keep the order of their records."""
    out = []
    for g, a, b in windows:
        tseq, recs = targets[g]
        alns, failed = [], False
        for pos, q, ops in recs:
            s, e = span(pos, len(tseq), ops)
            if max(a, s) >= min(b, e):
                continue
            if not ct.conforming(pos, len(q), len(tseq), ops):
                failed = True
                continue
            st, qs, ts, _, _ = cut(pos, q, tseq, ops, a, b)
            alns.append((st, qs, ts))
        out.append((b - a, [] if failed else alns, failed))
    return out


def tiled(tlen, W, O):
    """Window i of a target: (begin, end, core begin, core end); the core [i W, min((i + 1) W, tlen)) is run as
    [max(0, i W - O), min(tlen, (i + 1) W + O))."""
    n = max(1, -(-tlen // W))
    return [(max(0, i * W - O), min(tlen, (i + 1) * W + O), i * W, min((i + 1) * W, tlen)) for i in range(n)]


def stitch(windows, min_len):
    """The joined pieces of one target.  windows: in order, (begin, core begin, core end, [(seq, pos, extra)]) with pos
    the window's per-base positions (1-based, dagcon_fetch_positions) and extra any per-base sequence sliced as the
    bases are (qualities), or None.  Global position g = pos + begin.  Of a segment the bases from the first one with
    g > core begin up to, not including, the first one from there on with g > core end are kept (first crossings only:
    nothing assumes that g is monotone); a segment whose kept part is empty is ignored.  The segment was cut at its
    core begin when bases lie in front of the kept part, at its core end when bases lie behind it.  A kept part that
    was cut at its core begin continues the piece before it when that piece is the kept part before it in this order,
    comes from the window just before, and was cut at its core end; otherwise it starts a new piece.  Pieces shorter
    than min_len are dropped.  Returns [(t0, t1, seq, extra)], t0 = g of the first base - 1, t1 = g of the last."""
    pieces = []
    open_w = None                                              # window index of the last piece, if it was cut at its core end
    for wi, (begin, c0, c1, segs) in enumerate(windows):
        for seq, pos, extra in segs:
            g = np.asarray(pos, dtype=np.int64) + begin
            over0 = np.flatnonzero(g > c0)
            if over0.size == 0:
                continue
            i0 = int(over0[0])
            over1 = np.flatnonzero(g[i0:] > c1)
            i1 = i0 + int(over1[0]) if over1.size else int(g.size)
            if i1 <= i0:
                continue
            part = [int(g[i0]) - 1, int(g[i1 - 1]), bytes(seq[i0:i1]), None if extra is None else bytes(extra[i0:i1])]
            if i0 > 0 and open_w is not None and open_w == wi - 1:
                last = pieces[-1]
                last[1] = part[1]; last[2] += part[2]
                if extra is not None:
                    last[3] += part[3]
            else:
                pieces.append(part)
            open_w = wi if i1 < g.size else None
    return [tuple(p) for p in pieces if len(p[2]) >= min_len]


# ---- per-base positions off the oracle's graph (tests/support_twin.py reads weights the same way) --------------------

def _node(L, g, v):
    base = C.create_string_buffer(1)
    w, cv, d, bb, bm = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L.og_node_info(g, v, base, C.byref(w), C.byref(cv), C.byref(d), C.byref(bb), C.byref(bm))
    return base.raw, bm.value


def target_positions(tlen, alns, min_len=500, trim=50, min_weight=6, backbone=None, with_support=False):
    """[(range0, range1, seq, positions)]: _bbMap of the best-path vertex of every consensus base, as main.cpp:130-138
    builds the graph.  None for a target the reference would not accept.  with_support: (.., weights, depths) too, as
    tests/support_twin.py reads them."""
    import oracle
    g = oracle.Graph(backbone=backbone) if backbone is not None else oracle.Graph(blen=tlen)
    for start, q, t in alns:
        if len(q) < min_len:
            continue
        q, t = oracle.normalize_gaps(q, t)
        q, t, start = oracle.trim_aln(q, t, start, trim)
        tb = sum(1 for ch in t if ch != GAP)
        if q and (start < 1 or start - 1 + tb > tlen):
            return None
        g.add_aln(start, q, t)
    if g.merge_nodes() != 0:
        return None
    path = g.best_path()
    eb, xb = _node(g.L, g.g, 0)[0], _node(g.L, g.g, tlen + 1)[0]
    ps, ws, ds = [], [], []
    for v in path:
        base, bm = _node(g.L, g.g, v)
        if base in (eb, xb):
            continue
        ps.append(bm)
        if with_support:
            w, cv = C.c_int(), C.c_int()
            d, bb, b2, one = C.c_int(), C.c_int(), C.c_int64(), C.create_string_buffer(1)
            g.L.og_node_info(g.g, v, one, C.byref(w), C.byref(cv), C.byref(d), C.byref(bb), C.byref(b2))
            ws.append(w.value)
            g.L.og_node_info(g.g, bm, one, C.byref(w), C.byref(cv), C.byref(d), C.byref(bb), C.byref(b2))
            ds.append(cv.value)
    if with_support:
        return [(r0, r1, s, ps[r0:r1], ws[r0:r1], ds[r0:r1]) for r0, r1, s in g.consensus_all(min_weight, min_len)]
    return [(r0, r1, s, ps[r0:r1]) for r0, r1, s in g.consensus_all(min_weight, min_len)]


def batch_positions(batch, min_cov=6, min_len=500, trim=50, min_weight=None):
    """Per target of a HostBatch [(range0, range1, seq, positions)] ([] below min_cov)."""
    if min_weight is None or min_weight < 0:
        min_weight = min_cov
    out = []
    for t in range(batch.n_targets):
        a0, a1 = int(batch.aln_begin[t]), int(batch.aln_begin[t + 1])
        if a1 == a0 or a1 - a0 < min_cov:
            out.append([])
            continue
        bb = None
        if batch.backbone is not None:
            o = int(batch.backbone_off[t])
            bb = batch.backbone[o:o + int(batch.tlen[t])].tobytes()
        out.append(target_positions(int(batch.tlen[t]), batch.target_alignments(t), min_len, trim, min_weight, bb))
    return out
