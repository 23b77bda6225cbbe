"""Per-base support (DAGCON_FLAG_BASE_SUPPORT) and the --fastq quality, computed on the CPU.

The support is read off the C oracle without changing it: oracle.Graph built as main.cpp:130-138 does (min_len filter,
normalizeGaps, trimAln, addAln), mergeNodes, bestPath; for every path vertex v that gives a consensus base (enter and exit
skipped, as consensus_all does) its weight and the coverage of _bbMap[v], then sliced by the oracle's segments.
The quality is the exact integer definition of pbdagcon_amd/csrc/host/fastq.h."""
import ctypes as C

import oracle


def quality(weight, depth):
    """Largest q >= 0 with 10^q * x^10 <= (c + 2)^10, c = max(depth, weight), x = c - weight + 1."""
    c = max(int(depth), int(weight))
    x = c - int(weight) + 1
    lhs, rhs = x ** 10, (c + 2) ** 10
    q = 0
    while lhs * 10 <= rhs:
        lhs *= 10
        q += 1
    return q


def quality_string(weights, depths):
    return bytes(33 + quality(w, d) for w, d in zip(weights, depths))


def fastq_record(name, seq, weights, depths):
    """'@' name, the sequence, '+', the qualities (name without the '@')."""
    return b"@%s\n%s\n+\n%s\n" % (name, seq, quality_string(weights, depths))


def _node(L, g, v):
    base = C.create_string_buffer(1)
    w, cv, d, bb, bm = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    L.og_node_info(g, v, base, C.byref(w), C.byref(cv), C.byref(d), C.byref(bb), C.byref(bm))
    return base.raw, w.value, cv.value, bm.value


def consensus_target_support(tlen, alns, min_len=500, trim=50, min_weight=6, backbone=None, raw=False):
    """oracle.consensus_target with the support: [(range0, range1, seq, weights, depths)].  alns = [(start, q, t)].
    None for a target the reference would not accept (an alignment leaves the backbone)."""
    g = oracle.Graph(backbone=backbone) if backbone is not None else oracle.Graph(blen=tlen)
    for start, q, t in alns:
        if len(q) < min_len:                                    # main.cpp:132
            continue
        if not raw:
            q, t = oracle.normalize_gaps(q, t)
            q, t, start = oracle.trim_aln(q, t, start, trim)
        tb = sum(1 for ch in t if ch != 0x2D)
        if q and (start < 1 or start - 1 + tb > tlen):
            return None
        g.add_aln(start, q, t)
    if g.merge_nodes() != 0:
        return None
    path = g.best_path()
    L = g.L
    eb, xb = _node(L, g.g, 0)[0], _node(L, g.g, tlen + 1)[0]
    ws, ds = [], []
    for v in path:
        base, w, _, bm = _node(L, g.g, v)
        if base in (eb, xb):
            continue
        ws.append(w)
        ds.append(_node(L, g.g, bm)[2])
    segs = g.consensus_all(min_weight, min_len)
    return [(r0, r1, s, ws[r0:r1], ds[r0:r1]) for r0, r1, s in segs]


def batch_support(batch, min_cov=6, min_len=500, trim=50, min_weight=None):
    """util.oracle_batch with the support, per target [(range0, range1, seq, weights, depths)]."""
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
        out.append(consensus_target_support(int(batch.tlen[t]), batch.target_alignments(t), min_len, trim, min_weight, bb))
    return out
