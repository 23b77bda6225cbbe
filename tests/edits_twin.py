"""CPU twin of dagcon_edits (include/dagcon.h): where a consensus segment differs from its target, read off the kinds
and positions of the best path, nothing aligned.  numpy / Python; the oracle is imported only by target_kinds, which
reads kinds and _bbMap off its graph as window_twin.target_positions reads positions.

    target_kinds(tlen, alns, ...)                    -> [(range0, range1, seq, positions, kinds)] | None
    segment_edits(target, pos, kind, seq, c_base)    -> (t0, t1, [(t_pos, t_len, c_off, c_len)])
    apply_edits(target, t0, t1, edits, seq_blob)     -> bytes: the invariant's left side
    batch_edits(targets, ...)                        -> per target [(seq, t0, t1, edits with c_off relative to seq)]
    stitch_edits(windows, min_len)                   -> the stitch of window_twin.stitch with every piece's edits
"""
import ctypes as C

GAP = 0x2D


def target_kinds(tlen, alns, min_len=500, trim=50, min_weight=6):
    """[(range0, range1, seq, positions, kinds)] of one target as main.cpp:130-138 builds its graph ('N' backbone):
    per consensus base the _bbMap of its best-path vertex and whether that vertex is a backbone vertex.  None for a
    target the reference would not accept."""
    import oracle
    g = oracle.Graph(blen=tlen)
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

    def node(v):
        base = C.create_string_buffer(1)
        w, cv, d, bb, bm = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        g.L.og_node_info(g.g, v, base, C.byref(w), C.byref(cv), C.byref(d), C.byref(bb), C.byref(bm))
        return base.raw, bm.value, bool(bb.value)
    eb, xb = node(0)[0], node(tlen + 1)[0]
    ps, ks = [], []
    for v in g.best_path():
        base, bm, bb = node(v)
        if base in (eb, xb):
            continue
        ps.append(bm); ks.append(bb)
    return [(r0, r1, s, ps[r0:r1], ks[r0:r1]) for r0, r1, s in g.consensus_all(min_weight, min_len)]


def _trim(target, seq, t_pos, t_len, c, c_len):
    while t_len and c_len and target[t_pos] == seq[c]:
        t_pos += 1; c += 1; t_len -= 1; c_len -= 1
    while t_len and c_len and target[t_pos + t_len - 1] == seq[c + c_len - 1]:
        t_len -= 1; c_len -= 1
    return t_pos, t_len, c, c_len


def segment_edits(target, pos, kind, seq, c_base=0):
    """The definition, base by base from the front.  target: the bytes positions refer to (a window's own); pos / kind
    / seq: one segment.  (t0, t1, [(t_pos, t_len, c_off, c_len)]) with c_off = c_base + the index in seq."""
    n = len(seq)
    assert len(pos) == len(kind) == n
    bbs = [i for i in range(n) if kind[i]]
    if not bbs:
        t0 = int(pos[0]) - 1
        return t0, t0, [(t0, 0, c_base, n)]
    assert all(pos[a] < pos[b] for a, b in zip(bbs, bbs[1:])), "backbone positions must rise strictly"
    t0, t1 = int(pos[bbs[0]]) - 1, int(pos[bbs[-1]])
    out = []
    if bbs[0] > 0:
        out.append((t0, 0, c_base, bbs[0]))
    for a, b in zip(bbs, bbs[1:]):
        c_len, t_len = b - a - 1, int(pos[b]) - int(pos[a]) - 1
        if not (c_len or t_len):
            continue
        t_pos, t_len, c, c_len = _trim(target, seq, int(pos[a]), t_len, a + 1, c_len)
        if t_len or c_len:
            out.append((t_pos, t_len, c_base + c, c_len))
    if bbs[-1] < n - 1:
        out.append((t1, 0, c_base + bbs[-1] + 1, n - 1 - bbs[-1]))
    return t0, t1, out


def apply_edits(target, t0, t1, edits, seq_blob):
    """target[t0:t1] with [t_pos, t_pos + t_len) replaced by seq_blob[c_off : c_off + c_len] for every edit, which must
    be ascending, disjoint and inside [t0, t1]."""
    out, at = [], t0
    for t_pos, t_len, c_off, c_len in edits:
        t_pos, t_len, c_off, c_len = int(t_pos), int(t_len), int(c_off), int(c_len)
        assert at <= t_pos and t_pos + t_len <= t1, "edits out of order, overlapping or outside the span"
        out.append(bytes(target[at:t_pos]))
        out.append(bytes(seq_blob[c_off:c_off + c_len]))
        at = t_pos + t_len
    out.append(bytes(target[at:t1]))
    return b"".join(out)


def batch_edits(targets, min_cov, min_len, trim):
    """targets = [(target bytes, [(start, q, t)])] (one per target or per window): per target
    [(seq, t0, t1, [(t_pos, t_len, c, c_len)])], c relative to seq; [] below min_cov; None where the reference would
    not accept the target."""
    out = []
    for tseq, alns in targets:
        if not alns or len(alns) < min_cov:
            out.append([])
            continue
        segs = target_kinds(len(tseq), alns, min_len, trim, min_cov)
        out.append(None if segs is None else [(s,) + segment_edits(tseq, ps, ks, s) for _, _, s, ps, ks in segs])
    return out


def stitch_edits(windows, min_len):
    """The joined pieces of one target with their edits (csrc/host/windows.h, DgStitch), base by base.  windows: in
    order, (begin, core begin, core end, [(seq, pos, t0, edits)]): a window's segments with their positions (1-based,
    relative to the window), span begin and edits as segment_edits gives them (t_pos relative to the window, c_off to
    seq).  Returns [(t0, t1, seq, e0, e1, [(t_pos, t_len, c_off, c_len)])] in target coordinates, c_off into the
    piece: t0_t1 is the record's name, [e0, e1) the span the edits apply to.

    The kept part [i0, i1) is window_twin.stitch's.  Every base of a segment either equals a target base or is an
    inserted base of one edit; an edit's target bases stand in front of the base behind the edit and go where that
    base goes.  A piece stands at a target position `at`.  A fresh piece starts at its first kept base's target base
    (behind a leading deletion; inserted bases: where their edit ends if its target bases are the part's, else where
    it begins), never in front of the end of the piece before it; a continued piece goes on where it stood.  Then, base
    by base: target bases between `at` and the base's own place are deleted; a base whose place lies in front of `at`
    is an inserted base there.  Runs of deletions and inserted bases with no equal base between them are one edit."""
    pieces, open_w, last_end = [], None, 0
    for wi, (begin, c0, c1, segs) in enumerate(windows):
        for seq, pos, t0, edits in segs:
            n = len(seq)
            g = [int(x) + begin for x in pos]
            i0 = next((i for i in range(n) if g[i] > c0), n)
            i1 = next((i for i in range(i0, n) if g[i] > c1), n)
            if i1 <= i0:
                continue
            tgt, ins_at, start_at, skip = [None] * n, [None] * n, [None] * n, {}
            c, t = 0, t0 + begin
            for tp, tl, co, cl in edits:
                tp += begin
                for i in range(c, co):
                    tgt[i] = t + (i - c)
                behind = co + cl
                for i in range(co, behind):
                    ins_at[i] = tp
                    start_at[i] = tp + tl if i0 <= behind < i1 else tp
                if tl:
                    skip[behind] = tp + tl
                c, t = behind, tp + tl
            for i in range(c, n):
                tgt[i] = t + (i - c)
            if i0 > 0 and open_w is not None and open_w == wi - 1 and pieces:
                p = pieces[-1]
                at = p["e1"]
            else:
                first = skip[i0] if i0 in skip else tgt[i0] if tgt[i0] is not None else start_at[i0]
                at = max(first, last_end)
                p = dict(t0=g[i0] - 1, seq=bytearray(), e0=at, ev=[])
                pieces.append(p)
            p["t1"] = g[i1 - 1]
            for i in range(i0, i1):
                k = len(p["seq"])
                if i in skip and skip[i] > at:
                    p["ev"].append(("D", at, skip[i] - at, k)); at = skip[i]
                x = tgt[i]
                if x is None:
                    if ins_at[i] > at:
                        p["ev"].append(("D", at, ins_at[i] - at, k)); at = ins_at[i]
                    p["ev"].append(("I", at, 1, k))
                elif x < at:
                    p["ev"].append(("I", at, 1, k))
                else:
                    if x > at:
                        p["ev"].append(("D", at, x - at, k))
                    p["ev"].append(("M", x, 1, k)); at = x + 1
                p["seq"].append(seq[i])
            p["e1"] = last_end = at
            open_w = wi if i1 < n else None
    out = []
    for p in pieces:
        if len(p["seq"]) < min_len:
            continue
        edits, run = [], None
        for what, at, ln, k in p["ev"] + [("M", 0, 0, 0)]:
            if what == "M":
                if run:
                    edits.append(tuple(run))
                run = None
                continue
            if run is None:
                run = [at, 0, k, 0]
            run[1 if what == "D" else 3] += ln
        out.append((p["t0"], p["t1"], bytes(p["seq"]), p["e0"], p["e1"], edits))
    return out
