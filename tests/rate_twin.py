"""CPU twin of the record filter (include/dagcon.h, dagcon_set_record_filter): the rating of one record from its ops,
its bases, its strand and its nibbles, and the pick -- error threshold, depth cap, order.  Plain Python: imports
neither the product nor the oracle.

    read_base(q, i, q_len, reverse=False, packed=False)     the byte the expansion writes for read base i
    rate(pos, q, t, ops, reverse=False, packed=False, q_len=None) -> (match, mismatch, ins, del)
    columns(ops)                                            the scan's column total
    passes(counts, max_error_ppm)
    cap(matches, depth)                                     positions kept of a list of record-level match counts
    pick(targets, max_error_ppm, max_depth, windows=None, reverse=None, packed=False) -> Pick
    parse_ppm(text)                                         --max-error's text as ppm, None for anything else
"""
import cigar_twin as ct
import window_twin as wt

NT16 = b"=ACMGRSVTWYHKDBN"
FATE_MAX_ERROR, FATE_MAX_DEPTH, FATE_NONCONFORMING = 1, 2, 4
_PAIR = {65: 84, 84: 65, 67: 71, 71: 67, 97: 116, 116: 97, 99: 103, 103: 99}


def read_base(q, i, q_len, reverse=False, packed=False):
    if packed:
        return NT16[(q[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15]
    if reverse:
        b = q[q_len - 1 - i]
        return _PAIR.get(b, b)
    return q[i]


def columns(ops):
    return sum(int(o) >> 4 for o in ops if (int(o) & 15) in ct._COL)


def rate(pos, q, t, ops, reverse=False, packed=False, q_len=None):
    """(match, mismatch, ins, del) of a conforming record, column by column."""
    q, t = bytes(q), bytes(t)
    if q_len is None:
        assert not packed
        q_len = len(q)
    qi, ti = 0, pos - 1
    m = x = ins = dele = 0
    for o in ops:
        code, n = int(o) & 15, int(o) >> 4
        if code in (ct.M, ct.EQ, ct.X):
            for k in range(n):
                if (read_base(q, qi + k, q_len, reverse, packed) & 0xDF) == (t[ti + k] & 0xDF):
                    m += 1
                else:
                    x += 1
            qi += n; ti += n
        elif code == ct.I:
            ins += n; qi += n
        elif code == ct.D:
            dele += n; ti += n
        elif code == ct.S:
            qi += n
    assert qi == q_len
    return m, x, ins, dele


def passes(counts, max_error_ppm):
    m, x, i, d = (int(v) for v in counts)
    return (x + i + d) * 1000000 <= int(max_error_ppm) * (m + x + i + d)


def cap(matches, depth):
    """Of a list of records' match counts, in the records' own order: the positions that stay under a cap of depth (0:
    off) -- the depth largest, a tie to the earlier one -- ascending."""
    if not depth or len(matches) <= depth:
        return list(range(len(matches)))
    order = sorted(range(len(matches)), key=lambda i: (-int(matches[i]), i))
    return sorted(order[:depth])


class Pick:
    """counts: per record (flat, batch order) its four counts; fate: per record the FATE_* bits; kept: per target
    (windows: per window) the in-target indices of the records that go into the graph, in their own order."""

    def __init__(self, counts, fate, kept):
        self.counts, self.fate, self.kept = counts, fate, kept

    def n_over_error(self):
        return sum(1 for f in self.fate if f & FATE_MAX_ERROR)

    def n_over_depth(self):
        return sum(1 for f in self.fate if f & FATE_MAX_DEPTH)


def pick(targets, max_error_ppm=1000000, max_depth=0, windows=None, reverse=None, packed=False):
    """targets = [(target bases, [(pos, read bases, ops)])] (read bases as the batch carries them: reverse is the flat
    per-record strand list of a stranded batch; packed: (nibble bytes, q_len) instead of read bases); windows = [(target
    index, begin, end)] or None."""
    counts, fate, first = [], [], []
    for bb, recs in targets:
        first.append(len(counts))
        for p, q, o in recs:
            q, ql = q if packed else (q, len(q))
            if not ct.conforming(p, ql, len(bb), o):
                counts.append((0, 0, 0, 0)); fate.append(FATE_NONCONFORMING)
                continue
            c = rate(p, q, bb, o, bool(reverse[len(counts)]) if reverse is not None else False, packed, ql)
            assert sum(c) == columns(o)
            counts.append(c)
            fate.append(0 if passes(c, max_error_ppm) else FATE_MAX_ERROR)
    groups = []                                       # per target / window: the flat indices of its candidates
    if windows is None:
        for g, (bb, recs) in enumerate(targets):
            groups.append((g, [first[g] + k for k in range(len(recs)) if fate[first[g] + k] == 0]))
    else:
        for g, a, b in windows:
            bb, recs = targets[g]
            mine = []
            for k, (p, q, o) in enumerate(recs):
                s, e = wt.span(p, len(bb), o)
                if max(a, s) < min(b, e) and fate[first[g] + k] == 0:
                    mine.append(first[g] + k)
            groups.append((g, mine))
    kept = []
    for g, mine in groups:
        stay = cap([counts[i][0] for i in mine], max_depth)
        for j, i in enumerate(mine):
            if j not in stay:
                fate[i] |= FATE_MAX_DEPTH
        kept.append([mine[j] - first[g] for j in stay])
    return Pick(counts, fate, kept)


def parse_ppm(text):
    """'0' or '1', optionally a point and one to six digits, at most 1: the value in parts per million; else None."""
    if not text or text[0] not in "01":
        return None
    frac = ""
    if len(text) > 1:
        if text[1] != "." or not 1 <= len(text) - 2 <= 6 or not text[2:].isdigit() or not text[2:].isascii():
            return None
        frac = text[2:]
    v = int(text[0]) * 1000000 + (int(frac.ljust(6, "0")) if frac else 0)
    return v if v <= 1000000 else None
