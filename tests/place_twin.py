"""CPU twin of dagcon_place (include/dagcon.h, k_place.hip.h): k-mer diagonal placement of a query on a target.

This build's own definition (the reference delegates the step to blasr); the device reproduces it bit for bit.
"""
import numpy as np

MAX_LEN = 65536
BIN_SHIFT = 6

_CODE = np.full(256, 4, np.uint8)
for _ch, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CODE[_ch] = _v
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(x: bytes) -> bytes:
    return x.translate(_RC)[::-1]


def kmers(x: bytes, k: int):
    """(values, valid) of the k-mers at positions 0 .. |x| - k: 2 bits a base, the first base most significant."""
    c = _CODE[np.frombuffer(x, np.uint8)] if x else np.zeros(0, np.uint8)
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    bad = np.concatenate(([0], np.cumsum(c == 4)))
    valid = bad[k:k + n] == bad[:n]
    cc = (c & 3).astype(np.int64)
    v = np.zeros(n, np.int64)
    for m in range(k):
        v = (v << 2) | cc[m:m + n]
    return v, valid


class TargetIndex:
    """The unmasked k-mers of a target, sorted by value: positions of values that occur at most max_occ times."""

    def __init__(self, t: bytes, k: int, max_occ: int):
        v, ok = kmers(t, k)
        j = np.flatnonzero(ok)
        key = v[j]
        order = np.argsort(key, kind="stable")
        key, j = key[order], j[order]
        if key.size:
            u, first, cnt = np.unique(key, return_index=True, return_counts=True)
            keep = np.repeat(cnt <= max_occ, cnt)
            key, j = key[keep], j[keep]
        self.key, self.pos, self.len = key, j, len(t)

    def votes(self, xk):
        """(i, j) of every vote on the target of x, given as kmers(x, k)."""
        v, ok = xk
        i = np.flatnonzero(ok)
        key = v[i]
        lo = np.searchsorted(self.key, key, "left")
        hi = np.searchsorted(self.key, key, "right")
        cnt = hi - lo
        tot = int(cnt.sum())
        if tot == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        rep = np.repeat(np.arange(i.size), cnt)
        within = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return i[rep], self.pos[lo[rep] + within]


def _argmax(h):
    """(count, smallest bin reaching it); (0, 0) for no votes."""
    if h.size == 0:
        return 0, 0
    b = int(np.argmax(h))
    return int(h[b]), b


def place(q: bytes, t: bytes, k: int = 12, max_occ: int = 4, index: TargetIndex = None, qk=None):
    """(votes_fwd, votes_rev, strand, t0, t1) of q on t; strand is '+', '-' or '.'.  qk: (kmers(q), kmers(rc(q)))."""
    lq, lt = len(q), len(t)
    if index is None:
        index = TargetIndex(t, k, max_occ)
    if qk is None:
        qk = (kmers(q, k), kmers(rc(q), k))
    per = []
    for xk in qk:
        i, j = index.votes(xk)
        b = (j - i + lq) >> BIN_SHIFT
        per.append((i, b, _argmax(np.bincount(b))))
    (vf, bf), (vr, br) = per[0][2], per[1][2]
    if vf == 0 and vr == 0:
        return 0, 0, ".", 0, 0
    s = 0 if vf >= vr else 1
    i, b, (_, B) = per[s]
    R = 2 + -(-lq // 512)
    cons = np.abs(b - B) <= R
    quarter = (4 * i) // lq
    ends = []
    for qq in (0, 3):
        sel = b[cons & (quarter == qq)]
        ends.append(_argmax(np.bincount(sel))[1] if sel.size else B)
    t0 = min(max(64 * ends[0] + 32 - lq, 0), lt)
    t1 = min(max(64 * ends[1] + 32, 0), lt)
    return vf, vr, "+-"[s], t0, t1


def place_pairs(seqs, pairs, k=12, max_occ=4):
    """dagcon_place's outputs for pairs = [(q, t)] over seqs, as Context.place returns them."""
    n = len(pairs)
    out = {name: np.zeros(n, np.uint32) for name in ("votes_fwd", "votes_rev", "t0", "t1")}
    strand = bytearray(n)
    cache, qk = {}, {}
    for a, (qi, ti) in enumerate(pairs):
        if ti not in cache:
            cache = {ti: TargetIndex(seqs[ti], k, max_occ)}     # pairs usually come grouped by target
        if qi not in qk:
            qk[qi] = (kmers(seqs[qi], k), kmers(rc(seqs[qi]), k))
        vf, vr, s, t0, t1 = place(seqs[qi], seqs[ti], k, max_occ, cache[ti], qk[qi])
        out["votes_fwd"][a], out["votes_rev"][a], out["t0"][a], out["t1"][a] = vf, vr, t0, t1
        strand[a] = ord(s)
    out["strand"] = bytes(strand)
    return out
