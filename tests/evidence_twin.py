"""CPU twin of dagcon_edit_support (include/dagcon.h has the rule): the alignments behind each edit, column by column in
plain Python.  The edits come from edits_twin.batch_edits or from the device's own arrays; the alignments are normalised
and trimmed with oracle.normalize_gaps / oracle.trim_aln as edits_twin.target_kinds does.

    edit_windows(T, S, t0, t1, edits, extend)      -> [(L, R)] per edit
    segment_groups(T, S, t0, t1, edits, extend)    -> [(first, last + 1, gL, gR, cL, cR)]
    columns(alns, min_len, trim)                   -> [(s0, q, t)] the alignments counted
    classify(tlen, s0, q, t, gL, gR, ref, alt)     -> None (not spanning) | "alt" | "ref" | "other"
    target_support(T, alns, segs, min_len, trim)   -> per segment, per edit (w_begin, w_end, span, alt, ref)
"""
import bisect

GAP = 0x2D


def sim(x, y):
    return ((x ^ y) & 0xDF) == 0


def sim_bytes(a, b):
    return len(a) == len(b) and all(sim(x, y) for x, y in zip(a, b))


def edit_windows(T, S, t0, t1, edits, extend=True):
    out = []
    for i, (tp, tl, c, cl) in enumerate(edits):
        L, R = tp, tp + tl
        lo = edits[i - 1][0] + edits[i - 1][1] if i else t0
        hi = edits[i + 1][0] if i + 1 < len(edits) else t1
        if extend and (tl == 0) != (cl == 0):
            u = S[c:c + cl] if cl else T[tp:tp + tl]
            k, j = len(u), 0
            while L > lo and sim(T[L - 1], u[(k - 1 - j) % k]):
                L -= 1; j += 1
            j = 0
            while R < hi and sim(T[R], u[j % k]):
                R += 1; j += 1
        out.append((L, R))
    return out


def segment_groups(T, S, t0, t1, edits, extend=True):
    win = edit_windows(T, S, t0, t1, edits, extend)
    groups, first = [], 0
    for i in range(1, len(edits) + 1):
        if i < len(edits) and win[i][0] <= win[i - 1][1]:
            continue
        gL, gR = win[first][0], win[i - 1][1]
        tpf, _, cf, _ = edits[first]
        tpl, tll, cl_, cll = edits[i - 1]
        groups.append((first, i, gL, gR, cf - (tpf - gL), cl_ + cll + (gR - tpl - tll)))
        first = i
    return groups


def columns(alns, min_len, trim):
    import oracle
    out = []
    for start, q, t in alns:
        if len(q) < min_len:
            continue
        q, t = oracle.normalize_gaps(q, t)
        q, t, start = oracle.trim_aln(q, t, start, trim)
        if q:
            out.append((start - 1, bytes(q), bytes(t)))
    return out


def coords(s0, t):
    """Per column its coordinate tc (s0 plus the target-base columns in front of it), and e0."""
    tcs, x = [], s0
    for tb in t:
        tcs.append(x)
        x += tb != GAP
    return tcs, x


def classify(tlen, s0, q, t, gL, gR, ref, alt, pre=None):
    tcs, e0 = pre if pre is not None else coords(s0, t)
    if not ((s0 <= gL - 1) if gL > 0 else s0 == 0):
        return None
    if not ((e0 - 1 >= gR) if gR < tlen else e0 == tlen):
        return None
    # (tcs never falls: only the columns with gL - 1 <= tc <= gR matter)
    near = range(bisect.bisect_left(tcs, gL - 1), bisect.bisect_right(tcs, gR))
    allele = bytes(q[i] for i in near
                   if q[i] != GAP and tcs[i] >= gL and (tcs[i] < gR or (tcs[i] == gR and t[i] == GAP)))
    good = True
    for b, exists in ((gL - 1, gL > 0), (gR, gR < tlen)):
        if exists:
            (i,) = [i for i in near if t[i] != GAP and tcs[i] == b]
            good = good and sim(q[i], t[i])
    if good and sim_bytes(allele, alt):
        return "alt"
    if good and sim_bytes(allele, ref):
        return "ref"
    return "other"


def target_support(T, alns, segs, min_len, trim, extend=True):
    """segs: [(seq, t0, t1, [(t_pos, t_len, c, c_len)])] of one target, c relative to seq.  Per segment a list with one
    (w_begin, w_end, span, alt, ref) per edit."""
    cols = [(s0, q, t, coords(s0, t)) for s0, q, t in columns(alns, min_len, trim)]
    out = []
    for S, t0, t1, edits in segs:
        per = [None] * len(edits)
        for first, end, gL, gR, cL, cR in segment_groups(T, S, t0, t1, edits, extend):
            assert 0 <= gL <= gR <= len(T) and 0 <= cL <= cR <= len(S)
            n = {"alt": 0, "ref": 0, "other": 0}
            for s0, q, t, pre in cols:
                k = classify(len(T), s0, q, t, gL, gR, T[gL:gR], S[cL:cR], pre)
                if k:
                    n[k] += 1
            for i in range(first, end):
                per[i] = (gL, gR, n["alt"] + n["ref"] + n["other"], n["alt"], n["ref"])
        out.append(per)
    return out
