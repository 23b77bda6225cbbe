"""CPU twin of dagcon_pileup / dagcon_pileup_sites (include/dagcon.h has the rule): what the alignments show at every
target position, column by column in plain Python on evidence_twin.columns / coords -- the alignments as the graph took
them (min_len, normalize_gaps, trim_aln, not empty).

    target_counts(tlen, alns, min_len, trim)   -> [[A, C, G, T, N, DEL, INS, 0]] per position
    sites(counts, min_count, min_frac_ppm)     -> [position] ascending
    line(name, pos0, ref, n)                   -> the text line of pbdagcon --pileup / --sites (no newline)
"""
import evidence_twin as ev

GAP = ev.GAP
A, C, G, T, N, DEL, INS = range(7)
LETTER = {ord("A"): A, ord("C"): C, ord("G"): G, ord("T"): T}


def target_counts(tlen, alns, min_len, trim):
    counts = [[0] * 8 for _ in range(tlen)]
    for s0, q, t in ev.columns(alns, min_len, trim):
        tcs, _ = ev.coords(s0, t)
        for i, (qb, tb) in enumerate(zip(q, t)):
            tc = tcs[i]
            if tb != GAP:
                counts[tc][DEL if qb == GAP else LETTER.get(qb & 0xDF, N)] += 1
            elif qb != GAP and i > 0 and t[i - 1] != GAP:
                # the first column of an insertion run: it belongs to the target base in front of it
                counts[tc - 1][INS] += 1
    return counts


def depth(n):
    return sum(n[:6])


def is_site(n, min_count, min_frac_ppm):
    d = depth(n)
    if d == 0:
        return False
    s2 = sorted(n[:6])[-2]
    m = max(s2, min(n[INS], d - n[INS]))
    return m >= min_count and m * 1000000 >= min_frac_ppm * d


def sites(counts, min_count, min_frac_ppm):
    return [p for p, n in enumerate(counts) if is_site([int(x) for x in n], min_count, min_frac_ppm)]


def line(name, pos0, ref, n):
    """ref: the target's byte (an int), or None for '.'."""
    return "\t".join([name, str(pos0 + 1), chr(ref) if ref is not None else ".", str(depth(n))] + [str(int(x)) for x in n[:7]])
