"""CPU twin of dagcon_site_reads (include/dagcon.h has the rule): which alignment shows which allele at each site of the
pile-up, and the two-way split of a target's alignments, in plain Python on evidence_twin.columns / coords and pileup_twin.

    taken(alns, min_len, trim)                  -> [(src, s0, q, t)] the taken alignments, src the index in alns
    entries(alns, min_len, trim, sites)         -> per taken alignment [(k, code)], k an index into sites (ascending positions)
    kind(n)                                     -> ("ins",) | ("base", k1, k2 or None) from a site's eight counts
    sign(code, n)                               -> M in {+1, 0, -1}
    split(ents, counts, rounds)                 -> (hap per alignment, phase per site); counts: the sites' eight counts
    target(tlen, alns, min_len, trim, opts, rounds) -> dict of one target's arrays
"""
import evidence_twin as ev
import pileup_twin as pt

GAP = ev.GAP
ROUNDS = 8


def taken(alns, min_len, trim):
    """evidence_twin.columns with the index each alignment came by (columns drops without saying which)."""
    out = []
    for src, aln in enumerate(alns):
        cols = ev.columns([aln], min_len, trim)
        if cols:
            out.append((src,) + cols[0])
    return out


def entries(alns, min_len, trim, sites):
    idx = {p: k for k, p in enumerate(sites)}
    out = []
    for _, s0, q, t in taken(alns, min_len, trim):
        tcs, _ = ev.coords(s0, t)
        # the pile-up's INS rule: the first column of a run counts at the base in front of it
        anchors = {tcs[i] - 1 for i in range(1, len(t)) if t[i] == GAP and q[i] != GAP and t[i - 1] != GAP}
        ent = []
        for i, (qb, tb) in enumerate(zip(q, t)):
            if tb != GAP and tcs[i] in idx:
                cls = pt.DEL if qb == GAP else pt.LETTER.get(qb & 0xDF, pt.N)
                ent.append((idx[tcs[i]], cls | (8 if tcs[i] in anchors else 0)))
        out.append(ent)
    return out


def kind(n):
    n = [int(x) for x in n]
    six = n[:6]
    d = sum(six)
    s2 = sorted(six)[-2]
    if min(n[pt.INS], d - n[pt.INS]) > s2:
        return ("ins",)
    k1 = max(range(6), key=lambda k: (six[k], -k))
    rest = [k for k in range(6) if k != k1]
    k2 = max(rest, key=lambda k: (six[k], -k))
    return ("base", k1, k2 if six[k2] > 0 else None)


def sign(code, n):
    kd = kind(n)
    if kd[0] == "ins":
        return -1 if code & 8 else 1
    cls = code & 7
    return 1 if cls == kd[1] else -1 if cls == kd[2] else 0


def sgn(x):
    return (x > 0) - (x < 0)


def split(ents, counts, rounds=ROUNDS, trace=None):
    """ents: per alignment [(k, code)]; counts[k]: the eight counts of site k.  trace: a list that gets (h, sigma) per round."""
    M = [{k: sign(code, counts[k]) for k, code in e} for e in ents]
    nz = [sum(1 for v in m.values() if v) for m in M]
    h = [0] * len(ents)
    sigma = [0] * len(counts)
    if not any(nz):
        return h, sigma
    seed = max(range(len(ents)), key=lambda x: (nz[x], -x))
    for k, v in M[seed].items():
        sigma[k] = v
    for _ in range(rounds):
        h = [sgn(sum(v * sigma[k] for k, v in m.items())) for m in M]
        acc = [0] * len(counts)
        for x, m in enumerate(M):
            for k, v in m.items():
                acc[k] += v * h[x]
        sigma = [sgn(a) for a in acc]
        if trace is not None:
            trace.append((list(h), list(sigma)))
    return [{1: 1, -1: 2, 0: 0}[v] for v in h], sigma


def target(tlen, alns, min_len, trim, opts=(0, 0), rounds=ROUNDS):
    """One target with a graph: counts, sites, the taken alignments' src, their entries, hap and phase, signed entries."""
    counts = pt.target_counts(tlen, alns, min_len, trim)
    sites = pt.sites(counts, *opts)
    tk = taken(alns, min_len, trim)
    ents = entries(alns, min_len, trim, sites)
    sc = [counts[p] for p in sites]
    hap, phase = split(ents, sc, rounds)
    return {"counts": counts, "sites": sites, "src": [x[0] for x in tk], "ents": ents, "hap": hap, "phase": phase,
            "signed": [sum(1 for k, code in e if sign(code, sc[k])) for e in ents]}


ALLELE = "ACGTN*"


def site_reads_line(rname, pos0, qname, code):
    return "\t".join([rname, str(pos0 + 1), qname, ALLELE[code & 7], str(code >> 3)])


def haplotag_line(rname, qname, hap, n_signed):
    return "\t".join([rname, qname, str(hap), str(n_signed)])
