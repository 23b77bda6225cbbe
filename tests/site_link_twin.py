"""CPU twin of dagcon_site_link (include/dagcon.h, rule 13): which sites of a target are carried by the same reads as other
sites near them, in plain Python on site_reads_twin's arrays.  Python ints serve as bit rows: bit x of a row is alignment
x of the target's taken alignments.

    options(max_conflict_ppm, min_cell, min_partners, reach) -> the four values with the defaults filled in
    rows(ents, counts)                          -> (P, M): per site the alignments with M = +1 and those with M = -1
    cells(Pi, Mi, Pj, Mj)                       -> (pp, mm, pm, mp)
    pair(Pi, Mi, Pj, Mj, opts)                  -> partners or not
    link(ents, counts, opts)                    -> (partners per site, linked per site)
    muted(ents, linked)                         -> the entries at linked sites (an entry with M = 0 takes no part in anything)
    target(tlen, alns, min_len, trim, site_opts, rounds, link_opts, hap, min_cov) -> site_reads_twin.target's dict, the split
                                                   run on the muted entries, with partners, linked and the tally
    linked_sites_line(rname, pos0, partners, linked) -> a line of pbdagcon --linked-sites
"""
import hap_twin as ht
import site_reads_twin as srt

DEFAULTS = (100000, 3, 2, 256)
MAX_REACH = 4096


def options(max_conflict_ppm=0, min_cell=0, min_partners=0, reach=0):
    return tuple(v or d for v, d in zip((max_conflict_ppm, min_cell, min_partners, reach), DEFAULTS))


def rows(ents, counts):
    P, M = [0] * len(counts), [0] * len(counts)
    for x, e in enumerate(ents):
        for k, code in e:
            m = srt.sign(code, counts[k])
            if m > 0:
                P[k] |= 1 << x
            elif m < 0:
                M[k] |= 1 << x
    return P, M


def _pop(v):
    return bin(v).count("1")


def cells(Pi, Mi, Pj, Mj):
    return _pop(Pi & Pj), _pop(Mi & Mj), _pop(Pi & Mj), _pop(Mi & Pj)


def pair_cells(pp, mm, pm, mp, opts):
    same, diff = pp + mm, pm + mp
    lo, hi = min(same, diff), max(same, diff)
    cell = min(pp, mm) if same >= diff else min(pm, mp)
    return lo * 1000000 <= opts[0] * (lo + hi) and cell >= opts[1]


def pair(Pi, Mi, Pj, Mj, opts):
    return pair_cells(*cells(Pi, Mi, Pj, Mj), opts)


def link(ents, counts, opts):
    """opts: options()'s four values.  Sites i and j are compared when their indices differ by at most reach."""
    P, M = rows(ents, counts)
    n = len(counts)
    reach, min_partners = opts[3], opts[2]
    partners = [0] * n
    for i in range(n):
        for j in range(i + 1, min(n, i + reach + 1)):
            if pair(P[i], M[i], P[j], M[j], opts):
                partners[i] += 1
                partners[j] += 1
    return partners, [int(p >= min_partners) for p in partners]


def muted(ents, linked):
    return [[(k, code) for k, code in e if linked[k]] for e in ents]


def target(tlen, alns, min_len, trim, site_opts=(0, 0), rounds=srt.ROUNDS, link_opts=None, hap=(0, 0), min_cov=0):
    """link_opts None: the switch off, site_reads_twin.target's own split.  The entries stay as they are; "signed" counts
    an alignment's entries with M != 0 under the mute, and the tally reads the same signs."""
    tw = srt.target(tlen, alns, min_len, trim, site_opts, rounds)
    sc = [tw["counts"][p] for p in tw["sites"]]
    read = tw["ents"]
    if link_opts is not None:
        tw["partners"], tw["linked"] = link(tw["ents"], sc, link_opts)
        read = muted(tw["ents"], tw["linked"])
        tw["hap"], tw["phase"] = srt.split(read, sc, rounds)
        tw["signed"] = [sum(1 for k, code in e if srt.sign(code, sc[k])) for e in read]
    tw["tally"] = ht.tally(dict(tw, ents=read), ht.held(alns, min_len), hap[0], hap[1], min_cov)
    return tw


def linked_sites_line(rname, pos0, partners, linked):
    return "\t".join([rname, str(pos0 + 1), str(partners), str(linked)])
