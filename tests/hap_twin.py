"""CPU twin of dagcon_hap_tally and of the groups of dagcon_upload_haps (include/dagcon.h, rules 6 and 7), in plain Python
on site_reads_twin.target's arrays.

    site_counts(ents, counts, hap)              -> per site [P1, M1, P2, M2]
    tally(tw, K, min_sites, min_reads, min_cov, ok) -> dict of one target's numbers; tw: site_reads_twin.target's dict
    held(alns, min_len)                         -> K: the alignments the pipeline holds for the target
    groups(alns, min_len, src, hap)             -> ([indices into alns of group 1], [of group 2])
    target_line / site_line / fasta_name        -> the lines of pbdagcon --hap-sites and the names of --hap-consensus
"""
import site_reads_twin as srt

MIN_SITES, MIN_READS = 2, 3


def site_counts(ents, counts, hap):
    """counts[k]: the eight counts of site k (what decides the sign).  Four counts a site over the signed entries of
    the labelled alignments."""
    out = [[0, 0, 0, 0] for _ in counts]
    for e, h in zip(ents, hap):
        if not h:
            continue
        for k, code in e:
            m = srt.sign(code, counts[k])
            if m:
                out[k][2 * (h - 1) + (0 if m > 0 else 1)] += 1
    return out


def held(alns, min_len):
    return sum(1 for _, q, _ in alns if len(q) >= min_len)


def tally(tw, K, min_sites=0, min_reads=0, min_cov=0, ok=True):
    """ok False: a failed target, all zeros."""
    sc = [tw["counts"][p] for p in tw["sites"]]
    cnt = site_counts(tw["ents"], sc, tw["hap"])
    n = [sum(1 for h in tw["hap"] if h == g) for g in (1, 2, 0)]
    n_sep = agree = disagree = 0
    for (p1, m1, p2, m2), sigma in zip(cnt, tw["phase"]):
        if not sigma:
            continue
        a, d = ((p1, m2), (m1, p2)) if sigma > 0 else ((m1, p2), (p1, m2))
        agree += sum(a); disagree += sum(d)
        n_sep += a[0] >= 1 and a[1] >= 1
    need = max(1, min_cov)
    split = (ok and n_sep >= (min_sites or MIN_SITES) and min(n[0], n[1]) >= (min_reads or MIN_READS)
             and K - n[1] >= need and K - n[0] >= need)
    if not ok:
        return {"n1": 0, "n2": 0, "n0": 0, "n_sep": 0, "agree": 0, "disagree": 0, "split": 0, "site_counts": []}
    return {"n1": n[0], "n2": n[1], "n0": n[2], "n_sep": n_sep, "agree": agree, "disagree": disagree, "split": int(split),
            "site_counts": cnt}


def groups(alns, min_len, src, hap):
    """src, hap: site_reads_twin.target's (the taken alignments).  An alignment of at least min_len columns that is not
    taken has no label: it is in both groups."""
    label = dict(zip(src, hap))
    out = ([], [])
    for i, (_, q, _) in enumerate(alns):
        if len(q) < min_len:
            continue
        h = label.get(i, 0)
        for g in (1, 2):
            if h in (0, g):
                out[g - 1].append(i)
    return out


def target_line(rname, t):
    return "\t".join(["#target", rname] + [str(t[k]) for k in ("n1", "n2", "n0", "n_sep", "agree", "disagree", "split")])


def site_line(rname, pos0, phase, c):
    return "\t".join([rname, str(pos0 + 1), str(phase)] + [str(x) for x in c])


def fasta_name(rname, label, r0, r1):
    return ">%s/hap%d/%d_%d" % (rname, label, r0, r1)
