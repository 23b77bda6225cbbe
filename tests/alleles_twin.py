"""CPU twin of dagcon_site_alleles (include/dagcon.h has the rule, 8): the alleles themselves at the sites of the pile-up, in
plain Python on evidence_twin.columns / coords, pileup_twin and site_reads_twin.entries.

    allele(q, t, i)                                -> the mapped bytes of the allele of the entry at column i of the trimmed columns
    key(a) / text(k)                               -> the 64-bit key of an allele; its text form
    table(keys)                                    -> [(key, count)] by count descending, ties by key ascending
    target(tlen, alns, min_len, trim, opts, rounds) -> site_reads_twin.target's dict plus "keys" (per alignment, per entry),
                                                      "tables" (per site [(key, count, (c1, c2, c0))]) and "ent_allele"
    site_alleles_line / vcf_header / vcf_record    -> the text of pbdagcon --site-alleles / --site-vcf
"""
from collections import Counter

import evidence_twin as ev
import pileup_twin as pt
import site_reads_twin as srt

GAP = ev.GAP
BASES = 20
LONG = 1 << 60
CODE = {ord("A"): 1, ord("C"): 2, ord("G"): 3, ord("T"): 4}
LETTERS = "?ACGTN"


def allele(q, t, i):
    """q, t: the alignment's trimmed columns; i: a column with a target base."""
    assert t[i] != GAP
    out = [] if q[i] == GAP else [q[i]]
    j = i + 1
    while j < len(t) and t[j] == GAP and q[j] != GAP:
        out.append(q[j])
        j += 1
    return bytes(b & 0xDF if b & 0xDF in CODE else ord("N") for b in out)


def key(a):
    k = 0
    for j, b in enumerate(a[:BASES]):
        k |= CODE.get(b, 5) << (3 * (BASES - 1 - j))
    return k | (LONG if len(a) > BASES else 0)


def text(k):
    s = ""
    for j in range(BASES):
        c = (k >> (3 * (BASES - 1 - j))) & 7
        if not c:
            break
        s += LETTERS[c]
    return (s or "-") + ("+" if k & LONG else "")


def table(keys):
    return sorted(Counter(keys).items(), key=lambda kc: (-kc[1], kc[0]))


def entry_keys(alns, min_len, trim, sites):
    """Per taken alignment the keys of its entries, parallel to site_reads_twin.entries."""
    idx = set(sites)
    out = []
    for _, s0, q, t in srt.taken(alns, min_len, trim):
        tcs, _ = ev.coords(s0, t)
        out.append([key(allele(q, t, i)) for i in range(len(t)) if t[i] != GAP and tcs[i] in idx])
    return out


def target(tlen, alns, min_len, trim, opts=(0, 0), rounds=srt.ROUNDS):
    tw = srt.target(tlen, alns, min_len, trim, opts, rounds)
    keys = entry_keys(alns, min_len, trim, tw["sites"])
    per_site = [[] for _ in tw["sites"]]
    for x, (e, ks) in enumerate(zip(tw["ents"], keys)):
        assert len(e) == len(ks)
        for (k, _), kk in zip(e, ks):
            per_site[k].append((kk, tw["hap"][x]))
    tables, where = [], []
    for ent in per_site:
        tb = table([kk for kk, _ in ent])
        hc = {kk: [0, 0, 0] for kk, _ in tb}
        for kk, h in ent:
            hc[kk][(h - 1) % 3] += 1                                   # hap 1, 2, 0 -> c1, c2, c0
        tables.append([(kk, c, tuple(hc[kk])) for kk, c in tb])
        where.append({kk: i for i, (kk, _) in enumerate(tb)})
    tw["keys"] = keys
    tw["tables"] = tables
    tw["ent_allele"] = [[where[k][kk] for (k, _), kk in zip(e, ks)] for e, ks in zip(tw["ents"], keys)]
    return tw


def site_alleles_line(rname, pos0, ref, n, k, count, hap=None):
    """ref: the target's byte (an int) or None for '.'; n: the site's eight counts; hap: (c1, c2, c0) or None for '.'."""
    h = [str(int(x)) for x in hap] if hap is not None else [".", ".", "."]
    return "\t".join([rname, str(pos0 + 1), chr(ref) if ref is not None else ".", str(pt.depth(n)), text(k), str(int(count))] + h)


def vcf_header(contigs, split):
    """contigs: [(name, length)]."""
    out = ["##fileformat=VCFv4.2", "##source=pbdagcon --site-vcf (this build's own rule, parity unpinned)"]
    out += ["##contig=<ID=%s,length=%d>" % c for c in contigs]
    out += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Alignments with a column at the site\'s target base">',
            '##INFO=<ID=AD,Number=R,Type=Integer,Description="Alignments that show the REF allele and each ALT allele between this target base and the next">']
    if split:
        out += ['##INFO=<ID=AD1,Number=R,Type=Integer,Description="AD among the alignments of read group 1">',
                '##INFO=<ID=AD2,Number=R,Type=Integer,Description="AD among the alignments of read group 2">']
    out += ["##pbdagcon_note=adjacent sites are not joined: a deletion of three bases is three records",
            "##pbdagcon_note=no genotype is called",
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    return out


def vcf_record(rname, tb, pos0, n, tab, min_count, split):
    """tb: the target's bases; tab: the site's table [(key, count, (c1, c2, c0))].  None: the site has no record."""
    if len(tb) < 2:
        return None
    r = tb[pos0]
    ref_key = key(bytes([r & 0xDF if r & 0xDF in CODE else ord("N")]))
    alts = [(k, c, h) for k, c, h in tab if not k & LONG and k != ref_key and c >= min_count]
    if not alts:
        return None
    refs = [(c, h) for k, c, h in tab if k == ref_key] or [(0, (0, 0, 0))]
    texts = ["" if k == 0 else text(k) for k, _, _ in alts]
    ref, pos = chr(r), pos0 + 1
    if any(k == 0 for k, _, _ in alts):
        if pos0 > 0:
            a = chr(tb[pos0 - 1])
            ref, texts, pos = a + ref, [a + x for x in texts], pos0
        else:
            a = chr(tb[1])
            ref, texts = ref + a, [x + a for x in texts]
    info = "DP=%d;AD=%s" % (pt.depth(n), ",".join(str(c) for c in [refs[0][0]] + [c for _, c, _ in alts]))
    if split:
        for j in (0, 1):
            info += ";AD%d=%s" % (j + 1, ",".join(str(h[j]) for h in [refs[0][1]] + [h for _, _, h in alts]))
    return "\t".join([rname, str(pos), ".", ref, ",".join(texts), ".", ".", info])
