"""CPU twin of dagcon_joined_sites (include/dagcon.h has the rule, 10): adjacent sites joined into runs and the tables of
what the spanning alignments show at all of a run's sites, in plain Python with dictionaries on alleles_twin.target.

    run_begins(pos)                                 -> where the runs of one target's ascending site positions begin (10.1)
    jkey(indices)                                   -> the joined key of a spanning member's allele indices (10.3)
    target(tlen, alns, min_len, trim, opts, rounds) -> alleles_twin.target's dict plus "run_begin" (one more for the end),
                                                       "spanning", "partial", "jtables" (per run [(key, count, (c1, c2, c0))])
                                                       and "ent_joined" (per alignment, per entry; NONE: a partial member)
    jtext(key, tables)                              -> (text, opaque) over the run's site tables (10.5)
    joined_alleles_line / vcf_header / vcf_record   -> the text of pbdagcon --joined-alleles / --joined-vcf
"""
import alleles_twin as at

SITES = 16
NONE = 0xFFFF


def run_begins(pos):
    out, first = [], 0
    for k, p in enumerate(pos):
        if k == 0 or p != pos[k - 1] + 1:
            first = k
        if (k - first) % SITES == 0:
            out.append(k)
    return out


def jkey(indices):
    assert len(indices) <= SITES
    return sum(min(a, 15) << (4 * (15 - j)) for j, a in enumerate(indices))


def target(tlen, alns, min_len, trim, opts=(0, 0), rounds=at.srt.ROUNDS):
    tw = at.target(tlen, alns, min_len, trim, opts, rounds)
    rb = run_begins(tw["sites"]) + [len(tw["sites"])]
    run_of = {k: r for r in range(len(rb) - 1) for k in range(rb[r], rb[r + 1])}
    members = [{} for _ in rb[:-1]]                                     # per run: alignment -> {site: allele index}
    for x, (e, ia) in enumerate(zip(tw["ents"], tw["ent_allele"])):
        for (k, _), a in zip(e, ia):
            members[run_of[k]].setdefault(x, {})[k] = a
    spanning, partial, jtables, index = [], [], [], []
    for r, mem in enumerate(members):
        sites = range(rb[r], rb[r + 1])
        keys = {x: jkey([has[k] for k in sites]) for x, has in mem.items() if len(has) == len(sites)}
        tb = at.table(keys.values())
        hc = {kk: [0, 0, 0] for kk, _ in tb}
        for x, kk in keys.items():
            hc[kk][(tw["hap"][x] - 1) % 3] += 1                         # hap 1, 2, 0 -> c1, c2, c0
        where = {kk: i for i, (kk, _) in enumerate(tb)}
        spanning.append(len(keys)); partial.append(len(mem) - len(keys))
        jtables.append([(kk, c, tuple(hc[kk])) for kk, c in tb])
        index.append({x: where[kk] for x, kk in keys.items()})
    tw["run_begin"], tw["spanning"], tw["partial"], tw["jtables"] = rb, spanning, partial, jtables
    tw["ent_joined"] = [[index[run_of[k]].get(x, NONE) for k, _ in e] for x, e in enumerate(tw["ents"])]
    return tw


def jtext(key, tables):
    """tables: the tables of the run's sites, in their order."""
    s = ""
    for j, tab in enumerate(tables):
        c = (key >> (4 * (15 - j))) & 15
        if c == 15 or tab[c][0] & at.LONG:
            return "*", True
        s += at.text(tab[c][0]).replace("-", "")
    return s or "-", False


def joined_alleles_line(rname, pos0, m, ref, span, part, text, count, hap=None):
    """ref: the run's target bytes or None for '.'; hap: (c1, c2, c0) or None for '.'."""
    h = [str(int(x)) for x in hap] if hap is not None else [".", ".", "."]
    return "\t".join([rname, str(pos0 + 1), str(pos0 + m), ref.decode() if ref is not None else ".", str(int(span)), str(int(part)), text, str(int(count))] + h)


def vcf_header(contigs, split):
    """contigs: [(name, length)]."""
    out = ["##fileformat=VCFv4.2", "##source=pbdagcon --joined-vcf (this build's own rule, parity unpinned)"]
    out += ["##contig=<ID=%s,length=%d>" % c for c in contigs]
    out += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Alignments with a column at every target base of the record\'s run of adjacent sites">',
            '##INFO=<ID=PART,Number=1,Type=Integer,Description="Alignments with a column at some but not all of them: not counted in AD">',
            '##INFO=<ID=AD,Number=R,Type=Integer,Description="Alignments of DP that show the REF bases and each ALT between the run\'s first target base and the one behind its last">']
    if split:
        out += ['##INFO=<ID=AD1,Number=R,Type=Integer,Description="AD among the alignments of read group 1">',
                '##INFO=<ID=AD2,Number=R,Type=Integer,Description="AD among the alignments of read group 2">']
    out += ["##pbdagcon_note=adjacent sites are joined into runs of at most 16: a longer stretch is several records",
            "##pbdagcon_note=shared leading and trailing bases of REF and ALT are not trimmed",
            "##pbdagcon_note=no genotype is called",
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    return out


def vcf_record(rname, tb, pos0, m, span, part, tab, min_count, split):
    """tb: the target's bases; tab: the run's table as [(text, opaque, count, (c1, c2, c0))].  None: the run has no record."""
    if m == len(tb):
        return None
    cls = "".join(chr(b & 0xDF) if b & 0xDF in at.CODE else "N" for b in tb[pos0:pos0 + m])
    ref_ad, alts = [0, 0, 0], {}
    for text, opaque, c, h in tab:
        if opaque:
            continue
        bases = "" if text == "-" else text
        if bases == cls:
            ref_ad = [ref_ad[0] + c, ref_ad[1] + h[0], ref_ad[2] + h[1]]
        elif c >= min_count:
            ad = alts.setdefault(bases, [0, 0, 0])                      # (a dict keeps the order of first appearance)
            ad[0] += c; ad[1] += h[0]; ad[2] += h[1]
    if not alts:
        return None
    ref, texts, pos = tb[pos0:pos0 + m].decode(), list(alts), pos0 + 1
    if "" in alts:
        if pos0 > 0:
            a = chr(tb[pos0 - 1])
            ref, texts, pos = a + ref, [a + x for x in texts], pos0
        else:
            a = chr(tb[pos0 + m])
            ref, texts = ref + a, [x + a for x in texts]
    info = "DP=%d;PART=%d" % (span, part)
    for j, name in enumerate(("AD", "AD1", "AD2")[:3 if split else 1]):
        info += ";%s=%s" % (name, ",".join(str(x[j]) for x in [ref_ad] + list(alts.values())))
    return "\t".join([rname, str(pos), ".", ref, ",".join(texts), ".", ".", info])
