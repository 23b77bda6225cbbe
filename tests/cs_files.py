"""The suite's own writer of PAF lines with cs:Z: tags, for the tests of `pbdagcon --paf --cs` (no minimap2 is behind
it).  Pure Python over cigar_twin, cs_twin and paf_files: imports neither the product nor the oracle.

An alignment is paf_files' dict plus cs (the text behind cs:Z:, bytes; None / False: the line carries no cs tag); cg
stays optional, so a line carries either tag, both or neither.

    with_cs(reads, alns, tseqs, long_form=False)   the alignments with their cs text (from the read in the target's
                                                   orientation: a '-' line needs nothing more)
    paf_text(reads, alns)                          LF text, the cs tag between other tags
    decoded(names, tseqs, alns)                    per target [(pos, read, ops)] as cs_twin.decode gives them, with the
                                                   flat flags and qnames cigar_twin.to_sam takes
    prefix(n)                                      cs text of exactly n bytes (n >= 2) that consumes prefix_bases(n)
                                                   read and target bases
"""
import cigar_twin as ct
import cs_twin as cst
import paf_files as pf


def with_cs(reads, alns, tseqs, long_form=False):
    out = []
    for x in alns:
        seq, c0, c1 = pf.oriented(reads, x)
        q = seq[c0:len(seq) - c1]
        out.append(dict(x, cs=cst.encode(x["ts"] + 1, q, tseqs[x["tname"]], x["ops"], long_form)))
    return out


def paf_line(x):
    f = pf.paf_line(x).split("\t")
    if x.get("cs") not in (None, False):
        f.insert(len(f) - 1, "cs:Z:" + bytes(x["cs"]).decode())
    return "\t".join(f)


def paf_text(reads, alns):
    return ("".join(paf_line(dict(x, qlen=x.get("qlen", len(reads.get(x["qname"], b""))))) + "\n" for x in alns)).encode()


def decoded(names, tseqs, alns):
    per, flags, qnames = [[] for _ in names], [], []
    for g, name in enumerate(names):
        for x in alns:
            if x["tname"] != name:
                continue
            ops, q, fl = cst.decode(x["cs"], tseqs[name], x["ts"] + 1)
            assert fl == 0
            per[g].append((x["ts"] + 1, q, ops))
            flags.append(16 if x["strand"] == "-" else 0)
            qnames.append(x["qname"])
    return per, flags, qnames


def prefix(n):
    """n bytes of :1 tokens, one of them *ac when n is odd."""
    assert n >= 2
    return b":1" * ((n - 3) // 2) + b"*ac" if n % 2 else b":1" * (n // 2)


def prefix_bases(n):
    return (n - 3) // 2 + 1 if n % 2 else n // 2
