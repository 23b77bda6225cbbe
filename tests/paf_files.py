"""A PAF writer for the tests of `pbdagcon --paf`, with the twin of the stranded expansion (include/dagcon.h,
dagcon_upload_cigar_strand).  Pure Python over cigar_twin: imports neither the product nor the oracle.

An alignment is a dict: qname, strand ('+' / '-'), qs, qe (the slice of the read AS THE READS FILE HAS IT), tname, tlen,
ts, te, ops (BAM-encoded, written against the slice for '+', against its reverse complement for '-'), and optionally
tp ('P' / 'S') and cg (False: the line carries no cg:Z: tag).  reads = {qname: bases as the reads file has them}.

    comp(byte), revcomp(bytes)                   the complement of the header: ACGT and acgt, anything else as it is
    strand_base(q, i, reverse)                   read base i of the expansion rule
    expand_strand(pos, q, t, ops, reverse)       cigar_twin.expand over strand_base
    from_twin(rng, targets, ...)                 twin targets -> (reads, alignments)
    paf_text(alns), reads_fasta(reads), reads_fastq(reads)
    sam_text(names, tlens, reads, alns)          the same alignments as SAM, through cigar_twin.to_sam
"""
import cigar_twin as ct

_PAIRS = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C"),
          ord("a"): ord("t"), ord("t"): ord("a"), ord("c"): ord("g"), ord("g"): ord("c")}
_TABLE = bytes(_PAIRS.get(b, b) for b in range(256))


def comp(b):
    return _PAIRS.get(b, b)


def revcomp(s):
    return bytes(s)[::-1].translate(_TABLE)


def strand_base(q, i, reverse):
    """Read base i of a record whose bases q lie as the reads file has them."""
    return comp(q[len(q) - 1 - i]) if reverse else q[i]


def expand_strand(pos, q, t, ops, reverse):
    return ct.expand(pos, bytes(strand_base(q, i, reverse) for i in range(len(q))), t, ops)


def tspan(ops):
    return sum(int(o) >> 4 for o in ops if (int(o) & 15) in (ct.M, ct.D, ct.EQ, ct.X))


def qspan(ops):
    return sum(int(o) >> 4 for o in ops if (int(o) & 15) in (ct.M, ct.I, ct.S, ct.EQ, ct.X))


def from_twin(rng, names, targets, alphabet=b"ACGTacgtN", max_flank=25, reverse_p=0.5, shared=2, sort_pos=False):
    """targets = [(target bases, [(pos, read bases in the target's orientation, ops)])] -> (reads, alns).  Every record
    becomes a slice inside a longer read (flanks of 0..max_flank bytes of `alphabet`, so qs > 0 and qe < qlen occur
    beside 0 and qlen), on either strand.  `shared` reads of target 0 get a second alignment, to target 1, of another
    slice on the other strand (xM: a read aligned to two targets).  sort_pos: a target's alignments ascending in ts."""
    reads, alns = {}, []
    for g, (tseq, recs) in enumerate(targets):
        for k, (pos, q, ops) in enumerate(recs):
            a, z = (int(x) for x in rng.integers(0, max_flank + 1, 2))
            junk = bytes(alphabet[i] for i in rng.integers(0, len(alphabet), a + z))
            full = junk[:a] + bytes(q) + junk[a:]                        # in the target's orientation
            rev = bool(rng.random() < reverse_p)
            qname = "read%d_%d" % (g, k)
            reads[qname] = revcomp(full) if rev else full
            qs = z if rev else a
            alns.append(dict(qname=qname, strand="-" if rev else "+", qs=qs, qe=qs + len(q), tname=names[g],
                             tlen=len(tseq), ts=pos - 1, te=pos - 1 + tspan(ops), ops=[int(o) for o in ops]))
    if len(targets) > 1:
        first = [x for x in alns if x["tname"] == names[0]][:shared]
        tl = len(targets[1][0])
        for j, x in enumerate(first):
            r = reads[x["qname"]]
            n = max(1, min(len(r) - 1, tl - 1) // 2)
            qs = min(1 + j, len(r) - n)
            ts = min(3 + 5 * j, tl - n)
            alns.append(dict(qname=x["qname"], strand="+" if x["strand"] == "-" else "-", qs=qs, qe=qs + n,
                             tname=names[1], tlen=tl, ts=ts, te=ts + n, ops=[ct.op("M", n)]))
    if sort_pos:
        alns.sort(key=lambda x: (names.index(x["tname"]), x["ts"]))
    return reads, alns


def paf_line(x):
    n = x["te"] - x["ts"]
    f = [x["qname"], str(x.get("qlen", 0)), str(x["qs"]), str(x["qe"]), x["strand"], x["tname"], str(x["tlen"]),
         str(x["ts"]), str(x["te"]), str(n), str(max(n, x["qe"] - x["qs"])), "60", "NM:i:0", "tp:A:" + x.get("tp", "P")]
    if x.get("cg", True):
        f.append("cg:Z:" + ct.cigar_string(x["ops"]))
    f.append("rl:i:0")
    return "\t".join(f)


def paf_text(reads, alns):
    """LF text, one line per alignment in the order given; qlen from the reads unless an alignment carries its own."""
    return ("".join(paf_line(dict(x, qlen=x.get("qlen", len(reads.get(x["qname"], b""))))) + "\n" for x in alns)).encode()


def reads_fasta(reads, width=60):
    return ct.to_fasta([n + " a description" for n in reads], list(reads.values()), width)


def reads_fastq(reads):
    return b"".join(b"@" + n.encode() + b" a description\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in reads.items())


def oriented(reads, x):
    """(read in the target's orientation, soft clip in front, soft clip behind) of an alignment."""
    r = reads[x["qname"]]
    if x["strand"] == "-":
        return revcomp(r), len(r) - x["qe"], x["qs"]
    return r, x["qs"], len(r) - x["qe"]


def sam_records(names, reads, alns):
    """Per target (in the order of names) [(pos, SEQ, ops)], with the flat flags and qnames cigar_twin.to_sam takes: SEQ is
    the whole read in the target's orientation, the slice's flanks are soft clips, '-' is FLAG 16."""
    per, flags, qnames = [[] for _ in names], [], []
    for g, name in enumerate(names):
        for x in alns:
            if x["tname"] != name:
                continue
            seq, c0, c1 = oriented(reads, x)
            ops = ([ct.op("S", c0)] if c0 else []) + list(x["ops"]) + ([ct.op("S", c1)] if c1 else [])
            per[g].append((x["ts"] + 1, seq, ops))
            flags.append(16 if x["strand"] == "-" else 0)
            qnames.append(x["qname"])
    return per, flags, qnames


def sam_text(names, tlens, reads, alns):
    per, flags, qnames = sam_records(names, reads, alns)
    return ct.to_sam(names, tlens, per, flags=flags, qnames=qnames)
