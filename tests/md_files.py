"""SAM and BAM files whose records carry an MD:Z tag, for the tests of `pbdagcon --sam --md` and `--bam --md`: SAM text
with the tag among other optional fields, BAM through bam_files' `tags` hook.  Imports neither the product nor the
oracle; no samtools stands behind it.

    records(names, targets, texts) -> [record dict]   targets = [(target bases, [(pos, read, ops)])], texts = [[MD text
                                                      or None: the record gets no tag]]
    sam_text(names, tlens, recs) / bam_file(names, tlens, recs)
"""
import bam_files as bf


def records(names, targets, texts, flags=None):
    out, i = [], 0
    for g, ((_, recs), per) in enumerate(zip(targets, texts)):
        for k, ((pos, q, ops), text) in enumerate(zip(recs, per)):
            out.append({"qname": "q%d_%d" % (g, k), "flag": 0 if flags is None else flags[i], "ref": g, "pos": pos,
                        "ops": [int(o) for o in ops], "seq": bytes(q), "md": None if text is None else bytes(text)})
            i += 1
    return out


def sam_text(names, tlens, recs, header=True):
    """QUAL is '*'; the MD:Z field stands between two other optional fields (an NM:i in front, an XS:Z that merely holds
    the letters MD:Z: behind it)."""
    lines = []
    if header:
        lines.append("@HD\tVN:1.6\tSO:coordinate")
        lines += ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in zip(names, tlens)]
        lines.append("@PG\tID:twin\tPN:md_files")
    for r in recs:
        f = [r["qname"], str(r["flag"]), names[r["ref"]] if r["ref"] >= 0 else "*", str(r["pos"]), "60",
             bf.cigar_string(r["ops"]), "*", "0", "0", r["seq"].decode() or "*", "*", "NM:i:0"]
        if r["md"] is not None:
            f.append("MD:Z:" + r["md"].decode())
        f.append("XS:Z:xMD:Z:9")
        lines.append("\t".join(f))
    return ("\n".join(lines) + "\n").encode()


def bam_file(names, tlens, recs, **kw):
    """The same records as BGZF-compressed BAM: NM:C in front of the MD:Z field, an XS:Z behind it."""
    out = []
    for r in recs:
        tags = b"NMC\x00" + (b"MDZ" + r["md"] + b"\0" if r["md"] is not None else b"") + b"XSZMD\0"
        out.append(dict(r, tags=tags))
    return bf.bgzf(bf.bam_bytes(list(zip(names, tlens)), out), **kw)
