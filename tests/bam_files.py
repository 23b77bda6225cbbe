"""A BAM writer for the tests of `pbdagcon --bam`, written from the SAM/BAM specification (SAMv1 sections 4.1, 4.2):
records to BAM bytes to BGZF members.  `struct` plus the standard library's zlib for raw DEFLATE and CRC32; imports
neither the product nor the oracle.  No htslib, samtools or pysam stands behind it: the reader it tests is pinned to
this writer and to the specification, nothing else.

A record is a dict: qname (str), flag (int), ref (index into refs, -1 for '*'), pos (1-based, 0 for none), ops (list of
len << 4 | code, [] for '*'), seq (bytes over =ACMGRSVTWYHKDBN, b"" for '*'), and optionally tags (raw bytes in front
of a CG tag, if one is written).

    pack_nibbles(seq) / unpack_nibbles(data, n)    the library-independent twin of the 4-bit table
    bam_bytes(refs, records, cg=True)              the uncompressed BAM stream
    bgzf(data, level, strategy, payload, eof)      BGZF members
    member_block_types(bgzf bytes)                 BTYPE of the first DEFLATE block of every member
    sam_text(refs, records)                        the SAM text of the same records
"""
import struct
import zlib

NT16 = b"=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
_CODE = {c: i for i, c in enumerate(NT16)}
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def pack_nibbles(seq):
    """Two bases a byte, the first in the high nibble; an odd last base leaves the low nibble 0."""
    seq = bytes(seq)
    out = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        if c not in _CODE:
            raise ValueError("base %r is not one of %s" % (bytes([c]), NT16.decode()))
        out[i >> 1] |= _CODE[c] << (4 if i % 2 == 0 else 0)
    return bytes(out)


def unpack_nibbles(data, n):
    data = bytes(data)
    return bytes(NT16[(data[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(n))


def ref_span(ops):
    return sum(o >> 4 for o in ops if (o & 15) in (0, 2, 3, 7, 8))


def reg2bin(beg, end):
    """SAMv1 5.3 (the reader does not use it; a writer fills it in)."""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def record_bytes(rec, cg=True):
    ops, seq = list(rec["ops"]), bytes(rec["seq"])
    name = rec["qname"].encode() + b"\0"
    pos0 = rec["pos"] - 1
    tags = bytes(rec.get("tags", b""))
    span = ref_span(ops)
    if len(ops) > 65535:
        # the real ops go into CG:B,I; the record carries <l_seq>S<ref_len>N
        if cg:
            tags += b"CGBI" + struct.pack("<i", len(ops)) + struct.pack("<%dI" % len(ops), *ops)
        ops = [(len(seq) << 4) | 4, (span << 4) | 3]
    body = struct.pack("<iiBBHHHiiii", rec["ref"], pos0, len(name), rec.get("mapq", 60),
                       reg2bin(max(pos0, 0), max(pos0, 0) + max(span, 1)), len(ops), rec["flag"], len(seq), -1, -1, 0)
    body += name + struct.pack("<%dI" % len(ops), *ops) + pack_nibbles(seq) + b"\xff" * len(seq) + tags
    return struct.pack("<i", len(body)) + body


def bam_bytes(refs, records, cg=True, text=None):
    """refs = [(name, length)]."""
    if text is None:
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    t = text.encode()
    out = [b"BAM\1", struct.pack("<i", len(t)), t, struct.pack("<i", len(refs))]
    for name, ln in refs:
        n = name.encode() + b"\0"
        out += [struct.pack("<i", len(n)), n, struct.pack("<i", ln)]
    out += [record_bytes(r, cg) for r in records]
    return b"".join(out)


def member(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    data = c.compress(payload) + c.flush()
    bsize = 18 + len(data) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1) + data +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def bgzf(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, payload=0xFF00, eof=True):
    """`payload` uncompressed bytes a member (at most 0xFF00, so that a stored member still fits 64 KiB)."""
    assert 1 <= payload <= 0xFF00
    out = [member(data[i:i + payload], level, strategy) for i in range(0, len(data), payload)]
    if eof:
        out.append(EOF_MEMBER)
    return b"".join(out)


def members(blob):
    """[(offset, size)] of the members, by BSIZE."""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 12:p + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        out.append((p, size))
        p += size
    return out


def member_block_types(blob):
    """BTYPE (0 stored, 1 fixed, 2 dynamic) of the first DEFLATE block of every member: bits 1..2 of its payload."""
    return [(blob[p + 18] >> 1) & 3 for p, _ in members(blob)]


def cigar_string(ops):
    return "".join("%d%s" % (o >> 4, OPS[o & 15]) for o in ops) or "*"


def sam_text(refs, records, header=True):
    lines = []
    if header:
        lines.append("@HD\tVN:1.6\tSO:coordinate")
        lines += ["@SQ\tSN:%s\tLN:%d" % r for r in refs]
    for r in records:
        lines.append("\t".join([r["qname"], str(r["flag"]), refs[r["ref"]][0] if r["ref"] >= 0 else "*", str(r["pos"]),
                                str(r.get("mapq", 60)), cigar_string(r["ops"]), "*", "0", "0",
                                bytes(r["seq"]).decode() or "*", "*"]))
    return ("\n".join(lines) + "\n").encode()
