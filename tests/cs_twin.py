"""CPU twin of the cs input (include/dagcon.h, dagcon_cs_batch): the decode rule of minimap2's cs:Z: text, its
inverse, and the judgement of a record.  Pure Python over cigar_twin: imports neither the product nor the oracle.

    tokens(cs)                                   [(op byte, body bytes)], or None when the first byte starts no op
    decode(cs, t, pos) -> (ops, q, flags)        the normative rule; flags: BAD_OP | BAD_BODY, then ops and q are empty
    why(cs, t, pos, q_len, t_span=None)          None for a conforming record, else which rule it breaks
    encode(pos, q, t, ops, long_form=False)      a record of cigar_twin as cs text, bodies lower-cased as minimap2 does

The reference reads no PAF; the rule is this build's own.  The cs text is in the target's orientation, so a record is
(pos, q_len, t_span, text) whatever the strand of its PAF line.
"""
import cigar_twin as ct

BAD_OP = 8          # a ~ op, or a first byte that starts no op
BAD_BODY = 16       # an empty body, a non-letter, a non-digit, :0, more than 9 digits, 2^28 or more, a * body not of two letters
OP_BYTES = b":*+-=~"


def _letters(b):
    return len(b) > 0 and all(65 <= (x & 0xDF) <= 90 for x in b)


def _upper(b):
    return bytes(x - 32 if 97 <= x <= 122 else x for x in b)


def tokens(cs):
    cs = bytes(cs)
    if not cs:
        return []
    if cs[0] not in OP_BYTES:
        return None
    out = []
    for i, x in enumerate(cs):
        if x in OP_BYTES:
            out.append([x, bytearray()])
        else:
            out[-1][1].append(x)
    return [(o, bytes(b)) for o, b in out]


def decode(cs, t, pos):
    """(BAM-encoded ops, read bases, flags).  A :n past the target's end gives as many bases as the target has: such
    a record is non-conforming by its totals (why), as is pos == 0."""
    toks = tokens(cs)
    if toks is None:
        return [], b"", BAD_OP
    flags = 0
    ops, q = [], bytearray()
    ti = pos - 1
    for o, body in toks:
        o = bytes([o])
        if o == b"~":
            flags |= BAD_OP
        elif o == b":":
            if not (1 <= len(body) <= 9 and body.isdigit() and 1 <= int(body) < (1 << 28)):
                flags |= BAD_BODY
                continue
            n = int(body)
            ops.append(ct.op("=", n))
            q += t[max(ti, 0):max(ti + n, 0)]
            ti += n
        elif o == b"*":
            if not (len(body) == 2 and _letters(body)):
                flags |= BAD_BODY
                continue
            ops.append(ct.op("X", 1))
            q += _upper(body[1:])
            ti += 1
        else:
            if not _letters(body):
                flags |= BAD_BODY
                continue
            ops.append(ct.op({b"=": "=", b"+": "I", b"-": "D"}[o], len(body)))
            if o != b"-":
                q += _upper(body)
            if o != b"+":
                ti += len(body)
    if flags:
        return [], b"", flags
    return ops, bytes(q), 0


def totals(ops):
    """(columns, read bases, target bases) of decoded ops."""
    ln = lambda codes: sum(int(o) >> 4 for o in ops if (int(o) & 15) in codes)
    return ln((ct.EQ, ct.X, ct.I, ct.D)), ln((ct.EQ, ct.X, ct.I)), ln((ct.EQ, ct.X, ct.D))


def why(cs, t, pos, q_len, t_span=None):
    ops, _, flags = decode(cs, t, max(pos, 1))
    if flags & BAD_OP:
        return "bad op"
    if flags & BAD_BODY:
        return "bad body"
    nc, nq, nt = totals(ops)
    if max(nc, nq, nt) >= 1 << 32:
        return "overflow"
    if pos == 0:
        return "pos is 0"
    if nq != q_len:
        return "q_len"
    if t_span is not None and nt != t_span:
        return "t_span"
    if pos - 1 + nt > len(t):
        return "past tlen"
    return None


def encode(pos, q, t, ops, long_form=False):
    """cs text of a conforming record without clips: :n (long form: =seq) only where read and target bytes are equal,
    *tq otherwise, +seq, -seq; bodies lower-cased.  Runs of equal bytes are merged across ops, as minimap2 writes them."""
    q, t = bytes(q), bytes(t)
    out = []
    run = bytearray()

    def flush():
        if run:
            out.append(b"=" + bytes(run).lower() if long_form else b":%d" % len(run))
            run.clear()
    qi, ti = 0, pos - 1
    for o in ops:
        code, n = int(o) & 15, int(o) >> 4
        if code in (ct.M, ct.EQ, ct.X):
            for k in range(n):
                if q[qi + k] == t[ti + k]:
                    run.append(q[qi + k])
                else:
                    flush()
                    out.append(b"*" + bytes([t[ti + k], q[qi + k]]).lower())
            qi += n; ti += n
        elif code == ct.I:
            flush()
            out.append(b"+" + q[qi:qi + n].lower())
            qi += n
        elif code == ct.D:
            flush()
            out.append(b"-" + t[ti:ti + n].lower())
            ti += n
        else:
            raise ValueError("cs has no op for CIGAR %s" % ct.OPS[code])
    flush()
    assert qi == len(q)
    return b"".join(out)
