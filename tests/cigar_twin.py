"""CPU twin of the CIGAR input (include/dagcon.h, dagcon_cigar_batch): the expansion rule, its inverse, and SAM /
FASTA text.  Pure numpy / Python: imports neither the product nor the oracle.

Ops are BAM-encoded integers, len << 4 | code, code 0..8 = M I D N S H P = X.

    expand(pos, q, t, ops)  -> (aln_start, qstr, tstr)      the normative rule
    compress(start, qstr, tstr, backbone, eqx=False) -> (pos, q, ops)
    compress_batch(batch, eqx=False) -> dict of the arrays of a dagcon_cigar_batch
    to_sam(...), to_fasta(...)
"""
import numpy as np

OPS = "MIDNSHP=X"
M, I, D, N, S, H, P, EQ, X = range(9)
_COL = (M, I, D, EQ, X)
_QRY = (M, I, S, EQ, X)
_TGT = (M, D, EQ, X)
GAP = 0x2D


def op(code, length):
    return (int(length) << 4) | (OPS.index(code) if isinstance(code, str) else int(code))


def cigar_string(ops):
    return "".join("%d%s" % (int(o) >> 4, OPS[int(o) & 15]) for o in ops) or "*"


def parse_cigar(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(op(ch, int(n)))
            n = ""
    assert n == ""
    return out


def conforming(pos, q_len, tlen, ops):
    """The record conforms to include/dagcon.h (what the device is expected to accept)."""
    ops = np.asarray(ops, dtype=np.int64)
    code, ln = ops & 15, ops >> 4
    if (code > 8).any() or (code == N).any() or (ln == 0).any() or pos == 0:
        return False
    nq = int(ln[np.isin(code, _QRY)].sum())
    nt = int(ln[np.isin(code, _TGT)].sum())
    return nq == q_len and pos - 1 + nt <= tlen


def expand(pos, q, t, ops):
    """(aln_start, qstr, tstr) of one conforming record: q its read bases, t its target's bases."""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1)
    assert conforming(pos, len(q), len(t), ops)
    code, ln = ops & 15, ops >> 4
    qa, ta = np.frombuffer(bytes(q), np.uint8), np.frombuffer(bytes(t), np.uint8)
    dq = np.where(np.isin(code, _QRY), ln, 0)
    dt = np.where(np.isin(code, _TGT), ln, 0)
    q0 = np.cumsum(dq) - dq                       # first read base of each op
    t0 = np.cumsum(dt) - dt + (pos - 1)
    col = np.isin(code, _COL)
    code, ln, q0, t0 = code[col], ln[col], q0[col], t0[col]
    ncol = int(ln.sum())
    c0 = np.cumsum(ln) - ln
    k = np.arange(ncol, dtype=np.int64) - np.repeat(c0, ln)      # offset inside the op
    cc = np.repeat(code, ln)
    qi, ti = np.repeat(q0, ln) + k, np.repeat(t0, ln) + k
    qs = np.full(ncol, GAP, np.uint8)
    ts = np.full(ncol, GAP, np.uint8)
    hq, ht = cc != D, cc != I
    qs[hq] = qa[qi[hq]]
    ts[ht] = ta[ti[ht]]
    return pos, qs.tobytes(), ts.tobytes()


def compress(start, qstr, tstr, backbone, eqx=False):
    """Gapped strings ('-' gaps only) back to (pos, read bases, ops); consecutive equal ops merged.  The target bases
    are the backbone's: the strings' target side must agree with it.  eqx: '=' / 'X' instead of 'M'."""
    qa, ta = np.frombuffer(bytes(qstr), np.uint8), np.frombuffer(bytes(tstr), np.uint8)
    assert qa.size == ta.size
    qg, tg = qa == GAP, ta == GAP
    assert not (qg & tg).any(), "a column of two gaps has no CIGAR op"
    tb = ta[~tg]
    assert start >= 1 and start - 1 + tb.size <= len(backbone)
    assert tb.tobytes() == bytes(backbone[start - 1:start - 1 + tb.size]), "target side differs from the backbone"
    code = np.where(tg, I, np.where(qg, D, np.where(qa == ta, EQ, X) if eqx else M)).astype(np.int64)
    if code.size == 0:
        return start, b"", []
    cut = np.flatnonzero(np.diff(code)) + 1
    first = np.concatenate([[0], cut])
    ln = np.diff(np.concatenate([first, [code.size]]))
    return start, qa[~qg].tobytes(), ((ln << 4) | code[first]).tolist()


def compress_batch(batch, eqx=False):
    """A HostBatch-like object (tlen, aln_begin, aln_start, aln_off, aln_len, qstr, tstr, backbone, backbone_off) as
    the arrays of a dagcon_cigar_batch (a dict; keys are the struct's fields, n_targets left out)."""
    T = int(batch.tlen.size)
    pos, q_off, q_len, op_begin, ops, qs = [], [], [], [0], [], []
    qp = 0
    for t in range(T):
        o = int(batch.backbone_off[t])
        bb = batch.backbone[o:o + int(batch.tlen[t])].tobytes()
        for a in range(int(batch.aln_begin[t]), int(batch.aln_begin[t + 1])):
            f, n = int(batch.aln_off[a]), int(batch.aln_len[a])
            p, q, oo = compress(int(batch.aln_start[a]), batch.qstr[f:f + n], batch.tstr[f:f + n], bb, eqx)
            pos.append(p); q_off.append(qp); q_len.append(len(q)); qs.append(q); qp += len(q)
            ops.append(np.asarray(oo, np.uint32))
            op_begin.append(op_begin[-1] + len(oo))
    return dict(tlen=np.asarray(batch.tlen, np.uint32), t_off=np.asarray(batch.backbone_off, np.uint64),
                t_blob=np.asarray(batch.backbone, np.uint8), rec_begin=np.asarray(batch.aln_begin, np.uint64),
                pos=np.asarray(pos, np.uint32), q_off=np.asarray(q_off, np.uint64), q_len=np.asarray(q_len, np.uint32),
                q_blob=np.frombuffer(b"".join(qs), np.uint8), op_begin=np.asarray(op_begin, np.uint64),
                ops=np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32))


def records_to_arrays(targets):
    """targets = [(target bases, [(pos, read bases, ops)])] as the arrays of a dagcon_cigar_batch (a dict)."""
    tlen, t_off, rec_begin, pos, q_off, q_len, op_begin, ops, tb, qb = [], [], [0], [], [], [], [0], [], [], []
    tp = qp = 0
    for tseq, recs in targets:
        tlen.append(len(tseq)); t_off.append(tp); tb.append(bytes(tseq)); tp += len(tseq)
        for p, q, oo in recs:
            pos.append(p); q_off.append(qp); q_len.append(len(q)); qb.append(bytes(q)); qp += len(q)
            ops.extend(int(x) for x in oo)
            op_begin.append(len(ops))
        rec_begin.append(len(pos))
    return dict(tlen=np.asarray(tlen, np.uint32), t_off=np.asarray(t_off, np.uint64),
                t_blob=np.frombuffer(b"".join(tb), np.uint8), rec_begin=np.asarray(rec_begin, np.uint64),
                pos=np.asarray(pos, np.uint32), q_off=np.asarray(q_off, np.uint64), q_len=np.asarray(q_len, np.uint32),
                q_blob=np.frombuffer(b"".join(qb), np.uint8), op_begin=np.asarray(op_begin, np.uint64),
                ops=np.asarray(ops, np.uint32))


def to_fasta(names, seqs, width=60):
    out = []
    for n, s in zip(names, seqs):
        s = bytes(s).decode()
        out.append(">" + n)
        out.extend(s[i:i + width] for i in range(0, len(s), width))
    return ("\n".join(out) + "\n").encode()


def to_sam(names, tlens, targets, header=True, flags=None, qnames=None):
    """SAM text (LF line ends) of targets = [[(pos, read bases, ops)]]: one @SQ per target, then the records target by
    target.  flags / qnames: optional per-record lists (flat, in record order); FLAG 0 and q<target>_<k> otherwise."""
    lines = []
    if header:
        lines.append("@HD\tVN:1.6\tSO:coordinate")
        lines.extend("@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in zip(names, tlens))
        lines.append("@PG\tID:twin\tPN:cigar_twin")
    i = 0
    for g, recs in enumerate(targets):
        for k, (p, q, oo) in enumerate(recs):
            fl = 0 if flags is None else flags[i]
            qn = "q%d_%d" % (g, k) if qnames is None else qnames[i]
            lines.append("\t".join([qn, str(fl), names[g], str(p), "60", cigar_string(oo), "*", "0", "0",
                                    bytes(q).decode() or "*", "*"]))
            i += 1
    return ("\n".join(lines) + "\n").encode()
