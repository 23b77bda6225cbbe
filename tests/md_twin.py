"""CPU twin of the MD input (include/dagcon.h, dagcon_md_tags): the grammar of an MD:Z text, what makes a record
non-conforming, and the target blob the device rebuilds from CIGAR, SEQ and MD.  numpy / re / Python on top of
cigar_twin: imports neither the product nor the oracle.

    encode(pos, q, t, ops) -> text             the MD:Z text of a conforming record against its target's bases
    events(text) -> (covered, [(k, letter)])   or None when the text breaks the grammar; k counts from pos - 1
    why(text, pos, q_len, tlen, ops) -> None | "grammar" | "covered" | "cigar"
    rebuild(targets, texts) -> (T, conflict)   targets = [(tlen, [(pos, q, ops)])], texts = [[text]]: per target its
                                               rebuilt bases (bytes) and whether its tags disagree
"""
import re

import numpy as np

import cigar_twin as ct

GRAMMAR = re.compile(rb"[0-9]+(?:(?:[A-Za-z]|\^[A-Za-z]+)[0-9]+)*")
TOKEN = re.compile(rb"[0-9]+|\^[A-Za-z]+|[A-Za-z]")
_MATCH = (ct.M, ct.EQ, ct.X)


def encode(pos, q, t, ops):
    """What an aligner writes: a number between any two letter groups (0 when nothing matched), bytes compared
    verbatim, the target's letters as they are."""
    out, run = [], 0
    qi, ti = 0, pos - 1
    for o in ops:
        code, ln = int(o) & 15, int(o) >> 4
        if code in _MATCH:
            for _ in range(ln):
                if q[qi] == t[ti]:
                    run += 1
                else:
                    out.append(b"%d%c" % (run, t[ti]))
                    run = 0
                qi += 1; ti += 1
        elif code == ct.D:
            out.append(b"%d^%s" % (run, bytes(t[ti:ti + ln])))
            run = 0
            ti += ln
        elif code in (ct.I, ct.S):
            qi += ln
    out.append(b"%d" % run)
    return b"".join(out)


def events(text):
    text = bytes(text)
    if not GRAMMAR.fullmatch(text):
        return None
    k, letters = 0, []
    for tok in TOKEN.findall(text):
        if tok[:1].isdigit():
            if len(tok) > 9 or int(tok) >= 1 << 28:
                return None
            k += int(tok)
        else:
            for b in tok.lstrip(b"^"):
                letters.append((k, b))
                k += 1
    return k, letters


def _tbases(ops):
    ops = np.asarray(ops, dtype=np.int64).reshape(-1)
    return int((ops >> 4)[np.isin(ops & 15, (ct.M, ct.D, ct.EQ, ct.X))].sum())


def why(text, pos, q_len, tlen, ops):
    ev = events(text)
    if ev is None:
        return "grammar"
    if not ct.conforming(pos, q_len, tlen, ops):
        return "cigar"
    if ev[0] != _tbases(ops):
        return "covered"
    return None


def rebuild(targets, texts):
    """Step 1: a letter of any conforming record; step 2: a read base under M / = / X where no record spells; step 3:
    'N'.  conflict: two letters differ at one position, or two read bases differ at a position no record spells."""
    T, conflict = [], []
    for (tlen, recs), mds in zip(targets, texts):
        assert len(recs) == len(mds)
        let = np.zeros(tlen, np.uint8)
        rb = np.zeros(tlen, np.uint8)
        let_c = np.zeros(tlen, bool)
        rb_c = np.zeros(tlen, bool)
        for (pos, q, ops), text in zip(recs, mds):
            if why(text, pos, len(q), tlen, ops) is not None:
                continue
            for k, b in events(text)[1]:
                x = pos - 1 + k
                let_c[x] |= let[x] != 0 and let[x] != b
                if let[x] == 0:
                    let[x] = b
            qa = np.frombuffer(bytes(q), np.uint8)
            qi, ti = 0, pos - 1
            for o in ops:
                code, ln = int(o) & 15, int(o) >> 4
                if code in _MATCH:
                    seg, cur = qa[qi:qi + ln], rb[ti:ti + ln]
                    rb_c[ti:ti + ln] |= (cur != 0) & (cur != seg)
                    rb[ti:ti + ln] = np.where(cur != 0, cur, seg)
                if code in ct._QRY:
                    qi += ln
                if code in ct._TGT:
                    ti += ln
        T.append(np.where(let != 0, let, np.where(rb != 0, rb, ord("N"))).astype(np.uint8).tobytes())
        conflict.append(bool(let_c.any() or (rb_c & (let == 0)).any()))
    return T, conflict
