"""CPU twin of the kept parts (include/dagcon.h, rule 12) and of pbdagcon --hap-contigs / --hap-windows,
written from the rule and not from the C++.  numpy / Python only.

    keep(pos, lo, hi)                   -> (i0, i1, p_first, p_last) of one segment; (0, 0, 0, 0): nothing kept
    contigs(windows, min_len)           -> [(t0, t1, seq, block)]: the joined pieces of one label of one target
    contig_lines(rname, label, ps, t0, t1, seq) -> the FASTA record
    window_line(...) / site_line(...)   -> the lines of --hap-windows
"""
import numpy as np


def keep(pos, lo, hi):
    """A segment's positions P (1-based, relative to its window).  i0: the least i with P(i) > lo; i1: the least i >= i0
    with P(i) > hi, else n.  Only first crossings count; nothing assumes that P is monotone.  Empty when there is no i0 or
    i1 == i0: then 0 0 0 0."""
    n = len(pos)
    i0 = next((i for i in range(n) if pos[i] > lo), None)
    if i0 is None:
        return 0, 0, 0, 0
    i1 = next((i for i in range(i0, n) if pos[i] > hi), n)
    if i1 == i0:
        return 0, 0, 0, 0
    return i0, i1, int(pos[i0]), int(pos[i1 - 1])


def contigs(windows, min_len):
    """The joined pieces of one label of one target.  windows: the DERIVED windows of that label in window order,
    (w, begin, block, [(seq, (i0, i1, p_first, p_last))]): the window's index among the target's windows, its begin, the
    block it belongs to and the keep record of every segment.  A kept part continues the piece before it iff it was cut at
    its core begin (i0 > 0), that piece is the kept part just before it in this order, comes from window w - 1, was cut at
    its core end (i1 < n), and both windows are of one block.  Everything else starts a new piece: an unsplit window in
    between has no derived window, so w - 1 is not there.  Pieces shorter than min_len are dropped.
    Returns [(t0, t1, seq, block)] with t0 = p_first + begin - 1 of the first part and t1 = p_last + begin of the last."""
    pieces = []
    last = None                                                # (window, block) of the last kept part, if it was cut at its core end
    for w, begin, block, segs in windows:
        for seq, (i0, i1, pf, pl) in segs:
            if i1 <= i0:
                continue
            if i0 > 0 and last == (w - 1, block):
                pieces[-1][1] = pl + begin
                pieces[-1][2] += bytes(seq[i0:i1])
            else:
                pieces.append([pf + begin - 1, pl + begin, bytes(seq[i0:i1]), block])
            last = (w, block) if i1 < len(seq) else None
    return [tuple(p) for p in pieces if len(p[2]) >= min_len]


def contig_record(rname, label, ps, t0, t1, seq):
    """One record of --hap-contigs: >RNAME/hap{1|2}/PS/t0_t1 and the bases on one line."""
    return ">%s/hap%d/%d/%d_%d\n%s\n" % (rname, label, ps, t0, t1, bytes(seq).decode())


def order_records(recs):
    """recs: [(t0, label, text)] of one target -> the texts by t0, label 1 before label 2 at equal t0."""
    return [x[2] for x in sorted(recs, key=lambda r: (r[0], r[1]))]


def window_line(rname, begin, end, ps, n1, n2, n0, sep, agree, disagree, split, flip):
    """#window RNAME BEGIN END PS N1 N2 N0 SEP AGREE DISAGREE SPLIT, in the block's orientation: under flip N1 and N2
    change places."""
    if flip:
        n1, n2 = n2, n1
    return "#window\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (rname, begin, end, ps, n1, n2, n0, sep, agree, disagree, split)


def site_line(rname, pos1, phase, p1, m1, p2, m2, flip):
    """RNAME POS PHASE P1 M1 P2 M2 (POS 1-based, target coordinates), in the block's orientation: under flip the two
    pairs change places and PHASE changes sign."""
    if flip:
        phase, p1, m1, p2, m2 = -phase, p2, m2, p1, m1
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d" % (rname, pos1, phase, p1, m1, p2, m2)
