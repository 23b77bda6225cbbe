"""Rule 11 of include/dagcon.h in plain Python: the edits of the two groups of a split target, paired.

A derived target is (spans, edits): spans = [(t0, t1)] of its segments in their order (None: the target failed),
edits = [(t_pos, t_len, alt bytes)] over all of its segments, in their order.  Derived targets come in pairs, label 1 at an
even d and label 2 at d ^ 1.  The twin asserts on every input what the kernel relies on (occupied intervals disjoint,
t_pos rising strictly) and what the rule promises (HOM and CLASH symmetric, mate an involution on HOM).

Also the lines of pbdagcon --hap-vcf (csrc/host/hap_vcf.h), formatted from the same arrays."""

NOCOVER, HET, CLASH, HOM = 0, 1, 2, 3
NONE = 0xFFFFFFFFFFFFFFFF
NAMES = {NOCOVER: "NOCOV", HET: "HET", CLASH: "CLASH", HOM: "HOM"}


def occupied(e):
    """[t_pos, t_pos + max(t_len, 1)): a pure insertion occupies the base behind it."""
    return e[0], e[0] + max(e[1], 1)


def overlap(a, b):
    (a0, a1), (b0, b1) = occupied(a), occupied(b)
    return a0 < b1 and b0 < a1


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and bytes(a[2]) == bytes(b[2])          # exact bytes: case counts


def covered(e, spans):
    return any(t0 <= e[0] and e[0] + e[1] <= t1 for t0, t1 in spans)


def check_ascent(edits):
    for a, b in zip(edits, edits[1:]):
        assert a[0] < b[0] and occupied(a)[1] <= occupied(b)[0], (a, b)


def pair(own, partner, spans, overlap=overlap, same=same, covered=covered, cover_first=False):
    """[(state, index into partner or None)] per edit of `own`.  spans: the partner's segments, None when it failed.  The
    keyword arguments exist for the tests, which show that a wrong version of each part is told from the right one."""
    out = []
    spans = spans or []
    partner = partner if spans else []
    for e in own:
        hom = [j for j, x in enumerate(partner) if same(e, x)]
        cl = [j for j, x in enumerate(partner) if overlap(e, x)]
        if hom:
            out.append((HOM, hom[0]))
        elif cover_first and covered(e, spans):
            out.append((HET, None))
        elif cl:
            out.append((CLASH, cl[0]))
        elif covered(e, spans):
            out.append((HET, None))
        else:
            out.append((NOCOVER, None))
    return out


def calls(targets):
    """targets: [(spans or None, edits)] of the derived batch, d and d ^ 1 partners.  Returns (state, mate), flat over the
    targets in their order, a failed target's edits left out as dagcon_fetch_edits leaves them out; mate is an index into
    the same flat arrays or NONE."""
    assert len(targets) % 2 == 0
    live = [[] if spans is None else list(edits) for spans, edits in targets]
    begin = [0]
    for e in live:
        check_ascent(e)
        begin.append(begin[-1] + len(e))
    state, mate = [], []
    per = []
    for d, own in enumerate(live):
        spans = targets[d ^ 1][0]
        p = pair(own, live[d ^ 1], spans)
        per.append(p)
        for s, j in p:
            state.append(s)
            mate.append(NONE if j is None else begin[d ^ 1] + j)
    # symmetry: the mate of a HOM is HOM and points back; the mate of a CLASH is CLASH (and clashes with it)
    for i, (s, m) in enumerate(zip(state, mate)):
        if s == HOM:
            assert state[m] == HOM and mate[m] == i
        elif s == CLASH:
            assert state[m] == CLASH
        else:
            assert m == NONE
    for d, p in enumerate(per):
        for k, (s, j) in enumerate(p):
            if s == CLASH:
                assert overlap(live[d][k], live[d ^ 1][j])
    return state, mate


def from_device(dev, status):
    """The derived batch in the twin's form, from the device's own arrays as test_edit_support._device lists them:
    dev[d] = [(seq, t0, t1, [(t_pos, t_len, c, c_len)])] per segment, status[d] the target's status."""
    out = []
    for per, st in zip(dev, status):
        if st:
            out.append((None, []))
            continue
        out.append(([(t0, t1) for _, t0, t1, _ in per],
                    [(tp, tl, bytes(seq[c:c + cl])) for seq, _, _, edits in per for tp, tl, c, cl in edits]))
    return out


# ---- pbdagcon --hap-vcf ------------------------------------------------------------------------------------------------

def anchor(T, tp, tl, alt):
    """The anchoring rule of pbdagcon --vcf: (POS, REF, ALT)."""
    ref, pos = T[tp:tp + tl], tp + 1
    if not tl or not alt:
        if tp > 0:
            ref, alt, pos = T[tp - 1:tp] + ref, T[tp - 1:tp] + alt, tp
        else:
            b = T[tp + tl:tp + tl + 1]
            ref, alt, pos = (ref + b) or b".", (alt + b) or b".", 1
    return pos, ref.decode(), alt.decode()


def header(contigs):
    out = ["##fileformat=VCFv4.2"] + ["##contig=<ID=%s,length=%d>" % c for c in contigs]
    out += ['##INFO=<ID=PAIR,Number=1,Type=String,Description="UNSPLIT: the target was not split, the edit is the one consensus\' own; HET: only this '
            'group\'s consensus carries the edit and the other covers it; HOM: both carry it; CLASH: the other group carries another edit that touches '
            'it; NOCOV: the other group has no consensus there (this build\'s own rule, parity unpinned)">',
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Unsplit target: alignments that span the edit\'s window">',
            '##INFO=<ID=AD,Number=R,Type=Integer,Description="Unsplit target: spanning alignments that carry the target\'s allele, the consensus\' allele">',
            '##INFO=<ID=DP1,Number=1,Type=Integer,Description="Alignments of group 1 that span the edit\'s window">',
            '##INFO=<ID=AD1,Number=R,Type=Integer,Description="Spanning alignments of group 1 that carry the target\'s allele, the edit\'s allele">',
            '##INFO=<ID=DP2,Number=1,Type=Integer,Description="Alignments of group 2 that span the edit\'s window">',
            '##INFO=<ID=AD2,Number=R,Type=Integer,Description="Spanning alignments of group 2 that carry the target\'s allele, the edit\'s allele">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype: group 1 | group 2 of a split target, 1/1 on an unsplit one">',
            '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set: a split target is one block">',
            "##pbdagcon_note=the reads the split left unlabelled are in both groups: DP1 + DP2 may exceed the target's depth",
            "##pbdagcon_note=a CLASH is written as two records, 1|. and .|1, not as one record 1|2; REF and ALT are not normalised",
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample"]
    return out


def unsplit_lines(name, T, edits, sup):
    """edits: [(t_pos, t_len, alt)], sup: [(span, ref, alt)] of an unsplit target, in their order."""
    out = []
    for (tp, tl, alt), (sp, nr, na) in zip(edits, sup):
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\tPAIR=UNSPLIT;DP=%d;AD=%d,%d\tGT\t1/1" % ((name,) + anchor(T, tp, tl, alt) + (sp, nr, na)))
    return out


def split_lines(name, T, e1, s1, c1, e2, s2, c2):
    """e: [(t_pos, t_len, alt)], s: [(span, ref, alt)], c: [(state, index into the other group's edits or None)] of the
    label-1 and the label-2 group.  Merged by (t_pos, label); the HOM mate of label 2 is not written."""
    rows = [(e[0], 1, k) for k, e in enumerate(e1)] + [(e[0], 2, k) for k, e in enumerate(e2) if c2[k][0] != HOM]
    out = []
    for _, label, k in sorted(rows):
        (tp, tl, alt), (sp, nr, na), (st, j) = (e1[k], s1[k], c1[k]) if label == 1 else (e2[k], s2[k], c2[k])
        info = "PAIR=%s;DP%d=%d;AD%d=%d,%d" % (NAMES[st], label, sp, label, nr, na)
        if st == HOM:
            info += ";DP2=%d;AD2=%d,%d" % s2[j]
        other = "1" if st == HOM else "0" if st == HET else "."
        gt = "1|" + other if label == 1 else other + "|1"
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\t%s\tGT:PS\t%s:1" % ((name,) + anchor(T, tp, tl, alt) + (info, gt)))
    return out
