"""Pileups with a single admissible cut position, on either side of each rule, for tests/test_cut_limits.py.

Where a partial-span pileup may be cut is decided by k_readspan (k_build.hip.h), the prologue k_merge_pro, k_cuts2 and
k_merge_fin (k_merge.hip.h): five conditions on a backbone position, three "one piece" fallbacks (256 dead zones,
DG_CUT_STARTS reads, DG_SH_MAX shared lists), a search window taken 64 positions a round, and the defer list bestPath
reads (DG_DEFER_MAX).  A wrong cut is exact on most inputs -- the worker behind usually comes first -- so parity on random
pileups says little; the families here leave one position open in a window and put the rule's boundary on it.

Every constructed alignment is a backbone that alternates A and C (a deleted base never equals the next read base, so no
gap moves) with inserted bases that are neither A nor C, except where a leading insertion must carry a backbone base;
oracle.normalize_gaps returns every one of them unchanged (asserted by merge_cases.target_of).

Three models, all over oracle/pymodel.py and in device vertex ids (device_ids: the map test_gpu_parity._oracle_graph
builds, restated):

  spans / spans_kernel   what k_readspan must find, said by meaning (first and last match column, the insertion columns
                         outside them) and as the kernel's two loops; a CPU test holds them equal on every read here.
  Cuts                   k_cuts2's search restated: pmin = 2 (maxlead + 2), want = min(blen / seg_min, seg_max, 64), the
                         ideal position 1 + s * blen / want, the window blen / want / 2 taken 64 positions a round, the
                         lowest admissible position, conditions (1), (4), (5), the fallbacks, the shared vertices, and
                         the fixed point of k_merge_fin's defer list.  It predicts the merge row (with condition (5)) and
                         the bestPath row (without).  It reads the graph as the prologue leaves it (Trace.snap): the
                         FIFO's levels 0 .. maxlead + 1, counted as dg_merge_segment counts them.
  sound                  the check that does not restate the kernel: on Trace, pymodel's mergeNodes with a log of every
                         list entry a visit adds or erases, (a) a cut vertex is dequeued from a FIFO that holds nothing
                         else, (b) the visits behind the prologue run through the segments in order (every vertex is
                         visited once, so the visits between two cuts are the live vertices between them), (c) a visit
                         of segment i adds or erases entries only in lists of segment i that name vertices of segment i,
                         or, in a list Cuts calls shared (out[enter], in[exit], the out-lists of the shared vertices),
                         entries that name vertices of segment i.  The prologue's visits and the exit's are set aside; a
                         prologue vertex that is not shared belongs to the segment its out-edges lead into (an edge into a
                         cut vertex is an entry of that vertex's in-list: the segment in front).  Of a cut
                         vertex the in-list belongs to the segment in front and the out-list to the one behind, and
                         mergeInNodes(cut) is the last act of the segment in front.  Changed edge counts are not logged.

MUTATIONS names the ways Cuts can be made wrong on purpose (CPU only: a wrong cut on the device is a data race).

Not reachable: DG_E_LIST_OVF.  The host sizes the worklist for every piece k_cuts2 can ask for,
`c->worklist_cap = max(c->worklist_cap, min(T * c->seg_max + 64, 0x0FFFFFFF))` (api_run.hip.h, dagcon_upload), and
k_cuts2 adds at most seg_max entries a target.  No family is built for it.
"""
import functools
import sys

import oracle
from oracle import pymodel
from merge_cases import CNS_OPTS, GAP, GRAPH_OPTS, host_full_span, target_of
from util import batch_from_targets, oracle_batch

# the device's constants, restated (dagcon_dev.h, k_merge.hip.h, api_ctx.h)
DG_SH_MAX, DG_DEFER_MAX, DG_CUT_STARTS, DG_DEAD_MAX, SH_LOG = 8, 64, 2048, 256, 16
NOSEG_END = 0xFFFFFFFF
DG_NF_DELETED, DG_NF_DEFER = 2, 8

MUTATIONS = ("pmin_ge", "dead_hi_minus", "dead_hi_plus", "c5_lo", "c5_hi", "c5_drop", "seg_lt", "win_le")


def plan(max_segments=0, min_segment_len=0, bp_segs=None):
    """dg_plan_pieces for a partial-span batch: (seg_max, seg_min, bp_max, bp_seg_min).  bp_segs: DAGCON_BP_SEGS."""
    seg_min = min_segment_len or 256
    seg_max = min(max_segments, 64) or 64
    bp_max = 1 if seg_max == 1 else min(64, 3 * seg_max)
    if bp_segs is not None and 1 <= bp_segs <= 64:
        bp_max = bp_segs
    return seg_max, seg_min, bp_max, (seg_min + 2) // 3


# ---- building blocks ---------------------------------------------------------------------------------------------------

def alternating(n):
    return bytes(b"AC"[i & 1] for i in range(n))


def cols(bb, start, ops):
    """An alignment that starts at base `start`.  ops: "M" matches the next base, "D" deletes it, "X" mismatches it (the
    normalized form: the base deleted, then a G inserted), bytes are inserted as they are."""
    q, t = bytearray(), bytearray()
    pos = start
    for op in ops:
        if isinstance(op, bytes):
            q += op
            t += bytes([GAP]) * len(op)
            continue
        b = bb[pos - 1]
        if op == "M":
            q.append(b); t.append(b)
        elif op == "D":
            q.append(GAP); t.append(b)
        else:
            q += bytes([GAP, ord("G")]); t += bytes([b, GAP])
        pos += 1
    return start, bytes(q), bytes(t)


def blocker(bb, opened, dele=(), s=1, e=None):
    """A read over bases s .. e that matches s, e and the bases in `opened`, deletes those in `dele` and mismatches every
    other one: no position it mismatches or deletes can be a cut (condition (1))."""
    e = len(bb) if e is None else e
    return cols(bb, s, ["M" if p in (s, e) or p in opened else "D" if p in dele else "X" for p in range(s, e + 1)])


def plain(bb, s, e, lead=b"", trail=b""):
    """A read that matches bases s .. e, behind `lead` and in front of `trail`."""
    return cols(bb, s, ([lead] if lead else []) + ["M"] * (e - s + 1) + ([trail] if trail else []))


# ---- k_readspan --------------------------------------------------------------------------------------------------------

def spans(aln):
    """(s, e, lead, trail) of a normalized alignment, by meaning: the positions of its first and last match column and the
    insertion columns in front of the first / behind the last; a read without a match column is all lead, s = e = 0."""
    s0, q, t = aln
    pos, match = s0, []
    for i, (a, b) in enumerate(zip(q, t)):
        if b != GAP:
            if a == b:
                match.append((i, pos))
            pos += 1
    if not match:
        return 0, 0, sum(b == GAP for b in t), 0
    (i0, s), (i1, e) = match[0], match[-1]
    return s, e, sum(b == GAP for b in t[:i0]), sum(b == GAP for b in t[i1 + 1:])


def spans_kernel(aln):
    """The same as k_readspan's two loops say it (lo = 0, hi = the columns: no trimming)."""
    s0, q, t = aln
    hi, ins = len(q), sum(b == GAP for b in t)
    lead = dels = trail = tdels = 0
    i = 0
    while i < hi:
        if q[i] == t[i]:
            break
        if t[i] == GAP:
            lead += 1
        elif q[i] == GAP:
            dels += 1
        i += 1
    if i == hi:
        return 0, 0, lead, 0
    k = hi
    while k > i + 1:
        if q[k - 1] == t[k - 1]:
            break
        if t[k - 1] == GAP:
            trail += 1
        elif q[k - 1] == GAP:
            tdels += 1
        k -= 1
    return s0 + dels, s0 + (hi - ins) - 1 - tdels, lead, trail


# ---- the reference's mergeNodes, logged ----------------------------------------------------------------------------------

def device_ids(tlen, alns):
    """Oracle id -> device id (test_gpu_parity._oracle_graph): the device numbers the inserted vertices whose _bbMap is p
    in (read, column) order, then backbone vertex p."""
    ins_pos = []
    for s, q, t in alns:
        bbp = s
        for a, b in zip(q, t):
            if a == b or a == GAP:
                bbp += 1
            elif b == GAP:
                ins_pos.append(bbp)
    gcount = [0] * (tlen + 2)
    for p in ins_pos:
        gcount[p] += 1
    gbase, acc = [], 0
    for p in range(tlen + 2):
        gbase.append(acc)
        acc += gcount[p] + 1
    o2d = [gbase[p] + gcount[p] for p in range(tlen + 2)]
    seen = [0] * (tlen + 2)
    for p in ins_pos:
        o2d.append(gbase[p] + seen[p])
        seen[p] += 1
    return o2d


class Trace(pymodel.AlnGraph):
    """AlnGraph whose mergeNodes logs, per visit, the FIFO's occupancy and every list entry mergeInNodes and mergeOutNodes
    add ("+") or erase ("-"): (op, side, owner, named).  With lvl_stop it also keeps the graph as the prologue leaves it
    (snap): dg_merge_segment's DG_MM_PROLOGUE counts a level whenever the head reaches the tail the level before ended at
    and stops in front of the first vertex of level lvl_stop + 1, or when the FIFO runs dry."""

    def __init__(self, *a, **kw):
        self.cur = None
        super().__init__(*a, **kw)
        self.visits, self.snap = [], None

    def _add_edge(self, u, v):
        e = super()._add_edge(u, v)
        if self.cur is not None:
            self.cur += [("+", "out", u, v), ("+", "in", v, u)]
        return e

    def _reap(self, n):
        if self.cur is not None:
            for e in self.nodes[n].out:
                self.cur += [("-", "out", n, e.dst), ("-", "in", e.dst, n)]
            for e in self.nodes[n].inn:
                self.cur += [("-", "in", n, e.src), ("-", "out", e.src, n)]
        super()._reap(n)

    def _snapshot(self, qh, queue):
        self.snap = dict(qh=qh, qt=len(queue), visited=list(queue[:qh]), in_exit=len(self.nodes[self.exit].inn),
                         out=[[e.dst for e in n.out] for n in self.nodes],
                         weight=[n.weight for n in self.nodes], deleted=[n.deleted for n in self.nodes])

    def merge_nodes(self, lvl_stop):
        queue, head = [self.enter], 0
        lvl, lvl_end = 0, 1
        while head < len(queue):
            if self.snap is None:
                if head == lvl_end:
                    lvl += 1
                    lvl_end = len(queue)
                if lvl > lvl_stop:
                    self._snapshot(head, queue)
            fifo = len(queue) - head
            u = queue[head]
            head += 1
            self.cur = tin = []
            self.merge_in(u)
            self.cur = tout = []
            self.merge_out(u)
            self.cur = None
            for e in self.nodes[u].out:
                e.visited = True
                if all(x.visited for x in self.nodes[e.dst].inn):
                    queue.append(e.dst)
            self.visits.append((u, fifo, tin, tout))
        if self.snap is None:
            self._snapshot(head, queue)
        return queue


class Pile:
    """One target: its reads' spans, its coverage, the logged merge, the device's ids."""

    def __init__(self, target):
        self.target = target
        self.tlen, self.alns, _ = target
        self.spans = [spans(a) for a in self.alns]
        self.maxlead = max(s[2] for s in self.spans)
        g = Trace(blen=self.tlen)
        for a in self.alns:
            g.add_aln(a[0], a[1].decode("latin1"), a[2].decode("latin1"))
        self.cov = [n.coverage for n in g.nodes[:self.tlen + 2]]
        self.backbone_n = self.tlen + 2
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 20000))
        try:
            g.merge_nodes(self.maxlead + 1)
        finally:
            sys.setrecursionlimit(old)
        self.g = g
        self.o2d = device_ids(self.tlen, self.alns)
        assert sorted(self.o2d) == list(range(len(g.nodes)))
        self.N = len(g.nodes)
        self.X = self.o2d[g.exit]
        snap = g.snap
        self.allow = snap["qh"] < snap["qt"]
        self.q0 = [self.o2d[v] for v in snap["visited"]]                 # queue0[0 .. nvis)
        self.exit_in_prologue = g.exit in snap["visited"]
        # pro_state[4t .. 4t + 3]
        self.pro_state = (snap["qh"], snap["qt"], snap["qh"], 1 if self.exit_in_prologue else 0)
        self.final_out = {self.o2d[o]: [self.o2d[e.dst] for e in n.out] for o, n in enumerate(g.nodes) if not n.deleted}

    def bbpos(self, o):
        return o if o < self.backbone_n else None

    def figures(self):
        return dict(tlen=self.tlen, reads=len(self.alns), maxlead=self.maxlead, nvis=len(self.q0), allow=self.allow,
                    exit_in_prologue=self.exit_in_prologue, vertices=self.N)


# ---- k_cuts2 and k_merge_fin's defer list, restated ----------------------------------------------------------------------

class Cuts:
    def __init__(self, pile, pl, mut=()):
        self.p, self.mut = pile, frozenset(mut)
        assert self.mut <= set(MUTATIONS)
        seg_max, seg_min, bp_max, bp_seg_min = pl
        p = pile
        snap = p.g.snap
        K = len(p.alns)
        # (4) dead zones behind read ends: the first 256 reads with a trailing run, in read order
        self.dead = [(e, e + tr + 1) for _, e, _, tr in p.spans if tr > 0]
        self.starts = [s for s, _, _, _ in p.spans][:DG_CUT_STARTS]
        allow = p.allow and len(self.dead) <= DG_DEAD_MAX and K <= DG_CUT_STARTS
        self.allow = allow
        self.pmin = 2 * (p.maxlead + 2)
        want = min(p.tlen // (seg_min or 1), seg_max, 64)
        self.want = 1 if (want < 1 or not allow) else want
        want_b = min(p.tlen // (bp_seg_min or 1), bp_max, 64)
        self.want_b = 1 if (want_b < 1 or not allow) else want_b
        self.skipped = 0
        self.merge_pos = self._search(self.want, True)
        self.bp_pos = self._search(self.want_b, False)
        self.wanted = self.want
        self.found = 1 + len(self.merge_pos)
        self.merge_row = [0] + [p.o2d[x] for x in self.merge_pos]
        self.bp_row = [0] + [p.o2d[x] for x in self.bp_pos]
        # the shared out-lists, twice at the most
        self.nseg = len(self.merge_row)
        self.shared_first = None
        for _ in range(2):
            sh = [0]
            if self.nseg > 1:
                for y in p.q0[1:]:
                    o = p.o2d.index(y)
                    if snap["deleted"][o] or y == p.X:
                        continue
                    segs = {self.seg_of(p.o2d[d], self.merge_row) for d in snap["out"][o] if p.o2d[d] != p.X}
                    if len(segs) > 1:
                        sh.append(y)
            if self.shared_first is None:
                self.shared_first = list(sh)
            if len(sh) <= DG_SH_MAX:
                break
            self.nseg = 1
        self.shared = sh
        if self.nseg == 1:
            self.merge_row = [0]
        self.defer = self._defer()

    def seg_of(self, d, row):
        if "seg_lt" in self.mut:
            return sum(c < d for c in row[1:])
        return sum(c <= d for c in row[1:])

    def _ok(self, pos, cond5):
        p, snap = self.p, self.p.g.snap
        v = pos                                            # oracle id of backbone vertex pos
        if snap["weight"][v] - 1 != p.cov[pos]:            # (1)
            return False
        adj = -1 if "dead_hi_minus" in self.mut else 1 if "dead_hi_plus" in self.mut else 0
        for e, hi in self.dead[:DG_DEAD_MAX]:              # (4)
            if e < pos <= hi + adj:
                return False
        if cond5 and "c5_drop" not in self.mut:            # (5)
            for d in snap["out"][v]:
                if d == p.g.exit or d >= p.backbone_n:
                    continue
                q = d
                for st in self.starts:
                    lo = st > pos + 1 if "c5_lo" in self.mut else st > pos
                    hi = st < q if "c5_hi" in self.mut else st <= q
                    if lo and hi:
                        return False
        return True

    def _search(self, want, cond5):
        blen = self.p.tlen
        out = []
        for s in range(1, want):
            p0 = 1 + s * blen // want
            span = blen // want // 2
            found, o = None, 0
            while o < span and found is None:
                for lane in range(64):
                    pos = p0 + o + lane
                    inside = o + lane <= span if "win_le" in self.mut else o + lane < span
                    above = pos >= self.pmin if "pmin_ge" in self.mut else pos > self.pmin
                    if inside and above and pos <= blen and self._ok(pos, cond5):
                        found = pos
                        break
                o += 64
            if found is None:
                self.skipped += cond5
            else:
                out.append(found)
        return out

    def worklist(self, t):
        """This target's rows of the worklist."""
        r = self.merge_row
        return [(t, r[s], r[s + 1] if s + 1 < len(r) else NOSEG_END) for s in range(len(r))]

    def _defer(self):
        """k_merge_fin: enter, the prologue's vertices with a successor in another bestPath piece than their own id's, and
        their ancestors among the prologue's vertices, to a fixed point; None past DG_DEFER_MAX."""
        p, row = self.p, self.bp_row
        dl = [0]
        if len(row) > 1:
            more = True
            while more:
                more = False
                for y in p.q0[1:]:
                    if y not in p.final_out or y in dl or y == p.X:
                        continue
                    sy = self.seg_of(y, row)
                    f = False
                    for d in p.final_out[y]:
                        if d == p.X:
                            continue
                        if d in dl or self.seg_of(d, row) != sy:
                            f = True
                            break
                    if f:
                        if len(dl) >= DG_DEFER_MAX:
                            return None
                        dl.append(y)
                        more = True
        return dl


# ---- the semantic check ---------------------------------------------------------------------------------------------------

def sound(pile, row, shared):
    """Whether the reference's sweep can be split at the cut vertices `row` (device ids, row[0] = 0) with the out-lists of
    `shared` (device ids) under the shared-list protocol: the list of what speaks against it, empty if nothing does."""
    p, g = pile, pile.g
    bad = []
    cuts = list(row)
    nseg = len(cuts)
    upper = cuts[1:] + [p.X]
    pro = set(p.q0)
    shared = set(shared)
    snap = g.snap

    def by_id(d):
        return sum(c <= d for c in cuts[1:])

    home = {}                                              # a prologue vertex that is not shared: where its out-edges lead
    for y in p.q0[1:]:
        o = p.o2d.index(y)
        if y in shared or y == p.X:
            continue
        ds = [p.o2d[d] for d in snap["out"][o] if p.o2d[d] != p.X]
        if ds:
            home[y] = sum(c < ds[0] for c in cuts[1:])     # (an edge into a cut vertex is the piece in front's)

    def names_ok(nm, i):
        if nm == p.X or nm == 0 or nm in shared:
            return True
        if nm in home:
            return home[nm] == i
        return cuts[i] <= nm <= upper[i]

    def list_ok(own, side, i):
        if own in home:
            return home[own] == i
        if own == cuts[i] and i > 0:
            return side == "out"
        if own == upper[i]:
            return side == "in"
        return cuts[i] < own < upper[i] or (i == 0 and own == 0)

    nvis = len(p.q0)
    seen_cut = set()
    cur = 0
    for idx, (u, fifo, tin, tout) in enumerate(g.visits):
        d = p.o2d[u]
        if idx < nvis:
            if d in cuts[1:]:
                bad.append(f"cut vertex {d} is visited by the prologue")
            continue
        if u == g.exit:
            continue
        if d in cuts[1:]:
            k = cuts.index(d)
            seen_cut.add(d)
            if fifo != 1:
                bad.append(f"cut vertex {d} is dequeued from a FIFO of {fifo}")
            phases = ((k - 1, tin), (k, tout))
            seg = k
        else:
            seg = home.get(d, by_id(d))
            phases = ((seg, tin), (seg, tout))
        if seg < cur:
            bad.append(f"vertex {d} of segment {seg} is visited behind one of segment {cur}")
        cur = max(cur, seg)
        for i, log in phases:
            for op, side, owner, named in log:
                own, nm = p.o2d[owner], p.o2d[named]
                if (side == "out" and own in shared) or (side == "in" and own == p.X):
                    if not names_ok(nm, i):
                        bad.append(f"visit of {d} (segment {i}): {op} {side}[{own}] (shared) names {nm}")
                elif not (list_ok(own, side, i) and names_ok(nm, i)):
                    bad.append(f"visit of {d} (segment {i}): {op} {side}[{own}] names {nm}")
    for c in cuts[1:]:
        if c not in seen_cut and not any("cut vertex %d " % c in b for b in bad):
            bad.append(f"cut vertex {c} is never dequeued")
    return bad


def appends(pile, row):
    """Entries the workers append to in[exit] and to out[enter], per segment of `row`: {"in": [..], "out": [..]}."""
    p, g = pile, pile.g
    cuts = list(row)
    out = {"in": [0] * len(cuts), "out": [0] * len(cuts)}
    for idx, (u, _, tin, tout) in enumerate(g.visits):
        if idx < len(p.q0) or u == g.exit:
            continue
        d = p.o2d[u]
        k = sum(c <= d for c in cuts[1:])
        for i, log in ((k - 1 if d in cuts[1:] else k, tin), (k, tout)):
            for op, side, owner, _ in log:
                if op == "+" and ((side == "in" and owner == g.exit) or (side == "out" and owner == g.enter)):
                    out[side][i] += 1
    return out


def read_dump(path):
    """A DAGCON_DUMP file (dump_target, api_records.hip.h) as a dict; the part behind the worklist where it is there."""
    import struct
    import numpy as np
    raw = open(path, "rb").read()
    N, bp_max, psz, seg_max = struct.unpack_from("4I", raw, 0)
    off = 16
    cuts = np.frombuffer(raw, np.uint32, bp_max + 2, off); off += 4 * (bp_max + 2)
    nd = np.frombuffer(raw, np.uint8, 32 * N, off).reshape(N, 32); off += 32 * N
    off += 4 * psz + 8 * N + 4 * N
    nl = struct.unpack_from("I", raw, off)[0]; off += 4
    wl = np.frombuffer(raw, np.uint32, 3 * nl, off).reshape(nl, 3); off += 12 * nl
    d = dict(N=N, bp_max=bp_max, seg_max=seg_max, bp_row=[int(x) for x in cuts[1:1 + int(cuts[0])]],
             flags=nd[:, 5].copy(), worklist=[tuple(int(x) for x in r) for r in wl])
    if off < len(raw):
        nsh = 2 + 2 * DG_SH_MAX
        d["sh_cnt"] = [int(x) for x in np.frombuffer(raw, np.uint32, nsh, off)]; off += 4 * nsh
        d["defer"] = [int(x) for x in np.frombuffer(raw, np.uint32, DG_DEFER_MAX + 1, off)]; off += 4 * (DG_DEFER_MAX + 1)
        d["pro_state"] = tuple(int(x) for x in np.frombuffer(raw, np.uint32, 4, off)); off += 16
        K = struct.unpack_from("I", raw, off)[0]; off += 4
        rd = np.frombuffer(raw, np.uint32, 4 * K, off).reshape(4, K)
        d["spans"] = [tuple(int(rd[j, r]) for j in range(4)) for r in range(K)]
    return d


# ---- the families ----------------------------------------------------------------------------------------------------------
# A family is a list of (name, target, pieces, expect): `pieces` the setting its figures are asserted at, `expect` the
# merge row's positions there (and the bestPath row's, where the family says something about it).

P64 = dict(max_segments=64, min_segment_len=64)       # 256 bases: ideal positions 65, 129, 193, windows of 32
L = 256
BB = alternating(L)


def _t(reads, bb=BB):
    return target_of(bb, reads)


def covers():
    """Condition (1) at 256 bases under P64.  The blocker leaves open: 80 in the first window, where one read ends and
    another starts (coverage counts them and the weight does too: taken); 140 and 150 in the second (the lower wins);
    200 and 210 in the third, where another read deletes 200 (covered, not passed: 210).  Control: the same with 80
    deleted by a read that crosses it: one piece fewer."""
    def reads(del80):
        r = [blocker(BB, {80, 140, 150, 200, 210}), plain(BB, 30, 80), plain(BB, 80, 120, lead=b"T"),
             cols(BB, 190, ["M"] * 10 + ["D"] + ["M"] * 9)]
        if del80:
            r.append(cols(BB, 75, ["M"] * 5 + ["D"] + ["M"] * 5))
        return r
    return [("covers", _t(reads(False)), P64, dict(merge=[80, 140, 210])),
            ("covers_deleted", _t(reads(True)), P64, dict(merge=[140, 210]))]


def _lead_target(n, m, pos, extras=True):
    """n bases, the only open position `pos`, a longest leading run of m.  Reads: the blocker; one that matches bases 2 and 3; with m > 0 a read whose
    leading run of m is interrupted by deletion columns, and one with no match column at all (m insertions); and a
    read whose only match column is its first (base 2, then an insertion, a deletion, an insertion: its dead zone ends
    at base 5, below every pmin but the first)."""
    bb = alternating(n)
    r = [blocker(bb, {pos}), plain(bb, 2, 3)]
    if m:
        ops = []
        for i in range(m):
            ops += [b"T", "D"] if i % 3 == 0 and i + 1 < m else [b"T"]
        s0 = 2
        nd = sum(o == "D" for o in ops)
        r.append(cols(bb, s0, ops + ["M"] * min(3, n - s0 - nd)))
        r.append((3, b"T" * m, bytes([GAP]) * m))
    if extras and m:
        r.append(cols(bb, 2, ["M", b"T", "D", b"T"]))
    return target_of(bb, r)


def lead():
    """Condition (2): pmin = 2 (maxlead + 2) = 4, 6, 18 for a longest leading run of 0, 1, 7.  The only open position at
    pmin (refused: one piece) and at pmin + 1 (taken).  A window that holds pmin needs 1 + blen / want <= pmin, so each
    target has its own length and min_segment_len; with maxlead = 0 no single window can hold both 4 and 5."""
    out = []
    for m, n_ref, s_ref, n_tak, s_tak in ((0, 6, 3, 8, 4), (1, 10, 4, 10, 4), (7, 32, 16, 32, 16)):
        pmin = 2 * (m + 2)
        out.append((f"lead{m}_at_pmin", _lead_target(n_ref, m, pmin), dict(max_segments=64, min_segment_len=s_ref),
                    dict(merge=[])))
        out.append((f"lead{m}_above", _lead_target(n_tak, m, pmin + 1), dict(max_segments=64, min_segment_len=s_tak),
                    dict(merge=[pmin + 1])))
    return out


def tiny():
    """Targets of 2 .. 6 bases under a read of four inserted bases and no match column (maxlead = 4, lvl_stop = 5: one chain
    from enter to exit), one that matches every base and one that starts at base 2: the prologue reaches exit up to
    some length (pro_state[3] & 1, nothing left in the FIFO, k_merge_fin skips its sweep) and not beyond; where the line
    lies is the model's to say."""
    out = []
    for n in range(2, 7):
        bb = alternating(n)
        reads = [(1, b"TGTG", bytes([GAP]) * 4), plain(bb, 1, n), plain(bb, 2, n)]
        out.append((f"tiny{n}", target_of(bb, reads), dict(max_segments=64, min_segment_len=1), None))
    return out


def _dead_target(r, e, pos, tdels=False, many=0):
    ops = ["M"] * 11
    if tdels:                                          # the run interrupted by deletions: M T D T D T ...
        for i in range(r):
            ops += [b"T"] + (["D"] if i + 1 < r and i < 2 else [])
    else:
        ops.append(b"T" * r)
    reads = [blocker(BB, {pos}), cols(BB, e - 10, ops)]
    for j in range(many):                              # reads of one base and a trailing T: a dead zone each
        reads.append(cols(BB, 2 + j % 50, ["M", b"T"]))
    return _t(reads)


def dead():
    """Condition (4) under P64: a read ends at e behind a trailing run of r = 1, 3, 40; the only open position at e + r + 1
    (refused) and at e + r + 2 (taken); r = 3 also with the run interrupted by two deletions.  Then 256 reads with
    trailing runs (zones kept: two pieces) and 257 (one piece)."""
    out = []
    for r, e in ((1, 70), (3, 70), (40, 100)):
        out.append((f"dead{r}_inside", _dead_target(r, e, e + r + 1), P64, dict(merge=[])))
        out.append((f"dead{r}_behind", _dead_target(r, e, e + r + 2), P64, dict(merge=[e + r + 2])))
    out.append(("dead3_tdels_inside", _dead_target(3, 70, 74, tdels=True), P64, dict(merge=[])))
    out.append(("dead3_tdels_behind", _dead_target(3, 70, 75, tdels=True), P64, dict(merge=[75])))
    out.append(("dead_256", _dead_target(1, 60, 80, many=255), P64, dict(merge=[80])))
    out.append(("dead_257", _dead_target(1, 60, 80, many=256), P64, dict(merge=[])))
    return out


def _starts_target(variant, many=0):
    p = 96                                             # the last position of P64's first window, inside bestPath's fifth
    if variant.startswith("ins"):                      # reads through v go on to bb(p + 1)
        reads = [blocker(BB, {p, p + 1})]
        s = p + 1 if variant == "ins_at" else p + 2
        reads.append(plain(BB, s, s + 20, lead=BB[p - 1:p] if variant == "ins_at" else b"T"))
    else:                                              # reads through v delete p + 1: (p, q) = (96, 98)
        reads = [blocker(BB, {p, p + 2}, dele={p + 1})]
        s = {"del_inside": p + 1, "del_at_q": p + 2, "del_behind_q": p + 3}[variant]
        reads.append(plain(BB, s, s + 20))
    for j in range(many):                              # reads of one base in front of the window
        reads.append(cols(BB, 2 + j % 50, ["M"]))
    return _t(reads)


def starts():
    """Condition (5) under P64, v = bb(96).  ins_at: the seeds' situation, a read starts at 97 behind a leading insertion of
    v's base (refused; at 98: taken).  del_*: every read through v deletes 97, a read starts at 97 (inside the stretch)
    and at 98 (at q): refused; at 99: taken.  bestPath's row has no condition (5) and takes 96 every time.  Then 2,048
    reads (in pieces) and 2,049 (DG_CUT_STARTS: one piece)."""
    out = []
    for v, m in (("ins_at", []), ("ins_behind", [96]), ("del_inside", []), ("del_at_q", []), ("del_behind_q", [96])):
        out.append((f"starts_{v}", _starts_target(v), P64, dict(merge=m, bp_has=96)))
    out.append(("starts_2048", _starts_target("ins_behind", many=2046), P64, dict(merge=[96])))
    out.append(("starts_2049", _starts_target("ins_behind", many=2047), P64, dict(merge=[])))
    return out


LW = 1200                                              # the long window: 1200 bases in 4 pieces, windows of 150
PLONG = dict(max_segments=64, min_segment_len=300)


def window():
    """The window is searched 64 positions a round.  1,200 bases under PLONG: want = 4, ideal positions 301, 601, 901,
    span 150.  The only open position of the first window at offsets 0, 63, 64, 149 (= span - 1: taken) and 150 (= span:
    not found, the piece is skipped and the row is one short).  The clamps of `want`: by blen / seg_min (PLONG), by
    seg_max (max_segments 3 at min_segment_len 4) and by 64 (max_segments 64 at min_segment_len 4: pieces of 18, windows
    of 9; the last ideal position, 1 + 63 * 1200 / 64 = 1182, has a window that ends at 1190 <= blen: p0 + span - 1 <= blen - blen / want / 2, so no
    window can pass blen and `pos <= blen` never decides)."""
    bb = alternating(LW)
    out = []
    for off in (0, 63, 64, 149, 150):
        tg = target_of(bb, [blocker(bb, {301 + off, 700, 1000, 1185}), plain(bb, 20, 60, lead=b"T")])
        out.append((f"window_off{off}", tg, PLONG, dict(merge=([301 + off] if off < 150 else []) + [700, 1000])))
    tg = out[0][1]
    out.append(("window_segmax", tg, dict(max_segments=3, min_segment_len=4), dict(merge=[1000], want=3)))
    out.append(("window_64", tg, dict(max_segments=64, min_segment_len=4), dict(merge=[301, 700, 1000, 1185], want=64)))
    return out


def shared():
    """DG_SH_MAX under P64, cuts at 80, 140, 210.  n letters, each the leading insertion of a read that starts in the first
    piece (bases 20, 22, ..) and of one that starts in the second (100, 102, ..): mergeOutNodes(enter) unites each pair
    into one prologue vertex with out-edges into two pieces.  Seven of them (8 lists with enter's): pieces kept.  Eight:
    the second attempt gives the target as one piece, and bestPath's row keeps its pieces.  shared_on_cut: one letter,
    the second read starts on the cut position itself (a vertex of the piece behind: `s_cut[c] <= d`)."""
    from bestpath_cases import LETTERS
    out = []
    for n in (7, 8):
        reads = [blocker(BB, {80, 140, 210})]
        for i in range(n):
            reads += [plain(BB, 20 + 2 * i, 23 + 2 * i, lead=LETTERS[i:i + 1]), plain(BB, 100 + 2 * i, 103 + 2 * i, lead=LETTERS[i:i + 1])]
        out.append((f"shared{n}", _t(reads), P64, dict(merge=[80, 140, 210], nshared=n + 1, nseg=4 if n == 7 else 1)))
    reads = [blocker(BB, {80, 140, 210}), plain(BB, 20, 23, lead=b"T"), plain(BB, 80, 83, lead=b"T")]
    out.append(("shared_on_cut", _t(reads), P64, dict(merge=[80, 140, 210], nshared=2, nseg=4)))
    return out


SLOT_SITES = tuple(10 + 4 * j for j in range(17))      # 10 .. 74: in front of the first cut (80) under P64


def slots():
    """DG_E_LOG_OVF under P64 (sh_log = 16 slots a segment behind a shared list), cut at 80.  in[exit]: at each of n sites p a
    read matches p, inserts T and matches p + 1, and a second one matches p and ends in a trailing T: mergeOutNodes(bb(p))
    unites the two T and the survivor gains an edge to exit, an append to in[exit] by the first piece's worker.
    out[enter]: the twin, a read matches q - 1, inserts a letter and matches q, and a second one begins with that letter
    in front of q (a letter per site: mergeOutNodes(enter) must leave them apart); mergeInNodes(bb(q)) moves enter's edge
    to the survivor, an append to out[enter].  n = 16 (no re-run) and 17 (one more)."""
    from bestpath_cases import LETTERS
    out = []
    for n in (16, 17):
        reads = [blocker(BB, {80})]
        for p in SLOT_SITES[:n]:
            reads += [cols(BB, p, ["M", b"T", "M"]), cols(BB, p, ["M", b"T"])]
        out.append((f"slots_in{n}", _t(reads), P64, dict(merge=[80], appends=("in", n))))
        reads = [blocker(BB, {80})]
        for j, p in enumerate(SLOT_SITES[:n]):
            x = LETTERS[j:j + 1]
            reads += [cols(BB, p, ["M", x, "M"]), cols(BB, p + 1, [x, "M"])]
        out.append((f"slots_out{n}", _t(reads), P64, dict(merge=[80], appends=("out", n))))
    return out


def defer():
    """DG_DEFER_MAX under P64: no merge cut (nothing open in the merge's windows), one bestPath cut at 100 (windows of 11 from
    94).  n chains of 8 inserted letters (the first letters differ), each the leading run of a read that starts at base
    30 + 2i and of one that starts at 110 + 2i: united by mergeOutNodes(enter) and its successors' visits, all of the
    prologue's (maxlead = 8), the last vertex of a chain with successors in both bestPath pieces, the other seven its
    ancestors.  defer63: seven chains and one of seven letters: 63 beside enter, kept.  defer64: eight chains: overflow,
    defer[0] = 0xFFFFFFFF."""
    from bestpath_cases import LETTERS
    out = []
    for name, lens in (("defer63", [8] * 7 + [7]), ("defer64", [8] * 8)):
        reads = [blocker(BB, {100})]
        for i, k in enumerate(lens):
            chain = LETTERS[i:i + 1] + LETTERS[20:20 + k - 1]
            reads += [plain(BB, 30 + 2 * i, 33 + 2 * i, lead=chain), plain(BB, 110 + 2 * i, 113 + 2 * i, lead=chain)]
        out.append((name, _t(reads), P64, dict(merge=[], bp=[100], defer=64 if name == "defer63" else None)))
    return out


def fullspan():
    """Full-span pileups for the partial-span kernels (DAGCON_GCUTS=1): every lead and trail zero, every start 1.  The
    blocker leaves every fourth base open (1, 5, 9, ..), two reads match everything: every window of P64 (32 wide) and of
    min_segment_len 4 (two wide, from 1 + 4 s) holds a base that condition (1) admits, so the row has `want` pieces."""
    reads = [blocker(BB, set(range(1, L + 1, 4))), plain(BB, 1, L), plain(BB, 1, L)]
    return [("fullspan", _t(reads), P64, dict(full=True))]


FAMILIES = dict(covers=covers, lead=lead, tiny=tiny, dead=dead, starts=starts, window=window, shared=shared, slots=slots,
                defer=defer, fullspan=fullspan)
# every family is also run at these settings (Cuts predicts the rows; nothing else is asserted of them there)
SETTINGS = (dict(max_segments=64, min_segment_len=4), P64, PLONG, dict())
BP_SEGS = 3                                            # DAGCON_BP_SEGS for the consensus runs: bestPath's pieces differ


class Case:
    """One target as a batch of its own."""

    def __init__(self, name, target, pieces, expect):
        self.name, self.target, self.pieces, self.expect = name, target, pieces, expect
        self.targets = [target]
        self.batch = batch_from_targets(self.targets)
        assert host_full_span(target) == bool(expect and expect.get("full")), name

    @functools.cached_property
    def pile(self):
        return Pile(self.target)

    @functools.lru_cache(maxsize=None)
    def cuts(self, max_segments=0, min_segment_len=0, bp_segs=None, mut=()):
        return Cuts(self.pile, plan(max_segments, min_segment_len, bp_segs), mut)

    @functools.cached_property
    def graphs(self):
        from test_gpu_parity import _oracle_graph
        return [_oracle_graph(self.batch, 0, 0, 0, True)]

    @functools.cached_property
    def consensus(self):
        return [oracle_batch(self.batch, **o) for o in CNS_OPTS]


@functools.lru_cache(maxsize=None)
def family(name):
    return [Case(*c) for c in FAMILIES[name]()]


MIXED = ("covers", "lead7_above", "tiny2", "dead3_behind", "starts_ins_at", "starts_del_behind_q", "dead40_inside",
         "tiny5", "lead1_at_pmin")


@functools.lru_cache(maxsize=None)
def mixed():
    """One batch of several families' targets: worklist rows and wl_first of different targets side by side."""
    by_name = {c.name: c for f in FAMILIES if f != "fullspan" for c in family(f)}
    cases = [by_name[n] for n in MIXED]
    return cases, batch_from_targets([c.target for c in cases])
