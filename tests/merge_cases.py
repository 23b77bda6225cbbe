"""Pileups that cross the fixed-size limits of the mergeNodes sweeps on purpose, for tests/test_merge_limits.py.

The three sweeps (k_merge, k_merge_q and the partial-span dg_merge_segment<true>) keep a few fixed-size structures and
a second code path behind each: 48 frames of the mergeInNodes recursion in LDS (DG_IN_STACK, in dg_visit_merging: one
text for all three), then the single-lane literal path; the youngest 256 / 16 queue entries in LDS (DG_QRING /
DQ_RING), then the queue in memory;
a row of 8 lanes (4 + 4 on its one-look path) and a wave of 64 (32 + 32 on its one-look path) as list widths, then
the literal path; stk_words of scratch, then DG_E_STACK and a re-run; and the host's span rule, which takes a batch
for full-span on (start == 1, columns >= target bases) alone.  Random pileups at the depths and run lengths the other
tests use never, or almost never, reach the paths behind them; the families here are built to.

Every constructed alignment is a backbone over AC with inserted bases that are neither A nor C, so oracle.normalize_gaps
returns it unchanged (asserted: the properties below are read off the strings).  The `depths` family alone is drawn
with util.random_target and is normalized like any other random input.

Measure is oracle.pymodel.AlnGraph with counters: what a family reaches is asserted on that model, on the CPU.  The
oracle's graphs and consensus of a case are cached here, per process: CPU preconditions and GPU tests share them.
"""
import functools
import itertools
import sys

import numpy as np

import oracle
from oracle import pymodel
from util import batch_from_targets, oracle_batch, random_target

GAP = 0x2D
OTHER = {ord("G"): ord("T"), ord("T"): ord("G")}


# ---- the model, with counters -----------------------------------------------------------------------------------------

class Measure(pymodel.AlnGraph):
    """AlnGraph whose mergeNodes counts: depth (deepest merge_in frame, the visit's own frame = 1), deep_groups (groups
    of two or more merged in frames deeper than 48), top_multi (depth-1 frames that merge two or more groups), in_len /
    out_len (the longest in / out list in which a group was merged), in_lens / out_lens (every such length), occupancy
    (the most entries the FIFO holds when a vertex is taken off it, that vertex included)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.depth = self.deep_groups = self.top_multi = self.occupancy = 0
        self.in_lens, self.out_lens = set(), set()
        self._d = 0

    def merge_in(self, n):
        self._d += 1
        self.depth = max(self.depth, self._d)
        d = self._d
        groups = {}
        for e in self.nodes[n].inn:
            if len(self.nodes[e.src].out) == 1:
                groups.setdefault(self.nodes[e.src].base, []).append(e.src)
        if sum(len(v) > 1 for v in groups.values()) >= 2 and d == 1:
            self.top_multi += 1
        for base in sorted(groups):
            nodes = groups[base]
            if len(nodes) <= 1:
                continue
            self.in_lens.add(len(self.nodes[n].inn))
            if d > 48:
                self.deep_groups += 1
            an = nodes[0]
            for ni in nodes[1:]:
                self.nodes[an].out[0].count += self.nodes[ni].out[0].count
                self.nodes[an].weight += self.nodes[ni].weight
            for v in nodes[1:]:
                for ie in list(self.nodes[v].inn):
                    e = self._find_edge(ie.src, an)
                    if e is not None:
                        e.count += ie.count
                    else:
                        ne = self._add_edge(ie.src, an)
                        ne.count, ne.visited = ie.count, ie.visited
                self._reap(v)
            self.merge_in(an)
            self._d = d
        self._d = d - 1

    def merge_out(self, n):
        groups = {}
        for e in self.nodes[n].out:
            if len(self.nodes[e.dst].inn) == 1:
                groups.setdefault(self.nodes[e.dst].base, []).append(e.dst)
        for base in sorted(groups):
            if len(groups[base]) > 1:
                self.out_lens.add(len(self.nodes[n].out))
        super().merge_out(n)

    def merge_nodes(self):
        queue, head = [self.enter], 0
        while head < len(queue):
            self.occupancy = max(self.occupancy, len(queue) - head)
            u = queue[head]
            head += 1
            self.merge_in(u)
            self.merge_out(u)
            for e in self.nodes[u].out:
                e.visited = True
                if all(x.visited for x in self.nodes[e.dst].inn):
                    queue.append(e.dst)
        return queue

    @property
    def in_len(self):
        return max(self.in_lens, default=0)

    @property
    def out_len(self):
        return max(self.out_lens, default=0)

    def figures(self):
        return dict(depth=self.depth, deep_groups=self.deep_groups, top_multi=self.top_multi, in_len=self.in_len,
                    out_len=self.out_len, occupancy=self.occupancy)


def measure(target):
    """The counters of one target (tlen, alns, backbone) after mergeNodes on the model, and its adjacency."""
    tlen, alns, _ = target
    g = Measure(blen=tlen)
    for s, q, t in alns:
        qn, tn = pymodel.normalize_gaps(q.decode(), t.decode())
        g.add_aln(s, qn, tn)
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 20000))
    try:
        g.merge_nodes()
    finally:
        sys.setrecursionlimit(old)
    return g


# ---- building blocks ---------------------------------------------------------------------------------------------------

def backbone(n, seed=5):
    """n bases over AC."""
    return bytes(b"AC"[i] for i in np.random.default_rng(seed).integers(0, 2, n))


def gt(n, seed):
    """n bases over GT."""
    return bytes(b"GT"[i] for i in np.random.default_rng(seed).integers(0, 2, n))


def ins_read(bb, runs):
    """The backbone with the run runs[p] inserted behind its first p bases (p = 0: leading, p = len(bb): trailing),
    full span: (1, q, t)."""
    q, t = bytearray(), bytearray()
    for p in range(len(bb) + 1):
        r = runs.get(p, b"")
        q += r
        t += bytes([GAP]) * len(r)
        if p < len(bb):
            q.append(bb[p]); t.append(bb[p])
    return 1, bytes(q), bytes(t)


def target_of(bb, alns):
    for s, q, t in alns:
        assert len(q) == len(t)
        assert oracle.normalize_gaps(q, t) == (q, t), "a constructed alignment must be normalized already"
    return len(bb), alns, bb


def host_full_span(target):
    """The host's rule (dagcon_upload): every read starts at 1 and has a column for every target base."""
    tlen, alns, _ = target
    return all(s == 1 and len(q) >= tlen for s, q, _ in alns)


def last_base(aln):
    """The last target base (1-based) a read has a column for."""
    s, _, t = aln
    return s - 1 + sum(c != GAP for c in t)


# ---- the families ------------------------------------------------------------------------------------------------------

S_DEEP = gt(59, 11) + b"G"           # the shared run suffix of `deep`: 60 bases over GT, ending in G


def deep(tlen=20, p=10):
    """mergeInNodes 61 frames deep behind base p, the hand-over at frame 48 with work left in the frames it re-evaluates.
    GGT+S and TTG+S differ from their first base on, so mergeOutNodes leaves them alone and mergeInNodes of the vertex
    behind the runs unites S base by base, one frame each.  Three five-base runs that end in T give the top frame a
    second group (T) that waits while the G group goes deep.  Two runs that join S 50 bases before its end, behind one
    and two bases of the letter S does not have there, give frame 51 a second group of its own.  Two clean reads."""
    bb = backbone(tlen)
    c = bytes([OTHER[S_DEEP[-51]]])
    runs = [b"GGT" + S_DEEP, b"TTG" + S_DEEP, b"GTGTT", b"TGTTT", b"TTTTT", c + S_DEEP[-50:], c + c + S_DEEP[-50:]]
    return target_of(bb, [ins_read(bb, {p: r}) for r in runs] + [ins_read(bb, {}), ins_read(bb, {})])


S_STACK = gt(1000, 12)


def stack(shared=True, tlen=20, p=10):
    """Two runs of 1002 bases that share their last 1000 (recursion 1001 deep: some 950 literal frames of 7 words, more
    than the 4096 words of a small batch), or, the control, two runs as long that share nothing (the other one is
    S with G and T exchanged).  Two clean reads."""
    bb = backbone(tlen)
    other = S_STACK if shared else bytes(OTHER[c] for c in S_STACK)
    runs = [b"GG" + S_STACK, b"TT" + other]
    return target_of(bb, [ins_read(bb, {p: r}) for r in runs] + [ins_read(bb, {}), ins_read(bb, {})])


LETTERS20 = b"BDEFGHIJKLMNOPQRSTUV"


def fan(letters, levels, tlen=24, p=12):
    """A read per word of letters^levels, inserted behind base p: len(letters)^levels reads, every branch of equal weight
    (bestPath's choice among them is decided by list order alone)."""
    bb = backbone(tlen)
    return target_of(bb, [ins_read(bb, {p: bytes(w)}) for w in itertools.product(letters, repeat=levels)])


FANS = {"fan32": (b"GT", 5), "fan27": (b"GTN", 3), "fan512": (b"GT", 9), "fan400": (LETTERS20, 2)}
FAN_RING = {"fan32": 16, "fan27": 16, "fan512": 256, "fan400": 256}      # the ring its occupancy must pass

# rows: 4 + 4 one look, 8 in dg_visit_merging (DgRow::IN_W and W); waves: 32 + 32 one look and DgWave::IN_W, 64 out
WIDTHS = (4, 5, 8, 9, 32, 33, 64, 65)


def width_out(L):
    """An out list of exactly L entries with groups in it: L - 1 reads insert GT or TG behind base p.  The vertex of base p
    then has the backbone edge and L - 1 first inserted bases in its out list (groups G and T, one group G where L = 4);
    the survivors leave no group on the in side."""
    bb = backbone(24)
    k = L - 1
    runs = [b"GT"] * k if k < 4 else [b"GT"] * (k // 2) + [b"TG"] * (k - k // 2)
    return target_of(bb, [ins_read(bb, {12: r}) for r in runs])


def width_in(L):
    """An in list of exactly L entries with groups in it: read i of L - 1 leaves the backbone i bases before base p (deleting
    them), inserts G or T and comes back at base p + 1.  The inserted vertices hang on L - 1 different backbone vertices,
    so mergeOutNodes never sees two of them together; the vertex of base p + 1 has the backbone edge and all of them in
    its in list."""
    p = L + 2
    bb = backbone(p + 8)
    k = L - 1
    alns = []
    for i in range(k):
        x = b"G" if k < 4 or i < k // 2 else b"T"
        q = bb[:p - i] + bytes([GAP]) * i + x + bb[p:]
        t = bb[:p] + bytes([GAP]) + bb[p:]
        alns.append((1, q, t))
    return target_of(bb, alns)


def _true_reads(bb, n=6):
    """n full-span reads that insert G, T, GT or nothing behind the same ten bases, in rotation: merge groups on both sides
    of those bases, some of them where the pretenders below leave or rejoin the backbone."""
    sites = (9, 25, 30, 31, 45, 59, 60, 70, 90, 110)
    out = []
    for r in range(n):
        runs = {}
        for j, p in enumerate(sites):
            x = (b"G", b"T", b"GT", b"")[(r + j) % 4]
            if x:
                runs[p] = x
        out.append(ins_read(bb, runs))
    return out


def span_pretenders():
    """Four targets of 120 bases under six true full-span reads and reads that only pass for full-span (start 1, at least
    120 columns): (a) ends at base 70 behind a 60-base trailing run; (b) ends at base 60 and carries a 70-base run behind
    base 30; (c) deletes the first 30 bases, so it enters the backbone at base 31, and inserts later; the last target has
    all three and a second (a) that ends at base 65 and shares the last 30 bases of its run with the first."""
    tlen = 120
    r60, r70 = gt(60, 21), gt(70, 22)

    def a(bb, end=70, run=r60):
        return 1, bb[:end] + run, bb[:end] + bytes([GAP]) * len(run)

    def b(bb):
        return 1, bb[:30] + r70 + bb[30:60], bb[:30] + bytes([GAP]) * 70 + bb[30:60]

    def c(bb):
        _, q, t = ins_read(bb[30:], {0: b"G", 17: b"TG", 55: b"T"})
        return 1, bytes([GAP]) * 30 + q, bb[:30] + t

    out = []
    for i, kinds in enumerate(("a", "b", "ac", "abcA")):
        bb = backbone(tlen, seed=30 + i)
        alns = _true_reads(bb)
        for k in kinds:
            alns.append({"a": a, "b": b, "c": c, "A": lambda x: a(x, 65, b"T" + gt(29, 23) + r60[-30:])}[k](bb))
        tg = target_of(bb, alns)
        assert host_full_span(tg) and any(last_base(x) < tlen - 20 for x in alns[6:])
        out.append(tg)
    return out


def span_partial():
    """Two targets of 120 bases under eight reads that start at bases 5 to 40 and run to the end; they insert G, T, GT, TT or
    nothing behind the same seven bases, in rotation, and every third read starts with an inserted G."""
    sites = (44, 50, 63, 64, 80, 100, 118)
    out = []
    for i in range(2):
        bb = backbone(120, seed=40 + i)
        alns = []
        for r in range(8):
            s = 5 + 5 * r
            runs = {0: b"G"} if r % 3 == 0 else {}
            for j, p in enumerate(sites):
                x = (b"G", b"T", b"GT", b"TT", b"")[(r + j + i) % 5]
                if x:
                    runs[p - (s - 1)] = x
            _, q, t = ins_read(bb[s - 1:], runs)
            alns.append((s, q, t))
        tg = target_of(bb, alns)
        assert not host_full_span(tg)
        out.append(tg)
    return out


DEPTHS = (41, 45, 50, 53, 54, 58, 61, 64, 65, 67, 69, 70)


def depths():
    """Twelve random full-span pileups of 20 to 100 bases at 41 to 70 reads, alphabets AC / ACGT / A in rotation."""
    rng = np.random.default_rng(8)
    out = []
    for i, k in enumerate(DEPTHS):
        tl = int(rng.integers(20, 101))
        alns, bb = random_target(rng, tl, k, alphabet=[b"AC", b"ACGT", b"A"][i % 3], sub=0.05, ins=0.15, dele=0.08,
                                 full_span=True)
        out.append((tl, alns, bb))
    return out


def slide(make, tlen=24, points=None):
    """One target per insertion point: 0 (a leading run: the chains hang on enter), every base, tlen (a trailing run)."""
    return [make(tlen=tlen, p=p) for p in (range(tlen + 1) if points is None else points)]


# ---- the cases: a batch each, the oracle's answers cached ---------------------------------------------------------------

def _targets(name):
    if name == "deep":
        return slide(deep)
    if name in ("fan32", "fan27"):
        return slide(lambda tlen, p: fan(*FANS[name], tlen=tlen, p=p))
    if name in ("fan512", "fan400"):
        return slide(lambda tlen, p: fan(*FANS[name], tlen=tlen, p=p), points=(0, 12, 24))
    if name == "widths":
        return [f(L) for L in WIDTHS for f in (width_in, width_out)]
    if name == "stack":
        return [stack(True)]
    if name == "stack_control":
        return [stack(False)]
    if name == "span":
        return span_pretenders()
    if name == "partial":
        return span_partial()
    if name == "depths":
        return depths()
    raise KeyError(name)


SWEPT = ("deep", "fan32", "fan27", "fan512", "fan400", "widths", "depths")    # through every kernel at both piece settings
ALL = SWEPT + ("stack", "stack_control", "span", "partial")
GRAPH_OPTS = dict(min_cov=0, min_len=0, trim=0, min_weight=0)
CNS_OPTS = (GRAPH_OPTS, dict(min_cov=0, min_len=0, trim=2, min_weight=1))


class Case:
    def __init__(self, name):
        self.name = name
        self.targets = _targets(name)
        self.batch = batch_from_targets(self.targets)
        self.full_span = all(host_full_span(t) for t in self.targets)

    @functools.cached_property
    def measured(self):
        return [measure(t) for t in self.targets]

    @functools.cached_property
    def graphs(self):
        """_oracle_graph of every target after mergeNodes, for _check_graphs."""
        from test_gpu_parity import _oracle_graph
        return [_oracle_graph(self.batch, t, 0, 0, True) for t in range(self.batch.n_targets)]

    @functools.cached_property
    def consensus(self):
        """The oracle's consensus under each of CNS_OPTS."""
        return [oracle_batch(self.batch, **o) for o in CNS_OPTS]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
