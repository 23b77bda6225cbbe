"""Pileups that cross the fixed-size limits of the bestPath sweeps on purpose, for tests/test_bestpath_limits.py.

bestPath (pbdagcon_amd/csrc/k_bestpath.hip.h) keeps as many fixed-size structures as the merge does, with a second code
path behind each: six out-edges in a staged LDS slot (DG_BOUT), then the pool; 64 edges a round of a wave, then the first
maximum carried into the next round; eight out-edges and 16 stack entries a row (DG_BRW, DG_BL_STK), then the piece is
given up and a wave does it over; 64 evaluation-stack entries in LDS (DG_BSTK), then the gstk scratch; a successor more
than 192 ids below the stream makes a vertex wait (DG_BFAR), 32 waiters at most (DG_BDEF), then the far successor is
chased after all; score rings of 256 and 32 ids, chunks of 64, 8 held-back results (DG_SR, DG_BRR, DG_BR, DG_BRP); the
walk's ring of 256, its prefetch of 192 and the 512-id jump of k_bp_walk_g's first piece (DG_WR); 256 pieces a target,
64 on the partial-span path (DG_BP_PIECES).  The families here are built to cross each of them from both sides.

Every constructed alignment is a backbone over AC with inserted bases that are neither A nor C, so oracle.normalize_gaps
returns it unchanged (asserted by merge_cases.target_of).  `widths` deletes the base behind its insertion site in every
read; its backbone alternates A and C so that the deleted base differs from the one behind it and the gap stays put.

Sweep is the schedule of the device's sweeps restated in plain Python, over the oracle's merged graph in device ids: what a
family reaches is asserted on it, on the CPU.  It says how vertices are scheduled and nothing about scores: the best
path, the consensus, the support and the positions a device run is held to are the oracle's, never Sweep's.

Not reached, and why.  DG_E_STACK raised by bestPath (a chase deeper than DG_BSTK + stk_words = 64 + 4096 entries): a
chase runs over vertices the stream has not reached, all of them inserted vertices of one backbone position (an edge
never leads to a lower position), along graph edges, so it is at most as long as the longest insertion run there.  The
edge it starts with was turned around by mergeInNodes, whose recursion united the run's suffix with another read's,
one frame a base: a chase of n entries takes a recursion n frames deep, and the merge's literal frames behind frame 48
cost 7 words of the same scratch against bestPath's one.  The merge raises DG_E_STACK at some 630 shared bases
(merge_cases.stack), the host grows stk_words by four and runs the batch again, and bestPath finds 16384 words and more.
One construction was tried for a chase that is a chain of many short merges under a full wait list (the 34 reads of
`waiters`, then 8 whose runs share ever shorter suffixes with the first: `nested`): every chase ends where its own shared suffix
ends, so the deepest is the longest single recursion again (max_sp 201 against merge_cases.Measure's depth 201, as in
`waiters`).  mergeOutNodes turns no edge around here: it keeps the first vertex of the out list, which is the lowest id.
No input was found that reaches it.
DG_DEFER_MAX and DG_SH_MAX are out of scope here: they need a model of k_merge_pro's prologue.
"""
import functools

import numpy as np

import oracle
from merge_cases import CNS_OPTS, GAP, GRAPH_OPTS, backbone, gt, host_full_span, ins_read, slide, target_of
from util import batch_from_targets, oracle_batch

# the device's constants, restated (k_bestpath.hip.h)
DG_BOUT, DG_BRW, DG_BL_STK, DG_BSTK, DG_BDEF, DG_BFAR = 6, 8, 16, 64, 32, 192
DG_SR, DG_BR, DG_BRR, DG_BRP, DG_WR = 256, 64, 32, 8, 256
STK_WORDS = 4096

# one-letter insertions that differ from each other and from every base and gap byte: printable, outside ACGTNacgtn-.
# and outside the bases of the enter and exit vertices; the first 69 in byte order (merge_cases.LETTERS20 has G, T and N)
LETTERS = bytes(b for b in range(33, 127) if b not in b"ACGTNacgtn-.^$")[:69]


# ---- the model: the sweeps' schedule over the merged graph in device ids -------------------------------------------------

class Sweep:
    """The merged graph of one target in device ids (out[v]: the out list of v in list order, None for a vertex the merge
    deleted) and what the sweeps do with it as one piece.

    Read off the graph: max_out (the longest out list), turned (edges whose destination id is below their source),
    reach_fwd / reach_back (the largest id distance of a forward / a turned-around edge), path_jumps (the id distances
    along the oracle's best path, which is given, not computed here).

    pure_chase(): a row.  The stream runs down the live vertices; a vertex with an unscored successor goes onto the stack
    and the first such successor is scored first.  chase_depth: the most entries on the stack (DG_BL_STK of them fit).

    wave(): a wave.  The stream's vertex is the bottom of the stack (sp = 1).  A round of 64 edges with unscored
    successors: if one of them lies more than DG_BFAR ids below the stream's vertex and waiting + sp <= DG_BDEF, the whole
    stack waits (the top for that successor, every entry under it for the one above) and the stream goes on; otherwise all
    of the round's unscored successors are pushed.  A vertex that gets its score wakes those that wait for it onto the
    stack.  max_sp: the largest sp (entries 2 .. sp live in S.stk, sp - 1 of them: the first entry in gstk is at
    sp == DG_BSTK + 2); max_waiting; parked: the times a stack was put on the wait list; full_chase: far misses that were
    chased because the list was full."""

    def __init__(self, adj, o2d, path):
        n = len(adj)
        self.n = n
        self.out = [None] * n
        for o, (_, _, _, dead, oe, _) in enumerate(adj):
            if not dead:
                self.out[o2d[o]] = [o2d[d] for d, _ in oe]
        live = [v for v in range(n) if self.out[v] is not None]
        self.live = len(live)
        self.max_out = max(len(self.out[v]) for v in live)
        self.turned = [(v, d) for v in live for d in self.out[v] if d < v]
        self.reach_fwd = max((d - v for v in live for d in self.out[v] if d > v), default=0)
        self.reach_back = max((v - d for v, d in self.turned), default=0)
        self.path = [o2d[o] for o in path]
        self.path_jumps = [b - a for a, b in zip(self.path, self.path[1:])]
        self.pure_chase()
        self.wave()

    def choice(self, v):
        """The index, in v's out list, of the edge the oracle's best path takes at v."""
        i = self.path.index(v)
        return self.out[v].index(self.path[i + 1])

    def pure_chase(self):
        scored = bytearray(self.n)
        depth = 0
        for v in range(self.n - 1, -1, -1):
            if self.out[v] is None or scored[v]:
                continue
            stack, n = [], v
            while True:
                if not scored[n]:
                    miss = next((d for d in self.out[n] if not scored[d]), None)
                    if miss is not None:
                        stack.append(n)
                        depth = max(depth, len(stack))
                        n = miss
                        continue
                    scored[n] = 1
                if not stack:
                    break
                n = stack.pop()
        assert all(scored[v] for v in range(self.n) if self.out[v] is not None)
        self.chase_depth = depth

    def wave(self):
        scored = bytearray(self.n)
        waiting = []                                  # (who, for whom)
        self.max_sp = self.max_waiting = self.parked = self.full_chase = 0
        for v in range(self.n - 1, -1, -1):
            if self.out[v] is None or scored[v]:
                continue
            stack = [v]
            while stack:
                self.max_sp = max(self.max_sp, len(stack))
                n = stack[-1]
                if scored[n]:
                    stack.pop()
                    continue
                again = False
                for e0 in range(0, len(self.out[n]), 64):
                    miss = [d for d in self.out[n][e0:e0 + 64] if not scored[d]]
                    if not miss:
                        continue
                    far = [d for d in miss if d < v - DG_BFAR]
                    if far and len(waiting) + len(stack) <= DG_BDEF:
                        above = far[0]
                        for who in reversed(stack):
                            waiting.append((who, above))
                            above = who
                        self.parked += 1
                        self.max_waiting = max(self.max_waiting, len(waiting))
                        stack = []
                    else:
                        self.full_chase += bool(far)
                        stack.extend(miss)
                    again = True
                    break
                if again:
                    continue
                scored[n] = 1
                stack.pop()
                woken = [w for w, b in waiting if b == n]
                if woken:
                    waiting = [(w, b) for w, b in waiting if b != n]
                    stack = (stack or [v]) + woken    # (the finished stream vertex stays the bottom)
        assert not waiting, "somebody still waits"
        assert all(scored[v] for v in range(self.n) if self.out[v] is not None)

    def figures(self):
        return dict(live=self.live, max_out=self.max_out, turned=len(self.turned), reach_fwd=self.reach_fwd,
                    reach_back=self.reach_back, chase_depth=self.chase_depth, max_sp=self.max_sp,
                    max_waiting=self.max_waiting, parked=self.parked, full_chase=self.full_chase)


# ---- the families ------------------------------------------------------------------------------------------------------

S_LONG = gt(200, 14)                       # the shared run of `suffix` and `waiters`: 200 bases over GT

SUFFIX_L = (14, 15, 16, 17, 18, 62, 63, 64, 65, 66, 189, 190, 191, 192, 193, 194)
SUFFIX_POINTS = (0, 9, 10, 11, 12, 20)


def suffix(L, tlen=20, p=10):
    """Two runs GG + S[:L] and TT + S[:L] behind base p, two clean reads: mergeInNodes unites S, and the second T keeps an
    edge to the first read's S[0], L + 1 ids below it."""
    bb = backbone(tlen)
    runs = [b"GG" + S_LONG[:L], b"TT" + S_LONG[:L]]
    return target_of(bb, [ins_read(bb, {p: r}) for r in runs] + [ins_read(bb, {}), ins_read(bb, {})])


WAITERS_K = (31, 32, 33, 34, 40)
WAITERS_POINTS = (0, 10, 12, 20)


def waiters(K, tlen=20, p=10):
    """K reads insert letter_r + S behind base p (200 bases shared, K different first letters), two clean reads: every
    read from the second on keeps an edge from its letter far back into the first read's chain."""
    bb = backbone(tlen)
    return target_of(bb, [ins_read(bb, {p: LETTERS[r:r + 1] + S_LONG}) for r in range(K)]
                     + [ins_read(bb, {}), ins_read(bb, {})])


def alternating(n):
    return bytes(b"AC"[i & 1] for i in range(n))


def width(W, heavy, d, tlen=20, p=10):
    """W - 1 different one-letter insertions behind base p, a read each, in list order; every read deletes base p + 1
    (where there is one).  The vertex of base p then has the backbone edge at index 0 and the letters at 1 .. W - 1.
    heavy: list indices whose letters get d reads in all (the extra reads come last, in the order of `heavy`)."""
    bb = alternating(tlen)

    def read(i):
        _, q, t = ins_read(bb, {p: LETTERS[i - 1:i]})
        if p < tlen:
            q = bytearray(q)
            q[p + 1] = GAP                      # (column p is the letter, column p + 1 the base behind it)
            q = bytes(q)
        return 1, q, t

    order = list(range(1, W)) + [i for _ in range(d - 1) for i in heavy]
    return target_of(bb, [read(i) for i in order])


def d_single(W):
    """Reads of one heavy letter among W - 2 single ones, K = W - 2 + d in all, that beat the backbone edge: a letter with c
    reads is worth 2c - K on top of the score behind the site, the backbone edge -10 - K / 2 (a backbone vertex of
    weight 1, then an edge nobody took), so 3d > W - 22; two more than that, and at least 2 to beat the other letters."""
    return max(2, (W - 22) // 3 + 3)


def d_tie(W):
    """The same with two heavy letters, K = W - 3 + 2d: d > (W - 3) / 2 - 10."""
    return max(2, (W - 23) // 2 + 3)


def d_light(W):
    """A heavy letter that still loses to the backbone edge (W >= 64): 3d < W - 22, and d >= 2."""
    return (W - 23) // 3 - 1


def width_variants(W):
    """(heavy, d, the index that has to win at a site inside the target): a single heavy letter at index 1, W - 1 and on both
    sides of 6, 8 and 64 where the list is that long; an exact tie of two heavy letters that straddle each of those
    limits (1 and W - 1 where there is none), the extra reads in both orders: the lower index wins; W >= 64: a heavy
    letter at the last index that loses to the backbone edge at index 0, 64 or more entries before it."""
    lims = [x for x in (DG_BOUT, DG_BRW, 64) if x <= W - 1]
    singles = sorted({1, W - 1} | {i for x in lims for i in (x - 1, x)})
    out = [((i,), d_single(W), i) for i in singles]
    for a, b in ([(x - 1, x) for x in lims] or [(1, W - 1)]):
        out += [((a, b), d_tie(W), a), ((b, a), d_tie(W), a)]
    if W >= 64:
        out.append(((W - 1,), d_light(W), 0))
    return out


WIDTHS_ROW = (6, 7, 8, 9)
WIDTHS_WAVE = (64, 65, 66, 70)
WIDTH_POINTS = {"widths_row": (0, 1, 9, 10, 11, 20), "widths_wave": (0, 10, 11, 20)}


def width_specs(name):
    """(W, heavy, d, wins, p) of every target of a widths batch, in batch order.  Behind the last base there is nothing to
    delete and the edge at index 0 leads to exit, which costs nothing to enter: there the heavy letter wins even where it
    is light."""
    return [(W, heavy, d, heavy[0] if wins == 0 and p == 20 else wins, p)
            for W in (WIDTHS_ROW if name == "widths_row" else WIDTHS_WAVE)
            for heavy, d, wins in width_variants(W) for p in WIDTH_POINTS[name]]


REACH = tuple(range(31, 35)) + tuple(range(63, 67)) + tuple(range(191, 195)) + tuple(range(255, 259)) + tuple(range(511, 515))
REACH_POINTS = (0, 10, 11, 12, 20)


def reach(R, tlen=20, p=10):
    """One read inserts R bases over GT behind base p, three clean reads: the backbone edge in front of the run reaches
    R + 1 ids ahead and the best path takes it."""
    bb = backbone(tlen)
    return target_of(bb, [ins_read(bb, {p: gt(R, 100 + R)})] + [ins_read(bb, {})] * 3)


# max_segments is documented as "at most 64" (include/dagcon.h) and the planner clamps it: 128 plans 64 merge pieces and
# 192 bestPath pieces.  DG_BP_PIECES itself is reached by the automatic setting, which gives a batch of up to 32 targets
# 256 merge pieces a target and min(256, 3 * 256) bestPath pieces (64 on the partial-span path).
PIECES_CLAMPED = dict(max_segments=128, min_segment_len=4)
PIECES_AUTO = dict(max_segments=0, min_segment_len=4)


def pieces():
    """A full-span target of 1,200 bases over ACGT, no two neighbours equal, under 6 reads.  Read r has an error every 37
    bases from base 10 + 3r on: a deleted base, one or two inserted bases, a substituted base, in rotation.  No two
    bases that some read does not match are neighbours, so of the two positions k_cuts looks at for each of 255 cuts
    (1200 / 256 / 2) one is always a base every read passes: the cuts saturate.  The alignments are raw (a substitution
    is a mismatch column) and are normalized like any other input; the letters are chosen so that no gap moves."""
    rng = np.random.default_rng(17)
    bb = bytearray()
    for _ in range(1200):
        bb.append(rng.choice([b for b in b"ACGT" if not bb or b != bb[-1]]))
    alns = []
    for r in range(6):
        q, t = bytearray(), bytearray()
        for i in range(1200):                                   # base i + 1
            kind = (i // 37 + r) % 3 if i >= 9 + 3 * r and (i - 9 - 3 * r) % 37 == 0 and i < 1190 else -1
            other = [b for b in b"ACGT" if b not in (bb[i - 1], bb[i], bb[i + 1 if i + 1 < 1200 else i])]
            if kind == 0:
                q.append(GAP); t.append(bb[i])
            elif kind == 2:
                q.append(other[0]); t.append(bb[i])
            else:
                q.append(bb[i]); t.append(bb[i])
            if kind == 1:
                for _ in range(1 + (i + r) % 2):
                    q.append(other[0]); t.append(GAP)
        alns.append((1, bytes(q), bytes(t)))
    return [(1200, alns, bytes(bb))]


def unmatched_bases(target):
    """The target bases (1-based) that some read of a full-span target has no match column for, after normalization."""
    out = set()
    for s, q, t in target[1]:
        qn, tn = oracle.normalize_gaps(q, t)
        pos = s
        for a, b in zip(qn, tn):
            if b != GAP:
                if a != b:
                    out.add(pos)
                pos += 1
    return out


def nested(K=8, tlen=20, p=10):
    """The one construction tried for a chase made of many short merges (module docstring): 34 `waiters` reads fill the wait
    list, then K reads x + S[-20 * (r + 1):] share ever shorter suffixes with the first."""
    bb = backbone(tlen)
    runs = [LETTERS[r:r + 1] + S_LONG for r in range(34)]
    runs += [LETTERS[34 + r:35 + r] + S_LONG[len(S_LONG) - 20 * (r + 1):] for r in range(K)]
    return target_of(bb, [ins_read(bb, {p: r}) for r in runs] + [ins_read(bb, {}), ins_read(bb, {})])


# ---- the cases: a batch each, the oracle's answers cached ---------------------------------------------------------------

def _targets(name):
    if name == "suffix":
        return [suffix(L, p=p) for L in SUFFIX_L for p in SUFFIX_POINTS]
    if name == "waiters":
        return [waiters(K, p=p) for K in WAITERS_K for p in WAITERS_POINTS]
    if name in WIDTH_POINTS:
        return [width(W, heavy, d, p=p) for W, heavy, d, _, p in width_specs(name)]
    if name == "reach":
        return [reach(R - 1, p=p) for R in REACH for p in REACH_POINTS]
    if name == "pieces":
        return pieces()
    if name == "nested":
        return slide(lambda tlen, p: nested(tlen=tlen, p=p), tlen=20, points=(10,))
    raise KeyError(name)


SWEPT = ("suffix", "waiters", "widths_row", "widths_wave", "reach")      # through every kernel set at both piece settings
ALL = SWEPT + ("pieces",)


class Case:
    def __init__(self, name):
        self.name = name
        self.targets = _targets(name)
        self.batch = batch_from_targets(self.targets)
        self.full_span = all(host_full_span(t) for t in self.targets)

    @functools.cached_property
    def graphs(self):
        """_oracle_graph of every target after mergeNodes, for _check_graphs."""
        from test_gpu_parity import _oracle_graph
        return [_oracle_graph(self.batch, t, 0, 0, True) for t in range(self.batch.n_targets)]

    @functools.cached_property
    def paths(self):
        """The oracle's best path of every target (og_best_path), in oracle ids."""
        out = []
        for tlen, alns, _ in self.targets:
            g = oracle.Graph(blen=tlen)
            for s, q, t in alns:
                g.add_aln(s, *oracle.normalize_gaps(q, t))
            assert g.merge_nodes() == 0
            out.append(g.best_path())
        return out

    @functools.cached_property
    def sweeps(self):
        return [Sweep(adj, o2d, path) for (adj, o2d), path in zip(self.graphs, self.paths)]

    @functools.cached_property
    def consensus(self):
        """The oracle's consensus under each of CNS_OPTS."""
        return [oracle_batch(self.batch, **o) for o in CNS_OPTS]

    @functools.cached_property
    def annotated(self):
        """Under each of CNS_OPTS, per target [(range0, range1, seq, positions, weights, depths)]: window_twin's positions
        and support_twin's support of every consensus base, read along the oracle's best path."""
        import support_twin
        import window_twin
        out = []
        for o in CNS_OPTS:
            pos = window_twin.batch_positions(self.batch, **o)
            sup = support_twin.batch_support(self.batch, **o)
            both = []
            for ps, ss in zip(pos, sup):
                assert [x[:3] for x in ps] == [x[:3] for x in ss]
                both.append([p + s[3:] for p, s in zip(ps, ss)])
            out.append(both)
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
