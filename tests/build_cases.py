"""Pileups that cross the fixed-size limits of the build stage (addAln on the device) on purpose, for
tests/test_build_limits.py.

The build stage is k_gsum / k_groups, k_gscan, k_carve, k_emit and k_lists (pbdagcon_amd/csrc/k_build.hip.h).  Its fixed
sizes, each with another code path behind it: batches of DG_EB = 8 positions (a departure cell staged in LDS or stored
straight to matD; the loop running on past the target's end while a read has yet to reach the exit); DG_ECOLS = 40 staged
columns from a multiple of 8, DG_ENEED = 16 of them wanted when a batch starts (a restage at the start of a batch, a restage
in the middle of a position); stretches of 1 << emit_shift positions (a lane enters at a checkpoint and looks back, the
last vertex made in a stretch looks ahead); DG_ERPW = 64 reads a wave (run lengths in byte or 32-bit cells and the wave's
own prefix, against k_groups' prefix in place); the fold of duplicate chains (one to three bases, an anchor that is a
backbone vertex made by this wave less than 16 positions back); 64 list entries on the lanes of k_lists, then LDS; 1024
positions a pass of k_gscan, 1024 targets a pass of k_carve, 8 positions a wave of k_groups, four positions a thread of
k_gsum<uint8_t>.  The families here are built to cross each of them from both sides.

Every constructed alignment is written in normalized form over a backbone of A and C: an inserted base is G or T (or a
letter the family names), the base behind a deletion run that a match follows is a letter that does not occur in the run
(`stoppers`), so oracle.normalize_gaps and trimAln at trim 0 return it unchanged (asserted by `target`): the columns lie
where the family put them.

`Emit` is k_emit's schedule restated in plain Python over those columns, for a given emit_shift and cell path, and
`Lists` is k_lists' construction of one list.  They say which path every (target, wave of reads, stretch, lane)
takes and nothing about values: every graph a device run is held to is oracle.Graph's, every consensus oracle_batch's.
"""
import collections
import functools

import oracle
from merge_cases import CNS_OPTS, GAP, GRAPH_OPTS, backbone, gt
from util import batch_from_targets, oracle_batch

# the device's constants, restated (k_build.hip.h)
DG_EB, DG_ECOLS, DG_ENEED, DG_ERPW, DG_WAVE = 8, 40, 16, 64, 64
EF_BB, EF_OWN = 1, 2
FOLD_FAR, FOLD_BASES = 16, 3
DEFAULT_SHIFT = 9
STOPPERS = b"NRYKMSWBDHVEFIJLOPQUXZ"                      # letters behind deletion runs: none of ACGT


# ---- building blocks ---------------------------------------------------------------------------------------------------

def M(n):
    return ("M", n)


def D(n):
    return ("D", n)


def I(x, seed=0):
    """An insertion run: the bases given, or x bases over GT."""
    return ("I", x if isinstance(x, bytes) else gt(x, 1000 + 7 * x + seed))


def rest(tlen, start, ops):
    """ops followed by matches up to the target's last base."""
    used = sum(n for k, n in ops if k in "MD")
    left = tlen - (start - 1) - used
    assert left >= 0
    return list(ops) + ([M(left)] if left else [])


def target(tlen, reads, fixed=None, seed=5):
    """(tlen, alns, backbone) of reads [(start, ops)] over a backbone of A and C; `fixed` {position: base} names backbone
    bases, and the position behind every deletion run that a match follows gets a letter that is not in the run.
    Asserts that every alignment is a fixed point of normalizeGaps (and of trimAln at trim 0)."""
    bb = bytearray(backbone(tlen, seed))
    for p, b in (fixed or {}).items():
        bb[p - 1] = b
    stops = collections.defaultdict(list)                 # position behind a run -> the runs (first, last) that end there
    for start, ops in reads:
        x = start
        for k, (op, n) in enumerate(ops):
            if op == "D" and k + 1 < len(ops) and ops[k + 1][0] == "M" and ops[k + 1][1] > 0:
                stops[x + n].append((x, x + n - 1))
            if op in "MD":
                x += n
        assert x - 1 <= tlen, (tlen, start, ops)
    for p in sorted(stops):
        if fixed and p in fixed:
            continue
        inside = {bb[i - 1] for a, b in stops[p] for i in range(a, b + 1)}
        bb[p - 1] = next(c for c in STOPPERS if c not in inside)
    alns = []
    for start, ops in reads:
        q, t, x = bytearray(), bytearray(), start - 1
        for op, n in ops:
            if op == "M":
                q += bb[x:x + n]; t += bb[x:x + n]; x += n
            elif op == "D":
                q += bytes([GAP]) * n; t += bb[x:x + n]; x += n
            else:
                q += n; t += bytes([GAP]) * len(n)
        q, t = bytes(q), bytes(t)
        assert len(q) == len(t) > 0
        assert oracle.normalize_gaps(q, t) == (q, t), ("a constructed alignment must be normalized already", start, ops)
        assert oracle.trim_aln(q, t, start, 0) == (q, t, start)
        alns.append((start, q, t))
    return tlen, alns, bytes(bb)


def chunks(reads, size, fill):
    """reads in groups of `size`, the last one filled up with `fill`."""
    out = [list(reads[i:i + size]) for i in range(0, len(reads), size)]
    out[-1] += [fill] * (size - len(out[-1]))
    return out


# ---- the model of k_emit ------------------------------------------------------------------------------------------------

def _columns(aln):
    return list(zip(aln[1], aln[2]))


def checkpoints(start, cols, shift, tlen):
    """dg_finish_alignment's checkpoints of one read: {stretch: first column that belongs to the stretch's first position}
    (the insertion run in front of that position included; a trailing run counts for the position behind the read)."""
    mask, ck, adv, run = (1 << shift) - 1, {}, 0, 0
    for ci, (qb, tb) in enumerate(cols):
        if qb == tb or qb == GAP:
            pos = start + adv
            if pos & mask == 0 and pos <= tlen + 1:
                ck[pos >> shift] = ci - run
            run = 0
            adv += 1
        elif tb == GAP:
            run += 1
    if run and (start + adv) & mask == 0 and start + adv <= tlen + 1:
        ck[(start + adv) >> shift] = len(cols) - run
    return ck


class Emit:
    """What k_emit does with one target: counters over every (wave of reads, stretch, lane).

    entry: how a lane comes into a stretch -- 'starts', 'later', 'ended', 'idle', ('match',), ('del', d), ('enter', d: nothing
    but d deletions in front), ('ins', d, how): behind an insertion run and d deletions, resolved by 'pfx' (emit_scan),
    'next' (the next read's cell) or 'gcount' (the target's last read).  stage_first / stage_batch / stage_column: a lane's
    first staging, a restage when a batch starts, a restage inside a position ((read, position) of each).  depart_lds /
    depart_direct: departures of backbone vertices staged in s_D or stored straight (look-aheads not counted);
    ahead: the look-ahead's kind, ('match',), ('del', d), ('ins', d), ('exit', d).  tail: the batches that ran past
    position tlen, [(first position, the exit is its first position)].  early: stretch waves of the batch's grid that
    return at once.  keys: {position: {wave: [(distance, bases, lane)]}}; groups: [(position, wave, distance, bases, n)]
    of two or more; nokey: reasons of the chains in front of a match that get no key (nokey_at: [(position, reason,
    bases)]); split: (position, distance, bases) of identical chains in two waves."""

    def __init__(self, tlen, alns, shift, scan, grid_tlen=None):
        self.tlen, self.shift, self.scan, self.K = tlen, shift, scan, len(alns)
        self.entry, self.ahead, self.nokey = collections.Counter(), collections.Counter(), collections.Counter()
        self.stage_first, self.stage_batch, self.stage_column = 0, [], []
        self.depart_lds = self.depart_direct = self.early = 0
        self.tail, self.groups, self.split, self.nokey_at = [], [], [], []
        self.exit_in_loop = self.exit_ahead = 0
        self.keys = collections.defaultdict(lambda: collections.defaultdict(list))
        reads = [(s, _columns(a), checkpoints(s, _columns(a), shift, tlen)) for a in alns for s in [a[0]]]
        nz = (((grid_tlen or tlen) + 2) >> shift) + 1
        for y in range((self.K + DG_ERPW - 1) // DG_ERPW):
            for z in range(nz):
                if (z << shift) > tlen + 1:
                    self.early += 1
                else:
                    self._wave(reads, y, z)
        for pos, waves in self.keys.items():
            per = [{(d, b) for d, b, _ in ch} for ch in waves.values()]
            for i in range(len(per)):
                for j in range(i + 1, len(per)):
                    self.split += [(pos,) + k for k in per[i] & per[j]]
            for y, ch in waves.items():
                cnt = collections.Counter((d, b) for d, b, _ in ch)
                self.groups += [(pos, y, d, b, n) for (d, b), n in cnt.items() if n > 1]

    def _wave(self, reads, y, z):
        blen, shift, K = self.tlen, self.shift, self.K
        exitpos, P0 = blen + 1, z << shift
        P1 = P0 + (1 << shift)
        L = []
        for lane in range(DG_ERPW):
            r = y * DG_ERPW + lane
            if r >= K:
                self.entry["idle"] += 1
                continue
            start, cols, ck = reads[r]
            s = dict(r=r, lane=lane, cols=cols, hi=len(cols), i=0, bbpos=start, prev_pos=0, fl=EF_BB | EF_OWN, c_base=None)
            if start >= P1:
                s["bbpos"] = None
                self.entry["later"] += 1
            elif start < P0:
                c = ck.get(z)
                if c is None or c >= s["hi"]:
                    s["bbpos"] = None
                    self.entry["ended"] += 1
                else:
                    s["i"], s["bbpos"], s["fl"] = c, P0, EF_BB
                    x, d, kind = c, 0, None
                    while x > 0:
                        x -= 1
                        qb, tb = cols[x]
                        if qb == tb:
                            s["prev_pos"] = P0 - 1 - d
                            kind = ("match",) if d == 0 else ("del", d)
                            break
                        if qb == GAP:
                            d += 1
                            continue
                        if tb == GAP:
                            s["prev_pos"], s["fl"] = P0 - d, 0
                            kind = ("ins", d, "pfx" if self.scan else "next" if r + 1 < K else "gcount")
                            break
                    self.entry[kind or ("enter", d)] += 1
            else:
                self.entry["starts"] += 1
            L.append(s)
        pos0 = P0
        while pos0 < P1 and (pos0 <= blen or (any(s["bbpos"] is not None for s in L) and pos0 <= blen + 2 * DG_EB)):
            if pos0 > blen:
                self.tail.append((pos0, pos0 == exitpos))
            for s in L:
                if s["bbpos"] is not None and s["i"] < s["hi"] and (s["c_base"] is None or s["i"] - s["c_base"] + DG_ENEED > DG_ECOLS):
                    if s["c_base"] is None:
                        self.stage_first += 1
                    else:
                        self.stage_batch.append((s["r"], pos0))
                    s["c_base"] = s["i"] & ~7
            for pos in range(pos0, pos0 + DG_EB):
                for s in L:
                    if s["bbpos"] != pos or pos >= P1:
                        continue
                    f_apos, f_fl, bases = s["prev_pos"], s["fl"], bytearray()
                    while True:
                        if s["i"] < s["hi"]:
                            if s["i"] - s["c_base"] >= DG_ECOLS:
                                self.stage_column.append((s["r"], pos))
                                s["c_base"] = s["i"] & ~7
                            qb, tb = s["cols"][s["i"]]
                        if s["i"] >= s["hi"] or qb == tb or qb == GAP:
                            break
                        assert tb == GAP
                        bases.append(qb)
                        self._depart(s, pos0)
                        s["prev_pos"], s["fl"] = pos, EF_OWN
                        s["i"] += 1
                    if s["i"] >= s["hi"]:
                        self.exit_in_loop += 1
                        self._depart(s, pos0)
                        s["bbpos"] = None
                        continue
                    if qb == tb:
                        if bases:
                            why = ("bases" if len(bases) > FOLD_BASES else "not backbone" if not f_fl & EF_BB else
                                   "not owned" if not f_fl & EF_OWN else "far" if pos - f_apos >= FOLD_FAR else None)
                            if why:
                                self.nokey[why] += 1
                                self.nokey_at.append((pos, why, bytes(bases)))
                            else:
                                self.keys[pos][y].append((pos - f_apos, bytes(bases), s["lane"]))
                        self._depart(s, pos0)
                        s["prev_pos"], s["fl"] = pos, EF_BB | EF_OWN
                    s["bbpos"] += 1
                    s["i"] += 1
            pos0 += DG_EB
        for s in L:
            if s["bbpos"] is None or not s["fl"] & EF_OWN:
                continue
            d, kind, i = 0, None, s["i"]
            while i < s["hi"]:
                qb, tb = s["cols"][i]
                if qb == tb:
                    kind = ("match",) if d == 0 else ("del", d)
                    break
                if qb == GAP:
                    d += 1
                elif tb == GAP:
                    kind = ("ins", d)
                    break
                i += 1
            if kind is None:
                self.exit_ahead += 1
            self.ahead[kind or ("exit", d)] += 1

    def _depart(self, s, pos0):
        if s["fl"] == EF_BB | EF_OWN:
            if s["prev_pos"] >= pos0:
                self.depart_lds += 1
            else:
                self.depart_direct += 1

    def figures(self):
        kinds = collections.Counter()
        for k, n in self.entry.items():
            kinds[k if isinstance(k, str) else k[0] + ("/" + k[2] if k[0] == "ins" else "")] += n
        return dict(entry=dict(kinds), stage_batch=len(self.stage_batch), stage_column=len(self.stage_column),
                    depart_lds=self.depart_lds, depart_direct=self.depart_direct,
                    ahead=dict(collections.Counter(k[0] for k in self.ahead.elements())),
                    tail=len(self.tail), early=self.early, groups=len(self.groups), nokey=dict(self.nokey), split=len(self.split))


def merged(figs):
    """The sum of several figures() (counters added, nested ones too)."""
    out = {}
    for f in figs:
        for k, v in f.items():
            if isinstance(v, dict):
                d = out.setdefault(k, {})
                for kk, vv in v.items():
                    d[kk] = d.get(kk, 0) + vv
            else:
                out[k] = out.get(k, 0) + v
    return out


# ---- the model of k_lists -----------------------------------------------------------------------------------------------

def read_paths(tlen, alns):
    """addAln's path of every read: ('B', position) for a backbone vertex, ('I', read, n) for the read's n-th inserted vertex."""
    out = []
    for r, (start, q, t) in enumerate(alns):
        path, pos, n = [("B", 0)], start, 0
        for qb, tb in zip(q, t):
            if qb == tb:
                path.append(("B", pos)); pos += 1
            elif qb == GAP:
                pos += 1
            elif tb == GAP:
                path.append(("I", r, n)); n += 1
        path.append(("B", tlen + 1))
        out.append(path)
    return out


class Lists:
    """k_lists' construction of the out and the in list of every backbone position of a deep target, from the reads'
    paths: a list keeps entry i on lane i while it has at most 64 entries and moves to LDS when the 65th arrives.
    lens: {('out' | 'in', position): entries}; hits_lanes / hits_lds: entries other than entry 0 found again in a later
    group of 64 reads while the list is on the lanes / in LDS, counted per read (the device peels equal cells of one group
    of reads in one round); hits: the same per list, {list: [on the lanes, in LDS]}; recur: the lists with such a hit;
    in_lds: the lists that moved; moved: {list: (the group of reads in which it moved, its entries then)}."""

    def __init__(self, tlen, alns):
        K = len(alns)
        dep, arr = collections.defaultdict(dict), collections.defaultdict(dict)
        for r, path in enumerate(read_paths(tlen, alns)):
            for a, b in zip(path, path[1:]):
                if a[0] == "B":
                    dep[a[1]][r] = b
                if b[0] == "B":
                    arr[b[1]][r] = a
        self.lens, self.recur, self.in_lds = {}, set(), set()
        self.hits, self.moved = collections.defaultdict(lambda: [0, 0]), {}
        self.hits_lanes = self.hits_lds = 0
        for side, cells, first in (("out", dep, 1), ("in", arr, -1)):
            for pos in range(tlen + 2):
                if (side == "out" and pos == tlen + 1) or (side == "in" and pos == 0):
                    continue
                entries, lds = {("B", pos + first): 0}, False
                for r in range(K):
                    v = cells[pos].get(r)
                    if v is None or (v == ("B", pos + first) and not lds):
                        continue
                    if v in entries:
                        if entries[v] < r // DG_WAVE and v != ("B", pos + first):
                            self.recur.add((side, pos))
                            self.hits[side, pos][lds] += 1
                            if lds:
                                self.hits_lds += 1
                            else:
                                self.hits_lanes += 1
                        continue
                    if len(entries) >= DG_WAVE and not lds:
                        lds = True
                        self.moved[side, pos] = (r // DG_WAVE, len(entries))
                    entries[v] = r // DG_WAVE
                self.lens[side, pos] = len(entries)
                if lds:
                    self.in_lds.add((side, pos))

    def figures(self):
        return dict(longest=max(self.lens.values()), in_lds=len(self.in_lds), recur=len(self.recur),
                    hits_lanes=self.hits_lanes, hits_lds=self.hits_lds)


# ---- the families ------------------------------------------------------------------------------------------------------

BATCH_TLEN = (6, 7, 8, 14, 15, 16, 17, 24)       # (24: the only one a deletion run of 17 fits into with a match on either side)


def batches():
    out = []
    for T in BATCH_TLEN:
        reads = [(1, [M(T)]), (1, [M(T), I(1)]), (1, [M(T), I(9)]), (T, [M(1)])]
        reads += [(1, [M(T - d), D(d)]) for d in (1, 7, 8, 9) if T - d >= 1]
        reads += [(1, rest(T, 1, [M(a), D(n)])) for n in (7, 8, 9, 17) for a in (1, 2) if a + n + 1 <= T]
        for grp in chunks(reads, 9 if len(reads) > 8 else 8, (1, [M(T)])):
            out.append(target(T, grp + [(1, [M(T)])] * max(0, 6 - len(grp))))
    return out


COLUMN_RUNS = (23, 24, 25, 39, 40, 41, 47, 48, 90)
COLUMN_PHASES = (0, 1, 7)
COLUMN_AT = (17, 33)                                 # the run stands in front of this position
COLUMN_TLEN = 120


def column_read(L, phase, at):
    """A lead of `phase` columns and at - 1 matches: the run's first column has index phase + at - 1, which is `phase`
    modulo 8 for both values of COLUMN_AT."""
    return 1, rest(COLUMN_TLEN, 1, ([I(phase, 3)] if phase else []) + [M(at - 1), I(L, phase)])


def column_read_last(L, phase):
    """The run in front of position 32, the first of its batch and the read's last: column index 31 + lead, the lead chosen
    for the phase.  Nothing behind the run's match column asks for a column."""
    lead = (phase + 1) % 8
    return 1, ([I(lead, 5)] if lead else []) + [M(31), I(L, phase), M(1)]


def columns():
    reads = [column_read(L, ph, at) for at in COLUMN_AT for ph in COLUMN_PHASES for L in COLUMN_RUNS]
    reads += [column_read_last(L, ph) for ph in COLUMN_PHASES for L in COLUMN_RUNS]
    # runs of 5 in front of eight positions in a row, 48 columns in one batch; alignments of 8n + 1 and of 8n + 7
    # columns with a run directly in front of the last column, and with a trailing run
    reads.append((1, rest(COLUMN_TLEN, 1, [M(16)] + [x for k in range(8) for x in (I(5, k), M(1))])))
    reads.append((1, [M(40), I(8), M(1)]))            # 49 columns
    reads.append((1, [M(40), I(14), M(1)]))           # 55 columns
    reads.append((1, [M(40), I(9)]))                  # 49 and 55 columns, the run the alignment's last columns
    reads.append((1, [M(40), I(15)]))
    return [target(COLUMN_TLEN, grp) for grp in chunks(reads, 8, (1, [M(COLUMN_TLEN)]))]


def stretch_reads(T, E, runs, gap=3):
    """Reads of a target of T bases around the stretch edge E (the first position of a stretch; E - 1 is the last one of
    the stretch in front)."""
    out = []
    for n in runs:
        for last in (E - 2, E - 1, E, E + 1):          # the run's last deleted base: before, on and behind the edge
            if last - n >= 1 and last < T:
                out.append((1, rest(T, 1, [M(last - n), D(n)])))
    for at in (E, E - 1):                              # an insertion run directly in front of the first / the last position
        out.append((1, rest(T, 1, [M(at - 1), I(3, at)])))
        out.append((1, rest(T, 1, [M(at - 1 - gap), I(2, at), D(gap)])))      # ... and a deletion run between it and the edge
    out.append((1, [M(E - 1)]))                        # ends on the edge
    out.append((1, [M(E - 1), I(2)]))
    out.append((1, [M(E)]))
    out.append((1, [M(E), I(4)]))
    out.append((E, [M(T - E + 1)]))                    # starts on it
    out.append((E, [I(3), M(T - E + 1)]))
    out.append((E - 1, [I(2), M(T - E + 2)]))
    out.append((1, rest(T, 1, [M(E - 2), D(3), I(2, E + 2)])))     # the look-ahead: deletions over the edge, then a run
    out.append((E - 2, rest(T, E - 2, [D(3)])))                    # nothing but deletions in front of the edge: behind enter
    return out


def with_last(reads, k):
    """reads with read k moved to the end: the target's last read."""
    return reads[:k] + reads[k + 1:] + [reads[k]]


STRETCH_LONG = 1038                                   # tlen + 2 = 1040: k_gscan's second pass as well


def stretches():
    out = []
    # shift 4: edges 32 and 48 of targets of 70 bases; a stretch that holds nothing but a read's deletions (16 .. 31 of 15 .. 47)
    for E, runs in ((32, (15, 16, 17)), (48, (15, 16, 17, 33))):
        reads = stretch_reads(70, E, runs)
        ins_first = next(k for k, (s, ops) in enumerate(reads) if ops[:2] == [M(E - 1), I(3, E)])
        for g, grp in enumerate(chunks(reads, 9, (1, [M(70)]))):
            out.append(target(70, grp))
        out.append(target(70, with_last(reads[ins_first:ins_first + 4], 0) ))            # the run in front of E in the last read
        out.append(target(70, with_last(reads[ins_first:ins_first + 4], 1)))            # the run and the deletions in the last read
    for T in (14, 15, 16):                             # tlen + 1 = 15, 16, 17
        out.append(target(T, [(1, [M(T)]), (1, [M(T), I(2)]), (1, [M(T - 1), D(1)])]))
    # the default stretch: edge 512 of a target of 1038 bases, and tlen + 1 = 511, 512, 513
    reads = stretch_reads(STRETCH_LONG, 512, (15, 16, 17, 33))
    reads += [(1, rest(STRETCH_LONG, 1, [M(at - 1), I(2, at)])) for at in range(1022, 1027)]      # (k_gscan: around position 1024)
    reads.append((1, rest(STRETCH_LONG, 1, [M(512 - 4), I(2, 512), D(3)])))      # once more, as the target's last read
    out.append(target(STRETCH_LONG, reads))
    for T in (510, 511, 512):
        out.append(target(T, [(1, [M(T)]), (1, [M(T), I(2)]), (1, [M(T - 1), D(1)])]))
    return out


def fold():
    out = []
    T = 50

    def at(p, run, lead=()):
        return 1, rest(T, 1, list(lead) + [M(p - 1), I(run)])

    def several(p_run, n):
        """n full-span reads that carry every chain of p_run {position: bases}."""
        ops, x = [], 1
        for p in sorted(p_run):
            ops += [M(p - x), I(p_run[p])]
            x = p
        return [(1, rest(T, 1, ops))] * n

    plain = (1, [M(T)])
    # identical chains of 1, 2, 3 and 4 bases in 2, 3 and 64 reads
    chains = {5: b"G", 9: b"GT", 13: b"TGT", 17: b"GTTG"}
    out.append(target(T, several(chains, 2) + [plain] * 2))
    out.append(target(T, [plain] + several(chains, 3) + [plain]))
    out.append(target(T, several(chains, 64)))
    # two and three distinct keys closing at one position, interleaved over the lanes; a fold at consecutive positions;
    # the bases at both ends of the range the device admits
    two = [at(20, [b"G", b"T"][r & 1]) for r in range(6)]
    three = [at(24, [b"G", b"T", b"GT"][r % 3]) for r in range(9)]
    out.append(target(T, two + three))
    out.append(target(T, [(1, rest(T, 1, [M(29), I(b"G"), M(1), I(b"T")]))] * 3 + [plain]))
    out.append(target(T, [at(11, b"!")] * 2 + [at(11, b"~")] * 2 + [at(12, b"!~")] * 2))
    # the substitution form at distances 2, 3, 15, 16, 17: k deleted bases, the deleted base, its replacement
    for k in (0, 1, 13, 14, 15):
        out.append(target(T, [(1, rest(T, 1, [M(10), D(k + 1), I(b"G")]))] * 3 + [plain, at(30, b"T")]))
    # the same base at two distances at one position; ACGT and CCGT at distance 2 (next to N and R: nothing slides)
    out.append(target(T, [(1, rest(T, 1, [M(10), D(1), I(b"G")]))] * 2 + [(1, rest(T, 1, [M(11), I(b"G")]))] * 2 + [plain]))
    out.append(target(T, [(1, rest(T, 1, [M(10), D(1), I(b"ACGT")]))] * 2 + [(1, rest(T, 1, [M(10), D(1), I(b"CCGT")]))] * 2 + [plain],
                      fixed={11: ord("R"), 12: ord("N")}))
    # chains whose anchor is enter: leading runs of reads that start at 1, 2 and 15; then next to partial-span reads
    lead = [(s, [I(b"GT"), M(T - s + 1)]) for s in (1, 2, 15) for _ in range(3)]
    out.append(target(T, lead))
    out.append(target(T, lead[3:] + [(20, [M(20)]), (1, [M(30)]), (2, [I(b"T"), M(40)])]))
    # the first chain of a lane in a stretch (shift 4: in front of position 16 and 32, anchored at 15 and 31) next to the
    # same chain anchored inside the stretch
    out.append(target(60, [(1, rest(60, 1, [M(15), I(b"GT"), M(2), I(b"GT"), M(14), I(b"T"), M(3), I(b"T")]))] * 3 + [(1, [M(60)])]))
    # a chain behind an inserted vertex: a run, the deleted base behind it, a run again (the anchor is no backbone vertex)
    out.append(target(T, [(1, rest(T, 1, [M(35), I(b"G"), D(1), I(b"T")]))] * 2 + [plain]))
    return out


def fold_two_waves(T=50):
    """128 reads: the same chain in lanes 63 | 64, in lanes 0 and 127, and in lanes 5, 62 | 65, 126 (a group in either
    wave).  More than a wave of reads: it travels with the deep family."""
    reads = [(1, [M(T)])] * 128
    reads[63] = reads[64] = (1, rest(T, 1, [M(20), I(b"TG")]))
    reads[0] = reads[127] = (1, rest(T, 1, [M(32), I(b"G")]))
    reads[5] = reads[62] = reads[65] = reads[126] = (1, rest(T, 1, [M(39), I(b"GG")]))
    return target(T, reads)


DEEP_K = (65, 127, 128, 129, 200)
LETTERS = bytes(b for b in range(33, 127) if b not in b"ACGTNacgtn-.^$" and b not in STOPPERS)


def letters2(r):
    """A run of two bases that no other read has."""
    return bytes([LETTERS[r % len(LETTERS)], LETTERS[r // len(LETTERS)]])


def deep_target(K, n_ins=None, ins_then_del=None, jumps=None, T=40):
    """K reads over 40 bases.  Reads 3 and 4 of every wave: the same chain in front of position 5 (a fold per wave).
    Position 10: a run of its own in front of it in each of the first n_ins reads (all of them by default).  Positions 16
    and 32: runs in reads 63, 64 and K - 1 (stretch edges under shift 4).  Behind position 20 read r deletes r % 15 bases;
    ins_then_del: the first so many reads have a run of their own in front of position 21 instead, and with `jumps` {read:
    deleted bases} only the reads named there delete anything."""
    n_ins = K if n_ins is None else n_ins
    reads = []
    for r in range(K):
        ops, x = [], 1

        def upto(p):
            nonlocal x
            if p > x:
                ops.append(M(p - x))
            x = max(x, p)
        if r % 64 in (3, 4):
            upto(5); ops.append(I(b"GT"))
        if r < n_ins:
            upto(10); ops.append(I(letters2(r)))
        if r in (63, 64, K - 1):
            upto(16); ops.append(I(2, r))
        upto(21)
        if ins_then_del is not None and r < ins_then_del:
            ops.append(I(letters2(r)))
        elif jumps is not None:
            if r in jumps:
                ops.append(D(jumps[r])); x += jumps[r]
        elif r % 15:
            ops.append(D(r % 15)); x += r % 15
        if r in (63, 64, K - 1) and x < 32:
            upto(32); ops.append(I(1, r))
        reads.append((1, rest(T, 1, ops)))
    return target(T, reads)


# One list, the out list of position 20, handed over from the lanes to LDS by design: 60 runs and the jumps over 1 and 2
# bases make 63 entries in the first group of 64 reads; in the second the jump over 1 base is found again on the lanes
# (read 64), the jump over 3 is the 64th entry (read 65) and the jump over 4 the 65th, which moves the list to LDS (read
# 66); in the third the jumps over 1, 2 and 4 bases are found again in LDS (reads 128 .. 130) and the jump over 5 is new.
HAND_OVER = {60: 1, 61: 2, 64: 1, 65: 3, 66: 4, 128: 1, 129: 2, 130: 4, 131: 5}


def deep():
    out = [deep_target(K) for K in DEEP_K]
    out += [deep_target(100, n_ins=n) for n in (62, 63, 64, 65)]          # lists of exactly 63, 64, 65 and 66 entries
    out.append(deep_target(130, n_ins=0, ins_then_del=61))               # 62 entries, then jumps: two on the lanes, the rest in LDS
    out.append(deep_target(140, n_ins=0, ins_then_del=60, jumps=HAND_OVER))
    out.append(fold_two_waves())
    return out


def scan_target(T, at, n_reads=3):
    """Runs in front of the positions `at` that exist (tlen + 1: a trailing run), in every one of n_reads reads, lengths
    1 .. 3 by read."""
    reads = []
    for r in range(n_reads):
        ops, x = [], 1
        for p in at:
            if p <= T + 1:
                ops += [M(p - x), I(1 + (r + p) % 3, r + p)]
                x = p
        reads.append((1, rest(T, 1, ops)))
    return target(T, reads)


def scans():
    out = [scan_target(T, range(1022, 1027)) for T in (1021, 1022, 1023)]     # tlen + 2 = 1023, 1024, 1025
    out += [scan_target(T, range(T - 1, T + 2)) for T in (31, 32, 33, 34)]    # tlen + 2 = 33 .. 36
    return out


CARVE_N = 2049
CARVE_MARKED = (0, 1023, 1024, 1025, 2048)
CARVE_SHORT = (1024, 1500)                        # every read below min_len: a bare backbone
CARVE_INACTIVE = (700, 1022, 2047)                # one read: below min_cov, skipped
CARVE_BAD = 1100                                  # start 0: non-conforming, tfail
CARVE_OPTS = dict(min_cov=2, min_len=5, trim=0, min_weight=0)
CARVE_GRAPHS = (0, 1, 2, 699, 701, 1021, 1023, 1024, 1025, 1026, 1099, 1101, 1102, 1499, 1500, 1501, 2045, 2046, 2048)


def carve():
    """2049 targets of 4 to 6 bases, 2 reads each with one inserted base; the marked ones are longer and have 3 reads."""
    out = []
    for t in range(CARVE_N):
        T = 4 + t % 3
        if t in CARVE_MARKED:
            T = 9 + CARVE_MARKED.index(t)
        if t in CARVE_SHORT:
            reads = [(1 + r, [M(2), I(1, t)]) for r in range(3 if t in CARVE_MARKED else 2)]      # 3 columns each
        elif t in CARVE_MARKED:
            reads = [(1, rest(T, 1, [M(2 + r), I(2, t + r)])) for r in range(3)]
        elif t in CARVE_INACTIVE:
            reads = [(1, rest(T, 1, [M(1), I(1, t)]))]
        else:
            reads = [(1, rest(T, 1, [M(1 + (t + r) % (T - 1)), I(1, t + r)])) for r in range(2)]
        tg = target(T, reads, seed=t)
        if t == CARVE_BAD:
            tg = (T, [(0, q, tt) for _, q, tt in tg[1]], tg[2])
        out.append(tg)
    return out


# ---- the extra targets that select the cell path ----------------------------------------------------------------------------

def wide_extra(run=256):
    """A small target with a run of 256 columns: byte cells overflow, the batch runs again with 32-bit cells.  (255: its
    narrow twin, which a byte still holds.)"""
    return target(12, [(1, rest(12, 1, [M(6), ("I", gt(256, 77)[:run])])), (1, [M(12)]), (1, [M(12)])])


def groups_extra():
    """A 65-read target: every target of the batch takes k_groups' prefix in place."""
    return target(12, [(1, rest(12, 1, [M(3 + r % 5), I(1 + r % 2, r)])) for r in range(65)])


CELLS = ("scan-byte", "scan-wide", "groups")
FAMILIES = {"batches": batches, "columns": columns, "stretches": stretches, "fold": fold, "deep": deep, "scans": scans,
            "carve": carve}
SHIFTS = {"batches": (4, None), "columns": (4, None), "stretches": (4, 6, None), "fold": (4, 6, None), "deep": (4, None),
          "scans": (4, None), "carve": (4, None)}
# the cell paths a family cannot take: a target of more than 64 reads is never on the scan paths, and no run of 256 fits
# the batch of 2049 tiny targets without a target that is not tiny (its wide run is the extra target's, as everywhere)
LEFT_OUT = {("deep", "scan-byte"), ("deep", "scan-wide"), ("carve", "scan-wide")}
SETTINGS = [(f, c, s) for f in FAMILIES for c in CELLS if (f, c) not in LEFT_OUT for s in SHIFTS[f]]


class Case:
    """A family under one cell path: its targets plus the extra target that selects the path."""

    def __init__(self, name, cells):
        self.name, self.cells = name, cells
        self.family = family(name)
        extra = {"scan-byte": [], "scan-wide": [wide_extra()], "groups": [groups_extra()]}[cells]
        self.targets = self.family + extra
        self.batch = batch_from_targets(self.targets)
        # scan-wide: the same batch with a run of 255, to size a context's arenas before the run whose re-runs are counted
        self.warm = batch_from_targets(self.family + [wide_extra(255)]) if cells == "scan-wide" else None
        self.opts = CARVE_OPTS if name == "carve" else GRAPH_OPTS
        self.cns_opts = (CARVE_OPTS, dict(CARVE_OPTS, trim=1)) if name == "carve" else CNS_OPTS + (dict(GRAPH_OPTS, min_cov=2, trim=1),)
        self.checked = list(CARVE_GRAPHS) + list(range(CARVE_N, len(self.targets))) if name == "carve" else list(range(len(self.targets)))
        self.failed = [CARVE_BAD] if name == "carve" else []
        self.max_k = max(len(t[1]) for t in self.targets)

    def oracle_view(self):
        """The batch the oracle answers for: a non-conforming target is one without alignments (the device drops it)."""
        if not self.failed:
            return self.batch
        return batch_from_targets([(t[0], [], t[2]) if i in self.failed else t for i, t in enumerate(self.targets)])

    @functools.cached_property
    def graphs(self):
        """{merged?: {target: _oracle_graph}} of the targets whose graphs are checked."""
        from test_gpu_parity import _oracle_graph
        b = self.oracle_view()
        skip = set(CARVE_INACTIVE) | set(self.failed) if self.name == "carve" else set()
        return {m: {t: _oracle_graph(b, t, self.opts["min_len"], 0, m) for t in self.checked if t not in skip} for m in (False, True)}

    @functools.cached_property
    def consensus(self):
        b = self.oracle_view()
        return [oracle_batch(b, **o) for o in self.cns_opts]


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def case(name, cells):
    return Case(name, cells)


@functools.lru_cache(maxsize=None)
def emit(name, shift, scan=True):
    """Emit of every target of a family at one stretch length, the grid sized for the family's longest target."""
    tg = family(name)
    longest = max(t[0] for t in tg)
    return [Emit(t[0], t[1], DEFAULT_SHIFT if shift is None else shift, scan, longest) for t in tg]
