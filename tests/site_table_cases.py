"""Batches that carry the site tables past every fixed size of their common path, for tests/test_site_table_limits.py.

The alleles at the sites (k_alleles.hip.h) and the joined runs (k_join.hip.h) share four fixed sizes that the batches of
test_site_alleles and test_site_join never reach:

  1,024 items      a round of dg_block_scan (k_scan.hip.h) behind k_al_soff, k_al_tscan, k_jn_stretch, k_jn_runs, k_jn_tscan
  1,024 blocks     the grid of k_al_table_deep and k_jn_table_deep, which loop `w += gridDim.x` over the deep sites / runs
  128 .. 4,096     the sizes n2 of the block sort (dg_al_block_sort), a power of two at or above the depth
  20 bases         a key's bases (DG_AL_BASES), bit 60 beyond

Four families, a construction each; a family's figures are asserted from the twin (join_twin.target through
test_site_join._expect) before the device runs:

  rounds(p)        two targets at 0 / 0, where every covered position is a site: a pad of p bases, then 200 bases, under
                   three whole reads and a fourth that shows another base at the sites numbered 1,020 .. 1,028
  past_the_grid()  2,120 bases under 65 whole reads and five shorter ones at 2 / 0.2: 1,061 sites, 1,039 runs, all deep
  sort_sizes(pat)  ten targets of 30 bases under 128, 129, 256, .. 2,049 whole reads at 0 / 0, `distinct` and `tied`
  key_length()     alleles of 19, 20, 21 and 22 bases at one site, in lane 60 of the walk's 64-column step, under trim 2

The schedules are restated over the twin's figures: block_scan (1,024 items a round, one carry), the five scans on it
(scans), deep_trips (the list index modulo 1,024 blocks), n2_of / block_table (the sort's size) and tables_with_cap (the
key's cap).  MUTATIONS names the ways they can be made wrong on purpose; no mutation is ever run on the device.

Two things the constructions cannot do, by the code's own arithmetic: oracle.trim_aln stops on a column with a target
base, so `hi` can end an insertion run (the run's last column is the alignment's last) but never cuts one in two; and at
an odd depth the counts of a table cannot all occur exactly twice, so one count occurs three times there.
"""
import functools
import itertools
from collections import Counter
from types import SimpleNamespace

import numpy as np

import alleles_twin as at
import evidence_twin as ev
import join_twin as jt
import site_reads_twin as srt
import test_site_join as tsj

ROUND, GRID = 1024, 1024                               # dg_block_scan's items a round; the deep kernels' blocks
WAVE = 64                                              # a deeper site / run goes on the deep list
N2_MIN, N2_MAX = 128, 4096
MUTATIONS = ("carry_dropped", "carry_early", "run_for_stretch", "one_trip", "stale_nd", "n2_small", "cap_21")
SCANS = ("k_al_soff", "k_al_tscan", "k_jn_stretch", "k_jn_runs", "k_jn_tscan")
U32 = 1 << 32


def _nonrep(rng, n, avoid=b""):
    return tsj._tes()._nonrep(rng, n, avoid)


def _case(name, strings, min_cov, min_len, trim, opts):
    tlens = [len(bb) for bb, _ in strings]
    exp = tsj._expect(strings, tlens, min_cov, min_len, trim, opts)
    return SimpleNamespace(name=name, strings=strings, tlens=tlens, min_cov=min_cov, min_len=min_len, trim=trim, opts=opts, exp=exp)


# ---- the schedules, restated --------------------------------------------------------------------------------------------

def block_scan(own, mut=None):
    """dg_block_scan: the exclusive prefix of `own`, 1,024 items a round; thread 1,023 leaves the carry (its offset plus its
    own count; a thread behind the last item has a count of 0).  Returns (offsets, total)."""
    off, carry = [], 0
    for i0 in range(0, len(own), ROUND):
        if mut == "carry_dropped" and i0:
            carry = 0
        chunk = list(own[i0:i0 + ROUND]) + [0] * (ROUND - len(own[i0:i0 + ROUND]))
        acc, offs = carry, []
        for x in chunk:
            offs.append(acc)
            acc += x
        off += offs[:len(own) - i0]
        carry = offs[-1] + (0 if mut == "carry_early" else chunk[-1])
    return off, carry


def figures(exp):
    """What the five scans read, from the twin's arrays of a batch: per site its target and position, its depth (a site's
    entries number its depth) and its alleles; per run its table's length."""
    sb = exp["site_begin"]
    tgt = [t for t in range(len(sb) - 1) for _ in range(sb[t], sb[t + 1])]
    n = len(exp["pos"])
    return dict(tgt=tgt, pos=list(exp["pos"]), depth=np.bincount(np.asarray(exp["ent_site"], np.int64), minlength=n).tolist(),
                al_nd=np.diff(exp["al_begin"]).tolist(), jn_nd=np.diff(exp["jal_begin"]).tolist())


def twin_arrays(exp):
    """The arrays the scans must give, from the twin alone."""
    f = figures(exp)
    return dict(soff=[0] + np.cumsum(f["depth"]).tolist(), al_begin=list(exp["al_begin"]), run_begin=list(exp["run_begin"]),
                jal_begin=list(exp["jal_begin"]))


def scans(exp, mut=None, scan=None, stale=0, al_nd=None, jn_nd=None):
    """The five scans in the device's order, `mut` applied to `scan` alone (run_for_stretch is k_jn_runs' own).  stale: what
    a word of jn_sfirst that no stretch wrote holds.  al_nd / jn_nd: table lengths other than the twin's (deep_trips)."""
    f = figures(exp)
    n = len(f["pos"])
    m = {s: (mut if s == scan else None) for s in SCANS}
    out = {}
    off, top = block_scan(f["depth"], m["k_al_soff"])
    out["soff"] = off + [top]
    off, top = block_scan(f["al_nd"] if al_nd is None else al_nd, m["k_al_tscan"])
    out["al_begin"] = off + [top]
    # k_jn_stretch: jn_run[k] = the stretch's number, jn_sfirst[number] = its first site
    nc = [1 if k == 0 or f["tgt"][k] != f["tgt"][k - 1] or f["pos"][k] != f["pos"][k - 1] + 1 else 0 for k in range(n)]
    off, _ = block_scan(nc, m["k_jn_stretch"])
    jn_run, sfirst = [0] * n, [stale] * (n + 1)
    for k in range(n):
        s = (off[k] + nc[k] - 1) % U32
        jn_run[k] = s
        if nc[k] and s <= n:
            sfirst[s] = k
    # k_jn_runs: a round loads 1,024 stretch numbers, then stores the run numbers over them
    rbeg, carry = [stale] * (n + 2), 0
    truth = None
    if mut == "run_for_stretch":
        truth = scans(exp)["jn_run"]
    for i0 in range(0, n, ROUND):
        if m["k_jn_runs"] == "carry_dropped" and i0:
            carry = 0
        head = []
        for k in range(i0, min(i0 + ROUND, n)):
            s = truth[k] if truth is not None and k >= ROUND else jn_run[k]
            fs = sfirst[s] if s <= k else k
            head.append(1 if fs > k or (k - fs) % jt.SITES == 0 else 0)
        acc, last_off = carry, carry
        for j, h in enumerate(head):
            k = i0 + j
            r = (acc + h - 1) % U32
            jn_run[k] = r
            if h and r <= n:
                rbeg[r] = k
            if k + 1 == n and r + 1 <= n + 1:
                rbeg[r + 1] = k + 1
            last_off = acc
            acc += h
        carry = acc if len(head) < ROUND else last_off + (0 if m["k_jn_runs"] == "carry_early" else head[-1])
    n_run = min(carry, n)
    out["jn_run"] = jn_run
    out["run_begin"] = rbeg[:n_run + 1]
    nd = f["jn_nd"] if jn_nd is None else jn_nd
    off, top = block_scan((list(nd) + [0] * n_run)[:n_run], m["k_jn_tscan"])
    out["jal_begin"] = off + [top]
    return out


def differs(exp, got):
    """Which of the twin's arrays `got` (scans) misses."""
    want = twin_arrays(exp)
    return [k for k in want if got[k] != want[k]]


def deep_list(lengths):
    """The deep list: the items above a wave's 64, here in ascending order (the device's order is the order of execution)."""
    return [k for k, d in enumerate(lengths) if d > WAVE]


def deep_trips(deep, nd, mut=None):
    """k_al_table_deep / k_jn_table_deep: block b builds the tables of list entries b, b + 1,024, ..; thread 0 clears s_nd
    in front of each, the heads are added to it and it is the table's length.  nd: the twin's table lengths, per item.
    Returns the lengths the device leaves for the listed items ({item: length}; an item no block reaches keeps 0)."""
    out = {k: 0 for k in deep}
    for b in range(min(GRID, len(deep))):
        s_nd = 0
        for trip, w in enumerate(range(b, len(deep), GRID)):
            if mut == "one_trip" and trip:
                break
            if not (mut == "stale_nd" and trip):
                s_nd = 0
            s_nd += nd[deep[w]]
            out[deep[w]] = s_nd
    return out


def with_trips(exp, mut=None):
    """scans with the deep sites' and deep runs' table lengths as deep_trips leaves them."""
    f = figures(exp)
    al_nd, jn_nd = list(f["al_nd"]), list(f["jn_nd"])
    for k, v in deep_trips(deep_list(f["depth"]), f["al_nd"], mut).items():
        al_nd[k] = v
    for r, v in deep_trips(deep_list(exp["spanning"]), f["jn_nd"], mut).items():
        jn_nd[r] = v
    return scans(exp, al_nd=al_nd, jn_nd=jn_nd)


def n2_of(depth, mut=None):
    n2 = N2_MIN
    while n2 < depth:
        n2 <<= 1
    if mut == "n2_small" and n2 > N2_MIN and depth == n2 // 2 + 1:
        n2 >>= 1
    return n2


def block_table(tab, mut=None):
    """The table a block builds from the keys of `tab` ([(key, count, ..)], the twin's): the first n2 places of the
    stretch are loaded, sorted by key, counted, and sorted by (count descending, key ascending)."""
    keys = [kk for kk, c, *_ in tab for _ in range(c)]
    return at.table(keys[:n2_of(len(keys), mut)])


def tables_with_cap(alns, min_len, trim, sites, cap=at.BASES):
    """Per site the counts of its alleles, descending, where a key holds `cap` bases and one bit for "longer"."""
    idx = {p: k for k, p in enumerate(sites)}
    per = [Counter() for _ in sites]
    for _, s0, q, t in srt.taken(alns, min_len, trim):
        tcs, _ = ev.coords(s0, t)
        for i in range(len(t)):
            if t[i] != ev.GAP and tcs[i] in idx:
                a = at.allele(q, t, i)
                per[idx[tcs[i]]][(a[:cap], len(a) > cap)] += 1
    return [sorted(c.values(), reverse=True) for c in per]


# ---- rounds: item 1,024 of the five scans ---------------------------------------------------------------------------------

PADS = (1008, 1016, 1023, 1024, 1025)
MAIN = 200
AROUND = range(1020, 1029)                             # the sites, by number, where one read shows another base
# the runs that hold items 1,023 and 1,024, and whether item 1,024 is a run's head
ROUNDS_WANT = {1008: (63, 64, True), 1016: (64, 64, False), 1023: (64, 64, False), 1024: (63, 64, True), 1025: (63, 64, True)}


@functools.lru_cache(maxsize=None)
def rounds(p):
    rng = np.random.default_rng(p)
    strings = []
    for first, n in ((0, p), (p, MAIN)):
        bb = _nonrep(rng, n)
        at_ = [g - first for g in AROUND if 0 <= g - first < n]
        strings.append((bb, [tsj._sub(bb, 0, n, [])] * 3 + ([tsj._sub(bb, 0, n, at_)] if at_ else [])))
    return _case("rounds%d" % p, strings, 3, 30, 0, (0, 0))


# ---- past_the_grid: more deep sites and deep runs than blocks -------------------------------------------------------------

GRID_LEN, GRID_READS = 2120, 65
GRID_SHORT = ((15, 2015), (215, 1815), (415, 1615), (615, 1415), (815, 1215))     # each begins on the middle site of a run of three and ends on the first of another
GRID_OPTS = (2, 200000)


def _grid_pair(j):
    return j % 100 == 7


@functools.lru_cache(maxsize=None)
def past_the_grid():
    """Even position x = 2 j in [10, 2110): of the 65 whole reads those with (r + j) % 3 == 0 show another base, less the
    last (j / 4) % 3 of them: 19 .. 22 reads.  What they show (one of the two bases that are neither the target's here nor
    its next, or nothing) depends on the read's rank among them and on j % 4: one other base (2 alleles); 16 and the rest
    another (3); 15, 3 and the rest, which delete the base (4); 14 and the rest, which delete it (3).  Where j % 100 == 7 the
    reads with (r + j) % 3 == 1 show another base at x + 1 as well: x, x + 1 and x + 2 are a run of three sites.  Five shorter reads, the
    target's own bases, nested inside one another, begin on the middle site of such a run and end on the first site of another."""
    bb = _nonrep(np.random.default_rng(GRID_LEN), GRID_LEN)
    q = [bytearray(bb) for _ in range(GRID_READS)]
    cuts = {0: (99, 99), 1: (16, 99), 2: (15, 18), 3: (14, 14)}

    def shown(x):
        # (another base is a deleted base and an inserted one: normalizeGaps would move it were it the target's next base)
        return [b for b in b"ACGT" if b not in (bb[x], bb[x + 1])] + [ev.GAP]
    for x in range(10, 2110, 2):
        j = x // 2
        d = [r for r in range(GRID_READS) if (r + j) % 3 == 0]
        d = d[:len(d) - (j // 4) % 3]
        c0, c1 = cuts[j % 4]
        for i, r in enumerate(d):
            q[r][x] = shown(x)[0 if i < c0 else 1 if i < c1 else 2]
        if _grid_pair(j):
            for r in range(GRID_READS):
                if (r + j) % 3 == 1:
                    q[r][x + 1] = shown(x + 1)[0]
    reads = [(1, bytes(r), bb) for r in q] + [tsj._sub(bb, s, e, []) for s, e in GRID_SHORT]
    return _case("past_the_grid", [(bb, reads)], 3, 30, 0, GRID_OPTS)


# ---- sort_sizes: every size of the block sort, from both sides ----------------------------------------------------------------

DEPTHS = tuple(d for k in range(7, 12) for d in (1 << k, (1 << k) + 1))     # 128, 129, 256, .. 2,048, 2,049
PATTERNS = ("distinct", "tied")
SORT_BB = tsj._capped(1)[0]
INS_AT = (2, 6, 10, 14, 18, 21, 25)                    # the bases of SORT_BB in front of a T: an inserted word over A C G stays there
SITE, OTHER_RUN = 10, (18, 21, 25)
WORDS7 = [bytes(w) for w in itertools.product(b"ACG", repeat=7)]
WORDS7_CG = [w for w in WORDS7 if w[0] != ord("A")]    # behind a deleted A: normalizeGaps would take a leading A for the base itself
WORDS3 = [b""] + [bytes(w) for w in itertools.product(b"ACG", repeat=3)][:13]     # a digit of base 14


def tied_sizes(depth):
    """Group sizes 1 1 2 2 .. g g B B that add up to `depth`, B the largest; at an odd depth a third group of 1.  g is 20 at
    the most, so that from depth 1,024 on B is more than 256."""
    odd = depth % 2
    g = 0
    while g < 20 and (g + 1) * (g + 2) + 2 * (g + 2) + odd <= depth:
        g += 1
    rest = depth - g * (g + 1) - odd
    sizes = [s for k in range(1, g + 1) for s in (k, k)] + [1] * odd + [rest // 2] * 2
    assert sum(sizes) == depth and rest // 2 > g
    return sizes


def _sort_read(ins, dele=()):
    q, t = bytearray(), bytearray()
    for x, b in enumerate(SORT_BB):
        q.append(ev.GAP if x in dele else b); t.append(b)
        w = ins.get(x, b"")
        q += w; t += b"-" * len(w)
    return (1, bytes(q), bytes(t))


@functools.lru_cache(maxsize=None)
def sort_sizes(pattern):
    """A target of SORT_BB per depth, every read whole.  distinct: read r inserts a seven-letter word of its own behind base
    10, the even reads the r / 2-th word, the odd ones the r / 2-th that does not begin with A, and those delete base 10 too
    (their words hang from base 9 in the consensus graph, which merges equal inserted bases group by group: half the
    group, a quarter of the time): as many alleles as reads at site 10, of the run [0, 16).  It writes its number as three digits of base 14 behind bases
    18, 21 and 25 (at most 14 alleles at each, so every nibble is an allele's own: as many joined keys as reads in the run
    [16, 30)).  tied: the reads in a shuffled order fall into groups of tied_sizes; group g inserts the g-th word behind
    base 10 and digit g % 14 behind base 18, but for the two largest, which show the bare base and no base at all (the graph
    of the consensus itself merges equal inserted bases group by group, and two groups of 814 equal words would take it
    seconds)."""
    assert all(SORT_BB[x + 1] == ord("T") for x in INS_AT) and {SITE} | set(OTHER_RUN) <= set(INS_AT)
    strings = []
    for depth in DEPTHS:
        if pattern == "distinct":
            reads = [_sort_read({SITE: (WORDS7_CG if r % 2 else WORDS7)[r // 2], 18: WORDS3[r % 14], 21: WORDS3[r // 14 % 14], 25: WORDS3[r // 196]},
                                {SITE} if r % 2 else ()) for r in range(depth)]
        else:
            group = np.repeat(np.arange(len(tied_sizes(depth))), tied_sizes(depth))
            group = group[np.random.default_rng(depth).permutation(depth)]
            last = len(tied_sizes(depth)) - 1
            reads = [_sort_read({}, {SITE} if g == last else ()) if g >= last - 1 else _sort_read({SITE: WORDS7[g], 18: WORDS3[g % 14]}) for g in group.tolist()]
        strings.append((SORT_BB, reads))
    return _case("sort_sizes_" + pattern, strings, 3, 5, 0, (0, 0))


# ---- key_length: the cap of 20 bases ------------------------------------------------------------------------------------------

KEY_TRIM = 2
KEY_SITE, KEY_END_SITE, KEY_SHORT = 62, 81, 84         # column 60 behind trim 2; the last site of the run [66, 82), in front of the last two bases of a read of 84
KEY_LANE = 60


@functools.lru_cache(maxsize=None)
def key_length():
    """100 bases over A C G with T at 63 and 82, under trim 2.  Behind base 62 (column 60 of every read: the 20 columns
    behind it cross the 64-column step) seven reads insert, S being 21 letters over A C G:
        S[:20], S[:19] + c, S[:21]     21, 21 and 22 bases with the column's own, the same first 20: one allele, bit 60
        S[:18] + d + S[19]             21 bases, another 20th: another allele, bit 60
        S[:19]                         20 bases, the first 20 of the three: a third allele, no bit 60
        S[:18], twice                  19 bases
    and three nothing.  Behind base 81 a read of 84 bases inserts 18 letters and one 25: trim 2 takes bases 82 and 83, the
    run's last column is the alignment's last, `hi` ends the look-ahead at 19 bases and at more than 20, and both reads
    span the run of sites [66, 82); a whole read inserts the same 18 letters, and a base ends its run."""
    rng = np.random.default_rng(20)
    bb = _nonrep(rng, 63, b"T") + b"T" + _nonrep(rng, 18, b"T") + b"T" + _nonrep(rng, 17, b"T")
    assert len(bb) == 100 and bb[KEY_SITE + 1] == bb[KEY_END_SITE + 1] == ord("T") and all(a != b for a, b in zip(bb, bb[1:]))
    S = bytes(rng.choice(np.frombuffer(b"ACG", np.uint8), 25))
    c, d = tsj._other(S[19]), tsj._other(S[18])                         # (A, or C for A: never T)

    def read(e, ins):
        q, t = bytearray(), bytearray()
        for x in range(e):
            q.append(bb[x]); t.append(bb[x])
            w = ins.get(x, b"")
            q += w; t += b"-" * len(w)
        return (1, bytes(q), bytes(t))
    words = [S[:20], S[:19] + bytes([c]), S[:21], S[:18] + bytes([d, S[19]]), S[:19], S[:18], S[:18], b"", b"", b""]
    reads = [read(100, {KEY_SITE: w}) for w in words]
    reads += [read(KEY_SHORT, {KEY_END_SITE: S[2:20]}), read(KEY_SHORT, {KEY_END_SITE: S[:25]}), read(100, {KEY_END_SITE: S[2:20]})]
    return _case("key_length", [(bb, reads)], 3, 30, KEY_TRIM, (0, 0))


# ---- which case must reject which wrong version ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("rounds"):
        return rounds(int(name[6:]))
    if name.startswith("sort_sizes_"):
        return sort_sizes(name[11:])
    return {"past_the_grid": past_the_grid, "key_length": key_length}[name]()


ROUND_CASES = tuple("rounds%d" % p for p in PADS)
# (mutation, scan) -> the cases that must reject it.  carry_early shows only where item 1,023 counts: every site has a depth
# and an allele, but only rounds1023 begins a stretch there (past_the_grid does too, but there a stretch numbered one too
# low still makes every site a head), and only it and past_the_grid a run
CARRY_REJECTS = {
    ("carry_dropped", "k_al_soff"): ROUND_CASES + ("past_the_grid",), ("carry_early", "k_al_soff"): ROUND_CASES + ("past_the_grid",),
    ("carry_dropped", "k_al_tscan"): ROUND_CASES + ("past_the_grid",), ("carry_early", "k_al_tscan"): ROUND_CASES + ("past_the_grid",),
    ("carry_dropped", "k_jn_stretch"): ROUND_CASES + ("past_the_grid",), ("carry_early", "k_jn_stretch"): ("rounds1023",),
    ("carry_dropped", "k_jn_runs"): ROUND_CASES + ("past_the_grid",), ("carry_early", "k_jn_runs"): ("rounds1023", "past_the_grid"),
    ("carry_dropped", "k_jn_tscan"): ("past_the_grid",), ("carry_early", "k_jn_tscan"): ("past_the_grid",),
}
# run_for_stretch, by what an unwritten word of jn_sfirst holds: 0 (a stretch that began at item 0: the heads fall on the
# multiples of 16, which is right where the pad is one) or a site behind the item (every item a head)
STRETCH_REJECTS = {0: ("rounds1016", "rounds1023", "rounds1025"), U32 - 1: ROUND_CASES}
