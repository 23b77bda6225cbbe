"""The fixed-size limits of the build stage (addAln on the device), each crossed on purpose (inputs and models: build_cases.py).

    structure (k_build.hip.h)                what lies behind it                                   crossed by
    DG_EB, 8 positions a batch               departure staged in s_D | stored straight to matD     batches: runs of 7, 8, 9, 17
                                             the loop past tlen, the exit first in its batch       batches: tlen + 1 = 8, 16
                                             the look-ahead that finds only deletions              batches, shift 4: ends in 1 .. 9 deleted
    DG_ECOLS 40 / DG_ENEED 16 columns        restage when a batch starts | inside a position       columns: runs of 23 .. 90 at phases 0, 1, 7
    1 << emit_shift positions a stretch      entry behind a match, d deletions, a run, enter;      stretches: edges 32, 48 (shift 4), 512
                                             ended, later; the look-ahead; waves that return
    the next read's cell | gcount            the insertion look-back of the target's last read     stretches, `groups` cell path
    DG_ERPW, 64 reads a wave                 byte cells | 32-bit cells | k_groups' prefix          every family on three cell paths
    the fold: 1 .. 3 bases, anchor owned,    no key: 4 bases, 16 positions, not owned, no          fold
    a backbone vertex, < 16 back             backbone vertex; chains split between two waves
    64 list entries on the lanes (k_lists)   the list in LDS; an entry found again on either       deep: 63 .. 66 and K + 1 entries
    1024 positions a pass (k_gscan)          s_carry                                               scans: tlen + 2 = 1023, 1024, 1025, 1040
    8 / 32 positions (k_groups), 4 (k_gsum)  the last wave, the vector and the scalar tail         scans: tlen + 2 = 33 .. 36
    1024 targets a pass (k_carve)            two carried sums, skipped targets count nothing       carve: 2049 targets

The first part runs on the CPU alone: it asserts on build_cases.Emit and build_cases.Lists -- k_emit's schedule and
k_lists' list construction restated over the columns -- that every family reaches what it is built to reach, and prints
the figures.  The GPU part sends every family through the three cell paths (byte cells, 32-bit cells after a re-run,
k_groups' prefix), at 16-position, 64-position and the default stretches, with every arena poisoned: the built graph,
the merged graph with the fold on and with it off against the oracle's, vertex by vertex and in list order, then the
consensus under three option sets.  All by equality; there is no tolerance anywhere.
"""
import collections

import pytest

import build_cases as bc
import oracle
from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs

gpu = pytest.mark.gpu
KNOBS = ("DAGCON_EMIT_SHIFT", "DAGCON_FOLD", "DAGCON_POISON", "DAGCON_MERGE_Q", "DAGCON_GCUTS")


def _sum(name, shift, scan=True):
    e = bc.emit(name, shift, scan)
    f = bc.merged([x.figures() for x in e])
    print(name, "shift", shift, "scan" if scan else "groups", f)
    return e, f


# ---- CPU: what every family reaches on the models ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(bc.FAMILIES))
def test_alignments_are_fixed_points_and_the_oracle_merges_them(name, oracle_lib):
    """Every constructed alignment is a fixed point of normalizeGaps (build_cases.target asserts it while it builds; here
    once more from the finished strings) and mergeNodes leaves no dangling vertex in any oracle graph.  carve: all but
    the non-conforming target, for which the oracle has no graph."""
    targets = bc.family(name)
    picked = [t for t in range(len(targets)) if name != "carve" or t != bc.CARVE_BAD]
    n = 0
    for i in picked:
        tlen, alns, _ = targets[i]
        g = oracle.Graph(blen=tlen)
        for s, q, t in alns:
            assert oracle.normalize_gaps(q, t) == (q, t)
            g.add_aln(s, q, t)
            n += 1
        assert g.merge_nodes() == 0
    print(name, len(targets), "targets,", n, "alignments checked")
    assert len(picked) == len(targets) - (name == "carve")


def test_batches_take_both_departure_routes_and_both_ways_to_the_exit():
    """tlen 6, 7, 8, 14, 15, 16, 17 (and 24, the shortest a deletion run of 17 fits into), 8 or 9 reads.  Measured at the
    default stretch: 1,136 departures staged in s_D, 186 stored straight (the anchor of a deletion run of 7 or more lies
    one or two batches back); the batch past tlen runs for tlen + 1 = 8 and 16, the exit its first position, and every
    read reaches the exit inside the loop.  At 16-position stretches: the exit of the 16-base targets is reached from the
    look-ahead of stretch 0, which finds nothing, 1, 2 or 9 deletions and no vertex (24 lanes), and for tlen + 1 = 16 the
    trailing runs bring stretch 1 to life, whose only batch starts on the exit."""
    e, f = _sum("batches", None)
    assert f["depart_lds"] > 0 and f["depart_direct"] > 0
    tlens = [t[0] for t in bc.family("batches")]
    tails = {T: x.tail for T, x in zip(tlens, e) if x.tail}
    assert set(tails) == {7, 15} and all(first for tl in tails.values() for _, first in tl)
    assert sum(x.exit_in_loop for x in e) == sum(x.K for x in e) and not f["ahead"]
    direct = {T: max(x.depart_direct for tt, x in zip(tlens, e) if tt == T) for T in tlens}
    assert direct[6] == 0 and direct[24] > 9                  # (one batch holds all of tlen 6; a run of 17 skips two)
    e4, f4 = _sum("batches", 4)
    ahead = collections.Counter()
    for x in e4:
        ahead.update(x.ahead)
    assert {("exit", 0), ("exit", 1), ("exit", 2), ("exit", 9)} <= set(ahead) and f4["ahead"]["exit"] == 24
    assert [x.tail for T, x in zip(tlens, e4) if T == 15] == [[(16, True)], []]
    assert f4["early"] > 0 and f4["entry"]["ended"] > 0 and f4["entry"]["del"] > 0


def test_columns_restage_at_the_designed_lengths():
    """Runs of 23, 24, 25, 39, 40, 41, 47, 48 and 90 columns whose first column has index 0, 1 and 7 modulo 8, in three
    places: in front of positions 17 and 33 of full-span reads, and in front of position 32 as the read's last base.  The
    last place is the clean one: at phase 0 the batch of position 32 restages when it starts, on the run's first column,
    so the 40 staged columns are the run's first 40.  Measured there, restages inside the position: L = 39: 0 (the match
    column is the 40th), L = 40: 1, L = 90: 2; phases 1 and 7: L = 25: 0, L = 39: 1.  In front of position 33: L = 25: 0,
    L = 39: 1 at phases 0 and 1.  A read with runs of 5 in front of eight positions in a row (48 columns in one batch)
    restages inside position 21.  At
    16-position stretches both kinds fire as well (20 and 63 times).  The last four reads: alignments of 49 and 55
    columns (hi = 1 and 7 modulo 8) with a run in front of the last column and with a trailing run."""
    e, f = _sum("columns", None)
    assert f["stage_batch"] > 0 and f["stage_column"] > 0
    counts = {}
    reads = [(t, r) for t in range(len(e)) for r in range(8)]
    places = [("at%d" % at, ph, L) for at in bc.COLUMN_AT for ph in bc.COLUMN_PHASES for L in bc.COLUMN_RUNS]
    places += [("last", ph, L) for ph in bc.COLUMN_PHASES for L in bc.COLUMN_RUNS]
    for key, (t, r) in zip(places, reads):
        counts[key] = (sum(1 for rr, _ in e[t].stage_batch if rr == r), sum(1 for rr, _ in e[t].stage_column if rr == r))
    for place in ("at17", "at33", "last"):
        for ph in bc.COLUMN_PHASES:
            print("columns", place, "phase", ph, [counts[place, ph, L] for L in bc.COLUMN_RUNS])
    assert [counts["last", 0, L][1] for L in bc.COLUMN_RUNS] == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    for ph in (1, 7):
        assert [counts["last", ph, L][1] for L in bc.COLUMN_RUNS] == [0, 0, 0, 1, 1, 1, 1, 1, 2]
    for ph in (0, 1):
        assert [counts["at33", ph, L][1] for L in bc.COLUMN_RUNS] == [0, 0, 0, 1, 1, 1, 1, 1, 2]
    assert all(counts["last", ph, L][0] == 1 for ph in bc.COLUMN_PHASES for L in bc.COLUMN_RUNS)
    t, r = reads[len(places)]
    assert [p for rr, p in e[t].stage_column if rr == r] == [21]
    ends = [bc.family("columns")[t][1][r] for t, r in reads[len(places) + 1:len(places) + 5]]
    assert [len(q) % 8 for _, q, _ in ends] == [1, 7, 1, 7]
    assert [t[-2:] for _, _, t in ends] == [b"-" + ends[0][2][-1:], b"-" + ends[1][2][-1:], b"--", b"--"]
    e4, f4 = _sum("columns", 4)
    assert f4["stage_batch"] > 0 and f4["stage_column"] > 0


def test_stretches_enter_and_leave_in_every_way():
    """Edges 32 and 48 of targets of 70 bases under 16-position stretches, edge 512 of a target of 1,038 bases under the
    default, targets with tlen + 1 = 15, 16, 17 and 511, 512, 513.  Measured at shift 4: lanes enter behind a match
    (2,490), behind 1 .. 33 deletions (57: runs of 15, 16, 17 and 33 that end before, on and behind an edge; 31 .. 33: the
    stretch in between holds nothing but the read's deletions), behind an insertion run and three deletions (8), behind
    enter and two deletions (3); 147 reads ended earlier, 142 start later, 965 stretch waves return at once.  The
    look-ahead finds a match, 1 .. 33 deletions and a match (44), a run, also behind two deletions (16), and nothing
    (exit: 9).  On the groups cell path the insertion look-back reads the next read's cell 4 times and gcount 4 times (the
    target's last read: two of the four in the targets built to end in the run and deletions read, asserted per target);
    at 64-position and default stretches once each, both in the long target, whose last read is built for it."""
    for shift in (4, 6, None):
        e, f = _sum("stretches", shift)
        ent, ah = collections.Counter(), collections.Counter()
        for x in e:
            ent.update(x.entry); ah.update(x.ahead)
        dels = {k[1] for k in ent if k[0] == "del"}
        assert {13, 14, 15, 16, 17, 31, 32, 33} <= dels
        assert ent["match",] > 0 and ent["ins", 3, "pfx"] > 0 and ent["ended"] > 0 and ent["later"] > 0 and ent["enter", 2] > 0
        assert f["early"] > 0
        assert {("match",), ("ins", 0), ("ins", 2), ("exit", 0), ("exit", 1)} <= set(ah) and {1, 2} <= {k[1] for k in ah if k[0] == "del"}
        if shift == 4:
            assert {15, 16, 17, 31, 32, 33} <= {k[1] for k in ah if k[0] == "del"}
        g = collections.Counter()
        for x in bc.emit("stretches", shift, False):
            g.update(x.entry)
        print("stretches shift", shift, "groups path: next", g["ins", 3, "next"], "gcount", g["ins", 3, "gcount"])
        assert g["ins", 3, "next"] > 0 and g["ins", 3, "gcount"] > 0
    # by design: of the two four-read targets at either edge the first ends in the plain run in front of the edge (its run
    # and deletions read is followed by another read), the second ends in the run and deletions read
    four = [x for x in bc.emit("stretches", 4, False) if x.K == 4 and x.tlen == 70]
    assert [(x.entry["ins", 3, "next"], x.entry["ins", 3, "gcount"]) for x in four] == [(1, 0), (0, 1)] * 2
    long = [x for x in bc.emit("stretches", None, False) if x.tlen == bc.STRETCH_LONG]
    assert [(x.entry["ins", 3, "next"], x.entry["ins", 3, "gcount"]) for x in long] == [(1, 1)]
    tl = [t[0] for t in bc.family("stretches")]
    assert {14, 15, 16, 510, 511, 512, bc.STRETCH_LONG} <= set(tl) and max(tl) + 2 == 1040


def test_fold_groups_and_the_chains_without_a_key():
    """17 targets of 50 and 60 bases.  Measured at the default stretch: 33 groups of two or more identical keys, of sizes 2
    (8), 3 (22) and 64 (3), at distances 1 (25), 2 (4), 3 (1) and 15 (3); position 24 of one target closes three groups
    at once; chains without a key: 73 of four bases (ACGT and CCGT at distance 2 among them: no group), 6 whose anchor
    lies 16 and 17 positions back, 2 behind an inserted vertex; identical chains in lanes 63 | 64, 0 | 127 and 5, 62 |
    65, 126 of 128 reads (a target of the deep family: more than a wave of reads) are split between two waves (3 keys;
    the last one is a group in either wave).  At 16-position
    stretches 15 chains are the first of a lane that entered at a checkpoint (anchor not owned), among them the chains
    in front of positions 16 and 32, whose twins in front of 18 and 35 do fold."""
    e, f = _sum("fold", None)
    sizes = collections.Counter(g[4] for x in e for g in x.groups)
    dist = collections.Counter(g[2] for x in e for g in x.groups)
    print("fold sizes", sorted(sizes.items()), "distances", sorted(dist.items()))
    assert set(sizes) == {2, 3, 64} and {1, 2, 3, 15} == set(dist)
    assert f["nokey"] == {"bases": 73, "far": 6, "not backbone": 2}
    # ACGT and CCGT at distance 2: four chains without a key at position 12, nothing else there, no group in the target
    acgt = [x for x, t in zip(e, bc.family("fold")) if any(b"ACGT" in q for _, q, _ in t[1])]
    assert len(acgt) == 1 and acgt[0].groups == [] and not acgt[0].keys
    assert sorted(acgt[0].nokey_at) == [(12, "bases", b"ACGT")] * 2 + [(12, "bases", b"CCGT")] * 2
    assert (0x41434754 | 2 << 24) == (0x43434754 | 2 << 24)                 # (what the keys would be without the guard)
    per_pos = collections.Counter((i, g[0]) for i, x in enumerate(e) for g in x.groups)
    assert max(per_pos.values()) == 3
    two = bc.emit("deep", None, False)[-1]
    assert two.K == 128 and sorted(two.split) == [(21, 1, b"TG"), (33, 1, b"G"), (40, 1, b"GG")]
    assert [(g[0], g[1], g[4]) for g in sorted(two.groups)] == [(40, 0, 2), (40, 1, 2)]
    bases = {g[3] for x in e for g in x.groups}
    assert {b"!", b"~", b"!~"} <= bases and not any(len(b) > 3 for b in bases)
    enter = [g for x in e for g in x.groups if g[0] == g[2]]                # distance == position: the anchor is enter
    assert {g[0] for g in enter} == {1, 2, 15}
    consecutive = [x for x in e if {30, 31} <= {g[0] for g in x.groups}]
    assert consecutive
    e4, f4 = _sum("fold", 4)
    assert f4["nokey"]["not owned"] == 15
    first = [x for x in e4 if x.tlen == 60][0]
    assert {g[0] for g in first.groups} == {18, 35} and first.nokey["not owned"] == 6


def test_deep_lists_on_both_sides_of_a_wave():
    """K = 65, 127, 128, 129 and 200 reads over 40 bases: the out list of position 9 and the in list of position 10 have
    K + 1 entries and move to LDS; four targets of 100 reads have exactly 63, 64, 65 and 66 entries there (the last two in
    LDS).  Behind position 20 read r deletes r % 15 bases: 15 lists whose entries recur in every group of 64 reads, found
    again on the lanes (254 times at K = 200).  130 reads, the first 61 with a run of their own in front of position 21:
    the out list of position 20 has 62 entries when the jumps begin, two of them find room on the lanes, the third moves the
    list to LDS inside the first group of reads, so its 14 recurrences are all found in LDS (the 14 found on the lanes belong
    to other lists of that target).  140 reads (build_cases.HAND_OVER): one list, the out list of position 20, that has 63
    entries after the first group of 64 reads, finds the jump over one base again on the lanes in the second group, moves
    to LDS there with its 65th entry, and finds three jumps again in LDS in the third group: 1 hit on the lanes, 3 in LDS, 66
    entries.  Hits are counted per read.  Every model length is the oracle's."""
    from test_gpu_parity import _oracle_graph
    targets = bc.family("deep")
    b = bc.case("deep", "groups").batch
    figs = []
    for i, (tlen, alns, _) in enumerate(targets):
        m = bc.Lists(tlen, alns)
        adj, _ = _oracle_graph(b, i, 0, 0, False)
        for (side, pos), n in m.lens.items():
            assert n == len(adj[pos][4 if side == "out" else 5]), (i, side, pos)
        figs.append((len(alns), m))
        print("deep K", len(alns), m.figures())
    for (K, m), want in zip(figs[:5], bc.DEEP_K):
        assert K == want and m.lens["out", 9] == m.lens["in", 10] == K + 1 and {("out", 9), ("in", 10)} == m.in_lds
        assert m.hits_lanes > 0 and len(m.recur) >= 2
    assert [m.lens["out", 9] for _, m in figs[5:9]] == [63, 64, 65, 66]
    assert [len(m.in_lds) for _, m in figs[5:9]] == [0, 0, 2, 2]
    last = figs[9][1]
    assert last.in_lds == {("out", 20)} and last.hits["out", 20] == [0, 14] and last.moved["out", 20] == (0, 64)
    assert last.hits_lanes == 14 and last.lens["out", 20] == 76
    K, hand = figs[10]
    assert K == 140 and hand.in_lds == {("out", 20)} and hand.moved["out", 20] == (1, 64)
    assert hand.hits["out", 20] == [1, 3] and hand.lens["out", 20] == 66
    e, f = _sum("deep", 4, False)
    assert f["groups"] > 0 and f["split"] > 0 and f["entry"]["idle"] > 0
    _sum("deep", None, False)


def test_scans_cross_their_passes():
    """tlen + 2 = 1023, 1024, 1025 (and 1040 in the stretches family) with runs in front of positions 1022 .. 1026 where
    they exist; tlen + 2 = 33 .. 36 with runs in front of the last three positions.  2,049 targets of 4 to 6 bases:
    vertices carried out of k_carve's first and second pass (printed), three targets below min_cov and one non-conforming
    target that count nothing, two whose reads are all below min_len."""
    tl = [t[0] + 2 for t in bc.family("scans")]
    assert tl == [1023, 1024, 1025, 33, 34, 35, 36]
    for tlen, alns, _ in bc.family("scans"):
        runs = {p for a in alns for p in _run_positions(a)}
        want = set(range(1022, 1027)) if tlen > 100 else set(range(tlen - 1, tlen + 2))
        assert runs == {p for p in want if p <= tlen + 1}
    tg = bc.family("carve")
    assert len(tg) == bc.CARVE_N == 2 * 1024 + 1
    skipped = set(bc.CARVE_INACTIVE) | {bc.CARVE_BAD}
    nodes = [0 if t in skipped else T + 2 + sum(len(_run_positions(a)) for a in alns if len(a[1]) >= bc.CARVE_OPTS["min_len"])
             for t, (T, alns, _) in enumerate(tg)]
    sums = [sum(nodes[:1024]), sum(nodes[:2048]), sum(nodes)]
    print("carve: vertices in front of target 1024, 2048, in all:", sums)
    assert 0 < sums[0] < sums[1] < sums[2] and sums[2] - sums[1] == nodes[2048] > 0
    assert all(len(tg[t][1]) == 1 for t in bc.CARVE_INACTIVE) and tg[bc.CARVE_BAD][1][0][0] == 0
    assert all(len(a[1]) < bc.CARVE_OPTS["min_len"] for t in bc.CARVE_SHORT for a in tg[t][1])
    assert all(len(tg[t][1]) == 3 and tg[t][0] >= 9 for t in bc.CARVE_MARKED)
    assert {t + 1 for t in skipped} <= set(bc.CARVE_GRAPHS) | skipped | {bc.CARVE_N}


def _run_positions(aln):
    """The position behind every inserted column of an alignment (one entry a column)."""
    s, q, t = aln
    out, pos = [], s
    for a, b in zip(q, t):
        if b == bc.GAP:
            out.append(pos)
        else:
            pos += 1
    return out


def test_every_setting_is_listed():
    """Three cell paths for every family but the ones that cannot take one: deep has more than 64 reads a target, and the
    2,049-target batch takes its 32-bit cells from the extra target alone, which is the same run as every other
    family's."""
    assert len(bc.SETTINGS) == sum(len(bc.SHIFTS[f]) * (3 - sum((f, c) in bc.LEFT_OUT for c in bc.CELLS)) for f in bc.FAMILIES)
    assert bc.LEFT_OUT == {("deep", "scan-byte"), ("deep", "scan-wide"), ("carve", "scan-wide")}
    for f in bc.FAMILIES:
        deepest = max(len(t[1]) for t in bc.family(f))
        assert (deepest > 64) == (f == "deep")
    assert len(bc.wide_extra()[1]) <= 64 and len(bc.wide_extra(255)[1]) <= 64 and len(bc.groups_extra()[1]) == 65
    assert max(len(q) for _, q, _ in bc.wide_extra(255)[1]) == max(len(q) for _, q, _ in bc.wide_extra()[1]) - 1
    assert any(len(q) >= 256 + 12 for _, q, _ in bc.wide_extra()[1])


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _set_env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _graph_run(factory, c, flags, merge, twice=False):
    """The context first runs a batch that sizes every arena: the batch itself, or on scan-wide its narrow twin (a run of
    255).  The re-runs counted afterwards then say which cells the batch took: none on scan-byte (no run outgrew a byte) and
    on groups, one on scan-wide, the one the run of 256 costs."""
    ctx = factory(flags=flags, **c.opts)
    try:
        ctx.consensus(c.batch if c.warm is None else c.warm, strict=not c.failed)
        assert ctx.timings()["reruns"] <= 1
        for nth in range(2 if twice else 1):
            ctx.consensus(c.batch, strict=not c.failed)
            tm = ctx.timings()
            # (scan-wide: the mark lasts while the same batch is uploaded again)
            assert tm["reruns"] == (1 if c.cells == "scan-wide" and nth == 0 else 0)
            assert sorted(t for t in range(c.batch.n_targets) if ctx.target_status[t]) == c.failed
            g = c.graphs[merge]
            _check_graphs(ctx, c.batch, 0, merge, targets=sorted(g), oracle_graphs=g)
    finally:
        ctx.close()
    return tm


STAGES = (("built", capi.FLAG_STOP_AFTER_BUILD, False, None), ("merged", capi.FLAG_STOP_AFTER_MERGE, True, None),
          ("merged, fold off", capi.FLAG_STOP_AFTER_MERGE, True, "0"))


@gpu
@pytest.mark.parametrize("name,cells,shift", bc.SETTINGS)
def test_family_in_every_setting(gpu_ctx_factory, monkeypatch, name, cells, shift):
    """A family on one cell path at one stretch length, every arena poisoned: the built graph (no fold by construction),
    the merged graph with the fold on and with it off, each against the oracle's vertex by vertex, in list order, with
    counts, weights, coverage and deleted flags; then the oracle's consensus under three option sets, fold on and off.
    The fold family runs every context twice on the same arenas.  The figures of each family are in the CPU tests above."""
    c = bc.case(name, cells)
    assert (c.max_k <= 64) == (cells != "groups")
    for stage, flags, merge, fold in STAGES:
        _set_env(monkeypatch, DAGCON_POISON=7, DAGCON_EMIT_SHIFT=shift, DAGCON_FOLD=fold)
        tm = _graph_run(gpu_ctx_factory, c, flags, merge, twice=(name == "fold"))
        print(name, cells, "shift", shift, stage, "reruns", tm["reruns"])
    for fold in (None, "0"):
        _set_env(monkeypatch, DAGCON_POISON=7, DAGCON_EMIT_SHIFT=shift, DAGCON_FOLD=fold)
        for opts, exp in zip(c.cns_opts, c.consensus):
            ctx = gpu_ctx_factory(**opts)
            try:
                got = ctx.consensus(c.batch, strict=not c.failed)
            finally:
                ctx.close()
            bad = [t for t in range(len(exp)) if got[t] != exp[t]]
            assert not bad, f"{name} {cells} shift {shift} fold {fold} {opts}: targets {bad[:8]}"
    assert sum(len(s) for segs in c.consensus[0] for _, _, s in segs) > 0
