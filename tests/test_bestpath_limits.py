"""The fixed-size limits of the bestPath sweeps, each crossed on purpose (inputs and model: bestpath_cases.py).

    structure (k_bestpath.hip.h)          what lies behind it                          crossed by
    DG_BOUT, 6 out-edges a staged slot    DG_BL_HBM: edges and terms from the pool     widths_row W = 6 | 7, 8, 9
    64 edges a round of a wave            the first maximum carried over, e0 += 64     widths_wave W = 64 | 65, 66, 70
    DG_BRW, 8 out-edges a row             the piece is marked, k_bp_sweep does it over widths_row W = 6, 7, 8 | 9
    DG_BL_STK, 16 stack entries a row     the same give-up                             suffix L = 14 .. 16 | 17, 18
    DG_BSTK, 64 stack entries in LDS      the gstk scratch                             suffix L = 62 .. 64 | 65, 66; waiters K >= 34
    DG_BFAR, 192 ids below the stream     the vertex waits                             suffix L = 189 .. 191 | 192 .. 194
    DG_BDEF, 32 waiters                   the far successor is chased after all        waiters K = 31, 32, 33 | 34, 40
    DG_BRR, a row's ring of 32 ids        flush, fence, score[] in HBM                 reach R + 1 = 31, 32 | 33, 34; suffix
    DG_BR, chunks of 64; DG_BRP           rscore of the resident chunk, else score[]   reach R + 1 = 63, 64 | 65, 66; suffix L >= 62
    DG_SR, the wave's ring of 256 ids     score[] in HBM                               reach R + 1 = 255, 256 | 257, 258; waiters
    the walk's prefetch, v + 192          the direct fetch of best[v] and the record   reach R + 1 = 191, 192 | 193, 194
    DG_WR, the walk's ring of 256         the same                                     reach R + 1 = 255, 256 | 257, 258
    v > 64 * cs + 512 (k_bp_walk_g)       the ring starts over                         reach R + 1 = 511, 512 | 513, 514, site on enter
    DG_BP_PIECES, 256 / 64 pieces         k_bp_join's s_off[257]                       pieces (the plan; see its test)
    DG_E_STACK raised by bestPath         the host grows stk_words and runs again      not reached: bestpath_cases' docstring

The first part runs on the CPU alone: it asserts on bestpath_cases.Sweep -- the sweeps' schedule restated over the
oracle's merged graph in device ids -- that every family reaches what it is built to reach, with members on both sides
of every limit, and prints the figures.  The GPU part sends every family through the wave kernels, the rows (with a
stack of 16, 1 and 0 entries), the whole-target sweep and the partial-span kernels, as one piece per target and in
pieces of four bases: the merged graph against the oracle's vertex by vertex (every buffer poisoned first), then the
consensus under two option sets, then weight, depth and position of every consensus base, which pin the path and not
its letters alone.  All by equality; there is no tolerance anywhere.
"""
import ctypes

import pytest

import bestpath_cases as bc
import merge_cases as mc
from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs

gpu = pytest.mark.gpu

ONE = dict(max_segments=1)
MANY = dict(max_segments=16, min_segment_len=4)
KNOBS = ("DAGCON_MERGE_Q", "DAGCON_GCUTS", "DAGCON_POISON", "DAGCON_BP_LANE", "DAGCON_BP_LANE_STACK", "DAGCON_BP_SEGS")
# kernel set: (environment, context flags, piece settings, the piece setting whose support and positions are checked)
KERNELS = {
    "waves": ({}, 0, (ONE, MANY), ONE),
    "rows": ({"DAGCON_BP_LANE": "2"}, 0, (ONE, MANY), ONE),
    "rows_stack0": ({"DAGCON_BP_LANE": "2", "DAGCON_BP_LANE_STACK": "0"}, 0, (ONE, MANY), MANY),
    "rows_stack1": ({"DAGCON_BP_LANE": "2", "DAGCON_BP_LANE_STACK": "1"}, 0, (ONE, MANY), MANY),
    "whole": ({}, capi.FLAG_DEBUG_RESWEEP, (MANY,), MANY),       # (k_bp_check returns at one piece)
    "partial": ({"DAGCON_GCUTS": "1"}, 0, (ONE, MANY), MANY),
}


# ---- CPU: what every family reaches on the model ------------------------------------------------------------------------

def _rows(name, labels, per):
    """The figures of a family, one printed line per dial value (per targets each: the insertion points); returns them
    as {label: [figures of each point]}."""
    c = bc.case(name)
    assert c.full_span and len(c.sweeps) == len(labels) * per
    out = {}
    for i, lab in enumerate(labels):
        figs = [s.figures() for s in c.sweeps[i * per:(i + 1) * per]]
        out[lab] = figs
        print(name, lab, {k: (v[0] if len(set(v)) == 1 else v) for k in figs[0] for v in [[f[k] for f in figs]]})
    return c, out


def test_suffix_crosses_the_row_stack_the_lds_stack_and_the_far_rule():
    """16 values of L at 6 insertion points (0: the chains hang on enter; 9 .. 12: every place relative to a cut of the
    four-base pieces; 20: the exit tree), 4 reads each.  Measured, the same at every point: exactly one turned-around
    edge, L + 1 ids back.  A row has L entries on its stack when it scores the last base of S: 14 .. 16 fit DG_BL_STK,
    17 and 18 do not.  A wave that chases has sp = L + 1, the stream's vertex included, L entries in S.stk / gstk:
    62 .. 64 stay in LDS, 65 puts its last entry into gstk[0], 66 one more.  The far rule:

        L      reach_back   max_sp   parked   max_waiting
        191    192          192      0        0           (never far: chased from the stream's vertex)
        192    193          194      1        1           (the second T waits; the first T, 192 above S[0], chases it all)
        193    194          3        2        3           (both wait; S[0] wakes them)
        194    195          3        2        3
    """
    c, rows = _rows("suffix", bc.SUFFIX_L, len(bc.SUFFIX_POINTS))
    for L, figs in rows.items():
        for f in figs:
            assert (f["turned"], f["reach_back"], f["chase_depth"]) == (1, L + 1, L)
            if L <= 191:
                assert (f["max_sp"], f["parked"], f["max_waiting"]) == (L + 1, 0, 0)
            elif L == 192:
                assert (f["max_sp"], f["parked"], f["max_waiting"]) == (194, 1, 1)
            else:
                assert (f["max_sp"], f["parked"], f["max_waiting"]) == (3, 2, 3)
            assert f["full_chase"] == 0 and f["max_out"] == 3
    depth = {L: rows[L][0]["chase_depth"] for L in rows}
    sp = {L: rows[L][0]["max_sp"] for L in rows}
    assert depth[16] == bc.DG_BL_STK and depth[17] == bc.DG_BL_STK + 1                  # a row's stack: full, one too many
    assert sp[64] - 1 == bc.DG_BSTK and sp[65] - 1 == bc.DG_BSTK + 1                      # S.stk full, gstk[0]
    assert rows[191][0]["reach_back"] == bc.DG_BFAR and rows[192][0]["reach_back"] == bc.DG_BFAR + 1
    assert max(s.live for s in c.sweeps) < 15000


def test_waiters_fill_the_wait_list_and_overflow_it():
    """K = 31, 32, 33, 34, 40 at 4 insertion points, K + 2 reads each.  Measured, the same at every point: K - 1 turned-around
    edges, up to 201 * (K - 1) ids back; the vertex in front has K + 1 out-edges.  Up to K = 33 every letter waits
    (K - 1 waiters: 30, 31, 32 = DG_BDEF) and nothing is chased.  At K = 34 the list is full when the stream reaches
    the second read's letter: it chases all of S, 200 entries on top of itself (sp 201, 136 of them in gstk), 8 of its
    misses far, and S[0] wakes the 32 on top of what is left; K = 40: 200 far misses chased.  A row chases 200 deep at
    every K and gives up."""
    c, rows = _rows("waiters", bc.WAITERS_K, len(bc.WAITERS_POINTS))
    for K, figs in rows.items():
        for f in figs:
            assert (f["turned"], f["max_out"], f["chase_depth"]) == (K - 1, K + 1, 200)
            assert f["reach_back"] > bc.DG_SR and f["max_waiting"] == min(K - 1, bc.DG_BDEF) == f["parked"]
            if K <= 33:
                assert f["full_chase"] == 0 and f["max_sp"] == K
            else:
                assert f["full_chase"] >= 1 and f["max_sp"] == 201 > bc.DG_BSTK + 1
    assert rows[33][0]["max_waiting"] == bc.DG_BDEF and rows[32][0]["max_waiting"] == bc.DG_BDEF - 1
    assert max(s.live for s in c.sweeps) < 15000 and max(s.n for s in c.sweeps) < 15000


@pytest.mark.parametrize("name", ["widths_row", "widths_wave"])
def test_widths_place_the_winner(name):
    """W - 1 one-letter insertions behind one base, every read deleting the next: an out list of exactly W entries, the
    backbone edge at index 0 (into a backbone vertex of weight 1: -10) and the letters at 1 .. W - 1 in read order.
    W = 6, 7 (DG_BOUT), 8, 9 (DG_BRW) at 6 insertion points, W = 64, 65, 66, 70 (a wave's round) at 4.  Per W
    (bestpath_cases.width_variants): one heavy letter at index 1, at W - 1 and on both sides of 6, 8 and 64 where the list
    is that long; two equally heavy letters that straddle each of those limits, their extra reads in both orders (the
    lower index wins); W >= 64: a letter at the last index that is heavy and still loses to index 0.  The index the
    oracle's best path takes at the site is asserted here, before any device runs: it is the one the variant was built
    for, and over the family it takes every value listed.  Measured: W = 65, 66 need 15 reads of one letter to beat the
    backbone edge (3d > W - 22); the family uses 17 where it has to win and 13 where it has to lose."""
    c = bc.case(name)
    specs = bc.width_specs(name)
    assert c.full_span and len(specs) == len(c.sweeps)
    won = {}
    for (W, heavy, d, wins, p), s, tg in zip(specs, c.sweeps, c.targets):
        site = [v for v in range(s.n) if s.out[v] is not None and len(s.out[v]) > 2]
        assert len(site) == 1 and s.max_out == W and len(s.out[site[0]]) == W
        assert len(tg[1]) == W - 1 + (d - 1) * len(heavy)
        got = s.choice(site[0])
        assert got == wins, (W, heavy, d, p, got)
        assert s.out[site[0]][0] == site[0] + len(tg[1]) + 1    # index 0 is the backbone edge, over every read's letter
        won.setdefault(W, set()).add(got)
    for W, idx in sorted(won.items()):
        print(name, "W", W, "winning indices", sorted(idx))
        assert {1, W - 1} <= idx and (W < 64 or 0 in idx)
        for lim in (bc.DG_BOUT, bc.DG_BRW, 64):
            if lim <= W - 1:
                assert {lim - 1, lim} <= idx
    assert all(s.turned == [] for s in c.sweeps)


def test_reach_crosses_the_rings_the_prefetch_and_the_jump():
    """One read with a run of R bases behind base p, three clean reads, R + 1 = 31 .. 34, 63 .. 66, 191 .. 194,
    255 .. 258, 511 .. 514 at 5 insertion points.  Measured: the backbone edge in front of the run reaches R + 1 ids
    ahead, and at every point but the last the best path takes it (path_jumps); behind the last base the run leads to
    exit for nothing (coverage 0 there) and the path walks all of it, R + 1 consecutive ids.  Runs of more than 255
    bases take the wide-cell re-run on the way (printed by the device tests)."""
    c, rows = _rows("reach", bc.REACH, len(bc.REACH_POINTS))
    for (R1, figs), i in zip(rows.items(), range(0, len(c.sweeps), len(bc.REACH_POINTS))):
        for p, f, s in zip(bc.REACH_POINTS, figs, c.sweeps[i:]):
            assert f["reach_fwd"] == R1 and f["turned"] == 0 and f["chase_depth"] == 0
            if p < 20:
                assert max(s.path_jumps) == R1 and s.path_jumps.count(R1) == 1
            else:
                assert set(s.path_jumps) == {1} and len(s.path) == 20 + R1 + 1
    for lim in (bc.DG_BRR, bc.DG_BR, bc.DG_BFAR, bc.DG_SR, bc.DG_WR, 512):
        assert {lim - 1, lim, lim + 1, lim + 2} <= set(bc.REACH)


def _plan(T, n_alns, sum_bb, partial, kw):
    lib = capi.load()
    lib.dagcon_debug_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * 4)()
    assert lib.dagcon_debug_plan(T, n_alns, sum_bb, partial, kw["max_segments"], kw.get("min_segment_len", 0), out) == 0
    return dict(seg_max=out[0], seg_min=out[1], use_q=out[2], bp_max=out[3])


def test_pieces_plan_saturates():
    """The planner's arithmetic for the `pieces` batch (one target, 1,200 bases, 6 reads, min_segment_len 4).  max_segments
    128 is clamped to the documented 64: 64 merge pieces, 192 bestPath pieces (64 on the partial-span path), so that
    setting stays short of DG_BP_PIECES.  The automatic setting (max_segments 0) gives 256 merge pieces and 256 bestPath
    pieces, DG_BP_PIECES, and 64 of each on the partial-span path; the device runs use both.  How many pieces k_cuts
    actually cuts for bestPath is not observable from outside (cuts_bp never leaves the device); the device test
    asserts merge_segments == 64 and == 256 as the sign that the merge's cuts, which come from the same candidates at
    the same spacing, saturate.  That they can: no two neighbouring bases are unmatched by some read, and k_cuts looks
    at two positions per cut at 256 pieces.  The settings of the other families: one piece, and 48 pieces for 16
    segments."""
    c = bc.case("pieces")
    assert c.full_span and c.batch.n_targets == 1 and c.batch.n_alns == 6
    for kw, partial, exp in ((bc.PIECES_CLAMPED, 0, (64, 4, 192)), (bc.PIECES_CLAMPED, 1, (64, 4, 64)),
                             (bc.PIECES_AUTO, 0, (256, 4, 256)), (bc.PIECES_AUTO, 1, (64, 4, 64))):
        pl = _plan(1, 6, 1202, partial, kw)
        print("pieces plan", kw, "partial-span", partial, pl)
        assert (pl["seg_max"], pl["seg_min"], pl["bp_max"]) == exp
    bad = bc.unmatched_bases(c.targets[0])
    print("pieces: bases some read does not match:", len(bad))
    assert len(bad) == 6 * 32 * 2 // 3                       # (32 sites a read; an insertion leaves every base matched)
    assert not any(b + 1 in bad for b in bad) and 1200 // 256 // 2 == 2
    assert _plan(96, 384, 96 * 22, 0, ONE)["bp_max"] == 1
    assert _plan(96, 384, 96 * 22, 0, MANY)["bp_max"] == 48
    assert all(bc.case(n).batch.n_targets < 256 for n in bc.ALL)           # (256 targets or more: 64 pieces at most)


def test_bestpath_cannot_outgrow_the_scratch_before_the_merge_does():
    """DG_E_STACK raised by bestPath is not reached (bestpath_cases' docstring has the argument).  Its premise, measured: on
    `nested`, the construction tried for a chase of many short merges under a full wait list, and on the deepest
    members of `suffix` and `waiters`, the wave's stack is never deeper than mergeInNodes' recursion (max_sp 201, 3
    and 201 against depths 201, 195 and 201), and a frame of that recursion behind the 48th costs 7 words of the
    scratch against one for a stack entry: a chase of DG_BSTK + 4096 + 1 entries needs 28,000 words in the merge first."""
    samples = [("nested", 0), ("suffix", len(bc.case("suffix").targets) - 1), ("waiters", len(bc.case("waiters").targets) - 1)]
    for name, i in samples:
        c = bc.case(name)
        s, m = c.sweeps[i], mc.measure(c.targets[i])
        print(name, i, s.figures(), m.figures())
        assert s.max_sp <= m.depth and s.chase_depth <= m.depth
        assert s.max_sp <= bc.DG_BSTK + bc.STK_WORDS and 7 * m.deep_groups <= bc.STK_WORDS
    n = bc.case("nested").sweeps[0]
    assert n.max_waiting == bc.DG_BDEF and n.full_chase >= 1 and n.max_sp > bc.DG_BSTK + 1
    assert 7 * (bc.DG_BSTK + bc.STK_WORDS + 1 - 48) > 4 * bc.STK_WORDS


@pytest.mark.parametrize("name", bc.ALL)
def test_oracle_answers_of_every_family(name, oracle_lib):
    """What the device runs below are held to: one segment per target under the plain options, at least as long as the
    target (the random pileup of `pieces`: less 60); weight, depth and position for every base of it."""
    c = bc.case(name)
    plain, trimmed = c.consensus
    print(name, "consensus bases:", sorted({sum(len(s[2]) for s in segs) for segs in plain}),
          "trim 2, min_weight 1:", sorted({sum(len(s[2]) for s in segs) for segs in trimmed}))
    assert len(plain) == len(trimmed) == c.batch.n_targets
    for t, segs in enumerate(plain):
        assert len(segs) == 1 and len(segs[0][2]) >= int(c.batch.tlen[t]) - (60 if name == "pieces" else 0)
    for opts, cns, ann in zip(bc.CNS_OPTS, c.consensus, c.annotated):
        for t in range(c.batch.n_targets):
            assert [x[:3] for x in ann[t]] == cns[t]
            assert all(len(x[3]) == len(x[4]) == len(x[5]) == len(x[2]) for x in ann[t])


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _set_env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph_run(factory, monkeypatch, c, env, flags, pieces):
    """The merged graph of every target against the oracle's, every buffer the kernels fill poisoned first: a wrong
    consensus below is then not the merge's doing.  Returns the run's timings."""
    _set_env(monkeypatch, DAGCON_POISON="15", **env)
    ctx = factory(flags=flags | capi.FLAG_STOP_AFTER_MERGE, **bc.GRAPH_OPTS, **pieces)
    try:
        ctx.consensus(c.batch)
        tm = ctx.timings()
        _check_graphs(ctx, c.batch, 0, True, oracle_graphs=c.graphs)
    finally:
        ctx.close()
    return tm


def _consensus_runs(factory, monkeypatch, c, env, flags, pieces):
    _set_env(monkeypatch, **env)
    reruns = []
    for opts, exp in zip(bc.CNS_OPTS, c.consensus):
        ctx = factory(flags=flags, **opts, **pieces)
        try:
            got = ctx.consensus(c.batch)
            reruns.append(ctx.timings()["reruns"])
        finally:
            ctx.close()
        bad = [t for t in range(len(exp)) if got[t] != exp[t]]
        assert not bad, f"{c.name} {env} flags {flags} {pieces} {opts}: targets {bad[:8]}"
    return reruns


def _annotated_runs(factory, monkeypatch, c, env, flags, pieces):
    """Weight, depth (FLAG_BASE_SUPPORT, against support_twin) and position (FLAG_BASE_POS, as test_windows.py checks it)
    of every consensus base, under both option sets."""
    _set_env(monkeypatch, **env)
    n = 0
    for opts, exp in zip(bc.CNS_OPTS, c.annotated):
        ctx = factory(flags=flags | capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS, **opts, **pieces)
        try:
            got = ctx.consensus(c.batch)
            pos, sup = ctx.base_positions(), ctx.base_support()
        finally:
            ctx.close()
        assert len(got) == len(pos) == len(sup) == len(exp)
        for t in range(len(exp)):
            assert got[t] == [x[:3] for x in exp[t]], f"{c.name} {env} {pieces} {opts}: target {t}"
            assert len(pos[t]) == len(sup[t]) == len(exp[t])
            for ps, (w, d), (_, _, seq, ep, ew, ed) in zip(pos[t], sup[t], exp[t]):
                assert ps.size == w.size == d.size == len(seq)
                assert ps.tolist() == ep, f"{c.name} {env} {pieces} {opts}: target {t}: positions"
                assert w.tolist() == ew and d.tolist() == ed, f"{c.name} {env} {pieces} {opts}: target {t}: support"
                n += len(seq)
    assert n > 0


@gpu
@pytest.mark.parametrize("kernels", sorted(KERNELS))
@pytest.mark.parametrize("name", bc.SWEPT)
def test_family_through_every_sweep(gpu_ctx_factory, monkeypatch, name, kernels):
    """Every family through the wave kernels (k_bp_sweep, k_bp_walk), the rows (k_bp_sweep_l, k_bp_walk_r; with a stack of
    16, 1 and 0 entries, so that every chase is at once the row's own, the row's first and k_bp_sweep's on top of what
    the row wrote), the whole-target sweep (k_bp_check's dg_bp_sweep_whole) and the partial-span kernels
    (dg_bp_sweep<true>, k_bp_comb, k_bp_abs, k_bp_choose, k_bp_walk_g), as one piece per target and in pieces of four
    bases: the oracle's merged graph first, then the oracle's consensus under the plain options and under trim 2 /
    min_weight 1, then at one piece setting weight, depth and position of every base.  The figures of each family are
    in the CPU tests above."""
    c = bc.case(name)
    env, flags, piece_settings, annotated = KERNELS[kernels]
    for pieces in piece_settings:
        tm = _graph_run(gpu_ctx_factory, monkeypatch, c, env, flags, pieces)
        if pieces is ONE:
            assert tm["merge_segments"] == c.batch.n_targets
        reruns = _consensus_runs(gpu_ctx_factory, monkeypatch, c, env, flags, pieces)
        print(name, kernels, pieces, "merge_segments", tm["merge_segments"], "reruns", tm["reruns"], reruns)
    _annotated_runs(gpu_ctx_factory, monkeypatch, c, env, flags, annotated)


@gpu
@pytest.mark.parametrize("kernels", sorted(KERNELS))
def test_pieces_saturate(gpu_ctx_factory, monkeypatch, kernels):
    """1,200 bases under 6 reads with min_segment_len 4, at max_segments 128 (clamped: 192 bestPath pieces planned) and at
    the automatic setting (256, DG_BP_PIECES: k_bp_join's s_off is full; 64 on the partial-span path, its own limit).
    The number of bestPath pieces is not observable from outside; merge_segments == 64 and == 256 on the full-span
    path say that the cuts saturate (test_pieces_plan_saturates).  Graph, consensus, support and positions as for every
    family."""
    c = bc.case("pieces")
    env, flags, _, _ = KERNELS[kernels]
    for pieces, nseg in ((bc.PIECES_CLAMPED, 64), (bc.PIECES_AUTO, 256)):
        tm = _graph_run(gpu_ctx_factory, monkeypatch, c, env, flags, pieces)
        reruns = _consensus_runs(gpu_ctx_factory, monkeypatch, c, env, flags, pieces)
        print("pieces", kernels, pieces, "merge_segments", tm["merge_segments"], "reruns", tm["reruns"], reruns)
        if kernels != "partial":
            assert tm["merge_segments"] == nseg
        _annotated_runs(gpu_ctx_factory, monkeypatch, c, env, flags, pieces)
