"""bestPath scores past 2^22 and 2^23: the bound on the pieces (dg_bp_exact), and the whole sweep behind it.

Stage (c) sweeps a target in concurrent pieces with relative fp32 scores.  That is the reference's sweep only while
every value is an exact multiple of 0.5, below 2^23; k_bp_check (full-span pileups) and k_bp_comb / k_bp_choose (partial
spans) hold the pieces to m + |above| + wmax < 2^22, and a target that fails is swept whole, in the reference's own
operations and order (dg_bp_sweep_whole).  Above 2^23 the reference's float rounding decides the path: the oracle (fp32,
as the reference) and its `wide` twin (double: exact arithmetic) give different consensus sequences, and a device that
stayed in pieces -- small, exact relative values -- would return the wide one.

The inputs are bound_cases.py's (families S, P, M; bands below, between, above).  The first part of this file runs on
the CPU alone and asserts that every input lies where its band says; the GPU tests take the oracle's results from the
same per-process cache.  Every device comparison is byte for byte against the fp32 oracle: there is no tolerance.
"""
import numpy as np
import pytest

import bound_cases as bc
import oracle
from pbdagcon_amd import capi, synth
from util import concat_batches, oracle_batch

gpu = pytest.mark.gpu
T22, T23 = bc.T22, bc.T23


# ---- CPU: the oracle's new entry point, and where each input lies -------------------------------------------------------

def test_stats_entry_point_is_the_default_path():
    """og_consensus_target_blob_stats in fp32 gives og_consensus_target_blob's segments (it is a second spelling of the
    same operations), and below 2^23 its wide mode gives them too, with the same scores: every value is exact there."""
    for b in (synth.make_batch(3, 1500, 24, seed=77), synth.make_batch(2, 2500, 40, seed=78, min_span=0.4)):
        exp = oracle_batch(b, **bc.OPTS)
        for t in range(b.n_targets):
            segs, st = bc.oracle_target(b, t)
            wsegs, wst = bc.oracle_target(b, t, wide=True)
            assert segs == exp[t] and wsegs == exp[t]
            assert st == wst and st["enter"] == st["max"] > 0.0 and st["min"] <= 0.0
            assert st["enter"] * 2 == int(st["enter"] * 2)
    a0, a1 = int(b.aln_begin[0]), int(b.aln_begin[1])
    args = (int(b.tlen[0]), b.aln_start[a0:a1].copy(), b.aln_off[a0:a1].copy(), b.aln_len[a0:a1].copy(), b.qstr, b.tstr)
    assert oracle.consensus_target_blob(*args, wide=True) == oracle.consensus_target_blob(*args)    # (wide without stats)


@pytest.mark.parametrize("family,band", sorted(bc.SIZES))
def test_input_lies_in_its_band(family, band):
    """s = the oracle's largest |score| (fp32 recurrence), K reads, L target bases; measured on the CPU:

        input       L      K    columns      s            oracle s   fp32 vs wide consensus
        S below     17300  501   8,737,300   4,070,193.5  0.34
        S between   17900  501   9,040,400   4,212,117.5  0.35
        S above     40000  501  20,203,000   9,438,838.0  0.75       40,010 / 40,012 bases, differ
        M below     23100  401   9,448,484   4,079,695.0  1.4
        M between   23800  401   9,734,807   4,203,977.0  1.4
        M above     53400  401  21,841,466   9,452,406.0  2.9        53,300 / 53,300 bases, equal (see below)
        P between   17300  651   9,028,412   4,198,040.0  0.38
        P above     39100  651  20,407,028   9,527,630.0  0.97       39,137 / 39,139 bases, differ

    below: 0.97 * 2^22 < s and s + K < 2^22.  between: 2^22 + K < s < 2^23 - K.  above: s > 2^23 + 2^20, and the
    oracle's consensus differs from its wide consensus -- but for family M, where it cannot: a plain pileup has no
    two candidates within 1 of each other (they differ by hundreds of reads), so rounding to a multiple of 1 decides
    nothing; M above has the magnitude, fp32 scores that differ from the exact ones (asserted), and the same path."""
    c = bc.case(family, band)
    print(c)
    assert 300 <= c.K <= 700 and c.columns < 30e6
    if band == "below":
        assert c.s > 0.97 * T22 and c.s + c.K < T22
    elif band == "between":
        assert T22 + c.K < c.s < T23 - c.K
    else:
        assert c.s > T23 + 2 ** 20
        print("wide:", c.wide_stats, [len(s[2]) for s in c.exp], [len(s[2]) for s in c.wide])
        assert c.wide_stats["enter"] != c.stats["enter"]            # the reference's rounding is at work
        if family != "M":
            assert c.wide != c.exp
            assert oracle_batch(c.batch, **bc.OPTS)[0] == c.exp     # ... and the stats entry point rounds as og_best_path does
    assert c.stats["enter"] == c.stats["max"]                       # the totals here are positive: see bound_cases.py
    assert len(c.exp) >= 1 and sum(len(s[2]) for s in c.exp) > 0.9 * c.L


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _run(batch, flags=0, max_segments=0):
    ctx = capi.Context(flags=flags, max_segments=max_segments, **bc.OPTS)
    try:
        return ctx.consensus(batch)
    finally:
        ctx.close()


def _check(got, c, what):
    """got (one target's segments) against the oracle's; says so when it is the wide answer instead."""
    ok = got == c.exp
    is_wide = c.wide is not None and got == c.wide
    assert ok, (f"{c.family} {c.band} {what}: consensus differs from the fp32 oracle"
                + (" and EQUALS the wide one: the device answered from pieces" if is_wide else "")
                + f"; lengths {[len(s[2]) for s in got]} against {[len(s[2]) for s in c.exp]}")


PLANS = {"default": dict(), "ms1": dict(max_segments=1), "ms8": dict(max_segments=8), "ms64": dict(max_segments=64),
         "resweep": dict(flags=capi.FLAG_DEBUG_RESWEEP)}


@gpu
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("band", ["below", "between", "above"])
@pytest.mark.parametrize("family", ["S", "M"])
def test_full_span_equals_oracle(family, band, plan):
    """k_bp_check's bound and dg_bp_sweep_whole: full-span targets under, between and over the two powers, under the
    default plan, at max_segments 1, 8 and 64 and with DAGCON_FLAG_DEBUG_RESWEEP."""
    c = bc.case(family, band)
    _check(_run(c.batch, **PLANS[plan])[0], c, plan)


@gpu
@pytest.mark.parametrize("max_segments", [0, 64])
@pytest.mark.parametrize("band", [b for f, b in sorted(bc.SIZES) if f == "P"])
def test_partial_span_equals_oracle(band, max_segments):
    """The partial-span machinery (p.gcuts): k_bp_comb's bound, k_bp_sweep_abs_g, k_bp_defer and k_bp_walk_g."""
    c = bc.case("P", band)
    _check(_run(c.batch, max_segments=max_segments)[0], c, f"max_segments={max_segments}")


@gpu
@pytest.mark.parametrize("variant", ["full_span", "gcuts"])
def test_one_target_resweeps_and_its_neighbours_do_not_notice(variant):
    """A small target, S above, another small target and S below in one batch: only S above has to be swept whole, and
    all four must equal the oracle -- twice, from the same context and upload.  gcuts: the second small target has
    partial spans, which puts the whole batch on the partial-span path.  timings()["reruns"] is printed, not asserted: a
    DG_E_STACK re-run of the whole sweep is legal."""
    above, below = bc.case("S", "above"), bc.case("S", "below")
    small = [synth.make_batch(1, 3000, 30, seed=4100),
             synth.make_batch(1, 5000, 40, seed=4200, min_span=0.5 if variant == "gcuts" else 1.0)]
    batch = concat_batches([small[0], above.batch, small[1], below.batch])
    exp = [oracle_batch(small[0], **bc.OPTS)[0], above.exp, oracle_batch(small[1], **bc.OPTS)[0], below.exp]
    ctx = capi.Context(**bc.OPTS)
    try:
        ctx.upload(batch)
        got = []
        for _ in range(2):
            ctx.run()
            got.append(ctx.fetch())
            print(variant, "reruns:", ctx.timings()["reruns"])
    finally:
        ctx.close()
    for i, g in enumerate(got):
        _check(g[1], above, f"{variant} run {i}")
        _check(g[3], below, f"{variant} run {i}")
        ok0, ok2 = g[0] == exp[0], g[2] == exp[2]
        assert ok0 and ok2, f"{variant} run {i}: the small neighbours of a target swept whole differ from the oracle ({ok0}, {ok2})"
    same = got[0] == got[1]
    assert same, f"{variant}: the second run of the same upload differs from the first"


@gpu
@pytest.mark.parametrize("stack", [None, "0", "1"])
def test_row_kernels_hand_their_target_to_the_check(stack, monkeypatch):
    """S above with DAGCON_BP_LANE=2: k_bp_sweep_l / k_bp_walk_r rows, whose target k_bp_check then sweeps whole; and
    with DAGCON_BP_LANE_STACK=0 / 1 (the values of test_round3_paths_and_their_checkers_agree), where rows give pieces
    up to k_bp_sweep first."""
    monkeypatch.setenv("DAGCON_BP_LANE", "2")
    if stack is not None:
        monkeypatch.setenv("DAGCON_BP_LANE_STACK", stack)
    c = bc.case("S", "above")
    _check(_run(c.batch)[0], c, f"DAGCON_BP_LANE=2 DAGCON_BP_LANE_STACK={stack}")


@gpu
def test_support_and_positions_of_a_target_swept_whole():
    """S above with FLAG_BASE_SUPPORT | FLAG_BASE_POS.  This is device against device: the Python twins of the
    annotations are too slow at this size, so the default plan (pieces, then the whole sweep, then the walks over the
    pieces) is compared with max_segments=1 (one piece from the start).  Both consensus results must equal the
    oracle's; base_support() and base_positions() of the two runs must be equal."""
    c = bc.case("S", "above")
    out = []
    for ms in (0, 1):
        ctx = capi.Context(flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS, max_segments=ms, **bc.OPTS)
        try:
            got = ctx.consensus(c.batch)
            out.append((got, ctx.base_support(), ctx.base_positions()))
        finally:
            ctx.close()
        _check(got[0], c, f"support max_segments={ms}")
    (_, sup0, pos0), (_, sup1, pos1) = out
    assert len(sup0[0]) == len(sup1[0]) == len(c.exp) and len(pos0[0]) == len(pos1[0]) == len(c.exp)
    for s in range(len(c.exp)):
        n = len(c.exp[s][2])
        assert sup0[0][s][0].size == n and pos0[0][s].size == n
        assert np.array_equal(sup0[0][s][0], sup1[0][s][0]), f"segment {s}: weights differ between the plans"
        assert np.array_equal(sup0[0][s][1], sup1[0][s][1]), f"segment {s}: depths differ between the plans"
        assert np.array_equal(pos0[0][s], pos1[0][s]), f"segment {s}: positions differ between the plans"
        assert int(sup0[0][s][1].max()) <= c.K and int(sup0[0][s][0].min()) >= bc.OPTS["min_cov"]
        assert int(pos0[0][s].max()) <= c.L and np.all(np.diff(pos0[0][s].astype(np.int64)) >= 0)
