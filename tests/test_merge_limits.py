"""The fixed-size limits of the mergeNodes sweeps, each crossed on purpose (inputs: merge_cases.py).

k_merge, k_merge_q and the partial-span dg_merge_segment<true> (k_merge_pro / k_merge_list / k_merge_fin) each keep
48 recursion frames, a ring of the youngest queue entries and a list per row or wave on chip, with a second path behind
every one of them; the literal path behind the frames has a scratch of stk_words and a re-run behind that; the host
picks the kernels by a span rule that is necessary, not sufficient.  The first part of this file runs on the CPU alone:
it asserts, on oracle/pymodel.py's AlnGraph with counters, that every family reaches what it is built to reach, prints
the figures, and records the oracle's consensus.  The GPU part sends every family through every kernel, as one piece
per target and in pieces of four bases, and compares the merged graph with the oracle's vertex by vertex and in list
order (every buffer poisoned first), then the consensus, by equality.  There is no tolerance anywhere.

Which kernel sweeps a batch: a full-span batch with max_segments set goes to k_merge_q, whatever its depth (q_kmax is 0
then), with DAGCON_MERGE_Q=0 to k_merge; DAGCON_GCUTS=1 sends it to the partial-span kernels.  One exception:
max_segments=1 plans one piece per target and the planner gives that to k_merge (dg_plan_pieces: use_q only where
seg_max != 1), so k_merge_q's own one-piece sweep -- the one in which the FIFO occupancies below hold for its ring -- is
run with max_segments=2 and a min_segment_len no target reaches (Q_ONE), next to the two settings every kernel gets.
"""
import ctypes

import pytest

import merge_cases as mc
from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs

gpu = pytest.mark.gpu

KERNELS = {"k_merge": {"DAGCON_MERGE_Q": "0"}, "k_merge_q": {}, "partial": {"DAGCON_GCUTS": "1"}}
ONE = dict(max_segments=1)
MANY = dict(max_segments=16, min_segment_len=4)
Q_ONE = dict(max_segments=2, min_segment_len=1 << 20)
KNOBS = ("DAGCON_MERGE_Q", "DAGCON_GCUTS", "DAGCON_POISON", "DAGCON_BP_LANE")


def _pieces(kernel):
    return (ONE, MANY, Q_ONE) if kernel == "k_merge_q" else (ONE, MANY)


# ---- CPU: what every family reaches on the model, and what the oracle makes of it -----------------------------------

def _figures(name):
    c = mc.case(name)
    figs = [m.figures() for m in c.measured]
    for k in figs[0]:
        vals = [f[k] for f in figs]
        print(f"{name}: {k} = {vals[0] if len(set(vals)) == 1 else vals}"
              + (f" (all {len(vals)} targets)" if len(set(vals)) == 1 and len(vals) > 1 else ""))
    assert all(mc.host_full_span(t) for t in c.targets) == (name != "partial")
    return c, figs


def test_deep_hands_over_at_frame_48():
    """25 targets of 24 bases, the runs behind base 0 .. 24, 9 reads each.  Measured on the model, the same at every
    insertion point: mergeInNodes 61 frames deep, 12 groups merged in frames past 48 (one of them the second group of
    frame 51), 1 visit whose own frame merges two groups (T waits while G goes deep); lists with a group are 8 long on
    either side, the FIFO holds 7."""
    c, figs = _figures("deep")
    assert len(figs) == 25
    for f in figs:
        assert f["depth"] >= 49 and f["deep_groups"] >= 1 and f["top_multi"] >= 1


def test_stack_outgrows_the_scratch_and_its_control_does_not():
    """4 reads on 20 bases.  Measured: recursion 1001 deep with 952 groups past frame 48, each a literal frame of
    3 + 2 * 2 = 7 words: 6664 words, more than the 4096 of a small batch and less than the 16384 of its re-run.  The
    control, two unshared runs of the same 1002 bases: depth 1, no group at all."""
    c, figs = _figures("stack")
    assert figs[0]["depth"] >= 1001 and 7 * figs[0]["deep_groups"] > 4096 and 7 * figs[0]["depth"] < 4 * 4096
    _, ctl = _figures("stack_control")
    assert ctl[0]["depth"] == 1 and ctl[0]["in_len"] == ctl[0]["out_len"] == 0
    assert [len(a[1]) for a in c.targets[0][1]] == [len(a[1]) for a in mc.case("stack_control").targets[0][1]]


@pytest.mark.parametrize("name", sorted(mc.FANS))
def test_fans_pass_the_rings(name):
    """A read per word behind one base.  Measured on the model, at every insertion point: FIFO occupancy = reads, and both
    the in list and the out list in which groups are merged = reads + 1:

        fan32   GT^5     32 reads   occupancy  32   lists  33     25 insertion points    passes DQ_RING (16)
        fan27   GTN^3    27 reads   occupancy  27   lists  28     25 insertion points    passes DQ_RING; leaves over lists of 3
        fan512  GT^9    512 reads   occupancy 512   lists 513     points 0, 12, 24       passes DG_QRING (256)
        fan400  20^2    400 reads   occupancy 400   lists 401     points 0, 12, 24       passes DG_QRING; bases beyond ACGTN

    (occupancy: with the target as one piece, hence the one-piece device runs)."""
    c, figs = _figures(name)
    letters, levels = mc.FANS[name]
    reads = len(letters) ** levels
    assert len(figs) == (3 if reads > 256 else 25)
    for f in figs:
        assert f["occupancy"] > mc.FAN_RING[name]
        assert f["occupancy"] == reads and f["in_len"] == f["out_len"] == reads + 1


def test_widths_are_exact():
    """Lists with a group of exactly 4, 5 (a row's one-look half and one more), 8, 9 (a row), 32, 33 (a wave's one-look half,
    and the longest in list dg_visit_merging takes on a wave, DgWave::IN_W), 64, 65 (a wave) entries, once on the in side
    with nothing to merge
    on the out side and once the other way round.  Measured: the longest list with a group is the width, on its side;
    the other side merges no group at all."""
    c, figs = _figures("widths")
    assert len(figs) == 2 * len(mc.WIDTHS)
    for i, L in enumerate(mc.WIDTHS):
        assert (figs[2 * i]["in_len"], figs[2 * i]["out_len"]) == (L, 0)
        assert (figs[2 * i + 1]["in_len"], figs[2 * i + 1]["out_len"]) == (0, L)
    assert max(len(t[1]) for t in c.targets) == 64


def test_span_pretenders_pass_the_host_rule():
    """Four targets of 120 bases, six true full-span reads each and one to four reads that start at 1, have 120 columns or
    more, and leave the backbone at base 70, 65 or 60 or enter it at base 31.  Measured: groups in lists of 4 - 6, and in
    the last target mergeInNodes(exit) 31 frames deep (the two trailing runs share 30 bases).  The partial batch: two
    targets, eight reads that start at bases 5 .. 40; groups in in lists of 5 and out lists of 9."""
    c, figs = _figures("span")
    for tlen, alns, _ in c.targets:
        assert all(s == 1 and len(q) >= tlen for s, q, _ in alns)
        assert any(mc.last_base(a) < tlen - 20 for a in alns)
        assert sum(mc.last_base(a) == tlen for a in alns) >= 6
    assert figs[3]["depth"] >= 31
    p, pf = _figures("partial")
    assert sorted({a[0] for t in p.targets for a in t[1]}) == list(range(5, 41, 5))
    assert all(f["in_len"] >= 2 and f["out_len"] >= 2 for f in pf)


def test_depths_lie_around_the_row_sweeps_limit():
    """Twelve random full-span pileups at 41 .. 70 reads: four at 53 or fewer (k_merge_q's own range: DQ_KMAX is 52), four
    at 54 .. 64, four at 65 .. 70 (a list longer than a wave).  Measured: out lists with a group of 18 .. 68 entries, in
    lists of up to 15, recursion up to 3 deep."""
    c, figs = _figures("depths")
    ks = [len(t[1]) for t in c.targets]
    assert ks == list(mc.DEPTHS) and all(20 <= t[0] <= 100 for t in c.targets)
    assert sum(k <= 53 for k in ks) >= 2 and sum(53 <= k <= 64 for k in ks) >= 2 and sum(k >= 65 for k in ks) >= 2
    assert max(f["out_len"] for f in figs) > 64 and min(f["out_len"] for f in figs) <= 32


@pytest.mark.parametrize("name", mc.ALL)
def test_oracle_consensus_of_every_family(name, oracle_lib):
    """What the device runs below are held to: one segment per target under the plain options (shorter than the target
    only where most reads delete bases: the in-side widths), and the model's merged graph equal to the oracle's wherever
    the model was run."""
    c = mc.case(name)
    plain, trimmed = c.consensus
    print(name, "consensus bases:", [sum(len(s[2]) for s in segs) for segs in plain],
          "trim 2, min_weight 1:", [sum(len(s[2]) for s in segs) for segs in trimmed])
    assert len(plain) == len(trimmed) == c.batch.n_targets
    for t, segs in enumerate(plain):
        assert len(segs) == 1 and len(segs[0][2]) >= (int(c.batch.tlen[t]) if name not in ("widths", "depths") else 14)
    if name != "depths":
        for t, m in enumerate(c.measured):
            assert m.adjacency() == c.graphs[t][0], f"{name} target {t}"


def test_one_piece_goes_to_k_merge_and_q_one_to_k_merge_q():
    """The planner's choice (host arithmetic, dagcon_debug_plan): max_segments=1 on a full-span batch is k_merge's, MANY and
    Q_ONE are k_merge_q's."""
    lib = capi.load()
    lib.dagcon_debug_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * 4)()
    for kw, seg_max, use_q in ((ONE, 1, 0), (MANY, 16, 1), (Q_ONE, 2, 1)):
        for T, k in ((25, 9), (3, 512), (12, 70)):
            assert lib.dagcon_debug_plan(T, T * k, T * 28, 0, kw["max_segments"], kw.get("min_segment_len", 0), out) == 0
            assert (out[0], out[2]) == (seg_max, use_q), (kw, list(out))


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _set_env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _graph_run(factory, monkeypatch, c, env, pieces):
    """The merged graph of every target against the oracle's, every buffer the kernels fill poisoned first.  Returns the
    run's timings."""
    _set_env(monkeypatch, DAGCON_POISON="15", **env)
    ctx = factory(flags=capi.FLAG_STOP_AFTER_MERGE, **mc.GRAPH_OPTS, **pieces)
    try:
        ctx.consensus(c.batch)
        tm = ctx.timings()
        _check_graphs(ctx, c.batch, 0, True, oracle_graphs=c.graphs)
    finally:
        ctx.close()
    return tm


def _consensus_runs(factory, monkeypatch, c, env, pieces, lanes=(None,)):
    for lane in lanes:
        _set_env(monkeypatch, **env, **({} if lane is None else {"DAGCON_BP_LANE": lane}))
        for opts, exp in zip(mc.CNS_OPTS, c.consensus):
            ctx = factory(**opts, **pieces)
            try:
                got = ctx.consensus(c.batch)
            finally:
                ctx.close()
            bad = [t for t in range(len(exp)) if got[t] != exp[t]]
            assert not bad, f"{c.name} {env} {pieces} {opts} BP_LANE={lane}: targets {bad[:8]}"


@gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", mc.SWEPT)
def test_family_through_every_kernel(gpu_ctx_factory, monkeypatch, name, kernel):
    """Every family through k_merge, k_merge_q and the partial-span kernels, as one piece per target and in pieces of four
    bases (the insertion point slides over the whole target, so the construction meets a cut vertex in every way: just
    before it, on it, just behind it, inside a piece; point 0 hangs the chains on enter, point tlen is mergeInNodes(exit),
    k_merge_fin and k_bp_xtree): the oracle's merged graph, vertex by vertex and in list order, then the oracle's
    consensus under the plain options and under trim 2 / min_weight 1.  All branches of a fan weigh the same, so its
    consensus is a tie-order test of bestPath too: the fans also run with DAGCON_BP_LANE 0 and 2.  The figures of each
    family are in the CPU tests above."""
    c = mc.case(name)
    n = c.batch.n_targets
    env = KERNELS[kernel]
    for pieces in _pieces(kernel):
        tm = _graph_run(gpu_ctx_factory, monkeypatch, c, env, pieces)
        print(name, kernel, pieces, "merge_segments", tm["merge_segments"], "reruns", tm["reruns"])
        if pieces is not MANY:
            assert tm["merge_segments"] == n
        elif kernel != "partial" and name != "depths":       # (a random deep pileup has no base that every read matches)
            assert tm["merge_segments"] > 2 * n              # the cuts were really used
        _consensus_runs(gpu_ctx_factory, monkeypatch, c, env, pieces,
                        lanes=(None, "0", "2") if name in mc.FANS else (None,))


def _reruns_twice(factory, batch, exp, opts, pieces):
    """The re-runs of a first and of a second consensus of the batch on one fresh context, both held to exp."""
    ctx = factory(**opts, **pieces)
    try:
        assert ctx.consensus(batch) == exp
        first = ctx.timings()["reruns"]
        assert ctx.consensus(batch) == exp
        return first, ctx.timings()["reruns"]
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_stack_rerun(gpu_ctx_factory, monkeypatch, kernel):
    """The literal path behind frame 48 outgrows stk_words (some 950 frames of 7 words against 4096), raises DG_E_STACK, the
    host grows the scratch by four and runs the batch again: the oracle's graph and consensus, on a fresh context, with
    more re-runs than the control needs on another fresh context (its runs are as long -- the wide-cell re-run -- and
    share nothing).  The context keeps the larger scratch, and the 32-bit run cells for a batch that shows a run of more
    than 255 gap columns in its strings: a second consensus gives the same answer with reruns == 0, the control's too.
    Measured, every kernel and piece setting: 3 re-runs against the control's 2, then 0 and 0.  (A batch without such a
    run gets byte cells again: test_run_cells.py::test_wide_batch_then_narrow_batch.)"""
    c, ctl = mc.case("stack"), mc.case("stack_control")
    env = KERNELS[kernel]
    for pieces in _pieces(kernel):
        tm = _graph_run(gpu_ctx_factory, monkeypatch, c, env, pieces)
        tm_ctl = _graph_run(gpu_ctx_factory, monkeypatch, ctl, env, pieces)
        print(kernel, pieces, "graph run: reruns", tm["reruns"], "control", tm_ctl["reruns"])
        assert tm["reruns"] > tm_ctl["reruns"]
        _set_env(monkeypatch, **env)
        for opts, exp, exp_ctl in zip(mc.CNS_OPTS, c.consensus, ctl.consensus):
            first, second = _reruns_twice(gpu_ctx_factory, c.batch, exp, opts, pieces)
            first_ctl, second_ctl = _reruns_twice(gpu_ctx_factory, ctl.batch, exp_ctl, opts, pieces)
            print(kernel, pieces, opts, "reruns", (first, second), "control", (first_ctl, second_ctl))
            assert first > first_ctl
            assert second == 0 and second_ctl == 0


@gpu
@pytest.mark.parametrize("merge_q", [None, "0"])
def test_span_rule_from_both_sides(gpu_ctx_factory, monkeypatch, merge_q):
    """Reads that pass the host's rule and are not full-span (they leave the backbone early behind long runs, or enter it at
    base 31) on the full-span kernels, which is what the host chooses for them (DAGCON_GCUTS unset, and 0), and on the
    partial-span kernels (1); reads that start at bases 5 .. 40 on the partial-span kernels (1) and on the full-span ones
    (0), where k_cuts' `weight - 1 == reads threaded` is all that keeps a cut away from a base some read does not pass.
    Every run: the oracle's graph and consensus.  The unset run cuts as the 0 run does."""
    for name, settings in (("span", (None, "0", "1")), ("partial", ("0", "1"))):
        c = mc.case(name)
        for pieces in (ONE, MANY) + ((Q_ONE,) if merge_q is None else ()):
            nseg = {}
            for gc in settings:
                env = {} if gc is None else {"DAGCON_GCUTS": gc}
                if merge_q is not None:
                    env["DAGCON_MERGE_Q"] = merge_q
                nseg[gc] = _graph_run(gpu_ctx_factory, monkeypatch, c, env, pieces)["merge_segments"]
                _consensus_runs(gpu_ctx_factory, monkeypatch, c, env, pieces)
            print(name, "DAGCON_MERGE_Q", merge_q, pieces, "merge_segments", nseg)
            if name == "span":
                assert nseg[None] == nseg["0"]
            if pieces is not MANY:
                assert set(nseg.values()) == {c.batch.n_targets}
