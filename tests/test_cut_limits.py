"""Every cut condition and limit of the partial-span merge, crossed on purpose (inputs and models: cut_cases.py).

k_readspan, k_merge_pro, k_cuts2 and k_merge_fin decide where a partial-span pileup may be cut.  The first part of this
file runs on the CPU alone: it asserts, on cut_cases' models, that every family has the one admissible position it is
built to have, on either side of its rule, prints the figures, holds every predicted merge row to `sound` (the check
that does not restate the kernel), and shows that each of eight wrong versions of the rule is rejected by a family.
The GPU part reads the device's cuts from a DAGCON_DUMP and compares them with the model's, vertex for vertex, then the
merged graph and the consensus with the oracle's, by equality.  The device only ever runs the committed code: no
mutation is run on it.
"""
import ctypes

import pytest

import cut_cases as cc
from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs

gpu = pytest.mark.gpu
KNOBS = ("DAGCON_MERGE_Q", "DAGCON_GCUTS", "DAGCON_POISON", "DAGCON_BP_LANE", "DAGCON_BP_SEGS", "DAGCON_DUMP")
FAMS = tuple(f for f in cc.FAMILIES if f != "fullspan")


def _settings(c):
    return [c.pieces] + [s for s in cc.SETTINGS if s != c.pieces]


# ---- CPU: the models, the families' figures, the mutations ----------------------------------------------------------------

def test_spans_by_meaning_and_by_the_kernels_loops():
    """k_readspan's two loops against the meaning of its four figures, on every read of every family, and the figures of the
    three reads the lead family is built around.  The backward loop's `k > i + 1` never decides: column i is the first
    match column, so the loop would stop on it anyway (a read whose only match column is its first: trail and tdels count
    every column behind it)."""
    n = 0
    for f in cc.FAMILIES:
        for c in cc.family(f):
            for a in c.target[1]:
                assert cc.spans(a) == cc.spans_kernel(a), (c.name, a)
                n += 1
    print("reads compared:", n)
    c = {x.name: x for x in cc.family("lead")}["lead7_above"]
    print("lead7_above spans (s, e, lead, trail):", c.pile.spans)
    # leading run of 7 interrupted by two deletions: rd_s advances by them, lead counts the insertions alone
    assert c.pile.spans[2] == (4, 6, 7, 0)
    assert c.pile.spans[3] == (0, 0, 7, 0)                # no match column at all
    assert c.pile.spans[4] == (2, 2, 0, 2)                # only match column is its first; one trailing deletion


def test_plan_is_the_hosts():
    """cut_cases.plan against dg_plan_pieces (dagcon_debug_plan, host arithmetic) for a partial-span batch."""
    lib = capi.load()
    lib.dagcon_debug_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    out = (ctypes.c_uint32 * 4)()
    for kw in cc.SETTINGS + (dict(max_segments=1), dict(max_segments=3, min_segment_len=4), dict(max_segments=64, min_segment_len=1)):
        for T, k, bb in ((1, 5, 260), (9, 30, 1500)):
            assert lib.dagcon_debug_plan(T, k, bb, 1, kw.get("max_segments", 0), kw.get("min_segment_len", 0), out) == 0
            seg_max, seg_min, bp_max, _ = cc.plan(**kw)
            assert (out[0], out[1], out[3]) == (seg_max, seg_min, bp_max), (kw, list(out))


def _check_expect(c, k):
    """The figures a family asserts of Cuts k at the case's own setting; the list of those that do not hold."""
    e, bad = c.expect or {}, []
    if "merge" in e and k.merge_pos != e["merge"]:
        bad.append(f"merge row at {k.merge_pos}, not {e['merge']}")
    if "bp" in e and k.bp_pos != e["bp"]:
        bad.append(f"bestPath row at {k.bp_pos}")
    if "bp_has" in e and e["bp_has"] not in k.bp_pos:
        bad.append(f"bestPath row {k.bp_pos} without {e['bp_has']}")
    if "want" in e and k.want != e["want"]:
        bad.append(f"want {k.want}")
    if "nshared" in e and len(k.shared_first) != e["nshared"]:
        bad.append(f"{len(k.shared_first)} shared lists")
    if "nseg" in e and k.nseg != e["nseg"]:
        bad.append(f"{k.nseg} pieces")
    if "defer" in e and (None if k.defer is None else len(k.defer)) != e["defer"]:
        bad.append(f"defer {k.defer and len(k.defer)}")
    return bad


@pytest.mark.parametrize("name", FAMS + ("fullspan",))
def test_family_has_its_single_position(name):
    """Each family's figures at its own setting (printed), and every merge row Cuts predicts, at every setting the device is
    run at, held to `sound`.  Measured:

        covers   256 bases, P64 (want 4, windows of 32 from 65, 129, 193): cuts at 80 (a read ends there and one starts
                 there), 140 (150 open too), 210 (200 deleted by a read that crosses it); 80 deleted as well: one fewer
        lead     maxlead 0 / 1 / 7: pmin 4 / 6 / 18 refused (one piece), 5 / 7 / 19 taken
        tiny     maxlead 4: the prologue reaches exit at 2, 3, 4 bases (FIFO dry, no cuts allowed), not at 5 and 6
        dead     r = 1, 3, 40: e + r + 1 refused, e + r + 2 taken, with deletions in the run too; 256 zones: two pieces,
                 257: one
        starts   v = bb(96): a read starts at 97 behind v's base, or at 97 / 98 where the reads through v delete 97:
                 refused, and bestPath's row takes 96; starts at 98 / 99: taken; 2,048 reads: two pieces, 2,049: one
        window   1,200 bases, windows of 150: offsets 0, 63, 64, 149 taken, 150 not found (three pieces, not four); want 3
                 by seg_max, 64 by the clamp (last window 1182 .. 1190)
        shared   7 united leading letters: 8 shared lists, four pieces; 8: nine, one piece, bestPath's row keeps four;
                 a second read that starts on the cut position is of the piece behind
        slots    16 and 17 appends to in[exit] and to out[enter] by the first piece's worker, none by the second
        defer    63 vertices beside enter (64 entries), and 64 (overflow)
        fullspan want pieces: 4 under P64, 64 at min_segment_len 4"""
    for c in cc.family(name):
        k = c.cuts(**c.pieces)
        print(c.name, c.pile.figures(), "pieces", c.pieces, "want", k.want, "pmin", k.pmin, "merge", k.merge_pos, "bestPath", k.bp_pos,
              "shared", k.shared_first, "nseg", k.nseg, "defer", None if k.defer is None else len(k.defer), "skipped", k.skipped)
        assert not _check_expect(c, k), c.name
        if c.expect and "appends" in c.expect:
            side, n = c.expect["appends"]
            a = cc.appends(c.pile, k.merge_row)
            print(c.name, "appends per segment", a)
            assert a[side] == [n, 0] and a["out" if side == "in" else "in"] == [0, 0]
        if name == "fullspan":
            for kw in (cc.P64, dict(max_segments=64, min_segment_len=4)):
                kk = c.cuts(**kw)
                assert kk.nseg == kk.want == (4 if kw is cc.P64 else 64)
        for kw in _settings(c):
            kk = c.cuts(**kw)
            bad = cc.sound(c.pile, kk.merge_row, kk.shared)
            assert not bad, (c.name, kw, bad[:4])


def test_tiny_targets_and_the_first_that_is_not():
    """The prologue reaches exit (pro_state[3] & 1) iff the FIFO runs dry within levels 0 .. maxlead + 1.  With a chain of
    four inserted bases from enter to exit that is so up to four bases, the smallest target for which it is not has five."""
    got = {c.pile.tlen: (c.pile.exit_in_prologue, c.pile.allow) for c in cc.family("tiny")}
    print(got)
    assert got == {2: (True, False), 3: (True, False), 4: (True, False), 5: (False, True), 6: (False, True)}


# which cases must reject which wrong version of the rule
REJECTS = {
    "pmin_ge": ("lead0_at_pmin", "lead1_at_pmin", "lead7_at_pmin"),
    "dead_hi_minus": ("dead1_inside", "dead3_inside", "dead40_inside", "dead3_tdels_inside"),
    "dead_hi_plus": ("dead1_behind", "dead3_behind", "dead40_behind", "dead3_tdels_behind"),
    "c5_lo": ("starts_ins_at", "starts_del_inside"),
    "c5_hi": ("starts_del_at_q",),
    "c5_drop": ("starts_ins_at", "starts_del_inside", "starts_del_at_q"),
    "seg_lt": ("shared_on_cut",),
    "win_le": ("window_off150",),
}
SOUND_REJECTS = {("c5_lo", "starts_ins_at"), ("c5_drop", "starts_ins_at")}     # where `sound` itself must speak


@pytest.mark.parametrize("mut", cc.MUTATIONS)
def test_mutation_is_rejected(mut):
    """Each wrong version of Cuts (`pos >= pmin`; the dead zone's upper end one less, one more; condition (5) missing the
    read that starts at p + 1, the one that starts at q, or dropped; segment-of-vertex with `<`; the window's
    `o + lane <= span`) changes a figure a family asserts; the seeds' situation is also rejected by `sound`, which knows
    nothing of the rule: mergeInNodes(bb(97)), a visit of the piece behind, unites v with the vertex in front of the
    read that starts there and rewrites lists of the piece in front.  CPU only."""
    by_name = {c.name: c for f in FAMS for c in cc.family(f)}
    for name in REJECTS[mut]:
        c = by_name[name]
        k = c.cuts(**c.pieces, mut=(mut,))
        figs = _check_expect(c, k)
        snd = cc.sound(c.pile, k.merge_row, k.shared)
        print(mut, name, "figures:", figs, "sound:", snd[:2])
        assert figs, (mut, name)
        if (mut, name) in SOUND_REJECTS:
            assert snd, (mut, name)
    # and no mutation is rejected by a case only because the unmutated model fails it
    for name in REJECTS[mut]:
        assert not _check_expect(by_name[name], by_name[name].cuts(**by_name[name].pieces))


def test_mixed_batch_is_partial_span():
    cases, batch = cc.mixed()
    assert batch.n_targets == len(cc.MIXED) and len({c.pile.tlen for c in cases}) >= 4


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _set_env(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare_dump(d, t, c, k, reruns):
    """The dump of target t against Cuts k of case c."""
    tag = (c.name, "target", t)
    assert [r for r in d["worklist"] if r[0] == t] == k.worklist(t), tag
    assert d["bp_row"] == k.bp_row, tag
    assert d["spans"] == [tuple(s) for s in c.pile.spans], tag
    assert d["pro_state"] == c.pile.pro_state, tag
    p, snap = c.pile, c.pile.g.snap
    sh = d["sh_cnt"]
    assert sh[0] == len(k.shared) and sh[1] == snap["in_exit"], tag
    assert [(sh[2 + 2 * i], sh[3 + 2 * i]) for i in range(sh[0])] == \
        [(y, len(snap["out"][p.o2d.index(y)])) for y in k.shared], tag
    if reruns == 0:
        flagged = sorted(v for v in range(d["N"]) if (d["flags"][v] & cc.DG_NF_DEFER) and not (d["flags"][v] & cc.DG_NF_DELETED))
        if k.defer is None:
            assert d["defer"][0] == 0xFFFFFFFF, tag
        else:
            assert d["defer"][0] == len(k.defer) and d["defer"][1:1 + len(k.defer)] == k.defer, tag
            assert flagged == sorted(k.defer), tag


def _graph_run(factory, monkeypatch, tmp_path, cases, batch, kw, env=None):
    """One poisoned run that stops behind the merge, a dump per target: the cuts against Cuts, merge_segments against the
    model's sum, the merged graph against the oracle's."""
    ks = [c.cuts(**kw) for c in cases]
    tm = None
    for t, (c, k) in enumerate(zip(cases, ks)):
        path = tmp_path / f"dump{t}.bin"
        _set_env(monkeypatch, DAGCON_POISON="15", DAGCON_DUMP=f"{t}:{path}", **(env or {}))
        ctx = factory(flags=capi.FLAG_STOP_AFTER_MERGE, **cc.GRAPH_OPTS, **kw)
        try:
            ctx.consensus(batch)
            tm = ctx.timings()
            _compare_dump(cc.read_dump(path), t, c, k, tm["reruns"])
            assert tm["merge_segments"] == sum(x.nseg for x in ks), (c.name, kw, tm)
            if t == 0:
                _check_graphs(ctx, batch, 0, True, oracle_graphs=[g for x in cases for g in x.graphs])
        finally:
            ctx.close()
    return tm


@gpu
@pytest.mark.parametrize("name", FAMS)
def test_family_cuts_on_the_device(gpu_ctx_factory, monkeypatch, tmp_path, name):
    """Every case as a batch of its own, at its own setting, at min_segment_len 4, 64 and 300 with max_segments 64 and at
    the automatic setting, every buffer poisoned: the worklist and bestPath's row from the dump equal Cuts' rows vertex
    for vertex, the reads' figures equal spans', pro_state, the shared lists and their lengths, the defer list and the
    DG_NF_DEFER flags equal the model's, merge_segments is the model's piece count, and the merged graph is the oracle's
    vertex by vertex and in list order."""
    for c in cc.family(name):
        for kw in _settings(c):
            tm = _graph_run(gpu_ctx_factory, monkeypatch, tmp_path, [c], c.batch, kw)
            print(c.name, kw, "merge_segments", tm["merge_segments"], "reruns", tm["reruns"])


@gpu
def test_mixed_batch_on_the_device(gpu_ctx_factory, monkeypatch, tmp_path):
    """Targets of several families in one batch, so that worklist rows and wl_first of different targets lie side by side:
    every target's rows, figures and graph as above, at every setting."""
    cases, batch = cc.mixed()
    for kw in cc.SETTINGS:
        tm = _graph_run(gpu_ctx_factory, monkeypatch, tmp_path, cases, batch, kw)
        print(kw, "merge_segments", tm["merge_segments"])


@gpu
@pytest.mark.parametrize("name", FAMS)
def test_family_consensus(gpu_ctx_factory, monkeypatch, name):
    """The consensus of every case equals the oracle's under the plain options and under trim 2 / min_weight 1, for
    max_segments 0, 1 and 64 (at min_segment_len 4), at the case's own setting, and there with DAGCON_BP_SEGS=3, where
    bestPath's pieces are fewer than the merge's."""
    for c in cc.family(name):
        runs = [(dict(), {}), (dict(max_segments=1), {}), (dict(max_segments=64, min_segment_len=4), {}), (c.pieces, {}),
                (c.pieces, {"DAGCON_BP_SEGS": str(cc.BP_SEGS)})]
        for kw, env in runs:
            _set_env(monkeypatch, **env)
            for opts, exp in zip(cc.CNS_OPTS, c.consensus):
                ctx = gpu_ctx_factory(**opts, **kw)
                try:
                    assert ctx.consensus(c.batch) == exp, (c.name, kw, env, opts)
                finally:
                    ctx.close()


@gpu
@pytest.mark.parametrize("side", ["in", "out"])
def test_slots_rerun(gpu_ctx_factory, monkeypatch, side):
    """Seventeen appends by one worker to in[exit] (out[enter]) outgrow its 16 slots: DG_E_LOG_OVF, sh_log doubled, the batch
    run again.  One re-run more than the 16-entry control on a fresh context, the oracle's consensus both times, and a
    second consensus on the same context without a re-run."""
    _set_env(monkeypatch)
    by_name = {c.name: c for c in cc.family("slots")}
    ctl, c = by_name[f"slots_{side}16"], by_name[f"slots_{side}17"]
    got = {}
    for x in (ctl, c):
        ctx = gpu_ctx_factory(**cc.CNS_OPTS[0], **cc.P64)
        try:
            assert ctx.consensus(x.batch) == x.consensus[0]
            first = ctx.timings()["reruns"]
            assert ctx.consensus(x.batch) == x.consensus[0]
            got[x.name] = (first, ctx.timings()["reruns"])
        finally:
            ctx.close()
    print(got)
    assert got[c.name][0] == got[ctl.name][0] + 1
    assert got[c.name][1] == 0 and got[ctl.name][1] == 0


@gpu
def test_full_span_through_the_partial_span_kernels(gpu_ctx_factory, monkeypatch, tmp_path):
    """A full-span pileup under DAGCON_GCUTS=1: every lead and trail zero, every start 1, and the merge row has the `want`
    pieces wherever condition (1) holds in every window: 4 under P64, 64 at min_segment_len 4."""
    (c,) = cc.family("fullspan")
    for kw, n in ((cc.P64, 4), (dict(max_segments=64, min_segment_len=4), 64)):
        tm = _graph_run(gpu_ctx_factory, monkeypatch, tmp_path, [c], c.batch, kw, env={"DAGCON_GCUTS": "1"})
        assert tm["merge_segments"] == n
        assert all(s == (1, 256, 0, 0) for s in c.pile.spans)
        _set_env(monkeypatch, DAGCON_GCUTS="1")
        for opts, exp in zip(cc.CNS_OPTS, c.consensus):
            ctx = gpu_ctx_factory(**opts, **kw)
            try:
                assert ctx.consensus(c.batch) == exp
            finally:
                ctx.close()
