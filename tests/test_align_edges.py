"""The -a aligner (k_align.hip.h, dagcon_align) where uniform random ACGT does not reach: tie-dense sequence, lengths on
the kernels' own periods, the lengths at which the kernel instance changes, and pairs that one band hands over to the
next.  On the CPU the tie order of both twins (oracle.banded_align; align_local_twin.align) is pinned, strings and
ends, to a DP over the whole matrix that knows nothing about bands; on the device dagcon_align / dagcon_align_ends are
compared with the twins byte for byte.  What a test is meant to cover (which pass decided a pair, that every outcome
appears) is asserted on the CPU, through the twins' stage reporters, before the device is used."""
import functools

import numpy as np
import pytest

import align_cases as cases
import align_local_twin as twin
import oracle

NONE, FOLLOWING, FIRST, FULL = oracle.STAGE_NONE, oracle.STAGE_FOLLOWING, oracle.STAGE_FIRST, oracle.STAGE_FULL
assert (NONE, FOLLOWING, FIRST, FULL) == (twin.STAGE_NONE, twin.STAGE_FOLLOWING, twin.STAGE_FIRST, twin.STAGE_FULL)
NOTHING = (b"", b"", (0, 0, 0, 0))


# ---------------------------------------------------------------------------------------------- the band-free DP


def plain_dp(q: bytes, t: bytes, local: bool):
    """The rule at the top of k_align.hip.h over the full (n + 1) x (m + 1) matrix, cell by cell, no band, no prefix
    minimum (written here, not align_local_twin.full_matrix, which the local test below is compared with as well):
    match -5, mismatch +6, insertion 4, deletion 5; the diagonal, then the insertion, then the deletion, each only
    when strictly better.  Global: walk back from (n, m).  Local: a score above 0 becomes 0 and starts an alignment,
    as does all of row 0; the end is the smallest score below 0, the later row, then the later cell winning a tie; walk
    back to a start.  -> (qaln, taln, (q_begin, q_end, t_begin, t_end))."""
    n, m = len(q), len(t)
    INF = 1 << 40
    H = [[0] * (m + 1) for _ in range(n + 1)]
    D = [[3] * (m + 1) for _ in range(n + 1)]
    if not local:
        for j in range(1, m + 1):
            H[0][j], D[0][j] = 5 * j, 2
    end = (n, m) if not local else None
    low = 0
    for i in range(1, n + 1):
        for j in range(m + 1):
            v, d = INF, 3
            if j > 0:
                v, d = H[i - 1][j - 1] + (-5 if q[i - 1] == t[j - 1] else 6), 0
            if H[i - 1][j] + 4 < v:
                v, d = H[i - 1][j] + 4, 1
            if j > 0 and H[i][j - 1] + 5 < v:
                v, d = H[i][j - 1] + 5, 2
            if local and v > 0:
                v, d = 0, 3
            H[i][j], D[i][j] = v, d
            if local and v < 0 and v <= low:
                low, end = v, (i, j)
    if end is None:
        return NOTHING
    (i, j), qa, ta = end, bytearray(), bytearray()
    while D[i][j] != 3:
        d = D[i][j]
        qa.append(q[i - 1] if d != 2 else 0x2D)
        ta.append(t[j - 1] if d != 1 else 0x2D)
        i, j = i - (d != 2), j - (d != 1)
    return bytes(qa[::-1]), bytes(ta[::-1]), (i, end[0], j, end[1])


@functools.lru_cache(maxsize=None)
def _small():
    return cases.small_tie_pairs(np.random.default_rng(101))


def _held(q, t, stage):
    """The pair's deciding band held the whole matrix: the first band does, or the full band (which does for every pair
    of at most 40 bases a side) decided."""
    L = max(len(q), len(t))
    assert L <= 40 and oracle.align_halfwidth(len(q), len(t)) >= L
    assert oracle.align_halfwidth(len(q), len(t)) == twin.halfwidth(len(q), len(t))
    assert oracle.align_halfwidth_first(len(q), len(t)) == twin.halfwidth_first(len(q), len(t))
    return twin.halfwidth_first(len(q), len(t)) >= L or stage == FULL


def test_global_tie_order_equals_band_free_dp(oracle_lib):
    """oracle.banded_align against plain_dp on tie-dense pairs of at most 40 bases: the aligned STRINGS.  A pair counts
    only when the band that decided it held the whole matrix (the first band does up to 36 bases; beyond, only a pair
    that the full band decided); at least 1,500 count."""
    n_held, n_full, by_family = 0, 0, {}
    for fam, q, t in _small():
        qa, ta, stage = oracle.banded_align_stage(q, t)
        assert (qa, ta) == oracle.banded_align(q, t)
        assert stage in (FIRST, FULL)                             # (too short for the following band; never nothing)
        if not _held(q, t, stage):
            assert max(len(q), len(t)) > 36
            continue
        n_held += 1
        n_full += stage == FULL
        by_family[fam] = by_family.get(fam, 0) + 1
        assert (qa, ta) == plain_dp(q, t, False)[:2], (fam, q, t)
    assert n_held >= 1500 and n_full >= 5, (n_held, n_full)
    assert set(by_family) == {"homopolymer", "tandem", "two_letter", "disjoint", "foreign", "n_lower"} and min(by_family.values()) >= 100


def test_local_tie_order_equals_band_free_dp():
    """align_local_twin.align against plain_dp (and against the twin's own full_matrix) on the same pairs: strings and
    ends; the same condition on the deciding band.  Pairs without a local alignment (no base in common) count: all
    three say so."""
    n_held, n_found = 0, 0
    for fam, q, t in _small():
        got = twin.align(q, t, stage=True)
        assert got[:3] == twin.align(q, t)
        if got[3] != NONE and not _held(q, t, got[3]):
            continue
        n_held += 1
        n_found += got[3] != NONE
        exp = plain_dp(q, t, True)
        assert got[:3] == exp, (fam, q, t)
        assert twin.full_matrix(q, t) == exp, (fam, q, t)
    assert n_held >= 1500 and n_found >= 1200, (n_held, n_found)


# ---------------------------------------------------------------------------------------------- the device


def _global_expected(pairs, static):
    """[(qaln, taln, stage)] of oracle.banded_align_stage; static: OG_NO_ADAPTIVE=1 (the test has set it)."""
    import os
    assert bool(os.environ.get("OG_NO_ADAPTIVE")) == static
    return [oracle.banded_align_stage(q, t) for q, t in pairs]


def _local_expected(pairs, static):
    return [twin.align(q, t, static_only=static, stage=True) for q, t in pairs]


def _mode(monkeypatch, static, rows=None):
    for k, on in (("DAGCON_ALIGN_STATIC", static), ("OG_NO_ADAPTIVE", static)):
        monkeypatch.setenv(k, "1") if on else monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DAGCON_ALIGN_ROWS", str(rows)) if rows else monkeypatch.delenv("DAGCON_ALIGN_ROWS", raising=False)


def _check_global(ctx, pairs, exp):
    got = ctx.align(pairs)
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e[:2]]
    assert not bad, [(i, len(pairs[i][0]), len(pairs[i][1]), exp[i][2]) for i in bad[:8]]
    assert ctx.align_ends() == [(0, len(q), 0, len(t)) if e[2] != NONE else (0, 0, 0, 0) for (q, t), e in zip(pairs, exp)]


def _check_local(ctx, pairs, exp):
    got, ends = ctx.align(pairs), ctx.align_ends()
    bad = [i for i, (g, x, e) in enumerate(zip(got, ends, exp)) if (g[0], g[1], x) != e[:3]]
    assert not bad, [(i, len(pairs[i][0]), len(pairs[i][1]), ends[i], exp[i][2:]) for i in bad[:8]]


def _local_ctx(factory):
    from pbdagcon_amd import capi
    return factory(flags=capi.FLAG_LOCAL_ALIGN)


# ---- tie-dense pairs at three scales around the halfwidth_first > 56 split

SCALES = (200, 1500, 5000)


@functools.lru_cache(maxsize=None)
def _tie_pairs(L, family=None):
    return [(q, t) for f, q, t in cases.tie_pairs_at(np.random.default_rng(200 + L), L) if family in (None, f)]


def _tie_stage_claims(L, exp, static):
    stages = [e[-1] for e in exp]
    if static or L == 200:
        assert FOLLOWING not in stages                            # static bands only
        assert twin.halfwidth_first(L, L) <= twin.WA or static
    else:
        assert twin.halfwidth_first(L - 61, L - 61) > twin.WA
        assert stages.count(FOLLOWING) >= 5, stages               # some tie-dense pairs go through the following band


@pytest.mark.gpu
@pytest.mark.parametrize("static", (False, True), ids=("default", "static"))
@pytest.mark.parametrize("L", SCALES)
def test_device_tie_dense_global(gpu_ctx_factory, monkeypatch, L, static):
    """Homopolymers, tandem repeats, two letters, no base in common, a foreign base in a repeat, N and lower case, with
    length differences 0, 1, 20 and 61, at 200 bases (static bands), 1.5 kb and 5 kb (following band): dagcon_align
    equals oracle.banded_align; again with the static bands alone."""
    _mode(monkeypatch, static)
    pairs = _tie_pairs(L)
    exp = _global_expected(pairs, static)
    _tie_stage_claims(L, exp, static)
    _check_global(gpu_ctx_factory(), pairs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("static", (False, True), ids=("default", "static"))
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("L", SCALES)
def test_device_tie_dense_local(gpu_ctx_factory, monkeypatch, L, family, static):
    """The same pairs on a DAGCON_FLAG_LOCAL_ALIGN context against align_local_twin.align: strings and ends.  A family
    a case (the twin is numpy, a row at a time).  Pairs without a base in common have no local alignment, in any
    band; of every other family the following band decides some pairs at 1.5 kb and at 5 kb."""
    _mode(monkeypatch, static)
    pairs = _tie_pairs(L, family)
    assert len(pairs) == 4
    exp = _local_expected(pairs, static)
    stages = [e[3] for e in exp]
    if family == "disjoint":
        assert stages == [NONE] * 4
    elif static or L == 200:
        assert FOLLOWING not in stages and NONE not in stages
    else:
        assert stages.count(FOLLOWING) >= 2 and NONE not in stages, stages
    _check_local(_local_ctx(gpu_ctx_factory), pairs, exp)


# ---- the kernels' periods

@functools.lru_cache(maxsize=None)
def _period_pairs():
    pairs = cases.period_pairs(np.random.default_rng(301))
    lens = {len(t) - twin.halfwidth_first(len(q), len(t)) for q, t in pairs}
    assert {63, 64, 65, 127, 128, 129} <= lens                    # targets that end where the t window refills
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("rows", (None, 64), ids=("one_group", "rows64"))
def test_device_periods_global(gpu_ctx_factory, monkeypatch, rows):
    """Lengths on the 64-character windows, the 16 staged rows and the 64-code flushes (cases.period_pairs), global;
    again with DAGCON_ALIGN_ROWS=64, which splits neighbours into different launch groups."""
    _mode(monkeypatch, False, rows)
    pairs = _period_pairs()
    exp = _global_expected(pairs, False)
    assert {len(e[0]) % 64 for e in exp} >= {0, 1, 63}            # path lengths on the flush period and one off it
    _check_global(gpu_ctx_factory(), pairs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", (None, 64), ids=("one_group", "rows64"))
def test_device_periods_local(gpu_ctx_factory, monkeypatch, rows):
    _mode(monkeypatch, False, rows)
    pairs = _period_pairs()
    exp = _local_expected(pairs, False)
    assert {len(e[0]) % 64 for e in exp} >= {0, 1, 63}
    _check_local(_local_ctx(gpu_ctx_factory), pairs, exp)


@pytest.mark.gpu
def test_device_revcomp_middle_element(gpu_ctx_factory):
    """k_align_revcomp through dagcon_consensus_pre: '-' strand records whose aligned length is odd (a middle column,
    complemented once) and even, six copies a target so that the column shows in the consensus; against
    oracle.simple_align + oracle.consensus_target."""
    rng = np.random.default_rng(302)
    targets, exp, parity = [], [], set()
    for n in (63, 64, 65, 127, 128, 129, 192, 193):
        t = cases.rand(rng, n)
        for q in (t, cases.mutated_to(rng, t, n, sub=0.02, ins=0.02, dele=0.02), cases.mutated_to(rng, t, n + 1, sub=0.02, ins=0.02, dele=0.02)):
            start, _, qa, ta = oracle.simple_align(0, n, b"-", q, t)
            parity.add(len(qa) % 2)
            targets.append((n, [(0, b"-", q, t)] * 6))
            exp.append(oracle.consensus_target(n, [(start, qa, ta)] * 6, 20, 0, 6))
    assert parity == {0, 1} and all(len(e) == 1 for e in exp)
    assert gpu_ctx_factory(min_cov=6, min_len=20, trim=0).consensus_pre(targets) == exp


# ---- the steps from one kernel instance to the next

@functools.lru_cache(maxsize=None)
def _steps():
    """[(band, L, w before, w at L)]: every step of dg_align_cells over the first band and over the full band, and
    the cap, computed from the twin's widths (test_instance_steps_are_all_there checks them against the oracle's)."""
    out = [("first", *s) for s in cases.instance_steps(twin.halfwidth_first)] + [("full", *s) for s in cases.instance_steps(twin.halfwidth)]
    return out


def test_instance_steps_are_all_there(oracle_lib):
    """Every instance is stepped into by the full band, the first band reaches 8 cells a lane below the cap, and the
    direction word widens (8 -> 12 cells) in both."""
    st = _steps()
    for _, L, a, b in st:
        for x in (L - 1, L):
            assert oracle.align_halfwidth(x, x) == twin.halfwidth(x, x)
            assert oracle.align_halfwidth_first(x, x) == twin.halfwidth_first(x, x)
    assert [cases.cells(b) for k, _, _, b in st if k == "full"] == [4, 6, 8, 12, 16, 16]
    assert [cases.cells(b) for k, _, _, b in st if k == "first"] == [4, 6, 8, 12]
    assert st[-1][3] == twin.MAXW and 80000 < st[-1][1] < 90000
    assert all(cases.cells(a) < cases.cells(b) or b == twin.MAXW for _, _, a, b in st)


def _step_pairs(L, seed, lengths=None):
    """At each of L - 1 and L (or at `lengths`): a mutated pair, and candidates for a pair with one block of
    w1 + w2 - 16 target bases missing from the middle of the read (then a little less or more, should the noise of the mutations move it out of
    the stage it is built for)."""
    rng = np.random.default_rng(seed)
    out = []
    for x in lengths or (L - 1, L):
        t = cases.rand(rng, x)
        mut = (cases.mutate(rng, t, sub=0.03, ins=0.03, dele=0.04)[:x], t)      # (q the shorter side: max(n, m) = x)
        d0 = twin.halfwidth_first(x, x) + twin.halfwidth(x, x) - 16

        def cand(t=t, d0=d0, x=x):
            for d in (d0, d0 - 4, d0 + 4, d0 - 8, d0 + 8):
                h = (x - d) // 2
                yield cases.mutate(rng, t[:h], sub=0.01, ins=0.01, dele=0.01) + cases.mutate(rng, t[h + d:], sub=0.01, ins=0.01, dele=0.01), t
        out.append((mut, cand))
    return out


def _settle_block(cand, expected_of):
    """The first block candidate that the full band decides, with its expected answer."""
    for c in cand():
        e = expected_of([c])[0]
        if e[-1] == FULL:
            return c, e
    raise AssertionError("no block pair of this step is decided by the full band")


def _settle(step_pairs, expected_of):
    """The pairs of a step with their expected answers in static-only mode: the mutated pair must be decided by the
    first band, the block pair by the full band."""
    pairs, exp = [], []
    for mut, cand in step_pairs:
        e = expected_of([mut])[0]
        assert e[-1] == FIRST, (len(mut[0]), len(mut[1]), e[-1])
        c, ec = _settle_block(cand, expected_of)
        pairs += [mut, c]; exp += [e, ec]
    return pairs, exp


def _step_ids(local):
    return ["%s-%d" % (k, L) for k, L, _, b in _steps() if not local or b <= 192]


@pytest.mark.gpu
@pytest.mark.parametrize("step", _step_ids(False))
def test_device_instance_steps_global(gpu_ctx_factory, monkeypatch, step):
    """A pair of length L - 1 and one of length L for the smallest L at which the first / the full band moves to the
    next kernel instance (and the L at which the full band reaches its cap), static bands alone: a mutated pair, which
    the first band decides, and a pair with a block indel, which touches the first band's margin and is decided by the
    full band."""
    _mode(monkeypatch, True)
    L = int(step.split("-")[1])
    pairs, exp = _settle(_step_pairs(L, 400 + L), lambda p: _global_expected(p, True))
    assert [e[2] for e in exp] == [FIRST, FULL, FIRST, FULL]
    _check_global(gpu_ctx_factory(), pairs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("mutated", "block"))
@pytest.mark.parametrize("below", (1, 0), ids=("L-1", "L"))
@pytest.mark.parametrize("step", _step_ids(True))
def test_device_instance_steps_local(gpu_ctx_factory, monkeypatch, step, below, kind):
    """The same on a local context, for the steps up to half-width 192 (the wider instances are the same template:
    the global run and test_device_local_align_equals_twin's 20 - 110 kb pairs cover them); a pair a case (the twin is
    numpy, a row at a time: the block pair of 42.7 kb, two bands of 385 and 705 cells, is the longest of them)."""
    _mode(monkeypatch, True)
    L = int(step.split("-")[1])
    (mut, cand), = _step_pairs(L, 400 + L, (L - below,))
    if kind == "mutated":
        pairs, exp = [mut], _local_expected([mut], True)
        assert exp[0][3] == FIRST
    else:
        c, e = _settle_block(cand, lambda p: _local_expected(p, True))
        pairs, exp = [c], [e]
    _check_local(_local_ctx(gpu_ctx_factory), pairs, exp)


# ---- hand-overs at the margin

SWEEP = range(30, 140)


@functools.lru_cache(maxsize=None)
def _sweep_pairs(tlen):
    t = cases.rand(np.random.default_rng(500 + tlen), tlen)
    return [cases.block_pair(t, d, sw) for d in SWEEP for sw in (False, True)]


def _sweep_claims(tlen, stages):
    want = (FIRST, FULL) if tlen == 300 else (FOLLOWING, FIRST, FULL)
    assert all(stages.count(s) >= 5 for s in want), {s: stages.count(s) for s in (NONE, FOLLOWING, FIRST, FULL)}


@pytest.mark.gpu
@pytest.mark.parametrize("tlen", (300, 1500))
def test_device_handovers_global(gpu_ctx_factory, monkeypatch, tlen):
    """t random, q = t without its middle d bases, and the roles swapped, for every d in 30 .. 139: the path comes to
    within DG_AL_MARGIN of an edge somewhere in the sweep, and the pair goes from the following band (1.5 kb) to the
    first static band to the full one; with them a pair that no band connects, so that dagcon_align sees every outcome
    in one call."""
    _mode(monkeypatch, False)
    pairs = list(_sweep_pairs(tlen))
    t5k = cases.rand(np.random.default_rng(77), 5000)
    pairs.append((t5k[:3], t5k))
    exp = _global_expected(pairs, False)
    _sweep_claims(tlen, [e[2] for e in exp[:-1]])
    assert exp[-1] == (b"", b"", NONE)
    _check_global(gpu_ctx_factory(), pairs, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["300-%s-all" % r for r in ("removed", "swapped")] + ["1500-%s-%d" % (r, c) for r in ("removed", "swapped") for c in range(4)])
def test_device_handovers_local(gpu_ctx_factory, monkeypatch, part):
    """The same sweep on a local context (the block sits between two matching flanks, which the local alignment spans
    as long as they outweigh it), one role a case, and of the 1.5 kb sweep every fourth d a case (the twin is numpy, a
    row at a time): every such quarter runs over the whole range, so each of its stages decides at least three of its
    pairs, twelve of the sweep's; a pair without a local alignment in the same call: ends (0, 0, 0, 0)."""
    _mode(monkeypatch, False)
    tlen, role, c = part.split("-")
    tlen = int(tlen)
    pairs = list(_sweep_pairs(tlen)[("removed", "swapped").index(role)::2])
    if c != "all":
        pairs = pairs[int(c)::4]
    t5k = cases.rand(np.random.default_rng(77), 5000)
    pairs.append((t5k[:3].translate(bytes.maketrans(b"ACGT", b"NNNN")), t5k))
    exp = _local_expected(pairs, False)
    stages = [e[3] for e in exp[:-1]]
    want = (FIRST, FULL) if tlen == 300 else (FOLLOWING, FIRST, FULL)
    assert all(stages.count(s) >= (5 if c == "all" else 3) for s in want), stages
    assert exp[-1] == NOTHING + (NONE,)
    assert sum(e[2] == (0, len(q), 0, len(t)) for (q, t), e in zip(pairs, exp)) >= len(pairs) // 2      # spans the block
    _check_local(_local_ctx(gpu_ctx_factory), pairs, exp)


@pytest.mark.gpu
def test_device_ad_rest_split(gpu_ctx_factory, monkeypatch):
    """Pairs of length 1,120 and 1,121, either side the longer: the last length whose first band is 56 cells wide, which
    goes straight to the static bands, and the first that tries the following band."""
    _mode(monkeypatch, False)
    assert (twin.halfwidth_first(1120, 1), twin.halfwidth_first(1121, 1)) == (twin.WA, twin.WA + 2)
    assert oracle.align_halfwidth_first(1120, 1120) == twin.WA and oracle.align_halfwidth_first(1, 1121) == twin.WA + 2
    rng = np.random.default_rng(601)
    pairs = []
    short = lambda s: cases.mutate(rng, s, sub=0.03, ins=0.03, dele=0.06)[:len(s)]     # noqa: E731
    for L in (1120, 1121):
        t = cases.rand(rng, L)
        pairs += [(short(t), t), (t, short(t)), (cases.mutated_to(rng, t, L, sub=0.02, ins=0.03, dele=0.03), t),
                  cases.block_pair(t, 60, False), cases.block_pair(t, 60, True)]
    assert [max(len(q), len(t)) for q, t in pairs] == [1120] * 5 + [1121] * 5
    exp, lexp = _global_expected(pairs, False), _local_expected(pairs, False)
    for e in (exp, lexp):
        assert FOLLOWING not in [x[-1] for x in e[:5]] and [x[-1] for x in e[5:]].count(FOLLOWING) >= 3
    _check_global(gpu_ctx_factory(), pairs, exp)
    _check_local(_local_ctx(gpu_ctx_factory), pairs, lexp)
