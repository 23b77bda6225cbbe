"""The record intake as one path: every input kind (plain, packed, stranded, cs) through both modes (whole targets,
windows) from one small set of alignments.  The per-kind tests (test_cigar, test_windows, test_bam, test_paf, test_cs)
pin each kind on its own; this pins the matrix, which is what a shared plan / expand step can break unnoticed.

The reference is dagcon_consensus on the twin's strings: cigar_twin.expand for whole targets, window_twin.window_targets
for windows.  A target (a window) that a non-conforming record fails has no twin strings: it is expected empty, with
DAGCON_ERR_NONCONFORMING as its status.
"""
import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import paf_files as pf
import window_twin as wt
from util import batch_from_targets

MIN_COV, MIN_LEN, TRIM = 4, 20, 5
W, O = 100, 10
NONCONFORMING = -4
TLENS = (300, 310, 290)


def _read(rng, bb, pos, ops, exact=False):
    """The read bases ops ask for at pos of bb: target bases under M / = (M: a few substituted unless exact), another
    base under X, random ones under I / S."""
    q = bytearray()
    x = pos - 1
    for o in ops:
        code, n = int(o) & 15, int(o) >> 4
        if code in (ct.M, ct.EQ, ct.X):
            for k in range(n):
                b = bb[x + k]
                if code == ct.X or (code == ct.M and not exact and rng.random() < 0.04):
                    b = b"ACGT"[(b"ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4]
                q.append(b)
        elif code in (ct.I, ct.S):
            q.extend(b"ACGT"[i] for i in rng.integers(0, 4, n))
        if code in (ct.M, ct.D, ct.EQ, ct.X):
            x += n
    return pos, bytes(q), [int(o) for o in ops]


def _random_ops(rng, span):
    """Ops that consume span target bases: M / = / X runs with short insertions and deletions between them."""
    ops, left = [], span
    while left > 0:
        n = min(left, int(rng.integers(5, 25)))
        ops.append(ct.op("M=X"[int(rng.choice(3, p=[0.7, 0.25, 0.05]))] if n > 1 else "M", n))
        left -= n
        if left > 3 and rng.random() < 0.6:
            if rng.random() < 0.5:
                ops.append(ct.op("I", int(rng.integers(1, 4))))
            else:
                d = int(rng.integers(1, 3)); ops.append(ct.op("D", d)); left -= d
    return ops


def _fillers(rng, bb, n):
    """n reads of 120 to 200 target bases whose starts are spread over the whole of bb."""
    out = []
    for k in range(n):
        span = int(rng.integers(120, 200))
        s = min(len(bb) - span, k * (len(bb) - 100) // max(1, n - 1))
        out.append(_read(rng, bb, s + 1, _random_ops(rng, span)))
    return out


def _tiles(ops):
    """Columns in front of every tile of 64 ops."""
    cols = [(int(o) >> 4) if (int(o) & 15) in ct._COL else 0 for o in ops]
    return [sum(cols[:k]) for k in range(0, len(ops), 64)]


@pytest.fixture(scope="module")
def case():
    """3 targets of about 300 bases with 8 records each, tiled into windows of 100 + 10 on either side; the named records
    are the edges the shared expand body and the two plans have (asserted below, so that they stay what they claim)."""
    rng = np.random.default_rng(20261018)
    bbs = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl)) for tl in TLENS]
    unit = [ct.op("M", 3), ct.op("I", 1), ct.op("M", 3), ct.op("D", 1)]
    named = {
        "ops64": (0, _read(rng, bbs[0], 11, unit * 16, exact=True)),                       # one tile
        "ops65": (0, _read(rng, bbs[0], 79, unit * 16 + [ct.op("M", 3)], exact=True)),      # two tiles; [78, 193)
        "cols64": (1, _read(rng, bbs[1], 20, [ct.op("M", 30), ct.op("I", 4), ct.op("M", 30)], exact=True)),
        "cols65": (1, _read(rng, bbs[1], 150, [ct.op("M", 30), ct.op("I", 5), ct.op("M", 30)], exact=True)),
        "clip3": (1, _read(rng, bbs[1], 100, [ct.op("S", 3), ct.op("M", 50), ct.op("I", 2), ct.op("M", 40), ct.op("S", 2)])),
        "ins_only": (1, _read(rng, bbs[1], 120, [ct.op("S", 2), ct.op("I", 5), ct.op("S", 1)])),
        "bad_op": (2, _read(rng, bbs[2], 50, [ct.op("M", 20), ct.op("N", 5), ct.op("M", 20)])),   # [49, 89): its first window only
    }
    targets = []
    for g, bb in enumerate(bbs):
        mine = [r for tg, r in named.values() if tg == g]
        targets.append((bb, mine + _fillers(rng, bb, 8 - len(mine))))
    wins = [(g, b, e) for g, bb in enumerate(bbs) for b, e, _, _ in wt.tiled(len(bb), W, O)]
    # the edges, checked against the twin
    rec = {k: r for k, (_, r) in named.items()}
    assert len(rec["ops64"][2]) == 64 and len(rec["ops65"][2]) == 65
    assert len(ct.expand(*rec["cols64"][:2], bbs[1], rec["cols64"][2])[1]) == 64
    assert len(ct.expand(*rec["cols65"][:2], bbs[1], rec["cols65"][2])[1]) == 65
    p, q, o = rec["ops65"]
    assert wt.span(p, TLENS[0], o) == (78, 193) and (0, 190, 300) in wins and (0, 0, 110) in wins
    tstr = ct.expand(p, q, bbs[0], o)[2]
    assert wt.first_col(tstr, 78, 193, 190) == _tiles(o)[1] == 128          # a window begins on a tile's first column
    assert 0 < wt.first_col(tstr, 78, 193, 110) < 128                       # a window ends strictly inside a tile
    assert (rec["clip3"][2][0] >> 4) % 2 == 1 and rec["clip3"][2][0] & 15 == ct.S
    p, q, o = rec["ins_only"]
    assert ct.conforming(p, len(q), TLENS[1], o) and wt.span(p, TLENS[1], o) == (119, 119)
    p, q, o = rec["bad_op"]
    assert not ct.conforming(p, len(q), TLENS[2], o)
    bad_wins = [i for i, (g, b, e) in enumerate(wins) if g == 2 and max(b, 49) < min(e, 89)]
    assert len(bad_wins) == 1 and sum(g == 2 for g, _, _ in wins) == 3          # one of target 2's three windows
    assert all(len(recs) == 8 for _, recs in targets)
    return targets, wins, bad_wins


def _cs_subset(targets):
    """What the cs form can say: no S op (cs has no clips) and no op code it has no letter for -- the records with either
    are left out of the cs leg, which is compared with the twin on what is left."""
    return [(bb, [r for r in recs if not any((o & 15) in (ct.S, ct.N) for o in r[2])]) for bb, recs in targets]


def _everything(ctx, segs):
    return segs, ctx.target_status.tolist(), ctx.base_support(), ctx.base_positions()


def _same(got, exp):
    assert got[0] == exp[0] and got[1] == exp[1]
    for x, y in ((got[2], exp[2]), (got[3], exp[3])):
        assert len(x) == len(y)
        for sx, sy in zip(x, y):
            assert len(sx) == len(sy)
            for ex, ey in zip(sx, sy):
                if isinstance(ex, tuple):
                    assert all(np.array_equal(u, v) for u, v in zip(ex, ey))
                else:
                    assert np.array_equal(ex, ey)


def _reference(ctx, targets, wins):
    """dagcon_consensus on the twin's strings, whole targets and windows; a failed target / window: empty, -4."""
    whole = []
    for bb, recs in targets:
        failed = any(not ct.conforming(p, len(q), len(bb), o) for p, q, o in recs)
        whole.append((len(bb), [] if failed else [ct.expand(p, q, bb, o) for p, q, o in recs], failed))
    out = []
    for per in (whole, wt.window_targets(targets, wins)):
        segs, status, sup, pos = _everything(ctx, ctx.consensus(batch_from_targets([(tl, alns, None) for tl, alns, _ in per])))
        assert all(s == 0 for s in status)
        for i, (_, _, failed) in enumerate(per):
            if failed:
                assert segs[i] == [] and sup[i] == [] and pos[i] == []
                status[i] = NONCONFORMING
        out.append((segs, status, sup, pos))
    return out


@pytest.mark.gpu
def test_every_kind_in_both_modes_equals_the_twin_strings(case):
    from pbdagcon_amd import capi
    targets, wins, bad_wins = case
    hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    n = sum(len(recs) for _, recs in targets)
    reverse = (np.arange(n) % 3 == 1).astype(np.uint8)             # every third record lies reversed in the "reads file"
    i = 0
    as_file = []
    for bb, recs in targets:
        as_file.append((bb, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(recs)]))
        i += len(recs)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    cs_targets = _cs_subset(targets)
    assert sum(len(r) for _, r in cs_targets) == n - 3 and all(len(r[2]) in (64, 65) for r in cs_targets[0][1][:2])
    forms = {
        "plain": (plain, targets),
        "packed": (plain.packed(), targets),
        "stranded": (capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), targets),
        "cs": (capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs])
                                               for bb, recs in cs_targets]), cs_targets),
    }
    assert forms["packed"][0].is_packed and 0 < int(reverse.sum()) < n
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        refs = {id(t): _reference(ctx, t, wins) for t in (targets, cs_targets)}
        exp_whole, exp_win = refs[id(targets)]
        # the case is not vacuous: consensus for the sound targets and most windows, the one bad record fails target 2
        # and the one window it meets and nothing else, and the insertions-only record is among target 1's records
        assert exp_whole[1] == [0, 0, NONCONFORMING] and exp_whole[0][0] and exp_whole[0][1]
        assert [i for i, s in enumerate(exp_win[1]) if s] == bad_wins and sum(bool(x) for x in exp_win[0]) >= 6
        assert refs[id(cs_targets)][0][1] == [0, 0, 0]
        for kind, (batch, twin_targets) in forms.items():
            r_whole, r_win = refs[id(twin_targets)]
            if kind == "cs":
                got_whole = _everything(ctx, ctx.consensus_cs(batch, strict=False))
                got_win = _everything(ctx, ctx.consensus_cs(batch, hw, strict=False))
            else:
                got_whole = _everything(ctx, ctx.consensus_cigar(batch, strict=False))
                got_win = _everything(ctx, ctx.consensus_cigar_windows(batch, hw, strict=False))
            _same(got_whole, r_whole)
            _same(got_win, r_win)
    finally:
        ctx.close()
