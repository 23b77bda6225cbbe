"""Windowed consensus for CIGAR input: per-base target positions (DAGCON_FLAG_BASE_POS, dagcon_fetch_positions), records
cut to windows on the device (dagcon_consensus_cigar_windows) and the cut / stitch rules themselves (tests/window_twin.py).
A window's result is pinned to the oracle through dagcon_consensus on the twin's piece strings."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cigar_twin as ct
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the cut ------------------------------------------------------------------------------------------------------

def _random_record(rng, tseq, s, e):
    """A conforming record over target bases [s, e) with every legal op code (M I D S H P = X), optional leading /
    trailing I and S.  Returns (pos, read, ops)."""
    ops, q = [], bytearray()
    if rng.random() < 0.5:
        ops.append(ct.op("H", int(rng.integers(1, 9))))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 6)); ops.append(ct.op("S", n)); q += bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), n))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 5)); ops.append(ct.op("I", n)); q += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    x = s
    while x < e:
        kind = "M=XD"[int(rng.integers(0, 4))]
        n = min(int(rng.integers(1, 12)), e - x)
        if kind == "D" and (x == s or x + n == e):
            kind = "M"                                             # (a record begins and ends on a base of its own)
        ops.append(ct.op(kind, n))
        if kind != "D":
            q += tseq[x:x + n] if kind != "X" else bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
        x += n
        if x < e:
            u = rng.random()
            if u < 0.25:
                n = int(rng.integers(1, 5)); ops.append(ct.op("I", n)); q += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
            elif u < 0.35:
                ops.append(ct.op("P", int(rng.integers(1, 4))))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 5)); ops.append(ct.op("I", n)); q += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 6)); ops.append(ct.op("S", n)); q += bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), n))
    assert ct.conforming(s + 1, len(q), len(tseq), ops)
    return s + 1, bytes(q), ops


def _cut_points(s, ops):
    """Target coordinates inside an M, inside a D, and on op boundaries of a record."""
    inside = {"M": [], "D": [], "edge": []}
    x = s
    for o in ops:
        code, n = o & 15, o >> 4
        if code in ct._TGT:
            inside["edge"].append(x)
            if n >= 2:
                inside["D" if code == ct.D else "M"].append(x + n // 2)
            x += n
    return inside


def test_cut_partitions_a_record():
    """Windows that tile the target partition a record's columns; each piece's strings are the slice of the whole
    expansion; aln_start counts the target bases in front of the cut.  Cuts inside an M, inside a D, on an op boundary,
    at s and at e are all met."""
    rng = np.random.default_rng(5)
    met = {"M": 0, "D": 0, "edge": 0, "s": 0, "e": 0}
    codes = set()
    for _ in range(120):
        tlen = int(rng.integers(40, 300))
        tseq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), tlen))
        s = int(rng.integers(0, tlen - 20)); e = int(rng.integers(s + 10, tlen + 1))
        pos, q, ops = _random_record(rng, tseq, s, e)
        codes |= {o & 15 for o in ops}
        start, qs, ts = ct.expand(pos, q, tseq, ops)
        pts = _cut_points(s, ops)
        cuts = {0, tlen}
        for kind in ("M", "D", "edge"):
            if pts[kind]:
                x = int(pts[kind][int(rng.integers(0, len(pts[kind])))])
                if x not in cuts:
                    cuts.add(x); met[kind] += 1
        if rng.random() < 0.5 and s not in cuts:
            cuts.add(s); met["s"] += 1
        if rng.random() < 0.5 and e not in cuts:
            cuts.add(e); met["e"] += 1
        cuts |= {int(x) for x in rng.integers(0, tlen, 3)}
        cuts = sorted(cuts)
        nxt = 0
        for a, b in zip(cuts, cuts[1:]):
            piece = wt.cut(pos, q, tseq, ops, a, b)
            if piece is None:
                assert max(a, s) >= min(b, e)
                continue
            st, pq, pt, c0, c1 = piece
            assert c0 == nxt and c1 > c0                           # the pieces' column ranges follow one another
            nxt = c1
            assert pq == qs[c0:c1] and pt == ts[c0:c1]
            A = max(a, s)
            assert st == A - a + 1
            assert sum(1 for ch in ts[:c0] if ch != ct.GAP) == A - s
            if A > s:
                assert pt[0] != ct.GAP                             # insertions in front of an interior cut stay left of it
        assert nxt == len(qs)                                      # ... and cover [0, columns)
    assert codes == {ct.M, ct.I, ct.D, ct.S, ct.H, ct.P, ct.EQ, ct.X}
    assert all(v > 10 for v in met.values()), met


def test_cut_overlapping_windows_and_nonconforming_span():
    """Overlapping windows give overlapping column ranges of the same expansion; a non-conforming record fails the
    windows its span meets and no other."""
    tseq = b"ACGTACGTACGTACGTACGT"
    ops = [ct.op("I", 2), ct.op("M", 4), ct.op("I", 1), ct.op("D", 3), ct.op("M", 5), ct.op("I", 2)]
    q = b"ttGTACgCGTACcc"
    assert ct.expand(3, q, tseq, ops) == (3, b"ttGTACg---CGTACcc", b"--GTAC-GTACGTAC--")
    # [s, e) = [2, 14): windows [0, 8) and [5, 20) overlap on [5, 8)
    # the leading insertion stays with the record; so does the insertion in front of base 6, which is left of the cut at 8
    assert wt.cut(3, q, tseq, ops, 0, 8) == (3, b"ttGTACg--", b"--GTAC-GT", 0, 9)
    # a cut at base 5, inside the M; the trailing insertion stays
    assert wt.cut(3, q, tseq, ops, 5, 20) == (1, b"Cg---CGTACcc", b"C-GTACGTAC--", 5, 17)
    # a cut at base 6 leaves the insertion in front of it out
    assert wt.cut(3, q, tseq, ops, 6, 9) == (1, b"---", b"GTA", 7, 10)
    assert wt.cut(3, q, tseq, ops, 14, 20) is None and wt.cut(3, q, tseq, ops, 0, 2) is None
    bad = [ct.op("M", 4), ct.op("N", 2), ct.op("M", 4)]
    targets = [(tseq, [(3, b"ACGTACGT", bad)])]
    res = wt.window_targets(targets, [(0, 0, 2), (0, 2, 6), (0, 9, 12), (0, 10, 20)])
    assert [f for _, _, f in res] == [False, True, True, False]     # span [2, 10): N consumes nothing
    assert wt.span(0, 20, ops) == (0, 12) and wt.span(30, 20, ops) == (19, 20)


# ---- CPU: the stitch ---------------------------------------------------------------------------------------------------

def _seg(first, n, begin, seq=None):
    """A segment of n bases whose positions are first, first + 1, ... (window-relative, 1-based)."""
    pos = np.arange(first, first + n)
    s = seq if seq is not None else bytes(65 + (int(p) + begin) % 26 for p in pos)
    return s, pos, None


def test_stitch_twin():
    """Join at the core boundary, a break inside a core, a segment that ends exactly at the core end, non-monotone
    positions, and the minimum length."""
    W, O, tlen = 100, 20, 250
    win = wt.tiled(tlen, W, O)
    assert win == [(0, 120, 0, 100), (80, 220, 100, 200), (180, 250, 200, 250)]
    # one segment per window, each spanning its whole window: one joined piece that covers the target once
    ws = [(b, c0, c1, [_seg(1, e - b, b)]) for b, e, c0, c1 in win]
    out = wt.stitch(ws, 10)
    assert len(out) == 1 and out[0][:2] == (0, 250) and out[0][2] == bytes(65 + g % 26 for g in range(1, 251))
    # a break inside the core of window 1: its first segment ends at global 150, the second starts at 161
    ws[1] = (80, 100, 200, [_seg(1, 70, 80), _seg(81, 60, 80)])
    out = wt.stitch(ws, 10)
    assert [(a, b) for a, b, _, _ in out] == [(0, 150), (160, 250)]
    # a segment that ends exactly at the core end was not cut there: no join with the next window
    ws[1] = (80, 100, 200, [_seg(1, 120, 80)])                      # global 81 .. 200
    out = wt.stitch(ws, 10)
    assert [(a, b) for a, b, _, _ in out] == [(0, 200), (200, 250)]
    # ... and one that starts exactly at the core begin of the next window was not cut there either
    ws[1] = (80, 100, 200, [_seg(1, 140, 80)])
    ws[2] = (180, 200, 250, [_seg(21, 50, 180)])                    # global 201 .. 250: nothing in front of the core
    out = wt.stitch(ws, 10)
    assert [(a, b) for a, b, _, _ in out] == [(0, 200), (200, 250)]
    # non-monotone positions: a merged insertion carries a position above the vertices that follow it; first crossings
    pos = np.concatenate([np.arange(1, 20), [23], np.arange(20, 141)])   # window 1: global 81 .. 99, 103, 100 .. 220
    seq = bytes(97 + i % 26 for i in range(pos.size))
    ws[1] = (80, 100, 200, [(seq, pos, None)])
    ws[2] = (180, 200, 250, [_seg(1, 70, 180)])
    out = wt.stitch(ws, 10)
    assert len(out) == 1
    t0, t1, s, extra = out[0]
    # window 0 gives global 1 .. 100 (100 bases); window 1 is kept from the base with g = 103 (index 19) to the first
    # g > 200 (index 121); window 2 from global 201
    assert (t0, t1) == (0, 250) and len(s) == 100 + (121 - 19) + 50
    assert s[100:202] == seq[19:121]
    # qualities are sliced as the bases are
    ws2 = [(b, c0, c1, [(sq, p, sq.lower())]) for (b, c0, c1, [(sq, p, _)]) in ws]
    out2 = wt.stitch(ws2, 10)
    assert out2[0][3] == out2[0][2].lower()
    # a window without segments (below min_cov) breaks the chain; short pieces are dropped
    ws = [(b, c0, c1, [_seg(1, e - b, b)]) for b, e, c0, c1 in win]
    ws[1] = (80, 100, 200, [])
    assert [(a, b) for a, b, _, _ in wt.stitch(ws, 10)] == [(0, 100), (200, 250)]
    assert [(a, b) for a, b, _, _ in wt.stitch(ws, 60)] == [(0, 100)]


def test_library_exports_the_window_entry_points():
    """The library exports the new symbols; the compiler's dagcon_windows is the size of its ctypes mirror; the flag
    has the value the header gives it and ABI stays 2."""
    import tempfile
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_fetch_positions", "dagcon_upload_cigar_windows", "dagcon_consensus_cigar_windows"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.dagcon_abi_version() == 2
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dagcon.h"
int main(void){printf("%zu %zu %zu %u %u\n", sizeof(dagcon_windows), offsetof(dagcon_windows, begin),
 offsetof(dagcon_windows, end), DAGCON_FLAG_BASE_POS, DAGCON_FLAGS_ALL); return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert out == [ctypes.sizeof(capi.Windows), capi.Windows.begin.offset, capi.Windows.end.offset, capi.FLAG_BASE_POS, 1 | 2 | 4 | 16 | 32 | 64 | 256]
    w = capi.HostWindows.tiled([250, 40, 0], 100, 20)
    assert list(zip(w.target.tolist(), w.begin.tolist(), w.end.tolist())) == [(0, 0, 120), (0, 80, 220), (0, 180, 250), (1, 0, 40)]


# ---- GPU: per-base positions ---------------------------------------------------------------------------------------------

def _check_pos(ctx, got, exp, targets=None):
    pos = ctx.base_positions()
    assert len(pos) == len(got) == len(exp)
    n = 0
    for t in (range(len(got)) if targets is None else targets):
        assert got[t] == [s[:3] for s in exp[t]], t
        assert len(pos[t]) == len(exp[t])
        for p, (_, _, seq, ep) in zip(pos[t], exp[t]):
            assert p.dtype == np.uint32 and p.size == len(seq)
            assert p.tolist() == ep, t
            n += p.size
    return n


def _pos_flags():
    from pbdagcon_amd import capi
    return capi.FLAG_BASE_POS, capi.FLAG_BASE_SUPPORT


def _both_ways(batch, exp, exp_pos, extra_flags=0, **kw):
    """BASE_POS alone and with BASE_SUPPORT: the consensus, the positions against the twin, and with both flags the
    support of a SUP-only context."""
    from pbdagcon_amd import capi
    POS, SUP = _pos_flags()
    sup_only = capi.Context(flags=SUP | extra_flags, **kw)
    try:
        assert sup_only.consensus(batch) == exp
        want_sup = sup_only.base_support()
    finally:
        sup_only.close()
    n = 0
    for flags in (POS, POS | SUP):
        ctx = capi.Context(flags=flags | extra_flags, **kw)
        try:
            got = ctx.consensus(batch)
            assert got == exp
            n += _check_pos(ctx, got, exp_pos)
            if flags & SUP:
                have = ctx.base_support()
                assert len(have) == len(want_sup)
                for a, b in zip(have, want_sup):
                    assert len(a) == len(b)
                    for (w0, d0), (w1, d1) in zip(a, b):
                        assert np.array_equal(w0, w1) and np.array_equal(d0, d1)
            else:
                with pytest.raises(capi.DagconError) as e:
                    ctx.fetch_support_raw()
                assert e.value.code == -8
        finally:
            ctx.close()
    assert n > 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_segments", [0, 1, 64])
def test_positions_full_span(max_segments):
    from pbdagcon_amd import synth
    batch = synth.make_batch(6, 2200, 16, seed=11 + max_segments)
    exp = oracle_batch(batch, 6, 500, 50)
    _both_ways(batch, exp, wt.batch_positions(batch, 6, 500, 50), min_cov=6, min_len=500, trim=50, max_segments=max_segments)


@pytest.mark.gpu
def test_positions_lane_walk(monkeypatch):
    """k_bp_walk_r with positions: forced on a small batch."""
    from pbdagcon_amd import synth
    batch = synth.make_batch(5, 3000, 20, seed=5)
    monkeypatch.setenv("DAGCON_BP_LANE", "2")
    exp = oracle_batch(batch, 6, 500, 50)
    _both_ways(batch, exp, wt.batch_positions(batch, 6, 500, 50), min_cov=6, min_len=500, trim=50)


@pytest.mark.gpu
def test_positions_partial_span_pileups():
    """k_cuts2 / k_bp_walk_g and its first piece, max_segments 0 / 64, DEBUG_RESWEEP.  Insertions give positions that
    repeat; the values are those of the oracle's _bbMap whatever their order."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(41)
    targets = []
    for tl, k in ((900, 14), (1400, 20), (2600, 9), (700, 30)):
        alns, bb = random_target(rng, tl, k, sub=0.04, ins=0.08, dele=0.05)
        targets.append((tl, alns, bb))
    batch = batch_from_targets(targets)
    exp = oracle_batch(batch, 3, 100, 5)
    exp_pos = wt.batch_positions(batch, 3, 100, 5)
    for extra, ms in ((0, 0), (0, 64), (capi.FLAG_DEBUG_RESWEEP, 0)):
        _both_ways(batch, exp, exp_pos, extra, min_cov=3, min_len=100, trim=5, max_segments=ms)
    flat = [p for t in exp_pos for s in t for p in s[3]]
    assert len(flat) != len(set(flat))


def _shifted_pileup(rng, tlen, lo, hi, n_reads):
    """A random_target pileup over positions [lo, hi) of a longer random backbone: nothing covers the rest."""
    alns, bb = random_target(rng, hi - lo, n_reads, sub=0.04, ins=0.08, dele=0.05)
    fill = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tlen - (hi - lo)))
    return tlen, [(s + lo, q, t) for s, q, t in alns], fill[:lo] + bb + fill[lo:]


@pytest.mark.gpu
@pytest.mark.parametrize("with_backbone", [False, True])
def test_positions_walk_lands_far_from_enter(with_backbone):
    """k_bp_walk_g's first piece when enter's best edge lands hundreds of ids away (the staging ring starts over after
    the jump; the piece stops at a cut that is not the first one), and a path that leaves for exit early.  With the
    backbones the uncovered vertices have weight 1: the -10 edges."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(7)
    targets = [_shifted_pileup(rng, 1500, 900, 1500, 12), _shifted_pileup(rng, 1500, 0, 600, 12),
               _shifted_pileup(rng, 2000, 700, 1400, 16)]
    batch = batch_from_targets(targets, with_backbone=with_backbone)
    exp = oracle_batch(batch, 3, 100, 5)
    exp_pos = wt.batch_positions(batch, 3, 100, 5)
    # what the test is about, on the reference's answer alone: the path's first base lies far behind enter (targets 0, 2),
    # its last one far before exit (target 1)
    assert all(len(segs) >= 1 for segs in exp_pos)
    lo = [min(p for s in segs for p in s[3]) for segs in exp_pos]
    hi = [max(p for s in segs for p in s[3]) for segs in exp_pos]
    assert lo[0] >= 800 and hi[1] <= 700 and lo[2] >= 600, (lo, hi)
    kw = dict(min_cov=3, min_len=100, trim=5)
    for extra, more in ((0, dict(max_segments=0)), (capi.FLAG_DEBUG_RESWEEP, dict(max_segments=0)),
                        (0, dict(max_segments=64)), (capi.FLAG_DEBUG_RESWEEP, dict(max_segments=64)),
                        (0, dict(max_segments=16, min_segment_len=4))):
        _both_ways(batch, exp, exp_pos, extra, **kw, **more)


@pytest.mark.gpu
def test_positions_real_backbone_and_resweep():
    from pbdagcon_amd import capi, synth
    batch = synth.make_batch(4, 1800, 14, seed=23, with_backbone=True)
    exp = oracle_batch(batch, 6, 500, 10)
    exp_pos = wt.batch_positions(batch, 6, 500, 10)
    for extra in (0, capi.FLAG_DEBUG_RESWEEP):
        _both_ways(batch, exp, exp_pos, extra, min_cov=6, min_len=500, trim=10)


@pytest.mark.gpu
def test_positions_state_errors():
    """DAGCON_ERR_STATE without the flag, before a fetch, under STOP_AFTER_*; n == seq_bytes."""
    from pbdagcon_amd import capi, synth
    POS, _ = _pos_flags()
    batch = synth.make_batch(2, 1200, 10, seed=2)
    plain = capi.Context()
    fresh = capi.Context(flags=POS)
    try:
        plain.consensus(batch)
        with pytest.raises(capi.DagconError) as e:
            plain.fetch_positions_raw()
        assert e.value.code == -8
        with pytest.raises(capi.DagconError) as e:
            fresh.fetch_positions_raw()
        assert e.value.code == -8
        fresh.upload(batch); fresh.run()
        with pytest.raises(capi.DagconError) as e:
            fresh.fetch_positions_raw()
        assert e.value.code == -8
        got = fresh.fetch()
        assert fresh.fetch_positions_raw().size == sum(len(s) for segs in got for _, _, s in segs) > 0
    finally:
        plain.close(); fresh.close()
    for stop in (capi.FLAG_STOP_AFTER_BUILD, capi.FLAG_STOP_AFTER_MERGE):
        c = capi.Context(flags=POS | stop)
        try:
            assert c.consensus(batch) == [[], []]
            with pytest.raises(capi.DagconError) as e:
                c.fetch_positions_raw()
            assert e.value.code == -8
        finally:
            c.close()


# ---- GPU: records cut to windows ---------------------------------------------------------------------------------------

def _contig(seed, tlen, n_reads, read_len, long_read=None):
    """A random target and conforming records mapped along it, in POS order: (target bases, [(pos, read, ops)])."""
    rng = np.random.default_rng(seed)
    alns_all, bb = random_target(rng, tlen, 1, full_span=True)
    recs = []
    spans = [(int(s), min(tlen, int(s) + read_len)) for s in sorted(rng.integers(0, max(1, tlen - read_len // 2), n_reads))]
    if long_read:
        spans.append(long_read)
        spans.sort()
    for k, (s, e) in enumerate(spans):
        sub_alns, _ = random_target(rng, e - s, 1, full_span=True)
        _, q, t = sub_alns[0]
        # the alignment was made against a random backbone of its own: put the contig's bases on its target side
        tb = bytearray(t); qb = bytearray(q); x = s
        for i in range(len(tb)):
            if tb[i] != ct.GAP:
                if qb[i] == tb[i]:
                    qb[i] = bb[x]
                tb[i] = bb[x]; x += 1
        recs.append(ct.compress(s + 1, bytes(qb), bytes(tb), bb, eqx=bool(k % 2)))
    return bb, recs


def _win_case():
    """Two targets.  Target 0 (3,000 bases): six windows of which two overlap, one no record reaches and one is below
    min_cov; one record crosses five of them.  Target 1: one window, the whole target."""
    bb0, recs0 = _contig(7, 3000, 60, 500, long_read=(150, 2450))
    # nothing maps to [2600, 3000) but one read: below min_cov; nothing at all to [2900, 3000)
    recs0 = [r for r in recs0 if wt.span(r[0], 3000, r[2])[1] <= 2600]
    recs0.append(ct.compress(2581, bb0[2580:2800], bb0[2580:2800], bb0))     # a perfect-match read over [2580, 2800)
    bb1, recs1 = _contig(9, 700, 12, 600)
    targets = [(bb0, recs0), (bb1, recs1)]
    windows = [(0, 0, 600), (0, 500, 1100), (0, 1100, 1600), (0, 1600, 2100), (0, 2100, 2700), (0, 2650, 2850), (0, 2900, 3000),
               (1, 0, 700)]
    return targets, windows


def _windows_obj(windows):
    from pbdagcon_amd import capi
    return capi.HostWindows([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])


def _cigar_batch(targets):
    from pbdagcon_amd import capi
    return capi.HostCigarBatch(**ct.records_to_arrays(targets))


def _strings_batch(wtargets):
    return batch_from_targets([(tl, alns, None) for tl, alns, _ in wtargets])


@pytest.mark.gpu
def test_windows_equal_strings_equal_oracle():
    """Per window: segments, support and positions of dagcon_consensus_cigar_windows are those of dagcon_consensus on
    the twin's piece strings, which equal the oracle's."""
    from pbdagcon_amd import capi
    import support_twin as st
    targets, windows = _win_case()
    wtargets = wt.window_targets(targets, windows)
    k = [len(a) for _, a, _ in wtargets]
    assert k[5] == 1 and k[6] == 0 and min(k[:5]) >= 6 and not any(f for _, _, f in wtargets)
    long_rec = [r for r in targets[0][1] if wt.span(r[0], 3000, r[2]) == (150, 2450)]
    assert len(long_rec) == 1 and sum(1 for g, a, b in windows[:7] if max(a, 150) < min(b, 2450)) == 5
    sb = _strings_batch(wtargets)
    cb, wo = _cigar_batch(targets), _windows_obj(windows)
    opts = dict(min_cov=4, min_len=100, trim=10)
    exp = oracle_batch(sb, 4, 100, 10)
    assert all(exp[i] for i in (0, 1, 2, 3, 4, 7)) and exp[5] == [] and exp[6] == []
    exp_pos = wt.batch_positions(sb, 4, 100, 10)
    exp_sup = st.batch_support(sb, 4, 100, 10)
    ctx = capi.Context(flags=capi.FLAG_BASE_POS | capi.FLAG_BASE_SUPPORT, **opts)
    try:
        for _ in range(2):                                           # (twice: the context's buffers are reused)
            got_s = ctx.consensus(sb)
            pos_s, sup_s = ctx.base_positions(), ctx.base_support()
            got_w = ctx.consensus_cigar_windows(cb, wo)
            assert got_w == got_s == exp
            assert ctx.target_status.tolist() == [0] * 8
            assert _check_pos(ctx, got_w, exp_pos) > 2000
            pos_w, sup_w = ctx.base_positions(), ctx.base_support()
            for a, b in zip(pos_w, pos_s):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
            for t, (a, b) in enumerate(zip(sup_w, sup_s)):
                assert [(w.tolist(), d.tolist()) for w, d in a] == [(w.tolist(), d.tolist()) for w, d in b]
                assert [(w.tolist(), d.tolist()) for w, d in a] == [(s[3], s[4]) for s in exp_sup[t]]
        # the three-step form, and the plain call on the same context afterwards
        ctx.upload_cigar_windows(cb, wo); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
        whole = capi.HostWindows([1], [0], [700])
        assert ctx.consensus_cigar_windows(cb, whole) == [exp[7]]
        assert ctx.consensus_cigar(_cigar_batch(targets[1:])) == [exp[7]]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_windows_graph_is_the_strings_graph():
    """DAGCON_FLAG_STOP_AFTER_BUILD on a small case: the graph addAln leaves is the same, vertex by vertex."""
    from pbdagcon_amd import capi
    bb, recs = _contig(17, 400, 14, 160)
    targets = [(bb, recs)]
    windows = [(0, 0, 150), (0, 100, 300), (0, 300, 400)]
    sb = _strings_batch(wt.window_targets(targets, windows))
    ctx = capi.Context(min_cov=0, min_len=0, trim=2, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    try:
        ctx.consensus(sb)
        a = [ctx.debug_graph(t) for t in range(3)]
        ctx.consensus_cigar_windows(_cigar_batch(targets), _windows_obj(windows))
        b = [ctx.debug_graph(t) for t in range(3)]
    finally:
        ctx.close()
    assert a == b and all(len(g) > 50 for g in a)


@pytest.mark.gpu
def test_windows_many_tiles_per_record():
    """Records of thousands of ops (tens of tiles; k_cigar_cut's search takes more than one round above 64 tiles): a
    26 kb target at 12x of full-length reads in windows of 5,000, against dagcon_consensus on the pieces."""
    from pbdagcon_amd import capi, synth
    big = synth.make_batch(1, 26000, 12, seed=3, with_backbone=True)
    arr = ct.compress_batch(big)
    cb = capi.HostCigarBatch(**arr)
    assert np.diff(cb.op_begin.astype(np.int64)).min() > 64 * 64
    bb = big.backbone.tobytes()
    recs = [(int(arr["pos"][a]), arr["q_blob"][int(arr["q_off"][a]):int(arr["q_off"][a]) + int(arr["q_len"][a])].tobytes(),
             arr["ops"][int(arr["op_begin"][a]):int(arr["op_begin"][a + 1])].tolist()) for a in range(12)]
    windows = [(0, b, e) for b, e, _, _ in wt.tiled(26000, 5000, 300)]
    sb = _strings_batch(wt.window_targets([(bb, recs)], windows))
    ctx = capi.Context()
    try:
        want = ctx.consensus(sb)
        assert all(want) and want == oracle_batch(sb)
        assert ctx.consensus_cigar_windows(cb, _windows_obj(windows)) == want
    finally:
        ctx.close()


@pytest.mark.gpu
def test_windows_nonconforming_record_fails_exactly_its_windows():
    from pbdagcon_amd import capi
    targets, windows = _win_case()
    bb0, recs0 = targets[0]
    # a record over [1150, 1650) with an N in it: windows 2 and 3 fail, the others are as before
    k = next(i for i, r in enumerate(recs0) if 1100 < wt.span(r[0], 3000, r[2])[0] < 1500 and 1650 < wt.span(r[0], 3000, r[2])[1] < 2050)
    p, q, ops = recs0[k]
    recs0 = list(recs0)
    recs0[k] = (p, q, ops[:3] + [ct.op("N", 4)] + ops[3:])
    bad_targets = [(bb0, recs0), targets[1]]
    wtargets = wt.window_targets(bad_targets, windows)
    assert [f for _, _, f in wtargets] == [False, False, True, True, False, False, False, False]
    exp = oracle_batch(_strings_batch(wtargets), 4, 100, 10)
    ctx = capi.Context(min_cov=4, min_len=100, trim=10)
    try:
        cb, wo = _cigar_batch(bad_targets), _windows_obj(windows)
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar_windows(cb, wo)
        assert e.value.code == -4
        got = ctx.consensus_cigar_windows(cb, wo, strict=False)
        assert ctx.target_status.tolist() == [0, 0, -4, -4, 0, 0, 0, 0]
        assert got == exp and got[2] == got[3] == [] and got[0] and got[1] and got[4] and got[7]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_windows_invalid_arguments():
    """end <= begin, end > tlen, a target out of range, windows out of order: DAGCON_ERR_INVALID_ARG; the existing
    refusals for a window too long or too deep."""
    from pbdagcon_amd import capi
    targets, windows = _win_case()
    cb = _cigar_batch(targets)
    ctx = capi.Context(min_cov=4, min_len=100, trim=10)
    try:
        for bad in ([(0, 100, 100)], [(0, 200, 100)], [(0, 0, 3001)], [(1, 0, 701)], [(2, 0, 10)],
                    [(1, 0, 700), (0, 0, 600)], [(0, 500, 1100), (0, 0, 600)]):
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cigar_windows(cb, _windows_obj(bad))
            assert e.value.code == -1, bad
        assert ctx.consensus_cigar_windows(cb, _windows_obj([])) == []
        # too deep: more pieces in one window than DAGCON_MAX_COVERAGE
        bb = targets[1][0]
        rec = ct.compress(1, bb[:150], bb[:150], bb)                 # (long enough to pass min_len: the limit counts those)
        deep = _cigar_batch([(bb, [rec] * (capi.MAX_COVERAGE + 1))])
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar_windows(deep, _windows_obj([(0, 0, 700)]))
        assert e.value.code == -5
        # too long: a window above the tlen limit that has records enough to be built (the limit is asked of those)
        tl = 4 * 65535
        tb = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGT", np.uint8), tl))
        long_t = _cigar_batch([(tb, [ct.compress(1, tb[:150], tb[:150], tb)] * 4)])
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar_windows(long_t, _windows_obj([(0, 0, tl)]))
        assert e.value.code == -5
        got = ctx.consensus_cigar_windows(long_t, _windows_obj([(0, 0, 1000), (0, tl - 1000, tl)]))
        assert len(got) == 2 and got[1] == [] and len(got[0]) == 1 and got[0][0][2] in tb[:150]
    finally:
        ctx.close()


# ---- end to end: pbdagcon --sam --ref --window ----------------------------------------------------------------------------

PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def mapped_reads(rng, bb, n_reads, read_len, sub=0.02, ins=0.04, dele=0.03):
    """n_reads records mapped at random offsets of the target bb, ascending in POS: [(pos, read, ops)] (numpy: one
    column per target base, an inserted column behind a base with probability ins; the ends are matches)."""
    tb = np.frombuffer(bb, np.uint8)
    tlen = tb.size
    recs = []
    for s in np.sort(rng.integers(0, max(1, tlen - read_len // 2), n_reads)):
        s = int(s); e = min(tlen, s + read_len)
        n = e - s
        u = rng.random(n)
        u[0] = u[-1] = 1.0
        q = tb[s:e].copy()
        subm = (u >= dele) & (u < dele + sub)
        q[subm] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(subm.sum()))
        q[u < dele] = ct.GAP
        insm = rng.random(n) < ins
        insm[-1] = False
        reps = 1 + insm.astype(np.int64)
        qs = np.repeat(q, reps); ts = np.repeat(tb[s:e], reps)
        second = np.cumsum(reps)[insm] - 1                             # the inserted column behind its base
        qs[second] = rng.choice(np.frombuffer(b"ACGT", np.uint8), second.size)
        ts[second] = ct.GAP
        recs.append(ct.compress(s + 1, qs.tobytes(), ts.tobytes(), bb, eqx=bool(len(recs) % 2)))
    return recs


def windowed_expected(names, targets, W, O, min_cov, min_len, trim, fastq):
    """twin cut + oracle per window + twin stitch, as the text pbdagcon --window prints."""
    import support_twin as st
    out = []
    for name, (bb, recs) in zip(names, targets):
        if not recs:
            continue
        spans = [wt.span(p, len(bb), ops) for p, _, ops in recs]
        ws = []
        for begin, end, c0, c1 in wt.tiled(len(bb), W, O):
            near = [r for r, (s, e) in zip(recs, spans) if s < end and e > begin]
            (tl, alns, failed), = wt.window_targets([(bb, near)], [(0, begin, end)])
            assert not failed
            segs = []
            if len(alns) >= max(min_cov, 1):
                for _, _, seq, ps, wv, dv in wt.target_positions(tl, alns, min_len, trim, min_cov, with_support=True):
                    segs.append((seq, ps, st.quality_string(wv, dv) if fastq else None))
            ws.append((begin, c0, c1, segs))
        for t0, t1, seq, qual in wt.stitch(ws, min_len):
            head = b"%s/%d_%d" % (name.encode(), t0, t1)
            out.append(b"@%s\n%s\n+\n%s\n" % (head, seq, qual) if fastq else b">%s\n%s\n" % (head, seq))
    return b"".join(out)


def _e2e_case(tmp_path, big=300000, depth=30):
    rng = np.random.default_rng(77)
    names = ["ctgA", "ctgB", "ctgC"]
    bbs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in (big, 5000, 4000)]
    targets = [(bbs[0], mapped_reads(rng, bbs[0], big * depth // 2000, 2000)),
               (bbs[1], mapped_reads(rng, bbs[1], 40, 2000)),
               (bbs[2], mapped_reads(rng, bbs[2], 3, 2000))]          # below -c
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta(names, bbs))
    sam = tmp_path / "in.sam"
    sam.write_bytes(ct.to_sam(names, [len(b) for b in bbs], [r for _, r in targets]))
    return names, targets, ref, sam


@pytest.mark.gpu
def test_pbdagcon_window_end_to_end(tmp_path):
    """A 300 kb target with 2 kb reads at 30x (about 4,500 records: above both per-target limits), a 5 kb target (one
    window) and a target below -c, through pbdagcon --sam --ref --window 10000: FASTA and --fastq byte for byte the
    twin cut + the oracle per window + the twin stitch, whatever --batch-targets; without --window the same command is
    refused as before."""
    names, targets, ref, sam = _e2e_case(tmp_path)
    assert len(targets[0][1]) > 4094 and len(targets[0][0]) > 262138

    def run(*args):
        return subprocess.run([_cli(), "--sam", "--ref", str(ref), *args, str(sam)], capture_output=True, timeout=900)
    want = windowed_expected(names, targets, 10000, 1000, 6, 500, 50, False)
    heads = [ln for ln in want.split(b"\n") if ln.startswith(b">")]
    assert any(h.startswith(b">ctgA/") for h in heads) and any(h.startswith(b">ctgB/") for h in heads)
    assert not any(h.startswith(b">ctgC/") for h in heads)
    print("expected records:", [h.decode() for h in heads])
    assert sum(len(x) for x in want.split(b"\n")[1::2]) > 290000
    out = run("--window", "10000")
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout == want
    out = run("--window", "10000", "--overlap", "1000", "--batch-targets", "7")
    assert out.returncode == 0 and out.stdout == want
    want_q = windowed_expected(names, targets, 10000, 1000, 6, 500, 50, True)
    out = run("--window", "10000", "--fastq")
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout == want_q
    plain = run()
    assert plain.returncode != 0 and plain.stderr


def test_window_usage_errors(tmp_path):
    """--window without --sam, with -a or --polish, --overlap below --trim + 64 or without --window: usage errors (exit
    2); records of one RNAME that are not ascending in POS: an error that names the line.  No GPU is needed to say so."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    rng = np.random.default_rng(3)
    bb = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000))
    recs = mapped_reads(rng, bb, 8, 800)
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [bb]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [3000], [recs]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    for args in (["--window", "1000", str(sam)], ["--sam", "--ref", str(ref), "--window", "1000", "-a", str(sam)],
                 ["--sam", "--ref", str(ref), "--window", "1000", "--polish", "1", str(sam)],
                 ["--sam", "--ref", str(ref), "--window", "1000", "--overlap", "113", str(sam)],
                 ["--sam", "--ref", str(ref), "--window", "1000", "-t", "10", "--overlap", "73", str(sam)],
                 ["--sam", "--ref", str(ref), "--overlap", "500", str(sam)], ["--sam", "--ref", str(ref), "--window", "0", str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
    h = run("--help")
    assert h.returncode == 0 and b"--window" in h.stdout and b"--overlap" in h.stdout and b"TARGET coordinates" in h.stdout
    # the accepted forms get as far as the device, which is not there
    for args in (["--window", "1000"], ["--window", "1000", "--overlap", "114"], ["--window", "1000", "-t", "10", "--overlap", "74"]):
        out = run("--sam", "--ref", str(ref), *args, str(sam))
        assert out.returncode == 1 and b"no CPU fallback" in out.stderr, args
    lines = ct.to_sam(["c"], [3000], [recs]).decode().splitlines()
    n_head = sum(1 for ln in lines if ln.startswith("@"))
    lines[n_head + 2], lines[n_head + 5] = lines[n_head + 5], lines[n_head + 2]
    assert int(lines[n_head + 3].split("\t")[3]) < int(lines[n_head + 2].split("\t")[3])
    bad = tmp_path / "bad.sam"; bad.write_text("\n".join(lines) + "\n")
    out = run("--sam", "--ref", str(ref), "--window", "1000", str(bad))
    assert out.returncode == 1 and ("line %d" % (n_head + 4)).encode() in out.stderr and b"POS" in out.stderr
