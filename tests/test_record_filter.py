"""The record filter (include/dagcon.h, dagcon_set_record_filter): --max-error and --max-depth for alignment records,
rated on the device.  The reference for the counts is tests/rate_twin.py; the reference for a selection is the same
entry point without a filter on a batch the test prunes on the host with the twin.

Every selection test asserts on the CPU, before the device runs, that the twin drops at least one record, keeps at
least one target or window at min_cov or above, and (for a cap) that some target or window is over the cap.
"""
import os
import subprocess

import numpy as np
import pytest

import bam_files as bf
import cigar_twin as ct
import cs_files as cf
import cs_twin as cst
import paf_files as pf
import rate_twin as rt
import window_twin as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
MIN_COV, MIN_LEN, TRIM = 4, 20, 5
NONCONFORMING, UNSUPPORTED, INVALID_ARG, STATE = -4, -5, -1, -8
PPM = 200000                       # 20 %: planted reads have every fourth base substituted (25 %)


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, timeout=600)


def _other(b):
    return b"ACGT"[(b"ACGT".index(bytes([b & 0xDF])) + 1) % 4] if bytes([b & 0xDF]) in (b"A", b"C", b"G", b"T") else 65


def _bases(rng, n):
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))


def _clean(rng, bb, pos, span):
    """A read of span target bases from pos at the generators' usual error rate: M / = / X runs (= and X truthful) with 3 %
    substitutions under M and short insertions and deletions between the runs."""
    ops, q, x, left = [], bytearray(), pos - 1, span
    while left > 0:
        n = min(left, int(rng.integers(10, 30)))
        kind = "M=X"[int(rng.choice(3, p=[0.8, 0.17, 0.03]))]
        if kind == "X":
            n = 1
        for k in range(n):
            b = bb[x + k]
            q.append(_other(b) if kind == "X" or (kind == "M" and rng.random() < 0.03) else b)
        ops.append(ct.op(kind, n)); x += n; left -= n
        if left > 3 and rng.random() < 0.4:
            if rng.random() < 0.5:
                k = int(rng.integers(1, 3)); ops.append(ct.op("I", k)); q.extend(_bases(rng, k))
            else:
                ops.append(ct.op("D", 1)); x += 1; left -= 1
    return pos, bytes(q), ops


def _planted(bb, pos, span):
    """A bad read: one M op, every fourth base substituted."""
    q = bytearray(bb[pos - 1:pos - 1 + span])
    for k in range(0, span, 4):
        q[k] = _other(q[k])
    return pos, bytes(q), [ct.op("M", span)]


def _pileup(seed, tlens=(300, 310, 290), depth=12, bad_at=(2, 6, 10), thin=True):
    """Targets of about 300 bases at 12x with three planted bad reads each, records ascending in pos; thin: one more target
    with 3 clean and 2 planted reads, at min_cov only without the filter."""
    rng = np.random.default_rng(seed)
    targets = []
    for tl in tlens:
        bb = _bases(rng, tl)
        recs = []
        for k in range(depth + len(bad_at)):
            span = int(rng.integers(120, 200))
            s = min(tl - span, k * (tl - 100) // (depth + len(bad_at) - 1))
            recs.append(_planted(bb, s + 1, span) if k in bad_at else _clean(rng, bb, s + 1, span))
        targets.append((bb, sorted(recs, key=lambda r: r[0])))       # (stable: a coordinate-sorted file)
    if thin:
        bb = _bases(rng, 200)
        targets.append((bb, [_clean(rng, bb, 1, 180), _planted(bb, 5, 180), _clean(rng, bb, 11, 180), _planted(bb, 15, 180),
                             _clean(rng, bb, 21, 179)]))
    return targets


def _prune(targets, kept):
    return [(bb, [recs[k] for k in keep]) for (bb, recs), keep in zip(targets, kept)]


def _assert_not_vacuous(targets, pk, depth=0, groups=None):
    """The conditions on every selection test, from the twin alone."""
    assert any(f & (rt.FATE_MAX_ERROR | rt.FATE_MAX_DEPTH) for f in pk.fate), "the twin drops nothing"
    assert any(len(k) >= MIN_COV for k in pk.kept), "the twin keeps nothing above min_cov"
    if depth:
        assert any(len(k) == depth for k in pk.kept) and pk.n_over_depth() > 0, "nothing is over the cap"


def _everything(ctx, segs):
    tm = ctx.timings()
    return (segs, ctx.target_status.tolist(), ctx.base_support(), ctx.base_positions(),
            [tm[k] for k in ("n_alignments", "n_columns", "n_nodes", "consensus_bases", "algorithmic_bytes")])


def _same(got, exp):
    assert got[0] == exp[0] and got[1] == exp[1] and got[4] == exp[4]
    for x, y in ((got[2], exp[2]), (got[3], exp[3])):
        assert len(x) == len(y)
        for sx, sy in zip(x, y):
            assert len(sx) == len(sy)
            for ex, ey in zip(sx, sy):
                if isinstance(ex, tuple):
                    assert all(np.array_equal(u, v) for u, v in zip(ex, ey))
                else:
                    assert np.array_equal(ex, ey)


def _context(**kw):
    from pbdagcon_amd import capi
    kw = dict(dict(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS), **kw)
    return capi.Context(**kw)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def _hand_records():
    """Hand-written records on four targets: every edge the rating kernels have (named in the GPU test)."""
    rng = np.random.default_rng(7)
    t0 = bytearray(_bases(rng, 700))
    t1 = bytearray(_bases(rng, 200))
    t1[40:50] = b"acgtnNacgt"                                        # lower case and N on the target side
    t2 = _bases(rng, 4300)
    t3 = _bases(rng, 120)
    t0, t1 = bytes(t0), bytes(t1)
    unit = [ct.op("M", 3), ct.op("I", 1), ct.op("M", 3), ct.op("D", 1)]

    def read(bb, pos, ops, flip=()):
        """The read ops ask for: target bases under M / = / X (upper-cased; flip: read-base indices substituted), random
        bases under I and S."""
        q, x = bytearray(), pos - 1
        for o in ops:
            code, n = o & 15, o >> 4
            if code in (ct.M, ct.EQ, ct.X):
                q.extend(bytes(bb[x:x + n]).upper()); x += n
            elif code in (ct.I, ct.S):
                q.extend(_bases(rng, n))
            elif code == ct.D:
                x += n
        for i in flip:
            q[i] = _other(q[i])
        return pos, bytes(q), list(ops)

    clip = read(t0, 300, [ct.op("H", 5), ct.op("S", 3), ct.op("M", 50), ct.op("P", 2), ct.op("I", 2), ct.op("M", 40), ct.op("S", 2)], flip=(10,))
    clip = (clip[0], clip[1][:20] + b"=" + clip[1][21:], clip[2])     # a BAM '=' base under M: matches only '='
    case = read(t1, 36, [ct.op("M", 20)])
    case = (case[0], case[1][:2].lower() + b"N" + case[1][3:8] + b"N" + case[1][9:], case[2])   # lower case and N on the read side
    named = [
        (0, "ops64", read(t0, 11, unit * 16, flip=(5, 40))),
        (0, "ops65", read(t0, 150, unit * 16 + [ct.op("M", 3)])),
        (0, "m200", read(t0, 400, [ct.op("M", 200)], flip=tuple(range(0, 200, 7)))),
        (0, "clip", clip),
        (0, "nocol_tile", read(t0, 500, [ct.op("S", 1)] * 64 + [ct.op("M", 30)], flip=(70,))),
        (1, "ins_edges", read(t1, 5, [ct.op("I", 3), ct.op("M", 20), ct.op("I", 2)])),
        (1, "eqx_lies", read(t1, 100, [ct.op("=", 10), ct.op("X", 5), ct.op("M", 10)], flip=(1, 4, 7))),
        (1, "case", case),
        (1, "empty", (1, b"", [])),
        (2, "big", read(t2, 50, [ct.op("M", 1), ct.op("I", 1)] * 4200, flip=tuple(range(0, 8400, 10)))),
        (3, "bad_op", read(t3, 10, [ct.op("M", 20), ct.op("N", 5), ct.op("M", 20)])),
        (3, "clean", read(t3, 20, [ct.op("M", 60)], flip=(3,))),
    ]
    bbs = [t0, t1, t2, t3]
    targets = [(bb, [r for g, _, r in named if g == i]) for i, bb in enumerate(bbs)]
    return targets, {n: r for _, n, r in named}


def test_twin_counts_add_up_to_the_columns():
    targets, rec = _hand_records()
    pk = rt.pick(targets)
    flat = [(bb, r) for bb, recs in targets for r in recs]
    assert len(flat) == 12
    for (bb, (p, q, o)), c, f in zip(flat, pk.counts, pk.fate):
        if f & rt.FATE_NONCONFORMING:
            assert c == (0, 0, 0, 0) and not ct.conforming(p, len(q), len(bb), o)
            continue
        assert sum(c) == rt.columns(o) == len(ct.expand(p, q, bb, o)[1])
        # against the expanded strings: a column of two bases matches when they are equal but for the case bit
        _, qs, ts = ct.expand(p, q, bb, o)
        both = [(a, b) for a, b in zip(qs, ts) if a != ct.GAP and b != ct.GAP]
        assert c[0] == sum((a & 0xDF) == (b & 0xDF) for a, b in both) and c[1] == len(both) - c[0]
        assert c[2] == sum(b == ct.GAP for b in ts) and c[3] == sum(a == ct.GAP for a in qs)
    assert [f for f in pk.fate if f] == [rt.FATE_NONCONFORMING]
    # the edges are what they claim
    assert len(rec["ops64"][2]) == 64 and len(rec["ops65"][2]) == 65 and len(rec["big"][2]) == 8400 > 64 * 64
    assert all(o & 15 == ct.S for o in rec["nocol_tile"][2][:64])
    assert (rec["clip"][2][1] >> 4) % 2 == 1 and rec["clip"][2][1] & 15 == ct.S and b"=" in rec["clip"][1]
    assert rec["ins_edges"][2][0] & 15 == ct.I and rec["ins_edges"][2][-1] & 15 == ct.I
    p, q, o = rec["eqx_lies"]
    assert rt.rate(p, q, targets[1][0], o) == (22, 3, 0, 0)           # three of the = columns differ, the X columns agree
    p, q, o = rec["case"]
    assert rt.rate(p, q, targets[1][0], o)[1] == 2 and any(97 <= b <= 122 for b in q)   # only N against a base differs... twice
    # strand and nibbles give the same counts from the bytes as the batch carries them
    p, q, o = rec["m200"]
    assert rt.rate(p, pf.revcomp(q), targets[0][0], o, reverse=True) == rt.rate(p, q, targets[0][0], o)
    p, q, o = rec["clip"]
    assert rt.rate(p, bf.pack_nibbles(q), targets[0][0], o, packed=True, q_len=len(q)) == rt.rate(p, q, targets[0][0], o)


def test_threshold_boundary():
    """100 columns with 15 errors: kept at 150000 ppm, dropped at 149999; a record of 0 columns passes anything."""
    bb = b"ACGT" * 30
    q = bytearray(bb[:50])
    for k in range(0, 44, 4):
        q[k] = _other(q[k])                                           # 11 mismatches
    rec = (1, bytes(q) + b"GG" + bb[50:73] + bb[75:98], [ct.op("M", 50), ct.op("I", 2), ct.op("M", 23), ct.op("D", 2), ct.op("M", 23)])
    c = rt.rate(rec[0], rec[1], bb, rec[2])
    assert sum(c) == 100 and c[1] + c[2] + c[3] == 15
    assert rt.passes(c, 150000) and not rt.passes(c, 149999)
    assert rt.pick([(bb, [rec])], 150000).fate == [0] and rt.pick([(bb, [rec])], 149999).fate == [rt.FATE_MAX_ERROR]
    assert rt.passes((0, 0, 0, 0), 0) and rt.passes((7, 0, 0, 0), 0) and not rt.passes((7, 1, 0, 0), 0)


def test_cap_ties_go_to_the_lower_index_and_order_stays():
    assert rt.cap([5, 9, 5, 9, 5], 3) == [0, 1, 3]                    # both 9s, then the first of the 5s
    assert rt.cap([5, 9, 5, 9, 5], 4) == [0, 1, 2, 3]
    assert rt.cap([1, 2, 3], 3) == [0, 1, 2] and rt.cap([1, 2, 3], 0) == [0, 1, 2]
    assert rt.cap([3, 1, 2], 1) == [0] and rt.cap([7, 7, 7], 2) == [0, 1]
    bb = b"ACGT" * 20
    recs = [(1, bb[:40], [ct.op("M", 40)]), (1, bb[:60], [ct.op("M", 60)]), (1, bb[:40], [ct.op("M", 40)])]
    pk = rt.pick([(bb, recs)], max_depth=2)
    assert pk.kept == [[0, 1]] and pk.fate == [0, 0, rt.FATE_MAX_DEPTH]


def _small_sam(tmp_path):
    bb = b"ACGTTGCA" * 10
    ref = tmp_path / "r.fa"
    ref.write_bytes(ct.to_fasta(["t"], [bb]))
    sam = tmp_path / "in.sam"
    sam.write_bytes(ct.to_sam(["t"], [len(bb)], [[(1, bb[:40], [ct.op("M", 40)])]]))
    return ref, sam


@pytest.mark.parametrize("text", ["0", "1", "0.15", "0.000001", "1.0", "1.000000", "0.5", "0.999999", "0.1500",
                                  "", ".5", "0.", "1.000001", "2", "0.1234567", "-0.1", "1e-1", "0,5", "00.5", "0.5x", "+0.5", "1.5"])
def test_max_error_text_is_parsed_without_floating_point(tmp_path, text):
    ref, sam = _small_sam(tmp_path)
    want = rt.parse_ppm(text)
    out = _run("--sam", "--ref", str(ref), "--max-error", text, "--max-depth", "8", "--dump-parsed", str(sam))
    if want is None:
        assert out.returncode == 2 and b"PARSE ERROR: --max-error" in out.stderr
    else:
        assert out.returncode == 0, out.stderr.decode()
        assert b"pbdagcon: record filter: max_error_ppm %d max_depth 8\n" % want in out.stderr
    assert rt.parse_ppm("0.15") == 150000 and rt.parse_ppm("0.000001") == 1 and rt.parse_ppm("1") == 1000000


def test_record_filter_usage_errors(tmp_path):
    ref, sam = _small_sam(tmp_path)
    m5 = tmp_path / "in.m5"
    m5.write_bytes(b"")
    for args in (["--sam", "--ref", str(ref), "--max-depth", "4095", str(sam)],
                 ["--sam", "--ref", str(ref), "--max-depth", "0", str(sam)],
                 ["--sam", "--ref", str(ref), "--max-depth", "x", str(sam)],
                 ["--sam", "--ref", str(ref), "--max-error", str(sam)],
                 ["--max-error", "0.1", str(m5)], ["--max-depth", "5", str(m5)],
                 ["-a", "--max-error", "0.1", str(m5)], ["-a", "--max-depth", "5", str(m5)]):
        out = _run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, (args, out.stderr)
    assert _run("--sam", "--ref", str(ref), "--max-depth", "4094", "--dump-parsed", str(sam)).returncode == 0
    helptext = _run("--help").stdout
    assert b"--max-error F" in helptext and b"--max-depth N" in helptext


def test_planted_and_clean_reads_lie_on_either_side_of_the_threshold():
    """What the selection tests rely on, from the twin alone."""
    for seed in (31, 32, 33):
        targets = _pileup(seed)
        pk = rt.pick(targets, PPM)
        i = 0
        for bb, recs in targets:
            for p, q, o in recs:
                planted = len(o) == 1
                assert bool(pk.fate[i] & rt.FATE_MAX_ERROR) == planted
                i += 1
        assert len(pk.kept[3]) == 3 < MIN_COV <= len(targets[3][1])   # the thin target falls below min_cov by the filter only


# ---- GPU: counts ----------------------------------------------------------------------------------------------------

def _forms(targets):
    """The four sources of one set of records, each with the twin's counts and fates for what it carries."""
    from pbdagcon_amd import capi
    n = sum(len(r) for _, r in targets)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    upper = [(bb, [(p, q.upper(), o) for p, q, o in recs]) for bb, recs in targets]          # BAM has no letter case
    packed = capi.HostCigarBatch(**ct.records_to_arrays(upper)).packed()
    packed_twin = [(bb, [(p, (bf.pack_nibbles(q), len(q)), o) for p, q, o in recs]) for bb, recs in upper]
    reverse = (np.arange(n) % 2 == 1).astype(np.uint8)
    as_file, i = [], 0
    for bb, recs in targets:
        as_file.append((bb, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(recs)]))
        i += len(recs)
    stranded = capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file))
    # cs: no clips, no padding, no N op; a record that is non-conforming claims one read base too many instead
    cs_in, cs_twin = [], []
    for bb, recs in targets:
        a, b = [], []
        for p, q, o in recs:
            if any((x & 15) in (ct.S, ct.H, ct.P) for x in o):
                continue
            if not ct.conforming(p, len(q), len(bb), o):
                q = bytes(bb[p - 1:p + 29]); o = [ct.op("M", 30)]
                a.append((p, len(q) + 1, 30, cst.encode(p, q, bb, o)))
                b.append((p, q + b"A", o))                                                    # (q_len and ops disagree: non-conforming)
                continue
            text = cst.encode(p, q, bb, o)
            dops, dq, fl = cst.decode(text, bb, p)
            assert fl == 0
            a.append((p, len(q), pf.tspan(o), text)); b.append((p, dq, dops))
        cs_in.append((bb, a)); cs_twin.append((bb, b))
    return {
        "plain": (plain, rt.pick(targets)),
        "packed": (packed, rt.pick(packed_twin, packed=True)),
        "stranded": (stranded, rt.pick(as_file, reverse=reverse.tolist())),
        "cs": (capi.HostCsBatch.from_records(cs_in), rt.pick(cs_twin)),
    }


def _stats_equal(st, pk):
    assert st["fate"].tolist() == pk.fate
    got = np.stack([st["match"], st["mismatch"], st["ins"], st["del"]], axis=1).tolist() if len(pk.fate) else []
    assert got == [list(c) for c in pk.counts]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "packed", "stranded", "cs"])
def test_counts_equal_the_twin(kind):
    """dagcon_fetch_record_stats against the twin, record by record, on the hand-written edges: 64 and 65 ops, a tile
    without a column, one M of 200, an odd leading clip, I first and last, = and X ops that lie, lower case and N on either
    side, a BAM '=' base, 0 ops, 8,400 ops (132 tiles: k_cigar_rate_sum's second round), and one non-conforming record."""
    targets, _ = _hand_records()
    batch, pk = _forms(targets)[kind]
    assert rt.FATE_NONCONFORMING in pk.fate and max(sum(c) for c in pk.counts) >= 8400
    ctx = _context(min_cov=1, min_len=1, trim=0)
    try:
        ctx.set_record_filter()                                         # {1000000, 0}: counts only
        segs = ctx.consensus_cs(batch, strict=False) if kind == "cs" else ctx.consensus_cigar(batch, strict=False)
        _stats_equal(ctx.record_stats(), pk)
        assert ctx.target_status.tolist() == [0, 0, 0, NONCONFORMING] and segs[3] == []
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4, 5])
def test_counts_with_idle_waves_in_the_last_workgroup(n):
    """k_cigar_rate_sum runs four records to a workgroup: 1, 4 and 5 records."""
    from pbdagcon_amd import capi
    targets, _ = _hand_records()
    sub = [(targets[0][0], targets[0][1][:n])]
    pk = rt.pick(sub)
    ctx = _context(min_cov=1, min_len=1, trim=0)
    try:
        ctx.set_record_filter()
        ctx.upload_cigar(capi.HostCigarBatch(**ct.records_to_arrays(sub)))
        _stats_equal(ctx.record_stats(), pk)
    finally:
        ctx.close()


# ---- GPU: selection, whole targets ----------------------------------------------------------------------------------

def _call(ctx, kind, targets, windows=None, reverse=None):
    """One consensus call of the kind on targets = [(bb, [(pos, read in target orientation, ops)])]."""
    from pbdagcon_amd import capi
    hw = None if windows is None else capi.HostWindows([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
    if kind == "cs":
        b = capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs]) for bb, recs in targets])
        return _everything(ctx, ctx.consensus_cs(b, hw, strict=False))
    if kind == "stranded":
        b = capi.HostCigarBatch(reverse=np.ones(sum(len(r) for _, r in targets), np.uint8),
                                **ct.records_to_arrays([(bb, [(p, pf.revcomp(q), o) for p, q, o in recs]) for bb, recs in targets]))
    else:
        b = capi.HostCigarBatch(**ct.records_to_arrays(targets))
        if kind == "packed":
            b = b.packed()
    return _everything(ctx, ctx.consensus_cigar(b, strict=False) if hw is None else ctx.consensus_cigar_windows(b, hw, strict=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ppm,depth", [("plain", PPM, 0), ("plain", 1000000, 8), ("plain", PPM, 8),
                                            ("packed", PPM, 8), ("stranded", PPM, 8), ("cs", PPM, 8)])
def test_selection_of_whole_targets_equals_the_pruned_batch(kind, ppm, depth):
    targets = _pileup(31)
    pk = rt.pick(targets, ppm, depth)
    _assert_not_vacuous(targets, pk, depth)
    if ppm != 1000000:
        assert len(pk.kept[3]) < MIN_COV <= len(targets[3][1])          # below min_cov only because of the filter
    ctx = _context()
    try:
        want = _call(ctx, kind, _prune(targets, pk.kept))
        assert sum(bool(s) for s in want[0]) >= 3 and (ppm == 1000000 or want[0][3] == [])
        ctx.set_record_filter(ppm, depth)
        got = _call(ctx, kind, targets)
        st = ctx.record_stats()
        _same(got, want)
        assert st["fate"].tolist() == pk.fate
        assert st["match"].tolist() == [c[0] for c in pk.counts]
        ctx.set_record_filter(None, None)
        unfiltered = _call(ctx, kind, targets)
        assert unfiltered[0] != got[0]                                   # the filter changed the answer
    finally:
        ctx.close()


# ---- GPU: selection, windows ----------------------------------------------------------------------------------------

def _windows(targets, W=100, O=10):
    return [(g, b, e) for g, (bb, _) in enumerate(targets) for b, e, _, _ in wt.tiled(len(bb), W, O)]


@pytest.mark.gpu
def test_windows_max_error_equals_the_pruned_batch():
    targets = _pileup(32)
    wins = _windows(targets)
    pk = rt.pick(targets, PPM, 0, windows=wins)
    _assert_not_vacuous(targets, pk)
    whole = rt.pick(targets, PPM, 0)
    ctx = _context()
    try:
        want = _call(ctx, "plain", _prune(targets, whole.kept), wins)
        assert sum(bool(s) for s in want[0]) >= 6
        ctx.set_record_filter(PPM, 0)
        got = _call(ctx, "plain", targets, wins)
        _same(got, want)
        assert ctx.record_stats()["fate"].tolist() == pk.fate
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ppm", [1000000, PPM])
def test_windows_max_depth_equals_one_pruned_call_per_window(ppm):
    """The cap is taken window by window: the reference is one unfiltered call per window on that window's kept records."""
    D = 6
    targets = _pileup(33, thin=False)
    wins = _windows(targets)
    assert any(a[0] == b[0] and b[1] < a[2] for a, b in zip(wins, wins[1:]))       # neighbours overlap
    pk = rt.pick(targets, ppm, D, windows=wins)
    _assert_not_vacuous(targets, pk, D)
    # a record that stays in one window and is capped out of its neighbour
    first = np.cumsum([0] + [len(r) for _, r in targets])
    split = [i for i, f in enumerate(pk.fate) if f & rt.FATE_MAX_DEPTH and
             any(first[g] + k == i for (g, _, _), keep in zip(wins, pk.kept) for k in keep)]
    assert split, "no record is kept in one window and capped out of another"
    ctx = _context()
    try:
        want = []
        for (g, b, e), keep in zip(wins, pk.kept):
            bb, recs = targets[g]
            want.append(_call(ctx, "plain", [(bb, [recs[k] for k in keep])], [(0, b, e)]))
        ctx.set_record_filter(ppm, D)
        got = _call(ctx, "plain", targets, wins)
        assert ctx.record_stats()["fate"].tolist() == pk.fate
        assert sum(bool(s) for s in got[0]) >= 6
        for w, one in enumerate(want):
            assert got[0][w] == one[0][0] and got[1][w] == one[1][0]
            _same(([got[0][w]], [got[1][w]], [got[2][w]], [got[3][w]], None), (one[0], one[1], one[2], one[3], None))
        assert got[4][0] == sum(o[4][0] for o in want)                   # n_alignments: the kept pieces, all windows
    finally:
        ctx.close()


# ---- GPU: the depth wall --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wall():
    """One target of 60 bases under 4,100 records of about 30: one more than DAGCON_MAX_COVERAGE + 5."""
    rng = np.random.default_rng(5)
    bb = _bases(rng, 60)
    recs = []
    for _ in range(4100):
        span = int(rng.integers(28, 33))
        s = int(rng.integers(0, 60 - span + 1))
        q = bytearray(bb[s:s + span])
        for k in rng.integers(0, span, int(rng.integers(0, 3))):
            q[k] = _other(q[k])
        recs.append((s + 1, bytes(q), [ct.op("M", span)]))
    return [(bb, recs)]


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [None, [(0, 0, 60)]])
def test_depth_wall(wall, windows):
    from pbdagcon_amd import capi
    pk = rt.pick(wall, 1000000, 64, windows=windows)
    _assert_not_vacuous(wall, pk, 64)
    assert len(wall[0][1]) > capi.MAX_COVERAGE and pk.n_over_depth() == 4100 - 64
    ctx = _context(min_len=20, trim=2)
    try:
        with pytest.raises(capi.DagconError) as e:                       # as ever without a filter
            _call(ctx, "plain", wall, windows)
        assert e.value.code == UNSUPPORTED
        want = _call(ctx, "plain", _prune(wall, pk.kept), windows)
        assert want[0][0] and want[4][0] == 64
        ctx.set_record_filter(max_depth=64)
        got = _call(ctx, "plain", wall, windows)
        _same(got, want)
        assert ctx.record_stats()["fate"].tolist() == pk.fate
    finally:
        ctx.close()


# ---- GPU: state rules -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_state_rules_and_invalid_filters():
    from pbdagcon_amd import capi, synth
    targets = _pileup(31)
    ctx = _context()
    try:
        def stats_code():
            with pytest.raises(capi.DagconError) as e:
                ctx.record_stats()
            return e.value.code
        plain = _call(ctx, "plain", targets)
        assert stats_code() == STATE                                     # no filter
        for bad in ((1000001, 0), (0, capi.MAX_COVERAGE + 1)):
            with pytest.raises(capi.DagconError) as e:
                ctx.set_record_filter(*bad)
            assert e.value.code == INVALID_ARG
        ctx.set_record_filter(PPM, 8)
        assert stats_code() == STATE                                     # no upload under it yet
        picked = _call(ctx, "plain", targets)
        assert len(ctx.record_stats()["fate"]) == sum(len(r) for _, r in targets) and picked[0] != plain[0]
        ctx.consensus(synth.make_batch(1, 300, 8, seed=3))
        assert stats_code() == STATE                                     # another kind of upload since
        ctx.set_record_filter(1000000, capi.MAX_COVERAGE)               # the largest legal cap
        ctx.set_record_filter(None, None)
        _same(_call(ctx, "plain", targets), plain)                       # off again: the unfiltered answer
        assert stats_code() == STATE
    finally:
        ctx.close()


# ---- GPU: the command line ------------------------------------------------------------------------------------------

def _files(tmp_path, tag, kind, names, targets):
    """The input of one kind for targets (records ascending in pos), and the arguments that name it."""
    ref = tmp_path / (tag + ".ref.fa")
    ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets], width=50))
    if kind == "sam":
        f = tmp_path / (tag + ".sam")
        f.write_bytes(ct.to_sam(names, [len(bb) for bb, _ in targets], [recs for _, recs in targets]))
        return ["--sam", "--ref", str(ref), str(f)]
    if kind == "bam":
        f = tmp_path / (tag + ".bam")
        recs = [dict(ref=g, pos=p, qname="q%d_%d" % (g, k), flag=0, ops=o, seq=q) for g, (_, rr) in enumerate(targets) for k, (p, q, o) in enumerate(rr)]
        f.write_bytes(bf.bgzf(bf.bam_bytes([(n, len(bb)) for n, (bb, _) in zip(names, targets)], recs)))
        return ["--bam", "--ref", str(ref), str(f)]
    reads, alns = pf.from_twin(np.random.default_rng(9), names, targets, alphabet=b"ACGT", shared=0, sort_pos=True)
    assert [(x["tname"], x["ts"] + 1, x["ops"]) for x in alns] == [(n, p, o) for n, (_, rr) in zip(names, targets) for p, _, o in rr]
    f = tmp_path / (tag + ".paf")
    if kind == "paf":
        rd = tmp_path / (tag + ".reads.fa")
        rd.write_bytes(pf.reads_fasta(reads))
        f.write_bytes(pf.paf_text(reads, alns))
        return ["--paf", "--ref", str(ref), "--reads", str(rd), str(f)]
    alns = cf.with_cs(reads, alns, {n: bb for n, (bb, _) in zip(names, targets)})
    f.write_bytes(cf.paf_text(reads, [dict(x, cg=False) for x in alns]))
    return ["--paf", "--cs", "--ref", str(ref), str(f)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sam", "bam", "paf", "cs"])
def test_pbdagcon_flags_equal_the_file_without_the_dropped_lines(tmp_path, kind):
    """--max-error 0.2 --max-depth 8 prints what the same command without the flags prints on the file without the records
    the twin drops, once with --fastq and once with --window (one window a target: the cap of a window is that of its
    target, so leaving lines out says it); stderr names the twin's two counts."""
    targets = [(bb, [(p, q, o) for p, q, o in recs]) for bb, recs in _pileup(34, thin=False)]
    names = ["ctg%d" % g for g in range(len(targets))]
    pk = rt.pick(targets, PPM, 8)
    _assert_not_vacuous(targets, pk, 8)
    assert pk.n_over_error() == 9 and pk.n_over_depth() == 12
    wins = [(g, 0, len(bb)) for g, (bb, _) in enumerate(targets)]
    assert rt.pick(targets, PPM, 8, windows=wins).kept == pk.kept
    full = _files(tmp_path, "full", kind, names, targets)
    pruned = _files(tmp_path, "pruned", kind, names, _prune(targets, pk.kept))
    opts = ["-c", str(MIN_COV), "-m", "50", "-t", "5"]
    flags = ["--max-error", "0.2", "--max-depth", "8"]
    line = b"pbdagcon: records left out: %d by --max-error, %d by --max-depth\n" % (pk.n_over_error(), pk.n_over_depth())
    for mode in (["--fastq"], ["--window", "1000", "--overlap", "69"]):
        want = _run(*opts, *mode, *pruned)
        assert want.returncode == 0 and want.stdout.count(b"ctg") >= 3, want.stderr.decode()
        got = _run(*opts, *mode, *flags, *full)
        assert got.returncode == 0, got.stderr.decode()
        assert got.stdout == want.stdout
        assert line in got.stderr and b"records left out" not in want.stderr
        assert _run(*opts, *mode, *full).stdout != got.stdout            # the flags changed the answer
