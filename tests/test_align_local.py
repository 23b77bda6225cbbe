"""The local-end mode of the -a aligner (DAGCON_FLAG_LOCAL_ALIGN, pbdagcon -a --local): its CPU twin
(align_local_twin.py) against a plain full-matrix local DP and the reference's one SimpleAligner known-answer test; the
SimpleAligner.cpp:51-62 finish in local mode; then the device (dagcon_align, dagcon_align_ends, dagcon_consensus_pre,
the command line) against the twin, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import align_local_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
RC = bytes.maketrans(b"ACGT", b"TGCA")


def _kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kat_graph.json")))["simple_aligner"]


def _rand(rng, n):
    return bytes(b"ACGT"[j] for j in rng.integers(0, 4, int(n)))


def _mutate(rng, t, sub=0.03, ins=0.08, dele=0.05):
    q = bytearray()
    for c in t:
        u = rng.random()
        if u < dele:
            continue
        q.append(c if u > dele + sub else b"ACGT"[rng.integers(0, 4)])
        while rng.random() < ins:
            q.append(b"ACGT"[rng.integers(0, 4)])
    return bytes(q)


def _flanked(rng, core, lo, hi):
    """core with random flanks of lo..hi bases on both ends."""
    return _rand(rng, rng.integers(lo, hi + 1)) + core + _rand(rng, rng.integers(lo, hi + 1))


# ---------------------------------------------------------------------------------------------- CPU: the twin


def test_twin_equals_full_matrix_local_dp():
    """On pairs the band holds whole (both sides under 25 bases), the band, the prefix-minimum deletion term and the
    clamp after it give what a plain cell-by-cell local DP over the whole matrix gives: strings and ends."""
    rng = np.random.default_rng(31)
    pairs = [(b"", b""), (b"A", b""), (b"", b"ACGT"), (b"A", b"A"), (b"A", b"C"), (b"AAAA", b"CCCC"),
             (b"ACGTACGT", b"A"), (b"G", b"ACGTACGG"), (b"ACGT" * 6, b"ACGT" * 6)]
    while len(pairs) < 300:
        kind = len(pairs) % 4
        if kind == 0:                                           # unrelated
            pairs.append((_rand(rng, rng.integers(0, 25)), _rand(rng, rng.integers(0, 25))))
        elif kind == 1:                                         # mutated
            t = _rand(rng, rng.integers(1, 21))
            pairs.append((_mutate(rng, t, sub=0.1, ins=0.1, dele=0.1)[:24], t))
        elif kind == 2:                                         # a core with flanks on either or both
            core = _rand(rng, rng.integers(4, 13))
            q = _rand(rng, rng.integers(0, 6)) + core + _rand(rng, rng.integers(0, 6))
            t = _rand(rng, rng.integers(0, 6)) + _mutate(rng, core, sub=0.1) + _rand(rng, rng.integers(0, 6))
            pairs.append((q[:24], t[:24]))
        else:                                                   # no base in common
            a = int(rng.integers(0, 4))
            pairs.append((b"ACGT"[a:a + 1] * int(rng.integers(1, 25)), b"ACGT"[(a + 1) % 4:(a + 1) % 4 + 1] * int(rng.integers(1, 25))))
    found = 0
    for q, t in pairs:
        assert twin.align(q, t) == twin.full_matrix(q, t), (q, t)
        found += twin.align(q, t)[2] != (0, 0, 0, 0)
    assert 150 < found < 300


def test_twin_reproduces_the_kat():
    """test/cpp/SimpleAlignerTest.cpp:8-21: the local alignment covers both strings whole (ends 0, 61, 0, 61), so the
    reverse-complemented target string and start == 1267 are the reference's, as for the global aligner."""
    k = _kat()
    q, t = k["qstr"].encode(), k["tstr"].encode()
    qa, ta, ends = twin.align(q, t)
    assert ends == (0, 61, 0, 61)
    start, end, qa2, ta2 = twin.finish(k["start"], k["tlen"], k["strand"].encode(), qa, ta, ends)
    assert ta2.decode() == k["expected_tstr"]
    assert start == k["expected_start"] == 1267
    assert end == k["start"] + 61


def test_finish_arithmetic(oracle_lib):
    """start = tstart + t_begin, end = tstart + t_end; '-': start = tlen - end; start += 1.  By hand with ends that
    leave both ends of t out, and equal to oracle.simple_align's when the ends are the whole of both."""
    qa, ta = b"AC-GT", b"ACTGT"
    # '+': the aligned target bases are t[5:40], the record's target substring starts at tstart = 100
    s, e, q2, t2 = twin.finish(100, 1000, b"+", qa, ta, (3, 7, 5, 40))
    assert (s, e, q2, t2) == (106, 140, qa, ta)
    # '-': the same bases lie at forward positions 1000 - 140 .. 1000 - 105 - 1, 1-based start 861
    s, e, q2, t2 = twin.finish(100, 1000, b"-", qa, ta, (3, 7, 5, 40))
    assert (s, e) == (861, 140)
    assert (q2, t2) == (b"AC-GT", b"ACAGT")
    # never leaves [1, tlen] when tstart + t_len <= tlen: the last target base lands on tlen
    s, e, _, _ = twin.finish(0, 60, b"-", qa, ta, (0, 4, 10, 60))
    assert s == 1 and e == 60
    s, e, _, _ = twin.finish(0, 60, b"+", qa, ta, (0, 4, 10, 60))
    assert s == 11 and s - 1 + 50 == 60
    rng = np.random.default_rng(5)
    for strand in (b"+", b"-"):
        tseq = _rand(rng, 80)
        qseq = _mutate(rng, tseq)
        s0, e0, qa0, ta0 = oracle_lib.simple_align(30, 200, strand, qseq, tseq)
        s1, e1, _, _ = twin.finish(30, 200, strand, qa0, ta0, (0, len(qseq), 0, len(tseq)))
        assert (s1, e1) == (s0, e0)


def test_cli_local_needs_align_and_is_listed():
    """--local without -a is a parse error (exit 2); --help lists it.  Neither needs a device."""
    out = subprocess.run([CLI, "--local", "in.pre"], capture_output=True, timeout=60)
    assert out.returncode == 2 and b"--local" in out.stderr
    out = subprocess.run([CLI, "--help"], capture_output=True, timeout=60)
    assert out.returncode == 0 and b"--local" in out.stdout


# ---------------------------------------------------------------------------------------------- GPU


def _pairs_families(rng):
    k = _kat()
    pairs = [(k["qstr"].encode(), k["tstr"].encode()),
             (b"", b""), (b"A", b""), (b"", b"ACGT"), (b"A", b"A"), (b"A", b"C"), (b"ACGTACGT", b"A"), (b"G", b"ACGTACGG")]
    for i in range(60):
        t = _rand(rng, rng.integers(1, 301))
        q = _mutate(rng, t) if i % 3 else _rand(rng, rng.integers(1, 301))
        pairs.append((q, t))
    for n in (1500, 4000, 9000):
        core = _rand(rng, n)
        pairs.append((_flanked(rng, _mutate(rng, core), 20, 200), _flanked(rng, core, 20, 200)))
        pairs.append((_flanked(rng, _mutate(rng, core), 20, 60), core))
    for n in (20000, 45000, 110000):
        t = _rand(rng, n)
        pairs.append((_mutate(rng, t), t))
    return pairs


@pytest.mark.gpu
def test_device_local_align_equals_twin(gpu_ctx_factory, monkeypatch):
    """dagcon_align on a DAGCON_FLAG_LOCAL_ALIGN context and dagcon_align_ends against the twin, bit for bit: the KAT,
    empty and one-base pairs, short random pairs, flanked pairs of 1.5 to 9 kb, pairs of 20 to 110 kb; again in several
    launch groups; and the static bands alone (every k_align_band instance) against the twin's static-only mode."""
    from pbdagcon_amd import capi
    pairs = _pairs_families(np.random.default_rng(61))
    exp = [twin.align(q, t) for q, t in pairs]
    assert exp[0][2] == (0, 61, 0, 61)
    assert any(e[2][0] > 0 or e[2][2] > 0 for e in exp)          # some local ends leave a flank out
    ctx = gpu_ctx_factory(flags=capi.FLAG_LOCAL_ALIGN)

    def check(expected):
        got = ctx.align(pairs)
        ends = ctx.align_ends()
        bad = [i for i, (g, e, x) in enumerate(zip(got, ends, expected)) if (g[0], g[1], e) != x]
        assert not bad, [(i, len(pairs[i][0]), len(pairs[i][1]), ends[i], expected[i][2]) for i in bad[:5]]
    check(exp)
    monkeypatch.setenv("DAGCON_ALIGN_ROWS", "5000")
    check(exp)
    monkeypatch.delenv("DAGCON_ALIGN_ROWS")
    monkeypatch.setenv("DAGCON_ALIGN_STATIC", "1")
    check([twin.align(q, t, static_only=True) for q, t in pairs])


@pytest.mark.gpu
def test_global_context_align_ends_are_full(gpu_ctx_factory):
    """A context without the flag: its strings are still oracle.banded_align's, and dagcon_align_ends gives the whole
    of both sequences (nothing for a pair the band could not align); a count other than the last call's is refused."""
    import oracle
    from pbdagcon_amd import capi
    rng = np.random.default_rng(62)
    pairs = [(_mutate(rng, t), t) for t in (_rand(rng, n) for n in (5, 120, 2500))]
    t = _rand(rng, 5000)
    pairs.append((t[:3], t))                                     # the band never connects the corners
    ctx = gpu_ctx_factory()
    assert ctx.align(pairs) == [oracle.banded_align(q, t) for q, t in pairs]
    assert ctx.align_ends() == [(0, len(q), 0, len(t)) for q, t in pairs[:3]] + [(0, 0, 0, 0)]
    ctx._align_n = 3
    with pytest.raises(capi.DagconError):
        ctx.align_ends()


@pytest.mark.gpu
def test_local_pair_without_a_match_is_dropped(gpu_ctx_factory):
    from pbdagcon_amd import capi
    ctx = gpu_ctx_factory(flags=capi.FLAG_LOCAL_ALIGN)
    assert ctx.align([(b"AAAA", b"CCCC")]) == [(b"", b"")]
    assert ctx.align_ends() == [(0, 0, 0, 0)]
    assert ctx.align_dropped() == 1


def _flanked_records(rng, n_targets=5, small=3):
    """.pre records with unaligned flanks on the reads and on their target substrings, both strands (tstart in the
    read's frame, m4topre.py:194-206) -> [(tlen, [(tstart, strand, qseq, tseq)])]; target `small` below min_cov."""
    targets = []
    for ti in range(n_targets):
        tlen = int(rng.integers(1500, 2600))
        target = _rand(rng, tlen)
        recs = []
        for r in range(9 if ti != small else 3):
            s = int(rng.integers(0, tlen // 4)); e = int(rng.integers(3 * tlen // 4, tlen + 1))
            strand = b"+-"[(r + ti) % 2:(r + ti) % 2 + 1]
            # the read covers [s + fl, e - fr) of the target and carries flanks of its own
            fl, fr = int(rng.integers(20, 80)), int(rng.integers(20, 80))
            core = target[s + fl:e - fr]
            tseq = target[s:e]
            if strand == b"-":
                core, tseq = core.translate(RC)[::-1], tseq.translate(RC)[::-1]
            qseq = _flanked(rng, _mutate(rng, core), 20, 80)
            tstart = s if strand == b"+" else tlen - e
            recs.append((tstart, strand, qseq, tseq))
        targets.append((tlen, recs))
    return targets


def _expected_pre(oracle, targets, local=True):
    exp = []
    for tlen, recs in targets:
        alns = []
        for tstart, strand, qseq, tseq in recs:
            if local:
                qa, ta, ends = twin.align(qseq, tseq)
                assert ends != (0, 0, 0, 0)
                st, _, qa, ta = twin.finish(tstart, tlen, strand, qa, ta, ends)
            else:
                st, _, qa, ta = oracle.simple_align(tstart, tlen, strand, qseq, tseq)
            alns.append((st, qa, ta))
        exp.append(oracle.consensus_target(tlen, alns, 500, 50, 6) if len(alns) >= 6 else [])
    return exp


@pytest.mark.gpu
def test_consensus_pre_local(gpu_ctx_factory):
    """dagcon_consensus_pre on a local context: twin alignment, the local finish, then oracle.consensus_target; and the
    local ends change the consensus of a flanked target against the global context's."""
    import oracle
    from pbdagcon_amd import capi
    targets = _flanked_records(np.random.default_rng(63))
    exp = _expected_pre(oracle, targets)
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_LOCAL_ALIGN)
    got = ctx.consensus_pre(targets)
    assert got == exp
    assert got[3] == []
    ends = ctx.align_ends()
    assert len(ends) == sum(len(r) for _, r in targets)
    assert [e for e in ends if e[0] > 0 and e[2] > 0]
    glob = gpu_ctx_factory(min_cov=6, min_len=500, trim=50).consensus_pre(targets)
    assert glob == _expected_pre(oracle, targets, local=False)
    assert any(g != x for g, x in zip(glob, got))


@pytest.mark.gpu
def test_cli_pre_local(tmp_path):
    """pbdagcon -a --local -j 2 file.pre equals the same composition on the CPU, byte for byte."""
    import oracle
    targets = _flanked_records(np.random.default_rng(64), n_targets=4, small=2)
    lines = []
    for ti, (tlen, recs) in enumerate(targets):
        for r, (tstart, strand, qseq, tseq) in enumerate(recs):
            lines.append(b" ".join([b"q%d_%d" % (ti, r), b"t%d" % ti, strand, b"%d" % tlen, b"%d" % tstart,
                                    b"%d" % (tstart + len(tseq)), qseq, tseq]))
    exp = []
    for ti, segs in enumerate(_expected_pre(oracle, targets)):
        for r0, r1, s_ in segs:
            exp.append(b">t%d/%d_%d\n%s\n" % (ti, r0, r1, s_))
    path = tmp_path / "in.pre"
    path.write_bytes(b"\n".join(lines) + b"\n")
    out = subprocess.run([CLI, "-a", "--local", "-j", "2", str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout == b"".join(exp) and len(exp) >= 3
