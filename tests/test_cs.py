"""cs input: dagcon_upload_cs / dagcon_consensus_cs (minimap2's cs:Z: text decoded on the device, k_cs.hip.h) and
`pbdagcon --paf --cs --ref`.

What is pinned to what.  cs_twin.decode is the header's rule; consensus_cs equals consensus_cigar (or _windows) on the
twin-decoded batch (segments, status, support, positions, the graph) and the oracle on the strings cigar_twin.expand
makes of it.  `pbdagcon --paf --cs` equals `pbdagcon --sam` in the parser dump and `pbdagcon --paf --reads` in its
output.  The PAF files come from tests/cs_files.py, this suite's own writer: no minimap2 is behind it.  The rule is
this build's own; the reference reads no PAF."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_twin as ct
import cs_files as cf
import cs_twin as cst
import paf_files as pf
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
MIN_COV, MIN_LEN, TRIM = 6, 100, 20


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _run(*args, env=None, stdin=None, timeout=600):
    return subprocess.run([_cli(), *args], capture_output=True, env=env, input=stdin, timeout=timeout)


def _mask(rng, bb, runs=3):
    """bb with a few stretches in lower case (a soft-masked target)."""
    b = bytearray(bb)
    for _ in range(runs):
        a = int(rng.integers(0, max(1, len(b) - 10)))
        n = int(rng.integers(3, 40))
        b[a:a + n] = bytes(b[a:a + n]).lower()
    return bytes(b)


def _twin_targets(seed, n_targets, reads, lo, hi, masked=True, alphabet=b"ACGT"):
    """[(target bases, [(pos, read bases over ACGTN, ops)])]: random pileups compressed to CIGAR records (M and = / X
    in turn), the target then soft-masked in places (the reads stay upper case)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n_targets):
        tl = int(rng.integers(lo, hi))
        alns, bb = random_target(rng, tl, reads, alphabet=alphabet)
        recs = [ct.compress(s, q, t, bb, g % 2 == 1) for s, q, t in alns]
        out.append((_mask(rng, bb) if masked else bb, recs))
    return out


def _cs_records(targets, long_form=False):
    """targets as [(target bases, [(pos, q_len, t_span, cs text)])]."""
    return [(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o, long_form)) for p, q, o in recs]) for bb, recs in targets]


def _decoded(cs_targets):
    """The twin-decoded CIGAR records of conforming cs records: [(target bases, [(pos, q, ops)])]."""
    out = []
    for bb, recs in cs_targets:
        dec = []
        for p, ql, ts, text in recs:
            assert cst.why(text, bb, p, ql, ts) is None, (text, cst.why(text, bb, p, ql, ts))
            ops, q, _ = cst.decode(text, bb, p)
            dec.append((p, q, ops))
        out.append((bb, dec))
    return out


def _strings(targets):
    return batch_from_targets([(len(bb), [ct.expand(p, q, bb, o) for p, q, o in recs], bb) for bb, recs in targets])


# ---- CPU ---------------------------------------------------------------------------------------------------------

def test_library_exports_the_cs_entry_points():
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_upload_cs", "dagcon_consensus_cs"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    # uint32 (+ pad), 3 pointers, uint64, 7 pointers, uint64 on LP64
    assert lib.dagcon_abi_version() == 2 and C.sizeof(capi.CsBatch) == 8 + 3 * 8 + 8 + 7 * 8 + 8 == 104
    src = " ".join(open(os.path.join(ROOT, "include", "dagcon.h")).read().replace(" * ", " ").split())
    assert "typedef struct dagcon_cs_batch" in src and "the reference reads no PAF, parity unpinned" in src
    hb = capi.HostCsBatch.from_records([(b"ACGTACGT", [(1, 3, 3, b":3"), (2, 2, 2, "*ca:1")])])
    assert hb.n_records == 2 and hb.cs_blob.tobytes() == b":3*ca:1" and hb.cs_off.tolist() == [0, 2] and hb.t_span.tolist() == [3, 2]
    assert capi.HostCsBatch.from_records([(b"ACGT", [(1, 1, 1, b":1")])], with_span=False).c_struct().t_span is None
    with pytest.raises(ValueError):
        capi.HostCsBatch(hb.tlen, hb.t_off, hb.t_blob, hb.rec_begin, hb.pos, hb.q_len, hb.cs_off, hb.cs_len, hb.cs_blob, t_span=[1])


@pytest.mark.parametrize("long_form", [False, True])
def test_decode_inverts_encode(long_form):
    """decode(encode(x)) gives back the read and the expansion of cigar_twin.expand, over a few hundred random
    alignments (M and = / X CIGARs, soft-masked targets, reads over ACGTN); the text is lower case but for digits."""
    targets = _twin_targets(5, 8, 40, 60, 500, alphabet=b"ACGTN")
    n = 0
    forms = set()
    for bb, recs in targets:
        for p, q, o in recs:
            text = cst.encode(p, q, bb, o, long_form)
            assert text == text.lower() and not (long_form and b":" in text)
            ops, q2, fl = cst.decode(text, bb, p)
            assert fl == 0 and q2 == q
            assert cst.totals(ops)[1:] == (len(q), pf.tspan(o))
            assert ct.expand(p, q2, bb, ops) == ct.expand(p, q, bb, o)
            assert cst.why(text, bb, p, len(q), pf.tspan(o)) is None
            forms |= {bytes([x]) for x in text if x in cst.OP_BYTES}
            n += 1
    assert n == 320 and forms == ({b"=", b"*", b"+", b"-"} if long_form else {b":", b"*", b"+", b"-"})
    # a soft-masked target base under an upper-case read base is a substitution, and comes back upper case
    assert cst.encode(1, b"AC", b"aC", [ct.op("M", 2)]) == b"*aa:1"
    assert cst.decode(b"*aa:1", b"aC", 1) == ([ct.op("X", 1), ct.op("=", 1)], b"AC", 0)
    assert cst.decode(b":2", b"aC", 1) == ([ct.op("=", 2)], b"aC", 0)
    assert cst.decode(b"=Ac+gT-tt*Nn", b"ACTTG", 1) == ([ct.op("=", 2), ct.op("I", 2), ct.op("D", 2), ct.op("X", 1)], b"ACGTN", 0)
    assert cst.decode(b"", b"ACGT", 2) == ([], b"", 0)


# every way a record can be non-conforming (include/dagcon.h): (text, pos, q_len, t_span or None, what the twin says);
# the target is T_BAD below
T_BAD = b"ACGTTGCAACGTTGCAACGT"
BAD = {
    "tilde": (b":3~ac12ac:2", 1, 5, None, "bad op"),
    "first_byte": (b"3:3", 1, 3, None, "bad op"),
    "first_byte_letter": (b"a+c", 1, 1, None, "bad op"),
    "empty_body": (b":3+*ac", 1, 4, None, "bad body"),
    "empty_body_at_end": (b":3+", 1, 3, None, "bad body"),
    "colon_alone": (b":", 1, 0, None, "bad body"),
    "non_letter": (b":3+a1", 1, 5, None, "bad body"),
    "non_letter_deletion": (b":3-a.", 1, 3, None, "bad body"),
    "non_letter_equal": (b"=ac@", 1, 3, None, "bad body"),
    "non_digit": (b":1a", 1, 1, None, "bad body"),
    "zero": (b":0", 1, 0, None, "bad body"),
    "zeros": (b":3:000", 1, 3, None, "bad body"),
    "two_to_28": (b":268435456", 1, 5, None, "bad body"),
    "ten_digits": (b":0000000003", 1, 3, None, "bad body"),
    "star_one": (b"*a:2", 1, 2, None, "bad body"),
    "star_three": (b"*acg", 1, 1, None, "bad body"),
    "star_digit": (b"*a1", 1, 1, None, "bad body"),
    "q_len_short": (b":3+ac", 1, 4, None, "q_len"),
    "q_len_long": (b":3+ac", 1, 6, None, "q_len"),
    "t_span": (b":3-ac", 1, 3, 4, "t_span"),
    "pos_zero": (b":3", 0, 3, None, "pos is 0"),
    "past_tlen": (b":19*ac:1", 1, 21, None, "past tlen"),
    "past_tlen_pos": (b":3", 19, 3, None, "past tlen"),
    "nine_digits": (b":123456789", 1, 123456789, None, "past tlen"),
    "overflow": (b":268435455" * 17, 1, 5, None, "overflow"),
}
GOOD = {
    "leading_zeros": (b":000000003", 1, 3, 3),
    "upper_ops": (b"=AC*GT+NN-GT", 1, 5, 5),
    "to_the_end": (b":3", 18, 3, 3),
    "empty": (b"", 1, 0, 0),
    "empty_at_the_end": (b"", 21, 0, 0),
}


def test_twin_flags_every_nonconforming_case():
    for name, (text, pos, ql, ts, want) in BAD.items():
        assert cst.why(text, T_BAD, pos, ql, ts) == want, name
    for name, (text, pos, ql, ts) in GOOD.items():
        assert cst.why(text, T_BAD, pos, ql, ts) is None, name
        assert cst.why(text, T_BAD, pos, ql, None) is None, name


def _parser_case(seed=3, long_form=False):
    """Three small targets: both strands, slices inside longer reads, reads shared between lines (a read aligned to two
    targets), the lines shuffled across targets."""
    rng = np.random.default_rng(seed)
    targets = _twin_targets(seed, 3, 5, 60, 200)
    names = ["ctg0", "ctg1|x", "ctg2"]
    reads, alns = pf.from_twin(rng, names, targets, alphabet=b"ACGTN")
    tseqs = {n: bb for n, (bb, _) in zip(names, targets)}
    alns = cf.with_cs(reads, alns, tseqs, long_form)
    assert {x["strand"] for x in alns} == {"+", "-"}
    assert len([q for q in reads if len({x["tname"] for x in alns if x["qname"] == q}) == 2]) == 2
    per = [[x for x in alns if x["tname"] == n] for n in names]
    order = rng.permutation(np.repeat(np.arange(3), [len(p) for p in per])).tolist()
    shuffled = [per[g].pop(0) for g in order]
    return names, targets, tseqs, reads, alns, shuffled


def _write_case(tmp_path, names, targets, tseqs, reads, alns, lines):
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta([n + " some description" for n in names], [t for t, _ in targets], width=50))
    per, flags, qnames = cf.decoded(names, tseqs, alns)
    sam = tmp_path / "in.sam"
    sam.write_bytes(ct.to_sam(names, [len(t) for t, _ in targets], per, flags=flags, qnames=qnames))
    paf = tmp_path / "in.paf"
    paf.write_bytes(cf.paf_text(reads, lines))
    return ref, sam, paf


@pytest.mark.parametrize("long_form", [False, True])
def test_cs_parser_dump_equals_sam_parser_dump(tmp_path, long_form):
    """pbdagcon --paf --cs --dump-parsed prints, byte for byte, what pbdagcon --sam --dump-parsed prints for the same
    alignments written with = / X CIGARs (SEQ the decoded read, no clips): targets in --ref order, a target's lines in
    file order, a file and stdin, -j 3 --batch-targets 1; tp:A:S lines and lines without cs:Z: are skipped and counted."""
    names, targets, tseqs, reads, alns, shuffled = _parser_case(3, long_form)
    lines = [dict(x, cg=False) for x in shuffled]
    lines.insert(2, dict(shuffled[0], tp="S"))
    lines.insert(5, dict(shuffled[1], cs=None))                       # (a cg tag alone is not enough)
    lines.insert(6, dict(shuffled[3], cs=None, cg=False, tname="nowhere"))    # (skipped before it is looked at)
    lines.append(dict(shuffled[2], tp="S", cs=None))
    ref, sam, paf = _write_case(tmp_path, names, targets, tseqs, reads, alns, lines)
    out = _run("--sam", "--ref", str(ref), "--dump-parsed", str(sam), env=NOGPU)
    assert out.returncode == 0, out.stderr.decode()
    want = out.stdout
    assert want.count(b"\n") == len(alns) and b"\t-\t" in want and b"\t+\t" in want and b"=" in want
    for src, stdin in ((str(paf), None), ("-", paf.read_bytes())):
        got = _run("--paf", "--cs", "--ref", str(ref), "--dump-parsed", "-v", src, env=NOGPU, stdin=stdin)
        assert got.returncode == 0, got.stderr.decode()
        assert got.stdout == want, src
        assert re.search(rb"\b2 PAF lines without a cs:Z: tag skipped \(run minimap2 with --cs\)", got.stderr), got.stderr
        assert re.search(rb"\b2 PAF lines skipped \(tp:A:S\)", got.stderr), got.stderr
        assert got.stderr.count(b"without a cs:Z:") == 1 and b"cg:Z:" not in got.stderr
    got = _run("--paf", "--cs", "--ref", str(ref), "--dump-parsed", "-j", "3", "--batch-targets", "1", str(paf), env=NOGPU)
    assert got.returncode == 0 and got.stdout == want


def test_cs_usage_and_input_errors(tmp_path):
    """Every usage error is exit 2 with PARSE ERROR; --paf --reads is what it was; a malformed line is exit 1 with a
    message that names the line; the query name is not looked up."""
    names, targets, tseqs, reads, alns, _ = _parser_case(4)
    ref, sam, paf = _write_case(tmp_path, names, targets, tseqs, reads, alns, alns)
    rd = tmp_path / "reads.fa"
    rd.write_bytes(pf.reads_fasta(reads))
    base = ["--paf", "--cs", "--ref", str(ref)]
    for args in (["--cs", "--ref", str(ref), str(paf)], ["--sam", "--cs", "--ref", str(ref), str(sam)],
                 base + ["--reads", str(rd), str(paf)], base + ["--sam", str(paf)], base + ["--bam", str(paf)],
                 base + ["-a", str(paf)], base + ["-a", "--local", str(paf)], base + ["--polish", "1", str(paf)],
                 ["--paf", "--cs", str(paf)], ["--paf", "--ref", str(ref), str(paf)]):
        out = _run(*args, "--dump-parsed", env=NOGPU)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, (args, out.stderr)
    help_text = _run("--help").stdout
    assert b"--cs" in help_text and b"cs:Z:" in help_text and b"are not read" in help_text
    assert not re.search(rb"cs:Z:,\s+MD:Z:", help_text)
    # every line carries both tags: --paf --reads reads the file as before
    old = _run("--paf", "--ref", str(ref), "--reads", str(rd), "--dump-parsed", str(paf), env=NOGPU)
    assert old.returncode == 0 and old.stdout.count(b"\n") == len(alns) and b"cs:Z:" not in old.stderr

    def dump(text):
        paf.write_bytes(text)
        return _run(*base, "--dump-parsed", str(paf), env=NOGPU)
    good = cf.paf_text(reads, alns).decode().split("\n")[:-1]
    assert dump(("\n".join(good) + "\n").encode()).returncode == 0
    k = 3

    def broken(edit):
        f = good[k].split("\t")
        edit(f)
        return ("\n".join(good[:k] + ["\t".join(f)] + good[k + 1:]) + "\n").encode()

    def setf(i, v):
        return lambda f: f.__setitem__(i, v)
    x = alns[k]
    cases = [
        (lambda f: f.__delitem__(slice(11, None)), rb"line 4: .*12 fields.* 11 fields"),
        (setf(4, "*"), rb"line 4: strand"),
        (setf(2, str(x["qe"])), rb"line 4: query slice"),
        (setf(3, str(len(reads[x["qname"]]) + 1)), rb"line 4: query slice"),
        (setf(2, "x"), rb"line 4: .*not an unsigned"),
        (setf(5, "nowhere"), rb"line 4: target nowhere is not a sequence of --ref"),
        (lambda f: (f.__setitem__(6, str(int(f[6]) + 1))), rb"line 4: target .* has length"),
        (lambda f: (f.__setitem__(8, str(int(f[6]) + 1))), rb"line 4: target range"),
        (setf(0, "nobody"), None),
    ]
    for edit, msg in cases:
        out = dump(broken(edit))
        if msg is None:
            assert out.returncode == 0 and out.stdout.count(b"\n") == len(alns) and b"nobody" in out.stdout
            continue
        assert out.returncode == 1 and out.stdout == b"", (msg, out.stderr)
        assert re.search(msg, out.stderr), (msg, out.stderr)


# ---- GPU ---------------------------------------------------------------------------------------------------------

def _everything(ctx, call):
    segs = call()
    return segs, ctx.target_status.tolist(), ctx.base_support(), ctx.base_positions()


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        assert len(x) == len(y)
        for sx, sy in zip(x, y):
            assert len(sx) == len(sy)
            for ex, ey in zip(sx, sy):
                if isinstance(ex, tuple):
                    assert all(np.array_equal(u, v) for u, v in zip(ex, ey))
                else:
                    assert np.array_equal(ex, ey)


def _batches(cs_targets, with_span=True):
    from pbdagcon_amd import capi
    return (capi.HostCsBatch.from_records(cs_targets, with_span=with_span),
            capi.HostCigarBatch(**ct.records_to_arrays(_decoded(cs_targets))))


def _graphs(cs_b, cg_b, n):
    """The graph addAln leaves for the first n targets, from either batch."""
    from pbdagcon_amd import capi
    ctx = capi.Context(min_cov=0, min_len=0, trim=0, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    try:
        ctx.consensus_cs(cs_b, strict=False)
        a = [ctx.debug_graph(t) for t in range(n)]
        ctx.consensus_cigar(cg_b, strict=False)
        b = [ctx.debug_graph(t) for t in range(n)]
    finally:
        ctx.close()
    return a, b


@pytest.fixture(scope="module")
def pileup():
    """8 targets of 300 to 600 bases, 12 reads each, and what the oracle makes of their expanded strings."""
    targets = _twin_targets(201, 8, 12, 300, 600, alphabet=b"ACGTN")
    exp = oracle_batch(_strings(targets), MIN_COV, MIN_LEN, TRIM)
    assert sum(bool(x) for x in exp) >= 6
    return targets, exp


@pytest.mark.gpu
@pytest.mark.parametrize("long_form", [False, True])
def test_cs_equals_cigar_equals_oracle(pileup, long_form):
    """consensus_cs == consensus_cigar on the twin-decoded batch == the oracle on the expanded strings: segments,
    target_status, base_support(), base_positions(), the counts in the timings and the graph of one target; the short
    and the long form of cs, with and without t_span; the three-step form."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    cs_targets = _cs_records(targets, long_form)
    cs_b, cg_b = _batches(cs_targets)
    assert oracle_batch(_strings(_decoded(cs_targets)), MIN_COV, MIN_LEN, TRIM) == exp
    assert int(cs_b.cs_len.max()) > 64 * 3 and (long_form or cs_b.nbytes < cg_b.nbytes)
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cs(cs_b))
        ta = ctx.timings()
        b = _everything(ctx, lambda: ctx.consensus_cigar(cg_b))
        tb = ctx.timings()
        _same(a, b)
        assert a[0] == exp
        for key in ("consensus_bases", "n_alignments", "n_targets"):
            if key in ta:
                assert ta[key] == tb[key], key
        assert ctx.consensus_cs(_batches(cs_targets, with_span=False)[0]) == exp
        ctx.upload_cs(cs_b); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
    finally:
        ctx.close()
    ga, gb = _graphs(cs_b, cg_b, 1)
    assert ga == gb and len(ga[0]) > 300


def _ops_text(rng, n_ops):
    """cs text of exactly n_ops ops and the read / target bases it consumes."""
    toks = [b":2", b"*ac", b"+g", b"-t", b"=a", b":11", b"+ca", b"-gg"]
    text = b"".join(toks[int(i)] for i in rng.integers(0, len(toks), n_ops))
    ops, _, fl = cst.decode(text, b"A" * 4096, 1)
    assert fl == 0 and len(ops) == n_ops
    return text


def _edge_records(p):
    """The shapes at which the tokeniser can go wrong, each behind a prefix of p bytes of ops (so the construct starts at
    byte p of the record's text, a step being 64 bytes), and the shapes that are about a record's op count on their own.
    (name, text); every record starts at pos 3 of a target of its own."""
    rng = np.random.default_rng(1000 + p)
    pre = cf.prefix(p)
    recs = [
        ("one_op", b":40"),
        ("one_colon", b":%d" % (p * 7)),
        ("ops63", _ops_text(rng, 63)), ("ops64", _ops_text(rng, 64)), ("ops65", _ops_text(rng, 65)), ("ops129", _ops_text(rng, 129)),
        ("plus_first_minus_last", b"+acg:5*ac" + pre + b"-tg"),
        ("empty", b""),
        ("op_start", pre + b"+ac:3"),                                 # p = 63, 64: an op start at byte 63 / 64
        ("digits3", pre + b":123:5"),
        ("digits9", pre + b":000000017*ag"),
        ("digits_end", pre + b":123"),                                # the number ends the text
        ("plus1", pre + b"+g:5"), ("plus64", pre + b"+" + b"acgt" * 16 + b":5"), ("plus200", pre + b"+" + b"gattc" * 40 + b":5"),
        ("equal200", pre + b"=" + b"gattc" * 40 + b":5"),
        ("minus70", pre + b"-" + b"gattcag" * 10 + b"*ca"),
        ("star", pre + b"*ac:5"),                                     # p = 62: * c | a;  p = 63: * | c a
        ("star_end", pre + b"*ag"),
        ("colon_then_star", pre + b":7*ga:5"),
    ]
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("p", [62, 63, 64, 65, 66])
def test_cs_tile_edges(p):
    """Every shape of _edge_records as the only record of a target of its own, the text blob shifted by p bytes of
    other text: consensus_cs equals consensus_cigar on the twin-decoded batch in everything, and the graphs addAln
    leaves are the same vertex by vertex (so the strings are, not merely the consensus).  A 9-digit :n that is inside
    2^28 but past tlen fails its own target only."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(p)
    cs_targets = []
    for name, text in _edge_records(p):
        bb = _mask(rng, bytes(b"ACGT"[i] for i in rng.integers(0, 4, 1300)))
        ops, q, fl = cst.decode(text, bb, 3)
        assert fl == 0, name
        _, nq, nt = cst.totals(ops)
        cs_targets.append((bb, [(3, nq, nt, text)]))
    n = len(cs_targets)
    cs_b, cg_b = _batches(cs_targets)
    assert int((cs_b.cs_len == 0).sum()) == 1 and int(cs_b.q_len[cs_b.cs_len == 0][0]) == 0
    # the blob shifted: p bytes of text that belong to no record in front
    from pbdagcon_amd.capi import HostCsBatch
    shifted = HostCsBatch(cs_b.tlen, cs_b.t_off, cs_b.t_blob, cs_b.rec_begin, cs_b.pos, cs_b.q_len, cs_b.cs_off + np.uint64(p),
                          cs_b.cs_len, b":9~" * 22 + cs_b.cs_blob.tobytes(), cs_b.t_span)
    shifted.cs_blob = np.ascontiguousarray(shifted.cs_blob[66 - p:])
    assert int(shifted.cs_off[0]) == p and shifted.cs_blob.size == cs_b.cs_blob.size + p
    ctx = capi.Context(min_cov=1, min_len=1, trim=0, min_weight=1, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        b = _everything(ctx, lambda: ctx.consensus_cigar(cg_b))
        assert b[1] == [0] * n and sum(bool(s) for s in b[0]) >= n // 2
        for batch in (cs_b, shifted):
            _same(_everything(ctx, lambda: ctx.consensus_cs(batch)), b)
        # a 9-digit number past tlen, straddling a step: its target fails, its neighbours are exact
        bad = list(cs_targets)
        bad[3] = (bad[3][0], [(3, cf.prefix_bases(p) + 123456789, None, cf.prefix(p) + b":123456789")])
        assert cst.why(bad[3][1][0][3], bad[3][0], 3, bad[3][1][0][1]) == "past tlen"
        from pbdagcon_amd.capi import HostCsBatch as H
        got = ctx.consensus_cs(H.from_records(bad, with_span=False), strict=False)
        assert ctx.target_status.tolist() == [0] * 3 + [-4] + [0] * (n - 4)
        assert got == b[0][:3] + [[]] + b[0][4:]
    finally:
        ctx.close()
    ga, gb = _graphs(shifted, cg_b, n)
    assert ga == gb


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BAD) + ["plus_longer_than_q_len", "colon_past_tlen_long"])
def test_cs_nonconforming_record_fails_its_target_only(pileup, case):
    """A target of its own (T_BAD, put in as target 2) holds the non-conforming record among conforming ones: the call
    returns DAGCON_OK, that target alone has DAGCON_ERR_NONCONFORMING and no segments, every other target -- the records
    that follow the bad one in the text and in the read buffer among them -- is exact.  A + body longer than q_len
    writes nothing past the record."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    cs_targets = _cs_records(targets)
    if case == "plus_longer_than_q_len":
        rec = (1, 7, None, b":5+" + b"acgt" * 300 + b":2")
    elif case == "colon_past_tlen_long":
        rec = (11, 5000, None, b":5000")
    else:
        text, pos, ql, ts, _ = BAD[case]
        rec = (pos, ql, ts, text)
    assert cst.why(rec[3], T_BAD, rec[0], rec[1], rec[2]) is not None
    with_span = rec[2] is not None
    good = [(pos, ql, ts, text) for text, pos, ql, ts in GOOD.values()]
    cs_targets.insert(2, (T_BAD, good[:2] + [rec] + good[2:]))
    hb = capi.HostCsBatch.from_records(cs_targets, with_span=with_span)
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cs(hb)
        assert e.value.code == -4
        got = ctx.consensus_cs(hb, strict=False)
        assert ctx.target_status.tolist() == [0, 0, -4] + [0] * (len(exp) - 2)
        assert got == exp[:2] + [[]] + exp[2:]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cs_conforming_corner_records(pileup):
    """The GOOD records (leading zeros, upper-case op bodies, a :n that ends on the target's last base, empty text)
    added to a target: still everything consensus_cigar gives on the decoded batch."""
    from pbdagcon_amd import capi
    targets, _ = pileup
    cs_targets = _cs_records(targets[:2])
    cs_targets.append((T_BAD, [(pos, ql, ts, text) for text, pos, ql, ts in GOOD.values()]))
    cs_b, cg_b = _batches(cs_targets)
    ctx = capi.Context(min_cov=1, min_len=1, trim=0, min_weight=1, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cs(cs_b))
        _same(a, _everything(ctx, lambda: ctx.consensus_cigar(cg_b)))
        assert a[1] == [0, 0, 0]
    finally:
        ctx.close()
    ga, gb = _graphs(cs_b, cg_b, 3)
    assert ga == gb


@pytest.mark.gpu
def test_cs_invalid_arguments(pileup):
    """cs_off + cs_len > cs_bytes, t_off + tlen > t_bytes and a rec_begin that is not monotone are
    DAGCON_ERR_INVALID_ARG for the call; results == NULL too."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    hb = capi.HostCsBatch.from_records(_cs_records(targets))
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)

    def variant(**kw):
        f = dict(tlen=hb.tlen, t_off=hb.t_off, t_blob=hb.t_blob, rec_begin=hb.rec_begin, pos=hb.pos, q_len=hb.q_len,
                 cs_off=hb.cs_off, cs_len=hb.cs_len, cs_blob=hb.cs_blob, t_span=hb.t_span)
        f.update(kw)
        return capi.HostCsBatch(**f)
    try:
        n = hb.n_records
        off, ln, toff, rb = hb.cs_off.copy(), hb.cs_len.copy(), hb.t_off.copy(), hb.rec_begin.copy()
        off[5] = hb.cs_blob.size
        ln[n - 1] += 1
        toff[hb.n_targets - 1] += 1
        rb[2] = rb[3] + 1
        for bad in (variant(cs_off=off), variant(cs_len=ln), variant(t_off=toff), variant(rec_begin=rb),
                    variant(cs_off=hb.cs_off + np.uint64(1 << 40))):
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cs(bad)
            assert e.value.code == -1
        b = hb.c_struct()
        assert ctx.L.dagcon_consensus_cs(ctx.h, C.byref(b), None, None) == -1
        assert ctx.consensus_cs(hb) == exp                            # (the context is as good as new)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cs_windows_equal_cigar_windows_equal_oracle():
    """consensus_cs(batch, windows) == consensus_cigar_windows on the twin-decoded batch == the oracle per window: windows
    of 100 to 150 bases with overlap, records that cross three windows and more; then one record made non-conforming
    (q_len off by one) fails exactly the windows it touches."""
    from pbdagcon_amd import capi
    targets = _twin_targets(211, 4, 12, 400, 600)
    targets = [(bb, sorted(recs, key=lambda r: r[0])) for bb, recs in targets]
    wins = [(g, b, e) for g, (bb, _) in enumerate(targets) for b, e, _, _ in wt.tiled(len(bb), 100 + 5 * g, 15)]
    assert all(e - b <= 150 and (100 <= e - b or e == len(targets[g][0])) for g, b, e in wins)
    hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    cs_targets = _cs_records(targets)
    cs_b, cg_b = _batches(cs_targets)
    dec = _decoded(cs_targets)
    crossing = sum(sum(w[0] == g and w[1] < p - 1 + pf.tspan(o) and p - 1 < w[2] for w in wins) >= 3 for g, (bb, recs) in enumerate(dec) for p, q, o in recs)
    assert crossing > 10
    per = wt.window_targets(dec, wins)
    assert not any(f for _, _, f in per)
    exp = oracle_batch(batch_from_targets([(tl, alns, None) for tl, alns, _ in per]), MIN_COV, 50, 10)
    assert sum(bool(x) for x in exp) > len(wins) // 3
    ctx = capi.Context(min_cov=MIN_COV, min_len=50, trim=10, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cs(cs_b, hw))
        b = _everything(ctx, lambda: ctx.consensus_cigar_windows(cg_b, hw))
        _same(a, b)
        assert a[0] == exp
        ctx.upload_cs(cs_b, hw); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
        # a record that starts inside its target and does not reach its end, one read base too many claimed
        G, k = next((g, i) for g, (bb, recs) in enumerate(cs_targets) for i, (p, ql, ts, t) in enumerate(recs)
                    if p > 120 and p - 1 + ts < len(bb) - 120)
        bb, recs = cs_targets[G]
        p, ql, ts, t = recs[k]
        bad = list(cs_targets)
        bad[G] = (bb, recs[:k] + [(p, ql + 1, ts, t)] + recs[k + 1:])
        touched = [i for i, (g, wb, we) in enumerate(wins) if g == G and wb < p - 1 + ts and p - 1 < we]
        assert 2 <= len(touched) < sum(w[0] == G for w in wins)
        for with_span in (True, False):
            got = ctx.consensus_cs(capi.HostCsBatch.from_records(bad, with_span=with_span), hw, strict=False)
            assert [i for i, s in enumerate(ctx.target_status.tolist()) if s] == touched
            assert all(ctx.target_status[i] == -4 for i in touched)
            assert got == [[] if i in touched else x for i, x in enumerate(exp)]
        # a record whose text breaks the grammar has no decoded span: t_span when given, else the base at pos
        bad[G] = (bb, recs[:k] + [(p, ql, ts, t + b"~")] + recs[k + 1:])
        ctx.consensus_cs(capi.HostCsBatch.from_records(bad), hw, strict=False)
        assert [i for i, s in enumerate(ctx.target_status.tolist()) if s] == touched
        ctx.consensus_cs(capi.HostCsBatch.from_records(bad, with_span=False), hw, strict=False)
        assert [i for i, s in enumerate(ctx.target_status.tolist()) if s] == [i for i, (g, wb, we) in enumerate(wins) if g == G and wb < p and p - 1 < we]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cs_case_of_bodies_and_soft_masked_targets(pileup):
    """Upper-case bodies give what lower-case bodies give (short and long form), and a soft-masked target passes
    through :n verbatim: the graph holds the target's lower-case bytes where the decoded read has them."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    for long_form in (False, True):
        low = _cs_records(targets[:3], long_form)
        up = [(bb, [(p, ql, ts, t.upper()) for p, ql, ts, t in recs]) for bb, recs in low]
        assert up != low
        ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
        try:
            a = _everything(ctx, lambda: ctx.consensus_cs(capi.HostCsBatch.from_records(low)))
            _same(a, _everything(ctx, lambda: ctx.consensus_cs(capi.HostCsBatch.from_records(up))))
            assert a[0] == exp[:3]
        finally:
            ctx.close()
    # text written without regard to case, as an aligner compares bases: :n runs over the target's lower-case stretches
    # (the writer above compares bytes, so there a masked base under an upper-case read base is a *), and the read the
    # device makes has the target's lower-case bytes at those places
    lower = [(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb.upper(), o)) for p, q, o in recs]) for bb, recs in targets[:3]]
    cs_b, cg_b = _batches(lower)
    assert re.search(rb"[acgt]", cg_b.q_blob.tobytes()) and re.search(rb"[acgt]", cg_b.t_blob.tobytes())
    ga, gb = _graphs(cs_b, cg_b, 3)
    assert ga == gb
    up_b = capi.HostCsBatch.from_records([(bb, [(p, ql, ts, t.upper()) for p, ql, ts, t in recs]) for bb, recs in lower])
    assert _graphs(up_b, cg_b, 3)[0] == gb
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        _same(_everything(ctx, lambda: ctx.consensus_cs(cs_b)), _everything(ctx, lambda: ctx.consensus_cigar(cg_b)))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pbdagcon_paf_cs_equals_paf_reads(tmp_path):
    """pbdagcon --paf --cs --ref prints, byte for byte, what pbdagcon --paf --ref --reads prints on the same lines (every
    line carries both tags): FASTA, --fastq, --window 200 with the smallest --overlap the command line takes (--trim + 64: 64 with -t 0; 40 is
    refused as a usage error); both strands, PAF lines
    shuffled across targets, several batches."""
    targets = _twin_targets(221, 6, 10, 300, 600, masked=False)
    names = ["ctg%d|x" % g for g in range(6)]
    rng = np.random.default_rng(15)
    reads, alns = pf.from_twin(rng, names, targets, alphabet=b"ACGTN", sort_pos=True)
    tseqs = {n: bb for n, (bb, _) in zip(names, targets)}
    alns = cf.with_cs(reads, alns, tseqs)
    assert {x["strand"] for x in alns} == {"+", "-"}
    per = [[x for x in alns if x["tname"] == n] for n in names]
    order = rng.permutation(np.repeat(np.arange(6), [len(p) for p in per])).tolist()
    shuffled = [per[g].pop(0) for g in order]
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta(names, [t for t, _ in targets], width=50))
    rd = tmp_path / "reads.fa"
    rd.write_bytes(pf.reads_fasta(reads))
    paf = tmp_path / "in.paf"
    paf.write_bytes(cf.paf_text(reads, shuffled))
    assert paf.read_bytes().count(b"cg:Z:") == paf.read_bytes().count(b"cs:Z:") == len(alns)

    def run(*args):
        out = _run(*args)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout
    old = ["--paf", "--ref", str(ref), "--reads", str(rd), "-m", "100", "-t", "10"]
    new = ["--paf", "--cs", "--ref", str(ref), "-m", "100", "-t", "10"]
    want = run(*old, str(paf))
    assert want.count(b">") >= 5
    assert run(*new, str(paf)) == want
    assert run(*new, "--batch-targets", "2", "--contexts", "2", "-j", "3", str(paf)) == want
    want = run(*old, "--fastq", str(paf))
    assert want.count(b"@ctg") >= 5 and run(*new, "--fastq", str(paf)) == want
    w = ["--window", "200", "--overlap", "64", "-t", "0"]
    want = run(*old, *w, str(paf))
    assert want.count(b">ctg") >= 3
    assert run(*new, *w, str(paf)) == want
    assert run(*new, *w, "--batch-targets", "3", str(paf)) == want
