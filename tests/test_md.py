"""MD input: dagcon_upload_cigar_md / dagcon_consensus_cigar_md / dagcon_fetch_md_targets (SAM / BAM records with an
MD:Z tag and no reference: the targets are rebuilt on the device, k_md.hip.h) and `pbdagcon --sam --md`, `--bam --md`.

What is pinned to what.  md_twin.rebuild is the header's rule; consensus_cigar_md with no target bases equals
consensus_cigar (or _windows, or the packed call) on the same batch with the twin's T, which equals consensus_cigar with
the true backbone and the oracle on the strings cigar_twin.expand makes; md_targets() equals the twin's T byte for byte.
`pbdagcon --sam --md` / `--bam --md` equal `pbdagcon --sam --ref` in the parser dump (plus the text column) and in their
output.  The files come from tests/md_files.py, this suite's own writer.  The rule is this build's own; the reference
reads no SAM."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_twin as ct
import md_files as mf
import md_twin as mt
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
MIN_COV, MIN_LEN, TRIM = 6, 100, 20
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _pileups(seed, n_targets, reads, lo, hi, alphabet=b"ACGTN"):
    """[(target bases, [(pos, read bases, ops)])]: random pileups compressed to CIGAR records, M and = / X in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n_targets):
        alns, bb = random_target(rng, int(rng.integers(lo, hi)), reads, alphabet=alphabet)
        out.append((bb, [ct.compress(s, q, t, bb, g % 2 == 1) for s, q, t in alns]))
    return out


def _texts(targets):
    return [[mt.encode(p, q, bb, o) for p, q, o in recs] for bb, recs in targets]


def _twin_T(targets, texts):
    return mt.rebuild([(len(bb), recs) for bb, recs in targets], texts)


def _strings(targets):
    return batch_from_targets([(len(bb), [ct.expand(p, q, bb, o) for p, q, o in recs], bb) for bb, recs in targets])


def _cigar_batch(targets, tseqs="own", packed=False):
    """The HostCigarBatch of the records; tseqs: "own" (the targets' bases), None (no target bases: the MD calls), or
    one bytes per target."""
    from pbdagcon_amd import capi
    arr = ct.records_to_arrays(targets)
    if tseqs is None:
        arr["t_blob"] = None
    elif tseqs != "own":
        assert [len(t) for t in tseqs] == [len(bb) for bb, _ in targets]
        arr["t_blob"] = np.frombuffer(b"".join(tseqs), np.uint8)
    hb = capi.HostCigarBatch(**arr)
    return hb.packed() if packed else hb


def _md_tags(texts):
    from pbdagcon_amd import capi
    return capi.HostMdTags.from_texts([t for per in texts for t in per])


# ---- CPU ---------------------------------------------------------------------------------------------------------

def test_library_exports_the_md_entry_points():
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_upload_cigar_md", "dagcon_consensus_cigar_md", "dagcon_fetch_md_targets"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    # 3 pointers and a uint64 on LP64
    assert lib.dagcon_abi_version() == 2 and C.sizeof(capi.MdTags) == 32
    src = " ".join(open(os.path.join(ROOT, "include", "dagcon.h")).read().replace(" * ", " ").split())
    assert "typedef struct dagcon_md_tags" in src and "the reference reads no SAM, parity unpinned" in src
    assert "[0-9]+(([A-Za-z]|\\^[A-Za-z]+)[0-9]+)*" in src and "its target's MD tags disagree" in src
    md = capi.HostMdTags.from_texts([b"5A3", "10", b""])
    assert md.n_records == 3 and md.md_blob.tobytes() == b"5A310" and md.md_off.tolist() == [0, 3, 5] and md.md_len.tolist() == [3, 2, 0]
    hb = capi.HostCigarBatch.from_records([(b"ACGTACGT", [(1, b"ACG", [("M", 3)])]), (b"ACG", [])])
    nb = capi.HostCigarBatch(hb.tlen, hb.t_off, None, hb.rec_begin, hb.pos, hb.q_off, hb.q_len, hb.q_blob, hb.op_begin, hb.ops)
    assert nb.c_struct().t_blob is None and nb.c_struct().t_bytes == 11 == hb.c_struct().t_bytes
    assert nb.packed().t_blob is None and nb.nbytes == hb.nbytes - 11
    for name in ("upload_cigar_md", "consensus_cigar_md", "md_targets"):
        assert callable(getattr(capi.Context, name))


@pytest.mark.parametrize("alphabet", [b"ACGT", b"ACGTN"])
def test_rebuild_inverts_encode(alphabet):
    """Over 40 seeds: the target rebuilt from CIGAR, SEQ and the encoded MD equals the backbone on every covered
    position and is N elsewhere, there is no conflict, and cigar_twin.expand gives the same pair of strings for every
    record with either target; M and = / X CIGARs."""
    covered_n = uncovered_n = 0
    for seed in range(40):
        targets = _pileups(seed, 2, 6, 150, 300, alphabet)
        texts = _texts(targets)
        T, conflict = _twin_T(targets, texts)
        assert conflict == [False, False]
        for (bb, recs), t, per in zip(targets, T, texts):
            cov = np.zeros(len(bb), bool)
            for (p, q, o), text in zip(recs, per):
                assert mt.why(text, p, len(q), len(bb), o) is None
                cov[p - 1:p - 1 + mt.events(text)[0]] = True
                assert ct.expand(p, q, t, o) == ct.expand(p, q, bb, o)
            ta, ba = np.frombuffer(t, np.uint8), np.frombuffer(bb, np.uint8)
            assert np.array_equal(ta[cov], ba[cov]) and (ta[~cov] == ord("N")).all()
            covered_n += int(cov.sum()); uncovered_n += int((~cov).sum())
    assert covered_n > 10000 and uncovered_n > 500


def test_encode_and_events_by_hand():
    #      0123456789
    bb = b"ACGTACGTAC"
    assert mt.encode(1, b"ACGTACGTAC", bb, [ct.op("M", 10)]) == b"10"
    assert mt.encode(2, b"CGAAC", bb, [ct.op("M", 2), ct.op("X", 1), ct.op("=", 2)]) == b"2T2"
    assert mt.encode(1, b"ACTT", bb, [ct.op("M", 2), ct.op("D", 2), ct.op("M", 2)]) == b"2^GT0A0C0"
    assert mt.encode(3, b"ttGTA", bb, [ct.op("S", 2), ct.op("M", 1), ct.op("I", 1), ct.op("M", 1)]) == b"1T0"
    assert mt.events(b"2^GT0A0C0") == (6, [(2, ord("G")), (3, ord("T")), (4, ord("A")), (5, ord("C"))])
    assert mt.events(b"3^AC0G2") == (8, [(3, ord("A")), (4, ord("C")), (5, ord("G"))])
    assert mt.events(b"000000017") == (17, []) and mt.events(b"0") == (0, []) and mt.events(b"1a0C1") == (4, [(1, ord("a")), (2, ord("C"))])


# every way a text can break the grammar (include/dagcon.h), and texts that do not
BAD_TEXT = {
    "empty": b"", "first_letter": b"A5", "first_caret": b"^A5", "caret_digit": b"5^3", "caret_end": b"5^", "two_letters": b"5AC3",
    "ends_letter": b"5A", "ends_deletion": b"5^AC", "other_byte": b"5*3", "blank": b"5 3", "ten_digits": b"0000000005",
    "two_to_28": b"268435456", "two_carets": b"5^^A3", "caret_after_letter": b"5A^C3", "minus": b"-5", "newline": b"8\n",
}
GOOD_TEXT = {"leading_zeros": b"000000008", "deletion_then_mismatch": b"2^AC0G3", "lower": b"3a4", "mismatches": b"0A0C0G0T4",
             "just_below": b"268435455"}


def _bad_records():
    """(name, pos, q, ops, text, what the twin says) against a target of 20 bases; each CIGAR consumes 8 target bases
    unless the case is about the CIGAR."""
    m8, q8 = [ct.op("M", 8)], b"ACGTACGT"
    out = [(name, 3, q8, m8, text, "grammar") for name, text in sorted(BAD_TEXT.items())]
    out += [("one_more", 3, q8, m8, b"9", "covered"), ("one_fewer", 3, q8, m8, b"3A3", "covered"),
            ("deletion_uncounted", 3, q8, [ct.op("M", 4), ct.op("D", 2), ct.op("M", 4)], b"8", "covered"),
            ("pos_zero", 0, q8, m8, b"8", "cigar"), ("past_tlen", 14, q8, m8, b"8", "cigar"),
            ("q_len", 3, q8 + b"A", m8, b"8", "cigar")]
    return out


def test_twin_flags_every_nonconforming_case_and_both_conflicts():
    for name, pos, q, ops, text, want in _bad_records():
        assert mt.why(text, pos, len(q), 20, ops) == want, name
    for name, text in GOOD_TEXT.items():
        ev = mt.events(text)
        assert ev is not None, name
        assert name == "just_below" or mt.why(text, 3, ev[0], 20, [ct.op("M", ev[0])]) is None, name
    m20 = [ct.op("M", 20)]
    a = b"ACGTAGGTACGTACGTACGT"
    # two records spell different letters at position 5; the read bases there do not matter
    T, c = mt.rebuild([(30, [(1, a, m20), (1, a, m20)])], [[b"5A14", b"5C14"]])
    assert c == [True]
    # two records match with different read bases at position 7, which nobody spells
    T, c = mt.rebuild([(30, [(1, a, m20), (1, a[:7] + b"A" + a[8:], m20)])], [[b"20", b"20"]])
    assert c == [True]
    # G under a match where another record spells T: no conflict, the letter wins
    T, c = mt.rebuild([(30, [(1, a, m20), (1, a[:5] + b"A" + a[6:], m20)])], [[b"20", b"5T14"]])
    assert c == [False] and T[0] == a[:5] + b"T" + a[6:] + b"N" * 10
    # a non-conforming record contributes nothing
    T, c = mt.rebuild([(30, [(1, a, m20), (1, b"T" * 20, m20)])], [[b"20", b"21"]])
    assert c == [False] and T[0] == a + b"N" * 10


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _run(*args, env=None, stdin=None, timeout=600):
    return subprocess.run([_cli(), *args], capture_output=True, env=env, input=stdin, timeout=timeout)


def _files(tmp_path, targets, names=None, drop=(), upper=True):
    """ref.fa, in.sam (no tags: for --ref), md.sam and md.bam (tags; the records whose flat index is in drop without)."""
    names = names or ["ctg%d|x" % g for g in range(len(targets))]
    tlens = [len(bb) for bb, _ in targets]
    texts = _texts(targets)
    flat = [t for per in texts for t in per]
    flat = [None if i in drop else t for i, t in enumerate(flat)]
    it = iter(flat)
    recs = mf.records(names, targets, [[next(it) for _ in per] for per in texts])
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta([n + " some description" for n in names], [bb for bb, _ in targets], width=50))
    sam = tmp_path / "in.sam"
    sam.write_bytes(ct.to_sam(names, tlens, [r for _, r in targets], qnames=[r["qname"] for r in recs]))
    mds = tmp_path / "md.sam"
    mds.write_bytes(mf.sam_text(names, tlens, recs))
    mdb = tmp_path / "md.bam"
    mdb.write_bytes(mf.bam_file(names, tlens, recs))
    return ref, sam, mds, mdb, flat


def test_md_parser_dump_equals_ref_parser_dump_plus_the_text(tmp_path):
    """pbdagcon --sam --md --dump-parsed and --bam --md --dump-parsed print, line for line, what --sam --ref --dump-parsed
    prints plus the MD text as one more column: a file and stdin, -j 3 --batch-targets 1.  Records without the tag are
    skipped and counted in one line on stderr."""
    targets = _pileups(3, 3, 5, 60, 200)
    ref, sam, mds, mdb, flat = _files(tmp_path, targets)
    out = _run("--sam", "--ref", str(ref), "--dump-parsed", str(sam), env=NOGPU)
    assert out.returncode == 0, out.stderr.decode()
    want = b"".join(line + b"\t" + t + b"\n" for line, t in zip(out.stdout.split(b"\n"), flat))
    assert want.count(b"\n") == 15
    for flag, path in (("--sam", mds), ("--bam", mdb)):
        for src, stdin in ((str(path), None), ("-", path.read_bytes())):
            got = _run(flag, "--md", "--dump-parsed", "-v", src, env=NOGPU, stdin=stdin)
            assert got.returncode == 0, got.stderr.decode()
            assert got.stdout == want, (flag, src)
            assert b"MD:Z:" not in got.stderr
        got = _run(flag, "--md", "--dump-parsed", "-j", "3", "--batch-targets", "1", str(path), env=NOGPU)
        assert got.returncode == 0 and got.stdout == want
    # records 2 and 7 carry no tag
    ref, sam, mds, mdb, flat = _files(tmp_path, targets, drop=(2, 7))
    lines = want.split(b"\n")[:-1]
    kept = b"".join(l + b"\n" for i, l in enumerate(lines) if i not in (2, 7))
    for flag, path, what in (("--sam", mds, b"SAM"), ("--bam", mdb, b"BAM")):
        got = _run(flag, "--md", "--dump-parsed", str(path), env=NOGPU)
        assert got.returncode == 0 and got.stdout == kept, flag
        assert re.search(rb"\b2 " + what + rb" records without an MD:Z: tag skipped", got.stderr), got.stderr
        assert got.stderr.count(b"without an MD:Z:") == 1


def test_md_usage_and_input_errors(tmp_path):
    """Every usage error is exit 2 with PARSE ERROR, said without a device; --sam / --bam without --ref and without --md
    say what they said; an RNAME without an @SQ line is exit 1 and names the line; --help states the rule."""
    targets = [(bb, sorted(recs, key=lambda r: r[0])) for bb, recs in _pileups(4, 2, 4, 60, 120)]
    ref, sam, mds, mdb, _ = _files(tmp_path, targets)
    for args in (["--md", str(mds)], ["--sam", "--md", "--ref", str(ref), str(mds)], ["--bam", "--md", "--ref", str(ref), str(mdb)],
                 ["--paf", "--md", "--ref", str(ref), str(mds)], ["--paf", "--cs", "--md", "--ref", str(ref), str(mds)],
                 ["--sam", "--md", "-a", str(mds)], ["--sam", "--md", "-a", "--local", str(mds)], ["--bam", "--md", "--polish", "1", str(mdb)],
                 ["--sam", "--bam", "--md", str(mds)], ["-a", "--md", str(mds)]):
        out = _run(*args, "--dump-parsed", env=NOGPU)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, (args, out.stderr)
    for flag, path in (("--sam", mds), ("--bam", mdb)):
        out = _run(flag, str(path), "--dump-parsed", env=NOGPU)
        assert out.returncode == 2 and ("PARSE ERROR: %s needs --ref <fasta>" % flag).encode() in out.stderr
    help_text = _run("--help").stdout
    assert b"--md" in help_text and b"MD:Z:" in help_text and b"are not read" in help_text and b"parity unpinned" in help_text
    assert b"[0-9]+(([A-Za-z]|^[A-Za-z]+)[0-9]+)*" in help_text and not re.search(rb"cs:Z:,\s+MD:Z:", help_text)
    # the header loses the @SQ line of the second target: its first record is line 5 of the file now
    text = mds.read_bytes().split(b"\n")
    assert text[2].startswith(b"@SQ\tSN:ctg1|x")
    n0 = len(targets[0][1])
    (tmp_path / "nosq.sam").write_bytes(b"\n".join(text[:2] + text[3:]))
    out = _run("--sam", "--md", "--dump-parsed", str(tmp_path / "nosq.sam"), env=NOGPU)
    assert out.returncode == 1 and re.search(rb"line %d: RNAME has no @SQ line" % (3 + n0 + 1), out.stderr), out.stderr
    out = _run("--sam", "--md", "--window", "100", "--overlap", "120", str(tmp_path / "nosq.sam"), env=NOGPU)
    assert out.returncode == 1 and re.search(rb"line %d: RNAME ctg1\|x has no @SQ line" % (3 + n0 + 1), out.stderr), out.stderr
    (tmp_path / "badsq.sam").write_bytes(b"@SQ\tSN:x\tLN:12a\n")
    out = _run("--sam", "--md", "--dump-parsed", str(tmp_path / "badsq.sam"), env=NOGPU)
    assert out.returncode == 1 and b"line 1: an @SQ line needs SN and a numeric LN" in out.stderr



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


def _graphs(calls, n):
    """The graph addAln leaves for the first n targets after each call (a function of the context)."""
    from pbdagcon_amd import capi
    ctx = capi.Context(min_cov=0, min_len=0, trim=0, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    try:
        out = []
        for call in calls:
            call(ctx)
            out.append([ctx.debug_graph(t) for t in range(n)])
    finally:
        ctx.close()
    return out


def _full_ctx(**kw):
    from pbdagcon_amd import capi
    return capi.Context(flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS, **kw)


@pytest.fixture(scope="module")
def pileup():
    """8 targets of 300 to 600 bases, 12 reads each over ACGTN, their MD texts, the twin's T, and what the oracle makes
    of the expanded strings."""
    targets = _pileups(301, 8, 12, 300, 600)
    texts = _texts(targets)
    T, conflict = _twin_T(targets, texts)
    assert not any(conflict) and any(b"N" in t for t in T)
    exp = oracle_batch(_strings(targets), MIN_COV, MIN_LEN, TRIM)
    assert sum(bool(x) for x in exp) >= 6
    return targets, texts, T, exp


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_md_equals_cigar_on_the_twin_target_equals_oracle(pileup, packed):
    """consensus_cigar_md without target bases == consensus_cigar with the twin's T == consensus_cigar with the true
    backbone == the oracle: segments, target_status, base_support(), base_positions(), the counts in the timings and the
    graph of one target; md_targets() is the twin's T; the three-step form."""
    targets, texts, T, exp = pileup
    md = _md_tags(texts)
    md_b = _cigar_batch(targets, None, packed)
    twin_b, true_b = _cigar_batch(targets, T, packed), _cigar_batch(targets, "own", packed)
    assert md_b.is_packed == packed and md_b.t_blob is None and int(md.md_len.max()) > 64 * 2
    assert T != [bb for bb, _ in targets]
    ctx = _full_ctx(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cigar_md(md_b, md))
        ta = ctx.timings()
        assert ctx.md_targets().tobytes() == b"".join(T)
        b = _everything(ctx, lambda: ctx.consensus_cigar(twin_b))
        tb = ctx.timings()
        c = _everything(ctx, lambda: ctx.consensus_cigar(true_b))
        _same(a, b)
        _same(a, c)
        assert a[0] == exp
        for key in ("consensus_bases", "n_alignments", "n_columns", "n_nodes"):
            if key in ta:
                assert ta[key] == tb[key], key
        ctx.upload_cigar_md(md_b, md); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
        assert ctx.md_targets().tobytes() == b"".join(T)
    finally:
        ctx.close()
    ga, gb = _graphs([lambda x: x.consensus_cigar_md(md_b, md, strict=False), lambda x: x.consensus_cigar(twin_b, strict=False)], 1)
    assert ga == gb and len(ga[0]) > 300


def _record_from_md(rng, text, front=b""):
    """A record the text describes: target bases (random; the text's letters where it has them), the read (the target
    under a match, another base under a mismatch, nothing under a deletion), M and D ops.  front: ops in front of it
    that consume no target base, with their read bases."""
    cov, letters = mt.events(text)
    bb = ACGT[rng.integers(0, 4, cov)].copy()
    kind = np.zeros(cov, np.uint8)                                   # 0 match, 1 mismatch, 2 deleted
    k = 0
    for tok in mt.TOKEN.findall(text):
        if tok[:1].isdigit():
            k += int(tok)
        else:
            body = tok.lstrip(b"^")
            bb[k:k + len(body)] = np.frombuffer(body, np.uint8)
            kind[k:k + len(body)] = 2 if tok[:1] == b"^" else 1
            k += len(body)
    q = bb.copy()
    mm = kind == 1
    q[mm] = np.where((bb[mm] & 0xDF) == ord("G"), ord("C"), ord("G"))
    ops, i = [], 0
    while i < cov:
        j = i
        while j < cov and (kind[j] == 2) == (kind[i] == 2):
            j += 1
        ops.append(ct.op("D" if kind[i] == 2 else "M", j - i))
        i = j
    return bb.tobytes(), q[kind != 2].tobytes(), ops


def _record_from_ops(rng, spec):
    """spec = [(op char, length)]: target bases, a read with a mismatch in every M / X op longer than 2, and the ops."""
    bb, q, ops = bytearray(), bytearray(), []
    for ch, ln in spec:
        seg = ACGT[rng.integers(0, 4, ln)].tobytes()
        if ch in "M=X":
            r = bytearray(seg)
            if ch == "X" or (ch == "M" and ln > 2):
                r[ln // 2] = ord("C") if seg[ln // 2] == ord("G") else ord("G")
            bb += seg; q += r
        elif ch == "D":
            bb += seg
        elif ch in "IS":
            q += seg
        ops.append(ct.op(ch, ln))
    return bytes(bb), bytes(q), ops


def _prefix(p):
    """p bytes of valid MD tokens that end with a letter (what follows begins with a number)."""
    return (b"12C" if p % 2 else b"") + b"2A" * ((p - 3 * (p % 2)) // 2)


def _groups(rng, n):
    """A text of n letter groups (mismatches and deletions) between n + 1 numbers."""
    toks = [b"A", b"c", b"^G", b"^TA", b"N"]
    nums = [b"0", b"1", b"3", b"12"]
    return b"".join(nums[int(rng.integers(0, 4))] + toks[int(rng.integers(0, 5))] for _ in range(n)) + b"2"


def _edge_records(p):
    """(name, target bases the record covers, read, ops, text): the shapes at which the tokeniser and the fill can go
    wrong, the text shapes behind p bytes of tokens (a step is 64 bytes)."""
    rng = np.random.default_rng(2000 + p)
    pre = _prefix(p)
    assert len(pre) == p and mt.events(pre + b"1") is not None
    texts = [
        ("digits3", pre + b"123T5"),                                  # p = 62, 63: the number straddles the step
        ("digits9", pre + b"000000017G4"),
        ("a0c", pre + b"4A0C3"),
        ("lone_zero", b"0"),
        ("one_number", b"40"),
        ("one_number_long", b"%d" % (100 + p)),
        ("caret", pre + b"5^ACG7"),                                   # p = 62: ^ at byte 63, its letters in the next step
        ("caret_after_zero", pre + b"0^TTG1"), ("caret_after_two_digits", pre + b"12^AC3"),
        ("del1", pre + b"3^A3"), ("del64", pre + b"3^" + b"ACGT" * 16 + b"3"), ("del70", pre + b"3^" + b"GATTCAG" * 10 + b"0C2"),
        ("del200", pre + b"3^" + b"GATTC" * 40 + b"5"),
        ("del_then_mismatch", pre + b"3^AC0G3"),
        ("digits_end", pre + b"123"),
        ("groups63", _groups(rng, 63)), ("groups64", _groups(rng, 64)), ("groups65", _groups(rng, 65)), ("groups129", _groups(rng, 129)),
        ("lower", pre + b"3a0^cg2"),
    ]
    out = []
    for name, text in texts:
        assert mt.events(text) is not None, name
        bb, q, ops = _record_from_md(rng, text)
        out.append((name, bb, q, ops, text))
    alt = [("M", 2), ("I", 1), ("M", 3), ("D", 1)]
    specs = [("ops%d" % n, [alt[i % 4] for i in range(n - 1)] + [("M", 4)]) for n in (63, 64, 65, 129)]
    specs += [("m%d" % n, [("M", n)]) for n in (64, 65, 200)]
    specs += [("clip_odd", [("S", 3), ("M", 50), ("I", 2), ("=", 30), ("X", 1), ("D", 3), ("M", 31), ("S", 1)]),
              ("clip_even", [("S", 2), ("M", 77)])]
    for name, spec in specs:
        bb, q, ops = _record_from_ops(rng, spec)
        out.append((name, bb, q, ops, mt.encode(1, q, bb, ops)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("p", [62, 63, 64, 65, 66])
def test_md_step_and_tile_edges(p):
    """Every shape of _edge_records as the only record of a target of its own, at pos 4 behind three bases nobody
    covers, unpacked and packed, and again with the text blob shifted by p bytes: consensus_cigar_md equals
    consensus_cigar on the twin's T in everything, md_targets() is the twin's T, and the graphs addAln leaves are the
    same vertex by vertex."""
    from pbdagcon_amd import capi
    targets, texts = [], []
    for name, bb, q, ops, text in _edge_records(p):
        full = b"GAT" + bb + b"TC"
        assert mt.why(text, 4, len(q), len(full), ops) is None, name
        targets.append((full, [(4, q, ops)]))
        texts.append([text])
    n = len(targets)
    T, conflict = _twin_T(targets, texts)
    assert not any(conflict)
    assert all(t == b"NNN" + bb[3:-2] + b"NN" for t, (bb, _) in zip(T, targets))
    md = _md_tags(texts)
    shifted = capi.HostMdTags(md.md_off + np.uint64(p), md.md_len, (b"9^*" * 22)[66 - p:] + md.md_blob.tobytes())
    assert int(shifted.md_off[0]) == p and shifted.md_blob.size == md.md_blob.size + p
    ctx = _full_ctx(min_cov=1, min_len=1, trim=0, min_weight=1)
    try:
        for packed in (False, True):
            md_b, twin_b = _cigar_batch(targets, None, packed), _cigar_batch(targets, T, packed)
            b = _everything(ctx, lambda: ctx.consensus_cigar(twin_b))
            assert b[1] == [0] * n and sum(bool(s) for s in b[0]) >= n // 2
            for tags in (md, shifted):
                _same(_everything(ctx, lambda: ctx.consensus_cigar_md(md_b, tags)), b)
                assert ctx.md_targets().tobytes() == b"".join(T)
    finally:
        ctx.close()
    md_b, twin_b = _cigar_batch(targets, None, True), _cigar_batch(targets, T, True)
    ga, gb = _graphs([lambda x: x.consensus_cigar_md(md_b, shifted, strict=False), lambda x: x.consensus_cigar(twin_b, strict=False)], n)
    assert ga == gb


@pytest.mark.gpu
def test_md_nonconforming_record_fails_its_target_only(pileup):
    """A target of its own (20 bases, put in as target 2) holds the non-conforming record among conforming ones: the call
    returns DAGCON_OK, that target alone has DAGCON_ERR_NONCONFORMING and no segments, every other target is exact, and
    md_targets() holds what the conforming records of the batch give.  Every grammar case, covered one more and one
    fewer, pos == 0, a record past tlen; then the texts that are fine."""
    from pbdagcon_amd import capi
    targets, texts, T, exp = pileup
    bb = b"ACGTACGTACGTACGTACGT"
    good = [(3, bb[2:10], [ct.op("M", 8)])] * 2
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        for name, pos, q, ops, text, _ in _bad_records():
            tg = targets[:2] + [(bb, good[:1] + [(pos, q, ops)] + good[1:])] + targets[2:]
            tx = texts[:2] + [[b"8", text, b"8"]] + texts[2:]
            t_bad, c_bad = _twin_T(tg[2:3], tx[2:3])
            assert c_bad == [False] and t_bad == [b"NN" + bb[2:10] + b"N" * 10]
            hb, md = _cigar_batch(tg, None), _md_tags(tx)
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cigar_md(hb, md)
            assert e.value.code == -4, name
            got = ctx.consensus_cigar_md(hb, md, strict=False)
            assert ctx.target_status.tolist() == [0, 0, -4] + [0] * (len(exp) - 2), name
            assert got == exp[:2] + [[]] + exp[2:], name
            assert ctx.md_targets().tobytes() == b"".join(T[:2] + t_bad + T[2:]), name
        for name, text in GOOD_TEXT.items():
            if name == "just_below":
                continue
            bbg, q, ops = _record_from_md(np.random.default_rng(1), text)
            tg = targets[:2] + [(bbg, [(1, q, ops)])] + targets[2:]
            got = ctx.consensus_cigar_md(_cigar_batch(tg, None), _md_tags(texts[:2] + [[text]] + texts[2:]))
            assert got == exp[:2] + [[]] + exp[2:], name
            assert ctx.md_targets().tobytes() == b"".join(T[:2] + [bbg] + T[2:]), name
    finally:
        ctx.close()


def _conflict_case(kind):
    """A target of 1,300 bases with three records: two at [0, 20) that disagree (kind "letters": they spell A and C at
    position 5; "bases": both match, with G and A at position 7; "letter_wins": G under a match where the other spells
    T, which is no conflict) and one at [700, 760) that has nothing to do with it."""
    rng = np.random.default_rng(9)
    a = b"ACGTAGGTACGTACGTACGT"
    far = ACGT[rng.integers(0, 4, 60)].tobytes()
    m20 = [ct.op("M", 20)]
    second, tx = {"letters": (a, [b"5A14", b"5C14"]), "bases": (a[:7] + b"A" + a[8:], [b"20", b"20"]),
                  "letter_wins": (a[:5] + b"A" + a[6:], [b"20", b"5T14"])}[kind]
    recs = [(1, a, m20), (1, second, m20), (701, far, [ct.op("M", 60)])]
    return (b"N" * 1300, recs), tx + [b"60"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["letters", "bases"])
def test_md_conflict_fails_its_target(pileup, kind):
    """Two records of a target disagree: that target gets DAGCON_ERR_NONCONFORMING; with windows, the windows its
    records meet (the record far from the disagreement too: every record of the target is non-conforming); another
    target in the batch is exact; record_stats has the fate NONCONFORMING for its records."""
    from pbdagcon_amd import capi
    targets, texts, T, _ = pileup
    tg, tx = _conflict_case(kind)
    assert _twin_T([tg], [tx])[1] == [True]
    batch = [targets[0], tg, targets[1]]
    btx = [texts[0], tx, texts[1]]
    hb, md = _cigar_batch(batch, None), _md_tags(btx)
    ctx = _full_ctx(min_cov=1, min_len=1, trim=0, min_weight=1)
    try:
        ctx.set_record_filter()
        want = _everything(ctx, lambda: ctx.consensus_cigar(_cigar_batch([targets[0], targets[1]], T[:2])))
        got = _everything(ctx, lambda: ctx.consensus_cigar_md(hb, md, strict=False))
        assert got[1] == [0, -4, 0] and got[0][1] == []
        _same((got[0][::2], got[1][::2], got[2][::2], got[3][::2]), want)
        st = ctx.record_stats()
        n0 = len(targets[0][1])
        assert st["fate"][n0:n0 + 3].tolist() == [capi.FATE_NONCONFORMING] * 3 and not st["fate"][:n0].any() and not st["fate"][n0 + 3:].any()
        assert not st["match"][n0:n0 + 3].any()
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar_md(hb, md)
        assert e.value.code == -4 and "MD tags disagree" in str(e.value)
        # windows of 500: [0, 500) and [500, 1000) hold records of the target, [1000, 1300) holds none
        wins = [(g, b, e) for g, (bb, _) in enumerate(batch) for b, e, _, _ in wt.tiled(len(bb), 500, 0)]
        hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        first = next(i for i, w in enumerate(wins) if w[0] == 1)
        ctx.consensus_cigar_md(hb, md, hw, strict=False)
        assert ctx.target_status.tolist() == [-4 if i in (first, first + 1) else 0 for i in range(len(wins))]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_md_letter_wins_over_a_match(pileup):
    """G under a match of one record where another record spells T: no failure, md_targets() has T there, and the
    result is consensus_cigar's on the twin's T."""
    targets, texts, T, _ = pileup
    tg, tx = _conflict_case("letter_wins")
    (t1,), (c1,) = _twin_T([tg], [tx])
    assert not c1 and t1[5:6] == b"T" and t1[4:5] == b"A" and t1[20:700] == b"N" * 680
    batch, btx = [targets[0], tg, targets[1]], [texts[0], tx, texts[1]]
    ctx = _full_ctx(min_cov=1, min_len=1, trim=0, min_weight=1)
    try:
        got = _everything(ctx, lambda: ctx.consensus_cigar_md(_cigar_batch(batch, None), _md_tags(btx)))
        assert got[1] == [0, 0, 0] and got[0][1]
        assert ctx.md_targets().tobytes() == T[0] + t1 + T[1]
        _same(got, _everything(ctx, lambda: ctx.consensus_cigar(_cigar_batch(batch, [T[0], t1, T[1]]))))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_md_windows_equal_cigar_windows_equal_oracle():
    """3 targets of 1,200 to 1,500 bases, windows tiled at 500 with overlap 150: consensus_cigar_md(windows) ==
    consensus_cigar_windows on the twin's T == the oracle per window; the three-step form."""
    from pbdagcon_amd import capi
    targets = _pileups(311, 3, 14, 1200, 1500, b"ACGT")
    targets = [(bb, sorted(recs, key=lambda r: r[0])) for bb, recs in targets]
    texts = _texts(targets)
    T, conflict = _twin_T(targets, texts)
    assert not any(conflict)
    wins = [(g, b, e) for g, (bb, _) in enumerate(targets) for b, e, _, _ in wt.tiled(len(bb), 500, 150)]
    hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    per = wt.window_targets([(t, recs) for t, (_, recs) in zip(T, targets)], wins)
    assert not any(f for _, _, f in per)
    exp = oracle_batch(batch_from_targets([(tl, alns, None) for tl, alns, _ in per]), MIN_COV, MIN_LEN, TRIM)
    assert sum(bool(x) for x in exp) >= len(wins) // 2
    md = _md_tags(texts)
    ctx = _full_ctx(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cigar_md(_cigar_batch(targets, None), md, hw))
        assert ctx.md_targets().tobytes() == b"".join(T)
        _same(a, _everything(ctx, lambda: ctx.consensus_cigar_windows(_cigar_batch(targets, T), hw)))
        assert a[0] == exp
        _same(a, _everything(ctx, lambda: ctx.consensus_cigar_md(_cigar_batch(targets, None, True), md, hw)))
        ctx.upload_cigar_md(_cigar_batch(targets, None), md, hw); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
    finally:
        ctx.close()


def _device_edits(ctx, got):
    ed = ctx.edits()
    sb, so, sl = ctx._segs
    out = []
    for t, segs in enumerate(got):
        per = []
        for k, (_, _, seq) in enumerate(segs):
            s = int(sb[t]) + k
            b, e = int(ed["edit_begin"][s]), int(ed["edit_begin"][s + 1])
            per.append((seq, int(ed["seg_t0"][s]), int(ed["seg_t1"][s]),
                        [(int(ed["t_pos"][i]), int(ed["t_len"][i]), int(ed["c_off"][i]) - int(so[s]), int(ed["c_len"][i]))
                         for i in range(b, e)]))
        out.append(per)
    return out


@pytest.mark.gpu
def test_md_under_the_record_filter_and_with_edits(pileup):
    """Under set_record_filter the results and record_stats equal the CIGAR call's on the twin's T; a record the filter
    drops that alone covers the last 40 bases of its target still contributes them to md_targets().  Under set_edits,
    edits() is equal, and the edits applied to md_targets() give every segment back."""
    import edits_twin as et
    targets, texts, _, _ = pileup
    rng = np.random.default_rng(4)
    bb0, recs0 = targets[0]
    tail = ACGT[rng.integers(0, 4, 40)].tobytes()
    bb0x = bb0 + tail
    noisy = bytearray(bb0x[-60:])
    for i in range(0, 60, 2):
        noisy[i] = ord("C") if noisy[i] == ord("G") else ord("G")
    lone = (len(bb0x) - 59, bytes(noisy), [ct.op("M", 60)])
    tg = [(bb0x, recs0 + [lone])] + targets[1:]
    tx = _texts(tg)
    T, conflict = _twin_T(tg, tx)
    assert not any(conflict) and T[0][-40:] == tail
    md, md_b, twin_b = _md_tags(tx), _cigar_batch(tg, None), _cigar_batch(tg, T)
    ctx = _full_ctx(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        ctx.set_record_filter(max_error_ppm=300000, max_depth=9)
        a = _everything(ctx, lambda: ctx.consensus_cigar_md(md_b, md))
        sa = ctx.record_stats()
        assert ctx.md_targets().tobytes() == b"".join(T)
        b = _everything(ctx, lambda: ctx.consensus_cigar(twin_b))
        sb = ctx.record_stats()
        _same(a, b)
        assert all(np.array_equal(sa[k], sb[k]) for k in sa)
        from pbdagcon_amd import capi
        assert sa["fate"][len(recs0)] == capi.FATE_MAX_ERROR and (sa["fate"] & capi.FATE_MAX_DEPTH).any()
        ctx.set_record_filter(None, None)
        ctx.set_edits(True)
        got = ctx.consensus_cigar_md(md_b, md)
        ea = _device_edits(ctx, got)
        tm = ctx.md_targets().tobytes()
        assert ea == _device_edits(ctx, ctx.consensus_cigar(twin_b))
        n, off = 0, 0
        for per, t in zip(ea, T):
            for seq, t0, t1, edits in per:
                assert et.apply_edits(tm[off:off + len(t)], t0, t1, edits, seq) == seq
                n += len(edits)
            off += len(t)
        assert n > 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_md_invalid_arguments_and_state(pileup):
    """md NULL with records, md_off + md_len > md_bytes, targets that are not ascending and disjoint, and what the CIGAR
    calls refuse: DAGCON_ERR_INVALID_ARG, and a valid call on the same context afterwards is exact.  md_targets() is
    DAGCON_ERR_STATE before any upload, after an upload of another kind and after a refused call."""
    from pbdagcon_amd import capi
    targets, texts, T, exp = pileup
    hb, md = _cigar_batch(targets, None), _md_tags(texts)
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)

    def batch(**kw):
        f = dict(tlen=hb.tlen, t_off=hb.t_off, t_blob=None, rec_begin=hb.rec_begin, pos=hb.pos, q_off=hb.q_off, q_len=hb.q_len,
                 q_blob=hb.q_blob, op_begin=hb.op_begin, ops=hb.ops)
        f.update(kw)
        return capi.HostCigarBatch(**f)

    def state_error():
        with pytest.raises(capi.DagconError) as e:
            ctx.md_targets()
        return e.value.code
    try:
        assert state_error() == -8
        n = md.n_records
        off, ln = md.md_off.copy(), md.md_len.copy()
        off[5] = md.md_blob.size
        ln[n - 1] += 1
        over = hb.t_off.copy(); over[3] -= 1                       # target 3 begins on the last byte of target 2
        swap = hb.t_off.copy(); swap[[0, 1]] = swap[[1, 0]]
        rb = hb.rec_begin.copy(); rb[2] = rb[3] + 1
        qo = hb.q_off.copy(); qo[7] = hb.q_blob.size
        wn = capi.HostWindows([0], [0], [int(hb.tlen[0]) + 1])
        cases = [(hb, capi.HostMdTags(off, md.md_len, md.md_blob), None), (hb, capi.HostMdTags(md.md_off, ln, md.md_blob), None),
                 (hb, capi.HostMdTags(md.md_off + np.uint64(1 << 40), md.md_len, md.md_blob), None), (hb, None, None),
                 (batch(t_off=over), md, None), (batch(t_off=swap), md, None), (batch(rec_begin=rb), md, None),
                 (batch(q_off=qo), md, None), (hb, md, wn)]
        for i, (b, m, w) in enumerate(cases):
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cigar_md(b, m, w)
            assert e.value.code == -1, i
            assert state_error() == -8
        bs, ms = hb.c_struct(), md.c_struct()
        assert ctx.L.dagcon_consensus_cigar_md(ctx.h, C.byref(bs), None, C.byref(ms), 0, None) == -1
        assert ctx.consensus_cigar_md(hb, md) == exp                  # (the context is as good as new)
        assert ctx.md_targets().tobytes() == b"".join(T)
        assert ctx.consensus_cigar(_cigar_batch(targets, T)) == exp
        assert state_error() == -8
        ctx.upload_cigar_md(hb, md)
        assert ctx.md_targets().tobytes() == b"".join(T)               # (valid from the upload on)
        ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pbdagcon_md_equals_pbdagcon_ref(tmp_path):
    """pbdagcon --sam --md and --bam --md print, byte for byte, what pbdagcon --sam --ref prints for the same records with
    an upper-case reference: FASTA, several batches, --window 400 --overlap 150 --fastq, the --edits file (whole targets
    and windows), --max-depth 8."""
    targets = _pileups(321, 5, 12, 500, 900, b"ACGT")
    targets = [(bb, sorted(recs, key=lambda r: r[0])) for bb, recs in targets]
    ref, sam, mds, mdb, _ = _files(tmp_path, targets)

    def run(*args):
        out = _run(*args)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout
    common = ["-m", "100", "-t", "10"]
    old = ["--sam", "--ref", str(ref), *common]
    news = [["--sam", "--md", *common, str(mds)], ["--bam", "--md", *common, str(mdb)]]
    want = run(*old, str(sam))
    assert want.count(b">ctg") >= 4
    for new in news:
        assert run(*new) == want
        assert run(*new, "--batch-targets", "2", "--contexts", "2", "-j", "3") == want
    w = ["--window", "400", "--overlap", "150", "--fastq"]
    want = run(*old, *w, str(sam))
    assert want.count(b"@ctg") >= 4
    for new in news:
        assert run(*new, *w) == want
        assert run(*new, *w, "--batch-targets", "3") == want
    want = run(*old, "--max-depth", "8", str(sam))
    for new in news:
        assert run(*new, "--max-depth", "8") == want
    for extra in ([], ["--window", "400", "--overlap", "150"], ["--window", "400", "--overlap", "150", "--batch-targets", "2"]):
        e0 = tmp_path / "old.edits"
        want = run(*old, *extra, "--edits", str(e0), str(sam))
        assert e0.read_bytes().count(b"#piece") >= 4 and e0.read_bytes().count(b"\n") > e0.read_bytes().count(b"#piece")
        for k, new in enumerate(news):
            e1 = tmp_path / ("new%d.edits" % k)
            assert run(*new, *extra, "--edits", str(e1)) == want
            assert e1.read_bytes() == e0.read_bytes(), (extra, new[0])
