"""PAF input: pbdagcon --paf --ref --reads, and the stranded entry points under it (dagcon_upload_cigar_strand /
dagcon_consensus_cigar_strand: the reads as the reads file has them, one strand flag per record, the bases of a reverse
record read backwards and complemented where k_cigar_expand gathers them).

What is pinned to what.  The stranded calls equal the unstranded calls on the same batch with every reverse record's
bases reverse-complemented on the host (segments, status, support, positions), and those equal the oracle through the
twin's strings (tests/paf_files.py: expand_strand, cigar_twin.expand over the header's index rule and complement).
`pbdagcon --paf` equals `pbdagcon --sam` on the same alignments, parser dump and output.  The PAF files come from
tests/paf_files.py, this suite's own writer: no minimap2 is behind it.  The complement (lower case too) is this build's
own rule; the reference reads no PAF."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_twin as ct
import paf_files as pf
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _run(*args, env=None, stdin=None, timeout=600):
    return subprocess.run([_cli(), *args], capture_output=True, env=env, input=stdin, timeout=timeout)


def _twin_targets(seed, n_targets, reads, lo, hi, full_span=False, eqx=False):
    """[(target bases, [(pos, read bases, ops)])] and the raw [(tlen, alns, backbone)] they come from."""
    rng = np.random.default_rng(seed)
    raw, out = [], []
    for g in range(n_targets):
        tl = int(rng.integers(lo, hi))
        alns, bb = random_target(rng, tl, reads, full_span=full_span)
        raw.append((tl, alns, bb))
        out.append((bb, [ct.compress(s, q, t, bb, eqx and g % 2 == 1) for s, q, t in alns]))
    return out, raw


# ---- CPU ---------------------------------------------------------------------------------------------------------

def test_library_exports_the_strand_entry_points():
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_upload_cigar_strand", "dagcon_consensus_cigar_strand"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.dagcon_abi_version() == 2 and C.sizeof(capi.CigarBatch) == 104
    src = open(os.path.join(ROOT, "include", "dagcon.h")).read()
    assert "this build's own, parity unpinned" in " ".join(src.replace(" * ", " ").split())


def test_strand_twin_agrees_with_the_host_reversed_read():
    """expand_strand (the header's index rule q[q_len - 1 - i] and comp, byte by byte) gives what cigar_twin.expand
    gives on the reverse complement made as a whole; comp swaps ACGT and acgt and keeps every other byte; a forward
    record is cigar_twin.expand itself.  Lengths 1, 2, 3 and records of more than 64 ops among them."""
    assert pf.revcomp(b"ACGTacgtNn-*RY") == b"YR*-nNacgtACGT"
    assert [pf.comp(b) for b in b"ACGTacgtN=.-"] == list(b"TGCAtgcaN=.-")
    assert all(pf.comp(pf.comp(b)) == b for b in range(256))
    assert sum(pf.comp(b) != b for b in range(256)) == 8
    targets, _ = _twin_targets(7, 3, 6, 150, 400)
    rng = np.random.default_rng(8)
    targets[0][1].extend([(5, b"g", [ct.op("M", 1)]), (9, b"Nt", [ct.op("=", 1), ct.op("X", 1)]),
                          (2, b"acG", [ct.op("S", 1), ct.op("M", 1), ct.op("I", 1)])])
    n_long = 0
    for tseq, recs in targets:
        for pos, q, ops in recs:
            q = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), len(q))) if rng.random() < 0.5 else q
            n_long += len(ops) > 64
            want = ct.expand(pos, q, tseq, ops)
            assert pf.expand_strand(pos, pf.revcomp(q), tseq, ops, True) == want
            assert pf.expand_strand(pos, q, tseq, ops, False) == want
    assert n_long >= 3


def test_host_batch_reverse_array():
    """HostCigarBatch takes reverse (one entry per record, kept as 0 / 1 bytes); packed() refuses such a batch."""
    from pbdagcon_amd import capi
    arr = ct.records_to_arrays([(b"ACGTACGT", [(1, b"ACG", [ct.op("M", 3)]), (2, b"CG", [ct.op("M", 2)])])])
    cb = capi.HostCigarBatch(reverse=[0, 7], **arr)
    assert cb.reverse.dtype == np.uint8 and cb.reverse.tolist() == [0, 1]
    assert capi.HostCigarBatch(**arr).reverse is None and capi.HostCigarBatch(**arr).packed().is_packed
    with pytest.raises(ValueError):
        cb.packed()
    with pytest.raises(ValueError):
        capi.HostCigarBatch(reverse=[1], **arr)


def _parser_case(seed=3):
    """Three small targets through from_twin: both strands, slices inside longer reads, lower case and N, a read
    aligned to two targets; then tp:A:S and cg-less lines in between and the lines shuffled across targets (a target's
    own lines stay in order)."""
    rng = np.random.default_rng(seed)
    targets, _ = _twin_targets(seed, 3, 5, 60, 200, eqx=True)
    targets[2][1].extend([(7, b"g", [ct.op("M", 1)]), (8, b"tN", [ct.op("=", 1), ct.op("X", 1)])])
    names = ["ctg0", "ctg1|x", "ctg2"]
    reads, alns = pf.from_twin(rng, names, targets)
    assert {x["strand"] for x in alns} == {"+", "-"}
    assert any(x["qs"] > 0 and x["qe"] < len(reads[x["qname"]]) for x in alns)
    two = [q for q in reads if len({x["tname"] for x in alns if x["qname"] == q}) == 2]
    assert len(two) == 2
    blob = b"".join(reads.values())
    assert re.search(rb"[acgt]", blob) and b"N" in blob
    # shuffled across targets: a random merge of the per-target lists
    per = [[x for x in alns if x["tname"] == n] for n in names]
    order = rng.permutation(np.repeat(np.arange(3), [len(p) for p in per])).tolist()
    shuffled = [per[g].pop(0) for g in order]
    assert [x["tname"] for x in shuffled] != sorted(x["tname"] for x in shuffled)
    return names, targets, reads, alns, shuffled


def _write_case(tmp_path, names, targets, reads, alns, lines, fastq=False):
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta([n + " some description" for n in names], [t for t, _ in targets], width=50))
    rd = tmp_path / ("reads.fq" if fastq else "reads.fa")
    rd.write_bytes(pf.reads_fastq(reads) if fastq else pf.reads_fasta(reads, 40))
    sam = tmp_path / "in.sam"
    sam.write_bytes(pf.sam_text(names, [len(t) for t, _ in targets], reads, alns))
    paf = tmp_path / "in.paf"
    text = pf.paf_text(reads, lines)
    assert b"\r" not in text and text.endswith(b"\n")
    paf.write_bytes(text)
    return ref, rd, sam, paf


def test_paf_parser_dump_equals_sam_parser_dump(tmp_path):
    """pbdagcon --paf --dump-parsed prints, byte for byte, what pbdagcon --sam --dump-parsed prints for the equivalent
    SAM records (soft clips qs and qlen - qe, swapped for '-'; SEQ the whole read in the target's orientation), targets
    in --ref order and a target's lines in file order: FASTA and FASTQ reads, a file and stdin; tp:A:S and cg-less lines
    are skipped and counted."""
    names, targets, reads, alns, shuffled = _parser_case()
    lines = list(shuffled)
    lines.insert(2, dict(shuffled[0], tp="S"))
    lines.insert(5, dict(shuffled[1], cg=False))
    lines.insert(6, dict(shuffled[3], cg=False, qname="nobody", tname="nowhere"))      # (skipped before it is looked at)
    lines.append(dict(shuffled[2], tp="S", cg=False))
    want = None
    for fastq in (False, True):
        ref, rd, sam, paf = _write_case(tmp_path, names, targets, reads, alns, lines, fastq)
        out = _run("--sam", "--ref", str(ref), "--dump-parsed", str(sam), env=NOGPU)
        assert out.returncode == 0, out.stderr.decode()
        want = out.stdout
        assert want.count(b"\n") == len(alns) and b"\t-\t" in want and b"\t+\t" in want
        for src, stdin in ((str(paf), None), ("-", paf.read_bytes())):
            got = _run("--paf", "--ref", str(ref), "--reads", str(rd), "--dump-parsed", "-v", src, env=NOGPU, stdin=stdin)
            assert got.returncode == 0, got.stderr.decode()
            assert got.stdout == want, (fastq, src)
            assert re.search(rb"\b2 PAF lines without a cg:Z: tag skipped", got.stderr), got.stderr
            assert re.search(rb"\b2 PAF lines skipped \(tp:A:S\)", got.stderr), got.stderr
            assert got.stderr.count(b"without a cg:Z:") == 1
        # -j and --batch-targets change nothing
        got = _run("--paf", "--ref", str(ref), "--reads", str(rd), "--dump-parsed", "-j", "3", "--batch-targets", "1", str(paf), env=NOGPU)
        assert got.returncode == 0 and got.stdout == want
    # the order is --ref order whatever the file's: the targets' lines the other way round give the same dump
    ref, rd, sam, paf = _write_case(tmp_path, names, targets, reads, alns, sorted(alns, key=lambda x: -names.index(x["tname"])))
    got = _run("--paf", "--ref", str(ref), "--reads", str(rd), "--dump-parsed", str(paf), env=NOGPU)
    assert got.returncode == 0 and got.stdout == want and b"cg:Z:" not in got.stderr


def test_paf_target_span_mismatch_skips_the_target(tmp_path):
    """A cg that does not consume exactly te - ts target bases takes its target out with a warning that names the line
    (exit 0, the other targets are complete), as the library does for a cg that does not fit qe - qs."""
    names, targets, reads, alns, _ = _parser_case(5)
    bad = next(i for i, x in enumerate(alns) if x["tname"] == names[1])
    lines = [dict(x) for x in alns]
    lines[bad]["te"] -= 1
    ref, rd, sam, paf = _write_case(tmp_path, names, targets, reads, [x for x in alns if x["tname"] != names[1]], lines)
    want = _run("--sam", "--ref", str(ref), "--dump-parsed", str(sam), env=NOGPU)
    got = _run("--paf", "--ref", str(ref), "--reads", str(rd), "--dump-parsed", str(paf), env=NOGPU)
    assert got.returncode == 0 and want.returncode == 0 and got.stdout == want.stdout
    assert re.search(rb"warning: target ctg1\|x skipped \(line %d: " % (bad + 1), got.stderr), got.stderr


def test_paf_usage_and_input_errors(tmp_path):
    """Every usage error is exit 2 before any input is opened; every malformed line, unknown name, duplicate read and
    length that disagrees with the files is exit 1 with a message that names the line (or the read)."""
    names, targets, reads, alns, _ = _parser_case(4)
    ref, rd, sam, paf = _write_case(tmp_path, names, targets, reads, alns, alns)
    base = ["--paf", "--ref", str(ref), "--reads", str(rd)]
    for args in (["--paf", "--reads", str(rd), str(paf)], ["--paf", "--ref", str(ref), str(paf)],
                 base + ["--sam", str(paf)], base + ["--bam", str(paf)], base + ["-a", str(paf)],
                 base + ["--polish", "1", str(paf)], ["--reads", str(rd), str(paf)],
                 ["--sam", "--ref", str(ref), "--reads", str(rd), str(sam)], base + ["--reads"]):
        out = _run(*args, "--dump-parsed", env=NOGPU)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, (args, out.stderr)
    help_text = _run("--help").stdout
    assert b"--paf" in help_text and b"--reads" in help_text and b"--bam" in help_text and b"are not read" in help_text

    def dump(text, reads_path=rd):
        paf.write_bytes(text)
        return _run("--paf", "--ref", str(ref), "--reads", str(reads_path), "--dump-parsed", str(paf), env=NOGPU)
    good = pf.paf_text(reads, alns).decode().split("\n")[:-1]
    assert dump(("\n".join(good) + "\n").encode()).returncode == 0
    k = 3                                                            # the line that is broken, 1-based k + 1

    def broken(edit):
        f = good[k].split("\t")
        edit(f)
        return ("\n".join(good[:k] + ["\t".join(f)] + good[k + 1:]) + "\n").encode()

    def setf(i, v):
        return lambda f: f.__setitem__(i, v)
    x = alns[k]
    cg = 14
    assert good[k].split("\t")[cg].startswith("cg:Z:")
    cases = [
        (lambda f: f.__delitem__(slice(11, None)), rb"line 4: .*12 fields.* 11 fields"),
        (setf(4, "*"), rb"line 4: strand"),
        (setf(4, "+-"), rb"line 4: strand"),
        (setf(2, str(x["qe"])), rb"line 4: query slice"),
        (setf(3, str(len(reads[x["qname"]]) + 1)), rb"line 4: query slice"),
        (setf(2, "x"), rb"line 4: .*not an unsigned"),
        (setf(0, "nobody"), rb"line 4: query nobody is not a sequence of --reads"),
        (setf(5, "nowhere"), rb"line 4: target nowhere is not a sequence of --ref"),
        (lambda f: (f.__setitem__(1, str(int(f[1]) + 1))), rb"line 4: query .* has length"),
        (lambda f: (f.__setitem__(6, str(int(f[6]) + 1))), rb"line 4: target .* has length"),
        (setf(cg, "cg:Z:12"), rb"line 4: malformed cg:Z:"),
        (setf(cg, "cg:Z:5Q"), rb"line 4: malformed cg:Z:"),
        (setf(cg, "cg:Z:"), None),                                   # (no ops: consumes no target base -> its target is skipped)
    ]
    for edit, msg in cases:
        out = dump(broken(edit))
        if msg is None:
            assert out.returncode == 0 and b"warning: target" in out.stderr and b"line 4" in out.stderr
            continue
        assert out.returncode == 1 and out.stdout == b"", (msg, out.stderr)
        assert re.search(msg, out.stderr), (msg, out.stderr)
    # the reads file: a name twice, neither FASTA nor FASTQ, a cut FASTQ record, a missing file
    twice = tmp_path / "twice.fa"
    twice.write_bytes(pf.reads_fasta(reads) + b">" + alns[0]["qname"].encode() + b"\nACGT\n")
    out = dump(("\n".join(good) + "\n").encode(), twice)
    assert out.returncode == 1 and alns[0]["qname"].encode() + b" occurs twice" in out.stderr
    twice.write_bytes(pf.reads_fastq(reads) + b"@" + alns[0]["qname"].encode() + b"\nACGT\n+\nIIII\n")
    out = dump(("\n".join(good) + "\n").encode(), twice)
    assert out.returncode == 1 and alns[0]["qname"].encode() + b" occurs twice" in out.stderr
    twice.write_bytes(b"\x1f\x8b\x08rest")
    out = dump(("\n".join(good) + "\n").encode(), twice)
    assert out.returncode == 1 and b"neither FASTA" in out.stderr
    twice.write_bytes(pf.reads_fastq(reads)[:-3].rsplit(b"\n", 2)[0] + b"\n")
    out = dump(("\n".join(good) + "\n").encode(), twice)
    assert out.returncode == 1 and b"four-line FASTQ" in out.stderr
    out = dump(("\n".join(good) + "\n").encode(), tmp_path / "none.fa")
    assert out.returncode == 1 and b"error opening file" in out.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------

def _stranded(targets, reverse, ids=None):
    """(the stranded batch: the bases of record r as a reads file would have them, reverse[r]; the unstranded batch with
    the bases in the target's orientation: the first one reverse-complemented on the host)."""
    from pbdagcon_amd import capi
    flat = [(bb, [(p, pf.revcomp(q) if reverse[i] else q, o) for i, (p, q, o) in zip(range(n0, n0 + len(recs)), recs)])
            for (bb, recs), n0 in zip(targets, np.cumsum([0] + [len(r) for _, r in targets])[:-1].tolist())]
    st = capi.HostCigarBatch(ids=ids, reverse=np.asarray(reverse, np.uint8), **ct.records_to_arrays(flat))
    un = capi.HostCigarBatch(ids=ids, **ct.records_to_arrays(targets))
    return st, un


def _twin_strings(targets_as_file, reverse):
    """The strings batch the twin makes of a stranded batch's records, for the oracle."""
    out, i = [], 0
    for bb, recs in targets_as_file:
        alns = []
        for p, q, o in recs:
            alns.append(pf.expand_strand(p, q, bb, o, bool(reverse[i])))
            i += 1
        out.append((len(bb), alns, bb))
    return batch_from_targets(out)


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


STRANDS = ["forward", "reverse", "mixed"]


@pytest.fixture(scope="module")
def pileup():
    targets, raw = _twin_targets(101, 5, 40, 900, 2200)
    sb = batch_from_targets(raw)
    return targets, oracle_batch(sb)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STRANDS)
def test_strand_equals_host_reversed_equals_oracle(pileup, kind):
    """consensus_cigar with reverse == consensus_cigar on the host-reversed batch == the oracle on the twin's strings:
    segments, target_status, base_support() and base_positions(); all forward, all reverse, mixed; records of several
    tiles (more than 64 ops); the three-step form."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    n = sum(len(r) for _, r in targets)
    rng = np.random.default_rng(11)
    reverse = {"forward": np.zeros(n, np.uint8), "reverse": np.ones(n, np.uint8), "mixed": rng.integers(0, 2, n).astype(np.uint8)}[kind]
    st, un = _stranded(targets, reverse)
    assert int(np.diff(st.op_begin.astype(np.int64)).min()) > 64
    assert (kind == "forward") == (st.q_blob.tobytes() == un.q_blob.tobytes())
    file_targets = [(bb, [(p, pf.revcomp(q) if reverse[i] else q, o) for i, (p, q, o) in zip(range(n0, n0 + len(recs)), recs)])
                    for (bb, recs), n0 in zip(targets, np.cumsum([0] + [len(r) for _, r in targets])[:-1].tolist())]
    assert oracle_batch(_twin_strings(file_targets, reverse)) == exp and all(exp)
    ctx = capi.Context(flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cigar(st))
        ta = ctx.timings()
        b = _everything(ctx, lambda: ctx.consensus_cigar(un))
        tb = ctx.timings()
        _same(a, b)
        assert a[0] == exp
        for key in ("consensus_bases", "n_alignments", "n_targets"):
            if key in ta:
                assert ta[key] == tb[key], key
        ctx.upload_cigar(st); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
    finally:
        ctx.close()


@pytest.mark.gpu
def test_strand_tiny_reads_soft_masked_bases_and_the_graph():
    """DAGCON_FLAG_STOP_AFTER_BUILD: the graph addAln leaves is the same, vertex by vertex, from the stranded batch and
    from the host-reversed one, so the strings are the same and not merely the consensus: reads of 1, 2, 3 and 4 bases,
    lower case, N and other bytes (complemented or kept as the header says), clips on either side of a reverse
    record, and two records that name the same bytes of q_blob on opposite strands."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(12)
    targets = []
    for g in range(2):
        tl = 150 + 37 * g
        alns, bb = random_target(rng, tl, 9, alphabet=b"ACGTacgtNn")
        recs = [ct.compress(s, q, t, bb, eqx=bool(g)) for s, q, t in alns]
        recs += [(4, b"g", [ct.op("M", 1)]), (9, b"tN", [ct.op("=", 1), ct.op("X", 1)]),
                 (11, b"aRc", [ct.op("M", 1), ct.op("I", 1), ct.op("M", 1)]),
                 (20, b"NNacgT*YKa", [ct.op("S", 2), ct.op("M", 2), ct.op("D", 3), ct.op("M", 2), ct.op("S", 4)])]
        targets.append((bb, recs))
    n = sum(len(r) for _, r in targets)
    reverse = np.ones(n, np.uint8)
    reverse[::3] = 0
    st, un = _stranded(targets, reverse)
    assert {1, 2, 3, 10} <= set(st.q_len.tolist())
    # one more record: the bytes of record 0, named a second time, on the other strand
    p0, q0, o0 = targets[0][1][0]
    q0r = pf.revcomp(q0)
    tl0 = len(targets[0][0])
    extra_ops = [ct.op("S", len(q0) - 1), ct.op("M", 1)] if len(q0) > 1 else [ct.op("M", 1)]

    def with_extra(cb, bases, rev):
        """cb plus a record at the end of target 0... as a new last target holding it alone (target 0's bases again)."""
        qb = cb.q_blob if bases is None else np.concatenate([cb.q_blob, np.frombuffer(bases, np.uint8)])
        q_off = np.concatenate([cb.q_off, [cb.q_off[0] if bases is None else cb.q_blob.size]]).astype(np.uint64)
        return capi.HostCigarBatch(np.concatenate([cb.tlen, [tl0]]), np.concatenate([cb.t_off, [cb.t_off[0]]]), cb.t_blob,
                                   np.concatenate([cb.rec_begin, [cb.rec_begin[-1] + 1]]), np.concatenate([cb.pos, [tl0]]),
                                   q_off, np.concatenate([cb.q_len, [len(q0)]]), qb,
                                   np.concatenate([cb.op_begin, [cb.op_begin[-1] + len(extra_ops)]]),
                                   np.concatenate([cb.ops, np.asarray(extra_ops, np.uint32)]),
                                   reverse=None if rev is None else np.concatenate([reverse, [rev]]))
    st2 = with_extra(st, None, 1 - int(reverse[0]))                  # overlapping range, opposite strand
    un2 = with_extra(un, q0r, None)
    assert int(st2.q_off[-1]) == int(st2.q_off[0]) and st2.reverse[-1] != st2.reverse[0]
    ctx = capi.Context(min_cov=0, min_len=0, trim=0, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    try:
        ctx.consensus_cigar(st2)
        a = [ctx.debug_graph(t) for t in range(3)]
        ctx.consensus_cigar(un2)
        b = [ctx.debug_graph(t) for t in range(3)]
    finally:
        ctx.close()
    assert a == b and all(len(g) > 100 for g in a[:2]) and len(a[2]) >= 3


@pytest.mark.gpu
def test_strand_nonconforming_reverse_record_fails_its_target_only(pileup):
    """A reverse record whose ops consume one base fewer than q_len fails its own target (DAGCON_ERR_NONCONFORMING, no
    segments); the other targets are complete and exact, and an out-of-blob q_off is INVALID_ARG as ever."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    targets = [(bb, list(recs)) for bb, recs in targets]
    p, q, o = targets[2][1][3]
    targets[2][1][3] = (p, q + b"A", o)
    n = sum(len(r) for _, r in targets)
    reverse = np.ones(n, np.uint8)
    reverse[1::2] = 0
    bad = sum(len(r) for _, r in targets[:2]) + 3
    reverse[bad] = 1
    st, un = _stranded(targets, reverse)
    ctx = capi.Context()
    try:
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar(st)
        assert e.value.code == -4
        got = ctx.consensus_cigar(st, strict=False)
        assert ctx.target_status.tolist() == [0, 0, -4, 0, 0]
        assert got == exp[:2] + [[]] + exp[3:]
        assert ctx.consensus_cigar(un, strict=False) == got
        arr = dict(tlen=st.tlen, t_off=st.t_off, t_blob=st.t_blob, rec_begin=st.rec_begin, pos=st.pos, q_off=st.q_off.copy(),
                   q_len=st.q_len, q_blob=st.q_blob, op_begin=st.op_begin, ops=st.ops)
        arr["q_off"][5] = st.q_blob.size
        with pytest.raises(capi.DagconError) as e:
            ctx.consensus_cigar(capi.HostCigarBatch(reverse=reverse, **arr))
        assert e.value.code == -1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_strand_windows_equal_host_reversed_windows_equal_oracle():
    """The same through windows (k_cigar_expand_cut_strand): windows with overlap that cut reverse records, against the
    unstranded windows call on the host-reversed batch (segments, status, support, positions) and against the oracle on
    the twin's pieces."""
    from pbdagcon_amd import capi
    targets, _ = _twin_targets(111, 3, 30, 1500, 2600)
    targets = [(bb, sorted(recs, key=lambda r: r[0])) for bb, recs in targets]
    n = sum(len(r) for _, r in targets)
    reverse = np.random.default_rng(13).integers(0, 2, n).astype(np.uint8)
    st, un = _stranded(targets, reverse)
    wins = [(g, b, e) for g, (bb, _) in enumerate(targets) for b, e, _, _ in wt.tiled(len(bb), 500, 150)]
    hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    per = wt.window_targets(targets, wins)
    assert not any(f for _, _, f in per)
    # a reverse record is cut by a window
    i = 0
    cut = 0
    for g, (bb, recs) in enumerate(targets):
        for p, q, o in recs:
            s, e = wt.span(p, len(bb), o)
            cut += bool(reverse[i]) and any(w[0] == g and s < w[1] < e for w in wins)
            i += 1
    assert cut > 10
    exp = oracle_batch(batch_from_targets([(tl, alns, None) for tl, alns, _ in per]), 6, 200, 50)
    assert sum(bool(x) for x in exp) > len(wins) // 2
    ctx = capi.Context(min_len=200, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        a = _everything(ctx, lambda: ctx.consensus_cigar_windows(st, hw))
        b = _everything(ctx, lambda: ctx.consensus_cigar_windows(un, hw))
        _same(a, b)
        assert a[0] == exp
        ctx.upload_cigar_windows(st, hw); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
    finally:
        ctx.close()


@pytest.mark.gpu
def test_strand_entry_points_with_reverse_null_are_the_unstranded_calls(pileup):
    """dagcon_consensus_cigar_strand(reverse = NULL) is dagcon_consensus_cigar, with windows dagcon_consensus_cigar_windows;
    results == NULL is INVALID_ARG."""
    from pbdagcon_amd import capi
    targets, exp = pileup
    un = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    wins = [(g, 0, len(bb)) for g, (bb, _) in enumerate(targets)]
    hw = capi.HostWindows([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    ctx = capi.Context()
    try:
        b, w = un.c_struct(), hw.c_struct()
        for win in (None, C.byref(w)):
            assert ctx.L.dagcon_upload_cigar_strand(ctx.h, C.byref(b), win, None) == 0
            ctx.run(); ctx.sync()
            assert ctx.fetch() == exp
        assert ctx.consensus_cigar(un) == exp
        assert ctx.L.dagcon_consensus_cigar_strand(ctx.h, C.byref(b), None, None, None) == -1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pbdagcon_paf_equals_sam(tmp_path):
    """pbdagcon --paf prints, byte for byte, what pbdagcon --sam prints for the same alignments: plain (one batch and
    several, on two contexts) and with --window W --overlap O --fastq; both strands, reads shared between targets, PAF
    lines shuffled across targets, FASTQ reads."""
    targets, _ = _twin_targets(121, 4, 30, 1000, 2000)
    names = ["ctg%d|x" % g for g in range(4)]
    rng = np.random.default_rng(14)
    reads, alns = pf.from_twin(rng, names, targets, sort_pos=True)
    assert {x["strand"] for x in alns} == {"+", "-"}
    per = [[x for x in alns if x["tname"] == n] for n in names]
    order = rng.permutation(np.repeat(np.arange(4), [len(p) for p in per])).tolist()
    shuffled = [per[g].pop(0) for g in order]
    ref, rd, sam, paf = _write_case(tmp_path, names, targets, reads, alns, shuffled, fastq=True)

    def run(*args):
        out = _run(*args)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout
    p = ["--paf", "--ref", str(ref), "--reads", str(rd)]
    s = ["--sam", "--ref", str(ref)]
    want = run(*s, str(sam))
    assert want.count(b">") >= 4
    assert run(*p, str(paf)) == want
    assert run(*p, "--batch-targets", "2", "--contexts", "2", "-j", "3", str(paf)) == want
    w = ["--window", "400", "--overlap", "150", "--fastq", "-m", "200"]
    want = run(*s, *w, str(sam))
    assert want.count(b"@ctg") >= 4
    assert run(*p, *w, str(paf)) == want
    assert run(*p, *w, "--batch-targets", "3", str(paf)) == want
