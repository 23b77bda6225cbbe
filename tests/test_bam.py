"""BAM input: pbdagcon --bam, and the packed entry points under it (dagcon_upload_cigar_packed /
dagcon_consensus_cigar_packed: read bases in BAM's 4-bit encoding, unpacked where k_cigar_expand gathers them).

What is pinned to what.  The packed calls equal the unpacked calls on the same batch (segments, status, support,
positions), and the unpacked calls equal the oracle through the strings path, the chain tests/test_cigar.py has.
`pbdagcon --bam` equals `pbdagcon --sam` on the same records, parser dump and output.  The BAM files come from
tests/bam_files.py, this suite's own writer from the SAM/BAM specification: no htslib, samtools or pysam is behind it,
so the reader's parity with other writers' files is unpinned.

Cases of the parser comparison: the small record set runs at every level x payload size x EOF setting; the set with
the record of more than 65,535 ops (a third of a megabyte of BAM) runs at every level and EOF setting with payloads
of 0xFF00 and 4,099 bytes only -- a one-byte payload would make a third of a million members of it in Python."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bam_files as bf
import cigar_twin as ct
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")

LEVELS = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
          (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)]
PAYLOADS = [0xFF00, 4099, 61, 1]


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _run(*args, env=None, stdin=None, timeout=600):
    return subprocess.run([_cli(), *args], capture_output=True, env=env, input=stdin, timeout=timeout)


def _rec(qname, flag, ref, pos, ops, seq):
    return dict(qname=qname, flag=flag, ref=ref, pos=pos, ops=list(ops), seq=bytes(seq))


# ---- CPU ---------------------------------------------------------------------------------------------------------

def test_library_exports_the_packed_entry_points():
    """The two entry points are exported and listed; the ABI version and the size of every struct the compiler sees
    are what their ctypes mirrors (and tests/test_abi.py, tests/test_cigar.py) have."""
    import tempfile
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_upload_cigar_packed", "dagcon_consensus_cigar_packed"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert lib.dagcon_abi_version() == 2
    prog = r'''
#include <stdio.h>
#include "dagcon.h"
int main(void){
 int (*up)(dagcon_ctx *, const dagcon_cigar_batch *, const dagcon_windows *) = dagcon_upload_cigar_packed;
 int (*co)(dagcon_ctx *, const dagcon_cigar_batch *, const dagcon_windows *, dagcon_results *) = dagcon_consensus_cigar_packed;
 printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(dagcon_opts), sizeof(dagcon_batch), sizeof(dagcon_pre_batch),
        sizeof(dagcon_cigar_batch), sizeof(dagcon_windows), sizeof(dagcon_results), sizeof(dagcon_support), up && co);
 return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-c", "-o", os.path.join(d, "s.o"), os.path.join(d, "s.c")])
        subprocess.check_call(["gcc", "-o", os.path.join(d, "s"), os.path.join(d, "s.o"), "-L", os.path.join(ROOT, "pbdagcon_amd"),
                               "-ldagcon_hip", "-Wl,-rpath," + os.path.join(ROOT, "pbdagcon_amd"), "-Wl,-rpath,/opt/rocm/lib"])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "s")], env=NOGPU).split()]
    assert out == [ctypes.sizeof(capi.Opts), ctypes.sizeof(capi.Batch), ctypes.sizeof(capi.PreBatch), ctypes.sizeof(capi.CigarBatch),
                   ctypes.sizeof(capi.Windows), ctypes.sizeof(capi.Results), ctypes.sizeof(capi.Support), 1]
    assert ctypes.sizeof(capi.CigarBatch) == 104 and ctypes.sizeof(capi.Windows) == 32


def test_nibbles_round_trip_and_packed_twin():
    """unpack(pack(x)) == x for odd and even lengths over all 16 letters; HostCigarBatch.packed() lays every record
    out as the twin does, each on a byte of its own; letters BAM does not have raise ValueError."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    assert bf.pack_nibbles(b"=ACMGRSVTWYHKDBN") == bytes.fromhex("0123456789abcdef")
    assert bf.pack_nibbles(b"ACG") == bytes([0x12, 0x40]) and bf.unpack_nibbles(bytes([0x12, 0x4f]), 3) == b"ACG"
    seqs = []
    for n in list(range(0, 40)) + [255, 256, 1001]:
        s = bytes(bf.NT16[i] for i in rng.integers(0, 16, n))
        assert len(bf.pack_nibbles(s)) == (n + 1) // 2 and bf.unpack_nibbles(bf.pack_nibbles(s), n) == s
        seqs.append(s)
    assert set(b"".join(seqs)) == set(bf.NT16)
    tseq = b"ACGT" * 300
    recs = [(1, s, [ct.op("S", len(s) - 1), ct.op("M", 1)] if len(s) > 1 else [ct.op("M", 1)]) for s in seqs if s]
    cb = capi.HostCigarBatch(**ct.records_to_arrays([(tseq, recs[:20]), (tseq, recs[20:])]))
    pb = cb.packed()
    assert pb.is_packed and not cb.is_packed and pb.packed() is pb
    assert pb.q_len.tolist() == cb.q_len.tolist() and pb.ops is cb.ops or np.array_equal(pb.ops, cb.ops)
    assert pb.q_blob.tobytes() == b"".join(bf.pack_nibbles(s) for _, s, _ in recs)
    off = np.concatenate([[0], np.cumsum([(len(s) + 1) // 2 for _, s, _ in recs])[:-1]])
    assert pb.q_off.tolist() == off.tolist()
    assert pb.nbytes == cb.nbytes - cb.q_blob.size + sum((len(s) + 1) // 2 for _, s, _ in recs)
    for bad in (b"ACGTa", b"ACG-", b"acgt", b"AC.T"):
        with pytest.raises(ValueError):
            capi.HostCigarBatch(**ct.records_to_arrays([(tseq, [(1, bad, [ct.op("M", len(bad))])])])).packed()


def _parser_records(seed=3, eqx=False, long_cigar=False):
    """refs, their bases, the records: random_target pileups through cigar_twin.compress (leading insertions among
    them), clips and pads, = and IUPAC letters, reads of 1 and 2 bases, reverse and supplementary flags, and unmapped,
    secondary and starred records in between."""
    rng = np.random.default_rng(seed)
    names, seqs, records = [], [], []
    lead = 0
    for g in range(3):
        tl = int(rng.integers(60, 200))
        alns, bb = random_target(rng, tl, 5)
        names.append("ctg%d" % g); seqs.append(bb)
        for k, (s, q, t) in enumerate(alns):
            lead += t[:1] == b"-"
            p, qq, ops = ct.compress(s, q, t, bb, eqx)
            records.append(_rec("q%d_%d" % (g, k), 0, g, p, ops, qq))
    assert lead >= 1
    r = records[5]                                                   # clipped flanks (an odd soft clip), a pad
    r["seq"] = b"NRY" + r["seq"] + b"K"
    r["ops"] = [ct.op("H", 4), ct.op("S", 3)] + r["ops"][:1] + [ct.op("P", 2)] + r["ops"][1:] + [ct.op("S", 1), ct.op("H", 1)]
    r = records[7]                                                   # '=' and every IUPAC letter in SEQ
    r["seq"] = bf.NT16 + r["seq"]
    r["ops"] = [ct.op("S", 16)] + r["ops"]
    records[2]["flag"] = 16
    records[3]["flag"] = 2048
    records[8]["flag"] = 2048 | 16
    records.insert(4, _rec("unmapped", 4, -1, 0, [], b"ACGTN"))
    records.insert(6, _rec("unmapped_placed", 4 | 16, 1, 17, [], b"GATTACA"))
    records.insert(9, _rec("secondary", 0x100, 1, 3, [ct.op("M", 4)], b"ACGT"))
    records.insert(11, _rec("no_ref", 0, -1, 0, [ct.op("M", 3)], b"ACG"))
    records.insert(12, _rec("no_cigar", 0, 1, 9, [], b"ACG"))
    records.insert(13, _rec("no_seq", 0, 1, 9, [ct.op("M", 3)], b""))
    records.append(_rec("one_base", 0, 2, 7, [ct.op("M", 1)], b"G"))
    records.append(_rec("two_bases", 16, 2, 8, [ct.op("=", 1), ct.op("X", 1)], b"TW"))
    records.append(_rec("one_of_three", 0, 2, 9, [ct.op("S", 1), ct.op("M", 1), ct.op("S", 1)], b"ACG"))
    if long_cigar:
        n = 32769
        bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, n + 50))
        names.append("long"); seqs.append(bb)
        ops = [ct.op("M", 1), ct.op("I", 1)] * (n - 1) + [ct.op("M", 1)]
        assert len(ops) == 65537
        q = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 2 * n - 1))
        records.append(_rec("long_cigar", 0, 3, 11, ops, q))
        records.append(_rec("after_long", 0, 3, 40, [ct.op("M", 5)], b"ACGTA"))
    refs = [(n, len(s)) for n, s in zip(names, seqs)]
    n_skip = 6
    return refs, seqs, records, n_skip


def _dump(fmt, ref, path, *extra):
    out = _run(fmt, "--ref", str(ref), "--dump-parsed", "-v", *extra, str(path), env=NOGPU)
    assert out.returncode == 0, out.stderr.decode()
    m = re.search(rb"(\d+) (SAM|BAM) records skipped", out.stderr)
    assert m, out.stderr
    return out.stdout, int(m.group(1)), out.stderr


def test_bam_parser_dump_equals_sam_parser_dump(tmp_path):
    """pbdagcon --bam --dump-parsed prints what pbdagcon --sam --dump-parsed prints for the SAM text of the same
    records, with the same skipped count, at every compression level (stored, fixed and dynamic blocks all occur: the
    first three bits of the members say so), payload size down to one byte (records straddle members), with and
    without the EOF member; -j, --slab-bytes and stdin change nothing."""
    seen_types = set()
    for eqx, long_cigar in ((False, False), (True, False), (False, True)):
        refs, seqs, records, n_skip = _parser_records(eqx=eqx, long_cigar=long_cigar)
        ref = tmp_path / "ref.fa"
        ref.write_bytes(ct.to_fasta([r[0] for r in refs], seqs, width=50))
        sam = tmp_path / "in.sam"
        sam.write_bytes(bf.sam_text(refs, records))
        want, skipped, _ = _dump("--sam", ref, sam)
        assert skipped == n_skip and want.count(b"\n") == len(records) - n_skip
        if eqx:
            assert b"=" in want and b"X" in want
        assert bf.NT16 in want and b"\tone_base\tG\t1M\n" in want and b"\ttwo_bases\tTW\t1=1X\n" in want
        raw = bf.bam_bytes(refs, records)
        if long_cigar:
            assert b"CGBI" in raw and b"\tlong_cigar\t" in want and want.count(b"1M1I") > 30000
        path = tmp_path / "in.bam"
        for level, strategy in LEVELS:
            for payload in (PAYLOADS[:2] if long_cigar else PAYLOADS):
                for eof in (True, False):
                    blob = bf.bgzf(raw, level, strategy, payload, eof)
                    types = bf.member_block_types(blob)
                    seen_types.update(types[:-1] if eof else types)
                    if payload < len(raw):
                        assert len(types) - eof >= 2                   # (records straddle members)
                    path.write_bytes(blob)
                    got, skipped, err = _dump("--bam", ref, path)
                    assert got == want, (level, strategy, payload, eof)
                    assert skipped == n_skip
                    assert (b"does not end with the empty BGZF member" in err) == (not eof)
        # the block types by level: stored at 0, fixed under Z_FIXED, dynamic at 6 with whole-size members
        assert set(bf.member_block_types(bf.bgzf(raw, 0, eof=False))) == {0}
        assert set(bf.member_block_types(bf.bgzf(raw, 6, zlib.Z_FIXED, eof=False))) == {1}
        assert 2 in bf.member_block_types(bf.bgzf(raw, 6, eof=False))
        blob = bf.bgzf(raw, 6, payload=977)
        path.write_bytes(blob)
        for extra in (["-j", "1"], ["-j", "7"], ["-j", "3", "--slab-bytes", "300"], ["--batch-targets", "1"]):
            assert _dump("--bam", ref, path, *extra)[0] == want
        out = _run("--bam", "--ref", str(ref), "--dump-parsed", "-", env=NOGPU, stdin=blob)
        assert out.returncode == 0 and out.stdout == want
    assert seen_types == {0, 1, 2}


def test_bam_errors_and_usage(tmp_path):
    """Every error of the reader has exit status 1 and names its member, record or reference; the usage errors have 2.
    No GPU is visible: none is needed to say so."""
    refs, seqs, records, _ = _parser_records()
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta([r[0] for r in refs], seqs))
    raw = bf.bam_bytes(refs, records)
    good = bf.bgzf(raw, 6, payload=500)
    path = tmp_path / "in.bam"

    def fails(blob, *words, extra=()):
        path.write_bytes(blob)
        out = _run("--bam", "--ref", str(ref), "--dump-parsed", *extra, str(path), env=NOGPU)
        assert out.returncode == 1, (words, out.stderr)
        for w in words:
            assert w in out.stderr, (w, out.stderr)
        return out
    path.write_bytes(good)
    assert _run("--bam", "--ref", str(ref), "--dump-parsed", str(path), env=NOGPU).returncode == 0
    mem = bf.members(good)
    assert len(mem) > 4
    # a flipped CRC byte and a wrong ISIZE, both in the third member
    p, size = mem[2]
    b = bytearray(good); b[p + size - 8] ^= 0x40
    fails(bytes(b), b"member 3", b"CRC32")
    b = bytearray(good); b[p + size - 4] ^= 0x01
    fails(bytes(b), b"member 3", b"ISIZE")
    # a corrupt payload: whatever the decoder meets first, the member is named
    b = bytearray(good)
    for k in range(20, 40):
        b[p + k] ^= 0xA5
    fails(bytes(b), b"member 3")
    # the file cut inside a member, and inside a record (the members themselves whole)
    fails(good[:mem[3][0] + 30], b"member 4", b"truncated")
    fails(good[:mem[3][0] + 7], b"member 4", b"truncated")
    n_whole = len(records) - 2
    whole = bf.bam_bytes(refs, records[:n_whole])
    fails(bf.bgzf(raw[:len(whole) + 40], 6, payload=500), ("record %d" % (n_whole + 1)).encode(), b"runs past the end")
    fails(bf.bgzf(raw[:len(whole) + 2], 6, payload=500), ("record %d" % (n_whole + 1)).encode(), b"runs past the end")
    # bad magic; plain gzip is not BGZF
    fails(bf.bgzf(b"BAM\2" + raw[4:]), b"magic")
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    fails(c.compress(raw) + c.flush(), b"member 1", b"BGZF")
    # refID >= n_ref
    bad = [dict(r) for r in records]
    bad[10]["ref"] = 3
    fails(bf.bgzf(bf.bam_bytes(refs, bad)), b"record 11", b"refID 3")
    # a reference length against --ref: the error --sam raises for a disagreeing @SQ LN, same exit status
    refs2 = list(refs); refs2[1] = (refs[1][0], refs[1][1] + 1)
    out = fails(bf.bgzf(bf.bam_bytes(refs2, records)), b"ctg1", b"--ref")
    sam = tmp_path / "bad.sam"
    sam.write_bytes(bf.sam_text(refs2, records))
    out_s = _run("--sam", "--ref", str(ref), "--dump-parsed", str(sam), env=NOGPU)
    assert out_s.returncode == out.returncode == 1 and b"ctg1" in out_s.stderr
    # a reference --ref does not hold, named by a record
    refs3 = list(refs); refs3[2] = ("nope", refs[2][1])
    first = next(i for i, r in enumerate(records) if r["ref"] == 2 and not (r["flag"] & 0x104) and r["ops"] and r["seq"])
    fails(bf.bgzf(bf.bam_bytes(refs3, records)), ("record %d" % (first + 1)).encode(), b"RNAME")
    # a reference coming back
    back = records + [dict(records[0])]
    fails(bf.bgzf(bf.bam_bytes(refs, back)), ("record %d" % len(back)).encode(), b"ctg0", b"come back")
    # descending pos with --window (the window driver parses before it asks for a GPU)
    srt = sorted((dict(r) for r in records if r["ref"] >= 0), key=lambda r: (r["ref"], r["pos"]))
    path.write_bytes(bf.bgzf(bf.bam_bytes(refs, srt)))
    out = _run("--bam", "--ref", str(ref), "--window", "100", "--overlap", "120", str(path), env=NOGPU)
    assert out.returncode == 1 and b"no CPU fallback" in out.stderr, out.stderr          # (sorted: read to the end)
    k = next(i for i, r in enumerate(srt) if i and r["ref"] == srt[i - 1]["ref"] == 0 and srt[i - 1]["pos"] > 1 and not r["flag"] & 0x104)
    desc = [dict(r) for r in srt]
    desc[k]["pos"] = desc[k - 1]["pos"] - 1
    path.write_bytes(bf.bgzf(bf.bam_bytes(refs, desc)))
    out = _run("--bam", "--ref", str(ref), "--window", "100", "--overlap", "120", str(path), env=NOGPU)
    assert out.returncode == 1 and ("record %d:" % (k + 1)).encode() in out.stderr and b"POS" in out.stderr and b"ctg0" in out.stderr, out.stderr
    path.write_bytes(bf.bgzf(bf.bam_bytes(refs, srt + [dict(srt[0])])))
    out = _run("--bam", "--ref", str(ref), "--window", "100", "--overlap", "120", str(path), env=NOGPU)
    assert out.returncode == 1 and ("record %d:" % (len(srt) + 1)).encode() in out.stderr and b"ctg0" in out.stderr, out.stderr
    # a placeholder CIGAR without its CG tag
    refs4, seqs4, records4, _ = _parser_records(long_cigar=True)
    ref.write_bytes(ct.to_fasta([r[0] for r in refs4], seqs4))
    k = next(i for i, r in enumerate(records4) if r["qname"] == "long_cigar")
    fails(bf.bgzf(bf.bam_bytes(refs4, records4, cg=False)), ("record %d" % (k + 1)).encode(), b"long_cigar", b"CG")
    # without a GPU the run itself fails loudly (no fallback), after reading
    path.write_bytes(bf.bgzf(bf.bam_bytes(refs4, records4)))
    out = _run("--bam", "--ref", str(ref), str(path), env=NOGPU)
    assert out.returncode == 1 and b"no CPU fallback" in out.stderr
    # usage
    for args in (["--bam", str(path)], ["--bam", "--sam", "--ref", str(ref), str(path)], ["--bam", "--ref", str(ref), "-a", str(path)],
                 ["--bam", "--ref", str(ref), "-a", "--local", str(path)], ["--bam", "--ref", str(ref), "--polish", "1", str(path)],
                 ["--bam", "--ref"]):
        out = _run(*args, env=NOGPU)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
    h = _run("--help", env=NOGPU)
    assert h.returncode == 0 and b"--bam" in h.stdout and b"are not read" in h.stdout
    assert b"BAM, PAF" not in h.stdout.replace(b"\n", b" ")


# ---- GPU ---------------------------------------------------------------------------------------------------------

IUPAC = np.frombuffer(b"ACGTNRYKMSWBDHV=", np.uint8)


def _clip(rng, p, q, ops, odd=None):
    """Soft-clipped flanks of random length (odd in front when asked) over all 16 letters, a hard clip and a pad."""
    a, z = int(rng.integers(0, 9)), int(rng.integers(0, 9))
    if odd is not None:
        a = (a | 1) if odd else (a & ~1)
    junk = bytes(rng.choice(IUPAC, a + z))
    k = int(rng.integers(1, max(2, len(ops))))
    ops = ([ct.op("H", 5)] + ([ct.op("S", a)] if a else []) + ops[:k] + [ct.op("P", 1)] + ops[k:] + ([ct.op("S", z)] if z else []))
    return p, junk[:a] + q + junk[a:], ops


def _packed_case(seed, full, eqx, min_cov, lo, hi, reads):
    """Pileups with clipped reads; the last but one target is below min_cov, the last holds a non-conforming record.
    Returns (strings batch, cigar batch, index of the failed target)."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(seed)
    targets, recs = [], []
    n = 6
    for g in range(n):
        tl = int(rng.integers(lo, hi))
        k = min_cov - 1 if g == n - 2 else reads
        alns, bb = random_target(rng, tl, k, full_span=full)
        targets.append((tl, alns, bb))
        rs = [_clip(rng, *ct.compress(s, q, t, bb, eqx), odd=bool(i % 2)) for i, (s, q, t) in enumerate(alns)]
        for (s, q, t), (p, qq, oo) in zip(alns, rs):
            assert ct.expand(p, qq, bb, oo) == (s, q, t)
        if g == n - 1:
            p, qq, oo = rs[2]
            rs[2] = (p, qq + b"A", oo)                                # one base more than the ops consume
        recs.append((bb, rs))
    sb = batch_from_targets(targets)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(recs))
    first = [int(cb.ops[int(o)]) & 15 for o in cb.op_begin[:-1]]
    assert first.count(ct.H) == len(first)
    soft = [int(cb.ops[int(o) + 1]) for o in cb.op_begin[:-1] if (int(cb.ops[int(o) + 1]) & 15) == ct.S]
    assert any((x >> 4) % 2 for x in soft) and any((x >> 4) % 2 == 0 for x in soft)      # first bases on both nibbles
    return sb, cb, n - 1


PARITY = [(full, opts, ms) for full in (True, False) for opts in ((6, 500, 50), (4, 60, 7)) for ms in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("full,opts,ms", PARITY)
def test_packed_equals_unpacked_equals_oracle(full, opts, ms):
    """consensus_cigar on the packed twin of a batch equals the unpacked batch -- segments, target_status,
    base_support(), base_positions() -- and both equal the oracle through the strings path: full-span and
    partial-span pileups, M and = / X ops, the option sets of tests/test_cigar.py, soft clips of odd and even length, a
    non-conforming record confined to its target, one target below min_cov."""
    from pbdagcon_amd import capi
    min_cov, min_len, trim = opts
    eqx = bool(ms)
    if min_len >= 500:
        sb, cb, bad = _packed_case(121 + full, full, eqx, min_cov, 900, 2200, 14 if full else 40)
    else:
        sb, cb, bad = _packed_case(131 + full, full, eqx, min_cov, 150, 700, 10 if full else 24)
    pb = cb.packed()
    assert pb.q_blob.size < cb.q_blob.size * 0.51 + cb.n_records
    exp = oracle_batch(sb, min_cov, min_len, trim)
    assert all(exp[:bad - 1]) and exp[bad - 1] == []
    exp[bad] = []
    ctx = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, max_segments=ms,
                       flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    try:
        res = []
        for b in (cb, pb, cb, pb):
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cigar(b)
            assert e.value.code == -4
            got = ctx.consensus_cigar(b, strict=False)
            res.append((got, ctx.target_status.tolist(), ctx.base_support(), ctx.base_positions(), ctx.timings()))
        # the three-step form
        ctx.upload_cigar(pb); ctx.run(); ctx.sync()
        assert ctx.fetch(strict=False) == exp
    finally:
        ctx.close()
    for got, status, sup, pos, tm in res:
        assert got == exp
        assert status == [0] * bad + [-4]
        assert [[(w.tolist(), d.tolist()) for w, d in t] for t in sup] == [[(w.tolist(), d.tolist()) for w, d in t] for t in res[0][2]]
        assert [[p.tolist() for p in t] for t in pos] == [[p.tolist() for p in t] for t in res[0][3]]
        for key in tm:
            if not key.startswith("ms_"):
                assert tm[key] == res[0][4][key], key
    assert sum(len(p) for t in res[1][3] for p in t) > 500


def _contig(seed, tlen, n_reads, read_len, long_read=None):
    """A random target and conforming records mapped along it, in POS order, every read with clipped flanks:
    (target bases, [(pos, read, ops)])."""
    rng = np.random.default_rng(seed)
    _, bb = random_target(rng, tlen, 1, full_span=True)
    recs = []
    spans = [(int(s), min(tlen, int(s) + read_len)) for s in sorted(rng.integers(0, max(1, tlen - read_len // 2), n_reads))]
    if long_read:
        spans.append(long_read)
        spans.sort()
    for k, (s, e) in enumerate(spans):
        sub_alns, _ = random_target(rng, e - s, 1, full_span=True)
        _, q, t = sub_alns[0]
        tb = bytearray(t); qb = bytearray(q); x = s
        for i in range(len(tb)):
            if tb[i] != ct.GAP:
                if qb[i] == tb[i]:
                    qb[i] = bb[x]
                tb[i] = bb[x]; x += 1
        recs.append(_clip(rng, *ct.compress(s + 1, bytes(qb), bytes(tb), bb, eqx=bool(k % 2)), odd=bool(k % 3 == 0)))
    return bb, recs


@pytest.mark.gpu
def test_packed_windows_equal_unpacked_equal_oracle():
    """The same with windows (HostWindows.tiled): a record crosses three windows; then a non-conforming record fails
    only the windows it has a piece in, from either form."""
    from pbdagcon_amd import capi
    bb0, recs0 = _contig(207, 2400, 70, 450, long_read=(650, 1650))
    bb1, recs1 = _contig(209, 650, 14, 600)
    targets = [(bb0, recs0), (bb1, recs1)]
    tlens = [2400, 650]
    wo = capi.HostWindows.tiled(tlens, 600, 100)
    windows = list(zip(wo.target.tolist(), wo.begin.tolist(), wo.end.tolist()))
    assert len(windows) == 4 + 2
    lr = [r for r in recs0 if wt.span(r[0], 2400, r[2]) == (650, 1650)]
    assert len(lr) == 1 and sum(1 for g, a, b in windows if g == 0 and max(a, 650) < min(b, 1650)) == 3
    opts = dict(min_cov=4, min_len=100, trim=10)

    def strings(tg):
        wtargets = wt.window_targets(tg, windows)
        return batch_from_targets([(tl, alns, None) for tl, alns, _ in wtargets]), [f for _, _, f in wtargets]
    sb, failed = strings(targets)
    assert not any(failed)
    exp = oracle_batch(sb, 4, 100, 10)
    assert sum(1 for e in exp if e) >= 5
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    pb = cb.packed()
    # a record inside [750, 1650) with an N in it: it fails the windows it reaches, no other
    k = next(i for i, r in enumerate(recs0) if 750 < wt.span(r[0], 2400, r[2])[0] and wt.span(r[0], 2400, r[2])[1] < 1650)
    p, q, ops = recs0[k]
    recs_bad = list(recs0)
    recs_bad[k] = (p, q, ops[:3] + [ct.op("N", 4)] + ops[3:])
    bad_targets = [(bb0, recs_bad), targets[1]]
    sb_bad, failed = strings(bad_targets)
    ks, ke = wt.span(*[recs_bad[k][0], 2400, recs_bad[k][2]])
    assert failed == [g == 0 and max(a, ks) < min(b, ke) for g, a, b in windows] and 1 <= sum(failed) <= 2 and not failed[0]
    exp_bad = oracle_batch(sb_bad, 4, 100, 10)
    cb_bad = capi.HostCigarBatch(**ct.records_to_arrays(bad_targets))
    ctx = capi.Context(flags=capi.FLAG_BASE_POS | capi.FLAG_BASE_SUPPORT, **opts)
    try:
        res = []
        for b in (cb, pb, pb):
            got = ctx.consensus_cigar_windows(b, wo)
            res.append((got, ctx.target_status.tolist(), ctx.base_support(), ctx.base_positions()))
        ctx.upload_cigar_windows(pb, wo); ctx.run(); ctx.sync()
        assert ctx.fetch() == exp
        for b in (cb_bad, cb_bad.packed()):
            with pytest.raises(capi.DagconError) as e:
                ctx.consensus_cigar_windows(b, wo)
            assert e.value.code == -4
            got = ctx.consensus_cigar_windows(b, wo, strict=False)
            assert ctx.target_status.tolist() == [-4 if f else 0 for f in failed]
            assert got == exp_bad and all(got[i] == [] for i, f in enumerate(failed) if f) and got[0] and got[3]
    finally:
        ctx.close()
    for got, status, sup, pos in res:
        assert got == exp and status == [0] * 6
        assert [[(w.tolist(), d.tolist()) for w, d in t] for t in sup] == [[(w.tolist(), d.tolist()) for w, d in t] for t in res[0][2]]
        assert [[p.tolist() for p in t] for t in pos] == [[p.tolist() for p in t] for t in res[0][3]]


@pytest.mark.gpu
def test_packed_record_past_q_bytes_is_refused_before_any_launch():
    """q_off + (q_len + 1) / 2 > q_bytes is DAGCON_ERR_INVALID_ARG for the call, with and without windows; a record
    that ends exactly at q_bytes is taken; the context stays usable."""
    from pbdagcon_amd import capi
    sb, cb, bad = _packed_case(141, True, False, 4, 150, 400, 8)
    pb = cb.packed()
    exp = oracle_batch(sb, 4, 60, 7)
    exp[bad] = []
    wo = capi.HostWindows.tiled(pb.tlen.tolist(), 1000, 0)
    last = pb.n_records - 1
    assert int(pb.q_off[last]) + (int(pb.q_len[last]) + 1) // 2 == pb.q_blob.size
    ctx = capi.Context(min_cov=4, min_len=60, trim=7)
    try:
        assert ctx.consensus_cigar(pb, strict=False) == exp
        launches = ctx.timings()
        for field, idx, val in (("q_off", 5, pb.q_blob.size), ("q_off", last, int(pb.q_off[last]) + 1),
                                ("q_len", 0, 2 * pb.q_blob.size + 1), ("q_len", last, int(pb.q_len[last]) + 2 - int(pb.q_len[last]) % 2)):
            twin = capi.HostCigarBatch(pb.tlen, pb.t_off, pb.t_blob, pb.rec_begin, pb.pos, pb.q_off.copy(), pb.q_len.copy(), pb.q_blob,
                                       pb.op_begin, pb.ops)
            twin.is_packed = True
            getattr(twin, field)[idx] = val
            for call in (lambda: ctx.consensus_cigar(twin, strict=False), lambda: ctx.consensus_cigar_windows(twin, wo, strict=False),
                         lambda: ctx.upload_cigar(twin)):
                with pytest.raises(capi.DagconError) as e:
                    call()
                assert e.value.code == -1, (field, idx)
        # an odd record may end in the middle of the last byte: one base more still fits it, and is non-conforming, not refused
        if int(pb.q_len[last]) % 2:
            twin = capi.HostCigarBatch(pb.tlen, pb.t_off, pb.t_blob, pb.rec_begin, pb.pos, pb.q_off, pb.q_len.copy(), pb.q_blob,
                                       pb.op_begin, pb.ops)
            twin.is_packed = True
            twin.q_len[last] += 1
            ctx.consensus_cigar(twin, strict=False)
            assert ctx.target_status.tolist()[bad] == -4
        assert ctx.consensus_cigar(pb, strict=False) == exp
        assert ctx.consensus_cigar_windows(pb, wo, strict=False) == exp
        assert launches is not None
    finally:
        ctx.close()


def mapped_reads(rng, bb, n_reads, read_len):
    """Records along a contig for the command line: upper-case ACGT reads with errors, POS ascending."""
    tlen = len(bb)
    out = []
    for s in sorted(rng.integers(0, max(1, tlen - read_len // 2), n_reads).tolist()):
        e = min(tlen, s + read_len)
        q, t = bytearray(), bytearray()
        for i in range(s, e):
            u = rng.random()
            if u < 0.03:
                q.append(ct.GAP); t.append(bb[i])
            elif u < 0.05:
                q.append(b"ACGT"[int(rng.integers(0, 4))]); t.append(bb[i])
            else:
                q.append(bb[i]); t.append(bb[i])
            if rng.random() < 0.04:
                q.append(b"ACGT"[int(rng.integers(0, 4))]); t.append(ct.GAP)
        out.append(ct.compress(s + 1, bytes(q), bytes(t), bb, eqx=bool(len(out) % 2)))
    return out


@pytest.mark.gpu
def test_pbdagcon_bam_equals_sam(tmp_path):
    """pbdagcon --bam prints, byte for byte, what pbdagcon --sam prints for the same records: plain, --fastq,
    --window W --overlap O in several groups (--batch-targets 2), several batches on two contexts, -j 1 against -j 4,
    and from stdin."""
    rng = np.random.default_rng(301)
    refs, seqs, records = [], [], []
    for g, (tl, n, rl) in enumerate(((6000, 260, 900), (1500, 40, 1500), (2500, 90, 800), (900, 3, 500), (1800, 50, 1200))):
        bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl))
        refs.append(("ctg%d|x" % g, tl)); seqs.append(bb)
        for k, r in enumerate(mapped_reads(rng, bb, n, rl)):
            p, q, ops = _clip(rng, *r, odd=bool(k % 2)) if k % 3 else r
            records.append(_rec("r%d_%d" % (g, k), 16 if k % 5 == 0 else 0, g, p, ops, q))
        records.append(_rec("u%d" % g, 4, -1, 0, [], b"ACGT"))
    ref = tmp_path / "ref.fa"
    ref.write_bytes(ct.to_fasta([n + " description" for n, _ in refs], seqs))
    sam = tmp_path / "in.sam"
    sam.write_bytes(bf.sam_text(refs, records))
    bam = tmp_path / "in.bam"
    blob = bf.bgzf(bf.bam_bytes(refs, records), 6, payload=30011)
    bam.write_bytes(blob)
    assert len(bf.members(blob)) > 8

    def run(*args, stdin=None):
        out = _run(*args, stdin=stdin)
        assert out.returncode == 0, out.stderr.decode()
        return out.stdout
    for mode in ([], ["--fastq"], ["--window", "1000", "--overlap", "200", "--batch-targets", "2"],
                 ["--window", "1000", "--overlap", "200", "--batch-targets", "2", "--fastq"]):
        opts = ["--ref", str(ref), "-m", "300", *mode]
        want = run("--sam", *opts, str(sam))
        assert want.count(b"\n") >= (8 if "--fastq" not in mode else 16), want[:200]
        assert run("--bam", *opts, "-j", "1", str(bam)) == want
        assert run("--bam", *opts, "-j", "4", str(bam)) == want
        if "--window" not in mode:
            assert run("--bam", *opts, "--batch-targets", "2", "--contexts", "2", "-j", "3", str(bam)) == want
    assert run("--bam", "--ref", str(ref), "-m", "300", "-", stdin=blob) == run("--sam", "--ref", str(ref), "-m", "300", str(sam))
