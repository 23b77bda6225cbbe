"""pbdagcon's input modes side by side: .m5, .pre (-a), --sam, --bam, --paf and --paf --cs from one set of alignments.
The per-format suites pin each format's parser and its errors; this pins what the command line's stages share between
the modes: that threads, slabs and batch sizes change no byte of what is parsed or printed, and what -v says about
skipped records, word for word."""
import os
import subprocess

import numpy as np
import pytest

import bam_files as bf
import cigar_twin as ct
import cs_files as cf
import paf_files as pf
from util import random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
NOGPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
RC = bytes.maketrans(b"ACGT", b"TGCA")
MODES = ("m5", "pre", "sam", "bam", "paf", "cs")
# stderr of --dump-parsed -v on the inputs below, as the command line printed it before its stages were split
SKIPPED = {
    "m5": b"", "pre": b"",
    "sam": b"pbdagcon: 2 SAM records skipped (FLAG 0x4 or 0x100, or RNAME, CIGAR or SEQ '*')\n",
    "bam": b"pbdagcon: 5 BAM records skipped (FLAG 0x4 or 0x100, refID < 0, no CIGAR or no SEQ)\n",
    "paf": b"pbdagcon: 1 PAF lines skipped (tp:A:S)\n",
    "cs": b"pbdagcon: 1 PAF lines skipped (tp:A:S)\n",
}


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


def _write_inputs(d, n_targets, tlen, reads, seed, full_span):
    """The same random_target pileups as .m5 and .pre text (both strands), SAM and BAM (two more records that are flagged
    out, BAM with an unmapped record per target besides), and PAF with cg:Z: and cs:Z: on every line (lines shuffled across
    targets, one of them repeated as tp:A:S).  Returns {mode: (flags, path)}."""
    rng = np.random.default_rng(seed)
    names = ["ctg%d|x" % g for g in range(n_targets)]
    targets = []
    for g in range(n_targets):
        alns, bb = random_target(rng, tlen + 7 * g, reads, full_span=full_span)
        targets.append((len(bb), sorted(alns, key=lambda a: a[0]), bb))
    m5, pre = [], []
    for g, (tl, alns, bb) in enumerate(targets):
        for k, (s, q, t) in enumerate(alns):
            rev = k % 3 == 1
            qq, tt = (q.translate(RC)[::-1], t.translate(RC)[::-1]) if rev else (q, t)
            qs, ts = qq.replace(b"-", b""), tt.replace(b"-", b"")
            m5.append("q%d_%d %d 0 %d + %s %d %d %d %s -1000 0 0 0 0 254 %s %s %s" % (
                g, k, len(qs), len(qs), names[g], tl, s - 1, s - 1 + len(ts), "-" if rev else "+", qq.decode(),
                "".join("|" if a == b else "*" for a, b in zip(qq, tt)), tt.decode()))
            t0 = tl - (s - 1 + len(ts)) if rev else s - 1          # (m4topre.py:194-206: the read's orientation)
            pre.append("q%d_%d %s %s %d %d %d %s %s" % (g, k, names[g], "-" if rev else "+", tl, t0, t0 + len(ts), qs.decode(), ts.decode()))
    recs = [sorted((ct.compress(s, q, t, bb, eqx=bool(g % 2)) for s, q, t in alns), key=lambda r: r[0])
            for g, (tl, alns, bb) in enumerate(targets)]
    # SAM and BAM: a copy of a record behind it in targets 0 and 1, flagged out, so that every mode keeps the same alignments
    srecs = [list(rs) for rs in recs]
    srecs[0].insert(3, srecs[0][2]); srecs[1].insert(2, srecs[1][1])
    flags = [16 if i % 4 == 1 else 0 for i in range(n_targets * reads + 2)]
    flags[3], flags[reads + 1 + 2] = 4, 0x100
    refs = [(n, tl) for n, (tl, _, _) in zip(names, targets)]
    brecs, i = [], 0
    for g, rs in enumerate(srecs):
        for k, (p, q, ops) in enumerate(rs):
            brecs.append(dict(qname="q%d_%d" % (g, k), flag=flags[i], ref=g, pos=p, ops=[int(o) for o in ops], seq=q))
            i += 1
        brecs.append(dict(qname="u%d" % g, flag=4, ref=-1, pos=0, ops=[], seq=b"ACGT"))
    rd, alns = pf.from_twin(rng, names, [(bb, rs) for (_, _, bb), rs in zip(targets, recs)], alphabet=b"ACGTN", shared=0, sort_pos=True)
    alns = cf.with_cs(rd, alns, {n: bb for n, (_, _, bb) in zip(names, targets)})
    per = [[x for x in alns if x["tname"] == n] for n in names]
    lines = [per[g].pop(0) for g in rng.permutation(np.repeat(np.arange(n_targets), [len(p) for p in per])).tolist()]
    lines.insert(2, dict(lines[0], tp="S"))
    files = {
        "in.m5": ("\n".join(m5) + "\n").encode(), "in.pre": ("\n".join(pre) + "\n").encode(),
        "ref.fa": ct.to_fasta([n + " some description" for n in names], [bb for _, _, bb in targets]),
        "in.sam": ct.to_sam(names, [tl for tl, _, _ in targets], srecs, flags=flags),
        "in.bam": bf.bgzf(bf.bam_bytes(refs, brecs), 6, payload=3001),
        "reads.fa": pf.reads_fasta(rd), "in.paf": cf.paf_text(rd, lines),
    }
    for name, data in files.items():
        (d / name).write_bytes(data)
    ref = ["--ref", str(d / "ref.fa")]
    return {"m5": ([], str(d / "in.m5")), "pre": (["-a"], str(d / "in.pre")), "sam": (["--sam", *ref], str(d / "in.sam")),
            "bam": (["--bam", *ref], str(d / "in.bam")), "paf": (["--paf", *ref, "--reads", str(d / "reads.fa")], str(d / "in.paf")),
            "cs": (["--paf", "--cs", *ref], str(d / "in.paf"))}


@pytest.fixture(scope="module")
def small_inputs(tmp_path_factory):
    return _write_inputs(tmp_path_factory.mktemp("cli_modes_small"), 3, 150, 5, 7, False)


@pytest.fixture(scope="module")
def gpu_inputs(tmp_path_factory):
    return _write_inputs(tmp_path_factory.mktemp("cli_modes_gpu"), 4, 800, 8, 11, True)


@pytest.mark.parametrize("mode", MODES)
def test_dump_is_the_same_on_one_thread_and_on_five_with_small_slabs(small_inputs, mode):
    """--dump-parsed -v of a three-target input: -j 1 and -j 5 --slab-bytes 300 --batch-targets 1 print the same stdout,
    a line for each of the 15 alignments, and stderr is the mode's 'skipped' line and nothing else."""
    flags, path = small_inputs[mode]
    outs = []
    for extra in (["-j", "1"], ["-j", "5", "--slab-bytes", "300", "--batch-targets", "1"]):
        out = subprocess.run([_cli(), *flags, "--dump-parsed", "-v", *extra, path], capture_output=True, env=NOGPU, timeout=120)
        assert out.returncode == 0, out.stderr.decode()
        assert out.stderr == SKIPPED[mode]
        outs.append(out.stdout)
    assert outs[0] == outs[1]
    assert outs[0].count(b"\n") == 15
    assert {ln.split(b"\t")[0] for ln in outs[0].splitlines()} == {b"ctg0|x", b"ctg1|x", b"ctg2|x"}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_output_is_the_same_in_one_batch_and_in_four_on_two_contexts(gpu_inputs, mode):
    """4 targets x 800 bases x 8 reads, -m 200: the default settings and --batch-targets 1 --contexts 2 -j 3 print the
    same bytes, a record for every target, and stderr carries no warning."""
    flags, path = gpu_inputs[mode]
    outs = []
    for extra in ([], ["--batch-targets", "1", "--contexts", "2", "-j", "3"]):
        out = subprocess.run([_cli(), *flags, "-m", "200", *extra, path], capture_output=True, timeout=300)
        assert out.returncode == 0, out.stderr.decode()
        assert b"warning" not in out.stderr, out.stderr.decode()
        outs.append(out.stdout)
    assert outs[0] == outs[1]
    assert {ln.split(b"/")[0] for ln in outs[0].splitlines() if ln.startswith(b">")} == {b">ctg%d|x" % g for g in range(4)}
