"""pbdagcon --fastq and dazcon --fastq: the records of the FASTA run ('@' for '>'), byte for byte, with qualities from
the per-base support of the CPU twin (tests/support_twin.py); the quality's integer definition against exact
arithmetic; the flag on the command lines."""
import os
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

import support_twin as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
DAZCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "dazcon")
LIMIT = 4096


# ---- CPU ---------------------------------------------------------------------------------------------------------

def _reference_table(cmax):
    """Q[c][x - 1] = floor(10 log10((c + 2) / x)) for x = 1 .. c + 1, from thresholds computed in 60-digit decimals:
    Q >= q iff x <= (c + 2) / 10^(q / 10); the threshold is an integer only for q a multiple of 10, where it is exact."""
    getcontext().prec = 60
    scale = [Decimal(10) ** (Decimal(-q) / 10) for q in range(1, 40)]
    out = []
    for c in range(cmax + 1):
        xs = np.arange(1, c + 2, dtype=np.int64)
        q = np.zeros(xs.size, np.int64)
        for k, f in enumerate(scale, start=1):
            if k % 10 == 0:
                q += xs * (10 ** (k // 10)) <= c + 2                  # (an integer power of ten: exact)
            else:
                q += xs <= int((c + 2) * f)                           # (irrational: x <= th iff x <= floor(th))
        out.append(q)
    return out


def test_quality_formula_is_exact():
    """support_twin.quality and pbdagcon_amd/csrc/host/fastq.h against floor(10 log10((c + 2) / x)) in exact
    arithmetic, for every (weight, depth) up to 4,096: c = max(depth, weight) and x = c - weight + 1 take every value
    with 1 <= x <= c + 1 (weight <= depth), and x = 1 for every weight above its depth."""
    ref = _reference_table(LIMIT)
    for c in (0, 1, 2, 7, 8, 97, 998, 1000, 2047, 4094, 4095, LIMIT):
        got = [st.quality(c - x + 1, c) for x in range(1, c + 2)]
        assert got == ref[c].tolist(), c
        assert st.quality(c, 0) == ref[c][0]                         # weight above depth: c = weight, x = 1
    assert max(int(r.max()) for r in ref) == 36
    # the C++ of the command lines, every (c, x) of the range
    import tempfile
    prog = r'''
#include <cstdio>
#include "fastq.h"
int main() {
    for (unsigned c = 0; c <= %d; c++) {
        for (unsigned x = 1; x <= c + 1; x++) putchar(33 + dg_quality(c - x + 1, c));
        if (dg_quality(c, 0) != dg_quality(c, c)) return 1;
    }
    return dg_quality(5600, 5600) == 37 && dg_quality(5601, 5601) == -1 ? 0 : 2;
}''' % LIMIT
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "q.cpp"), "w").write(prog)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                               "-o", os.path.join(d, "q"), os.path.join(d, "q.cpp")])
        out = subprocess.run([os.path.join(d, "q")], capture_output=True, timeout=300)
    assert out.returncode == 0
    exp = b"".join(bytes((33 + r).astype(np.uint8)) for r in ref)
    assert out.stdout == exp
    # the twin's quality string and record layout
    assert st.quality_string([6, 3, 0], [6, 6, 6]) == bytes([33 + 9, 33 + 3, 33 + 0])
    assert st.fastq_record(b"t/0_3", b"ACG", [6, 3, 0], [6, 6, 6]) == b"@t/0_3\nACG\n+\n*$!\n"


def _cli(path):
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return path


def test_fastq_flag_parses_and_is_listed(tmp_path):
    """--fastq is in both --help texts with its quality definition, and parses (parser-only test hooks, no GPU)."""
    for cli in (PBDAGCON, DAZCON):
        h = subprocess.run([_cli(cli), "--help"], capture_output=True, text=True)
        assert h.returncode == 0 and "--fastq" in h.stdout and "Laplace" in h.stdout and "log10" in h.stdout
    from pbdagcon_amd import synth
    m5 = tmp_path / "in.m5"
    m5.write_bytes(synth.to_m5(synth.make_batch(2, 600, 6, seed=4)))
    a = subprocess.run([PBDAGCON, "--fastq", "--dump-parsed", str(m5)], capture_output=True)
    b = subprocess.run([PBDAGCON, "--dump-parsed", str(m5)], capture_output=True)
    assert a.returncode == 0 and a.stdout == b.stdout
    assert subprocess.run([PBDAGCON, "--fastqq", str(m5)], capture_output=True).returncode == 2
    s, o = tmp_path / "r.txt", tmp_path / "o.txt"
    s.write_text("1 " + "ACGT" * 100 + "\n2 " + "ACGT" * 100 + "\n")
    o.write_text("O 1 2 0 0 300 0 300 10 A A\n")
    a = subprocess.run([DAZCON, "-a", str(o), "-s", str(s), "--fastq", "--dump-hits", "-c", "0"], capture_output=True)
    b = subprocess.run([DAZCON, "-a", str(o), "-s", str(s), "--dump-hits", "-c", "0"], capture_output=True)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _fasta_records(out):
    lines = out.split(b"\n")
    assert lines[-1] == b""
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 2)]


def _check_fastq(fasta, fastq, supports):
    """fastq == the FASTA run's records with '@' and the qualities of `supports` ([(weights, depths)] per record)."""
    recs = _fasta_records(fasta)
    assert fasta.startswith(b">") and len(recs) == len(supports) and recs
    exp = b"".join(st.fastq_record(name, seq, w, d) for (name, seq), (w, d) in zip(recs, supports))
    assert fastq == exp


def _run(cli, args, **kw):
    out = subprocess.run([cli, *args], capture_output=True, timeout=600, **kw)
    assert out.returncode == 0, out.stderr.decode()
    return out.stdout


class _Record:
    """oracle.consensus_target that keeps the twin's support of every call (for the compositions of other tests)."""

    def __init__(self):
        self.calls = []

    def __call__(self, tlen, alns, min_len=500, trim=50, min_weight=6, backbone=None):
        segs = st.consensus_target_support(tlen, alns, min_len, trim, min_weight, backbone)
        self.calls.append(segs)
        return [s[:3] for s in segs]


@pytest.mark.gpu
def test_pbdagcon_fastq_m5(tmp_path):
    """The input of test_cli_end_to_end (a group below -c, '-' strand records): --fastq against the FASTA run and the
    twin; and with --contexts 2 and small --batch-targets, and --slab-bytes, the same bytes."""
    from pbdagcon_amd import synth
    batch = synth.make_batch(5, 1500, 12, seed=31)
    lines = synth.to_m5(batch).decode().splitlines()
    keep = [ln for i, ln in enumerate(lines) if not (24 <= i < 33)]
    path = tmp_path / "in.m5"
    path.write_bytes(("\n".join(keep) + "\n").encode())
    fasta = _run(PBDAGCON, ["-c", "6", "-m", "500", "-t", "50", "-j", "1", str(path)])
    fastq = _run(PBDAGCON, ["-c", "6", "-m", "500", "-t", "50", "-j", "1", "--fastq", str(path)])
    sup = []
    for t in range(batch.n_targets):
        alns = [a for i, a in enumerate(batch.target_alignments(t)) if not (24 <= 12 * t + i < 33)]
        if len(alns) < 6:
            continue
        sup += [(w, d) for _, _, _, w, d in st.consensus_target_support(int(batch.tlen[t]), alns, 500, 50, 6)]
    _check_fastq(fasta, fastq, sup)
    assert fastq.count(b"\n@") + 1 == 4
    for extra in (["--contexts", "2", "--batch-targets", "1"], ["--contexts", "2", "--batch-targets", "2", "-j", "3",
                                                                 "--slab-bytes", "20000"]):
        assert _run(PBDAGCON, ["--fastq", *extra, str(path)]) == fastq


@pytest.mark.gpu
@pytest.mark.parametrize("local", [False, True])
def test_pbdagcon_fastq_pre(tmp_path, monkeypatch, local):
    """-a (both strands) and -a --local, on the records and CPU compositions of test_cli_pre_input_with_align and
    test_cli_pre_local."""
    import oracle
    import test_align_local as tal
    rec = _Record()
    monkeypatch.setattr(oracle, "consensus_target", rec)
    if local:
        targets = tal._flanked_records(np.random.default_rng(64), n_targets=4, small=2)
        tal._expected_pre(oracle, targets)
    else:
        from test_gpu_parity import _mutate
        rng = np.random.default_rng(8)
        rc = bytes.maketrans(b"ACGT", b"TGCA")
        targets = []
        for ti in range(4):
            tlen = int(rng.integers(1500, 2500))
            target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
            recs = []
            for r in range(10 if ti != 2 else 3):
                s = int(rng.integers(0, tlen // 4)); e = int(rng.integers(3 * tlen // 4, tlen + 1))
                strand = b"+-"[r % 2:r % 2 + 1]
                tseq = target[s:e] if strand == b"+" else target[s:e].translate(rc)[::-1]
                qseq = _mutate(rng, tseq)
                recs.append((s if strand == b"+" else tlen - e, strand, qseq, tseq))
            targets.append((tlen, recs))
        for tlen, recs in targets:
            if len(recs) >= 6:
                alns = []
                for ts, sd, q, t in recs:
                    st_, _, qa, ta = oracle.simple_align(ts, tlen, sd, q, t)
                    alns.append((st_, qa, ta))
                oracle.consensus_target(tlen, alns, 500, 50, 6)
    lines = []
    for ti, (tlen, recs) in enumerate(targets):
        for r, (tstart, strand, qseq, tseq) in enumerate(recs):
            lines.append(b" ".join([b"q%d_%d" % (ti, r), b"t%d" % ti, strand, b"%d" % tlen, b"%d" % tstart,
                                    b"%d" % (tstart + len(tseq)), qseq, tseq]))
    path = tmp_path / "in.pre"
    path.write_bytes(b"\n".join(lines) + b"\n")
    args = ["-a"] + (["--local"] if local else []) + ["-j", "2"]
    fasta = _run(PBDAGCON, args + [str(path)])
    fastq = _run(PBDAGCON, args + ["--fastq", str(path)])
    sup = [(w, d) for segs in rec.calls for _, _, _, w, d in segs]
    _check_fastq(fasta, fastq, sup)
    assert [s for _, s in _fasta_records(fasta)] == [s for segs in rec.calls for _, _, s, _, _ in segs]


@pytest.mark.gpu
def test_pbdagcon_fastq_polish(tmp_path, monkeypatch):
    """-a --polish N: the qualities are the last round's, from the oracle graph of the CPU composition of
    test_cli_polish_rounds."""
    import oracle
    from test_gpu_parity import _mutate, _polish_twin
    rng = np.random.default_rng(21)
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    trim, min_cov, min_len = 20, 6, 500
    lines, targets = [], []
    for ti in range(3):
        truth = bytes(b"ACGT"[j] for j in rng.integers(0, 4, int(rng.integers(1500, 2000))))
        backbone = _mutate(rng, truth, sub=0.04, ins=0.06, dele=0.06)
        tlen = len(backbone)
        recs = []
        for r in range(24):
            s = 0 if r % 3 else int(rng.integers(0, tlen // 5))
            e = tlen if r % 3 else int(rng.integers(4 * tlen // 5, tlen + 1))
            ts, te = int(s * len(truth) / tlen), int(e * len(truth) / tlen)
            strand = b"+-"[r % 2:r % 2 + 1]
            q_fwd = _mutate(rng, truth[ts:te], sub=0.03, ins=0.07, dele=0.05)
            tseq_fwd = backbone[s:e]
            qseq = q_fwd if strand == b"+" else q_fwd.translate(rc)[::-1]
            tseq = tseq_fwd if strand == b"+" else tseq_fwd.translate(rc)[::-1]
            tstart = s if strand == b"+" else tlen - e
            lines.append(b" ".join([b"q%d_%d" % (ti, r), b"t%d" % ti, strand, b"%d" % tlen, b"%d" % tstart,
                                    b"%d" % (tstart + len(tseq)), qseq, tseq]))
            recs.append((tstart, strand, qseq, tseq, q_fwd))
        targets.append((tlen, recs))
    path = tmp_path / "in.pre"
    path.write_bytes(b"\n".join(lines) + b"\n")
    for rounds in (1, 2):
        sup = []
        for tlen, recs in targets:
            rec = _Record()
            monkeypatch.setattr(oracle, "consensus_target", rec)
            segs = _polish_twin(tlen, recs, rounds, trim, min_cov, min_len)
            monkeypatch.undo()
            assert segs and [s[:3] for s in rec.calls[-1]] == segs
            sup += [(w, d) for _, _, _, w, d in rec.calls[-1]]
        args = ["-a", "-t", str(trim), "--polish", str(rounds)]
        fasta = _run(PBDAGCON, args + [str(path)])
        fastq = _run(PBDAGCON, args + ["--fastq", str(path)])
        _check_fastq(fasta, fastq, sup)


@pytest.mark.gpu
def test_dazcon_fastq_text(tmp_path):
    """dazcon --fastq on the text input of test_dazcon_end_to_end: %d/%d/%d_%d names, real backbones."""
    import daz_model as dm
    rng = np.random.default_rng(3)
    reads, lines, model = dm.synth_dataset(rng, n_targets=4, tlen=(1500, 2600), n_b=(8, 14))
    s, a = tmp_path / "reads.txt", tmp_path / "ovl.txt"
    s.write_text("".join(f"{i} {seq}\n" for i, seq in sorted(reads.items())))
    a.write_text("\n".join(lines) + "\n")
    args = ["-s", str(s), "-a", str(a), "--batch-targets", "3"]
    fasta = _run(DAZCON, args)
    fastq = _run(DAZCON, args + ["--fastq"])
    sup = []
    for aid, recs in model.items():
        hits = dm.sort_hits(dm.group_hits(recs, len(reads[aid]), {r["bread"]: len(reads[r["bread"] + 1]) for r in recs}),
                            len(reads[aid]), False)
        alns = [(r["abpos"] + 1, r["qstr"].encode(), r["tstr"].encode()) for h in hits for r in h.records]
        sup += [(w, d) for _, _, _, w, d in st.consensus_target_support(len(reads[aid]), alns, 500, 10, 6,
                                                                          backbone=reads[aid].encode())]
    _check_fastq(fasta, fastq, sup)


@pytest.mark.gpu
def test_dazcon_fastq_las_db(tmp_path):
    """dazcon --fastq on the .las / .db input of test_dazcon_on_las_and_db."""
    import daz_model as dm
    import oracle
    from test_dazcon import _las_case
    rng = np.random.default_rng(17)
    reads, ovl, db, las = _las_case(tmp_path, rng, n_targets=4, cov=12, tlen=2500)
    args = ["-a", las, "-s", db, "-c", "4", "-l", "500"]
    fasta = _run(DAZCON, args)
    fastq = _run(DAZCON, args + ["--fastq"])
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    by_a, sup = {}, []
    for o in ovl:
        by_a.setdefault(o["aread"], []).append(o)
    for ai in sorted(by_a):
        a = reads[ai].encode()
        hits = dm.sort_hits(dm.group_hits(by_a[ai], len(a), {o["bread"]: len(reads[o["bread"]]) for o in by_a[ai]}),
                            len(a), False)[:85]
        alns = []
        for h in hits:
            for r in h.records:
                b = reads[r["bread"]].encode()
                if r["flags"] & 1:
                    b = b.translate(rc)[::-1]
                qa, ta = oracle.banded_align(b[r["bbpos"]:r["bepos"]], a[r["abpos"]:r["aepos"]])
                alns.append((r["abpos"] + 1, qa, ta))
        if len(alns) < 4:
            continue
        sup += [(w, d) for _, _, _, w, d in st.consensus_target_support(len(a), alns, 500, 10, 4, backbone=a)]
    _check_fastq(fasta, fastq, sup)
