"""dagcon_set_edit_support / dagcon_fetch_edit_support (include/dagcon.h, csrc/k_evidence.hip.h) and pbdagcon --vcf: the
alignments behind each edit.  CPU: the rule by hand on the twin (tests/evidence_twin.py), its invariants on random
pile-ups, the binding, the usage errors, csrc/host/vcf.h against a Python formatter.  GPU: the device's five arrays equal
the twin's field for field -- once with the oracle's edits, once with the twin fed the device's own edit arrays -- and
the consensus and the edit arrays do not change with the switch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import edits_twin as et
import evidence_twin as ev
import md_files as mf
import md_twin as mt
import paf_files as pf
import window_twin as wt
from util import random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
STATE, NONCONFORMING = -8, -4


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


# ---- CPU: the rule by hand -------------------------------------------------------------------------------------------

def _count(T, S, edits, cols, extend=True, t0=0, t1=None):
    """Per group of one segment (gL, gR, ref allele, alt allele, [class of each alignment]); cols = [(s0, q, t)] as they
    are, nothing normalised."""
    out = []
    for first, end, gL, gR, cL, cR in ev.segment_groups(T, S, t0, len(T) if t1 is None else t1, edits, extend):
        out.append((gL, gR, T[gL:gR], S[cL:cR], [ev.classify(len(T), s0, q, t, gL, gR, T[gL:gR], S[cL:cR]) for s0, q, t in cols]))
    return out


def test_homopolymer_insertion_is_alt_only_with_the_extension():
    #     01234567
    T = b"CGAAAATC"
    S = b"CGAAAAATC"
    edits = [(6, 0, 6, 1)]                                       # the inserted A stands at the run's right end
    left = (0, b"CGAAAAATC", b"CG-AAAATC")                       # a read writes it at the run's left end
    plain = (0, b"CGAAAATC", b"CGAAAATC")
    (g,) = _count(T, S, edits, [left, plain])
    assert g == (2, 6, b"AAAA", b"AAAAA", ["alt", "ref"])
    (g,) = _count(T, S, edits, [left, plain], extend=False)
    assert g == (6, 6, b"", b"A", ["ref", "ref"])                # no window: the read's base is not seen at all


def test_dinucleotide_repeat():
    #     01234567
    T = b"GACACACT"
    S = b"GACACT"
    edits = [(1, 2, 1, 0)]                                       # AC dropped, written at the repeat's left end
    mid = (0, b"GAC--ACT", T)
    right = (0, b"GACAC--T", T)
    none = (0, T, T)
    odd = (0, b"GACA--CT", T)                                    # CA dropped: the same bytes again
    one = (0, b"GACAC-CT", T)                                    # one base dropped: neither allele
    (g,) = _count(T, S, edits, [mid, right, none, odd, one])
    assert g == (1, 7, b"ACACAC", b"ACAC", ["alt", "alt", "ref", "alt", "other"])


def test_substitution_and_a_mismatching_flank():
    T = b"ACGTAC"
    S = b"ACTTAC"
    edits = [(2, 1, 2, 1)]
    cols = [(0, S, T), (0, T, T), (0, b"ACCTAC", T), (0, b"AGTTAC", T), (0, b"ACT-AC", T), (1, b"CTTAC", T[1:]), (2, b"TTAC", T[2:]),
            (0, b"ACTT", T[:4]), (0, b"ACT", T[:3])]
    (g,) = _count(T, S, edits, cols)
    # alt, ref, a third base, a wrong left flank, a missing right flank, a read that begins at the flank, and reads that
    # begin or end inside: the last three do not span
    assert g == (2, 3, b"G", b"T", ["alt", "ref", "other", "other", "other", "alt", None, "alt", None])


def test_two_touching_edits_are_one_group():
    #     01234
    T = b"GCAAT"
    S = b"GTAAAT"
    edits = [(1, 1, 1, 1), (4, 0, 4, 1)]                         # C -> T, and an A more in the run behind it
    both = (0, b"GTAAAT", b"GCAA-T")
    sub_only = (0, b"GTAAT", T)
    none = (0, T, T)
    (g,) = _count(T, S, edits, [both, sub_only, none])
    assert g == (1, 4, b"CAA", b"TAAA", ["alt", "other", "ref"])
    # without the extension the insertion's window is [4, 4): the two do not touch
    assert [x[:2] for x in _count(T, S, edits, [both], extend=False)] == [(1, 2), (4, 4)]


def test_edits_at_position_0_and_at_tlen():
    T = b"ACGT"
    S = b"GACGTT"
    edits = [(0, 0, 0, 1), (4, 0, 5, 1)]
    full = (0, b"GACGTT", b"-ACGT-")
    bare = (0, T, T)
    late = (1, b"CGTT", b"CGT-")                                 # begins at base 1: cannot say anything about base 0
    early = (0, b"GACG", b"-ACG")
    a, b = _count(T, S, edits, [full, bare, late, early])
    assert a == (0, 0, b"", b"G", ["alt", "ref", None, "alt"])
    assert b == (3, 4, b"T", b"TT", ["alt", "ref", "alt", None])


def test_case_only_edit_alt_is_tested_first():
    T = b"ACgTA"
    S = b"ACGTA"
    edits = [(2, 1, 2, 1)]
    (g,) = _count(T, S, edits, [(0, S, T), (0, T, T), (0, b"ACTTA", T)])
    assert g == (2, 3, b"g", b"G", ["alt", "alt", "other"])


def test_target_support_normalises_and_carries_group_values(oracle_lib):
    """target_support itself: the alignments go through normalize_gaps / trim_aln, alignments below min_len are not
    counted, and every edit of a group carries the group's values."""
    T = b"GCAAT" + b"CGTACGTAGC"
    S = b"GTAAAT" + b"CGTACGTAGC"
    edits = [(1, 1, 1, 1), (4, 0, 4, 1)]
    alns = [(1, S, b"GCAA-T" + T[5:]), (1, S, b"GCA-AT" + T[5:]), (1, T, T), (1, b"GC", b"GC")]
    (per,) = ev.target_support(T, alns, [(S, 0, len(T), edits)], 4, 0)
    assert per == [(1, 4, 3, 2, 1), (1, 4, 3, 2, 1)]


def _small_pileup(rng, k):
    tlen = int(rng.integers(8, 70))
    alns, bb = random_target(rng, tlen, int(rng.integers(3, 8)), alphabet=b"AC" if k % 3 == 0 else b"ACGT",
                             sub=0.06, ins=0.12, dele=0.08, full_span=bool(k % 2))
    return alns, bb


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    rng = np.random.default_rng(77)
    n_edits = n_ext = n_multi = n_edge = 0
    for k in range(1500):
        alns, bb = _small_pileup(rng, k)
        trim = int(rng.integers(0, 3))
        (segs,) = et.batch_edits([(bb, alns)], 3, 4, trim)
        if not segs:
            continue
        sup = ev.target_support(bb, alns, segs, 4, trim)
        n_aln = len(ev.columns(alns, 4, trim))
        for (S, t0, t1, edits), per in zip(segs, sup):
            plain = ev.edit_windows(bb, S, t0, t1, edits, extend=False)
            n_ext += sum(1 for a, b in zip(plain, ev.edit_windows(bb, S, t0, t1, edits)) if a != b)
            groups = ev.segment_groups(bb, S, t0, t1, edits)
            assert all(a[3] < b[2] for a, b in zip(groups, groups[1:]))         # at least one base between two groups
            for first, end, gL, gR, cL, cR in groups:
                assert t0 <= gL <= gR <= t1
                if ev.sim_bytes(bb[gL:gR], S[cL:cR]):                           # only a case-only change may look alike
                    assert all(tl == cl and ev.sim_bytes(bb[tp:tp + tl], S[c:c + cl]) for tp, tl, c, cl in edits[first:end])
                n_multi += end - first >= 2
                n_edge += gL == 0 or gR == len(bb)
                assert all(per[i] == per[first] for i in range(first, end))
            for w0, w1, span, alt, ref in per:
                assert alt + ref <= span <= n_aln
            n_edits += len(edits)
    print("edits %d, extended windows %d, groups of two or more %d, at an edge %d" % (n_edits, n_ext, n_multi, n_edge))
    assert n_edits >= 1000 and n_ext >= 500 and n_multi >= 30 and n_edge >= 10


def test_binding_exports_and_struct_size():
    from pbdagcon_amd import capi
    assert "dagcon_set_edit_support" in capi.EXPORTS and "dagcon_fetch_edit_support" in capi.EXPORTS
    lib = capi.load()
    assert hasattr(lib, "dagcon_set_edit_support") and hasattr(lib, "dagcon_fetch_edit_support")
    prog = '#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu\\n", sizeof(dagcon_edit_support)); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert ctypes.sizeof(capi.EditSupport) == int(out[0])
    assert callable(capi.Context.set_edit_support) and callable(capi.Context.edit_support)


def test_vcf_usage_errors(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    vcf = tmp_path / "o.vcf"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for args in (["--vcf", str(vcf), str(m5)], ["-a", "--vcf", str(vcf), str(m5)], [str(m5), "--vcf"],
                 rec + ["--dump-parsed", "--vcf", str(vcf), str(sam)],
                 rec + ["--window", "100", "--overlap", "70", "--vcf", str(vcf), str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not vcf.exists()
    # a file that cannot be written is said before anything runs
    out = run(*rec, "--vcf", str(tmp_path / "no_such_dir" / "o.vcf"), str(sam))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0 and b"--vcf FILE" in h.stdout
    assert b"parity unpinned" in h.stdout.split(b"\n  --vcf FILE")[1].split(b"\n  --fastq")[0]


_VCF_MAIN = r"""
#include <iostream>
#include "vcf.h"
// stdin: "name target t_pos t_len alt span ref alt gL gR" per line ('-' for an empty alt); stdout: the header, then the lines
int main() {
    std::string out, name, target, alt;
    uint32_t tp, tl, sp, nr, na, gl, gr;
    dg_vcf_header(out); dg_vcf_contig(out, "ctg", 12345); dg_vcf_columns(out);
    while (std::cin >> name >> target >> tp >> tl >> alt >> sp >> nr >> na >> gl >> gr) {
        if (alt == "-") alt.clear();
        dg_vcf_line(out, name, target.data(), (uint32_t)target.size(), tp, tl, alt.data(), (uint32_t)alt.size(), sp, nr, na, gl, gr);
    }
    std::cout << out;
    return 0;
}
"""


def _vcf_line(name, T, tp, tl, alt, span, n_ref, n_alt, gL, gR):
    """The anchoring rule of pbdagcon --vcf, in Python."""
    ref, pos = T[tp:tp + tl], tp + 1
    if not tl or not alt:
        if tp > 0:
            ref, alt, pos = T[tp - 1:tp] + ref, T[tp - 1:tp] + alt, tp
        else:
            b = T[tp + tl:tp + tl + 1]
            ref, alt, pos = (ref + b) or b".", (alt + b) or b".", 1
    return "%s\t%d\t.\t%s\t%s\t.\t.\tDP=%d;AD=%d,%d;WIN=%d-%d" % (name, pos, ref.decode(), alt.decode(), span, n_ref, n_alt, gL + 1, gR)


def test_vcf_header_formats_the_anchoring_cases(tmp_path):
    src = tmp_path / "vcf_main.cpp"; src.write_text(_VCF_MAIN)
    exe = tmp_path / "vcf_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    T = b"ACGTTTGA"
    cases = [(3, 1, b"C", 9, 2, 7, 3, 4),            # a substitution keeps its coordinates
             (2, 2, b"TCA", 5, 1, 4, 2, 4),          # a replacement of another length too
             (6, 0, b"T", 8, 3, 5, 3, 6),            # an insertion: the base in front of it
             (3, 2, b"", 8, 3, 5, 3, 6),             # a deletion likewise
             (0, 0, b"GG", 4, 1, 3, 0, 0),           # an insertion at position 0: the base behind it
             (0, 2, b"", 4, 1, 3, 0, 2),             # a deletion at position 0
             (8, 0, b"A", 4, 1, 3, 7, 8),            # an insertion at tlen
             (0, 8, b"", 1, 0, 1, 0, 8)]             # the whole target gone: no anchor
    text = "".join("ctg %s %d %d %s %d %d %d %d %d\n" % (T.decode(), tp, tl, alt.decode() or "-", sp, nr, na, gl, gr)
                   for tp, tl, alt, sp, nr, na, gl, gr in cases)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    head = [ln for ln in out if ln.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1] == "##contig=<ID=ctg,length=12345>"
    assert [ln.split(",")[0] for ln in head[2:5]] == ["##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=WIN"]
    assert head[5] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and len(head) == 6
    body = [ln for ln in out if not ln.startswith("#")]
    assert body == [_vcf_line("ctg", T, *c) for c in cases]
    assert body[2].split("\t")[1:5] == ["6", ".", "T", "TT"] and body[4].split("\t")[1:5] == ["1", ".", "A", "GGA"]
    assert body[5].split("\t")[1:5] == ["1", ".", "ACG", "G"] and body[7].split("\t")[3:5] == ["ACGTTTGA", "."]


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _records(bb, alns, eqx=False):
    return [ct.compress(s, q, t, bb, eqx=eqx and bool(k % 2)) for k, (s, q, t) in enumerate(alns)]


def _strings(targets):
    """[(target bytes, [(start, q, t)])] of record targets; a target with a non-conforming record: None."""
    out = []
    for bb, recs in targets:
        if any(not ct.conforming(p, len(q), len(bb), o) for p, q, o in recs):
            out.append(None)
        else:
            out.append((bb, [ct.expand(p, q, bb, o) for p, q, o in recs]))
    return out


def _twin_edits(strings, min_cov, min_len, trim):
    return [[] if s is None else x for s, x in
            zip(strings, et.batch_edits([s if s is not None else (b"", []) for s in strings], min_cov, min_len, trim))]


def _twin_support(strings, segs, min_len, trim):
    """Flat, in the order of the edits: (w_begin, w_end, span, alt, ref)."""
    out = []
    for s, per in zip(strings, segs):
        if s is not None and per:
            out += [x for seg in ev.target_support(s[0], s[1], per, min_len, trim) for x in seg]
    return out


def _device(ctx, got):
    """The device's edits in the twin's form (as test_edits._device), and its support, flat."""
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


def _flat(sup):
    return list(zip(*(sup[k].tolist() for k in ("w_begin", "w_end", "span", "alt", "ref"))))


def _run(call, strings, min_cov, min_len, trim, oracle_edits=True, prepare=None):
    """call(ctx) -> results.  One context with edits only, one with edits and support: the same consensus and edits; the
    support equals the twin's, from the oracle's edits and from the device's own.  (flat support, device edits, status,
    re-runs)."""
    from pbdagcon_amd import capi
    off = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
    on = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
    try:
        for c in (off, on):
            if prepare:
                prepare(c)
            c.set_edits(True)
        on.set_edit_support(True)
        got_off = call(off)
        dev_off = _device(off, got_off)
        with pytest.raises(capi.DagconError) as e:
            off.edit_support()
        assert e.value.code == STATE
        got = call(on)
        dev = _device(on, got)
        sup = _flat(on.edit_support())
        status = on.target_status.tolist()
        reruns = on.timings()["reruns"]
    finally:
        off.close(); on.close()
    assert got == got_off and dev == dev_off
    assert len(sup) == sum(len(e) for per in dev for _, _, _, e in per)
    want = None
    if oracle_edits:
        exp = _twin_edits(strings, min_cov, min_len, trim)
        want = _twin_support(strings, exp, min_len, trim)
        assert sup == want                                           # the twin on the oracle's edits
        assert dev == exp
    # ... and on the device's own edit arrays (the same computation where those equal the oracle's)
    assert sup == (want if want is not None and dev == exp else _twin_support(strings, dev, min_len, trim))
    return sup, dev, status, reruns


def _whole(targets):
    from pbdagcon_amd import capi
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    return lambda c: c.consensus_cigar(cb, strict=False)


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 2])
def test_random_small_targets(oracle_lib, trim):
    """300 small targets in one batch, one with a non-conforming record: no entries for it, the others intact."""
    rng = np.random.default_rng(300 + trim)
    targets = []
    for k in range(300):
        alns, bb = _small_pileup(rng, k)
        targets.append((bb, _records(bb, alns, eqx=True)))
    bad = 150
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = _strings(targets)
    assert strings[bad] is None and sum(s is None for s in strings) == 1
    sup, dev, status, _ = _run(_whole(targets), strings, 3, 4, trim)
    assert status[bad] == NONCONFORMING and dev[bad] == [] and sum(1 for s in status if s) == 1
    spans = [x[2] for x in sup]
    print("edits %d, alt %d, ref %d, span %d" % (len(sup), sum(x[3] for x in sup), sum(x[4] for x in sup), sum(spans)))
    assert len(sup) > 200 and sum(x[3] for x in sup) > sum(x[4] for x in sup) > 0
    assert any(x[1] - x[0] >= 3 for x in sup)
    # (trimAln takes `trim` target bases off either end of every alignment: with trim > 0 no column holds base 0, no
    # segment begins there, and no window can; the edge is this test's only with trim 0)
    assert any(x[0] == 0 for x in sup) == (trim == 0)


def _retarget(start, tstr, tseq):
    """tstr with the bytes of tseq at the positions it consumes."""
    out, x = bytearray(tstr), start - 1
    for i, ch in enumerate(out):
        if ch != ct.GAP:
            out[i] = tseq[x]; x += 1
    return bytes(out)


def _nonrep(rng, n, avoid=b""):
    out = bytearray()
    while len(out) < n:
        b = int(rng.choice(np.frombuffer(b"ACGT", np.uint8)))
        if b not in avoid and (not out or out[-1] != b):
            out.append(b)
    return bytes(out)


def _period_target(rng, P):
    """P bases, a run of 70 A holding one A more in most reads, 30 bases, a run of 130 C holding one C less, 40 bases.
    Reads begin at base 0 or 63, 64, 65 bases in front of the first run, so that its window [P, P + 70) begins at
    columns 63, 64, 65 of an alignment; a quarter of the reads carry neither change, one has a wrong base in front of
    the first run."""
    bb = _nonrep(rng, P, b"A") + b"A" * 70 + _nonrep(rng, 30, b"AC") + b"C" * 130 + _nonrep(rng, 40, b"C")
    r1, r2 = P, P + 100
    alns = []
    for k in range(12):
        s = (0, P - 63, P - 64, P - 65)[k % 4] if k < 8 else 0
        carry = k % 4 != 3 or k < 4
        ins_at, del_at = r1 + int(rng.integers(0, 71)), r2 + int(rng.integers(0, 130))
        q, t = bytearray(), bytearray()
        for x in range(s, len(bb)):
            if carry and x == ins_at:
                q.append(ord("A")); t.append(ct.GAP)
            if carry and x == del_at:
                q.append(ct.GAP); t.append(bb[x]); continue
            q.append((ord("G") if bb[x] != ord("G") else ord("T")) if k == 9 and x == P - 1 else bb[x]); t.append(bb[x])
        alns.append((s + 1, bytes(q), bytes(t)))
    return bb, _records(bb, alns)


@pytest.mark.gpu
def test_windows_longer_than_a_step_and_the_64_column_period(oracle_lib):
    rng = np.random.default_rng(64)
    targets = [_period_target(rng, P) for P in (80, 100, 127, 128, 129)]
    strings = _strings(targets)
    sup, dev, status, _ = _run(_whole(targets), strings, 3, 30, 0)
    assert status == [0] * 5
    at = 0
    for P, per in zip((80, 100, 127, 128, 129), dev):
        n = sum(len(e) for _, _, _, e in per)
        flat, at = sup[at:at + n], at + n
        wins = {(a, b): (sp, al, rf) for a, b, sp, al, rf in flat}
        assert (P, P + 70) in wins and (P + 100, P + 230) in wins, (P, flat)
        sp, al, rf = wins[(P, P + 70)]
        assert al >= 6 and rf >= 1 and sp > al + rf                  # (the read with the wrong flank is "other")
        sp, al, rf = wins[(P + 100, P + 230)]
        assert al >= 6 and rf >= 1 and sp == 12


def _dense_target(rng, tlen=600, step=5):
    """Eight reads agree on a change every `step` bases (a substitution, or one base dropped), two carry none.  Bases
    280 to 340 are twenty runs of three equal bases, A, C, G, T in turn, and the eight reads drop one base of each: every
    deletion's window is its whole run, the windows touch, and the stretch is one group of twenty edits."""
    bb = bytearray(_nonrep(rng, tlen))
    for r in range(20):
        bb[280 + 3 * r:283 + 3 * r] = b"ACGT"[r % 4:r % 4 + 1] * 3
    bb[279] = ord("C") if bb[278] != ord("C") else ord("G")
    bb[340] = ord("C") if bb[341] != ord("C") else ord("G")
    bb = bytes(bb)
    q, t = bytearray(), bytearray()
    for x in range(tlen):
        if 280 <= x < 340:
            q.append(ct.GAP if (x - 280) % 3 == 1 else bb[x]); t.append(bb[x])
        elif x % step == 2 and 2 < x < tlen - 3 and not 275 <= x < 345:
            if (x // step) % 3 == 0:
                q.append(ct.GAP); t.append(bb[x])
            else:
                q.append(next(b for b in b"ACGT" if b not in (bb[x], bb[x - 1], bb[x + 1]))); t.append(bb[x])
        else:
            q.append(bb[x]); t.append(bb[x])
    alns = [(1, bytes(q), bytes(t))] * 8 + [(1, bb, bb)] * 2
    return bb, _records(bb, alns)


@pytest.mark.gpu
def test_the_64_edit_period_and_the_arena_rerun(oracle_lib):
    rng = np.random.default_rng(6)
    targets = [_dense_target(rng) for _ in range(30)]
    strings = _strings(targets)
    sup, dev, status, reruns = _run(_whole(targets), strings, 3, 30, 0)
    assert status == [0] * 30
    sum_bb = sum((len(bb) + 2 + 3) & ~3 for bb, _ in targets)
    assert len(sup) > sum_bb // 8 + 1024 and reruns >= 1            # the edit arena's first size did not hold them
    crossing = 0
    for (bb, _), per in zip(targets, dev):
        assert len(per) == 1 and len(per[0][3]) >= 100
        S, t0, t1, edits = per[0]
        crossing += any(first // 64 != (end - 1) // 64 for first, end, *_ in ev.segment_groups(bb, S, t0, t1, edits))
    assert crossing >= 25                                            # a group with edits on both sides of edit 64
    assert sum(1 for x in sup if x[3] == 8 and x[4] == 2) > len(sup) // 2


def _adjacent_target(rng, b, tlen=200):
    """Two adjacent segments whose groups touch at base b.  Five reads end in front of b, five begin at it, and eight
    whole reads carry a G between b - 1 and b: the best path runs through that G, whose weight is below min_cov, so the
    consensus is cut there into [.., b) and [b, ..).  Bases b - 3 .. b - 1 are AAA with an A more (the first segment's
    last edit, window [b - 3, b)), bases b .. b + 2 are CCC with a C less (the second segment's first edit, window
    [b, b + 3)).  Six more reads cross without the G, three with the A more and three without it, and begin so that the
    column of base b is column 0, 1 and 63 of a 64-column step: the second group's left flank, base b - 1, then lies in
    the step before, at lane 0, and 62 lanes down."""
    bb = bytearray(_nonrep(rng, tlen))
    bb[b - 3:b] = b"AAA"; bb[b:b + 3] = b"CCC"
    bb[b - 4] = ord("G") if bb[b - 5] != ord("G") else ord("T")
    bb[b + 3] = ord("G") if bb[b + 4] != ord("G") else ord("T")
    bb = bytes(bb)

    def read(s, e, g, ins_a=True):
        q, t = bytearray(), bytearray()
        for i in range(s, e):
            if i == b:
                if ins_a:
                    q.append(ord("A")); t.append(ct.GAP)
                if g:
                    q.append(ord("G")); t.append(ct.GAP)
            if i == b + 1:
                q.append(ct.GAP); t.append(bb[i]); continue
            q.append(bb[i]); t.append(bb[i])
        if e == b:
            q.append(ord("A")); t.append(ct.GAP)
        return (s + 1, bytes(q), bytes(t))
    alns = [read(0, b, False) for _ in range(5)] + [read(b, tlen, False) for _ in range(5)] + [read(0, tlen, True) for _ in range(8)]
    alns += [read(s, tlen, False) for s in (b - 127, b - 128, b - 126)]                 # b - s + 1 columns in front of base b
    alns += [read(s, tlen, False, ins_a=False) for s in (b - 128, b - 129, b - 127)]    # b - s columns
    return bb, _records(bb, alns)


@pytest.mark.gpu
def test_touching_groups_of_adjacent_segments(oracle_lib):
    rng = np.random.default_rng(1)
    targets = [_adjacent_target(rng, b) for b in (130, 131, 140)]
    strings = _strings(targets)
    # on the CPU first: the input is what it is meant to be
    for (bb, alns), b in zip(strings, (130, 131, 140)):
        where = {(ev.coords(s0, t)[0][i] - b, i % 64) for s0, q, t in ev.columns(alns[-6:], 30, 0) for i in range(len(t))
                 if t[i] != ct.GAP and ev.coords(s0, t)[0][i] == b}
        assert where == {(0, 0), (0, 1), (0, 63)}
    sup, dev, status, _ = _run(_whole(targets), strings, 9, 30, 0)
    assert status == [0] * 3
    at = 0
    for per, b in zip(dev, (130, 131, 140)):
        assert [(t0, t1) for _, t0, t1, _ in per] == [(0, b), (b, 200)]          # adjacent
        assert sup[at:at + 2] == [(b - 3, b, 14, 3, 3), (b, b + 3, 14, 3, 0)]    # touching; the reads at columns 0, 1, 63 are alt / ref
        at += 2


@pytest.mark.gpu
def test_an_alignment_on_the_redo_path(oracle_lib):
    """The input of test_gpu_parity.test_long_gap_runs_take_the_redo_path as records: a 700-column insertion sends one
    alignment through k_normalize_slow, whose columns are read like every other's."""
    rng = np.random.default_rng(21)
    tl = 900
    alns, bb = random_target(rng, tl, 8, alphabet=b"ACGT", full_span=True, sub=0.02, ins=0.08, dele=0.04)
    bbs = bytearray(bb)
    bbs[300:520] = b"A" * 220
    bb = bytes(bbs)
    alns = [(s, q, _retarget(s, t, bb)) for s, q, t in alns]
    extra = []
    for k in range(6):
        q, t = bytearray(), bytearray()
        for i in range(tl):
            if k % 3 == 0 and i == 200:
                n_ins = 300 if k == 0 else 700
                ins = bytes(b"ACGT"[j] for j in rng.integers(0, 4, n_ins))
                q += ins; t += b"-" * n_ins
            if k % 3 == 1 and 600 <= i < 850:
                q.append(0x2D); t.append(bb[i]); continue
            if k % 3 == 2 and i == 299:
                q += b"A" * 3; t += b"-" * 3
            q.append(bb[i]); t.append(bb[i])
        extra.append((1, bytes(q), bytes(t)))
    alns2 = [(1, bytes(bb[i] if rng.random() > 0.05 else 0x2D for i in range(tl)), bb) for _ in range(3)]
    targets = [(bb, _records(bb, alns + extra + alns2))]
    strings = _strings(targets)
    assert strings[0] is not None
    sup, dev, status, _ = _run(_whole(targets), strings, 6, 500, 50)
    assert status == [0] and len(sup) >= 1
    # k_norm_chunk gives up on an alignment whose look-ahead outgrows its second window of 512 columns (DG_NW_BIG): the
    # read with 700 inserted columns is such a one.  It covers the whole target and passes min_len, so every group that
    # all counted alignments span has it among them -- were its columns misread, these counts would not be the twin's
    counted = ev.columns(strings[0][1], 500, 50)
    assert any(sum(1 for c in t if c == ct.GAP) >= 700 for _, _, t in counted)
    assert any(x[2] == len(counted) for x in sup)


def _variant_targets(seed, n, lo, hi, full_span=None):
    """As test_edits._random_targets without the soft mask: reads that share variants, so that the consensus differs
    from its target."""
    import test_edits as te
    return te._random_targets(seed, n, lo, hi, mask=False, full_span=full_span)


@pytest.mark.gpu
def test_the_kinds_give_the_plain_call_s_arrays(oracle_lib):
    from pbdagcon_amd import capi
    targets = _variant_targets(91, 20, 150, 400, full_span=True)
    strings = _strings(targets)
    n = sum(len(recs) for _, recs in targets)
    reverse = (np.arange(n) % 3 == 1).astype(np.uint8)
    as_file, i = [], 0
    for bb, recs in targets:
        as_file.append((bb, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(recs)]))
        i += len(recs)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    arr = ct.records_to_arrays(targets); arr["t_blob"] = None
    md = capi.HostMdTags.from_texts([mt.encode(p, q, bb, o) for bb, recs in targets for p, q, o in recs])
    cs = capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs]) for bb, recs in targets])
    calls = {"plain": lambda c: c.consensus_cigar(plain), "packed": lambda c: c._intake(plain.packed(), None, plain, True),
             "stranded": lambda c: c._intake(capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), None, None, True),
             "cs": lambda c: c.consensus_cs(cs), "md": lambda c: c.consensus_cigar_md(capi.HostCigarBatch(**arr), md)}
    ref = None
    for kind, call in calls.items():
        sup, dev, status, _ = _run(call, strings, 3, 30, 5, oracle_edits=kind == "plain")
        assert status == [0] * 20, kind
        if ref is None:
            ref = (sup, dev)
            assert len(sup) > 100 and sum(x[3] for x in sup) > sum(x[4] for x in sup) > 0
        assert (sup, dev) == ref, kind


@pytest.mark.gpu
def test_windows_equal_the_twin_per_window(oracle_lib):
    from pbdagcon_amd import capi
    targets = _variant_targets(77, 20, 120, 120)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 40, 10)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    assert not any(f for _, _, f in per) and len(wins) == 60
    strings = [(targets[g][0][a:b], alns) for (g, a, b), (_, alns, _) in zip(wins, per)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sup, dev, status, _ = _run(lambda c: c.consensus_cigar_windows(cb, hw), strings, 3, 30, 5)
    assert len(sup) > 60 and sum(1 for p in dev if p) > 40


@pytest.mark.gpu
def test_record_filter_left_out_records_are_not_counted(oracle_lib):
    from pbdagcon_amd import capi
    targets = _variant_targets(13, 15, 150, 300)
    depth = 5
    assert all(len(recs) > depth for _, recs in targets)
    probe = capi.Context(min_cov=3, min_len=30, trim=5, flags=capi.FLAG_BASE_POS)
    try:
        probe.set_record_filter(max_depth=depth)
        probe.consensus_cigar(capi.HostCigarBatch(**ct.records_to_arrays(targets)))
        fate = probe.record_stats()["fate"]
    finally:
        probe.close()
    assert (fate & capi.FATE_MAX_DEPTH).any()
    kept, i = [], 0
    for bb, recs in targets:
        kept.append((bb, [r for k, r in enumerate(recs) if not fate[i + k]]))
        i += len(recs)
    assert all(len(recs) == depth for _, recs in kept)
    sup, dev, status, _ = _run(_whole(targets), _strings(kept), 3, 30, 5, prepare=lambda c: c.set_record_filter(max_depth=depth))
    assert len(sup) > 30 and max(x[2] for x in sup) <= depth and any(x[2] == depth for x in sup)


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    from util import batch_from_targets
    targets = _variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sb = batch_from_targets([(len(bb), [ct.expand(p, q, bb, o) for p, q, o in recs], None) for bb, recs in targets])

    def code(f):
        with pytest.raises(capi.DagconError) as e:
            f()
        return e.value.code
    c = capi.Context(min_cov=3, min_len=30, trim=5, flags=capi.FLAG_BASE_POS)
    try:
        assert code(lambda: c.set_edit_support(True)) == STATE       # edits off
        assert code(c.edit_support) == STATE
        assert code(lambda: c.set_edit_support(False)) == STATE
        c.set_edits(True)
        c.consensus_cigar(cb)
        assert c.edits()["t_pos"].size > 0 and code(c.edit_support) == STATE     # the switch off at the upload
        c.set_edit_support(True)
        assert code(c.edit_support) == STATE                         # on now, but the batch was uploaded without it
        c.upload_cigar(cb); c.run(); c.sync()
        assert code(c.edit_support) == STATE                         # before a fetch
        c.fetch()
        n = c.edits()["t_pos"].size
        assert c.edit_support()["span"].size == n > 0
        c.consensus(sb)
        assert code(c.edit_support) == STATE                         # dagcon_consensus: no record upload
        c.consensus_cigar(cb)
        assert c.edit_support()["span"].size == n
        c.set_edits(False)                                           # edits off turns it off
        assert code(c.edit_support) == STATE
        c.consensus_cigar(cb)
        assert code(c.edit_support) == STATE and code(c.edits) == STATE
        c.set_edits(True)
        c.consensus_cigar(cb)
        assert c.edits()["t_pos"].size == n and code(c.edit_support) == STATE
    finally:
        c.close()


def _undo_anchor(pos, ref, alt):
    """The (t_pos, REF, ALT) an --edits line may have had for a VCF line.  An edit with bytes on both sides has neither
    its first nor its last bytes in common (the trim), so a shared first byte is the anchor in front and, at POS 1, a
    shared last byte may be the anchor behind; the two readings of 'G -> GGG' at POS 1 are the same variant."""
    out = []
    if ref[:1] == alt[:1]:
        out.append((pos, ref[1:], alt[1:]))
    if pos == 1 and ref[-1:] == alt[-1:]:
        out.append((0, ref[:-1], alt[:-1]))
    return out or [(pos - 1, ref, alt)]


@pytest.mark.gpu
def test_pbdagcon_vcf(oracle_lib, tmp_path):
    """--sam --ref --edits E --vcf V on 20 targets: stdout and E are those of the command without --vcf, the VCF lines map
    one to one onto E's edit lines after undoing the anchor, DP / AD / WIN equal the twin; --bam --md --vcf gives the
    same file."""
    targets = _variant_targets(101, 20, 150, 300, full_span=True)
    names = ["ctg%d" % i for i in range(20)]
    tl = [len(bb) for bb, _ in targets]
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [r for _, r in targets]))
    texts = [[mt.encode(p, q, bb, o) for p, q, o in recs] for bb, recs in targets]
    bam = tmp_path / "in.bam"; bam.write_bytes(mf.bam_file(names, tl, mf.records(names, targets, texts)))
    ed, ed2, vcf, vcf2 = (tmp_path / x for x in ("e.tsv", "e2.tsv", "o.vcf", "o2.vcf"))
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    plain = subprocess.run(base + ["--sam", "--ref", str(ref), "--edits", str(ed2), str(sam)], capture_output=True, timeout=300)
    got = subprocess.run(base + ["--sam", "--ref", str(ref), "--edits", str(ed), "--vcf", str(vcf), str(sam)], capture_output=True, timeout=300)
    md = subprocess.run(base + ["--bam", "--md", "--vcf", str(vcf2), str(bam)], capture_output=True, timeout=300)
    for r in (plain, got, md):
        assert r.returncode == 0, r.stderr.decode()
    assert got.stdout == plain.stdout == md.stdout and got.stdout.count(b">") >= 20
    assert ed.read_bytes() == ed2.read_bytes()
    assert vcf.read_bytes() == vcf2.read_bytes()
    lines = vcf.read_text().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[1:21] == ["##contig=<ID=%s,length=%d>" % x for x in zip(names, tl)]
    body = [ln.split("\t") for ln in lines if not ln.startswith("#")]
    elines = [ln.split("\t") for ln in ed.read_text().splitlines() if not ln.startswith("#")]
    assert len(body) == len(elines) > 50
    byname = dict(zip(names, (bb for bb, _ in targets)))
    for v, e in zip(body, elines):
        assert v[0] == e[0] and v[2] == "." and v[5] == v[6] == "."
        assert (int(e[1]), int(e[2]), e[3], e[4]) in [(t_pos, t_pos + len(r), r.decode() or "-", a.decode() or "-")
                                                      for t_pos, r, a in _undo_anchor(int(v[1]), v[3].encode(), v[4].encode())], (v, e)
        T = byname[v[0]]
        assert "\t".join(v[:5]) == _vcf_line(v[0], T, int(e[1]), int(e[2]) - int(e[1]), b"" if e[4] == "-" else e[4].encode(), 0, 0, 0, 0, 0).rsplit("\t", 3)[0]
    # DP / AD / WIN against the twin, fed the edits of the file itself
    strings = _strings(targets)
    segs, cur = [[] for _ in targets], None
    fasta = got.stdout.decode().split("\n")[1::2]
    k = 0
    for ln in ed.read_text().splitlines():
        f = ln.split("\t") if not ln.startswith("#") else ln.split(" ")
        if ln.startswith("#piece "):
            cur = (fasta[k].encode(), int(f[2]), int(f[3]), [])
            segs[names.index(f[1])].append(cur); k += 1
        else:
            alt = "" if f[4] == "-" else f[4]
            done = sum(cl for _, _, _, cl in cur[3]) - sum(tl_ for _, tl_, _, _ in cur[3])
            cur[3].append((int(f[1]), int(f[2]) - int(f[1]), int(f[1]) - cur[1] + done, len(alt)))
    want = _twin_support(strings, segs, 30, 5)
    assert [v[7] for v in body] == ["DP=%d;AD=%d,%d;WIN=%d-%d" % (sp, rf, al, a + 1, b) for a, b, sp, al, rf in want]
