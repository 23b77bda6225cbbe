"""Per-read alleles at the sites and the two-way read split (dagcon_set_site_reads, pbdagcon --site-reads / --haplotag):
the rule by hand and the twin's invariants on the CPU, the device against the twin byte for byte on the GPU.
include/dagcon.h states the rule; site_reads_twin.py is it in Python."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import evidence_twin as ev
import md_twin as mt
import paf_files as pf
import pileup_twin as pt
import site_reads_twin as srt
import window_twin as wt
from util import batch_from_targets, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID, NONCONFORMING = -8, -1, -4
GAP = 0x2D
A, C, G, T, N, DEL = range(6)
INS = 8                                                          # the ins bit of a code
W = 64                                                           # the wave: columns a step of the walk, entries a stride of the split


def _tes():
    import test_edit_support as tes
    return tes


def _tp():
    import test_pileup as tp
    return tp


def _cli():
    return _tes()._cli()


def _n(**kw):
    return _tp()._n(**kw)


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def test_the_rule_by_hand(oracle_lib):
    """Twelve columns: four reads on ACGTACGTACGT.  r0 and r1 read the target; r2 and r3 drop base 3 and insert behind
    base 6; r3 is below min_len in another run."""
    bb = b"ACGTACGTACGT"
    ref = (1, bb, bb)
    alt = (1, b"ACG-ACGGTACGT", b"ACGTACG-TACGT")
    alns = [ref, ref, alt, alt]
    tw = srt.target(12, alns, 4, 0, (2, 200000))
    assert tw["sites"] == [3, 6] and tw["src"] == [0, 1, 2, 3]
    assert tw["counts"][3] == _n(T=2, DEL=2) and tw["counts"][6] == _n(G=4, INS=2)
    assert tw["ents"] == [[(0, T), (1, G)], [(0, T), (1, G)], [(0, DEL), (1, G | INS)], [(0, DEL), (1, G | INS)]]
    # site 3: a base site, k1 = T (index 3 before DEL, 5), k2 = DEL; site 6: min(INS, depth - INS) = 2 > s2 = 0: an insertion site
    assert srt.kind(tw["counts"][3]) == ("base", T, DEL) and srt.kind(tw["counts"][6]) == ("ins",)
    assert [[srt.sign(c, tw["counts"][tw["sites"][k]]) for k, c in e] for e in tw["ents"]] == [[1, 1], [1, 1], [-1, -1], [-1, -1]]
    # the seed is alignment 0 (two signed entries like the others, the lowest x); one round settles it
    assert tw["hap"] == [1, 1, 2, 2] and tw["phase"] == [1, 1] and tw["signed"] == [2, 2, 2, 2]
    trace = []
    srt.split(tw["ents"], [tw["counts"][p] for p in tw["sites"]], 2, trace)
    assert trace[0] == trace[1] == ([1, 1, -1, -1], [1, 1])
    # every position a site: the entries are the target-base columns, in ascending position
    all_ = srt.target(12, alns, 4, 0, (0, 0))
    assert all_["sites"] == list(range(12)) and [len(e) for e in all_["ents"]] == [12] * 4
    assert all([k for k, _ in e] == list(range(12)) for e in all_["ents"])
    # an alignment below min_len is not numbered: src keeps the caller's index
    short = srt.target(12, [ref, (1, b"ACG", b"ACG"), alt, alt, ref], 4, 0, (2, 200000))
    assert short["src"] == [0, 2, 3, 4] and short["hap"] == [1, 2, 2, 1]
    # a leading inserted column counts nowhere and sets no ins bit; a mismatch is DEL and ins at its base
    lead = srt.target(4, [(1, b"TACGT", b"-ACGT"), (1, b"ACGT", b"ACGT"), (1, b"ATGT", b"ACGT")], 1, 0, (0, 0))
    assert lead["ents"][0] == [(0, A), (1, C), (2, G), (3, T)] and lead["ents"][2][1] == (1, DEL | INS)
    # a tie leaves a read unassigned: it reads T at site 3 with the first group and inserts at 6 with the second
    mix = (1, b"ACGTACGGTACGT", b"ACGTACG-TACGT")
    tie = srt.target(12, [ref, ref, alt, alt, mix], 4, 0, (2, 200000))
    assert tie["hap"] == [1, 1, 2, 2, 0]


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    rng = np.random.default_rng(79)
    n_ent = n_ins = n_signed = n_assigned = 0
    for k in range(600):
        alns, bb = _tes()._small_pileup(rng, k)
        trim = int(rng.integers(0, 3))
        opts = (0, 0) if k % 2 else (2, 200000)
        tw = srt.target(len(bb), alns, 4, trim, opts)
        sums = [[0] * 7 for _ in tw["sites"]]
        for e in tw["ents"]:
            assert [s for s, _ in e] == sorted({s for s, _ in e})            # ascending, one entry a site
            for s, code in e:
                sums[s][code & 7] += 1
                sums[s][6] += code >> 3
                assert code & 7 <= 5 and code >> 4 == 0
        assert sums == [tw["counts"][p][:7] for p in tw["sites"]]            # the defining invariant
        # one round more changes nothing wherever the run had stopped changing
        sc = [tw["counts"][p] for p in tw["sites"]]
        trace = []
        more = srt.split(tw["ents"], sc, srt.ROUNDS + 1, trace)
        if len(trace) >= 2 and trace[srt.ROUNDS - 1] == trace[srt.ROUNDS - 2]:
            assert more == (tw["hap"], tw["phase"])
        n_ent += sum(len(e) for e in tw["ents"]); n_ins += sum(c >> 3 for e in tw["ents"] for _, c in e)
        n_signed += sum(tw["signed"]); n_assigned += sum(1 for h in tw["hap"] if h)
    print("entries %d, with ins %d, signed %d, alignments assigned %d" % (n_ent, n_ins, n_signed, n_assigned))
    assert n_ent > 20000 and n_ins > 1000 and n_signed > 10000 and n_assigned > 1000


def test_signs():
    kind, sign = srt.kind, srt.sign
    # k1 ties go to the lowest index, k2 to the lowest among the others
    assert kind(_n(A=3, C=3)) == ("base", A, C) and kind(_n(C=3, DEL=3, G=3)) == ("base", C, G)
    assert kind(_n(T=5, A=2, DEL=2)) == ("base", T, A)
    # k2 with count 0 is no class: only k1 carries a sign
    assert kind(_n(G=4)) == ("base", G, None)
    assert [sign(c, _n(G=4)) for c in (G, A, DEL)] == [1, 0, 0]
    assert [sign(c, _n(A=3, C=3, T=1)) for c in (A, C, T, A | INS)] == [1, -1, 0, 1]
    # the insertion-site boundary: min(INS, depth - INS) == s2 is a base site, one more an insertion site
    assert kind(_n(A=6, C=2, INS=2)) == ("base", A, C) and kind(_n(A=6, C=2, INS=3)) == ("ins",)
    assert kind(_n(A=6, C=2, INS=6)) == ("base", A, C) and kind(_n(A=6, C=2, INS=5)) == ("ins",)
    assert [sign(c, _n(A=6, C=2, INS=3)) for c in (A, C, A | INS, C | INS, DEL)] == [1, 1, -1, -1, 1]
    assert srt.sgn(0) == 0 and srt.sgn(-3) == -1 and srt.sgn(2) == 1


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    names = ("dagcon_set_site_reads", "dagcon_fetch_site_reads")
    lib = capi.load()
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %zu\\n", sizeof(dagcon_site_reads_opts), '
            'sizeof(dagcon_site_reads)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert [ctypes.sizeof(x) for x in (capi.SiteReadsOpts, capi.SiteReads)] == [int(x) for x in out]
    for m in ("set_site_reads", "site_reads"):
        assert callable(getattr(capi.Context, m))
    assert lib.dagcon_abi_version() == 2


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    sr, ht = tmp_path / "o.reads", tmp_path / "o.tags"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for flag, f in (("--site-reads", sr), ("--haplotag", ht)):
        for args in ([str(m5), flag],
                     rec + ["--window", "200", "--overlap", "120", flag, str(f), str(sam)],
                     ["-a", flag, str(f), str(m5)], ["-a", "--polish", "1", flag, str(f), str(m5)],
                     rec + ["--dump-parsed", flag, str(f), str(sam)],
                     [flag, str(f), "--site-min-frac", "1.5", str(m5)]):
            out = run(*args)
            assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
            assert not f.exists()
        # a file that cannot be written is said before anything runs
        out = run(*rec, flag, str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr, flag
    # the thresholds go with either flag, without --sites
    out = run("--site-reads", str(tmp_path / "no_such_dir" / "o.txt"), "--site-min-frac", "0.3", "--site-min-count", "3", str(m5))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --site-reads FILE")[1].split(b"\n  --fastq")[0]
    assert b"RNAME POS QNAME ALLELE INS" in text and b"\n  --haplotag FILE" in text and b"RNAME QNAME HAP" in text
    assert text.count(b"parity unpinned") == 2 and b"[--site-reads FILE] [--haplotag FILE]" in h.stdout


_SR_MAIN = r"""
#include <iostream>
#include "site_reads.h"
// stdin: "r rname pos0 qname code" | "h rname qname hap n" | "s code n0 .. n7" per line; stdout: the lines, the sign
int main() {
    std::string out, kind, rname, qname;
    while (std::cin >> kind) {
        if (kind == "r") { unsigned long long pos; unsigned code; std::cin >> rname >> pos >> qname >> code; dg_site_read_line(out, rname, pos, qname, (uint8_t)code); }
        else if (kind == "h") { unsigned hap; unsigned long long n; std::cin >> rname >> qname >> hap >> n; dg_haplotag_line(out, rname, qname, hap, n); }
        else { unsigned code, v[8]; uint16_t n[8]; std::cin >> code; for (int k = 0; k < 8; k++) { std::cin >> v[k]; n[k] = (uint16_t)v[k]; }
               out += std::to_string(dg_sr_sign((uint8_t)code, n)); out += '\n'; }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatters_against_python(tmp_path):
    src = tmp_path / "sr_main.cpp"; src.write_text(_SR_MAIN)
    exe = tmp_path / "sr_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    reads = [("ctg", 0, "q0_1", A), ("a/b|c", 4294967295, "m/1/0_9", DEL | INS), ("x", 41, "r", N), ("x", 41, "r", T | INS)]
    tags = [("ctg", "q0_1", 0, 0), ("ctg", "q0_2", 2, 123456789012), ("x", "r", 1, 7)]
    piles = [_n(A=3, C=3), _n(C=3, DEL=3, G=3), _n(G=4), _n(A=3, C=3, T=1), _n(A=6, C=2, INS=2), _n(A=6, C=2, INS=3), _n(A=6, C=2, INS=6),
             _n(A=6, C=2, INS=5), _n(A=4094, DEL=4094, INS=4094)]
    signs = [(c | i, n) for n in piles for c in range(6) for i in (0, INS)]
    text = "".join("r %s %d %s %d\n" % x for x in reads) + "".join("h %s %s %d %d\n" % x for x in tags)
    text += "".join("s %d %s\n" % (c, " ".join(map(str, n))) for c, n in signs)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert out == [srt.site_reads_line(*x) for x in reads] + [srt.haplotag_line(*x) for x in tags] + [str(srt.sign(c, n)) for c, n in signs]
    assert out[0] == "ctg\t1\tq0_1\tA\t0" and out[1] == "a/b|c\t4294967296\tm/1/0_9\t*\t1" and out[5] == "ctg\tq0_2\t2\t123456789012"


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _code(f):
    return _tp()._code(f)


def _device(call, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None, flags=0):
    """One context with the pile-up and the switch on: (results, pileup, sites, site reads, status, re-runs)."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=flags)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*opts)
        c.set_site_reads(phase, rounds)
        got = call(c)
        sr, ps, pu = c.site_reads(), c.pileup_sites(), c.pileup()
        return got, pu, ps, sr, c.target_status.tolist(), c.timings()["reruns"]
    finally:
        c.close()


def _expect(strings, tlens, min_cov, min_len, trim, opts, rounds, status, n_given=None, src=None):
    """The arrays the twin expects.  strings[t]: (target, alignments the pipeline sees) or None; n_given[t]: alignments the
    caller gave for target t (default: those of strings); src[t][i]: the caller's index of alignment i of strings[t]
    (default: its place in the batch)."""
    out = {k: [] for k in ("aln_tgt", "aln_src", "ent_site", "ent_code", "hap", "phase", "pos")}
    out["ent_begin"], out["site_begin"] = [0], [0]
    base = 0
    for t, (s, tl) in enumerate(zip(strings, tlens)):
        n_al = 0 if s is None else len(s[1])
        if s is not None and not status[t] and n_al >= max(1, min_cov):
            tw = srt.target(tl, s[1], min_len, trim, opts, rounds or srt.ROUNDS)
            sb = len(out["pos"])
            for i, e, h in zip(tw["src"], tw["ents"], tw["hap"]):
                out["aln_tgt"].append(t); out["aln_src"].append(src[t][i] if src is not None else base + i); out["hap"].append(h)
                out["ent_site"] += [sb + k for k, _ in e]; out["ent_code"] += [c for _, c in e]
                out["ent_begin"].append(len(out["ent_site"]))
            out["pos"] += tw["sites"]; out["phase"] += tw["phase"]
        out["site_begin"].append(len(out["pos"]))
        base += n_given[t] if n_given is not None else n_al
    return out


def _check(dev, exp, phase=True):
    pu, ps, sr = dev
    assert ps["site_begin"].tolist() == exp["site_begin"] and ps["pos"].tolist() == exp["pos"]
    for k in ("aln_tgt", "aln_src", "ent_begin", "ent_site", "ent_code"):
        assert sr[k].tolist() == exp[k], k
    if phase:
        assert sr["hap"].tolist() == exp["hap"] and sr["phase"].tolist() == exp["phase"]
    else:
        assert sr["hap"] is None and sr["phase"] is None
    # the sum invariant from the device's own arrays
    sums = np.zeros((ps["pos"].size, 8), np.int64)
    np.add.at(sums, (sr["ent_site"].astype(np.int64), (sr["ent_code"] & 7).astype(np.int64)), 1)
    np.add.at(sums, (sr["ent_site"].astype(np.int64), np.full(sr["ent_site"].size, 6)), (sr["ent_code"] >> 3).astype(np.int64))
    assert np.array_equal(sums, ps["counts"].astype(np.int64))
    assert (sr["ent_code"] & 7).max(initial=0) <= 5 and (sr["ent_code"] >> 4).max(initial=0) == 0


def _run(call, strings, tlens, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None, n_given=None, src=None):
    got, pu, ps, sr, status, reruns = _device(call, min_cov, min_len, trim, opts, phase, rounds, prepare)
    exp = _expect(strings, tlens, min_cov, min_len, trim, opts, rounds, status, n_given, src)
    _check((pu, ps, sr), exp, phase)
    return sr, ps, status, reruns, exp


def _tlens(targets):
    return [len(bb) for bb, _ in targets]


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 2])
@pytest.mark.parametrize("opts", [(0, 0), (2, 200000)])
def test_random_small_targets(oracle_lib, trim, opts):
    """150 small targets in one batch, one with a non-conforming record: no alignments and no entries of it."""
    tes = _tes()
    rng = np.random.default_rng(300 + trim)
    targets = []
    for k in range(150):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns, eqx=True)))
    bad = 75
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = tes._strings(targets)
    assert strings[bad] is None
    sr, ps, status, _, exp = _run(tes._whole(targets), strings, _tlens(targets), 3, 4, trim, opts, n_given=[len(r) for _, r in targets])
    assert status[bad] == NONCONFORMING and sum(1 for s in status if s) == 1 and bad not in sr["aln_tgt"].tolist()
    print("alignments %d, entries %d, with ins %d, hap %s" % (sr["aln_tgt"].size, sr["ent_site"].size, int((sr["ent_code"] >> 3).sum()),
                                                           np.bincount(sr["hap"], minlength=3).tolist()))
    assert sr["aln_tgt"].size > 400 and sr["ent_site"].size > (5000 if opts == (0, 0) else 500) and (sr["ent_code"] >> 3).sum() > 100
    assert np.bincount(sr["hap"], minlength=3)[1:].min() > 0                 # both labels occur


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(0, 0), (2, 200000)])
def test_the_64_column_period(oracle_lib, opts):
    """test_pileup's hand-built reads: what each puts at columns 63 / 64 of its alignment is in its name.  At 0 / 0 every
    target-base column is an entry, so there is a site at column 63 and at column 64 of an alignment, alignments of exactly
    64 and 65 columns, and every alignment begins and ends on a site; at 2 / 200000 the run behind base P - 1 makes a site."""
    tes, tp = _tes(), _tp()
    rng = np.random.default_rng(64)
    Ps = (80, 100, 127, 128, 129)
    targets = []
    for P in Ps:
        reads, bb, recs = tp._lane_reads(rng, tes._nonrep(rng, P + 150), P)
        targets.append((bb, recs))
    strings = tes._strings(targets)
    # on the CPU first: the input is what it is meant to be
    for (bb, alns), P in zip(strings, Ps):
        cols = ev.columns(alns, 30, 0)
        assert len(cols) == len(alns)
        here = set()
        for s0, q, t in cols:
            here.add(("columns", len(t)))
            for i in range(len(t)):
                if t[i] != GAP:
                    here.add(("base", i % 64))
                    if i + 1 < len(t) and t[i + 1] == GAP and q[i + 1] != GAP:
                        here.add(("anchor", i % 64))
            here.add(("lead", next(i for i in range(len(t)) if t[i] != GAP)))
        assert {("columns", 64), ("columns", 65), ("base", 63), ("base", 0), ("anchor", 63), ("anchor", 62), ("lead", 63), ("lead", 64)} <= here, (P, sorted(here))
    sr, ps, status, _, exp = _run(tes._whole(targets), strings, _tlens(targets), 3, 30, 0, opts)
    assert status == [0] * 5
    for t, P in enumerate(Ps):
        s = int(ps["site_begin"][t]) + ps["pos"][int(ps["site_begin"][t]):int(ps["site_begin"][t + 1])].tolist().index(P - 1)
        at = sr["ent_code"][sr["ent_site"] == s]
        assert int((at >> 3).sum()) == 3 and at.size == int(ps["counts"][s][:6].sum())


def _piles(n_sites, tl, depth=6):
    """A target of tl bases under `depth` reads, every read its own target string: half read A and half C at the first
    n_sites positions, all read G behind them."""
    alns = []
    for k in range(depth):
        s = (b"A" if k < depth // 2 else b"C") * n_sites + b"G" * (tl - n_sites)
        alns.append((1, s, s))
    return (b"N" * tl, alns)


@pytest.mark.gpu
def test_depth_and_packing(oracle_lib):
    """Depth 70 at the sites of one target; targets with exactly W and W + 1 sites (W = 64: a wave's columns a step and a
    wave's entries a stride), with 256 and 257 (the split's block of sites a stride)."""
    strings = [_piles(3, 40, depth=70), _piles(W, 100), _piles(W + 1, 100), _piles(256, 300), _piles(257, 300), _piles(1, 40)]
    tlens = [len(bb) for bb, _ in strings]
    batch = batch_from_targets([(tl, alns, None) for tl, (_, alns) in zip(tlens, strings)])
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), strings, tlens, 3, 30, 0, (2, 200000))
    assert status == [0] * 6
    assert np.diff(ps["site_begin"]).tolist() == [3, W, W + 1, 256, 257, 1]
    assert sr["hap"].tolist() == [1] * 35 + [2] * 35 + ([1] * 3 + [2] * 3) * 5
    assert np.diff(sr["ent_begin"]).tolist() == [3] * 70 + [W] * 6 + [W + 1] * 6 + [256] * 6 + [257] * 6 + [1] * 6


@pytest.mark.gpu
def test_arena_growth(oracle_lib):
    """At 0 / 0 every target-base column is an entry: 40 reads of 400 bases are 16,000 entries in an arena whose first size
    is a 64th of the columns + 4,096.  The batch runs again with a larger one; the consensus and the pile-up are those of
    a context without the switch."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    alns, bb = random_target(rng, 400, 40, full_span=True, sub=0.02, ins=0.03, dele=0.03)
    strings = [(bb, alns)]
    batch = batch_from_targets([(400, alns, None)])
    assert sum(len(q) for _, q, _ in alns) // 64 + 4096 < 40 * 380
    got, pu, ps, sr, status, reruns = _device(lambda c: c.consensus(batch), 3, 30, 5, (0, 0))
    _check((pu, ps, sr), _expect(strings, [400], 3, 30, 5, (0, 0), 0, status))
    assert status == [0] and sr["ent_site"].size > 40 * 380
    off = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        off.set_pileup(0, 0)
        got_off = off.consensus(batch)
        assert _code(off.site_reads) == STATE
        pu_off, ps_off, reruns_off = off.pileup(), off.pileup_sites(), off.timings()["reruns"]
    finally:
        off.close()
    assert reruns > reruns_off                                         # the re-run happened, and it was the entry arena's
    assert got == got_off
    for k in ("pos_begin", "counts"):
        assert np.array_equal(pu[k], pu_off[k])
    for k in ("site_begin", "pos", "counts"):
        assert np.array_equal(ps[k], ps_off[k])


@pytest.mark.gpu
def test_the_aln_src_map_of_a_string_batch(oracle_lib):
    """Alignments below min_len in the middle of a target, a target below min_cov between two others, an alignment that
    is empty after the trim, and a non-conforming target: aln_src is the index in the caller's batch."""
    rng = np.random.default_rng(11)
    a0, bb0 = random_target(rng, 120, 6, full_span=True, sub=0.05, ins=0.05, dele=0.05)
    a0[2] = (a0[2][0], a0[2][1][:20], a0[2][2][:20])                  # below min_len 30
    a0[4] = (a0[4][0], a0[4][1][:25], a0[4][2][:25])
    a1, bb1 = random_target(rng, 90, 2, full_span=True)                # below min_cov 3
    a2, bb2 = random_target(rng, 150, 7, full_span=True, sub=0.05, ins=0.05, dele=0.05)
    # 30 columns and 8 target bases: the trim of 5 from either end leaves nothing
    a2[3] = (40, b"ACGT" + b"A" * 22 + b"ACGT", bytes(bb2[39:43]) + b"-" * 22 + bytes(bb2[43:47]))
    a3, bb3 = random_target(rng, 100, 5, full_span=True)
    a3[1] = (90, a3[1][1], a3[1][2])                                   # leaves the backbone
    a4, bb4 = random_target(rng, 80, 4, full_span=True, sub=0.08)
    strings = [(bb0, a0), (bb1, a1), (bb2, a2), (bb3, a3), (bb4, a4)]
    tlens = [120, 90, 150, 100, 80]
    assert ev.columns([a2[3]], 30, 5) == [] and len(a2[3][1]) >= 30
    batch = batch_from_targets([(tl, alns, None) for tl, (_, alns) in zip(tlens, strings)])
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch, strict=False), strings, tlens, 3, 30, 5, (0, 0))
    assert status == [0, 0, 0, NONCONFORMING, 0]
    assert sr["aln_src"].tolist() == [0, 1, 3, 5] + [8, 9, 10, 12, 13, 14] + [20, 21, 22, 23]
    assert sr["aln_tgt"].tolist() == [0] * 4 + [2] * 6 + [4] * 4
    assert int(ps["site_begin"][4]) == int(ps["site_begin"][3])         # the non-conforming target: no sites, no entries


@pytest.mark.gpu
def test_the_aln_src_map_under_the_record_filter(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(13, 10, 150, 300)
    depth = 5
    probe = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        probe.set_record_filter(max_depth=depth)
        probe.consensus_cigar(capi.HostCigarBatch(**ct.records_to_arrays(targets)))
        fate = probe.record_stats()["fate"]
    finally:
        probe.close()
    assert (fate & capi.FATE_MAX_DEPTH).any()
    kept, src, i = [], [], 0
    for bb, recs in targets:
        kept.append((bb, [r for k, r in enumerate(recs) if not fate[i + k]]))
        src.append([i + k for k in range(len(recs)) if not fate[i + k]])
        i += len(recs)
    sr, ps, status, _, exp = _run(tes._whole(targets), tes._strings(kept), _tlens(targets), 3, 30, 5, (2, 200000),
                                  prepare=lambda c: c.set_record_filter(max_depth=depth), src=src)
    assert status == [0] * 10 and sr["aln_src"].size == 10 * depth
    assert sr["aln_src"].tolist() != list(range(10 * depth))            # (the filter left records out in the middle)


@pytest.mark.gpu
def test_every_way_in_gives_the_same_arrays(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(91, 12, 150, 400, full_span=True)
    strings = tes._strings(targets)
    tlens = _tlens(targets)
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
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    calls = {"strings": lambda c: c.consensus(sb),
             "plain": lambda c: c.consensus_cigar(plain), "packed": lambda c: c._intake(plain.packed(), None, plain, True),
             "stranded": lambda c: c._intake(capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), None, None, True),
             "cs": lambda c: c.consensus_cs(cs), "md": lambda c: c.consensus_cigar_md(capi.HostCigarBatch(**arr), md)}
    ref = None
    for kind, call in calls.items():
        got, pu, ps, sr, status, _ = _device(call, 3, 30, 5, (2, 200000))
        assert status == [0] * 12, kind
        if ref is None:
            ref = sr
            _check((pu, ps, sr), _expect(strings, tlens, 3, 30, 5, (2, 200000), 0, status))
            assert sr["ent_site"].size > 300 and sr["aln_src"].tolist() == list(range(n))
        for k in ref:
            assert np.array_equal(sr[k], ref[k]), (kind, k)


@pytest.mark.gpu
def test_consensus_pre_on_the_aligner_s_strings(oracle_lib):
    """dagcon_consensus_pre: the twin is fed the strings dagcon_align returns for the same pairs; aln_src is the record."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(7)
    targets, pairs, starts = [], [], []
    for ti in range(3):
        tlen = int(rng.integers(300, 400))
        target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
        recs = []
        for r in range(6):
            s = int(rng.integers(0, tlen // 5)); e = int(rng.integers(4 * tlen // 5, tlen + 1))
            if ti == 1 and r == 2:
                e = s + 60                                             # its alignment is below min_len 100
            tseq = target[s:e]
            qseq = bytearray()
            for ch in tseq:
                u = rng.random()
                if u < 0.04:
                    continue
                qseq.append(ch if u > 0.06 else b"ACGT"[rng.integers(0, 4)])
                if rng.random() < 0.06:
                    qseq.append(b"ACGT"[rng.integers(0, 4)])
            recs.append((s, b"+", bytes(qseq), tseq))
            pairs.append((bytes(qseq), tseq)); starts.append(s + 1)
        targets.append((tlen, recs))
    al = capi.Context(min_cov=3, min_len=100, trim=10)
    try:
        aligned = al.align(pairs)
    finally:
        al.close()
    strings, i = [], 0
    for tlen, recs in targets:
        strings.append((b"N" * tlen, [(starts[i + k], *aligned[i + k]) for k in range(len(recs))]))
        i += len(recs)
    sr, ps, status, _, exp = _run(lambda c: c.consensus_pre(targets), strings, [t for t, _ in targets], 3, 100, 10, (2, 200000))
    assert status == [0] * 3 and sr["aln_src"].tolist() == [k for k in range(18) if k != 8] and sr["ent_site"].size > 50


@pytest.mark.gpu
def test_windows_equal_the_twin_per_window(oracle_lib):
    """A window is a target of the pipeline; aln_src is the record of the piece."""
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(77, 8, 120, 120)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 40, 10)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    assert not any(f for _, _, f in per) and len(wins) == 24
    strings = [(targets[g][0][a:b], alns) for (g, a, b), (_, alns, _) in zip(wins, per)]
    first = np.concatenate([[0], np.cumsum([len(r) for _, r in targets])]).tolist()
    src = []
    for g, a, b in wins:
        bb, recs = targets[g]
        src.append([first[g] + k for k, (p, q, o) in enumerate(recs) if max(a, wt.span(p, len(bb), o)[0]) < min(b, wt.span(p, len(bb), o)[1])])
    assert [len(s) for s in src] == [len(alns) for _, alns in strings]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sr, ps, status, _, exp = _run(lambda c: c.consensus_cigar_windows(cb, hw), strings, [b - a for _, a, b in wins], 3, 30, 5, (2, 200000), src=src)
    assert sr["aln_tgt"].size > 60 and sr["ent_site"].size > 20


def _planted(seed=3, err=0.01):
    """Two haplotypes of a 600-base target that differ by a substitution every 40-60 bases and by one inserted base; 12
    full-span reads of each with a few random errors, the first 12 of the first.  The target is the first haplotype."""
    tes = _tes()
    rng = np.random.default_rng(seed)
    bb = tes._nonrep(rng, 600)
    subs, x = {}, int(rng.integers(20, 40))
    while x < 590:
        subs[x] = next(b for b in b"ACGT" if b != bb[x] and b != bb[x - 1] and b != bb[x + 1])
        x += int(rng.integers(40, 61))
    ins_at = 305
    assert ins_at not in subs and ins_at - 1 not in subs
    ins_base = next(b for b in b"ACGT" if b != bb[ins_at] and b != bb[ins_at - 1])
    alns, n_err = [], 0
    for k in range(24):
        second = k >= 12
        q, t = bytearray(), bytearray()
        for p in range(600):
            if second and p == ins_at:
                q.append(ins_base); t.append(GAP)
            b = subs[p] if second and p in subs else bb[p]
            if rng.random() < err and p not in subs and not ins_at - 2 <= p <= ins_at + 1:
                b = next(c for c in b"ACGT" if c != b); n_err += 1
            q.append(b); t.append(bb[p])
        alns.append((1, bytes(q), bytes(t)))
    return bb, alns, sorted(subs), ins_at, n_err


@pytest.mark.gpu
def test_the_split_a_planted_case(oracle_lib):
    bb, alns, subs, ins_at, n_err = _planted()
    assert len(subs) >= 10 and n_err >= 24
    # on the twin alone first: the planted groups come back exactly; the seed is a read of the first haplotype, so that is 1
    tw = srt.target(600, alns, 500, 50, (2, 200000))
    assert set(p for p in subs if 50 <= p < 550) <= set(tw["sites"]) and ins_at - 1 in tw["sites"]
    assert srt.kind(tw["counts"][ins_at - 1]) == ("ins",)
    assert tw["hap"] == [1] * 12 + [2] * 12 and all(v for v in tw["phase"])
    batch = batch_from_targets([(600, alns, None)])
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), [(bb, alns)], [600], 6, 500, 50, (2, 200000))
    assert status == [0] and sr["hap"].tolist() == [1] * 12 + [2] * 12


def _chain():
    """12 reads of 40 bases, read i over [20 i, 20 i + 40): it overlaps reads i - 1 and i + 1 alone.  In the overlap of
    reads i and i + 1 the later read has one wrong base, the only sites at 1 / 200000; read 0 has one of them, reads 1
    to 10 two, so the seed is read 1 and read k is k - 1 hops from it."""
    tes = _tes()
    bb = tes._nonrep(np.random.default_rng(12), 260)
    alns = []
    for i in range(12):
        s = 20 * i
        q = bytearray(bb[s:s + 40])
        if i:
            q[10] = next(b for b in b"ACGT" if b not in (bb[s + 9], bb[s + 10], bb[s + 11]))
        alns.append((s + 1, bytes(q), bytes(bb[s:s + 40])))
    return bb, alns


@pytest.mark.gpu
def test_the_split_hops(oracle_lib):
    bb, alns = _chain()
    tw = srt.target(260, alns, 30, 0, (1, 200000), 3)
    assert tw["sites"] == [20 * i + 10 for i in range(1, 12)] and tw["signed"] == [1] + [2] * 10 + [1]
    # reads further than 3 hops from read 1 are 0, in the twin
    assert [bool(h) for h in tw["hap"]] == [True] * 5 + [False] * 7
    assert all(srt.target(260, alns, 30, 0, (1, 200000), 64)["hap"])
    batch = batch_from_targets([(260, alns, None)])
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), [(bb, alns)], [260], 1, 30, 0, (1, 200000), rounds=3)
    assert [bool(h) for h in sr["hap"].tolist()] == [True] * 5 + [False] * 7
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), [(bb, alns)], [260], 1, 30, 0, (1, 200000), rounds=64)
    assert all(sr["hap"].tolist()) and sr["hap"].tolist() == [2, 1] * 6
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), [(bb, alns)], [260], 1, 30, 0, (1, 200000))     # the default: 8
    assert [bool(h) for h in sr["hap"].tolist()] == [True] * 10 + [False] * 2


@pytest.mark.gpu
def test_the_split_degenerate_cases(oracle_lib):
    """A target without an informative site beside one with sites: by rule 3 every site has signed entries (its largest
    class), so a target has no informative site exactly when it has no site; its alignments are numbered and stay 0.
    Then thresholds that list no site at all: n_aln alignments, no entries.  And phase off: no hap, no phase."""
    strings = [_piles(5, 40), _piles(0, 40), _piles(2, 40)]
    batch = batch_from_targets([(40, alns, None) for _, alns in strings])
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), strings, [40] * 3, 3, 30, 0, (2, 200000))
    assert np.diff(ps["site_begin"]).tolist() == [5, 0, 2]
    assert sr["hap"].tolist() == [1, 1, 1, 2, 2, 2] + [0] * 6 + [1, 1, 1, 2, 2, 2] and sr["aln_tgt"].tolist() == [0] * 6 + [1] * 6 + [2] * 6
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), strings, [40] * 3, 3, 30, 0, (4, 200000))
    assert ps["pos"].size == 0 and sr["aln_tgt"].size == 18 and sr["ent_site"].size == 0 and sr["ent_begin"].tolist() == [0] * 19
    assert not sr["hap"].any() and sr["phase"].size == 0
    sr, ps, status, _, exp = _run(lambda c: c.consensus(batch), strings, [40] * 3, 3, 30, 0, (2, 200000), phase=False)
    assert sr["ent_site"].size == 6 * 7


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    plain = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        want = plain.consensus_cigar(cb)
        plain.set_pileup(2, 200000)
        assert plain.consensus_cigar(cb) == want
        want_ps, want_pu = plain.pileup_sites(), plain.pileup()
        assert _code(plain.site_reads) == STATE                      # a context that never heard of the switch
    finally:
        plain.close()
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        assert _code(c.site_reads) == STATE                          # nothing yet
        c.set_site_reads(True)
        assert c.consensus_cigar(cb) == want                         # the pile-up off at the upload: as a plain context
        assert _code(c.site_reads) == STATE and _code(c.pileup_sites) == STATE
        c.set_site_reads(None)
        c.set_pileup(2, 200000)
        assert c.consensus_cigar(cb) == want
        c.set_site_reads(True)                                       # set after the upload
        assert _code(c.site_reads) == STATE
        assert _code(lambda: c.set_site_reads(True, 65)) == INVALID  # refused: the switch stays as it was
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.site_reads) == STATE                          # before a fetch
        assert c.fetch() == want
        first = c.site_reads()
        assert first["ent_site"].size > 0 and first["hap"].any()
        again = c.site_reads()                                       # asked twice
        assert all(np.array_equal(first[k], again[k]) for k in first)
        c.set_site_reads(True, 64)
        c.set_site_reads(False)                                      # on, without the split
        assert c.consensus_cigar(cb) == want
        nophase = c.site_reads()
        assert nophase["hap"] is None and nophase["phase"] is None and np.array_equal(nophase["ent_code"], first["ent_code"])
        c.set_site_reads(None)                                       # off again: consensus, sites and counts byte for byte
        assert np.array_equal(c.site_reads()["ent_site"], first["ent_site"])    # (this batch's results stay)
        assert c.consensus_cigar(cb) == want
        assert _code(c.site_reads) == STATE
        ps, pu = c.pileup_sites(), c.pileup()
        assert all(np.array_equal(ps[k], want_ps[k]) for k in ps) and all(np.array_equal(pu[k], want_pu[k]) for k in pu)
    finally:
        c.close()
    stop = capi.Context(min_cov=3, min_len=30, trim=5, flags=capi.FLAG_STOP_AFTER_MERGE)
    try:
        stop.set_pileup(2, 200000); stop.set_site_reads(True)
        stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
        assert _code(stop.site_reads) == STATE
    finally:
        stop.close()


@pytest.mark.gpu
def test_pbdagcon_site_reads_and_haplotag(oracle_lib, tmp_path):
    tes = _tes()
    targets = tes._variant_targets(101, 8, 150, 300, full_span=True)
    names = ["ctg%d" % i for i in range(8)]
    tl = _tlens(targets)
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [r for _, r in targets]))
    strings = tes._strings(targets)
    m5 = tmp_path / "in.m5"
    from pbdagcon_amd import synth
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    sb.ids = names
    m5.write_bytes(synth.to_m5(sb))
    f = {k: tmp_path / k for k in ("r", "h", "s", "r2", "h2", "r3", "h3")}
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    rec = ["--sam", "--ref", str(ref)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r

    def lines(opts, qname):
        reads, tags, sites = [], [], []
        for g, (bb, alns) in enumerate(strings):
            tw = srt.target(tl[g], alns, 30, 5, opts)
            for k, p in enumerate(tw["sites"]):
                sites.append(pt.line(names[g], p, bb[p], tw["counts"][p]))
                for i, e in zip(tw["src"], tw["ents"]):
                    reads += [srt.site_reads_line(names[g], p, qname(g, i, alns[i]), c) for kk, c in e if kk == k]
            tags += [srt.haplotag_line(names[g], qname(g, i, alns[i]), h, n) for i, h, n in zip(tw["src"], tw["hap"], tw["signed"])]
        return reads, tags, sites
    sam_name = lambda g, i, aln: "q%d_%d" % (g, i)
    m5_name = lambda g, i, aln: "q%07d_%d/0_%d" % (g, i, sum(1 for ch in aln[1] if ch != GAP))
    plain = run(*rec, str(sam))
    got = run(*rec, "--site-reads", str(f["r"]), "--haplotag", str(f["h"]), "--sites", str(f["s"]), str(sam))
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 8
    reads, tags, sites = lines((2, 200000), sam_name)
    assert f["r"].read_text().splitlines() == reads and len(reads) > 200
    assert f["h"].read_text().splitlines() == tags and len(tags) == sum(len(a) for _, a in strings)
    assert f["s"].read_text().splitlines() == sites and {t.split("\t")[2] for t in tags} >= {"1", "2"}
    # the .m5 of the same alignments, other thresholds, no --sites, two batches, two parsing threads
    got = run("--site-reads", str(f["r2"]), "--haplotag", str(f["h2"]), "--site-min-frac", "0.3", "--site-min-count", "3", "--batch-targets", "5",
              "-j", "2", str(m5))
    assert got.stdout == run(str(m5)).stdout
    reads, tags, _ = lines((3, 300000), m5_name)
    assert f["r2"].read_text().splitlines() == reads and len(reads) > 100 and f["h2"].read_text().splitlines() == tags
    # one flag alone; --haplotag alone turns the split on
    run(*rec, "--haplotag", str(f["h3"]), str(sam)); run(*rec, "--site-reads", str(f["r3"]), str(sam))
    assert f["h3"].read_bytes() == f["h"].read_bytes() and f["r3"].read_bytes() == f["r"].read_bytes()
