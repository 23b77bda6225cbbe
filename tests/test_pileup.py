"""Per-position allele counts (dagcon_set_pileup, pbdagcon --pileup / --sites): the rule by hand and the twin's invariants
on the CPU, the device against the twin field for field on the GPU.  include/dagcon.h states the rule; pileup_twin.py is it
in Python."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import evidence_twin as ev
import md_files as mf
import md_twin as mt
import paf_files as pf
import pileup_twin as pt
import window_twin as wt
from util import batch_from_targets, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID, NONCONFORMING = -8, -1, -4
GAP = 0x2D


def _tes():
    import test_edit_support as tes
    return tes


def _cli():
    return _tes()._cli()


def _n(**kw):
    """A position's eight counts from names."""
    n = [0] * 8
    for k, v in kw.items():
        n[getattr(pt, k)] = v
    return n


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def test_the_rule_by_hand(oracle_lib):
    def counts(tlen, alns, min_len=1, trim=0):
        return pt.target_counts(tlen, alns, min_len, trim)
    # a substitution: normalizeGaps writes a mismatch as the target base dropped and the read base inserted behind it
    assert counts(4, [(1, b"ACGT", b"AGGT")]) == [_n(A=1), _n(DEL=1, INS=1), _n(G=1), _n(T=1)]
    # lower case counts with upper case
    assert counts(4, [(1, b"acgt", b"acgt"), (1, b"ACGT", b"ACGT")]) == [_n(A=2), _n(C=2), _n(G=2), _n(T=2)]
    # a foreign byte goes to N
    assert counts(4, [(1, b"ANGT", b"ANGT"), (1, b"A*GT", b"A*GT")]) == [_n(A=2), _n(N=2), _n(G=2), _n(T=2)]
    # a deletion
    assert counts(4, [(1, b"A-GT", b"ACGT")]) == [_n(A=1), _n(DEL=1), _n(G=1), _n(T=1)]
    # an insertion run of three is counted once, at the base in front of it
    assert counts(3, [(1, b"ATTTCG", b"A---CG")]) == [_n(A=1, INS=1), _n(C=1), _n(G=1)]
    # two runs behind two bases
    assert counts(3, [(1, b"ATCTG", b"A-C-G")]) == [_n(A=1, INS=1), _n(C=1, INS=1), _n(G=1)]
    # a leading inserted column counts nowhere
    assert counts(3, [(1, b"TACG", b"-ACG")]) == [_n(A=1), _n(C=1), _n(G=1)]
    # a read that begins at base 5 (start is 1-based)
    assert counts(8, [(5, b"ACG", b"ACG")]) == [_n()] * 4 + [_n(A=1), _n(C=1), _n(G=1), _n()]
    # an alignment below min_len is not counted
    assert counts(4, [(1, b"ACG", b"ACG"), (1, b"ACGT", b"ACGT")], min_len=4) == [_n(A=1), _n(C=1), _n(G=1), _n(T=1)]
    # trimAln takes `trim` target bases off either end first
    got = counts(6, [(1, b"ACGTAC", b"ACGTAC")], trim=1)
    (s0, q, t), = ev.columns([(1, b"ACGTAC", b"ACGTAC")], 1, 1)
    assert s0 >= 1 and len(t) <= 4
    assert got[0] == _n() and got[5] == _n() and sum(pt.depth(n) for n in got) == len(t) and got[s0] == _n(**{chr(b"ACGTAC"[s0]): 1})
    # INS <= depth: the anchor of a run is a target-base column of the same alignment
    assert all(n[pt.INS] <= pt.depth(n) for n in counts(3, [(1, b"ATCTG", b"A-C-G")] * 3 + [(1, b"ACG", b"ACG")]))


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    rng = np.random.default_rng(78)
    n_cols = n_runs = n_lead = n_del = n_multi = 0
    for k in range(1500):
        alns, bb = _tes()._small_pileup(rng, k)
        trim = int(rng.integers(0, 3))
        counts = pt.target_counts(len(bb), alns, 4, trim)
        cols = runs = 0
        for s0, q, t in ev.columns(alns, 4, trim):
            cols += sum(1 for x in t if x != GAP)
            seen_base, i = False, 0
            while i < len(t):
                if t[i] == GAP and q[i] != GAP:
                    j = i
                    while j < len(t) and t[j] == GAP and q[j] != GAP:
                        j += 1
                    runs += seen_base
                    n_lead += not seen_base
                    n_multi += j - i >= 2
                    i = j
                    continue
                seen_base = seen_base or t[i] != GAP
                i += 1
        assert sum(pt.depth(n) for n in counts) == cols
        assert sum(n[pt.INS] for n in counts) == runs
        assert all(n[pt.INS] <= pt.depth(n) and n[7] == 0 for n in counts)
        n_cols += cols; n_runs += runs; n_del += sum(n[pt.DEL] for n in counts)
    print("target-base columns %d, insertion runs with an anchor %d (two columns or more: %d), leading runs %d, deletions %d"
          % (n_cols, n_runs, n_multi, n_lead, n_del))
    assert n_cols >= 100000 and n_runs >= 10000 and n_multi >= 2000 and n_lead >= 300 and n_del >= 5000


def test_the_site_rule_by_hand():
    site = pt.is_site
    # s2 is the second largest of the six, ties as they fall
    assert site(_n(A=3, C=3), 3, 500000) and not site(_n(A=3, C=3), 4, 0)
    assert site(_n(A=5, G=2, DEL=2), 2, 0) and not site(_n(A=5, G=2, DEL=2), 3, 0)
    assert site(_n(A=5, DEL=4), 4, 0) and site(_n(N=2, T=7), 2, 0)
    assert not site(_n(A=9), 1, 0)
    # the insertion allele alone makes a site
    assert site(_n(A=10, INS=4), 4, 400000) and not site(_n(A=10, INS=4), 5, 0)
    # min(INS, depth - INS): every read inserting is no second allele
    assert not site(_n(A=10, INS=10), 1, 0) and site(_n(A=10, INS=7), 3, 0) and not site(_n(A=10, INS=7), 4, 0)
    # the ppm boundary exactly: 1 of 4
    assert site(_n(A=3, C=1), 1, 250000) and not site(_n(A=3, C=1), 1, 250001)
    # 0 / 0 lists every position with depth, and only those
    counts = [_n(A=4), _n(), _n(DEL=1), _n(A=2, C=2, INS=1)]
    assert pt.sites(counts, 0, 0) == [0, 2, 3] and pt.sites(counts, 1, 0) == [3] and pt.sites(counts, 2, 1000000) == []
    assert pt.sites(counts, 2, 500000) == [3] and pt.sites(counts, 2, 500001) == []


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    names = ("dagcon_set_pileup", "dagcon_fetch_pileup", "dagcon_fetch_pileup_sites")
    lib = capi.load()
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(dagcon_pileup_opts), '
            'sizeof(dagcon_pileup), sizeof(dagcon_pileup_sites)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert [ctypes.sizeof(x) for x in (capi.PileupOpts, capi.Pileup, capi.PileupSites)] == [int(x) for x in out]
    for m in ("set_pileup", "pileup", "pileup_sites"):
        assert callable(getattr(capi.Context, m))


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    pu, st = tmp_path / "o.pileup", tmp_path / "o.sites"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for args in ([str(m5), "--pileup"], [str(m5), "--sites"],
                 ["--pileup", str(pu), "--site-min-frac", "0.3", str(m5)], ["--pileup", str(pu), "--site-min-count", "3", str(m5)],
                 ["--site-min-count", "3", str(m5)],
                 ["--sites", str(st), "--site-min-frac", "1.5", str(m5)], ["--sites", str(st), "--site-min-frac", "0.1234567", str(m5)],
                 ["--sites", str(st), "--site-min-count", "x", str(m5)],
                 ["-a", "--polish", "1", "--pileup", str(pu), str(m5)], ["-a", "--polish", "1", "--sites", str(st), str(m5)],
                 rec + ["--dump-parsed", "--pileup", str(pu), str(sam)], rec + ["--dump-parsed", "--sites", str(st), str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not pu.exists() and not st.exists()
    # a file that cannot be written is said before anything runs
    for flag in ("--pileup", "--sites"):
        out = run(*rec, flag, str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr, flag
    h = run("--help")
    assert h.returncode == 0
    for flag in (b"--pileup FILE", b"--sites FILE"):
        assert flag in h.stdout
    text = h.stdout.split(b"\n  --pileup FILE")[1].split(b"\n  --fastq")[0]
    assert b"parity unpinned" in text and b"RNAME POS REF DEPTH A C G T N DEL INS" in text
    assert b"--site-min-frac F (default 0.2" in text and b"--site-min-count N (default 2)" in text and b"own choice" in text


_PILE_MAIN = r"""
#include <iostream>
#include "pileup.h"
// stdin: "name pos0 ref n0 .. n7" per line ('.' for no ref byte); stdout: the lines
int main() {
    std::string out, name, ref;
    unsigned long long pos;
    unsigned v[8];
    while (std::cin >> name >> pos >> ref >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6] >> v[7]) {
        uint16_t n[8];
        for (int k = 0; k < 8; k++) n[k] = (uint16_t)v[k];
        dg_pileup_line(out, name, pos, ref == "." ? (char)0 : ref[0], n);
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatter_against_python(tmp_path):
    src = tmp_path / "pile_main.cpp"; src.write_text(_PILE_MAIN)
    exe = tmp_path / "pile_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    cases = [("ctg", 0, ord("A"), _n(A=4)), ("ctg", 41, ord("c"), _n(A=1, C=2, G=3, T=4, N=5, DEL=6, INS=7)),
             ("a/b|c", 4294967295, None, _n(DEL=4094, INS=4094)), ("x", 9, ord("N"), _n(A=4094, C=4094, G=4094, T=4094, N=4094, DEL=4094))]
    text = "".join("%s %d %s %s\n" % (name, pos, chr(ref) if ref is not None else ".", " ".join(map(str, n))) for name, pos, ref, n in cases)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert out == [pt.line(*c) for c in cases]
    assert out[0] == "ctg\t1\tA\t4\t4\t0\t0\t0\t0\t0\t0" and out[2].split("\t")[1:4] == ["4294967296", ".", "4094"]
    assert out[3].split("\t")[3] == str(6 * 4094)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _twin(strings, tlens, min_cov, min_len, trim, status=None):
    """Per target the twin's counts ([tlen, 8] uint16): zero for a target that failed, has a non-conforming record, or
    has fewer than min_cov alignments (no graph is built for it)."""
    out = []
    for k, (s, tl) in enumerate(zip(strings, tlens)):
        if s is None or (status is not None and status[k]) or len(s[1]) < max(1, min_cov):
            out.append(np.zeros((tl, 8), np.uint16))
        else:
            out.append(np.array(pt.target_counts(tl, s[1], min_len, trim), np.uint16).reshape(tl, 8))
    return out


def _code(f):
    from pbdagcon_amd import capi
    with pytest.raises(capi.DagconError) as e:
        f()
    return e.value.code


def _run(call, strings, tlens, min_cov, min_len, trim, opts=(0, 0), prepare=None, flags=0, check=True):
    """call(ctx) -> results.  One context with the switch off, one with it on: the same consensus; counts and sites equal
    the twin's field for field, the sites also sites() of the device's own counts.  (counts per target, sites per target,
    status, re-runs)"""
    from pbdagcon_amd import capi
    off = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=flags)
    on = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=flags)
    try:
        for c in (off, on):
            if prepare:
                prepare(c)
        on.set_pileup(*opts)
        got_off = call(off)
        assert _code(off.pileup) == STATE and _code(off.pileup_sites) == STATE
        got = call(on)
        ps, pu = on.pileup_sites(), on.pileup()            # (the sites came with the fetch, the counts come when asked)
        status = on.target_status.tolist()
        reruns = on.timings()["reruns"]
    finally:
        off.close(); on.close()
    assert got == got_off
    T = len(tlens)
    assert pu["pos_begin"].tolist() == np.concatenate([[0], np.cumsum(tlens)]).tolist() and pu["counts"].shape == (sum(tlens), 8)
    assert ps["site_begin"].size == T + 1 and ps["pos"].size == ps["counts"].shape[0] == int(ps["site_begin"][T])
    counts = [pu["counts"][int(pu["pos_begin"][t]):int(pu["pos_begin"][t + 1])] for t in range(T)]
    sites = [(ps["pos"][int(ps["site_begin"][t]):int(ps["site_begin"][t + 1])].tolist(),
              ps["counts"][int(ps["site_begin"][t]):int(ps["site_begin"][t + 1])]) for t in range(T)]
    for t in range(T):
        pos, cn = sites[t]
        assert pos == pt.sites(counts[t], *opts), t                      # the device's list on the device's own counts
        assert np.array_equal(cn, counts[t][pos]), t
    if check:
        want = _twin(strings, tlens, min_cov, min_len, trim, status)
        for t in range(T):
            assert np.array_equal(counts[t], want[t]), (t, np.argwhere(counts[t] != want[t])[:5].tolist())
            assert sites[t][0] == pt.sites(want[t], *opts), t
    return counts, sites, status, reruns


def _tlens(targets):
    return [len(bb) for bb, _ in targets]


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 2])
def test_random_small_targets(oracle_lib, trim):
    """300 small targets in one batch, one with a non-conforming record: all zero and no sites for it."""
    tes = _tes()
    rng = np.random.default_rng(300 + trim)
    targets = []
    for k in range(300):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns, eqx=True)))
    bad = 150
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = tes._strings(targets)
    assert strings[bad] is None and sum(s is None for s in strings) == 1
    counts, sites, status, _ = _run(tes._whole(targets), strings, _tlens(targets), 3, 4, trim, opts=(2, 200000))
    assert status[bad] == NONCONFORMING and sum(1 for s in status if s) == 1
    assert not counts[bad].any() and sites[bad][0] == []
    tot = np.concatenate(counts).astype(np.int64).sum(axis=0)
    print("A C G T N DEL INS 0: %s, sites %d" % (tot.tolist(), sum(len(p) for p, _ in sites)))
    assert tot[:4].min() > 1000 and tot[pt.DEL] > 1000 and tot[pt.INS] > 1000 and tot[7] == 0
    assert sum(len(p) for p, _ in sites) > 300


def _lane_reads(rng, bb, P):
    """Hand-built reads on a target without equal neighbours, so that normalizeGaps moves nothing: what each puts at
    columns 63 / 64 of its alignment is in the name."""
    tes = _tes()
    L = len(bb)

    def other(*avoid):
        return next(b for b in b"ACGT" if b not in avoid)

    def read(s, e, ins_at=None, n_ins=2, del_at=None, lead=0):
        q, t = bytearray(), bytearray()
        for _ in range(lead):
            q.append(other(bb[s])); t.append(GAP)
        for x in range(s, e):
            if x == ins_at:
                a = other(bb[x], bb[x - 1])
                for k in range(n_ins):
                    q.append(a if k % 2 == 0 else other(bb[x], a)); t.append(GAP)
            if x == del_at:
                q.append(GAP); t.append(bb[x]); continue
            q.append(bb[x]); t.append(bb[x])
        return (s + 1, bytes(q), bytes(t))
    reads = {"run over 63|64": read(P - 63, L, ins_at=P), "anchor 63, run at 0": read(P - 64, L, ins_at=P),
             "run at 1": read(P - 65, L, ins_at=P), "deletion at 63": read(P - 63, L, del_at=P),
             "deletion at 0": read(P - 64, L, del_at=P), "last base at 63": read(P - 64, P), "last base at 0": read(P - 64, P + 1),
             "first base at 63": read(P, L, lead=63), "first base at 0 of the next step": read(P, L, lead=64)}
    plain = [read(0, L) for _ in range(3)]
    return reads, bb, tes._records(bb, list(reads.values()) + plain)


@pytest.mark.gpu
def test_the_64_column_period(oracle_lib):
    tes = _tes()
    rng = np.random.default_rng(64)
    targets, seen = [], set()
    for P in (80, 100, 127, 128, 129):
        reads, bb, recs = _lane_reads(rng, tes._nonrep(rng, P + 150), P)
        targets.append((bb, recs))
    strings = tes._strings(targets)
    # on the CPU first: the input is what it is meant to be
    for (bb, alns), P in zip(strings, (80, 100, 127, 128, 129)):
        cols = ev.columns(alns, 30, 0)
        assert len(cols) == len(alns)
        here = set()
        for s0, q, t in cols:
            tb = [i for i in range(len(t)) if t[i] != GAP]
            here.add(("first", tb[0] % 64)); here.add(("last", tb[-1] % 64))
            for i in range(1, len(t)):
                if t[i] == GAP and t[i - 1] != GAP:
                    j = i
                    while j < len(t) and t[j] == GAP:
                        j += 1
                    here.add(("run", i % 64, (i - 1) % 64, i // 64 != (j - 1) // 64))
                if q[i] == GAP:
                    here.add(("del", i % 64))
        assert {("run", 63, 62, True), ("run", 0, 63, False), ("del", 0), ("del", 63), ("first", 0), ("first", 63),
                ("last", 0), ("last", 63)} <= here, (P, sorted(here))
        seen |= here
    counts, sites, status, _ = _run(tes._whole(targets), strings, _tlens(targets), 3, 30, 0)
    assert status == [0] * 5
    for c, P in zip(counts, (80, 100, 127, 128, 129)):
        assert int(c[P - 1][pt.INS]) == 3 and int(c[P][pt.DEL]) == 2 and int(c[:, pt.INS].sum()) == 3


@pytest.mark.gpu
def test_depth_and_packing(oracle_lib):
    """One target of 120 bases under 700 reads; every read is its own target string, so both letters of a packed word
    stand at one position: A and C at the even positions, G and T at the odd ones, N and DEL at position 60, where 300
    reads drop the base and 300 of the others insert behind it.  Both halves of every word exceed 255 at once.  That 4094
    fits is by the argument in include/dagcon.h, not by a run."""
    from pbdagcon_amd import capi
    tl = 120
    alns = []
    for k in range(700):
        first = k < 350
        q, t = bytearray(), bytearray()
        for x in range(tl):
            b = (ord("A") if first else ord("C")) if x % 2 == 0 else (ord("G") if first else ord("T"))
            if x == 60:
                if 200 <= k < 500:
                    q.append(GAP); t.append(ord("A") if first else ord("C")); continue
                b = ord("N")
            q.append(b); t.append(b)
            if x == 60 and (k < 150 or k >= 550):
                q.append(ord("A")); t.append(GAP)
        alns.append((1, bytes(q), bytes(t)))
    strings = [(b"N" * tl, alns)]
    # on the CPU first
    want = pt.target_counts(tl, alns, 30, 0)
    for x in range(tl):
        if x == 60:
            assert want[x] == _n(N=400, DEL=300, INS=300)
        else:
            assert want[x] == (_n(A=350, C=350) if x % 2 == 0 else _n(G=350, T=350))
    batch = batch_from_targets([(tl, alns, None)])
    counts, sites, status, _ = _run(lambda c: c.consensus(batch), strings, [tl], 3, 30, 0, opts=(300, 400000))
    assert status == [0]
    assert sites[0][0] == list(range(tl))                           # 350 of 700, and 300 of 700 at position 60
    assert int(counts[0].max()) == 400 and not counts[0][:, 7].any()


def _redo_target(rng):
    """The input of test_edit_support.test_an_alignment_on_the_redo_path."""
    tes = _tes()
    tl = 900
    alns, bb = random_target(rng, tl, 8, alphabet=b"ACGT", full_span=True, sub=0.02, ins=0.08, dele=0.04)
    bbs = bytearray(bb)
    bbs[300:520] = b"A" * 220
    bb = bytes(bbs)
    alns = [(s, q, tes._retarget(s, t, bb)) for s, q, t in alns]
    extra = []
    for k in range(6):
        q, t = bytearray(), bytearray()
        for i in range(tl):
            if k % 3 == 0 and i == 200:
                n_ins = 300 if k == 0 else 700
                ins = bytes(b"ACGT"[j] for j in rng.integers(0, 4, n_ins))
                q += ins; t += b"-" * n_ins
            if k % 3 == 1 and 600 <= i < 850:
                q.append(GAP); t.append(bb[i]); continue
            if k % 3 == 2 and i == 299:
                q += b"A" * 3; t += b"-" * 3
            q.append(bb[i]); t.append(bb[i])
        extra.append((1, bytes(q), bytes(t)))
    alns2 = [(1, bytes(bb[i] if rng.random() > 0.05 else GAP for i in range(tl)), bb) for _ in range(3)]
    return bb, tes._records(bb, alns + extra + alns2)


@pytest.mark.gpu
def test_an_alignment_on_the_redo_path(oracle_lib):
    tes = _tes()
    targets = [_redo_target(np.random.default_rng(21))]
    strings = tes._strings(targets)
    assert strings[0] is not None
    counted = ev.columns(strings[0][1], 500, 50)
    long_ = [(s0, q, t) for s0, q, t in counted if sum(1 for c in t if c == GAP) >= 700]
    assert len(long_) == 1
    s0, q, t = long_[0]
    tcs, _ = ev.coords(s0, t)
    # (normalizeGaps slides inserted bases that equal the target base behind them: the 700 columns are several runs)
    anchors = [tcs[i] - 1 for i in range(1, len(t)) if t[i] == GAP and q[i] != GAP and t[i - 1] != GAP]
    assert len(anchors) >= 2
    runs = [len(r) for r in "".join("-" if x == GAP else "x" for x in t).split("x") if r]
    assert max(runs) >= 64 and sum(runs) >= 700                     # a run longer than a step of 64 columns
    counts, sites, status, _ = _run(tes._whole(targets), strings, _tlens(targets), 6, 500, 50)
    assert status == [0]
    want = pt.target_counts(900, strings[0][1], 500, 50)
    for a in anchors:                                               # INS at its anchors
        assert int(counts[0][a][pt.INS]) == want[a][pt.INS] >= 1
    # its bases everywhere: it spans the target, so the deepest positions count every alignment
    assert int(counts[0][:, :6].sum(axis=1).max()) == len(counted)


@pytest.mark.gpu
def test_every_way_in_gives_the_same_arrays(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(91, 20, 150, 400, full_span=True)
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
        counts, sites, status, _ = _run(call, strings, tlens, 3, 30, 5, opts=(2, 200000))
        assert status == [0] * 20, kind
        flat = (np.concatenate(counts).tolist(), [p for p, _ in sites])
        if ref is None:
            ref = flat
            assert sum(len(p) for p, _ in sites) > 50
        assert flat == ref, kind


@pytest.mark.gpu
def test_consensus_pre_counts_on_the_aligner_s_strings(oracle_lib):
    """dagcon_consensus_pre: the twin is fed the strings dagcon_align returns for the same pairs ('+' strand)."""
    from pbdagcon_amd import capi
    import oracle
    rng = np.random.default_rng(7)
    targets, pairs, starts = [], [], []
    for ti in range(4):
        tlen = int(rng.integers(600, 900))
        target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
        recs = []
        for r in range(7):
            s = int(rng.integers(0, tlen // 5)); e = int(rng.integers(4 * tlen // 5, tlen + 1))
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
    assert all(len(q) == len(t) >= 400 for _, alns in strings for _, q, t in alns)
    counts, sites, status, _ = _run(lambda c: c.consensus_pre(targets), strings, [t for t, _ in targets], 3, 100, 10, opts=(2, 200000))
    assert status == [0] * 4 and sum(int(c.sum()) for c in counts) > 10000


@pytest.mark.gpu
def test_windows_equal_the_twin_per_window(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(77, 20, 120, 120)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 40, 10)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    assert not any(f for _, _, f in per) and len(wins) == 60
    strings = [(targets[g][0][a:b], alns) for (g, a, b), (_, alns, _) in zip(wins, per)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    counts, sites, status, _ = _run(lambda c: c.consensus_cigar_windows(cb, hw), strings, [b - a for _, a, b in wins], 3, 30, 5, opts=(2, 200000))
    assert sum(1 for c in counts if c.any()) > 40 and sum(len(p) for p, _ in sites) > 20


@pytest.mark.gpu
def test_record_filter_left_out_records_are_not_counted(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(13, 15, 150, 300)
    depth = 5
    assert all(len(recs) > depth for _, recs in targets)
    probe = capi.Context(min_cov=3, min_len=30, trim=5)
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
    counts, sites, status, _ = _run(tes._whole(targets), tes._strings(kept), _tlens(targets), 3, 30, 5,
                                    prepare=lambda c: c.set_record_filter(max_depth=depth))
    deepest = max(int(c[:, :6].sum(axis=1).max()) for c in counts)
    assert deepest == depth


def _two_letter_piles(n, tl, same=False):
    """n targets of tl bases under 6 reads, every read its own target string: three read A everywhere and three read C
    (same: all six read A)."""
    out = []
    for _ in range(n):
        alns = [(1, (b"A" if same or k < 3 else b"C") * tl, (b"A" if same or k < 3 else b"C") * tl) for k in range(6)]
        out.append((b"N" * tl, alns))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("min_count", [0, 1, 3])
def test_sites_over_the_thresholds(oracle_lib, min_count):
    tes = _tes()
    rng = np.random.default_rng(800 + min_count)
    targets = []
    for k in range(60):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns)))
    strings = tes._strings(targets)
    n_sites = []
    for ppm in (0, 1, 250000, 500000, 1000000):
        counts, sites, status, _ = _run(tes._whole(targets), strings, _tlens(targets), 3, 4, 0, opts=(min_count, ppm))
        n_sites.append(sum(len(p) for p, _ in sites))
    print("min_count %d: sites %s" % (min_count, n_sites))
    assert n_sites == sorted(n_sites, reverse=True) and n_sites[0] > n_sites[3] > 0 == n_sites[4]
    if min_count == 0:
        assert n_sites[0] == int((np.concatenate(counts)[:, :6].sum(axis=1) > 0).sum())     # 0 / 0: every position with depth


@pytest.mark.gpu
def test_every_position_a_site_crosses_the_arena_and_counts_stay(oracle_lib):
    """40 targets of 60 bases, three reads A and three reads C everywhere: at 0 / 0 (and at 3 / 500000) every position is
    a site, 2,400 of them in an arena whose first size is 2,400 / 8 + 1,024: the batch runs again with a larger one, and
    the counts of that second execution are still the twin's, not twice them."""
    n, tl = 40, 60
    strings = _two_letter_piles(n, tl)
    batch = batch_from_targets([(tl, alns, None) for _, alns in strings])
    assert n * tl > n * tl // 8 + 1024
    for opts in ((0, 0), (3, 500000)):
        counts, sites, status, reruns = _run(lambda c: c.consensus(batch), strings, [tl] * n, 3, 30, 0, opts=opts)
        assert status == [0] * n and reruns >= 1
        assert all(p == list(range(tl)) for p, _ in sites)
        assert all((c == np.array(_n(A=3, C=3), np.uint16)).all() for c in counts)
    # identical reads: no second allele anywhere, and no re-run either
    same = _two_letter_piles(n, tl, same=True)
    batch2 = batch_from_targets([(tl, alns, None) for _, alns in same])
    counts, sites, status, reruns = _run(lambda c: c.consensus(batch2), same, [tl] * n, 3, 30, 0, opts=(1, 1))
    assert reruns == 0 and all(p == [] for p, _ in sites) and all((c == np.array(_n(A=6), np.uint16)).all() for c in counts)


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sb = batch_from_targets([(len(bb), [ct.expand(p, q, bb, o) for p, q, o in recs], None) for bb, recs in targets])
    n_pos = sum(_tlens(targets))
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        assert _code(c.pileup) == STATE and _code(c.pileup_sites) == STATE       # nothing yet
        assert _code(lambda: c.set_pileup(2, 1000001)) == INVALID
        c.consensus_cigar(cb)
        assert _code(c.pileup) == STATE and _code(c.pileup_sites) == STATE       # the switch off at the upload
        c.set_pileup(2, 200000)
        assert _code(c.pileup) == STATE                              # on now, but the batch was uploaded without it
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.pileup) == STATE and _code(c.pileup_sites) == STATE       # before a fetch
        c.fetch()
        first = c.pileup()["counts"]
        n_sites = c.pileup_sites()["pos"].size
        assert first.shape == (n_pos, 8) and first.any() and n_sites > 0
        assert np.array_equal(c.pileup()["counts"], first)           # asked twice
        assert _code(lambda: c.set_pileup(2, 1000001)) == INVALID    # refused: the switch stays as it was
        c.consensus(sb)                                              # dagcon_consensus after a record upload: the same alignments
        assert np.array_equal(c.pileup()["counts"], first) and c.pileup_sites()["pos"].size == n_sites
        c.set_pileup(0, 0)                                           # the thresholds are read at the upload
        assert c.pileup_sites()["pos"].size == n_sites
        c.consensus_cigar(cb)
        assert c.pileup_sites()["pos"].size == int((first[:, :6].sum(axis=1) > 0).sum()) > n_sites
        c.set_pileup(None)
        assert np.array_equal(c.pileup()["counts"], first)           # off for the next upload; this batch's results stay
        c.consensus_cigar(cb)
        assert _code(c.pileup) == STATE and _code(c.pileup_sites) == STATE
        c.set_pileup()
        c.consensus(sb)
        assert np.array_equal(c.pileup()["counts"], first)
    finally:
        c.close()


def _lines(names, tlens, refs, counts_of, listed):
    """The file the twin expects: per target, per listed position, the line."""
    out = []
    for g, name in enumerate(names):
        for p in listed(g):
            out.append(pt.line(name, p, refs[g][p] if refs is not None else None, counts_of(g, p)))
    return out


@pytest.mark.gpu
def test_pbdagcon_pileup_and_sites(oracle_lib, tmp_path):
    tes = _tes()
    targets = tes._variant_targets(101, 20, 150, 300, full_span=True)
    names = ["ctg%d" % i for i in range(20)]
    tl = _tlens(targets)
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [r for _, r in targets]))
    texts = [[mt.encode(p, q, bb, o) for p, q, o in recs] for bb, recs in targets]
    bam = tmp_path / "in.bam"; bam.write_bytes(mf.bam_file(names, tl, mf.records(names, targets, texts)))
    strings = tes._strings(targets)
    m5 = tmp_path / "in.m5"
    from pbdagcon_amd import synth
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    sb.ids = names
    m5.write_bytes(synth.to_m5(sb))
    f = {k: tmp_path / k for k in ("e", "e2", "p", "s", "p2", "s2", "p3", "s3", "p4", "s4")}
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    rec = ["--sam", "--ref", str(ref)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    plain = run(*rec, "--edits", str(f["e2"]), str(sam))
    got = run(*rec, "--edits", str(f["e"]), "--pileup", str(f["p"]), "--sites", str(f["s"]), str(sam))
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 20 and f["e"].read_bytes() == f["e2"].read_bytes()
    want = _twin(strings, tl, 3, 30, 5)
    refs = [bb for bb, _ in targets]
    exp_p = _lines(names, tl, refs, lambda g, p: want[g][p], lambda g: [p for p in range(tl[g]) if want[g][p][:6].any()])
    exp_s = _lines(names, tl, refs, lambda g, p: want[g][p], lambda g: pt.sites(want[g], 2, 200000))
    assert f["p"].read_text().splitlines() == exp_p and len(exp_p) > 3000
    assert f["s"].read_text().splitlines() == exp_s and 20 < len(exp_s) < len(exp_p)
    # --bam --md: the same two files, REF from the rebuilt targets
    md = run("--bam", "--md", "--pileup", str(f["p2"]), "--sites", str(f["s2"]), str(bam))
    assert md.stdout == plain.stdout
    assert f["p2"].read_bytes() == f["p"].read_bytes() and f["s2"].read_bytes() == f["s"].read_bytes()
    # .m5: the same lines with REF as '.', and other thresholds
    t5 = run("--pileup", str(f["p3"]), "--sites", str(f["s3"]), "--site-min-frac", "0.3", "--site-min-count", "3", str(m5))
    assert t5.stdout.count(b">") >= 20
    assert f["p3"].read_text().splitlines() == _lines(names, tl, None, lambda g, p: want[g][p], lambda g: [p for p in range(tl[g]) if want[g][p][:6].any()])
    assert f["s3"].read_text().splitlines() == _lines(names, tl, None, lambda g, p: want[g][p], lambda g: pt.sites(want[g], 3, 300000))
    # --window: per position the line of the window whose core holds it
    W, O = 100, 70
    run(*rec, "--window", str(W), "--overlap", str(O), "--pileup", str(f["p4"]), "--sites", str(f["s4"]), str(sam))
    exp_p, exp_s = [], []
    for g, (bb, recs) in enumerate(targets):
        tiles = wt.tiled(tl[g], W, O)
        per = wt.window_targets(targets, [(g, a, b) for a, b, _, _ in tiles])
        for (a, b, c0, c1), (wl, alns, failed) in zip(tiles, per):
            assert not failed
            (cn,) = _twin([(bb[a:b], alns)], [wl], 3, 30, 5)
            for p in range(c0, c1):
                if cn[p - a][:6].any():
                    exp_p.append(pt.line(names[g], p, bb[p], cn[p - a]))
                    if pt.is_site([int(x) for x in cn[p - a]], 2, 200000):
                        exp_s.append(pt.line(names[g], p, bb[p], cn[p - a]))
    assert f["p4"].read_text().splitlines() == exp_p and len(exp_p) > 3000
    assert f["s4"].read_text().splitlines() == exp_s and len(exp_s) > 20
