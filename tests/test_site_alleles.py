"""The alleles at the sites, counted on the device (dagcon_set_site_alleles, pbdagcon --site-alleles / --site-vcf): the rule
by hand and the twin's invariants on the CPU, the device against the twin by exact equality on the GPU.
include/dagcon.h states the rule (8); alleles_twin.py is it in Python."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import alleles_twin as at
import cigar_twin as ct
import cs_twin as cst
import evidence_twin as ev
import md_files as mf
import md_twin as mt
import paf_files as pf
import pileup_twin as pt
import site_reads_twin as srt
from util import batch_from_targets, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID, NONCONFORMING = -8, -1, -4
GAP = 0x2D
K = at.key


def _tsr():
    import test_site_reads as tsr
    return tsr


def _tes():
    import test_edit_support as tes
    return tes


def _cli():
    return _tes()._cli()


def _code(f):
    return _tsr()._code(f)


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def _one(tlen, alns, min_len=1, trim=0, opts=(0, 0)):
    return at.target(tlen, alns, min_len, trim, opts)


def test_the_rule_by_hand(oracle_lib):
    # a substitution: normalizeGaps writes the target base dropped and the read base inserted behind it: the allele is T
    sub = _one(4, [(1, b"ATGT", b"ACGT")])
    assert ev.columns([(1, b"ATGT", b"ACGT")], 1, 0) == [(0, b"A-TGT", b"AC-GT")]
    assert [at.text(k) for k in sub["keys"][0]] == ["A", "T", "G", "T"] and sub["ents"][0][1] == (1, pt.DEL | 8)
    # a kept base plus an insertion; a deletion
    both = _one(4, [(1, b"ACTGT", b"AC-GT"), (1, b"A-GT", b"ACGT")])
    assert [at.text(k) for k in both["keys"][0]] == ["A", "CT", "G", "T"] and [at.text(k) for k in both["keys"][1]] == ["A", "-", "G", "T"]
    assert both["keys"][1][1] == 0 and [x[:2] for x in both["tables"][1]] == [(0, 1), (K(b"CT"), 1)]
    # lower case maps to the letter, a foreign byte to N
    low = _one(4, [(1, b"act*t", b"ac-gt")])
    assert [at.text(k) for k in low["keys"][0]] == ["A", "CT", "N", "T"]
    # the key: 3 bits a base from bit 57 down, a shorter allele before its extensions, - first
    assert K(b"A") == 1 << 57 and K(b"AC") == (1 << 57) | (2 << 54) and K(b"") == 0 and K(b"T" * 20) == int("4" * 20, 8)
    assert K(b"") < K(b"A") < K(b"AA") < K(b"AC") < K(b"C") < K(b"N") < K(b"A" * 21)
    # runs of exactly 19, 20 and 21 bases behind a kept base are alleles of 20, 21 and 22: no flag, flag, flag; of 18: none
    for n_ins, text in ((18, "A" + "CG" * 9), (19, "A" + "CG" * 9 + "C"), (20, "A" + "CG" * 9 + "C+"), (21, "A" + "CG" * 9 + "C+")):
        run = (b"CG" * 11)[:n_ins]
        tw = _one(3, [(1, b"A" + run + b"TA", b"A" + b"-" * n_ins + b"TA")])
        assert at.text(tw["keys"][0][0]) == text and bool(tw["keys"][0][0] & at.LONG) == (n_ins >= 20), n_ins
    # ... and a run of 19, 20, 21 behind a deleted base is the allele itself
    for n_ins, long_ in ((19, False), (20, False), (21, True)):
        run = (b"CG" * 11)[:n_ins]
        tw = _one(3, [(1, b"A-" + run + b"A", b"AT" + b"-" * n_ins + b"A")])
        assert tw["keys"][0][1] == K(run) and bool(K(run) & at.LONG) == long_ and at.text(K(run)) == run[:20].decode() + ("+" if long_ else "")
    # two long runs with the same first 20 bases are one allele
    a, b = b"A" + b"CG" * 12 + b"TA", b"A" + b"CG" * 10 + b"GCGC" + b"TA"
    lump = _one(3, [(1, a, b"A" + b"-" * 24 + b"TA"), (1, b, b"A" + b"-" * 24 + b"TA"), (1, b"ATA", b"ATA")])
    assert [x[:2] for x in lump["tables"][0]] == [(K(b"A" + b"CG" * 10), 2), (K(b"A"), 1)] and [ia[0] for ia in lump["ent_allele"]] == [0, 0, 1]
    # the trim: it takes target bases off either end.  A run whose base goes is left in front of the first column and
    # belongs nowhere; a run behind the last kept base stays whole and ends at the alignment's last column
    left, right = (1, b"ACGTTTTACGTACG", b"ACG----ACGTACG"), (1, b"ACGTACGTTTTACG", b"ACGTACG----ACG")
    assert ev.columns([left], 1, 3) == [(3, b"TTTTACGT", b"----ACGT")] and ev.columns([right], 1, 3) == [(3, b"TACGTTTT", b"TACG----")]
    assert [at.text(k) for k in _one(10, [left])["keys"][0]] == ["A", "C", "GTTTT", "A", "C", "G", "T", "A", "C", "G"]
    assert [at.text(k) for k in _one(10, [left], trim=3)["keys"][0]] == ["A", "C", "G", "T"]
    assert [at.text(k) for k in _one(10, [right], trim=3)["keys"][0]] == ["T", "A", "C", "GTTTT"]
    # a count tie is ordered by key: C before G before T, whatever the order of the reads
    tie = _one(1, [(1, b"T", b"A"), (1, b"G", b"A"), (1, b"C", b"A"), (1, b"G", b"A"), (1, b"C", b"A"), (1, b"T", b"A")])
    assert [(at.text(k), c) for k, c, _ in tie["tables"][0]] == [("C", 2), ("G", 2), ("T", 2)]
    assert tie["ent_allele"] == [[2], [1], [0], [1], [0], [2]]


def _bases(kk):
    """The bases a key holds (at most 20)."""
    return sum(1 for j in range(at.BASES) if (kk >> (3 * j)) & 7)


def _groupings(tw):
    """The defining invariants of one target's twin arrays.  (A key alone does not say whether its first base is the kept
    base or the first inserted one -- a substitution is the new base and nothing else, which is the point of the rule --
    so the six counters and INS come back from the table through the entries' codes.)"""
    for p, tab in zip(tw["sites"], tw["tables"]):
        n = tw["counts"][p]
        assert sum(c for _, c, _ in tab) == pt.depth(n) and all(sum(h) == c for _, c, h in tab)
        assert [(-c, kk) for kk, c, _ in tab] == sorted((-c, kk) for kk, c, _ in tab) and len({kk for kk, _, _ in tab}) == len(tab)
    seven = [[0] * 7 for _ in tw["sites"]]
    for e, ks, ia in zip(tw["ents"], tw["keys"], tw["ent_allele"]):
        for (k, code), kk, i in zip(e, ks, ia):
            assert tw["tables"][k][i][0] == kk
            cls, ins, first, L = code & 7, code >> 3, (kk >> 57) & 7, _bases(kk)
            # cls == DEL iff no base is kept: the allele is the run alone; otherwise it begins with the class's own letter
            assert (first == cls + 1 and ins == (L > 1)) if cls != pt.DEL else ins == (L > 0)
            seven[k][cls] += 1; seven[k][6] += L > (cls != pt.DEL)
    assert seven == [tw["counts"][p][:7] for p in tw["sites"]]


def _pileups(n, seed=81):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        alns, bb = _tes()._small_pileup(rng, k)
        out.append((bb, alns, int(rng.integers(0, 3)), (0, 0) if k % 2 else (2, 200000)))
    return out


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    n_al = n_long = n_multi = 0
    for bb, alns, trim, opts in _pileups(300):
        tw = at.target(len(bb), alns, 4, trim, opts)
        _groupings(tw)
        n_al += sum(len(t) for t in tw["tables"]); n_multi += sum(1 for t in tw["tables"] if len(t) > 2)
        n_long += sum(1 for t in tw["tables"] for kk, _, _ in t if len(at.text(kk)) > 2)
    print("alleles %d, sites with more than two %d, alleles of more than two bases %d" % (n_al, n_multi, n_long))
    assert n_al > 5000 and n_multi > 300 and n_long > 100


def _text(lib, key, cap=24):
    buf = ctypes.create_string_buffer(max(cap, 1))
    rc = lib.dagcon_allele_text(key, buf, cap)
    return rc, buf.value.decode()


def test_allele_text_against_the_twin(oracle_lib):
    from pbdagcon_amd import capi
    lib = capi.load()
    keys = {0, K(b"A" * 20), K(b"N" * 21), K(b"ACGTN")}
    for bb, alns, trim, opts in _pileups(300):
        keys |= {kk for ks in at.target(len(bb), alns, 4, trim, opts)["keys"] for kk in ks}
    assert len(keys) > 100
    for kk in sorted(keys):
        assert _text(lib, kk) == (0, at.text(kk)) and capi.allele_text(kk) == at.text(kk)
    assert capi.allele_text(0) == "-" and capi.allele_text(K(b"G" * 25)) == "G" * 20 + "+"
    # a buffer too small: the text and its 0 must fit; nothing is written half
    assert _text(lib, K(b"ACG"), 3)[0] == INVALID and _text(lib, K(b"ACG"), 4) == (0, "ACG")
    assert _text(lib, 0, 1)[0] == INVALID and _text(lib, 0, 2) == (0, "-") and _text(lib, K(b"T" * 30), 21)[0] == INVALID
    assert lib.dagcon_allele_text(K(b"A"), None, 8) == INVALID
    # integers that are no key: a bit above 60, a code above 5, a base behind an empty place, the flag without 20 bases
    for bad in (1 << 61, 6 << 57, 1 << 54, at.LONG | K(b"ACG")):
        assert _text(lib, bad)[0] == INVALID
        with pytest.raises(capi.DagconError):
            capi.allele_text(bad)


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in ("dagcon_set_site_alleles", "dagcon_fetch_site_alleles", "dagcon_allele_text"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = '#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu\\n", sizeof(dagcon_site_alleles)); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert ctypes.sizeof(capi.SiteAlleles) == int(out[0]) == 56
    for m in ("set_site_alleles", "site_alleles"):
        assert callable(getattr(capi.Context, m))
    assert callable(capi.allele_text) and lib.dagcon_abi_version() == 2


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for flag in ("--site-alleles", "--site-vcf"):
        f = tmp_path / ("o" + flag)
        # every refusal of --site-reads (test_site_reads.test_usage_errors_and_help)
        for args in ([str(m5), flag],
                     rec + ["--window", "200", "--overlap", "120", flag, str(f), str(sam)],
                     ["-a", flag, str(f), str(m5)], ["-a", "--polish", "1", flag, str(f), str(m5)],
                     rec + ["--dump-parsed", flag, str(f), str(sam)],
                     [flag, str(f), "--site-min-frac", "1.5", str(m5)]):
            out = run(*args)
            assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
            assert not f.exists()
        out = run(*rec, flag, str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr, flag
    # --site-vcf needs the target's bases: refused on .m5 input; --site-alleles is not
    out = run("--site-vcf", str(tmp_path / "o.vcf"), str(m5))
    assert out.returncode == 2 and b"PARSE ERROR" in out.stderr and not (tmp_path / "o.vcf").exists()
    out = run("--site-alleles", str(tmp_path / "no_such_dir" / "o.txt"), "--site-min-frac", "0.3", "--site-min-count", "3", str(m5))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --site-alleles FILE")[1].split(b"\n  -v, --verbose")[0]
    assert b"RNAME POS REF DEPTH ALLELE COUNT H1 H2 H0" in text and b"\n  --site-vcf FILE" in text
    assert b"RNAME POS . REF ALT . . DP=depth;AD=ref,alt1,.." in text and b"AD1=..;AD2=.." in text
    flat = b" ".join(text.split())
    assert b"Adjacent sites are NOT joined: a deletion of three bases is three records" in flat and b"No genotype is called" in flat
    assert b"[--site-alleles FILE] [--site-vcf FILE]" in h.stdout.split(b"\n")[0]


_AL_MAIN = r"""
#include <iostream>
#include "alleles.h"
// stdin: "a rname pos0 ref n0..n7 key count split c1 c2 c0" | "h split n name len .." | "v rname tb pos0 n0..n7 min_count split n_al (key count c1 c2 c0).."
int main() {
    std::string out, kind, rname, tb;
    while (std::cin >> kind) {
        unsigned v[8]; uint16_t n[8];
        if (kind == "a") {
            unsigned long long pos, key; std::string ref; unsigned count, split, h[3];
            std::cin >> rname >> pos >> ref; for (int k = 0; k < 8; k++) { std::cin >> v[k]; n[k] = (uint16_t)v[k]; }
            std::cin >> key >> count >> split >> h[0] >> h[1] >> h[2];
            const uint16_t hap[3] = {(uint16_t)h[0], (uint16_t)h[1], (uint16_t)h[2]};
            dg_site_allele_line(out, rname, pos, ref == "." ? 0 : ref[0], n, key, count, split ? hap : nullptr);
        } else if (kind == "h") {
            unsigned split, k; std::string contigs, name; unsigned len;
            std::cin >> split >> k;
            while (k--) { std::cin >> name >> len; contigs += "##contig=<ID=" + name + ",length=" + std::to_string(len) + ">\n"; }
            dg_site_vcf_header(out, contigs, split != 0);
        } else {
            unsigned pos, min_count, split, n_al;
            std::cin >> rname >> tb >> pos; for (int k = 0; k < 8; k++) { std::cin >> v[k]; n[k] = (uint16_t)v[k]; }
            std::cin >> min_count >> split >> n_al;
            std::vector<uint64_t> key(n_al); std::vector<uint32_t> count(n_al); std::vector<uint16_t> hap(3 * n_al);
            for (unsigned i = 0; i < n_al; i++) { unsigned long long kk; unsigned h[3]; std::cin >> kk >> count[i] >> h[0] >> h[1] >> h[2]; key[i] = kk; for (int j = 0; j < 3; j++) hap[3 * i + j] = (uint16_t)h[j]; }
            const size_t before = out.size();
            dg_site_vcf_record(out, rname, tb.data(), (uint32_t)tb.size(), pos, n, key.data(), count.data(), split ? hap.data() : nullptr, n_al, min_count);
            if (out.size() == before) out += "(none)\n";
        }
    }
    std::cout << out;
    return 0;
}
"""


def _n(**kw):
    return _tsr()._n(**kw)


def test_the_line_formatters_against_python(tmp_path):
    src = tmp_path / "al_main.cpp"; src.write_text(_AL_MAIN)
    exe = tmp_path / "al_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"), "-o", str(exe), str(src)])
    lines = [("ctg", 0, ord("A"), _n(A=3, DEL=2, INS=1), K(b"A"), 2, (1, 1, 0)), ("ctg", 0, ord("A"), _n(A=3, DEL=2, INS=1), 0, 2, None),
             ("a/b|c", 4294967295, None, _n(G=4094), K(b"G" * 21), 4094, (4094, 0, 0)), ("x", 41, ord("n"), _n(N=1), K(b"NAC"), 1, (0, 0, 1))]
    tb = b"ACGTAC"
    tab = [(K(b"C"), 5, (3, 1, 1)), (K(b"G"), 3, (0, 3, 0)), (0, 2, (1, 1, 0)), (K(b"CTT"), 2, (2, 0, 0)), (K(b"T" * 21), 2, (0, 0, 2)), (K(b"T"), 1, (0, 1, 0))]
    n = _n(C=7, G=3, T=3, DEL=2, INS=4)
    recs = [("c", tb, 1, n, tab, 2, True),                      # anchored on the base in front: a deleted base among the ALTs; the long allele and the rare one are left out
            ("c", tb, 1, n, tab, 3, False),                     # min_count 3 leaves G alone: not anchored
            ("c", tb, 1, n, tab, 1, True),                      # min_count 1: T comes in too
            ("c", b"CGTA", 0, n, tab, 2, True),                 # position 0: anchored on the base behind
            ("c", tb, 1, n, tab[:1], 1, True),                  # a site with no ALT
            ("c", tb, 1, n, tab, 6, True),                      # ... no ALT deep enough
            ("c", b"C", 0, n, tab, 1, True),                    # a target of one base
            ("c", b"ANGTAC", 1, n, tab, 2, False),              # the REF allele is not in the table: AD begins with 0
            ("c", b"AcGTAC", 1, n, tab, 2, False)]              # a lower-case REF base is the same allele, printed as it is
    heads = [(True, [("c", 6), ("a/b|c", 70000)]), (False, [])]
    text = "".join("a %s %d %s %s %d %d %d %s\n" % (r, p, chr(ref) if ref else ".", " ".join(map(str, nn)), kk, c, 1 if h else 0, " ".join(map(str, h or (0, 0, 0))))
                   for r, p, ref, nn, kk, c, h in lines)
    text += "".join("h %d %d %s\n" % (s, len(cs), " ".join("%s %d" % c for c in cs)) for s, cs in heads)
    text += "".join("v %s %s %d %s %d %d %d %s\n" % (r, t.decode(), p, " ".join(map(str, nn)), mc, sp, len(tt), " ".join("%d %d %d %d %d" % ((kk, c) + h) for kk, c, h in tt))
                    for r, t, p, nn, tt, mc, sp in recs)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    exp = [at.site_alleles_line(*x) for x in lines]
    for s, cs in heads:
        exp += at.vcf_header(cs, s)
    exp += [at.vcf_record(*x) or "(none)" for x in recs]
    assert out == exp
    assert exp[0] == "ctg\t1\tA\t5\tA\t2\t1\t1\t0" and exp[1] == "ctg\t1\tA\t5\t-\t2\t.\t.\t." and exp[2].split("\t")[4] == "G" * 20 + "+"
    v = exp[-len(recs):]
    assert v[0] == "c\t1\t.\tAC\tAG,A,ACTT\t.\t.\tDP=15;AD=5,3,2,2;AD1=3,0,1,2;AD2=1,3,1,0"
    assert v[1] == "c\t2\t.\tC\tG\t.\t.\tDP=15;AD=5,3" and v[2].split("\t")[4] == "AG,A,ACTT,AT"
    assert v[3] == "c\t1\t.\tCG\tGG,G,CTTG\t.\t.\tDP=15;AD=5,3,2,2;AD1=3,0,1,2;AD2=1,3,1,0"
    assert v[4] == v[5] == v[6] == "(none)" and v[7].split("\t")[3:5] == ["AN", "AC,AG,A,ACTT"] and v[7].endswith("AD=0,5,3,2,2")
    assert v[8].split("\t")[3:5] == ["Ac", "AG,A,ACTT"]


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _device(call, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None):
    """One context with the pile-up, the site reads and the switch on: everything it gives."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*opts)
        c.set_site_reads(phase, rounds)
        c.set_site_alleles(True)
        got = call(c)
        sa = c.site_alleles()
        return {"got": got, "sa": sa, "sr": c.site_reads(), "ps": c.pileup_sites(), "pu": c.pileup(), "status": c.target_status.tolist(),
                "reruns": c.timings()["reruns"], "tally": None}
    finally:
        c.close()


def _expect(strings, tlens, min_cov, min_len, trim, opts, rounds, status, n_given=None, src=None):
    """test_site_reads._expect's arrays and the alleles', from one twin run per target."""
    out = {k: [] for k in ("aln_tgt", "aln_src", "ent_site", "ent_code", "hap", "phase", "pos", "key", "count", "hap_count", "ent_allele")}
    out["ent_begin"], out["site_begin"], out["al_begin"] = [0], [0], [0]
    base = 0
    for t, (s, tl) in enumerate(zip(strings, tlens)):
        n_al = 0 if s is None else len(s[1])
        if s is not None and not status[t] and n_al >= max(1, min_cov):
            tw = at.target(tl, s[1], min_len, trim, opts, rounds or srt.ROUNDS)
            sb = len(out["pos"])
            for i, e, h, ia in zip(tw["src"], tw["ents"], tw["hap"], tw["ent_allele"]):
                out["aln_tgt"].append(t); out["aln_src"].append(src[t][i] if src is not None else base + i); out["hap"].append(h)
                out["ent_site"] += [sb + k for k, _ in e]; out["ent_code"] += [c for _, c in e]; out["ent_allele"] += ia
                out["ent_begin"].append(len(out["ent_site"]))
            out["pos"] += tw["sites"]; out["phase"] += tw["phase"]
            for tab in tw["tables"]:
                out["key"] += [kk for kk, _, _ in tab]; out["count"] += [c for _, c, _ in tab]; out["hap_count"] += [list(h) for _, _, h in tab]
                out["al_begin"].append(len(out["key"]))
        out["site_begin"].append(len(out["pos"]))
        base += n_given[t] if n_given is not None else n_al
    return out


def _check(dev, exp, phase=True):
    sa, sr, ps = dev["sa"], dev["sr"], dev["ps"]
    _tsr()._check((dev["pu"], ps, sr), exp, phase)
    for k in ("al_begin", "key", "count", "ent_allele"):
        assert sa[k].tolist() == exp[k], k
    if phase:
        assert sa["hap_count"].tolist() == exp["hap_count"]
    else:
        assert sa["hap_count"] is None
    # from the device's own arrays: the indices line up with the sites and the entries, the counts are the entries' recount
    assert sa["al_begin"].size == ps["pos"].size + 1 and sa["ent_allele"].size == sr["ent_site"].size
    nd = np.diff(sa["al_begin"]).astype(np.int64)
    site = sr["ent_site"].astype(np.int64)
    assert (sa["ent_allele"].astype(np.int64) < nd[site]).all()
    at_ = sa["al_begin"][:-1].astype(np.int64)[site] + sa["ent_allele"].astype(np.int64)
    assert np.array_equal(np.bincount(at_, minlength=sa["key"].size), sa["count"].astype(np.int64))
    assert np.array_equal(np.add.reduceat(sa["count"].astype(np.int64), sa["al_begin"][:-1].astype(np.int64)) if nd.size else np.zeros(0, np.int64),
                          ps["counts"][:, :6].astype(np.int64).sum(axis=1))
    if phase:
        who = np.repeat(np.arange(sr["aln_tgt"].size), np.diff(sr["ent_begin"]).astype(np.int64))
        col = (sr["hap"][who].astype(np.int64) - 1) % 3
        re = np.zeros((sa["key"].size, 3), np.int64)
        np.add.at(re, (at_, col), 1)
        assert np.array_equal(re, sa["hap_count"].astype(np.int64))
    # cls != DEL: the allele begins with the class's letter and ins says that more follows; cls == DEL: ins says that anything does
    kk = sa["key"][at_] if at_.size else np.zeros(0, np.uint64)
    first = ((kk >> np.uint64(57)) & np.uint64(7)).astype(np.int64)
    cls, ins = (sr["ent_code"] & 7).astype(np.int64), (sr["ent_code"] >> 3) == 1
    kept = cls != 5
    assert np.array_equal(first[kept], cls[kept] + 1) and np.array_equal(ins[kept], (kk[kept] & np.uint64((1 << 57) - 1)) != 0)
    assert np.array_equal(ins[~kept], kk[~kept] != 0)


def _run(call, strings, tlens, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None, n_given=None, src=None):
    dev = _device(call, min_cov, min_len, trim, opts, phase, rounds, prepare)
    exp = _expect(strings, tlens, min_cov, min_len, trim, opts, rounds, dev["status"], n_given, src)
    _check(dev, exp, phase)
    return dev, exp


def _strings_call(strings):
    batch = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    return lambda c: c.consensus(batch, strict=False)


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 2])
@pytest.mark.parametrize("opts", [(0, 0), (2, 200000)])
def test_random_small_targets(oracle_lib, trim, opts):
    """6 targets of 80-300 bases under 6-14 reads, the split on and off."""
    rng = np.random.default_rng(500 + trim)
    strings = []
    for k in range(6):
        alns, bb = random_target(rng, int(rng.integers(80, 301)), int(rng.integers(6, 15)), sub=0.05, ins=0.08, dele=0.05, full_span=bool(k % 2))
        strings.append((bb, alns))
    tlens = [len(bb) for bb, _ in strings]
    for phase in (True, False):
        dev, exp = _run(_strings_call(strings), strings, tlens, 3, 30, trim, opts, phase)
        assert dev["status"] == [0] * 6
    sa = dev["sa"]
    print("sites %d, alleles %d, entries %d" % (sa["al_begin"].size - 1, sa["key"].size, sa["ent_allele"].size))
    assert sa["key"].size > (1500 if opts == (0, 0) else 100) and np.diff(sa["al_begin"]).max() >= 3 and sa["ent_allele"].max() >= 2


def _read(bb, s, e, ins=(), dele=(), tail=0):
    """bases [s, e) of bb; ins: {x: n} n bases in front of base x, none equal to a neighbour; dele: bases dropped; tail:
    inserted columns behind the last base."""
    def other(*avoid):
        return next(b for b in b"ACGT" if b not in avoid)
    q, t = bytearray(), bytearray()
    for x in range(s, e):
        if x in ins:
            a = other(bb[x], bb[x - 1])
            for k in range(ins[x]):
                q.append(a if k % 2 == 0 else other(bb[x], bb[x - 1], a)); t.append(GAP)
        if x in dele:
            q.append(GAP); t.append(bb[x]); continue
        q.append(bb[x]); t.append(bb[x])
    for k in range(tail):
        q.append(other(bb[e - 1], bb[min(e, len(bb) - 1)]) if k % 2 == 0 else other(bb[e - 1], other(bb[e - 1], bb[min(e, len(bb) - 1)]))); t.append(GAP)
    return (s + 1, bytes(q), bytes(t))


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(0, 0), (2, 200000)])
def test_the_64_column_period(oracle_lib, opts):
    """Hand-built reads on a target without equal neighbours, every one beginning at base 10: an entry in lane 63 whose run
    begins in the next step, one in lane 62 whose run crosses it, a run of 70 columns (more than a step: a long allele), a
    run of 30 that begins in lane 50, a run that ends at the alignment's last column, alignments of exactly 64 and 65 columns."""
    tes = _tes()
    bb = tes._nonrep(np.random.default_rng(64), 260)
    s = 10
    reads = [_read(bb, s, 250, ins={s + 64: 3}), _read(bb, s, 250, ins={s + 63: 3}), _read(bb, s, 250, ins={s + 20: 70}), _read(bb, s, 250, ins={s + 51: 30}),
             _read(bb, s, 200, tail=2), _read(bb, s, s + 64), _read(bb, s, s + 65), _read(bb, s, 250, ins={s + 64: 3}), _read(bb, s, 250, ins={s + 63: 3}),
             _read(bb, s, 250, ins={s + 20: 70}), _read(bb, s, 250, dele={s + 63}), _read(bb, s, 250),
             _read(bb, s, 250, ins={s + 64: 3}), _read(bb, s, 250, ins={s + 63: 3}), _read(bb, s, 250, ins={s + 20: 70})]
    cols = ev.columns(reads, 30, 0)
    assert len(cols) == len(reads) and [len(t) for _, _, t in cols][5:7] == [64, 65]
    for i, (first, n) in enumerate(((64, 3), (63, 3), (20, 70), (51, 30))):
        _, q, t = cols[i]
        assert t[first - 1] != GAP and all(x == GAP for x in t[first:first + n]) and t[first + n] != GAP and GAP not in q[first - 1:first + n]
    assert cols[4][2][-2:] == bytes([GAP, GAP]) and cols[4][2][-3] != GAP and cols[10][1][63] == GAP
    dev, exp = _run(_strings_call([(bb, reads)]), [(bb, reads)], [260], 1, 30, 0, opts)
    assert dev["status"] == [0]
    texts = {at.text(int(k)) for k in dev["sa"]["key"]}
    # (the runs of 3 and of 70 are in three reads of 15 each: sites at 2 / 200000 too; the deleted base and the run of 30 are in one)
    assert any(x.endswith("+") for x in texts) and any(len(x) == 4 for x in texts) and (opts != (0, 0) or ("-" in texts and any(len(x) == 21 for x in texts)))


def _staircase(distinct):
    """A target of 60 A under reads that all begin at its first base: 235 of 10 bases, one of 20, one of 30, 62 of 40, one of
    50: depths 300, 65, 64, 63, 1 from the left.  distinct: every read carries, behind bases 5, 15, 25, 35 and 45 (where it has
    them), six inserted bases of C G T that spell its own number: at those sites every read shows another allele."""
    bb = b"A" * 60
    spans = [50] + [40] * 62 + [30] + [20] + [10] * 235
    alns = []
    for r, e in enumerate(spans):
        q, t = bytearray(), bytearray()
        for x in range(e):
            q.append(bb[x]); t.append(bb[x])
            if distinct and x % 10 == 5:
                w = bytes(b"CGT"[(r // 3 ** j) % 3] for j in range(6))
                q += w; t += b"-" * 6
        alns.append((1, bytes(q), bytes(t)))
    return bb, alns


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [True, False])
def test_the_depth_cut(oracle_lib, distinct):
    """Sites of depth 1, 63, 64, 65 and 300 in one target: a wave sorts a site of up to 64 entries, a block a deeper one."""
    bb, alns = _staircase(distinct)
    dev, exp = _run(_strings_call([(bb, alns)]), [(bb, alns)], [60], 1, 5, 0, (0, 0))
    assert dev["status"] == [0]
    ps, sa = dev["ps"], dev["sa"]
    depth = ps["counts"][:, :6].astype(np.int64).sum(axis=1)
    nd = np.diff(sa["al_begin"]).astype(np.int64)
    assert ps["pos"].tolist() == list(range(50)) and depth.tolist() == [300] * 10 + [65] * 10 + [64] * 10 + [63] * 10 + [1] * 10
    if distinct:
        assert nd[5::10].tolist() == [300, 65, 64, 63, 1] and nd[4::10].tolist() == [1] * 5
        assert sorted(sa["ent_allele"][dev["sr"]["ent_site"] == 5].tolist()) == list(range(300))
    else:
        assert nd.tolist() == [1] * 50 and sa["count"].tolist() == depth.tolist() and not sa["ent_allele"].any()


@pytest.mark.gpu
def test_the_deepest_site(oracle_lib):
    """One target at depth 4,094: 40 bases, every read with a wrong base now and then and, behind base 20, eight inserted
    bases that spell its number: a site of 4,094 alleles, the most a block sorts."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(4094)
    bb = b"A" * 40
    wrong = rng.random((capi.MAX_COVERAGE, 40)) < 0.02
    alns = []
    for r in range(capi.MAX_COVERAGE):
        q, t = bytearray(), bytearray()
        for x in range(40):
            q.append(b"CGT"[r % 3] if wrong[r, x] and x != 20 else bb[x]); t.append(bb[x])
            if x == 20:
                q += bytes(b"CGT"[(r // 3 ** j) % 3] for j in range(8)); t += b"-" * 8
        alns.append((1, bytes(q), bytes(t)))
    dev, exp = _run(_strings_call([(bb, alns)]), [(bb, alns)], [40], 6, 5, 0, (0, 0), phase=False)
    assert dev["status"] == [0]
    sa, ps = dev["sa"], dev["ps"]
    nd = np.diff(sa["al_begin"]).astype(np.int64)
    k = ps["pos"].tolist().index(20)
    assert nd[k] == capi.MAX_COVERAGE and int(ps["counts"][k][:6].sum()) == capi.MAX_COVERAGE and nd.size > 20 and sorted(set(nd.tolist()))[-2] <= 4


@pytest.mark.gpu
def test_the_split_s_counts_on_the_planted_case(oracle_lib):
    bb, alns, subs, ins_at, n_err = _tsr()._planted()
    dev, exp = _run(_strings_call([(bb, alns)]), [(bb, alns)], [600], 6, 500, 50, (2, 200000))
    sa, sr, ps = dev["sa"], dev["sr"], dev["ps"]
    assert sr["hap"].tolist() == [1] * 12 + [2] * 12
    # a planted substitution: the target's base in group 1, the other base in group 2 (but for a read error), nothing unlabelled
    p = next(x for x in subs if 60 <= x < ins_at)
    k = ps["pos"].tolist().index(p)
    a0 = int(sa["al_begin"][k])
    assert at.text(int(sa["key"][a0])) in (chr(bb[p]), chr(alns[12][1][p])) and sa["hap_count"][a0:a0 + 2, 2].tolist() == [0, 0]
    assert sa["hap_count"][a0:a0 + 2, :2].max(axis=1).min() >= 10 and sa["hap_count"][:, 2].sum() == 0
    # the planted insertion: the kept base alone in group 1, the kept base and the inserted one in group 2
    k = ps["pos"].tolist().index(ins_at - 1)
    a0 = int(sa["al_begin"][k])
    assert sorted(len(at.text(int(x))) for x in sa["key"][a0:a0 + 2]) == [1, 2]


@pytest.mark.gpu
def test_every_way_in_gives_the_same_arrays(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(91, 12, 150, 400, full_span=True)
    strings = tes._strings(targets)
    tlens = [len(bb) for bb, _ in targets]
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
    calls = {"strings": _strings_call(strings),
             "plain": lambda c: c.consensus_cigar(plain), "packed": lambda c: c._intake(plain.packed(), None, plain, True),
             "stranded": lambda c: c._intake(capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), None, None, True),
             "cs": lambda c: c.consensus_cs(cs), "md": lambda c: c.consensus_cigar_md(capi.HostCigarBatch(**arr), md)}
    ref = None
    for kind, call in calls.items():
        dev = _device(call, 3, 30, 5, (2, 200000))
        assert dev["status"] == [0] * 12, kind
        if ref is None:
            ref = dev["sa"]
            _check(dev, _expect(strings, tlens, 3, 30, 5, (2, 200000), 0, dev["status"]))
            assert ref["key"].size > 100 and np.diff(ref["al_begin"]).max() >= 3
        for k in ref:
            assert np.array_equal(dev["sa"][k], ref[k]), (kind, k)


@pytest.mark.gpu
def test_consensus_pre_on_the_aligner_s_strings(oracle_lib):
    """dagcon_consensus_pre: the twin is fed the strings dagcon_align returns for the same pairs."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(7)
    targets, pairs, starts = [], [], []
    for ti in range(3):
        tlen = int(rng.integers(300, 400))
        target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
        recs = []
        for r in range(6):
            s = int(rng.integers(0, tlen // 5)); e = int(rng.integers(4 * tlen // 5, tlen + 1))
            qseq = bytearray()
            for ch in target[s:e]:
                u = rng.random()
                if u < 0.04:
                    continue
                qseq.append(ch if u > 0.06 else b"ACGT"[rng.integers(0, 4)])
                if rng.random() < 0.06:
                    qseq.append(b"ACGT"[rng.integers(0, 4)])
            recs.append((s, b"+", bytes(qseq), target[s:e]))
            pairs.append((bytes(qseq), target[s:e])); starts.append(s + 1)
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
    dev, exp = _run(lambda c: c.consensus_pre(targets), strings, [t for t, _ in targets], 3, 100, 10, (2, 200000))
    assert dev["status"] == [0] * 3 and dev["sa"]["key"].size > 50


@pytest.mark.gpu
def test_under_the_record_filter(oracle_lib):
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
    dev, exp = _run(tes._whole(targets), tes._strings(kept), [len(bb) for bb, _ in targets], 3, 30, 5, (2, 200000),
                    prepare=lambda c: c.set_record_filter(max_depth=depth), src=src)
    assert dev["status"] == [0] * 10 and dev["sa"]["count"].max() <= depth


@pytest.mark.gpu
def test_a_batch_with_a_failed_target(oracle_lib):
    """40 small record targets, one with a non-conforming record: its sites and entries are gone from every array, and the
    indices still line up with dagcon_fetch_pileup_sites and dagcon_fetch_site_reads (_check)."""
    tes = _tes()
    rng = np.random.default_rng(302)
    targets = []
    for k in range(40):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns, eqx=True)))
    bad = 20
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = tes._strings(targets)
    assert strings[bad] is None
    dev, exp = _run(tes._whole(targets), strings, [len(bb) for bb, _ in targets], 3, 4, 1, (0, 0), n_given=[len(r) for _, r in targets])
    assert dev["status"][bad] == NONCONFORMING and sum(1 for s in dev["status"] if s) == 1 and bad not in dev["sr"]["aln_tgt"].tolist()
    assert int(dev["ps"]["site_begin"][bad]) == int(dev["ps"]["site_begin"][bad + 1]) and dev["sa"]["key"].size > 1000


@pytest.mark.gpu
def test_arena_growth(oracle_lib):
    """test_site_reads.test_arena_growth's batch: at 0 / 0 the entries outgrow the arena's first size and the batch runs
    again; the alleles still equal the twin, and everything else is what a context without the switch gives."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    alns, bb = random_target(rng, 400, 40, full_span=True, sub=0.02, ins=0.03, dele=0.03)
    batch = batch_from_targets([(400, alns, None)])
    assert sum(len(q) for _, q, _ in alns) // 64 + 4096 < 40 * 380
    dev, exp = _run(lambda c: c.consensus(batch), [(bb, alns)], [400], 3, 30, 5, (0, 0))
    assert dev["status"] == [0] and dev["sa"]["ent_allele"].size > 40 * 380
    off = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        off.set_pileup(0, 0)
        got_off = off.consensus(batch)
        reruns_off = off.timings()["reruns"]
    finally:
        off.close()
    assert dev["reruns"] > reruns_off and dev["got"] == got_off


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    # what a context gives with the switch off: the consensus, the pile-up, the sites, the site reads, the tally
    plain = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        plain.set_pileup(2, 200000); plain.set_site_reads(True); plain.set_hap_consensus(1, 2)
        want = plain.consensus_cigar(cb)
        want_all = (plain.pileup_sites(), plain.pileup(), plain.site_reads(), plain.hap_tally())
        assert _code(plain.site_alleles) == STATE                      # the switch off at the upload
    finally:
        plain.close()
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        assert _code(c.site_alleles) == STATE                          # nothing yet
        c.set_site_alleles(True)
        assert c.consensus_cigar(cb) == want                           # the pile-up and the site reads off at the upload
        assert _code(c.site_alleles) == STATE and _code(c.site_reads) == STATE
        c.set_pileup(2, 200000)
        assert c.consensus_cigar(cb) == want                           # the site reads off
        assert _code(c.site_alleles) == STATE
        c.set_pileup(None); c.set_site_reads(True)
        assert c.consensus_cigar(cb) == want                           # the pile-up off
        assert _code(c.site_alleles) == STATE
        c.set_pileup(2, 200000); c.set_hap_consensus(1, 2)
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.site_alleles) == STATE                          # before a fetch
        assert c.fetch() == want
        first = c.site_alleles()
        assert first["key"].size > 0 and first["hap_count"][:, :2].any()
        again = c.site_alleles()                                       # asked twice
        assert all(np.array_equal(first[k], again[k]) for k in first)
        # with the switch on everything else is byte for byte what it is with it off
        got_all = (c.pileup_sites(), c.pileup(), c.site_reads(), c.hap_tally())
        for a, b in zip(got_all, want_all):
            assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        c.set_site_alleles(False)                                      # off: this batch's results stay, the next has none
        assert np.array_equal(c.site_alleles()["key"], first["key"])
        assert c.consensus_cigar(cb) == want
        assert _code(c.site_alleles) == STATE and c.site_reads()["ent_site"].size > 0
        c.set_site_alleles(True)                                       # and on again
        assert c.consensus_cigar(cb) == want
        third = c.site_alleles()
        assert all(np.array_equal(first[k], third[k]) for k in first)
        c.upload_haps()                                                # the derived batch has it off
        assert _code(c.site_alleles) == STATE
        c.run(); c.fetch()
        assert _code(c.site_alleles) == STATE
        c.set_site_alleles(False)
        c.upload_cigar(cb)                                             # a later upload
        assert _code(c.site_alleles) == STATE
    finally:
        c.close()
    for flag in (capi.FLAG_STOP_AFTER_MERGE, capi.FLAG_STOP_AFTER_BUILD):
        stop = capi.Context(min_cov=3, min_len=30, trim=5, flags=flag)
        try:
            stop.set_pileup(2, 200000); stop.set_site_reads(True); stop.set_site_alleles(True)
            stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
            assert _code(stop.site_alleles) == STATE
        finally:
            stop.close()


def _cli_lines(strings, names, tl, opts, split, with_ref=True):
    lines, vcf = [], at.vcf_header(list(zip(names, tl)), split)
    for g, (bb, alns) in enumerate(strings):
        tw = at.target(tl[g], alns, 30, 5, opts)
        for p, tab in zip(tw["sites"], tw["tables"]):
            lines += [at.site_alleles_line(names[g], p, bb[p] if with_ref else None, tw["counts"][p], kk, c, h if split else None) for kk, c, h in tab]
            rec = at.vcf_record(names[g], bb, p, tw["counts"][p], tab, opts[0], split)
            if rec:
                vcf.append(rec)
    return lines, vcf


@pytest.mark.gpu
def test_pbdagcon_site_alleles_and_site_vcf(oracle_lib, tmp_path):
    tes = _tes()
    targets = tes._variant_targets(101, 8, 150, 300, full_span=True)
    names = ["ctg%d" % i for i in range(8)]
    tl = [len(bb) for bb, _ in targets]
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [r for _, r in targets]))
    strings = tes._strings(targets)
    from pbdagcon_amd import synth
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    sb.ids = names
    m5 = tmp_path / "in.m5"; m5.write_bytes(synth.to_m5(sb))
    f = {k: tmp_path / k for k in ("a", "v", "a2", "v2", "h", "a3", "a4", "v4")}
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    rec = ["--sam", "--ref", str(ref)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    plain = run(*rec, str(sam))
    got = run(*rec, "--site-alleles", str(f["a"]), "--site-vcf", str(f["v"]), str(sam))
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 8
    lines, vcf = _cli_lines(strings, names, tl, (2, 200000), False)
    assert f["a"].read_text().splitlines() == lines and len(lines) > 100 and all(x.endswith("\t.\t.\t.") for x in lines)
    assert f["v"].read_text().splitlines() == vcf and len(vcf) > 30 + 8
    # --bam --md with the two flags alone: REF and the anchors come from the targets the device rebuilt, fetched for them
    texts = [[mt.encode(p, q, bb, o) for p, q, o in recs] for bb, recs in targets]
    bam = tmp_path / "in.bam"; bam.write_bytes(mf.bam_file(names, tl, mf.records(names, targets, texts)))
    got = run("--bam", "--md", "--site-alleles", str(f["a4"]), "--site-vcf", str(f["v4"]), str(bam))
    assert got.stdout == plain.stdout and f["a4"].read_bytes() == f["a"].read_bytes() and f["v4"].read_bytes() == f["v"].read_bytes()
    # with the split on
    got = run(*rec, "--site-alleles", str(f["a2"]), "--site-vcf", str(f["v2"]), "--haplotag", str(f["h"]), str(sam))
    assert got.stdout == plain.stdout
    lines, vcf = _cli_lines(strings, names, tl, (2, 200000), True)
    assert f["a2"].read_text().splitlines() == lines and f["v2"].read_text().splitlines() == vcf
    assert any(";AD1=" in x for x in vcf) and not all(x.endswith("\t0\t0\t" + x.split("\t")[5]) for x in lines)
    # the .m5 of the same alignments: no REF, other thresholds, two batches
    got = run("--site-alleles", str(f["a3"]), "--site-min-frac", "0.3", "--site-min-count", "3", "--batch-targets", "5", "-j", "2", str(m5))
    assert got.stdout == run(str(m5)).stdout
    lines, _ = _cli_lines(strings, names, tl, (3, 300000), False, with_ref=False)
    assert f["a3"].read_text().splitlines() == lines and len(lines) > 50
