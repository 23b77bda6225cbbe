"""Adjacent sites joined into one variant record, counted on the device (dagcon_set_site_join, pbdagcon --joined-alleles /
--joined-vcf): the rule by hand and the twin's invariants on the CPU, the device against the twin by exact equality on the
GPU.  include/dagcon.h states the rule (10); join_twin.py is it in Python.  Every figure a GPU case is built to reach is
asserted from the twin before the device runs."""
import ctypes
import itertools
import os
import subprocess
import tempfile
from collections import Counter

import numpy as np
import pytest

import alleles_twin as at
import cigar_twin as ct
import cs_twin as cst
import join_twin as jt
import md_twin as mt
import paf_files as pf
import pileup_twin as pt
import site_reads_twin as srt
from util import batch_from_targets, random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, NONCONFORMING = -8, -4
GAP = 0x2D
NONE = jt.NONE


def _tsa():
    import test_site_alleles as tsa
    return tsa


def _tes():
    import test_edit_support as tes
    return tes


def _cli():
    return _tes()._cli()


def _code(f):
    return _tsa()._code(f)


def _other(b, k=0):
    return [x for x in b"ACGT" if x != b][k]


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def test_the_rule_by_hand(oracle_lib):
    """tlen 12, six reads: three delete positions 4 - 6, two carry the adjacent substitutions C8G A9T, one is the target's
    own bases and ends behind position 5.  At 2 / 0.2 the sites are 4 5 6 and 8 9: two runs."""
    bb = b"ACGTGCATCAGT"
    dele, sub, short = (1, b"ACGT---TCAGT", bb), (1, b"ACGTGCATGTGT", bb), (1, bb[:6], bb[:6])
    tw = jt.target(12, [dele] * 3 + [sub] * 2 + [short], 1, 0, (2, 200000))
    assert tw["sites"] == [4, 5, 6, 8, 9] and tw["run_begin"] == [0, 3, 5] and tw["hap"] == [1, 1, 1, 2, 2, 2]
    # the sites' own tables: a tie goes to the lower key, and - is the lowest
    assert [[(at.text(k), c) for k, c, _ in t] for t in tw["tables"]] == [[("-", 3), ("G", 3)], [("-", 3), ("C", 3)], [("-", 3), ("A", 2)], [("C", 3), ("G", 2)], [("A", 3), ("T", 2)]]
    # run 0: five alignments have an entry at 4, 5 and 6, the short one only at 4 and 5; depth(6) = 5 + 0, depth(4) = 5 + 1
    assert tw["spanning"] == [5, 5] and tw["partial"] == [1, 0]
    assert tw["jtables"][0] == [(0x0000000000000000, 3, (3, 0, 0)), (0x1110000000000000, 2, (0, 2, 0))]
    # run 1: the substitutions ride together: one joined allele of two reads, not two records that forgot each other
    assert tw["jtables"][1] == [(0x0000000000000000, 3, (3, 0, 0)), (0x1100000000000000, 2, (0, 2, 0))]
    assert tw["ent_joined"] == [[0] * 5] * 3 + [[1] * 5] * 2 + [[NONE, NONE]]
    text = [[jt.jtext(k, tw["tables"][b:e]) for k, _, _ in tab] for tab, b, e in zip(tw["jtables"], tw["run_begin"], tw["run_begin"][1:])]
    assert text == [[("-", False), ("GCA", False)], [("CA", False), ("GT", False)]]
    # the key: a nibble a site from the top, 15 for "allele 15 or later"
    assert jt.jkey([1, 2, 3]) == 0x123 << 52 and jt.jkey([15, 16, 40, 14]) == 0xFFFE << 48 and jt.jkey([0] * 16) == 0 and jt.jkey([1] * 16) == int("1" * 16, 16)
    # the runs: a stretch is cut from its first site every 16; a gap of one position begins another stretch
    assert jt.run_begins(list(range(5, 38))) == [0, 16, 32] and jt.run_begins([3, 4, 6, 7, 8]) == [0, 2] and jt.run_begins([]) == []
    assert jt.run_begins(list(range(16)) + list(range(17, 34))) == [0, 16, 32]
    # the lines
    ln = jt.joined_alleles_line("c", 4, 3, bb[4:7], 5, 1, "-", 3, (3, 0, 0))
    assert ln == "c\t5\t7\tGCA\t5\t1\t-\t3\t3\t0\t0"
    tab = [(t, o, c, h) for (t, o), (_, c, h) in zip(text[0], tw["jtables"][0])]
    assert jt.vcf_record("c", bb, 4, 3, 5, 1, tab, 2, True) == "c\t4\t.\tTGCA\tT\t.\t.\tDP=5;PART=1;AD=2,3;AD1=0,3;AD2=2,0"
    tab = [(t, o, c, h) for (t, o), (_, c, h) in zip(text[1], tw["jtables"][1])]
    assert jt.vcf_record("c", bb, 8, 2, 5, 0, tab, 2, False) == "c\t9\t.\tCA\tGT\t.\t.\tDP=5;PART=0;AD=3,2"
    assert jt.vcf_record("c", bb, 8, 2, 5, 0, tab, 3, False) is None


def _invariants(tw):
    """The defining invariants of one target's twin arrays."""
    rb = tw["run_begin"]
    assert rb[0] == 0 or not tw["sites"]
    per_site = [Counter() for _ in tw["sites"]]                           # entries of the spanning members, by allele index
    depth_part = Counter()
    for x, (e, ia, ij) in enumerate(zip(tw["ents"], tw["ent_allele"], tw["ent_joined"])):
        assert len(e) == len(ij)
        assert [k for k, _ in e] == list(range(e[0][0], e[0][0] + len(e))) if e else True       # consecutive sites
        for (k, _), a, j in zip(e, ia, ij):
            if j == NONE:
                depth_part[k] += 1
            else:
                per_site[k][min(a, 15)] += 1
    for r, tab in enumerate(tw["jtables"]):
        m = rb[r + 1] - rb[r]
        assert 1 <= m <= jt.SITES
        assert sum(c for _, c, _ in tab) == tw["spanning"][r] and all(sum(h) == c for _, c, h in tab)
        assert [(-c, kk) for kk, c, _ in tab] == sorted((-c, kk) for kk, c, _ in tab) and len({kk for kk, _, _ in tab}) == len(tab)
        assert all(kk & ((1 << (4 * (16 - m))) - 1) == 0 for kk, _, _ in tab)
        for j in range(m):
            k = rb[r] + j
            # 10.2: the depth of every site of the run
            assert pt.depth(tw["counts"][tw["sites"][k]]) == tw["spanning"][r] + depth_part[k]
            # marginalising the run's table over site j gives the site's table restricted to the spanning members
            marg = Counter()
            for kk, c, _ in tab:
                marg[(kk >> (4 * (15 - j))) & 15] += c
            assert marg == per_site[k]
    # a member is partial in a run, or all its entries there carry the index of one joined allele
    members = Counter()
    for x, (e, ij) in enumerate(zip(tw["ents"], tw["ent_joined"])):
        for r in range(len(rb) - 1):
            mine = [j for (k, _), j in zip(e, ij) if rb[r] <= k < rb[r + 1]]
            if mine:
                members[(r, mine[0] != NONE)] += 1
                assert len(set(mine)) == 1 and (len(mine) == rb[r + 1] - rb[r]) == (mine[0] != NONE)
    assert [members[(r, True)] for r in range(len(rb) - 1)] == tw["spanning"] and [members[(r, False)] for r in range(len(rb) - 1)] == tw["partial"]


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    n_runs = n_long = n_part = n_multi = 0
    rng = np.random.default_rng(10)
    for k in range(300):
        # (whole and partial reads under both pairs of thresholds: k % 2 picks the reads, k // 2 % 2 the thresholds)
        alns, bb = _tes()._small_pileup(rng, k)
        tw = jt.target(len(bb), alns, 4, int(rng.integers(0, 3)), (0, 0) if k // 2 % 2 else (2, 200000))
        _invariants(tw)
        n_runs += len(tw["spanning"]); n_long += sum(1 for a, b in zip(tw["run_begin"], tw["run_begin"][1:]) if b - a > 1)
        n_part += sum(1 for p in tw["partial"] if p); n_multi += sum(1 for t in tw["jtables"] if len(t) > 2)
    print("runs %d, of more than one site %d, with partial members %d, with more than two joined alleles %d" % (n_runs, n_long, n_part, n_multi))
    assert n_runs > 500 and n_long > 300 and n_part > 100 and n_multi > 100


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in ("dagcon_set_site_join", "dagcon_fetch_joined_sites"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = '#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %u\\n", sizeof(dagcon_joined_sites), DG_JN_SITES); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert ctypes.sizeof(capi.JoinedSites) == int(out[0]) == 80 and int(out[1]) == jt.SITES == 16
    for m in ("set_site_join", "joined_sites"):
        assert callable(getattr(capi.Context, m))
    assert lib.dagcon_abi_version() == 2


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for flag in ("--joined-alleles", "--joined-vcf"):
        f = tmp_path / ("o" + flag)
        # every refusal of --site-alleles (test_site_alleles.test_usage_errors_and_help)
        for args, why in (([str(m5), flag], b"needs a file name"),
                          (rec + ["--window", "200", "--overlap", "120", flag, str(f), str(sam)], b"do not go with --window, -a or --polish (they go where --site-reads goes)"),
                          (["-a", flag, str(f), str(m5)], b"do not go with --window, -a or --polish"), (["-a", "--polish", "1", flag, str(f), str(m5)], b"do not go with --window, -a or --polish"),
                          (rec + ["--dump-parsed", flag, str(f), str(sam)], b"do not go with --dump-parsed (nothing is run, the files would not be written)"),
                          ([flag, str(f), "--site-min-frac", "1.5", str(m5)], b"PARSE ERROR")):
            out = run(*args)
            assert out.returncode == 2 and b"PARSE ERROR" in out.stderr and why in out.stderr, (args, out.stderr)
            assert not f.exists()
        out = run(*rec, flag, str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr, flag
    # --joined-vcf needs the target's bases: refused on .m5 input; --joined-alleles is not, and it takes the sites' thresholds
    out = run("--joined-vcf", str(tmp_path / "o.vcf"), str(m5))
    assert out.returncode == 2 and b"--joined-vcf needs --sam, --bam or --paf" in out.stderr and not (tmp_path / "o.vcf").exists()
    out = run("--joined-alleles", str(tmp_path / "no_such_dir" / "o.txt"), "--site-min-frac", "0.3", "--site-min-count", "3", str(m5))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --joined-alleles FILE")[1].split(b"\n  -v, --verbose")[0]
    assert b"RNAME POS END REF SPAN PARTIAL ALLELE COUNT H1 H2 H0" in text and b"\n  --joined-vcf FILE" in text
    flat = b" ".join(text.split())
    assert b"RNAME POS . REF ALT . . DP=span;PART=partial;AD=ref,alt1,.." in flat and b"AD1=..;AD2=.." in flat
    assert b"bases of REF and ALT are NOT trimmed" in flat and b"No genotype is called" in flat and b"A deletion of three bases is one record" in flat
    assert b"[--site-vcf FILE] [--joined-alleles FILE] [--joined-vcf FILE]" in h.stdout.split(b"\n")[0]


_JN_MAIN = r"""
#include <iostream>
#include "joined.h"
// stdin: "t m key (n_al key..) x m"                                      -> the text of a joined key over m site tables
//        "a rname pos0 m ref span part text count split c1 c2 c0"
//        "h split n name len .."
//        "v rname tb pos0 m span part min_count split n (text opaque count c1 c2 c0).."
int main() {
    std::string out, kind, rname, tb;
    while (std::cin >> kind) {
        if (kind == "t") {
            unsigned m; unsigned long long key;
            std::cin >> m >> key;
            std::vector<uint64_t> begin(1, 0), keys;
            for (unsigned j = 0; j < m; j++) { unsigned n; std::cin >> n; while (n--) { unsigned long long k; std::cin >> k; keys.push_back(k); } begin.push_back(keys.size()); }
            keys.push_back(0);
            std::string text;
            const bool plain = dg_joined_text(text, key, begin.data(), keys.data(), 0, m);
            out += text + (plain ? " plain\n" : " opaque\n");
        } else if (kind == "a") {
            unsigned long long pos; unsigned m, span, part, count, split, h[3]; std::string ref, text;
            std::cin >> rname >> pos >> m >> ref >> span >> part >> text >> count >> split >> h[0] >> h[1] >> h[2];
            const uint16_t hap[3] = {(uint16_t)h[0], (uint16_t)h[1], (uint16_t)h[2]};
            dg_joined_allele_line(out, rname, pos, m, ref == "." ? nullptr : ref.data(), span, part, text, count, split ? hap : nullptr);
        } else if (kind == "h") {
            unsigned split, k; std::string contigs, name; unsigned len;
            std::cin >> split >> k;
            while (k--) { std::cin >> name >> len; contigs += "##contig=<ID=" + name + ",length=" + std::to_string(len) + ">\n"; }
            dg_joined_vcf_header(out, contigs, split != 0);
        } else {
            unsigned pos, m, span, part, min_count, split, n;
            std::cin >> rname >> tb >> pos >> m >> span >> part >> min_count >> split >> n;
            std::vector<std::string> text(n); std::vector<uint8_t> opaque(n); std::vector<uint32_t> count(n); std::vector<uint16_t> hap(3 * n + 3);
            for (unsigned i = 0; i < n; i++) { unsigned o, h[3]; std::cin >> text[i] >> o >> count[i] >> h[0] >> h[1] >> h[2]; opaque[i] = (uint8_t)o; for (int j = 0; j < 3; j++) hap[3 * i + j] = (uint16_t)h[j]; }
            const size_t before = out.size();
            dg_joined_vcf_record(out, rname, tb.data(), (uint32_t)tb.size(), pos, m, span, part, text, opaque, count.data(), split ? hap.data() : nullptr, min_count);
            if (out.size() == before) out += "(none)\n";
        }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatters_against_python(tmp_path):
    """csrc/host/joined.h in a program of its own (built with the address and undefined-behaviour sanitizers) against the twin's lines."""
    src = tmp_path / "jn_main.cpp"; src.write_text(_JN_MAIN)
    exe = tmp_path / "jn_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"), "-o", str(exe), str(src)])
    K = at.key
    many = [(K(bytes([b"ACGT"[i % 4], b"ACGT"[i // 4]])), 1) for i in range(16)] + [(K(b"TTT"), 1)]
    tabs = [[(K(b"A"), 5), (0, 3), (K(b"ACG"), 1)], [(0, 4), (K(b"C"), 3), (K(b"G" * 21), 2)], many]
    texts = [(0x000 << 52, tabs[:2]), (0x100 << 52, tabs[:2]), (0x210 << 52, tabs[:2]), (0x020 << 52, tabs[:2]), (0x00E << 52, tabs), (0x00F << 52, tabs), (0x11F << 52, tabs),
             (0x1 << 60, tabs[1:2]), (0x2 << 60, tabs[1:2])]
    lines = [("ctg", 0, 3, b"ACG", 7, 2, "-", 4, (1, 2, 1)), ("a/b|c", 4294967280, 16, None, 4094, 0, "*", 4094, None), ("x", 41, 1, b"n", 1, 0, "ACGTN", 1, (0, 0, 1))]
    tb = b"ACGTAcGTAC"
    tab = [("GT", False, 5, (3, 1, 1)), ("CT", False, 3, (0, 3, 0)), ("-", False, 2, (1, 1, 0)), ("*", True, 2, (2, 0, 0)), ("GTT", False, 2, (0, 0, 2)), ("CT", False, 2, (1, 1, 0)), ("G", False, 1, (0, 1, 0))]
    recs = [("c", tb, 2, 2, 17, 3, tab, 2, True),                    # anchored on the base in front: the empty allele among the ALTs; CT twice is one ALT; * and the rare one are left out
            ("c", tb, 2, 2, 17, 3, tab, 3, False),                   # min_count 3 leaves CT alone (its second line of 2 does not count): not anchored
            ("c", tb, 2, 2, 17, 3, tab, 1, True),                    # min_count 1: G comes in too
            ("c", tb[2:], 0, 2, 17, 3, tab, 2, True),                # position 0: anchored on the base behind the run
            ("c", tb, 2, 2, 5, 0, tab[:1], 1, True),                 # a run with no ALT
            ("c", tb, 2, 2, 17, 3, tab, 6, True),                    # ... no ALT deep enough
            ("c", b"GT", 0, 2, 17, 3, tab, 1, True),                 # a run that covers its whole target
            ("c", tb, 4, 2, 17, 3, tab, 2, False),                   # the REF bases are not in the table: AD begins with 0; the lower-case REF base is printed as it is
            ("c", b"ACgtAC", 2, 2, 17, 3, tab, 2, False)]            # ... and is the same allele as GT
    heads = [(True, [("c", 6), ("a/b|c", 70000)]), (False, [])]
    text = "".join("t %d %d %s\n" % (len(tt), kk, " ".join("%d %s" % (len(t), " ".join(str(k) for k, _ in t)) for t in tt)) for kk, tt in texts)
    text += "".join("a %s %d %d %s %d %d %s %d %d %s\n" % (r, p, m, ref.decode() if ref else ".", sp, pa, tx, c, 1 if h else 0, " ".join(map(str, h or (0, 0, 0))))
                    for r, p, m, ref, sp, pa, tx, c, h in lines)
    text += "".join("h %d %d %s\n" % (s, len(cs), " ".join("%s %d" % c for c in cs)) for s, cs in heads)
    text += "".join("v %s %s %d %d %d %d %d %d %d %s\n" % (r, t.decode(), p, m, sp, pa, mc, s, len(tt), " ".join("%s %d %d %d %d %d" % ((tx, o, c) + h) for tx, o, c, h in tt))
                    for r, t, p, m, sp, pa, tt, mc, s in recs)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    exp = ["%s %s" % (tx, "opaque" if o else "plain") for tx, o in (jt.jtext(kk, [[(k, c, None) for k, c in t] for t in tt]) for kk, tt in texts)]
    exp += [jt.joined_alleles_line(*x) for x in lines]
    for s, cs in heads:
        exp += jt.vcf_header(cs, s)
    exp += [jt.vcf_record(*x) or "(none)" for x in recs]
    assert out == exp
    assert exp[:9] == ["A plain", "-" + " plain", "ACGC plain", "* opaque", "AGT plain", "* opaque", "* opaque", "C plain", "* opaque"]
    assert exp[9] == "ctg\t1\t3\tACG\t7\t2\t-\t4\t1\t2\t1" and exp[10] == "a/b|c\t4294967281\t4294967296\t.\t4094\t0\t*\t4094\t.\t.\t."
    v = exp[-len(recs):]
    assert v[0] == "c\t2\t.\tCGT\tCCT,C,CGTT\t.\t.\tDP=17;PART=3;AD=5,5,2,2;AD1=3,1,1,0;AD2=1,4,1,0"
    assert v[1] == "c\t3\t.\tGT\tCT\t.\t.\tDP=17;PART=3;AD=5,3" and v[2].split("\t")[4] == "CCT,C,CGTT,CG"
    assert v[3] == "c\t1\t.\tGTA\tCTA,A,GTTA\t.\t.\tDP=17;PART=3;AD=5,5,2,2;AD1=3,1,1,0;AD2=1,4,1,0"
    assert v[4] == v[5] == v[6] == "(none)" and v[7].split("\t")[3:5] == ["TAc", "TGT,TCT,T,TGTT"] and v[7].endswith("AD=0,5,5,2,2")
    assert v[8].split("\t")[3:5] == ["Cgt", "CCT,C,CGTT"]
    assert any("not trimmed" in x for x in exp) and any("no genotype is called" in x for x in exp)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _device(call, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None):
    """One context with the pile-up, the site reads, the alleles and the switch on: everything it gives."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*opts)
        c.set_site_reads(phase, rounds)
        c.set_site_alleles(True)
        c.set_site_join(True)
        got = call(c)
        js = c.joined_sites()
        return {"got": got, "js": js, "sa": c.site_alleles(), "sr": c.site_reads(), "ps": c.pileup_sites(), "pu": c.pileup(), "status": c.target_status.tolist(),
                "reruns": c.timings()["reruns"]}
    finally:
        c.close()


def _expect(strings, tlens, min_cov, min_len, trim, opts, rounds=0, status=None, n_given=None, src=None):
    """test_site_alleles._expect's arrays and the join's, from one twin run per target; "tw": the twin's dict per target."""
    out = {k: [] for k in ("aln_tgt", "aln_src", "ent_site", "ent_code", "hap", "phase", "pos", "key", "count", "hap_count", "ent_allele",
                           "run_begin", "spanning", "partial", "jkey", "jcount", "jhap", "ent_joined", "tw")}
    out["ent_begin"], out["site_begin"], out["al_begin"], out["jal_begin"] = [0], [0], [0], [0]
    status = status or [0] * len(strings)
    base = 0
    for t, (s, tl) in enumerate(zip(strings, tlens)):
        n_al = 0 if s is None else len(s[1])
        tw = None
        if s is not None and not status[t] and n_al >= max(1, min_cov):
            tw = jt.target(tl, s[1], min_len, trim, opts, rounds or srt.ROUNDS)
            sb = len(out["pos"])
            for i, e, h, ia, ij in zip(tw["src"], tw["ents"], tw["hap"], tw["ent_allele"], tw["ent_joined"]):
                out["aln_tgt"].append(t); out["aln_src"].append(src[t][i] if src is not None else base + i); out["hap"].append(h)
                out["ent_site"] += [sb + k for k, _ in e]; out["ent_code"] += [c for _, c in e]; out["ent_allele"] += ia; out["ent_joined"] += ij
                out["ent_begin"].append(len(out["ent_site"]))
            out["pos"] += tw["sites"]; out["phase"] += tw["phase"]
            for tab in tw["tables"]:
                out["key"] += [kk for kk, _, _ in tab]; out["count"] += [c for _, c, _ in tab]; out["hap_count"] += [list(h) for _, _, h in tab]
                out["al_begin"].append(len(out["key"]))
            out["run_begin"] += [sb + b for b in tw["run_begin"][:-1]]; out["spanning"] += tw["spanning"]; out["partial"] += tw["partial"]
            for tab in tw["jtables"]:
                out["jkey"] += [kk for kk, _, _ in tab]; out["jcount"] += [c for _, c, _ in tab]; out["jhap"] += [list(h) for _, _, h in tab]
                out["jal_begin"].append(len(out["jkey"]))
        out["tw"].append(tw)
        out["site_begin"].append(len(out["pos"]))
        base += n_given[t] if n_given is not None else n_al
    out["run_begin"].append(len(out["pos"]))
    return out


def _check(dev, exp, phase=True):
    js, sa, sr, ps = dev["js"], dev["sa"], dev["sr"], dev["ps"]
    _tsa()._check(dev, exp, phase)
    for k, e in (("run_begin", "run_begin"), ("spanning", "spanning"), ("partial", "partial"), ("jal_begin", "jal_begin"), ("key", "jkey"), ("count", "jcount"),
                 ("ent_joined", "ent_joined")):
        assert js[k].tolist() == exp[e], k
    if phase:
        assert js["hap_count"].tolist() == exp["jhap"]
    else:
        assert js["hap_count"] is None
    # from the device's own arrays: the runs tile the sites, the counts are the spanning members' recount, and the key of
    # every spanning member is its entries' alleles, a nibble each
    rb = js["run_begin"].astype(np.int64)
    assert rb.size == js["spanning"].size + 1 and js["ent_joined"].size == sr["ent_site"].size and (np.diff(rb) >= 1).all() and (np.diff(rb) <= 16).all()
    site = sr["ent_site"].astype(np.int64)
    run = np.searchsorted(rb, site, side="right") - 1
    ej = js["ent_joined"].astype(np.int64)
    span = ej != NONE
    assert (ej[span] < np.diff(js["jal_begin"]).astype(np.int64)[run[span]]).all()
    head = span & (site == rb[run])
    at_ = js["jal_begin"][:-1].astype(np.int64)[run[head]] + ej[head]
    assert np.array_equal(np.bincount(at_, minlength=js["key"].size), js["count"].astype(np.int64))
    assert np.array_equal(np.bincount(run[head], minlength=js["spanning"].size), js["spanning"].astype(np.int64))
    nib = np.minimum(sa["ent_allele"].astype(np.uint64), np.uint64(15)) << (np.uint64(4) * (np.uint64(15) - (site - rb[run]).astype(np.uint64)))
    full = js["jal_begin"][:-1].astype(np.int64)[run[span]] + ej[span]
    got = np.zeros(js["key"].size, np.uint64)
    # (every member of one joined allele ors the same nibbles in)
    np.bitwise_or.at(got, full, nib[span])
    assert np.array_equal(got, js["key"])


def _run(call, strings, tlens, min_cov, min_len, trim, opts=(0, 0), phase=True, rounds=0, prepare=None, n_given=None, src=None, exp=None, status=None):
    exp = exp or _expect(strings, tlens, min_cov, min_len, trim, opts, rounds, status, n_given, src)
    dev = _device(call, min_cov, min_len, trim, opts, phase, rounds, prepare)
    assert dev["status"] == (status or [0] * len(strings))
    _check(dev, exp, phase)
    return dev, exp


def _strings_call(strings):
    return _tsa()._strings_call(strings)


def _runs(exp):
    return np.diff(exp["run_begin"]).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 2])
@pytest.mark.parametrize("opts", [(0, 0), (2, 200000)])
def test_random_small_targets(oracle_lib, trim, opts):
    """8 targets of 40-200 bases under 4-12 reads, the split on and off."""
    rng = np.random.default_rng(900 + trim)
    strings = []
    for k in range(8):
        alns, bb = random_target(rng, int(rng.integers(40, 201)), int(rng.integers(4, 13)), sub=0.05, ins=0.08, dele=0.06, full_span=bool(k % 2))
        strings.append((bb, alns))
    tlens = [len(bb) for bb, _ in strings]
    exp = _expect(strings, tlens, 3, 30, trim, opts)
    lens = _runs(exp)
    print("runs %d, longest %d, joined alleles %d, partial members %d" % (len(lens), max(lens), len(exp["jkey"]), sum(exp["partial"])))
    assert len(lens) > (50 if opts == (0, 0) else 40) and max(lens) == (16 if opts == (0, 0) else max(lens)) and max(lens) >= 3
    # (at 0 / 0 every read end lies inside a run; at 2 / 0.2 few do, and test_partial_members plants them)
    assert (sum(exp["partial"]) > 10 and NONE in exp["ent_joined"]) or opts != (0, 0)
    assert max(x for x in exp["ent_joined"] if x != NONE) >= 2
    for phase in (True, False):
        _run(_strings_call(strings), strings, tlens, 3, 30, trim, opts, phase, exp=exp)


def _stretch_target(rng, n, s, L):
    """n bases without equal neighbours whose bases [s, s + L) hold no T and whose base s + L is T: normalizeGaps pushes a
    gap to the right past every target base that equals the read's next base, so a deletion of [s, s + L) stays where it is
    only if none of its bases is the one behind it."""
    tes = _tes()
    while True:
        bb = tes._nonrep(rng, s) + tes._nonrep(rng, L, avoid=b"T") + b"T" + tes._nonrep(rng, n - s - L - 1)
        if all(bb[i] != bb[i + 1] for i in range(n - 1)):
            return bb


def _sub(bb, s, e, at_):
    """bases [s, e) of bb with another base at every position of at_."""
    q = bytearray(bb[s:e])
    for x in at_:
        q[x - s] = _other(bb[x])
    return (s + 1, bytes(q), bb[s:e])


@pytest.mark.gpu
def test_run_lengths(oracle_lib):
    """Stretches of 1, 2, 15, 16, 17, 32 and 33 adjacent sites, a target each: four reads delete the stretch, two put
    another base in its middle and two at its last position.  At 2 / 0.2 the stretch is the target's only sites."""
    tsa, tes = _tsa(), _tes()
    rng = np.random.default_rng(16)
    strings, want = [], []
    s = 20
    for L in (1, 2, 15, 16, 17, 32, 33):
        bb = _stretch_target(rng, 80, s, L)
        inside = [s + L // 2] + ([s + L - 1] if L > 1 else [])
        reads = [tsa._read(bb, 0, 80, dele=set(range(s, s + L)))] * 4 + [_sub(bb, 0, 80, inside[:1])] * 2 + [_sub(bb, 0, 80, inside[1:])] * 2
        strings.append((bb, reads)); want.append([16] * (L // 16) + ([L % 16] if L % 16 else []))
    tlens = [80] * len(strings)
    exp = _expect(strings, tlens, 3, 30, 0, (2, 200000))
    for tw, L, w in zip(exp["tw"], (1, 2, 15, 16, 17, 32, 33), want):
        assert tw["sites"] == list(range(s, s + L)) and np.diff(tw["run_begin"]).tolist() == w and tw["spanning"] == [8] * len(w) and tw["partial"] == [0] * len(w)
        assert all(len(t) >= 2 for t in tw["jtables"]) and tw["jtables"][0][0][:2] == (0, 4)
    assert want[4] == [16, 1] and want[6] == [16, 16, 1] and want[5] == [16, 16] and want[3] == [16] and want[2] == [15]
    _run(_strings_call(strings), strings, tlens, 3, 30, 0, (2, 200000), exp=exp)


@pytest.mark.gpu
def test_partial_members(oracle_lib):
    """A run of five sites [s, s + 5) under eight whole reads; beside them reads that begin at the run's first site, one
    position behind it, at its last site and one behind that, and reads whose last base is at each of those four."""
    tsa, tes = _tsa(), _tes()
    s, L = 40, 5
    bb = _stretch_target(np.random.default_rng(5), 90, s, L)
    whole = [tsa._read(bb, 0, 90, dele=set(range(s, s + L)))] * 4 + [_sub(bb, 0, 90, [s + 2])] * 4
    begins = [tsa._read(bb, a, 90) for a in (s, s + 1, s + L - 1, s + L)]
    ends = [tsa._read(bb, 0, e + 1) for e in (s, s + 1, s + L - 1, s + L)]
    reads = whole + begins + ends
    exp = _expect([(bb, reads)], [90], 3, 30, 0, (2, 200000))
    tw = exp["tw"][0]
    # spanning: the eight, the read that begins at s, the two that end at the last site and behind it; partial: two and two
    assert tw["sites"] == list(range(s, s + L)) and tw["spanning"] == [11] and tw["partial"] == [4] and len(tw["src"]) == 16
    assert [ij.count(NONE) for ij in tw["ent_joined"]] == [0] * 8 + [0, 4, 1, 0] + [1, 2, 0, 0] and [len(ij) for ij in tw["ent_joined"]][8:] == [5, 4, 1, 0, 1, 2, 5, 5]
    _run(_strings_call([(bb, reads)]), [(bb, reads)], [90], 3, 30, 0, (2, 200000), exp=exp)


@pytest.mark.gpu
def test_the_64_entry_period(oracle_lib):
    """At 0 / 0 every position is a site and an entry: reads that begin 0 .. 15 bases behind the first covered base f have
    the head of the run at f + 64 at entries 64, 63 .. 49 and that of the run at f + 80 at entries 80, 79 .. 65: runs of 16
    that begin in every lane from 49 to 63 and straddle the entry loop's step, with 63, 64 and 65 entries in front."""
    tsa, tes = _tsa(), _tes()
    rng = np.random.default_rng(64)
    bb = tes._nonrep(rng, 200)
    f = 10
    reads = []
    for a in range(f, f + 16):
        wrong = sorted(set(int(x) for x in rng.integers(f + 60, f + 100, 3)))
        reads.append(_sub(bb, a, 190, wrong) if a % 3 else tsa._read(bb, a, 190, dele={f + 70, f + 71} if a % 2 else {f + 66}))
    reads += [tsa._read(bb, f, 190)] * 3
    exp = _expect([(bb, reads)], [200], 3, 30, 0, (0, 0))
    tw = exp["tw"][0]
    heads = set(tw["run_begin"][:-1])
    front = {i for e in tw["ents"] for i, (k, _) in enumerate(e) if k in heads and i + 16 <= len(e)}
    assert tw["sites"] == list(range(f, 190)) and set(range(49, 66)) <= front and {63, 64, 65} <= front
    assert np.diff(tw["run_begin"]).tolist() == [16] * 11 + [4] and max(len(t) for t in tw["jtables"]) >= 4 and sum(tw["partial"]) >= 15
    _run(_strings_call([(bb, reads)]), [(bb, reads)], [200], 3, 30, 0, (0, 0), exp=exp)


def _stairs():
    """A target of 40 bases under reads that all begin at its first base: 100 of 10 bases, one of 20, one of 33 and 63 of 40.  At
    0 / 0 the runs are [0, 16), [16, 32) and [32, 40): 65 alignments span the first (a block sorts their keys), 64 the
    second (a wave does), 63 the third.  Read r puts other bases at 1 + r % 8, 17 + r % 7 and 33 + r % 5."""
    bb = _tes()._nonrep(np.random.default_rng(65), 40)
    reads = []
    for r, e in enumerate([40] * 63 + [33, 20] + [10] * 100):
        q = bytearray(bb[:e])
        for x, k in ((1 + r % 8, r // 8), (17 + r % 7, r // 7), (33 + r % 5, r // 5)):
            if x < e and k % 4:
                q[x] = _other(bb[x], k % 4 - 1)
        reads.append((1, bytes(q), bb[:e]))
    return bb, reads


@pytest.mark.gpu
def test_the_sort_hand_over(oracle_lib):
    bb, reads = _stairs()
    exp = _expect([(bb, reads)], [40], 3, 5, 0, (0, 0))
    tw = exp["tw"][0]
    assert np.diff(tw["run_begin"]).tolist() == [16, 16, 8] and tw["spanning"] == [65, 64, 63] and tw["partial"] == [100, 1, 1]
    assert [len(t) for t in tw["jtables"]] >= [20, 20, 10] and pt.depth(tw["counts"][0]) == 165
    _run(_strings_call([(bb, reads)]), [(bb, reads)], [40], 3, 5, 0, (0, 0), exp=exp)


@pytest.mark.gpu
def test_the_deepest_run(oracle_lib):
    """test_site_alleles.test_the_deepest_site's batch, 40 bases at depth 4,094, with one adjacent site more: every second
    read inserts eight bases that spell its number behind base 20, every third puts another base at 21.  At 2 / 0.2 those
    two positions are the sites, one run that all 4,094 alignments span: the most a block sorts."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(4094)
    bb = b"A" * 40
    wrong = rng.random((capi.MAX_COVERAGE, 40)) < 0.02
    alns = []
    for r in range(capi.MAX_COVERAGE):
        q, t = bytearray(), bytearray()
        for x in range(40):
            q.append(b"CGT"[r % 3] if (wrong[r, x] and x not in (20, 21)) or (x == 21 and r % 3 == 0) else bb[x]); t.append(bb[x])
            if x == 20 and r % 2 == 0:
                q += bytes(b"CGT"[(r // 3 ** j) % 3] for j in range(8)); t += b"-" * 8
        alns.append((1, bytes(q), bytes(t)))
    exp = _expect([(bb, alns)], [40], 6, 5, 0, (2, 200000))
    tw = exp["tw"][0]
    assert tw["sites"] == [20, 21] and tw["run_begin"] == [0, 2] and tw["spanning"] == [4094] and tw["partial"] == [0]
    # 2,047 reads with a run of their own and the bare base: 2,048 alleles at 20.  Indices 1 .. 14 are one read each, so one
    # joined allele each; index 0 and "15 or later" meet both alleles of 21: 14 + 2 + 2
    assert len(tw["tables"][0]) == 2048 and len(tw["tables"][1]) == 2 and len(tw["jtables"][0]) == 18 and max(ia[0] for ia in tw["ent_allele"]) == 2047
    _run(_strings_call([(bb, alns)]), [(bb, alns)], [40], 6, 5, 0, (2, 200000), phase=False, exp=exp)


def _capped(n):
    """30 bases under 20 whole reads: read r < n - 1 inserts the r-th three-base word over A C G (in the keys' order; base 11
    is T, so normalizeGaps leaves the word where it is) behind base 10, the others nothing: n alleles at site 10, index 0 the
    bare base, index r + 1 read r's.  Reads 2 3, 6 7, 10 11, 14 15 and 18 19 put A at 11: ten A and ten T there, A first."""
    bb = b"ACGTACGTACATGCATGCATGCTAGCTAGC"
    words = [bytes(w) for w in itertools.product(b"ACG", repeat=3)]
    reads = []
    for r in range(20):
        q, t = bytearray(), bytearray()
        for x in range(30):
            q.append(_other(bb[x]) if x == 11 and r // 2 % 2 else bb[x]); t.append(bb[x])
            if x == 10 and r < n - 1:
                q += words[r]; t += b"---"
        reads.append((1, bytes(q), bytes(t)))
    return bb, reads


@pytest.mark.gpu
def test_the_nibble_cap(oracle_lib):
    strings = [_capped(n) for n in (15, 16, 17)]
    exp = _expect(strings, [30] * 3, 3, 5, 0, (2, 200000))
    seen = set()
    for n, tw, (bb, _) in zip((15, 16, 17), exp["tw"], strings):
        assert tw["sites"] == [10, 11] and tw["run_begin"] == [0, 2] and tw["spanning"] == [20] and len(tw["tables"][0]) == n
        seen |= {ia[0] for ia in tw["ent_allele"]}
        assert [ia[0] for ia in tw["ent_allele"]][:n - 1] == list(range(1, n))
        tab = tw["jtables"][0]
        capped = [(kk, c) for kk, c, _ in tab if kk >> 60 == 15]
        # index 14 keeps a nibble of its own; 15 and 16, on reads 14 and 15 with the same base at 11, are one joined allele
        assert any(kk >> 60 == 14 for kk, _, _ in tab) == (n >= 15) and capped == {15: [], 16: [(0xF0 << 56, 1)], 17: [(0xF0 << 56, 2)]}[n]
        texts = [jt.jtext(kk, tw["tables"]) + (c, h) for kk, c, h in tab]
        assert [t[:3] for t in texts if t[1]] == [("*", True, c) for _, c in capped]
        rec = jt.vcf_record("c", bb, 10, 2, 20, 0, texts, 1, False)
        assert "*" not in rec and len(rec.split("\t")[4].split(",")) == len(tab) - 1 - len(capped)
    assert {14, 15, 16} <= seen
    _run(_strings_call(strings), strings, [30] * 3, 3, 5, 0, (2, 200000), exp=exp)


@pytest.mark.gpu
def test_the_target_boundary(oracle_lib):
    """Two targets: the last position of the first and position 0 of the second are their only sites.  Two runs."""
    tes = _tes()
    rng = np.random.default_rng(2)
    a, b = tes._nonrep(rng, 50), tes._nonrep(rng, 60)
    strings = [(a, [_sub(a, 0, 50, [49])] * 3 + [_sub(a, 0, 50, [])] * 3), (b, [_sub(b, 0, 60, [0])] * 3 + [_sub(b, 0, 60, [])] * 3)]
    exp = _expect(strings, [50, 60], 3, 30, 0, (2, 200000))
    assert exp["pos"] == [49, 0] and exp["site_begin"] == [0, 1, 2] and exp["run_begin"] == [0, 1, 2] and exp["spanning"] == [6, 6]
    _run(_strings_call(strings), strings, [50, 60], 3, 30, 0, (2, 200000), exp=exp)
    # ... and at 0 / 0, where every position of both is a site: no run holds sites of both
    exp = _expect(strings, [50, 60], 3, 30, 0, (0, 0))
    assert _runs(exp) == [16, 16, 16, 2] + [16, 16, 16, 12] and 50 in exp["run_begin"]
    _run(_strings_call(strings), strings, [50, 60], 3, 30, 0, (0, 0), exp=exp)


@pytest.mark.gpu
def test_a_batch_with_a_failed_target(oracle_lib):
    """test_site_alleles.test_a_batch_with_a_failed_target's batch: the failed target has no runs, and the runs of the
    targets behind it still line up with the sites."""
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
    status = [0] * 40; status[bad] = NONCONFORMING
    tlens = [len(bb) for bb, _ in targets]
    exp = _expect(strings, tlens, 3, 4, 1, (0, 0), status=status, n_given=[len(r) for _, r in targets])
    assert exp["tw"][bad] is None and len(exp["spanning"]) > 80 and exp["site_begin"][bad] == exp["site_begin"][bad + 1] and sum(exp["partial"]) > 50
    assert any(exp["site_begin"][bad] == b for b in exp["run_begin"])
    _run(tes._whole(targets), strings, tlens, 3, 4, 1, (0, 0), exp=exp, status=status)


@pytest.mark.gpu
def test_arena_growth(oracle_lib):
    """test_site_alleles.test_arena_growth's batch: the entries outgrow the arena's first size and the batch runs again;
    the cursors and the partial counts start from zero again, so nothing is counted twice."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    alns, bb = random_target(rng, 400, 40, full_span=True, sub=0.02, ins=0.03, dele=0.03)
    batch = batch_from_targets([(400, alns, None)])
    assert sum(len(q) for _, q, _ in alns) // 64 + 4096 < 40 * 380
    exp = _expect([(bb, alns)], [400], 3, 30, 5, (0, 0))
    assert len(exp["ent_joined"]) > 40 * 380 and sum(exp["spanning"]) > 20 * 36 and len(exp["spanning"]) >= 24
    dev, _ = _run(lambda c: c.consensus(batch), [(bb, alns)], [400], 3, 30, 5, (0, 0), exp=exp)
    off = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        off.set_pileup(0, 0)
        got_off = off.consensus(batch)
        reruns_off = off.timings()["reruns"]
    finally:
        off.close()
    assert dev["reruns"] > reruns_off and dev["got"] == got_off


@pytest.mark.gpu
def test_every_way_in_gives_the_same_arrays(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(91, 12, 150, 400, full_span=True)
    strings = tes._strings(targets)
    tlens = [len(bb) for bb, _ in targets]
    exp = _expect(strings, tlens, 3, 30, 5, (2, 200000))
    assert len(exp["jkey"]) > 100 and max(_runs(exp)) >= 2
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    cs = capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs]) for bb, recs in targets])
    calls = {"strings": _strings_call(strings), "cigar": lambda c: c.consensus_cigar(plain), "cs": lambda c: c.consensus_cs(cs)}
    ref = None
    for kind, call in calls.items():
        dev, _ = _run(call, strings, tlens, 3, 30, 5, (2, 200000), exp=exp)
        ref = ref or dev["js"]
        for k in ref:
            assert np.array_equal(dev["js"][k], ref[k]), (kind, k)


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    # what a context gives with the switch off: the consensus, the pile-up, the sites, the site reads, the alleles, the tally
    plain = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        plain.set_pileup(2, 200000); plain.set_site_reads(True); plain.set_site_alleles(True); plain.set_hap_consensus(1, 2)
        want = plain.consensus_cigar(cb)
        want_all = (plain.pileup_sites(), plain.pileup(), plain.site_reads(), plain.site_alleles(), plain.hap_tally())
        assert _code(plain.joined_sites) == STATE                      # the switch off at the upload
    finally:
        plain.close()
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        assert _code(c.joined_sites) == STATE                          # nothing yet
        c.set_site_join(True)
        assert c.consensus_cigar(cb) == want                           # everything it rests on off at the upload
        assert _code(c.joined_sites) == STATE and _code(c.site_reads) == STATE
        c.set_pileup(2, 200000); c.set_site_reads(True)
        assert c.consensus_cigar(cb) == want                           # the alleles off
        assert _code(c.joined_sites) == STATE and _code(c.site_alleles) == STATE and c.site_reads()["ent_site"].size > 0
        c.set_site_alleles(True); c.set_site_reads(None)
        assert c.consensus_cigar(cb) == want                           # the site reads off
        assert _code(c.joined_sites) == STATE
        c.set_site_reads(True); c.set_hap_consensus(1, 2)
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.joined_sites) == STATE                          # before a fetch
        assert c.fetch() == want
        first = c.joined_sites()
        assert first["key"].size > 0 and first["hap_count"][:, :2].any() and first["spanning"].size > 0
        again = c.joined_sites()                                       # asked twice
        assert all(np.array_equal(first[k], again[k]) for k in first)
        # with the switch on everything else is byte for byte what it is with it off
        got_all = (c.pileup_sites(), c.pileup(), c.site_reads(), c.site_alleles(), c.hap_tally())
        for a, b in zip(got_all, want_all):
            assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        c.set_site_join(False)                                         # off: this batch's results stay, the next has none
        assert np.array_equal(c.joined_sites()["key"], first["key"])
        assert c.consensus_cigar(cb) == want
        assert _code(c.joined_sites) == STATE and c.site_alleles()["key"].size > 0
        c.set_site_join(True)                                          # and on again
        assert c.consensus_cigar(cb) == want
        third = c.joined_sites()
        assert all(np.array_equal(first[k], third[k]) for k in first)
        c.upload_haps()                                                # the derived batch has it off
        assert _code(c.joined_sites) == STATE
        c.run(); c.fetch()
        assert _code(c.joined_sites) == STATE
        c.set_site_join(False)
        c.upload_cigar(cb)                                             # a later upload
        assert _code(c.joined_sites) == STATE
    finally:
        c.close()
    for flag in (capi.FLAG_STOP_AFTER_MERGE, capi.FLAG_STOP_AFTER_BUILD):
        stop = capi.Context(min_cov=3, min_len=30, trim=5, flags=flag)
        try:
            stop.set_pileup(2, 200000); stop.set_site_reads(True); stop.set_site_alleles(True); stop.set_site_join(True)
            stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
            assert _code(stop.joined_sites) == STATE
        finally:
            stop.close()


def _cli_lines(strings, names, tl, opts, split, with_ref=True):
    lines, vcf = [], jt.vcf_header(list(zip(names, tl)), split)
    for g, (bb, alns) in enumerate(strings):
        tw = jt.target(tl[g], alns, 30, 5, opts)
        rb = tw["run_begin"]
        for r, tab in enumerate(tw["jtables"]):
            p, m = tw["sites"][rb[r]], rb[r + 1] - rb[r]
            texts = [jt.jtext(kk, tw["tables"][rb[r]:rb[r + 1]]) + (c, h) for kk, c, h in tab]
            lines += [jt.joined_alleles_line(names[g], p, m, bb[p:p + m] if with_ref else None, tw["spanning"][r], tw["partial"][r], tx, c, h if split else None) for tx, _, c, h in texts]
            rec = jt.vcf_record(names[g], bb, p, m, tw["spanning"][r], tw["partial"][r], texts, opts[0], split)
            if rec:
                vcf.append(rec)
    return lines, vcf


@pytest.mark.gpu
def test_pbdagcon_joined_alleles_and_joined_vcf(oracle_lib, tmp_path):
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
    f = {k: tmp_path / k for k in ("a", "v", "sv", "sv0", "sa", "sa0", "a2", "v2", "h", "a3")}
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    rec = ["--sam", "--ref", str(ref)]
    lines, vcf = _cli_lines(strings, names, tl, (2, 200000), False)
    assert len(lines) > 100 and len(vcf) > 20 + 11 and any(int(x.split("\t")[2]) > int(x.split("\t")[1]) for x in lines) and any(len(x.split("\t")[3]) > 2 for x in vcf[-20:])

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    plain = run(*rec, "--site-vcf", str(f["sv0"]), "--site-alleles", str(f["sa0"]), str(sam))
    got = run(*rec, "--joined-alleles", str(f["a"]), "--joined-vcf", str(f["v"]), "--site-vcf", str(f["sv"]), "--site-alleles", str(f["sa"]), str(sam))
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 8
    # the sites' own files, written in the same command, are what they are without the new flags
    assert f["sv"].read_bytes() == f["sv0"].read_bytes() and f["sa"].read_bytes() == f["sa0"].read_bytes() and f["sv"].stat().st_size > 1000
    assert f["a"].read_text().splitlines() == lines and all(x.endswith("\t.\t.\t.") for x in lines)
    assert f["v"].read_text().splitlines() == vcf
    # the two flags alone, with the split on
    got = run(*rec, "--joined-alleles", str(f["a2"]), "--joined-vcf", str(f["v2"]), "--haplotag", str(f["h"]), str(sam))
    assert got.stdout == plain.stdout
    lines, vcf = _cli_lines(strings, names, tl, (2, 200000), True)
    assert f["a2"].read_text().splitlines() == lines and f["v2"].read_text().splitlines() == vcf and any(";AD1=" in x for x in vcf)
    # the .m5 of the same alignments: no REF, other thresholds, two batches
    got = run("--joined-alleles", str(f["a3"]), "--site-min-frac", "0.3", "--site-min-count", "3", "--batch-targets", "5", "-j", "2", str(m5))
    assert got.stdout == run(str(m5)).stdout
    lines, _ = _cli_lines(strings, names, tl, (3, 300000), False, with_ref=False)
    assert f["a3"].read_text().splitlines() == lines and len(lines) > 50
