"""dagcon_set_hap_consensus: the tally of the two-way split against tests/hap_twin.py, exactly, and the batch
dagcon_upload_haps derives on the device against a fresh context and the oracle on the groups' strings; the binding, the
state rules and pbdagcon --hap-consensus / --hap-sites."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import hap_twin as ht
import md_twin as mt
import paf_files as pf
import site_reads_twin as srt
import window_twin as wt
from util import batch_from_targets, oracle_batch, random_target
from test_site_reads import _planted, _chain, _piles, _code, _tes, _tlens, _cli, GAP, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, NONCONFORMING = -8, -4
NAMES = ("dagcon_set_hap_consensus", "dagcon_fetch_hap_tally", "dagcon_upload_haps", "dagcon_fetch_hap_map")
KEYS = ("n1", "n2", "n0", "n_sep", "agree", "disagree", "split")


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def _six():
    bb = b"ACGTACGTACGT"
    ref = (1, bb, bb)
    alt = (1, b"ACG-ACGGTAAGT", b"ACGTACG-TACGT")                     # drops base 3, inserts behind base 6, another base at 9
    mix = (1, b"ACGTACGGTAAGT", b"ACGTACG-TACGT")                     # reads base 3 with the first, the rest with the second
    return ref, alt, mix


def test_the_tally_rule_by_hand(oracle_lib):
    """Six reads on ACGTACGTACGT, three sites.  The mixed read goes with the second group two sites to one, so it is the
    one entry that disagrees; with the alt reads first the seed is one of them and every phase is -1."""
    ref, alt, mix = _six()
    alns = [ref, ref, ref, alt, alt, mix]
    tw = srt.target(12, alns, 4, 0, (2, 200000))
    assert tw["sites"] == [3, 6, 9] and tw["hap"] == [1, 1, 1, 2, 2, 2] and tw["phase"] == [1, 1, 1]
    assert ht.held(alns, 4) == 6
    t = ht.tally(tw, 6, 0, 0, 3)
    # site 3: hap 1 reads T three times (P1), hap 2 drops it twice (M2) and reads it once (P2: the mixed read)
    assert t["site_counts"] == [[3, 0, 1, 2], [3, 0, 0, 3], [3, 0, 0, 3]]
    assert [t[k] for k in KEYS] == [3, 3, 0, 3, 5 + 6 + 6, 1, 1]
    # the other order: phase -1 at every site, so agree_k is M1 + P2
    swapped = [alt, alt, ref, ref, ref, mix]
    tw2 = srt.target(12, swapped, 4, 0, (2, 200000))
    assert tw2["hap"] == [1, 1, 2, 2, 2, 1] and tw2["phase"] == [-1, -1, -1]
    t2 = ht.tally(tw2, 6, 0, 0, 3)
    assert t2["site_counts"] == [[1, 2, 3, 0], [0, 3, 3, 0], [0, 3, 3, 0]]
    assert [t2[k] for k in KEYS] == [3, 3, 0, 3, 17, 1, 1]
    # the thresholds: the defaults are 2 sites and 3 reads; either group is K - n of the other = 3 reads deep
    assert ht.tally(tw, 6, 3, 3, 3)["split"] == 1 and ht.tally(tw, 6, 4, 0, 3)["split"] == 0
    assert ht.tally(tw, 6, 0, 4, 3)["split"] == 0 and ht.tally(tw, 6, 0, 0, 4)["split"] == 0
    assert ht.tally(tw, 6, 0, 0, 0)["split"] == 1                     # max(1, min_cov)
    failed = ht.tally(tw, 6, 0, 0, 3, ok=False)
    assert [failed[k] for k in KEYS] == [0] * 7 and failed["site_counts"] == []
    # a site is separating only when each label shows its own allele: take the second group's reads of site 6 away
    one = dict(tw, ents=[[e for e in x if e[0] != 1] if h == 2 else x for x, h in zip(tw["ents"], tw["hap"])])
    t3 = ht.tally(one, 6, 0, 0, 3)
    assert t3["site_counts"][1] == [3, 0, 0, 0] and t3["n_sep"] == 2 and t3["agree"] == 5 + 3 + 6
    # the groups: an unlabelled read and a read that is not taken are in both, a read below min_len in neither
    tie = (1, b"ACGTACGGTACGT", b"ACGTACG-TACGT")                     # one site each way: unassigned
    alt0 = (1, b"ACG-ACGGTACGT", b"ACGTACG-TACGT")                    # (without the change at base 9: two sites)
    alns4 = [ref, ref, (1, b"ACG", b"ACG"), alt0, alt0, tie]
    tw4 = srt.target(12, alns4, 4, 0, (2, 200000))
    assert tw4["src"] == [0, 1, 3, 4, 5] and tw4["hap"] == [1, 1, 2, 2, 0]
    assert ht.groups(alns4, 4, tw4["src"], tw4["hap"]) == ([0, 1, 5], [3, 4, 5])
    assert ht.groups(alns4, 4, tw4["src"][:-1], tw4["hap"][:-1]) == ([0, 1, 5], [3, 4, 5])      # (not taken: the same place)


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    tes = _tes()
    rng = np.random.default_rng(83)
    n_split = n_dis = n_sep = 0
    for k in range(400):
        alns, bb = tes._small_pileup(rng, k)
        trim = int(rng.integers(0, 3))
        opts = (0, 0) if k % 2 else (2, 200000)
        tw = srt.target(len(bb), alns, 4, trim, opts)
        sc = [tw["counts"][p] for p in tw["sites"]]
        t = ht.tally(tw, ht.held(alns, 4), 1 + k % 3, 1 + k % 2, 3)
        signed = [0] * len(sc)
        for e in tw["ents"]:
            for s, code in e:
                signed[s] += srt.sign(code, sc[s]) != 0
        assert all(sum(c) <= n for c, n in zip(t["site_counts"], signed))
        assert t["agree"] + t["disagree"] == sum(sum(c) for c, sg in zip(t["site_counts"], tw["phase"]) if sg)
        assert t["n1"] + t["n2"] + t["n0"] == len(tw["src"]) and t["n_sep"] <= sum(1 for sg in tw["phase"] if sg)
        g1, g2 = ht.groups(alns, 4, tw["src"], tw["hap"])
        assert len(g1) == ht.held(alns, 4) - t["n2"] and len(g2) == ht.held(alns, 4) - t["n1"]
        n_split += t["split"]; n_dis += t["disagree"]; n_sep += t["n_sep"]
    print("split %d, disagreeing entries %d, separating sites %d" % (n_split, n_dis, n_sep))
    assert n_split > 20 and n_dis > 100 and n_sep > 200


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(dagcon_hap_opts), '
            'sizeof(dagcon_hap_tally), sizeof(dagcon_hap_map)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert [ctypes.sizeof(x) for x in (capi.HapOpts, capi.HapTally, capi.HapMap)] == [int(x) for x in out]
    for m in ("set_hap_consensus", "hap_tally", "upload_haps", "hap_map"):
        assert callable(getattr(capi.Context, m))
    assert lib.dagcon_abi_version() == 2


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    fc, fs = tmp_path / "o.fa", tmp_path / "o.sites"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for flag, f in (("--hap-consensus", fc), ("--hap-sites", fs)):
        for args in ([str(m5), flag],
                     rec + ["--window", "200", "--overlap", "120", flag, str(f), str(sam)],
                     ["-a", flag, str(f), str(m5)], ["-a", "--polish", "1", flag, str(f), str(m5)],
                     rec + ["--dump-parsed", flag, str(f), str(sam)],
                     [flag, str(f), "--hap-min-sites", "x", str(m5)], [flag, str(f), "--hap-min-reads", str(m5)],
                     [flag, str(f), "--site-min-frac", "1.5", str(m5)]):
            out = run(*args)
            assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
            assert not f.exists()
        # a file that cannot be written is said before anything runs
        out = run(*rec, flag, str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr, flag
    # the thresholds of the sites go with either flag, without --sites; the split's own need one of the two
    out = run("--hap-sites", str(tmp_path / "no_such_dir" / "o.txt"), "--site-min-frac", "0.3", "--site-min-count", "3", "--hap-min-sites", "3",
              "--hap-min-reads", "4", str(m5))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    out = run("--hap-min-sites", "3", str(m5))
    assert out.returncode == 2 and b"PARSE ERROR" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --fastq")[1].split(b"\n  -v, --verbose")[0]
    assert b"\n  --hap-consensus FILE" in text and b">RNAME/hap1/r0_r1" in text and b"\n  --hap-sites FILE" in text
    assert b"#target RNAME N1 N2 N0 SEP AGREE DISAGREE SPLIT" in text and b"RNAME POS PHASE P1 M1 P2 M2" in text
    assert text.count(b"parity unpinned") == 2
    usage = h.stdout.split(b"\n")[0]
    assert b"[--site-reads FILE] [--haplotag FILE] [--hap-consensus FILE [--hap-min-sites N] [--hap-min-reads N]] [--hap-sites FILE] [--fastq]" in usage


_HAP_MAIN = r"""
#include <iostream>
#include "hap.h"
// stdin: "t rname n1 n2 n0 sep agree disagree split" | "s rname pos0 phase p1 m1 p2 m2" | "i rname label" per line
int main() {
    std::string out, kind, rname;
    while (std::cin >> kind >> rname) {
        if (kind == "t") { unsigned v[7]; for (auto &x : v) std::cin >> x; dg_hap_target_line(out, rname, v[0], v[1], v[2], v[3], v[4], v[5], v[6]); }
        else if (kind == "s") { unsigned long long pos; int phase; unsigned v[4]; uint16_t c[4]; std::cin >> pos >> phase;
                                for (int k = 0; k < 4; k++) { std::cin >> v[k]; c[k] = (uint16_t)v[k]; } dg_hap_site_line(out, rname, pos, phase, c); }
        else { unsigned label; std::cin >> label; out += dg_hap_id(rname, label); out += '\n'; }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatters_against_python(tmp_path):
    src = tmp_path / "hap_main.cpp"; src.write_text(_HAP_MAIN)
    exe = tmp_path / "hap_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    tgts = [("ctg", (3, 3, 0, 3, 17, 1, 1)), ("a/b|c", (4094, 4094, 4094, 262138, 4294967295, 4294967295, 0)), ("x", (0,) * 7)]
    sites = [("ctg", 0, 1, (3, 0, 1, 2)), ("a/b|c", 4294967295, -1, (4094, 4094, 65535, 0)), ("x", 41, -1, (0, 0, 0, 0))]
    ids = [("ctg", 1), ("m/1/0_9", 2)]
    text = "".join("t %s %s\n" % (n, " ".join(map(str, v))) for n, v in tgts)
    text += "".join("s %s %d %d %s\n" % (n, p, ph, " ".join(map(str, c))) for n, p, ph, c in sites)
    text += "".join("i %s %d\n" % x for x in ids)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    want = [ht.target_line(n, dict(zip(KEYS, v))) for n, v in tgts] + [ht.site_line(*x) for x in sites]
    want += [ht.fasta_name(n, g, 5, 9)[1:].rsplit("/", 1)[0] for n, g in ids]
    assert out == want
    assert out[0] == "#target\tctg\t3\t3\t0\t3\t17\t1\t1" and out[3] == "ctg\t1\t1\t3\t0\t1\t2" and out[4] == "a/b|c\t4294967296\t-1\t4094\t4094\t65535\t0"
    assert out[6] == "ctg/hap1" and out[7] == "m/1/0_9/hap2" and ht.fasta_name("ctg", 1, 5, 9) == ">ctg/hap1/5_9"


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _expect_tally(strings, tlens, min_cov, min_len, trim, opts, rounds, hap, status):
    """What the twin expects of hap_tally(): per target the seven numbers, the sites' counts of the targets that have any."""
    out = {k: [] for k in KEYS}
    out["site_counts"] = []
    for t, (s, tl) in enumerate(zip(strings, tlens)):
        n_al = 0 if s is None else len(s[1])
        if s is not None and not status[t] and n_al >= max(1, min_cov):
            tw = srt.target(tl, s[1], min_len, trim, opts, rounds or srt.ROUNDS)
            x = ht.tally(tw, ht.held(s[1], min_len), hap[0], hap[1], min_cov)
        else:
            x = dict(zip(KEYS, [0] * 7), site_counts=[])
        for k in KEYS:
            out[k].append(x[k])
        out["site_counts"] += x["site_counts"]
    return out


def _expect_map(strings, min_len, sr, split, n_given=None, src=None):
    """The derived batch, from the device's own labels: per group (target, label, indices into the target's strings)."""
    label = {(int(t), int(s)): int(h) for t, s, h in zip(sr["aln_tgt"], sr["aln_src"], sr["hap"])}
    out = {"src_target": [], "label": [], "aln_begin": [0], "aln_src": []}
    groups, base = [], 0
    for t, s in enumerate(strings):
        n_al = 0 if s is None else len(s[1])
        name = (lambda i, t=t, base=base: src[t][i] if src is not None else base + i)
        if split[t]:
            for g in (1, 2):
                idx = [i for i, (_, q, _) in enumerate(s[1]) if len(q) >= min_len and label.get((t, name(i)), 0) in (0, g)]
                out["src_target"].append(t); out["label"].append(g)
                out["aln_src"] += [name(i) for i in idx]; out["aln_begin"].append(len(out["aln_src"]))
                groups.append((t, g, idx))
        base += n_given[t] if n_given is not None else n_al
    return out, groups


def _hap_run(call, strings, tlens, min_cov, min_len, trim, opts=(2, 200000), hap=(0, 0), rounds=0, prepare=None, flags=0, n_given=None, src=None,
             backbones=None):
    """One context with the three switches on: the first batch by `call`, its tally against the twin, then the derived
    batch: its map against lists built from the device's labels, its results against a fresh context and the oracle on
    the groups' strings.  Returns what the tests look at further."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=flags)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*opts)
        c.set_site_reads(True, rounds)
        c.set_hap_consensus(*hap)
        first = call(c)
        sr, ps, status, reruns = c.site_reads(), c.pileup_sites(), c.target_status.tolist(), c.timings()["reruns"]
        tally = c.hap_tally()
        again = c.hap_tally()
        assert all(np.array_equal(tally[k], again[k]) for k in tally)
        exp = _expect_tally(strings, tlens, min_cov, min_len, trim, opts, rounds, hap, status)
        for k in KEYS:
            assert tally[k].tolist() == exp[k], (k, tally[k].tolist(), exp[k])
        assert tally["site_counts"].tolist() == exp["site_counts"] and tally["site_counts"].shape[0] == ps["pos"].size
        emap, groups = _expect_map(strings, min_len, sr, tally["split"], n_given, src)
        c.upload_haps()
        hm = c.hap_map()
        for k in emap:
            assert hm[k].tolist() == emap[k], k
        c.run(); c.sync()
        got = c.fetch()
        assert c.target_status.tolist() == [0] * len(groups) and len(got) == len(groups)
        extra = {}
        if flags & capi.FLAG_BASE_SUPPORT:
            extra["support"] = c.base_support()
        if flags & capi.FLAG_BASE_POS:
            extra["positions"] = c.base_positions()
        # the derived batch has no optional output, and is not a batch to derive from
        for f in (c.site_reads, c.pileup, c.pileup_sites, c.hap_tally, c.upload_haps):
            assert _code(f) == STATE
        assert all(np.array_equal(c.hap_map()[k], hm[k]) for k in hm)
    finally:
        c.close()
    if groups:
        gb = batch_from_targets([(tlens[t], [strings[t][1][i] for i in idx], backbones[t] if backbones else None) for t, g, idx in groups],
                                with_backbone=backbones is not None)
        fresh = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=flags)
        try:
            want = fresh.consensus(gb)
            if "support" in extra:
                ws = fresh.base_support()
                assert all(np.array_equal(a, b) for x, y in zip(extra["support"], ws) for p, q in zip(x, y) for a, b in zip(p, q))
                assert [len(x) for x in extra["support"]] == [len(x) for x in ws]
            if "positions" in extra:
                wp = fresh.base_positions()
                assert all(np.array_equal(a, b) for x, y in zip(extra["positions"], wp) for a, b in zip(x, y))
                assert [len(x) for x in extra["positions"]] == [len(x) for x in wp]
        finally:
            fresh.close()
        assert got == want                                             # segment for segment: range0, range1, bytes
        assert got == oracle_batch(gb, min_cov, min_len, trim)
    else:
        assert got == []
    return {"first": first, "sr": sr, "ps": ps, "status": status, "reruns": reruns, "tally": tally, "map": hm, "groups": groups, "got": got}


def _strings_call(strings, tlens, backbones=None):
    batch = batch_from_targets([(tl, alns, backbones[t] if backbones else None) for t, (tl, (_, alns)) in enumerate(zip(tlens, strings))],
                               with_backbone=backbones is not None)
    return lambda c: c.consensus(batch, strict=False)


@pytest.mark.gpu
def test_the_planted_case(oracle_lib):
    bb, alns, subs, ins_at, n_err = _planted()
    tw = srt.target(600, alns, 500, 50, (2, 200000))
    assert tw["hap"] == [1] * 12 + [2] * 12
    t = ht.tally(tw, 24, 0, 0, 6)
    inside = [p for p in subs if 50 <= p < 550]
    # on the twin first: every planted substitution inside the trim is a separating site, and the target is split
    for p in inside:
        p1, m1, p2, m2 = t["site_counts"][tw["sites"].index(p)]
        sg = tw["phase"][tw["sites"].index(p)]
        assert sg and (p1 >= 1 and m2 >= 1 if sg > 0 else m1 >= 1 and p2 >= 1), p
    assert t["split"] == 1 and t["n_sep"] >= len(inside) + 1 and t["n1"] == t["n2"] == 12
    r = _hap_run(_strings_call([(bb, alns)], [600]), [(bb, alns)], [600], 6, 500, 50)
    assert r["tally"]["split"].tolist() == [1] and r["map"]["label"].tolist() == [1, 2]
    assert r["map"]["aln_src"].tolist() == list(range(24))
    # the groups' sequences differ at the planted positions, and each is its haplotype there (the target is the first)
    (s1,), (s2,) = r["got"]

    def major(col):
        return int(np.bincount([q[col] for _, q, _ in alns[12:]]).argmax())
    h1 = bytes(bb)
    h2 = bytearray(bb)
    for p in subs:
        h2[p] = major(p if p < ins_at else p + 1)
        assert h2[p] != bb[p]
    h2 = bytes(h2[:ins_at]) + bytes([major(ins_at)]) + bytes(h2[ins_at:])
    # each group's consensus is a stretch of its own haplotype that covers every planted position inside the trim
    o1, o2 = h1.find(s1[2]), h2.find(s2[2])
    assert o1 >= 0 and o2 >= 0 and s2[2] not in h1 and s1[2] not in h2
    assert o1 <= inside[0] and o1 + len(s1[2]) > inside[-1] and o2 <= inside[0] and o2 + len(s2[2]) > inside[-1] + 1
    assert all(s1[2][p - o1] == bb[p] and s2[2][(p if p < ins_at else p + 1) - o2] == h2[p if p < ins_at else p + 1] != bb[p] for p in inside)


@pytest.mark.gpu
def test_depth_and_strides(oracle_lib):
    """Depth 70 (both halves of a counter word above zero), W and W + 1 sites (the wave's stride over an alignment's
    entries), 256 and 257 (the block's stride over a target's sites), and a target with one site, which is not split."""
    strings = [_piles(3, 40, depth=70), _piles(W, 100), _piles(W + 1, 100), _piles(256, 300), _piles(257, 300), _piles(1, 40)]
    tlens = [len(bb) for bb, _ in strings]
    tw = srt.target(40, strings[0][1], 30, 0, (2, 200000))
    assert ht.tally(tw, 70, 2, 0, 3)["site_counts"] == [[35, 0, 0, 35]] * 3            # P1 and M2: the low half of one word, the high half of the other
    mixed = [x for x in ht.site_counts(tw["ents"], [tw["counts"][p] for p in tw["sites"]], [1, 2] * 35) if x != [18, 17, 17, 18]]
    assert mixed == []                                                                # (labels that cut across: both halves of both words)
    r = _hap_run(_strings_call(strings, tlens), strings, tlens, 3, 30, 0, hap=(2, 0))
    assert r["status"] == [0] * 6 and r["tally"]["split"].tolist() == [1, 1, 1, 1, 1, 0]
    assert r["tally"]["n_sep"].tolist() == [3, W, W + 1, 256, 257, 1]
    assert r["tally"]["agree"].tolist() == [210, 6 * W, 6 * (W + 1), 6 * 256, 6 * 257, 6] and not r["tally"]["disagree"].any()
    assert r["map"]["src_target"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.gpu
def test_thresholds_and_an_empty_derived_batch(oracle_lib):
    strings = [_piles(5, 40), _piles(0, 40), _piles(2, 40)]
    for hap, want in (((3, 0), [1, 0, 0]), ((0, 4), [0, 0, 0])):
        exp = [ht.tally(srt.target(40, a, 30, 0, (2, 200000)), 6, hap[0], hap[1], 3)["split"] for _, a in strings]
        assert exp == want
        r = _hap_run(_strings_call(strings, [40] * 3), strings, [40] * 3, 3, 30, 0, hap=hap)
        assert r["tally"]["split"].tolist() == want and r["tally"]["n_sep"].tolist() == [5, 0, 2]
        assert r["map"]["src_target"].size == 2 * sum(want) and len(r["got"]) == 2 * sum(want)


@pytest.mark.gpu
def test_unlabelled_reads_are_in_both_groups(oracle_lib):
    bb, alns = _chain()
    tw = srt.target(260, alns, 30, 0, (1, 200000), 3)
    assert [bool(h) for h in tw["hap"]] == [True] * 5 + [False] * 7
    t = ht.tally(tw, 12, 2, 2, 1)
    assert (t["n1"], t["n2"], t["n0"], t["split"]) == (2, 3, 7, 1) and t["n_sep"] >= 2
    r = _hap_run(_strings_call([(bb, alns)], [260]), [(bb, alns)], [260], 1, 30, 0, opts=(1, 200000), hap=(2, 2), rounds=3)
    assert r["tally"]["split"].tolist() == [1]
    b = r["map"]["aln_begin"].tolist()
    g1, g2 = r["map"]["aln_src"][b[0]:b[1]].tolist(), r["map"]["aln_src"][b[1]:b[2]].tolist()
    assert set(g1) & set(g2) == set(range(5, 12)) and len(g1) == 12 - 3 and len(g2) == 12 - 2


@pytest.mark.gpu
def test_random_small_targets_with_a_failed_one(oracle_lib):
    tes = _tes()
    rng = np.random.default_rng(300)
    targets = []
    for k in range(150):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns, eqx=True)))
    bad = 75
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = tes._strings(targets)
    assert strings[bad] is None
    twins = [ht.tally(srt.target(len(s[0]), s[1], 4, 0, (2, 200000)), ht.held(s[1], 4), 1, 1, 3) for s in strings if s is not None and len(s[1]) >= 3]
    assert sum(t["split"] for t in twins) > 20 and sum(t["disagree"] for t in twins) > 50      # on the twin first
    r = _hap_run(tes._whole(targets), strings, _tlens(targets), 3, 4, 0, hap=(1, 1), n_given=[len(x) for _, x in targets])
    assert r["status"][bad] == NONCONFORMING and sum(1 for s in r["status"] if s) == 1
    assert [int(r["tally"][k][bad]) for k in KEYS] == [0] * 7
    assert int(r["ps"]["site_begin"][bad]) == int(r["ps"]["site_begin"][bad + 1])       # its sites are not in site_counts either
    assert bad not in r["map"]["src_target"].tolist() and r["tally"]["split"].sum() > 20 and r["tally"]["disagree"].sum() > 50


@pytest.mark.gpu
def test_arena_growth_counts_nothing_twice(oracle_lib):
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    alns, bb = random_target(rng, 400, 40, full_span=True, sub=0.02, ins=0.03, dele=0.03)
    assert sum(len(q) for _, q, _ in alns) // 64 + 4096 < 40 * 380
    r = _hap_run(_strings_call([(bb, alns)], [400]), [(bb, alns)], [400], 3, 30, 5, opts=(0, 0))
    off = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        off.set_pileup(0, 0)
        off.consensus(batch_from_targets([(400, alns, None)]))
        reruns_off = off.timings()["reruns"]
    finally:
        off.close()
    assert r["reruns"] > reruns_off and r["tally"]["agree"][0] + r["tally"]["disagree"][0] > 1000


@pytest.mark.gpu
def test_poisoned_buffers(oracle_lib, monkeypatch):
    monkeypatch.setenv("DAGCON_POISON", "15")
    strings = [_piles(5, 40), _piles(0, 40), _piles(W + 1, 100), (b"N" * 50, _piles(3, 50)[1][:2])]      # (the last: below min_cov)
    tlens = [40, 40, 100, 50]
    r = _hap_run(_strings_call(strings, tlens), strings, tlens, 3, 30, 0)
    assert r["tally"]["split"].tolist() == [1, 0, 1, 0] and r["tally"]["n_sep"].tolist() == [5, 0, W + 1, 0]


def _ways_in():
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(91, 12, 150, 400, full_span=True)
    strings = tes._strings(targets)
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
    return targets, strings, calls


@pytest.mark.gpu
def test_every_way_in_gives_the_same_groups(oracle_lib):
    targets, strings, calls = _ways_in()
    tlens = _tlens(targets)
    exp = [ht.tally(srt.target(tl, a, 30, 5, (2, 200000)), ht.held(a, 30), 0, 0, 3)["split"] for tl, (_, a) in zip(tlens, strings)]
    assert sum(exp) >= 2                                               # on the twin first: there is something to derive
    ref = None
    for kind, call in calls.items():
        r = _hap_run(call, strings, tlens, 3, 30, 5)
        assert r["status"] == [0] * 12 and r["tally"]["split"].tolist() == exp, kind
        if ref is None:
            ref = r
        assert r["got"] == ref["got"] and all(np.array_equal(r["map"][k], ref["map"][k]) for k in ref["map"]), kind


@pytest.mark.gpu
def test_consensus_pre_on_the_aligner_s_strings(oracle_lib):
    from pbdagcon_amd import capi
    rng = np.random.default_rng(7)
    targets, pairs, starts = [], [], []
    for ti in range(2):
        tlen = int(rng.integers(300, 400))
        target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
        other = bytearray(target)
        for p in range(40, tlen - 40, 45):
            other[p] = next(b for b in b"ACGT" if b != target[p])
        recs = []
        for r in range(10):
            s = int(rng.integers(0, 20)); e = int(rng.integers(tlen - 20, tlen + 1))
            src = (target, bytes(other))[r % 2][s:e]
            qseq = bytearray()
            for ch in src:
                u = rng.random()
                if u < 0.01:
                    continue
                qseq.append(ch)
                if rng.random() < 0.01:
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
    tlens = [t for t, _ in targets]
    exp = [ht.tally(srt.target(tl, a, 100, 10, (2, 200000)), ht.held(a, 100), 0, 0, 3)["split"] for tl, (_, a) in zip(tlens, strings)]
    assert exp == [1, 1]
    r = _hap_run(lambda c: c.consensus_pre(targets), strings, tlens, 3, 100, 10)
    assert r["tally"]["split"].tolist() == [1, 1] and r["map"]["aln_src"].max() == 19


@pytest.mark.gpu
def test_windows_each_window_is_a_target(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(77, 8, 120, 120)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 40, 10)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    strings = [(targets[g][0][a:b], alns) for (g, a, b), (_, alns, _) in zip(wins, per)]
    first = np.concatenate([[0], np.cumsum([len(r) for _, r in targets])]).tolist()
    src = []
    for g, a, b in wins:
        bb, recs = targets[g]
        src.append([first[g] + k for k, (p, q, o) in enumerate(recs) if max(a, wt.span(p, len(bb), o)[0]) < min(b, wt.span(p, len(bb), o)[1])])
    tlens = [b - a for _, a, b in wins]
    exp = [ht.tally(srt.target(tl, a, 30, 5, (2, 200000)), ht.held(a, 30), 1, 1, 3)["split"] for tl, (_, a) in zip(tlens, strings)]
    assert sum(exp) >= 2
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    r = _hap_run(lambda c: c.consensus_cigar_windows(cb, hw), strings, tlens, 3, 30, 5, hap=(1, 1), src=src)
    assert r["tally"]["split"].tolist() == exp


@pytest.mark.gpu
def test_under_the_record_filter_aln_src_is_the_caller_s_record(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(13, 10, 150, 300)
    depth = 7
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
    strings = tes._strings(kept)
    tlens = _tlens(targets)
    exp = [ht.tally(srt.target(tl, a, 30, 5, (2, 200000)), ht.held(a, 30), 1, 2, 3)["split"] for tl, (_, a) in zip(tlens, strings)]
    assert sum(exp) >= 1
    r = _hap_run(tes._whole(targets), strings, tlens, 3, 30, 5, hap=(1, 2), prepare=lambda c: c.set_record_filter(max_depth=depth), src=src)
    assert r["tally"]["split"].tolist() == exp
    assert not set(r["map"]["aln_src"].tolist()) & set(np.flatnonzero(fate).tolist())


@pytest.mark.gpu
def test_a_real_backbone_and_the_per_base_outputs(oracle_lib):
    from pbdagcon_amd import capi
    bb, alns, subs, ins_at, n_err = _planted(seed=4)
    strings = [(bb, alns), _piles(3, 40, depth=12)]
    assert [ht.tally(srt.target(tl, a, 30, 0, (2, 200000)), ht.held(a, 30), 0, 0, 6)["split"] for tl, (_, a) in zip([600, 40], strings)] == [1, 1]
    # a backbone that is not the reads' target string: where no read covers, the backbone's own bases would show
    backbones = [bytes(bb), b"T" * 40]
    r = _hap_run(_strings_call(strings, [600, 40], backbones), strings, [600, 40], 6, 30, 0, backbones=backbones,
                 flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    assert r["tally"]["split"].tolist() == [1, 1] and len(r["got"]) == 4


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        for f in (c.hap_tally, c.upload_haps, c.hap_map):
            assert _code(f) == STATE                                 # nothing yet
        c.set_pileup(2, 200000); c.set_site_reads(True)
        want = c.consensus_cigar(cb)                                 # the switch off: a context that never heard of it
        assert _code(c.hap_tally) == STATE and _code(c.upload_haps) == STATE
        c.set_hap_consensus(1, 1)                                    # set after the upload
        assert _code(c.hap_tally) == STATE and _code(c.upload_haps) == STATE
        c.set_site_reads(False)                                      # the split off at the upload
        assert c.consensus_cigar(cb) == want
        assert _code(c.hap_tally) == STATE and _code(c.upload_haps) == STATE and c.site_reads()["hap"] is None
        c.set_site_reads(None)                                       # the site reads off
        assert c.consensus_cigar(cb) == want and _code(c.hap_tally) == STATE
        c.set_site_reads(True)
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.hap_tally) == STATE and _code(c.upload_haps) == STATE    # before a fetch
        assert c.fetch() == want
        tally = c.hap_tally()
        assert tally["split"].any()
        c.upload_haps()
        assert _code(c.upload_haps) == STATE and _code(c.hap_tally) == STATE    # twice in a row
        assert _code(c.site_reads) == STATE and _code(c.pileup) == STATE and _code(c.pileup_sites) == STATE
        assert _code(c.fetch) == STATE                               # the results of the first batch are gone
        hm = c.hap_map()
        c.run(); c.sync()
        assert len(c.fetch()) == hm["label"].size == 2 * int(tally["split"].sum())
        assert _code(c.hap_tally) == STATE and _code(c.upload_haps) == STATE and _code(c.site_reads) == STATE
        assert c.consensus_cigar(cb) == want                         # the context goes on: the switches are as they were
        assert _code(c.hap_map) == STATE                             # after a later upload
        assert all(np.array_equal(c.hap_tally()[k], tally[k]) for k in tally)
        c.set_hap_consensus(None)
        assert c.consensus_cigar(cb) == want and _code(c.hap_tally) == STATE and c.site_reads()["hap"] is not None
    finally:
        c.close()
    stop = capi.Context(min_cov=3, min_len=30, trim=5, flags=capi.FLAG_STOP_AFTER_MERGE)
    try:
        stop.set_pileup(2, 200000); stop.set_site_reads(True); stop.set_hap_consensus()
        stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
        assert _code(stop.hap_tally) == STATE and _code(stop.upload_haps) == STATE
    finally:
        stop.close()


@pytest.mark.gpu
def test_the_switch_changes_nothing_else(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 6, 150, 250)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    out = []
    for on in (False, True):
        c = capi.Context(min_cov=3, min_len=30, trim=5)
        try:
            c.set_pileup(2, 200000); c.set_site_reads(True)
            if on:
                c.set_hap_consensus()
            out.append((c.consensus_cigar(cb), c.pileup(), c.pileup_sites(), c.site_reads()))
        finally:
            c.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_pbdagcon_hap_consensus_and_hap_sites(oracle_lib, tmp_path):
    from pbdagcon_amd import synth
    tes = _tes()
    targets = tes._variant_targets(101, 8, 150, 300, full_span=True)
    names = ["ctg%d" % i for i in range(8)]
    tl = _tlens(targets)
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [r for _, r in targets]))
    strings = tes._strings(targets)
    m5 = tmp_path / "in.m5"
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    sb.ids = names
    m5.write_bytes(synth.to_m5(sb))
    base = [_cli(), "-c", "3", "-m", "30", "-t", "5"]
    rec = ["--sam", "--ref", str(ref)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r

    def lines(opts, hap):
        fasta, sites, n_split = [], [], 0
        for g, (bb, alns) in enumerate(strings):
            tw = srt.target(tl[g], alns, 30, 5, opts)
            t = ht.tally(tw, ht.held(alns, 30), hap[0], hap[1], 3)
            sites.append(ht.target_line(names[g], t))
            sites += [ht.site_line(names[g], p, sg, c) for p, sg, c in zip(tw["sites"], tw["phase"], t["site_counts"]) if sg]
            if not t["split"]:
                continue
            n_split += 1
            for label, idx in zip((1, 2), ht.groups(alns, 30, tw["src"], tw["hap"])):
                (segs,) = oracle_batch(batch_from_targets([(tl[g], [alns[i] for i in idx], None)]), 3, 30, 5)
                for r0, r1, seq in segs:
                    fasta += [ht.fasta_name(names[g], label, r0, r1), seq.decode()]
        return fasta, sites, n_split
    fasta, sites, n_split = lines((2, 200000), (0, 0))
    assert n_split >= 1 and len(fasta) >= 4                            # on the twin first
    f = {k: tmp_path / k for k in ("c", "s", "c2", "s2", "s3", "h", "c3", "s4")}
    plain = run(*rec, str(sam))
    got = run(*rec, "--hap-consensus", str(f["c"]), "--hap-sites", str(f["s"]), str(sam))
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 8
    assert f["c"].read_text().splitlines() == fasta and f["s"].read_text().splitlines() == sites
    # the same with two batches and two parsing threads
    got = run(*rec, "--hap-consensus", str(f["c3"]), "--hap-sites", str(f["s4"]), "--batch-targets", "5", "-j", "2", str(sam))
    assert got.stdout == plain.stdout and f["c3"].read_bytes() == f["c"].read_bytes() and f["s4"].read_bytes() == f["s"].read_bytes()
    # the .m5 of the same alignments, other thresholds, two batches, two parsing threads
    fasta2, sites2, n2 = lines((3, 300000), (1, 2))
    assert n2 >= 1
    got = run("--hap-consensus", str(f["c2"]), "--hap-sites", str(f["s2"]), "--site-min-frac", "0.3", "--site-min-count", "3", "--hap-min-sites", "1",
              "--hap-min-reads", "2", "--batch-targets", "5", "-j", "2", str(m5))
    assert got.stdout == run(str(m5)).stdout
    assert f["c2"].read_text().splitlines() == fasta2 and f["s2"].read_text().splitlines() == sites2
    # one flag alone turns everything it needs on, and leaves --haplotag's file as it is without it
    run(*rec, "--hap-sites", str(f["s3"]), "--haplotag", str(f["h"]), str(sam))
    assert f["s3"].read_bytes() == f["s"].read_bytes()
    run(*rec, "--haplotag", str(tmp_path / "h0"), str(sam))
    assert f["h"].read_bytes() == (tmp_path / "h0").read_bytes()
