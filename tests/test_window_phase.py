"""Phase across windows (dagcon_set_window_phase, pbdagcon --window --phase-windows): the rule by hand, the binding, the
usage errors and the host's pair link and vote on the CPU; the device against the twin on the GPU.  include/dagcon.h
states the rule (9); window_phase_twin.py is it in Python."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import md_twin as mt
import paf_files as pf
import site_reads_twin as srt
import window_phase_twin as wpt
import window_twin as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -8, -1
GAP = 0x2D
OPTS = (2, 200000)                                               # the pile-up's thresholds of every run here


def _tsr():
    import test_site_reads as tsr
    return tsr


def _cli():
    return _tsr()._cli()


def _code(f):
    return _tsr()._code(f)


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def _pair(same, diff, zeros=0, **kw):
    """Two windows of one target that share same + diff + zeros records: the counts the twin finds, and whether it links."""
    n = same + diff + zeros
    tgt = [0] * n + [1] * n
    src = list(range(n)) * 2
    hap = [1] * n + [1] * same + [2] * diff + [0] * zeros
    s, d, block, flip, ohap, _ = wpt.link([0, 0], tgt, src, hap, [], [], **kw)
    assert (s, d) == ([0, same], [0, diff])
    return block[1] == 0, flip[1], ohap[n:]


def test_the_rule_by_hand():
    # hi at min_links - 1 and at min_links, the default 3 and one given
    assert not _pair(2, 0)[0] and _pair(3, 0)[0] and not _pair(0, 2)[0] and _pair(0, 3)[0]
    assert not _pair(4, 0, min_links=5)[0] and _pair(5, 0, min_links=5)[0] and _pair(1, 0, min_links=1)[0]
    # lo * 1000000 one below, equal to and one above max_conflict_ppm * (hi + lo): hi 3, lo 1 is 250000 ppm, the default
    assert _pair(3, 1)[0] and _pair(3, 1, max_conflict_ppm=250000)[0] and not _pair(3, 1, max_conflict_ppm=249999)[0]
    assert wpt.linked(7, 3, 1, 300000) and wpt.linked(7, 3, 1, 300001) and not wpt.linked(7, 3, 1, 299999)       # 3000000 against ppm * 10
    assert not wpt.linked(999999, 333334, 1, 250000) and wpt.linked(999999, 333333, 1, 250000)                   # one above, equal
    assert wpt.linked(3000000000, 1000000000, 1, 250000)                                                         # past 32 bits: no overflow
    # same == diff never links, whatever the thresholds
    for n in (1, 3, 50):
        assert not _pair(n, n, min_links=1, max_conflict_ppm=1000000)[0]
    assert not wpt.linked(0, 0, 1, 1000000)
    # the larger side decides the orientation; a label of 0 on either side does not count
    linked, flip, ohap = _pair(1, 4, zeros=3)
    assert linked and flip == 1 and ohap == [2] + [1] * 4 + [0] * 3
    n = 4
    s, d, block, flip, _, _ = wpt.link([0, 0], [0] * n + [1] * n, list(range(n)) * 2, [0, 1, 1, 1] + [1, 0, 1, 1], [], [])
    assert (s[1], d[1]) == (2, 0) and block == [0, 1]
    # flips xor along a chain of four: windows 1 and 3 name the labels the other way round
    recs = list(range(5))
    hap = [1, 1, 1, 2, 2] + [2, 2, 2, 1, 1] + [2, 2, 2, 1, 1] + [1, 1, 1, 2, 2]
    tgt = [w for w in range(4) for _ in recs]
    sites, phase = [0, 1, 1, 2, 3], [1, 1, -1, 0, -1]
    s, d, block, flip, ohap, ophase = wpt.link([7] * 4, tgt, recs * 4, hap, sites, phase)
    assert s == [0, 0, 5, 0] and d == [0, 5, 0, 5] and block == [0] * 4 and flip == [0, 1, 1, 0]
    assert ohap == [1, 1, 1, 2, 2] * 4 and ophase == [1, -1, 1, 0, -1]
    # a break restarts flip at 0 and block at w: window 2 shares two records only
    tgt2 = [0] * 5 + [1] * 5 + [2] * 2 + [3] * 2
    src2 = recs * 2 + [0, 1] * 2
    hap2 = [1, 1, 1, 2, 2] + [2, 2, 2, 1, 1] + [1, 1] + [2, 2]
    s, d, block, flip, ohap, _ = wpt.link([0] * 4, tgt2, src2, hap2, [], [])
    assert block == [0, 0, 2, 3] and flip == [0, 1, 0, 0] and ohap[10:] == hap2[10:] and (s[3], d[3]) == (0, 2)
    # a change of target breaks, even when both windows hold record number 0 (and 1, 2)
    s, d, block, flip, _, _ = wpt.link([0, 1], [0] * 3 + [1] * 3, [0, 1, 2] * 2, [1] * 6, [], [])
    assert s == [0, 0] and d == [0, 0] and block == [0, 1]
    s, d, block, flip, _, _ = wpt.link([1, 1], [0] * 3 + [1] * 3, [0, 1, 2] * 2, [1] * 6, [], [])
    assert s == [0, 3] and block == [0, 0]
    # nothing depends on an order
    perm = np.random.default_rng(1).permutation(20)
    got = wpt.link([7] * 4, [tgt[i] for i in perm], [(recs * 4)[i] for i in perm], [hap[i] for i in perm], sites[::-1], phase[::-1])
    assert got[:4] == ([0, 0, 5, 0], [0, 5, 0, 5], [0] * 4, [0, 1, 1, 0]) and got[5] == ophase[::-1]
    assert sorted(zip([tgt[i] for i in perm], [(recs * 4)[i] for i in perm], got[4])) == sorted(zip(tgt, recs * 4, [1, 1, 1, 2, 2] * 4))
    # the vote: the block with the most labelled pieces, ties to the lower block; V decides, 0 on a tie
    assert wpt.vote([(4, 1), (4, 1), (9, 2)]) == (1, 4) and wpt.vote([(4, 1), (9, 2)]) == (1, 4) and wpt.vote([(9, 2), (4, 1), (9, 0)]) == (1, 4)
    assert wpt.vote([(4, 1), (4, 2), (9, 2)]) == (0, 4) and wpt.vote([(4, 0), (9, 0)]) == (0, None) and wpt.vote([(4, 0), (9, 2)]) == (2, 9)
    assert wpt.haplotag_line("c", "q", 2, 7, 151) == "c\tq\t2\t7\t151" and wpt.haplotag_line("c", "q", 0, 0, None) == "c\tq\t0\t0\t."


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in ("dagcon_set_window_phase", "dagcon_fetch_window_phase"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %zu\\n", sizeof(dagcon_window_phase_opts), '
            'sizeof(dagcon_window_phase)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert [ctypes.sizeof(x) for x in (capi.WindowPhaseOpts, capi.WindowPhase)] == [int(x) for x in out]
    for m in ("set_window_phase", "window_phase"):
        assert callable(getattr(capi.Context, m))
    assert lib.dagcon_abi_version() == 2


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    sr, ht = tmp_path / "o.reads", tmp_path / "o.tags"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    win = rec + ["--window", "200", "--overlap", "120"]
    for args in (rec + ["--phase-windows", "--haplotag", str(ht), str(sam)],                          # without --window
                 win + ["--phase-windows", str(sam)],                                                 # with neither file
                 win + ["--phase-min-links", "2", str(sam)], win + ["--phase-max-conflict", "0.1", str(sam)],
                 win + ["--phase-min-links", "2", "--haplotag", str(ht), str(sam)],                   # (and the combination stays refused without the flag)
                 win + ["--phase-windows", "--phase-max-conflict", "1.000001", "--haplotag", str(ht), str(sam)],
                 win + ["--phase-windows", "--phase-max-conflict", "0.1234567", "--site-reads", str(sr), str(sam)],
                 win + ["--site-reads", str(sr), str(sam)], win + ["--haplotag", str(ht), str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not sr.exists() and not ht.exists()
    for flag in ("--hap-consensus", "--hap-sites", "--site-alleles", "--site-vcf", "--vcf"):          # out of scope: still refused
        out = run(*win, "--phase-windows", "--haplotag", str(ht), flag, str(tmp_path / "o.x"), str(sam))
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, flag
    # the combination is legal with the flag: the files are opened before anything runs
    out = run(*win, "--phase-windows", "--phase-max-conflict", "1", "--haplotag", str(tmp_path / "no_such_dir" / "o.txt"), str(sam))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --overlap O")[1].split(b"\n  --max-error F")[0]
    assert b"\n  --phase-windows " in text and b"--phase-min-links N" in text and b"--phase-max-conflict F" in text
    assert b"RNAME QNAME HAP SITES PS" in text and text.count(b"parity unpinned") == 1


_WP_MAIN = r"""
#include <iostream>
#include "window_phase.h"
// stdin, one case a line: "p ml ppm has_prev prev_flip prev_block w n_prev (rec hap)* n_cur (rec hap)*" -> "same diff flip block"
//                         "v n (block hap)*" -> "hap labelled block"
//                         "h rname qname hap sites labelled ps" -> the line
int main() {
    std::string out, kind;
    while (std::cin >> kind) {
        if (kind == "p") {
            unsigned ml, ppm, has_prev, pf; unsigned long long pb, w; size_t n;
            std::cin >> ml >> ppm >> has_prev >> pf >> pb >> w;
            std::vector<DgWpPiece> a[2];
            for (int k = 0; k < 2; k++) { std::cin >> n; for (size_t i = 0; i < n; i++) { unsigned long long r; unsigned h; std::cin >> r >> h; a[k].push_back(DgWpPiece{r, (uint8_t)h}); } }
            uint32_t same = 0, diff = 0;
            if (has_prev) dg_wp_pair(a[0], a[1], same, diff);
            const DgWpLink l = dg_wp_step(has_prev != 0, DgWpLink{(uint8_t)pf, pb}, w, same, diff, ml, ppm);
            out += std::to_string(same) + " " + std::to_string(diff) + " " + std::to_string((unsigned)l.flip) + " " + std::to_string(l.block) + "\n";
        } else if (kind == "v") {
            size_t n; std::cin >> n;
            std::vector<DgWpVote> v;
            for (size_t i = 0; i < n; i++) { unsigned long long b; unsigned h; std::cin >> b >> h; v.push_back(DgWpVote{b, (uint8_t)h}); }
            unsigned hap = 0; uint64_t block = 0;
            const bool lab = dg_wp_vote(v, hap, block);
            out += std::to_string(hap) + " " + std::to_string((int)lab) + " " + std::to_string(block) + "\n";
        } else {
            std::string rname, qname; unsigned hap, lab; unsigned long long sites, ps;
            std::cin >> rname >> qname >> hap >> sites >> lab >> ps;
            dg_wp_haplotag_line(out, rname, qname, hap, sites, lab != 0, ps);
        }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_host_pair_link_and_vote_against_the_twin(tmp_path):
    src = tmp_path / "wp_main.cpp"; src.write_text(_WP_MAIN)
    exe = tmp_path / "wp_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    rng = np.random.default_rng(20)
    text, want = [], []
    for case in range(3000):
        # two windows that share some of up to 12 records; labels 0, 1, 2; thresholds around the counts
        pool = np.sort(rng.choice(40, size=int(rng.integers(0, 13)), replace=False))
        pieces = []
        for k in range(2):
            keep = pool[rng.random(pool.size) < 0.8]
            flipped = rng.random() < 0.5
            pieces.append([(int(r), int(rng.choice([0, 1, 2], p=[0.15, 0.6, 0.25]) if rng.random() < 0.3 else 1 + (int(r) % 2 ^ flipped))) for r in keep])
        ml, ppm = int(rng.integers(0, 6)), int(rng.choice([0, 1, 100000, 250000, 333333, 333334, 500000, 1000000]))
        has_prev, pf, pb, w = int(rng.random() < 0.85), int(rng.integers(0, 2)), int(rng.integers(0, 50)), int(rng.integers(50, 99))
        text.append("p %d %d %d %d %d %d %d %s %d %s" % (ml, ppm, has_prev, pf, pb, w, len(pieces[0]), " ".join("%d %d" % x for x in pieces[0]),
                                                         len(pieces[1]), " ".join("%d %d" % x for x in pieces[1])))
        # the twin, on two windows of one target (has_prev) or of two, in a scrambled order
        al = [(0, r, h) for r, h in pieces[0]] + [(1, r, h) for r, h in pieces[1]]
        al = [al[i] for i in rng.permutation(len(al))]
        s, d, block, flip, _, _ = wpt.link([0, 0 if has_prev else 1], [x[0] for x in al], [x[1] for x in al], [x[2] for x in al], [], [], ml, ppm)
        lk = block[1] == 0
        want.append("%d %d %d %d" % (s[1], d[1], pf ^ flip[1] if lk else 0, pb if lk else w))
    n_tied = n_two = 0
    for case in range(3000):
        # a record's pieces over up to three blocks: tied blocks and records with pieces in two blocks among them
        blocks = rng.choice([3, 17, 40], size=int(rng.integers(1, 4)), replace=False)
        v = [(int(rng.choice(blocks)), int(rng.choice([0, 1, 2], p=[0.2, 0.5, 0.3]))) for _ in range(int(rng.integers(0, 7)))]
        per = {}
        for b, h in v:
            if h:
                per[b] = per.get(b, 0) + 1
        n_two += len(per) >= 2
        n_tied += len(per) >= 2 and sorted(per.values())[-1] == sorted(per.values())[-2]
        text.append("v %d %s" % (len(v), " ".join("%d %d" % x for x in v)))
        hap, b = wpt.vote(v)
        want.append("%d %d %d" % (hap, b is not None, b or 0))
    assert n_tied > 200 and n_two > 1000
    tags = [("ctg", "q0_1", 0, 0, None), ("a/b|c", "m/1/0_9", 2, 123456789012, 4294967296), ("x", "r", 1, 7, 1)]
    text += ["h %s %s %d %d %d %d" % (r, q, h, n, ps is not None, ps or 0) for r, q, h, n, ps in tags]
    want += [wpt.haplotag_line(*x) for x in tags]
    out = subprocess.run([str(exe)], input=("\n".join(text) + "\n").encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert len(out) == len(want)
    bad = [(t, o, w) for t, o, w in zip(text, out, want) if o != w]
    assert not bad, bad[:3]
    linked = sum(1 for t, o in zip(text, out) if t[0] == "p" and int(o.split()[3]) < 50)
    assert 300 < linked < 2700 and out[-3] == "ctg\tq0_1\t0\t0\t."


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _device(call, min_cov, min_len, trim, wp=(0, 0), prepare=None):
    """One context with the pile-up, the split and the switch on: (site reads, sites, window phase, status)."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*OPTS)
        c.set_site_reads(True)
        c.set_window_phase(*wp)
        call(c)
        return c.site_reads(), c.pileup_sites(), c.window_phase(), c.target_status.tolist()
    finally:
        c.close()


def _twin(hw, sr, ps, wp=(0, 0)):
    """The twin on the device's own site reads."""
    site_tgt = np.repeat(np.arange(hw.n_windows), np.diff(ps["site_begin"].astype(np.int64)))
    return wpt.link(hw.target.tolist(), sr["aln_tgt"].tolist(), sr["aln_src"].tolist(), sr["hap"].tolist(), site_tgt.tolist(), sr["phase"].tolist(), *wp)


KEYS = ("same", "diff", "block", "flip", "hap", "phase")


def _equal(dev, tw, what=""):
    for k, t in zip(KEYS, tw):
        assert dev[k].tolist() == t, (what, k)


def _run(call, hw, min_cov, min_len, trim, wp=(0, 0), prepare=None):
    sr, ps, dev, status = _device(call, min_cov, min_len, trim, wp, prepare)
    tw = _twin(hw, sr, ps, wp)
    _equal(dev, tw)
    return sr, ps, dev, status, tw


def _cpu_chain(targets, hw, min_cov, min_len, trim, wp=(0, 0)):
    """The whole chain on the CPU: site_reads_twin.target per window, then the twin.  Returns (aln_tgt, aln_src, hap) and
    the twin's six arrays."""
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    first = np.concatenate([[0], np.cumsum([len(r) for _, r in targets])]).tolist()
    aln_tgt, aln_src, hap, site_tgt, phase = [], [], [], [], []
    for w, ((g, a, b), (tl, alns, failed)) in enumerate(zip(wins, wt.window_targets(targets, wins))):
        bb, recs = targets[g]
        src = [first[g] + k for k, (p, q, o) in enumerate(recs) if max(a, wt.span(p, len(bb), o)[0]) < min(b, wt.span(p, len(bb), o)[1])]
        if failed or len(alns) < max(1, min_cov):
            continue
        tw = srt.target(tl, alns, min_len, trim, OPTS)
        aln_tgt += [w] * len(tw["src"]); aln_src += [src[i] for i in tw["src"]]; hap += tw["hap"]
        site_tgt += [w] * len(tw["sites"]); phase += tw["phase"]
    return (aln_tgt, aln_src, hap), wpt.link(hw.target.tolist(), aln_tgt, aln_src, hap, site_tgt, phase, *wp)


N_FRONT = 3


def _planted_records(chimeras=0):
    """The planted target of test_site_reads as records, ordered so that the seeds of neighbouring windows come from
    different haplotypes: first N_FRONT reads of the first haplotype that cover only [0, 330), then the 12 of the second,
    then the other 9 of the first; then `chimeras` reads that are the first haplotype up to base 300 and the second behind
    it.  Returns (bb, records, the planted group of every record: 1, 2, or 0 for a chimera)."""
    bb, alns, subs, ins_at, n_err = _tsr()._planted()
    a_reads, b_reads = alns[:12], alns[12:]
    recs = [ct.compress(1, q[:330], t[:330], bb) for _, q, t in a_reads[:N_FRONT]]
    recs += [ct.compress(s, q, t, bb) for s, q, t in b_reads] + [ct.compress(s, q, t, bb) for s, q, t in a_reads[N_FRONT:]]
    groups = [1] * N_FRONT + [2] * 12 + [1] * (12 - N_FRONT)
    for k in range(chimeras):
        (_, qa, ta), (_, qb, tb) = a_reads[N_FRONT + k], b_reads[k]
        recs.append(ct.compress(1, qa[:300] + qb[300:], ta[:300] + tb[300:], bb))       # (column 300 is base 300 in both: the inserted base lies behind it)
        groups.append(0)
    return bb, recs, groups


def _n_blocks(block):
    return len(set(block))


@pytest.mark.gpu
def test_planted_haplotypes_with_forced_flips(oracle_lib):
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records()
    targets = [(bb, recs)]
    hw = capi.HostWindows.tiled([600], 150, 30)
    # on the twin first: both orientations occur, and the four windows are one block
    (c_tgt, c_src, c_hap), cpu = _cpu_chain(targets, hw, 6, 30, 5)
    assert hw.n_windows == 4 and set(cpu[3]) == {0, 1} and cpu[2] == [0] * 4
    assert {(w, h) for w, r, h in zip(c_tgt, c_src, c_hap) if groups[r] == 1} == {(0, 1), (1, 1), (2, 2), (3, 2)}   # each window's own names
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(cb, hw), hw, 6, 30, 5)
    assert status == [0] * 4
    assert (sr["aln_tgt"].tolist(), sr["aln_src"].tolist(), sr["hap"].tolist()) == (c_tgt, c_src, c_hap)
    _equal(dev, cpu, "the chain on the CPU")
    # after orientation every record has one label in all its windows, and the labels are the planted groups
    assert dev["hap"].tolist() == [groups[r] for r in sr["aln_src"].tolist()] and sr["aln_src"].size == 3 * 3 + 21 * 4


@pytest.mark.gpu
def test_both_sides_of_each_threshold(oracle_lib):
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records(chimeras=2)
    targets = [(bb, recs)]
    hw = capi.HostWindows.tiled([600], 150, 30)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    _, cpu = _cpu_chain(targets, hw, 6, 30, 5)
    same, diff = cpu[0], cpu[1]
    lo = [min(s, d) for s, d in zip(same, diff)]
    w = lo.index(2)                                              # the boundary the two chimeras cross: they disagree with the others
    hi = max(same[w], diff[w])
    assert lo.count(2) == 1 and hi >= 20 and cpu[2] == [0] * 4
    ppm = -(-2 * 1000000 // (hi + 2))
    # (min_links, max_conflict_ppm), whether the chimeras' boundary links, and the number of blocks where the rest is known to hold
    for wp, links, blocks in (((hi, 0), True, None), ((hi + 1, 0), False, None), ((1, ppm), True, 1), ((1, ppm - 1), False, 2)):
        sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(cb, hw), hw, 6, 30, 5, wp)
        assert dev["same"].tolist() == same and dev["diff"].tolist() == diff
        expect = [0] * 4
        for k in range(1, 4):
            expect[k] = expect[k - 1] if wpt.linked(same[k], diff[k], *wp) else k
        assert dev["block"].tolist() == expect and (expect[w] != w) == links, wp
        assert blocks is None or _n_blocks(expect) == blocks, wp


def _cut(aln, a, b):
    """The columns of a full-span alignment string from target base a up to, not including, target base b."""
    start, q, t = aln
    at = np.concatenate([[0], np.cumsum(np.frombuffer(t, np.uint8) != GAP)])      # target bases in front of each column
    k0, k1 = int(np.searchsorted(at, a, "right")) - 1, int(np.searchsorted(at, b, "left"))
    return a + 1, q[k0:k1], t[k0:k1]


@pytest.mark.gpu
def test_natural_breaks(oracle_lib):
    """Two targets and more in one batch: the planted one; the same with a record that does not conform inside window 2
    alone; one whose last window holds two pieces, below min_cov; one with the reads of one haplotype, so no site.  At
    min_len 100 the front reads' pieces of 60 bases in window 2 are not taken there: they are not shared."""
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records()
    _, alns, _, _, _ = _tsr()._planted()
    bad = (341, bb[340:409], [ct.op("M", 70)])                   # 70 columns, 69 read bases
    assert not ct.conforming(bad[0], len(bad[1]), 600, bad[2])
    short = [ct.compress(*(a if k in (0, 12) else _cut(a, 0, 400)), bb) for k, a in enumerate(alns)]
    one_hap = [ct.compress(*a, bb) for a in alns[:12]]
    targets = [(bb, recs), (bb, recs + [bad]), (bb, short), (bb, one_hap)]
    hw = capi.HostWindows.tiled([600] * 4, 150, 30)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(cb, hw, strict=False), hw, 6, 100, 5)
    assert [s != 0 for s in status] == [k == 6 for k in range(16)]
    assert tw[2] == [0, 0, 0, 0, 4, 4, 6, 7, 8, 8, 8, 11, 12, 13, 14, 15] and tw[3][:4] == [0, 0, 1, 1]
    taken = set(zip(sr["aln_tgt"].tolist(), sr["aln_src"].tolist()))
    assert all((1, r) in taken and (2, r) not in taken for r in range(N_FRONT)) and (2, N_FRONT) in taken      # the piece below min_len
    assert not any(w in (6, 11) for w, _ in taken) and np.diff(ps["site_begin"])[12:].tolist() == [0] * 4
    assert dev["same"][11] == 0 and dev["diff"][11] == 0 and not dev["hap"][sr["aln_tgt"] >= 12].any()
    # a depth cap that keeps a record in one window and drops it in the next: 12 reads over [0, 400), then 12 over [250, 600),
    # which match fewer bases.  Windows 1 and 2 hold pieces of all 24 and keep the first 12 and the best 6 of the others;
    # window 3 holds the second 12 alone and keeps them all
    two = [ct.compress(*_cut(alns[k // 2 + 12 * (k % 2)], 0, 400), bb) for k in range(12)]
    two += [ct.compress(*_cut(alns[k // 2 + 12 * (k % 2)], 250, 600), bb) for k in range(12)]
    one = capi.HostCigarBatch(**ct.records_to_arrays([(bb, two)]))
    hw1 = capi.HostWindows.tiled([600], 150, 30)
    sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(one, hw1), hw1, 6, 50, 5, prepare=lambda c: c.set_record_filter(1000000, 18))
    per = [set(sr["aln_src"][sr["aln_tgt"] == w].tolist()) for w in range(4)]
    assert [len(p) for p in per] == [12, 18, 18, 12] and per[1] == per[2] and len(per[3] - per[2]) == 6 and per[3] >= per[2] - per[0]
    assert tw[0][3] + tw[1][3] == 6 and tw[0][2] + tw[1][2] == 18 and all(dev["hap"].tolist())


def _two_window_case(n_prev_only, shared_at, n_cur, place):
    """A 100-base target, windows [0, 60) and [40, 100).  Reads over [0, 40) lie in window 0 alone, reads over [60, 100) in
    window 1 alone, reads over [0, 100) in both.  place: "first" / "last": one shared read, the lowest / highest record
    of window 0; "none": no shared read; "lanes": shared reads at the places `shared_at` of window 1's n_cur alignments.
    Reads alternate between two haplotypes that differ at bases 10, 30, 50, 70, 90."""
    rng = np.random.default_rng(7)
    bb = _tsr()._tes()._nonrep(rng, 100)
    alt = bytearray(bb)
    for p in (10, 30, 50, 70, 90):
        alt[p] = next(b for b in b"ACGT" if b not in (bb[p - 1], bb[p], bb[p + 1]))
    count = [0]

    def read(a, b):
        count[0] += 1
        src = alt if count[0] % 2 else bb
        return (a + 1, bytes(src[a:b]), [ct.op("M", b - a)])
    if place == "lanes":
        cur = [read(0, 100) if k in shared_at else read(60, 100) for k in range(n_cur)]
        return bb, [read(0, 40) for _ in range(n_prev_only)] + cur
    only = [read(0, 40) for _ in range(n_prev_only)]
    cur = [read(60, 100) for _ in range(n_cur)]
    if place == "first":
        return bb, [read(0, 100)] + only + cur
    if place == "last":
        return bb, only + [read(0, 100)] + cur
    return bb, only + cur


@pytest.mark.gpu
def test_the_search_and_the_lane_stride(oracle_lib):
    """k_wl_pairs' periods: predecessor windows of 1, 2, 3, 63, 64 and 65 alignments with the shared record at the first
    place, at the last and not there; current windows of 64, 65 and 129 taken alignments with shared records at lanes 0,
    63 and at the first and last place of the steps behind."""
    from pbdagcon_amd import capi
    cases = [(P, place) for P in (1, 2, 3, 63, 64, 65) for place in ("first", "last", "none")]
    targets = [_two_window_case(P - (place != "none"), None, 4, place) for P, place in cases]
    lanes = {64: (0, 63), 65: (0, 63, 64), 129: (0, 63, 64, 127, 128)}
    targets += [_two_window_case(5, at, C, "lanes") for C, at in lanes.items()]
    hw = capi.HostWindows([t for t in range(len(targets)) for _ in (0, 1)], [0, 40] * len(targets), [60, 100] * len(targets))
    # on the twin first (the whole chain on the CPU)
    global OPTS
    keep, OPTS = OPTS, (1, 200000)
    try:
        (c_tgt, c_src, c_hap), cpu = _cpu_chain(targets, hw, 1, 10, 0)
        n_in = [c_tgt.count(w) for w in range(hw.n_windows)]
        for k, (P, place) in enumerate(cases):
            assert n_in[2 * k] == P and cpu[0][2 * k + 1] + cpu[1][2 * k + 1] == (1 if P > 1 and place != "none" else 0), (P, place)
        for k, (C, at) in enumerate(lanes.items()):
            w = 2 * (len(cases) + k) + 1
            assert n_in[w] == C and cpu[0][w] + cpu[1][w] == len(at) and all(c_hap[i] for i in range(len(c_tgt)) if c_tgt[i] == w)
        cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
        sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(cb, hw), hw, 1, 10, 0, (1, 1000000))
    finally:
        OPTS = keep
    assert (sr["aln_tgt"].tolist(), sr["aln_src"].tolist(), sr["hap"].tolist()) == (c_tgt, c_src, c_hap)
    assert dev["same"].tolist() == cpu[0] and dev["diff"].tolist() == cpu[1]
    assert {b for b, w in zip(dev["block"].tolist(), range(hw.n_windows)) if w % 2} >= {2 * (len(cases) + k) for k in range(3)}   # those link


def _chain(n, turns=(), bare=()):
    """n windows [20 w, 20 w + 40) over a target of 20 n + 120 bases; reads of 100 bases start every 4 bases, about 25
    deep.  The two haplotypes differ at every base = 5 mod 10 outside the windows in `bare`.  The read that starts with
    window w is listed in front of all others, those of later windows first: it is the lowest record among the reads that
    cover window w whole, so it is the seed, and its haplotype names label 1 there.  It is the second haplotype for w in
    `turns`, else the first; the other reads alternate."""
    rng = np.random.default_rng(n)
    L = 20 * n + 120
    bb = _tsr()._tes()._nonrep(rng, L)
    alt = np.frombuffer(bb, np.uint8).copy()
    code = np.frombuffer(b"ACGT", np.uint8)
    for p in range(5, L - 1, 10):
        if any(20 * k <= p < 20 * k + 40 for k in bare):
            continue
        alt[p] = next(b for b in code if b not in (bb[p - 1], bb[p], bb[p + 1]))
    alt = alt.tobytes()
    lead, rest = [], []
    for j, s in enumerate(range(0, L - 99, 4)):
        w = s // 20
        if s % 20 == 0 and w < n:
            lead.append((s + 1, (alt if w in turns else bb)[s:s + 100], [ct.op("M", 100)]))
        else:
            rest.append((s + 1, (alt if j % 2 else bb)[s:s + 100], [ct.op("M", 100)]))
    return bb, lead[::-1] + rest


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_the_wave_ladder_and_the_scan_s_round(oracle_lib, n):
    """k_wl_scan's periods: chains of 63 / 64 / 65 and 1,023 / 1,024 / 1,025 windows.  The orientation turns at the
    windows either side of 64 and of 1,024; in a second chain of 65 and of 1,025 windows a window without a site breaks
    the chain there."""
    from pbdagcon_amd import capi
    hw = capi.HostWindows([0] * n, [20 * w for w in range(n)], [20 * w + 40 for w in range(n)])
    turns = {w for w in (63, 65, 1023, 1025) if w < n}             # the seeds' haplotype alternates over 62 .. 66 and 1,022 .. 1,026
    variants = [(turns, ())] + ([((), tuple(w for w in (63, 1023) if w < n))] if n in (65, 1025) else [])
    for turns, bare in variants:
        targets = [_chain(n, turns, bare)]
        cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
        sr, ps, dev, status, tw = _device(lambda c: c.consensus_cigar_windows(cb, hw), 6, 20, 0) + (None,)
        tw = _twin(hw, sr, ps)
        # on the twin first: where the orientation turns, and where the chain breaks
        flip, block = tw[3], tw[2]
        assert status == [0] * n and all(6 <= c <= 40 for c in np.bincount(sr["aln_tgt"], minlength=n).tolist())
        if not bare:
            assert block == [0] * n
            assert [w for w in range(1, n) if flip[w] != flip[w - 1]] == sorted(w for t in turns for w in (t, t + 1) if w < n)
        else:
            heads = sorted({0} | {w for b in bare for w in (b, b + 1)})
            assert sorted(set(block)) == heads and all(block[w] == max(h for h in heads if h <= w) for w in range(n)) and not any(flip)
            assert all(tw[0][w] == tw[1][w] == 0 for b in bare for w in (b, b + 1))
        _equal(dev, tw, (n, bare))


@pytest.mark.gpu
def test_every_window_entry_point_gives_the_same_arrays(oracle_lib):
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records(chimeras=2)
    targets = [(bb, recs), (bb, recs[::-1])]
    hw = capi.HostWindows.tiled([600, 600], 150, 30)
    n = 2 * len(recs)
    reverse = (np.arange(n) % 3 == 1).astype(np.uint8)
    as_file, i = [], 0
    for t, rs in targets:
        as_file.append((t, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(rs)]))
        i += len(rs)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    arr = ct.records_to_arrays(targets); arr["t_blob"] = None
    md = capi.HostMdTags.from_texts([mt.encode(p, q, t, o) for t, rs in targets for p, q, o in rs])
    cs = capi.HostCsBatch.from_records([(t, [(p, len(q), pf.tspan(o), cst.encode(p, q, t, o)) for p, q, o in rs]) for t, rs in targets])
    calls = {"plain": lambda c: c.consensus_cigar_windows(plain, hw), "packed": lambda c: c._intake(plain.packed(), hw, plain, True),
             "stranded": lambda c: c._intake(capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), hw, None, True),
             "cs": lambda c: c.consensus_cs(cs, hw), "md": lambda c: c.consensus_cigar_md(capi.HostCigarBatch(**arr), md, hw)}
    ref = None
    for kind, call in calls.items():
        sr, ps, dev, status, tw = _run(call, hw, 6, 30, 5)
        assert status == [0] * 8, kind
        if ref is None:
            ref = dev
            assert set(dev["flip"].tolist()) == {0, 1} and dev["block"].tolist() == [0] * 4 + [4] * 4 and dev["diff"].max() > 20
        for k in ref:
            assert np.array_equal(dev[k], ref[k]), (kind, k)


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records()
    cb = capi.HostCigarBatch(**ct.records_to_arrays([(bb, recs)]))
    hw = capi.HostWindows.tiled([600], 150, 30)
    c = capi.Context(min_cov=6, min_len=30, trim=5)
    try:
        assert _code(c.window_phase) == STATE                        # nothing yet
        c.set_pileup(*OPTS); c.set_site_reads(True); c.set_window_phase()
        c.consensus_cigar(cb)                                        # the switch without windows
        assert _code(c.window_phase) == STATE and c.site_reads()["hap"].any()
        c.set_site_reads(False)                                      # the switch without phase
        c.consensus_cigar_windows(cb, hw)
        assert _code(c.window_phase) == STATE and c.site_reads()["hap"] is None
        c.set_site_reads(True)
        c.upload_cigar_windows(cb, hw); c.run(); c.sync()
        assert _code(c.window_phase) == STATE                        # before a fetch
        c.fetch()
        first = c.window_phase()
        again = c.window_phase()                                     # asked twice, and before the site reads
        assert first["block"].tolist() == [0] * 4 and all(np.array_equal(first[k], again[k]) for k in first)
        _equal(first, _twin(hw, c.site_reads(), c.pileup_sites()))
        c.set_window_phase(100)                                      # nothing links at 100
        assert _code(lambda: c.set_window_phase(1, 1000001)) == INVALID    # refused: the earlier setting still holds
        c.consensus_cigar_windows(cb, hw)
        assert c.window_phase()["block"].tolist() == [0, 1, 2, 3] and not c.window_phase()["flip"].any()
        c.set_window_phase(None)                                     # off: this batch's results stay, the next has none
        assert c.window_phase()["block"].tolist() == [0, 1, 2, 3]
        c.consensus_cigar_windows(cb, hw)
        assert _code(c.window_phase) == STATE and c.site_reads()["hap"].any()
        c.set_window_phase(); c.set_hap_consensus()
        c.consensus_cigar_windows(cb, hw)
        assert c.window_phase()["block"].tolist() == [0] * 4
        c.upload_haps()                                              # the derived batch has it off
        assert _code(c.window_phase) == STATE
        c.run(); c.sync(); c.fetch()
        assert _code(c.window_phase) == STATE
    finally:
        c.close()
    stop = capi.Context(min_cov=6, min_len=30, trim=5, flags=capi.FLAG_STOP_AFTER_MERGE)
    try:
        stop.set_pileup(*OPTS); stop.set_site_reads(True); stop.set_window_phase()
        stop.upload_cigar_windows(cb, hw); stop.run(); stop.sync(); stop.fetch()
        assert _code(stop.window_phase) == STATE                     # wherever dagcon_fetch_site_reads is
    finally:
        stop.close()


@pytest.mark.gpu
def test_switch_off(oracle_lib):
    """The results, the sites and the site reads of a windows batch do not know whether the switch was ever set."""
    from pbdagcon_amd import capi
    tes = _tsr()._tes()
    targets = tes._variant_targets(77, 8, 120, 120)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 40, 10)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    got = []
    for mode in ("never", "on", "off again"):
        c = capi.Context(min_cov=3, min_len=30, trim=5)
        try:
            c.set_pileup(*OPTS); c.set_site_reads(True)
            if mode != "never":
                c.set_window_phase()
            if mode == "off again":
                c.consensus_cigar_windows(cb, hw)
                assert c.window_phase()["same"].size == 24
                c.set_window_phase(None)
            res = c.consensus_cigar_windows(cb, hw)
            if mode != "on":
                assert _code(c.window_phase) == STATE
            got.append((res, c.pileup_sites(), c.site_reads(), c.pileup(), c.timings()["reruns"]))
        finally:
            c.close()
    for res, ps, sr, pu, reruns in got[1:]:
        assert res == got[0][0] and reruns == got[0][4]
        for a, b in ((ps, got[0][1]), (sr, got[0][2]), (pu, got[0][3])):
            assert all(np.array_equal(a[k], b[k]) for k in b)
    assert got[0][2]["hap"].any()


@pytest.mark.gpu
def test_pbdagcon_phase_windows(oracle_lib, tmp_path):
    from pbdagcon_amd import capi
    bb, recs, groups = _planted_records(chimeras=2)
    name, W, O = "ctg", 150, 70
    qn = ["q0_%d" % k for k in range(len(recs))]
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta([name], [bb]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam([name], [600], [recs]))
    # the twin's text, from the arrays of one upload of all the windows (which are the twin's own: checked here too)
    tiles = wt.tiled(600, W, O)
    hw = capi.HostWindows.tiled([600], W, O)
    cb = capi.HostCigarBatch(**ct.records_to_arrays([(bb, recs)]))
    sr, ps, dev, status, tw = _run(lambda c: c.consensus_cigar_windows(cb, hw), hw, 6, 30, 5)
    assert set(tw[3]) == {0, 1} and tw[2] == [0] * 4
    site_w = np.repeat(np.arange(4), np.diff(ps["site_begin"].astype(np.int64))).tolist()
    core = [tiles[w][2] - tiles[w][0] <= int(p) < tiles[w][3] - tiles[w][0] for w, p in zip(site_w, ps["pos"].tolist())]
    ents = [[] for _ in core]                                        # per site its entries: (record, code), in record order
    n_signed = {}
    for x, r in enumerate(sr["aln_src"].tolist()):
        n_signed.setdefault(r, 0)
        for e in range(int(sr["ent_begin"][x]), int(sr["ent_begin"][x + 1])):
            k, code = int(sr["ent_site"][e]), int(sr["ent_code"][e])
            ents[k].append((r, code))
            n_signed[r] += bool(core[k] and srt.sign(code, ps["counts"][k].tolist()))
    reads = [srt.site_reads_line(name, int(ps["pos"][k]) + tiles[site_w[k]][0], qn[r], code) for k in range(len(core)) if core[k] for r, code in sorted(ents[k])]
    labels = wpt.record_labels(sr["aln_tgt"].tolist(), sr["aln_src"].tolist(), dev["hap"].tolist(), dev["block"].tolist())
    tags = [wpt.haplotag_line(name, qn[r], labels[r][0], n_signed[r], None if labels[r][1] is None else 1 + tiles[labels[r][1]][2]) for r in sorted(labels)]
    assert len(tags) == len(recs) and len(reads) > 200 and len({int(ps["pos"][k]) + tiles[site_w[k]][0] for k in range(len(core)) if core[k]}) == sum(core)
    # every read its planted label and one PS; a chimera is what most of its pieces say
    assert [t.split("\t")[2:] for t in tags[:24]] == [[str(g), t.split("\t")[3], "1"] for g, t in zip(groups[:24], tags)]
    base = [_cli(), "-c", "6", "-m", "30", "-t", "5", "--sam", "--ref", str(ref), "--window", str(W), "--overlap", str(O)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    plain = run(str(sam))
    assert plain.stdout.count(b">") >= 1
    for k, bt in enumerate(([], ["--batch-targets", "1"], ["--batch-targets", "2"])):
        fr, fh = tmp_path / ("r%d" % k), tmp_path / ("h%d" % k)
        got = run("--phase-windows", "--site-reads", str(fr), "--haplotag", str(fh), "-v", *bt, str(sam))
        assert got.stdout == plain.stdout, bt
        assert fr.read_text().splitlines() == reads and fh.read_text().splitlines() == tags, bt
        assert b"--phase-windows: 1 blocks over 4 windows" in got.stderr
    # one file alone, and thresholds that link nothing: every window a block of its own, PS by the window that holds most pieces
    fh = tmp_path / "h_alone"
    run("--phase-windows", "--haplotag", str(fh), str(sam))
    assert fh.read_text().splitlines() == tags
    got = run("--phase-windows", "--phase-min-links", "100", "--phase-max-conflict", "0.5", "--haplotag", str(fh), "-v", "--batch-targets", "3", str(sam))
    assert b"--phase-windows: 4 blocks over 4 windows" in got.stderr and {t.split("\t")[4] for t in fh.read_text().splitlines()} == {"1"}
