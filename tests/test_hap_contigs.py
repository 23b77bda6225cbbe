"""Phased contigs across windows (pbdagcon --window --phase-windows --hap-contigs / --hap-windows), the groups in the
caller's orientation (dagcon_upload_haps_swapped) and the kept part of every segment cut on the device
(dagcon_set_window_keep, rule 12 of include/dagcon.h): the twin against the existing stitch, the binding, the usage errors
and the line formatters on the CPU; the device against the twin on the GPU.  hap_contigs_twin.py is the rule in Python;
tests/test_keep_host.py runs the kernel's step on the CPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bam_files as bf
import cigar_twin as ct
import hap_contigs_twin as hct
import hap_twin as ht
import site_reads_twin as srt
import window_twin as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -8, -1
OPTS = (2, 200000)                                               # the pile-up's thresholds of every run here
NAMES = ("dagcon_upload_haps_swapped", "dagcon_set_window_keep", "dagcon_fetch_window_keep")


def _twp():
    import test_window_phase as twp
    return twp


def _tes():
    import test_edit_support as tes
    return tes


def _cli():
    return _tes()._cli()


def _code(f):
    from pbdagcon_amd import capi
    with pytest.raises(capi.DagconError) as e:
        f()
    return e.value.code


# ---- CPU: the twin against the existing stitch ------------------------------------------------------------------------

def test_contigs_of_one_block_and_one_label_are_the_plain_stitch():
    """window_twin.stitch joins the windows of a target from their per-base positions; contigs joins them from the keep
    records.  With every window in one block the two are one rule."""
    rng = np.random.default_rng(4)
    n_joined = n_breaks = 0
    for case in range(300):
        W, O = int(rng.integers(20, 60)), int(rng.integers(5, 20))
        tlen = int(rng.integers(W, 5 * W))
        plain, derived = [], []
        for wi, (begin, end, c0, c1) in enumerate(wt.tiled(tlen, W, O)):
            segs, krecs = [], []
            x = int(rng.integers(0, 4))
            while x < end - begin - 5 and rng.random() < 0.9:   # segments: stretches of the window, with inserted bases and a dip now and then
                y = min(end - begin, x + int(rng.integers(5, end - begin + 1)))
                pos = []
                for p in range(x + 1, y + 1):
                    pos.append(p)
                    if rng.random() < 0.1:
                        pos.append(p + 1)                      # an inserted base: the position of the target base behind it
                if rng.random() < 0.1 and len(pos) > 6:
                    pos[3] = max(1, pos[3] - int(rng.integers(1, 9)))      # nothing assumes that the positions are monotone
                seq = bytes(rng.choice(list(b"ACGT"), size=len(pos)).tolist())
                segs.append((seq, pos, None))
                krecs.append((seq, hct.keep(pos, c0 - begin, c1 - begin)))
                x = y + int(rng.integers(0, 12))
            plain.append((begin, c0, c1, segs))
            derived.append((wi, begin, 0, krecs))
        for min_len in (0, 30):
            want = wt.stitch(plain, min_len)
            got = hct.contigs(derived, min_len)
            assert [g[:3] for g in got] == [w[:3] for w in want], case
            n_joined += sum(1 for w in want if w[1] - w[0] > W + O)
            n_breaks += len(want) > 1
    assert n_joined > 50 and n_breaks > 50


def test_the_block_condition_and_a_missing_window():
    seq = b"ACGTACGTAC"
    cut_end, cut_begin = (0, 6, 1, 6), (4, 10, 7, 12)            # window 0 cut at its core end, window 1 at its core begin
    two = [(0, 0, 0, [(seq, cut_end)]), (1, 2, 0, [(seq, cut_begin)])]
    assert hct.contigs(two, 0) == [(0, 14, seq[:6] + seq[4:], 0)]
    other_block = [(0, 0, 0, [(seq, cut_end)]), (1, 2, 1, [(seq, cut_begin)])]
    assert hct.contigs(other_block, 0) == [(0, 6, seq[:6], 0), (8, 14, seq[4:], 1)]
    gap = [(0, 0, 0, [(seq, cut_end)]), (2, 2, 0, [(seq, cut_begin)])]           # window 1 was not split: no derived window
    assert [c[:2] for c in hct.contigs(gap, 0)] == [(0, 6), (8, 14)]
    not_cut = [(0, 0, 0, [(seq, (0, 10, 1, 10))]), (1, 2, 0, [(seq, cut_begin)])]   # the piece before ran to its segment's end
    assert len(hct.contigs(not_cut, 0)) == 2
    from_start = [(0, 0, 0, [(seq, cut_end)]), (1, 2, 0, [(seq, (0, 10, 7, 16))])]   # i0 == 0: not cut at its core begin
    assert len(hct.contigs(from_start, 0)) == 2
    empty_between = [(0, 0, 0, [(seq, cut_end), (seq, (0, 0, 0, 0))]), (1, 2, 0, [(seq, cut_begin)])]   # an empty part is ignored
    assert len(hct.contigs(empty_between, 0)) == 1
    assert hct.contigs(two, 13) == [] and len(hct.contigs(two, 12)) == 1          # pieces shorter than -m are dropped, joined ones counted whole
    recs = [(10, 2, "b"), (0, 2, "a2"), (0, 1, "a1"), (10, 1, "c")]
    assert hct.order_records(recs) == ["a1", "a2", "c", "b"]
    assert hct.contig_record("ctg", 2, 151, 150, 600, b"ACGT") == ">ctg/hap2/151/150_600\nACGT\n"


# ---- CPU: the binding, the command line, the formatters ----------------------------------------------------------------

def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %zu\\n", sizeof(dagcon_window_keep_opts), '
            'sizeof(dagcon_window_keep)); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert [ctypes.sizeof(x) for x in (capi.WindowKeepOpts, capi.WindowKeep)] == out == [24, 40]
    for m in ("upload_haps", "set_window_keep", "window_keep"):
        assert callable(getattr(capi.Context, m))
    assert lib.dagcon_abi_version() == 2
    head = open(os.path.join(ROOT, "include", "dagcon.h")).read()
    rule = head.split(" * 12. ")[1].split("*/")[0]
    assert "PARITY UNPINNED" in head.split(" * 12. ")[0][-300:] and "Only first\n *     crossings count" in rule and "0 0 0 0" in rule


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    fc, fw, ht_ = tmp_path / "o.fa", tmp_path / "o.win", tmp_path / "o.tags"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))
    m5 = tmp_path / "in.m5"; m5.write_text("")

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    win = rec + ["--window", "200", "--overlap", "120"]
    for args in (rec + ["--hap-contigs", str(fc), str(sam)], rec + ["--hap-windows", str(fw), str(sam)],           # without --window
                 win + ["--hap-contigs", str(fc), str(sam)], win + ["--hap-windows", str(fw), str(sam)],           # without --phase-windows
                 rec + ["--phase-windows", "--hap-contigs", str(fc), str(sam)],
                 ["--hap-contigs", str(fc), str(m5)], ["-a", "--hap-contigs", str(fc), str(m5)], ["-a", "--polish", "1", "--hap-windows", str(fw), str(m5)],
                 win + ["--phase-windows", "--hap-contigs"], win + ["--phase-windows", "--hap-contigs", str(fc), "--hap-windows"],
                 win + ["--phase-windows", "--dump-parsed", "--hap-contigs", str(fc), str(sam)],
                 win + ["--phase-windows", "--hap-contigs", str(fc), "--hap-min-sites", "x", str(sam)],
                 win + ["--phase-windows", "--hap-contigs", str(fc), "--site-min-frac", "1.5", str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not fc.exists() and not fw.exists()
    # what stays refused with --window, beside the new flags too
    for flag in ("--hap-consensus", "--hap-sites", "--hap-vcf", "--site-alleles", "--site-vcf", "--vcf"):
        out = run(*win, "--phase-windows", "--hap-contigs", str(fc), flag, str(tmp_path / "o.x"), str(sam))
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, flag
    # either flag alone is enough for --phase-windows, and the thresholds go with them: the files are opened before anything runs
    for args in (["--hap-contigs", str(tmp_path / "no_such_dir" / "o.fa")], ["--hap-windows", str(tmp_path / "no_such_dir" / "o.win")],
                 ["--hap-min-sites", "3", "--hap-min-reads", "4", "--site-min-count", "2", "--phase-min-links", "2", "--hap-contigs", str(fc),
                  "--hap-windows", str(tmp_path / "no_such_dir" / "o.win")],
                 ["--haplotag", str(ht_), "--hap-contigs", str(tmp_path / "no_such_dir" / "o.fa")]):
        out = run(*win, "--phase-windows", *args, str(sam))
        assert out.returncode == 1 and b"cannot write" in out.stderr and b"no_such_dir" in out.stderr, args
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --hap-contigs FILE")[1].split(b"\n  <input>")[0]
    assert b"\n  --hap-windows FILE" in text and b">RNAME/hap{1|2}/PS/t0_t1" in text and text.count(b"parity unpinned") == 1
    assert b"#window RNAME BEGIN END PS N1 N2 N0 SEP AGREE DISAGREE SPLIT" in text and b"RNAME POS PHASE P1 M1 P2 M2" in text
    assert b"--hap-contigs FILE" in h.stdout.split(b"\n")[0]      # the synopsis
    # the new text stands behind every flag an existing test cuts the help at
    assert h.stdout.index(b"\n  --hap-contigs FILE") > h.stdout.index(b"\n  --contexts N")


_HC_MAIN = r"""
#include <iostream>
#include "hap_contigs.h"
// stdin, one case a line: "w rname begin end ps n1 n2 n0 sep agree disagree split flip" -> the #window line
//                         "s rname pos1 phase p1 m1 p2 m2 flip" -> the site line
//                         "c rname min_len n (label w begin block n_bases i0 i1 p_first p_last)*" -> the records of one target (bases: ACGT by index)
int main() {
    std::string out, kind, rname;
    while (std::cin >> kind >> rname) {
        if (kind == "w") {
            unsigned long long b, e, ps; unsigned v[7], flip;
            std::cin >> b >> e >> ps;
            for (unsigned &x : v) std::cin >> x;
            std::cin >> flip;
            dg_hap_window_line(out, rname, b, e, ps, v[0], v[1], v[2], v[3], v[4], v[5], v[6], flip != 0);
        } else if (kind == "s") {
            unsigned long long pos1; int phase; unsigned c[4], flip;
            std::cin >> pos1 >> phase >> c[0] >> c[1] >> c[2] >> c[3] >> flip;
            const uint16_t cc[4] = {(uint16_t)c[0], (uint16_t)c[1], (uint16_t)c[2], (uint16_t)c[3]};
            dg_hap_window_site_line(out, rname, pos1, phase, cc, flip != 0);
        } else {
            size_t min_len, n;
            std::cin >> min_len >> n;
            DgHapStitch st[2];
            for (size_t k = 0; k < n; k++) {
                unsigned label, begin, nb, i0, i1, pf, pl; long long w; unsigned long long block;
                std::cin >> label >> w >> begin >> block >> nb >> i0 >> i1 >> pf >> pl;
                std::string seq(nb, 'A');
                for (unsigned i = 0; i < nb; i++) seq[i] = "ACGT"[(i + (unsigned)w) & 3u];
                st[label - 1].add(w, begin, block, seq.data(), nb, i0, i1, pf, pl);
            }
            dg_hap_contig_records(out, rname, st, min_len, [](uint64_t block) { return block * 100u + 1u; });
        }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_host_stitch_and_the_line_formatters_against_the_twin(tmp_path):
    src = tmp_path / "hc_main.cpp"; src.write_text(_HC_MAIN)
    exe = tmp_path / "hc_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    rng = np.random.default_rng(9)
    text, want = [], []
    for flip in (0, 1):
        v = [int(x) for x in rng.integers(0, 4000000000, size=7)]
        text.append("w a/b|c 150 300 4294967297 %s %d" % (" ".join(map(str, v)), flip))
        want.append(hct.window_line("a/b|c", 150, 300, 4294967297, *v, flip))
        c = [int(x) for x in rng.integers(0, 65536, size=4)]
        for phase in (1, -1):
            text.append("s ctg 123456789012 %d %s %d" % (phase, " ".join(map(str, c)), flip))
            want.append(hct.site_line("ctg", 123456789012, phase, *c, flip))
    assert hct.window_line("c", 0, 150, 1, 7, 5, 3, 4, 40, 2, 1, 1) == "#window\tc\t0\t150\t1\t5\t7\t3\t4\t40\t2\t1"
    assert hct.site_line("c", 31, 1, 9, 0, 1, 8, 1) == "c\t31\t-1\t1\t8\t9\t0"
    n_multi = 0
    for case in range(400):
        # one target: up to six windows of 40 bases with 10 on either side, blocks that change now and then, windows that
        # are missing for one label or both, segments with every kind of keep record
        parts, derived = [], {1: [], 2: []}
        block = 0
        for w in range(int(rng.integers(1, 7))):
            begin = max(0, 40 * w - 10)
            if w and rng.random() < 0.2:
                block = w
            for label in (1, 2):
                if rng.random() < 0.15:
                    continue
                segs = []
                for _ in range(int(rng.integers(1, 3))):
                    nb = int(rng.integers(1, 70))
                    kind = rng.random()
                    i0 = 0 if kind < 0.3 else int(rng.integers(0, nb))
                    i1 = nb if kind > 0.7 else int(rng.integers(i0, nb + 1))
                    pf, pl = (int(rng.integers(1, 60)), int(rng.integers(1, 60))) if i1 > i0 else (0, 0)
                    if i1 == i0:
                        i0 = i1 = 0
                    seq = bytes(b"ACGT"[(i + w) & 3] for i in range(nb))
                    segs.append((seq, (i0, i1, pf, pl)))
                    parts.append("%d %d %d %d %d %d %d %d %d" % (label, w, begin, block, nb, i0, i1, pf, pl))
                derived[label].append((w, begin, block, segs))
        min_len = int(rng.choice([0, 20, 60]))
        text.append("c tgt%d %d %d %s" % (case, min_len, len(parts), " ".join(parts)))
        recs = [(c[0], label, hct.contig_record("tgt%d" % case, label, c[3] * 100 + 1, c[0], c[1], c[2])) for label in (1, 2) for c in hct.contigs(derived[label], min_len)]
        n_multi += len(recs) > 2
        want += [ln for r in hct.order_records(recs) for ln in r.splitlines()]
    assert n_multi > 100
    out = subprocess.run([str(exe)], input=("\n".join(text) + "\n").encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert out == want


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _flat_keep(positions, lo, hi, src=None):
    """The twin's records for per-target, per-segment positions (Context.base_positions()), as four lists."""
    exp = [hct.keep(p.tolist(), int(lo[src[t] if src is not None else t]), int(hi[src[t] if src is not None else t])) for t, segs in enumerate(positions) for p in segs]
    return {k: [e[i] for e in exp] for i, k in enumerate(("i0", "i1", "p_first", "p_last"))}


def _assert_keep(got, exp, what=""):
    for k in ("i0", "i1", "p_first", "p_last"):
        assert got[k].tolist() == exp[k], (what, k, got[k].tolist(), exp[k])


def _plain_reads(bb, a, b, n):
    return [(a + 1, bytes(bb[a:b]), [ct.op("M", b - a)]) for _ in range(n)]


@pytest.mark.gpu
def test_keep_on_a_windows_upload(oracle_lib):
    """One clean target of 200 bases under six identical reads, uploaded as many windows of the same [0, 200), each with a
    (lo, hi) of its own: with P(i) = i + 1 the pair puts i0 = lo and i1 = hi, so the boundaries of tests/test_keep_host.py
    are met through the real pos_out.  Then the same with the edits on (bit 31 is set on the device), segment counts of 1,
    4 and 5 (a block holds four waves), and a batch with a coverage gap, a window below min_cov and a failed window."""
    from pbdagcon_amd import capi
    rng = np.random.default_rng(11)
    bb = _tes()._nonrep(rng, 200)
    pairs = [(0, 200), (0, 64), (0, 65), (63, 64), (63, 65), (63, 200), (64, 65), (64, 129), (64, 200), (1, 63), (62, 128), (127, 128), (128, 129), (128, 200),
             (199, 200), (0, 0), (100, 100), (200, 200), (200, 250), (0, 1000), (70, 90), (70, 71), (5, 5000)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays([(bb, _plain_reads(bb, 0, 200, 6))]))
    for n_win in (1, 4, 5, len(pairs)):
        use = pairs[:n_win] if n_win == len(pairs) else pairs[3:3 + n_win]
        lo, hi = [p[0] for p in use], [p[1] for p in use]
        hw = capi.HostWindows([0] * n_win, [0] * n_win, [200] * n_win)
        seen = []
        for edits in (False, True):
            c = capi.Context(min_cov=3, min_len=30, trim=0, flags=capi.FLAG_BASE_POS)
            try:
                c.set_edits(edits)
                c.set_window_keep(lo, hi)
                res = c.consensus_cigar_windows(cb, hw)
                assert [len(x) for x in res] == [1] * n_win and all(x[0][2] == bytes(bb) for x in res)
                wk = c.window_keep()
                again = c.window_keep()
                assert all(np.array_equal(wk[k], again[k]) for k in wk)
                pos = c.base_positions()
                assert all(p[0].tolist() == list(range(1, 201)) for p in pos)
                _assert_keep(wk, _flat_keep(pos, lo, hi), (n_win, edits))
                if edits:
                    assert c.edits()["seg_t0"].size == n_win     # (the edit kernels ran on the same pos_out)
                seen.append(wk)
            finally:
                c.close()
        assert all(np.array_equal(seen[0][k], seen[1][k]) for k in seen[0])
        if n_win == len(pairs):
            kept = {(a, b) for a, b in zip(seen[0]["i0"].tolist(), seen[0]["i1"].tolist())}
            assert {(0, 200), (0, 64), (63, 64), (63, 65), (64, 65), (64, 200), (128, 129), (199, 200), (70, 71)} <= kept and (0, 0) in kept
            assert seen[0]["i0"].tolist().count(0) >= 7 and {0, 63, 64} <= set(seen[0]["i0"].tolist()) and {64, 65, 200} <= set(seen[0]["i1"].tolist())
    # a gap in the coverage (two segments), a window below min_cov, a window failed by a non-conforming record
    gap = _plain_reads(bb, 0, 90, 6) + _plain_reads(bb, 110, 200, 6)
    few = _plain_reads(bb, 0, 200, 2)
    bb3 = _tes()._nonrep(rng, 300)
    bad = (141, bytes(bb3[140:159]), [ct.op("M", 20)])               # 20 columns, 19 read bases: inside window [100, 200) alone
    assert not ct.conforming(bad[0], len(bad[1]), 300, bad[2])
    targets = [(bb, _plain_reads(bb, 0, 200, 6)), (bb, gap), (bb, few), (bb3, _plain_reads(bb3, 0, 300, 6) + [bad])]
    hw = capi.HostWindows([0, 1, 2, 3, 3, 3], [0, 0, 0, 0, 100, 200], [200, 200, 200, 100, 200, 300])
    lo, hi = [10, 20, 0, 5, 5, 5], [150, 180, 200, 50, 50, 50]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    for edits in (False, True):
        c = capi.Context(min_cov=3, min_len=30, trim=0, flags=capi.FLAG_BASE_POS)
        try:
            c.set_edits(edits)
            c.set_window_keep(lo, hi)
            res = c.consensus_cigar_windows(cb, hw, strict=False)
            assert [len(x) for x in res] == [1, 2, 0, 1, 0, 1] and [s != 0 for s in c.target_status.tolist()] == [False] * 4 + [True, False]
            wk = c.window_keep()
            pos = c.base_positions()
            _assert_keep(wk, _flat_keep(pos, lo, hi), edits)
            # the first segment of the gapped window ends below hi; the second begins above lo: kept to its end, from its start
            assert wk["i0"].tolist() == [10, 20, 0, 5, 5] and wk["i1"].tolist() == [150, 90, 70, 50, 50] and wk["p_first"].tolist() == [11, 21, 111, 6, 6]
        finally:
            c.close()


def _planted():
    """The planted target of test_window_phase as one batch of four windows, with what the tests here need beside it."""
    from pbdagcon_amd import capi
    twp = _twp()
    bb, recs, groups = twp._planted_records()
    targets = [(bb, recs)]
    hw = capi.HostWindows.tiled([600], 150, 30)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    src = [[k for k, (p, q, o) in enumerate(recs) if max(a, wt.span(p, 600, o)[0]) < min(b, wt.span(p, 600, o)[1])] for _, a, b in wins]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    tiles = wt.tiled(600, 150, 30)
    lo = [t[2] - t[0] for t in tiles]
    hi = [t[3] - t[0] for t in tiles]
    return dict(bb=bb, recs=recs, groups=groups, targets=targets, hw=hw, wins=wins, per=per, src=src, cb=cb, lo=lo, hi=hi, tiles=tiles)


MIN_COV, MIN_LEN, TRIM = 6, 30, 5


def _first_batch(c, P, keep=None):
    """The planted windows with the pile-up, the split, the window phase and the tally on: (results, site reads, window phase, tally)."""
    c.set_pileup(*OPTS); c.set_site_reads(True); c.set_window_phase(); c.set_hap_consensus()
    if keep is not None:
        c.set_window_keep(*keep)
    res = c.consensus_cigar_windows(P["cb"], P["hw"])
    return res, c.site_reads(), c.window_phase(), c.hap_tally()


def _expect_groups(P, sr, ohap):
    """Per derived target in the caller's orientation (window, label, indices into the window's pieces), from the
    device's own oriented labels: label L holds the window's pieces whose oriented label is L or 0."""
    label = {(int(t), int(s)): int(h) for t, s, h in zip(sr["aln_tgt"], sr["aln_src"], ohap)}
    out = []
    for w, (tl, alns, failed) in enumerate(P["per"]):
        for L in (1, 2):
            out.append((w, L, [i for i, (_, q, _) in enumerate(alns) if len(q) >= MIN_LEN and label.get((w, P["src"][w][i]), 0) in (0, L)]))
    return out


@pytest.mark.gpu
def test_swapped_groups(oracle_lib):
    from pbdagcon_amd import capi
    from util import batch_from_targets, oracle_batch
    P = _planted()
    twp = _twp()
    # on the CPU first: all four windows are split at the default thresholds, and both orientations occur
    (c_tgt, c_src, c_hap), cpu = twp._cpu_chain(P["targets"], P["hw"], MIN_COV, MIN_LEN, TRIM)
    split = [ht.tally(srt.target(tl, alns, MIN_LEN, TRIM, OPTS), ht.held(alns, MIN_LEN), 0, 0, MIN_COV)["split"] for tl, alns, _ in P["per"]]
    assert split == [1] * 4 and set(cpu[3]) == {0, 1} and cpu[2] == [0] * 4
    runs = {}
    for mode in ("plain", "zeros", "flip"):
        c = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
        try:
            res, sr, wp, tally = _first_batch(c, P)
            assert tally["split"].tolist() == [1] * 4 and wp["flip"].tolist() == cpu[3] and wp["block"].tolist() == [0] * 4
            if mode == "plain":
                c.upload_haps()
            else:
                c.upload_haps(swap=np.zeros(4, np.uint8) if mode == "zeros" else wp["flip"])
            hm = c.hap_map()
            c.run(); c.sync()
            runs[mode] = (c.fetch(), hm, sr, wp, c.target_status.tolist())
        finally:
            c.close()
    # NULL and all zeros are dagcon_upload_haps
    assert runs["zeros"][0] == runs["plain"][0] and all(np.array_equal(runs["zeros"][1][k], runs["plain"][1][k]) for k in runs["plain"][1])
    got, hm, sr, wp, status = runs["flip"]
    assert status == [0] * 8 and hm["src_target"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and hm["label"].tolist() == [1, 2] * 4
    groups = _expect_groups(P, sr, wp["hap"].tolist())
    exp_src = [P["src"][w][i] for w, L, idx in groups for i in idx]
    assert hm["aln_src"].tolist() == exp_src and hm["aln_begin"].tolist() == np.concatenate([[0], np.cumsum([len(idx) for _, _, idx in groups])]).tolist()
    # label 1 is planted group 1 (and the unlabelled reads) in every window, whatever the window's own names are
    for d, (w, L, idx) in enumerate(groups):
        planted = {P["groups"][P["src"][w][i]] for i in idx}
        assert planted == {L}, (w, L, planted)
        assert len(idx) == sum(1 for r in P["src"][w] if P["groups"][r] == L)
    # a flipped window's groups are the plain run's, the other way round
    pm = runs["plain"][1]
    for w in range(4):
        a = [pm["aln_src"][int(pm["aln_begin"][2 * w + k]):int(pm["aln_begin"][2 * w + k + 1])].tolist() for k in (0, 1)]
        b = [hm["aln_src"][int(hm["aln_begin"][2 * w + k]):int(hm["aln_begin"][2 * w + k + 1])].tolist() for k in (0, 1)]
        assert b == (a[::-1] if wp["flip"][w] else a)
        assert got[2 * w:2 * w + 2] == (runs["plain"][0][2 * w:2 * w + 2][::-1] if wp["flip"][w] else runs["plain"][0][2 * w:2 * w + 2])
    # each derived window is the oracle's consensus of the group's strings
    gb = batch_from_targets([(P["per"][w][0], [P["per"][w][1][i] for i in idx], None) for w, L, idx in groups])
    assert got == oracle_batch(gb, MIN_COV, MIN_LEN, TRIM)


def _derived_run(c, P, keep_first=False):
    """First batch, then the derived batch in the block's orientation under the windows' cores: (results, hap map, keep, positions)."""
    res, sr, wp, tally = _first_batch(c, P, (P["lo"], P["hi"]) if keep_first else None)
    first_keep = c.window_keep() if keep_first else None
    first_pos = c.base_positions() if keep_first else None
    if not keep_first:
        c.set_window_keep(P["lo"], P["hi"])
    c.upload_haps(swap=wp["flip"])
    hm = c.hap_map()
    c.run(); c.sync()
    got = c.fetch()
    return dict(res=res, wp=wp, got=got, hm=hm, keep=c.window_keep(), pos=c.base_positions(), first_keep=first_keep, first_pos=first_pos)


@pytest.mark.gpu
def test_keep_on_the_derived_batch(oracle_lib):
    from pbdagcon_amd import capi
    P = _planted()
    for keep_first in (False, True):
        c = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
        try:
            r = _derived_run(c, P, keep_first)
            assert len(r["got"]) == 8 and sum(len(x) for x in r["got"]) == r["keep"]["i0"].size >= 8
            _assert_keep(r["keep"], _flat_keep(r["pos"], P["lo"], P["hi"], r["hm"]["src_target"].tolist()), keep_first)
            if keep_first:
                _assert_keep(r["first_keep"], _flat_keep(r["first_pos"], P["lo"], P["hi"]), "first batch")
            # the inner windows are cut on both sides, the outer ones on one
            n = [len(x[0][2]) for x in r["got"]]
            assert all(len(x) == 1 for x in r["got"])
            assert [i > 0 for i in r["keep"]["i0"].tolist()] == [False] * 2 + [True] * 6 and [i < m for i, m in zip(r["keep"]["i1"].tolist(), n)] == [True] * 6 + [False] * 2
        finally:
            c.close()


@pytest.mark.gpu
def test_keep_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    P = _planted()
    lo, hi, cb, hw = P["lo"], P["hi"], P["cb"], P["hw"]
    plain = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        assert _code(lambda: plain.set_window_keep(lo, hi)) == STATE and _code(plain.window_keep) == STATE     # no DAGCON_FLAG_BASE_POS
    finally:
        plain.close()
    c = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
    try:
        assert _code(c.window_keep) == STATE                         # nothing yet
        want = c.consensus_cigar_windows(cb, hw)                     # the switch off: a context that never heard of it
        want_pos = c.base_positions()
        tm = c.timings()
        assert _code(c.window_keep) == STATE
        c.set_window_keep(lo, hi)                                    # set after the upload
        assert _code(c.window_keep) == STATE
        c.consensus_cigar(cb)                                        # whole targets: as if off
        assert _code(c.window_keep) == STATE
        c.upload_cigar_windows(cb, hw); c.run(); c.sync()
        assert _code(c.window_keep) == STATE                         # before a fetch
        assert c.fetch() == want
        first = c.window_keep()
        _assert_keep(first, _flat_keep(c.base_positions(), lo, hi))
        assert _code(lambda: c.set_window_keep([5, 5, 5, 5], [9, 9, 4, 9])) == INVALID     # lo > hi: the switch stays as it was
        assert c.consensus_cigar_windows(cb, hw) == want and all(np.array_equal(c.window_keep()[k], first[k]) for k in first)
        c.set_window_keep(lo[:3], hi[:3])                            # n is not the number of windows: refused before any launch
        assert _code(lambda: c.upload_cigar_windows(cb, hw)) == INVALID
        assert _code(c.window_keep) == STATE and _code(c.fetch) == STATE
        c.set_window_keep(None)                                      # off again: results, positions and counts of a context that never set it
        assert c.consensus_cigar_windows(cb, hw) == want and _code(c.window_keep) == STATE
        assert all(np.array_equal(a, b) for x, y in zip(c.base_positions(), want_pos) for a, b in zip(x, y))
        tm2 = c.timings()
        assert all(tm2[k] == tm[k] for k in ("reruns", "n_nodes", "n_columns", "merge_segments", "consensus_bases", "n_alignments"))
        # behind a windows upload that ran without it, dagcon_upload_haps reads the switch too -- and checks n
        c.set_pileup(*OPTS); c.set_site_reads(True); c.set_window_phase(); c.set_hap_consensus()
        c.consensus_cigar_windows(cb, hw)
        flip = c.window_phase()["flip"]
        c.set_window_keep(lo[:3], hi[:3])
        assert _code(lambda: c.upload_haps(swap=flip)) == INVALID
        assert _code(c.fetch) == STATE and _code(c.hap_map) == STATE      # as after any failed upload
        c.set_window_keep(None)
        c.consensus_cigar_windows(cb, hw)
        c.upload_haps(swap=flip)                                     # the switch off at dagcon_upload_haps: as if off
        c.run(); c.sync()
        off = c.fetch()
        assert _code(c.window_keep) == STATE and len(c.base_positions()) == 8
        c.set_window_keep(lo, hi)
        c.consensus_cigar_windows(cb, hw)
        assert c.window_keep()["i0"].size == 4
        c.upload_haps(swap=flip)
        assert _code(c.window_keep) == STATE                         # after a later upload; before the derived batch's fetch
        c.run(); c.sync()
        assert c.fetch() == off and c.window_keep()["i0"].size == sum(len(x) for x in off)
        c.consensus_cigar(cb)                                        # and after any later upload
        assert _code(c.window_keep) == STATE
    finally:
        c.close()
    # behind a whole-target record upload the derived batch has it off
    w = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
    try:
        w.set_pileup(*OPTS); w.set_site_reads(True); w.set_hap_consensus(); w.set_window_keep([0], [600])
        w.consensus_cigar(cb)
        assert w.hap_tally()["split"].size == 1 and _code(w.window_keep) == STATE
        w.upload_haps(); w.run(); w.sync(); w.fetch()
        assert _code(w.window_keep) == STATE
    finally:
        w.close()
    stop = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS | capi.FLAG_STOP_AFTER_MERGE)
    try:
        stop.set_window_keep(lo, hi)
        stop.upload_cigar_windows(cb, hw); stop.run(); stop.sync(); stop.fetch()
        assert _code(stop.window_keep) == STATE                      # wherever dagcon_fetch_positions is
    finally:
        stop.close()


@pytest.mark.gpu
def test_poisoned_buffers(oracle_lib, monkeypatch):
    from pbdagcon_amd import capi
    P = _planted()
    clean = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
    try:
        want = _derived_run(clean, P, True)
    finally:
        clean.close()
    monkeypatch.setenv("DAGCON_POISON", "15")
    c = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
    try:
        r = _derived_run(c, P, True)
    finally:
        c.close()
    assert r["got"] == want["got"] and r["res"] == want["res"]
    for k in ("keep", "first_keep"):
        assert all(np.array_equal(r[k][x], want[k][x]) for x in want[k]), k


# ---- GPU: the files ----------------------------------------------------------------------------------------------------

def _api_files(targets, names, W, O, min_cov, min_len, trim, hap=(0, 0)):
    """The twin's two files from the API's arrays: every target's windows in ONE upload (so every link is the device's),
    then the derived batch in the block's orientation under the windows' cores."""
    from pbdagcon_amd import capi
    tlens = [len(bb) for bb, _ in targets]
    hw = capi.HostWindows.tiled(tlens, W, O)
    tiles = [(g,) + t for g, tl in enumerate(tlens) for t in wt.tiled(tl, W, O)]
    lo = [t[3] - t[1] for t in tiles]
    hi = [t[4] - t[1] for t in tiles]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
    try:
        c.set_pileup(*OPTS); c.set_site_reads(True); c.set_window_phase(); c.set_hap_consensus(*hap)
        c.consensus_cigar_windows(cb, hw, strict=False)
        sr, ps, wp, tally = c.site_reads(), c.pileup_sites(), c.window_phase(), c.hap_tally()
        c.set_window_keep(lo, hi)
        c.upload_haps(swap=wp["flip"])
        hm = c.hap_map()
        c.run(); c.sync()
        got = c.fetch(strict=False)
        keep = c.window_keep()
    finally:
        c.close()
    first = np.concatenate([[0], np.cumsum([len(wt.tiled(tl, W, O)) for tl in tlens])]).tolist()
    ps_of = lambda w: 1 + tiles[int(wp["block"][w])][3]
    win_lines = []
    for w, (g, begin, end, c0, c1) in enumerate(tiles):
        flip = int(wp["flip"][w])
        win_lines.append(hct.window_line(names[g], c0, c1, ps_of(w), *(int(tally[k][w]) for k in ("n1", "n2", "n0", "n_sep", "agree", "disagree", "split")), flip))
        for s in range(int(ps["site_begin"][w]), int(ps["site_begin"][w + 1])):
            p = int(ps["pos"][s])
            if sr["phase"][s] and lo[w] <= p < hi[w]:
                win_lines.append(hct.site_line(names[g], p + begin + 1, int(sr["phase"][s]), *(int(x) for x in tally["site_counts"][s]), flip))
    fasta, contigs = [], []
    seg = 0
    per = {}
    for d, segs in enumerate(got):
        w, L = int(hm["src_target"][d]), int(hm["label"][d])
        g = tiles[w][0]
        krecs = []
        for _, _, seq in segs:
            krecs.append((seq, tuple(int(keep[k][seg]) for k in ("i0", "i1", "p_first", "p_last"))))
            seg += 1
        per.setdefault((g, L), []).append((w - first[g], tiles[w][1], int(wp["block"][w]), krecs))
    for g in range(len(targets)):
        recs = []
        for L in (1, 2):
            for t0, t1, seq, block in hct.contigs(per.get((g, L), []), min_len):
                recs.append((t0, L, hct.contig_record(names[g], L, 1 + tiles[block][3], t0, t1, seq)))
                contigs.append((g, L, 1 + tiles[block][3], t0, t1, seq))
        fasta += hct.order_records(recs)
    return "".join(fasta), "".join(x + "\n" for x in win_lines), contigs, dict(wp=wp, tally=tally, tiles=tiles)


def _cli_run(tmp_path, tag, base, extra, inp):
    fc, fw = tmp_path / ("c_" + tag), tmp_path / ("w_" + tag)
    r = subprocess.run(base + ["--phase-windows", "--hap-contigs", str(fc), "--hap-windows", str(fw), *extra, str(inp)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout, fc.read_text(), fw.read_text()


def _bam(names, tlens, targets):
    records = [dict(qname="q%d_%d" % (g, k), flag=0, ref=g, pos=p, ops=[int(x) for x in oo], seq=bytes(q)) for g, recs in enumerate(targets) for k, (p, q, oo) in enumerate(recs)]
    return bf.bgzf(bf.bam_bytes(list(zip(names, tlens)), records))


@pytest.mark.gpu
def test_pbdagcon_hap_contigs_and_hap_windows(oracle_lib, tmp_path):
    """The planted SAM at --window 150 --overlap 70 (the command line refuses an overlap below --trim + 64, so 30 is not
    to be had there; the API tests above run at 30)."""
    twp = _twp()
    bb, recs, groups = twp._planted_records()
    _, alns, subs, ins_at, _ = twp._tsr()._planted()
    name, W, O = "ctg", 150, 70
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta([name], [bb]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam([name], [600], [recs]))
    bam = tmp_path / "in.bam"; bam.write_bytes(_bam([name], [600], [recs]))
    fasta, windows, contigs, api = _api_files([(bb, recs)], [name], W, O, 6, 30, 5)
    assert api["tally"]["split"].tolist() == [1] * 4 and set(api["wp"]["flip"].tolist()) == {0, 1} and api["wp"]["block"].tolist() == [0] * 4
    # two contigs, each spanning the target (but for the trimmed ends), each its haplotype's sequence and nothing of the other's
    assert [(c[1], c[2]) for c in contigs] == [(1, 1), (2, 1)] and all(c[3] <= 10 and c[4] >= 590 for c in contigs)
    # (the second haplotype: what most of its twelve reads say, column by column; 601 columns, the inserted base at ins_at)
    cols = np.array([np.frombuffer(q, np.uint8) for _, q, _ in alns[12:]])
    second = bytes(int(np.bincount(cols[:, j]).argmax()) for j in range(601))
    assert sum(second[p + (p >= ins_at)] != bb[p] for p in subs) == len(subs) >= 10
    (_, _, _, a0, a1, s1), (_, _, _, b0, b1, s2) = contigs
    assert s1 == bytes(bb[a0:a1])
    assert s2 == second[b0:b1 + 1] and b0 < ins_at < b1 and s1 != s2
    assert windows.count("#window") == 4 and len(windows.splitlines()) > 4 + len(subs) // 2
    base = [_cli(), "-c", "6", "-m", "30", "-t", "5", "--ref", str(ref), "--window", str(W), "--overlap", str(O)]
    plain = subprocess.run(base + ["--sam", str(sam)], capture_output=True, timeout=300)
    assert plain.returncode == 0 and plain.stdout.count(b">") >= 1
    for tag, kind, extra, inp in (("b1", "--sam", ["--batch-targets", "1"], sam), ("b2", "--sam", ["--batch-targets", "2"], sam),
                                  ("b4", "--sam", ["--batch-targets", "4"], sam), ("bam", "--bam", ["--batch-targets", "3"], bam)):
        out, fc, fw = _cli_run(tmp_path, tag, base + [kind], extra, inp)
        assert out == plain.stdout, tag                               # stdout is what it is without the two flags
        assert fc == fasta and fw == windows, tag
    # beside the files of --phase-windows: those do not change either
    fh = tmp_path / "tags"
    only = subprocess.run(base + ["--sam", "--phase-windows", "--haplotag", str(fh), str(sam)], capture_output=True, timeout=300)
    tags = fh.read_text()
    both = subprocess.run(base + ["--sam", "--phase-windows", "--haplotag", str(fh), "--hap-contigs", str(tmp_path / "c_x"), "--batch-targets", "2", str(sam)], capture_output=True, timeout=300)
    assert only.returncode == 0 and both.returncode == 0 and fh.read_text() == tags and (tmp_path / "c_x").read_text() == fasta and both.stdout == plain.stdout


@pytest.mark.gpu
def test_breaks_end_both_contigs(oracle_lib, tmp_path):
    """The input of test_window_phase.test_natural_breaks through the command line (the non-conforming record moved to
    where only window 2 runs at this overlap): a failed window, a window below min_cov and a target without a site break
    the blocks and end both contigs; so does a window in the middle whose reads do not split."""
    twp = _twp()
    bb, recs, groups = twp._planted_records()
    _, alns, _, _, _ = twp._tsr()._planted()
    bad = (372, bb[371:378], [ct.op("M", 8)])                       # 8 columns, 7 read bases, over [371, 379): the run of window 2 alone at this overlap
    assert not ct.conforming(bad[0], len(bad[1]), 600, bad[2])
    short = [ct.compress(*(a if k in (0, 12) else twp._cut(a, 0, 400)), bb) for k, a in enumerate(alns)]
    one_hap = [ct.compress(*a, bb) for a in alns[:12]]
    # a window in the middle whose reads do not split: every read of the second haplotype ends at base 300 or begins at 450
    middle = [ct.compress(*a, bb) for a in alns[:12]] + [ct.compress(*twp._cut(a, 0, 300), bb) for a in alns[12:]] + [ct.compress(*twp._cut(a, 450, 600), bb) for a in alns[12:]]
    names = ["planted", "failed", "short", "one_hap", "middle"]
    targets = [(bb, recs), (bb, recs + [bad]), (bb, short), (bb, one_hap), (bb, middle)]
    W, O = 150, 70
    fasta, windows, contigs, api = _api_files(targets, names, W, O, 6, 100, 5)
    split = api["tally"]["split"].reshape(5, 4).tolist()
    block = api["wp"]["block"].reshape(5, 4).tolist()
    assert split == [[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0], [0, 0, 0, 0], [1, 1, 0, 1]]
    assert block == [[0, 0, 0, 0], [4, 4, 6, 7], [8, 8, 8, 11], [12, 13, 14, 15], [16, 16, 18, 19]]
    by = {}
    for g, L, ps, t0, t1, seq in contigs:
        by.setdefault((g, L), []).append((ps, t0, t1))
    assert [len(by[(0, L)]) for L in (1, 2)] == [1, 1] and (3, 1) not in by and (3, 2) not in by
    # the failed window ends both contigs, and PS changes there: the blocks break at it
    for L in (1, 2):
        assert len(by[(1, L)]) >= 2 and len({x[0] for x in by[(1, L)]}) >= 2 and all(not (x[1] < 300 and x[2] > 450) for x in by[(1, L)])
    # the unsplit window in the middle ends both contigs: none crosses [300, 450)
    for L in (1, 2):
        if (4, L) in by:
            assert all(not (x[1] < 300 and x[2] > 450) for x in by[(4, L)])
    assert (4, 1) in by and len(by[(4, 1)]) >= 2
    if block[4][3] == block[4][0]:
        assert len({x[0] for x in by[(4, 1)]}) == 1                  # PS changes only at a block break
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb] * 5))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, [600] * 5, [r for _, r in targets]))
    base = [_cli(), "-c", "6", "-m", "100", "-t", "5", "--ref", str(ref), "--window", str(W), "--overlap", str(O), "--sam"]
    plain = subprocess.run(base + [str(sam)], capture_output=True, timeout=300)
    assert plain.returncode == 0
    for tag, extra in (("all", []), ("b3", ["--batch-targets", "3"])):
        out, fc, fw = _cli_run(tmp_path, tag, base, extra, sam)
        assert out == plain.stdout and fc == fasta and fw == windows, tag
