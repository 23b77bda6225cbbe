"""The sites the same reads carry (dagcon_set_site_link, pbdagcon --link-sites / --linked-sites): the rule by hand, the
motivation and the twin's invariants on the CPU, the device against the twin by equality on the GPU.  include/dagcon.h,
rule 13, states the rule; site_link_twin.py is it in Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cigar_twin as ct
import site_link_twin as slt
import site_reads_twin as srt
import window_twin as wt
from util import batch_from_targets
from test_site_reads import _planted, _piles, _code, _tes, _tlens, _cli, GAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID, NONCONFORMING = -8, -1, -4
KEYS = ("n1", "n2", "n0", "n_sep", "agree", "disagree", "split")
SITES = (2, 200000)


# ---- pile-ups by hand: a read is its own target string, so a position's classes are the reads' letters there ------------

def _cols(tl, depth, cols, start=None, fill=b"G"):
    """cols: {position: one letter per read}.  start[x]: first position of read x (0-based), it runs to the end."""
    alns = []
    for x in range(depth):
        s = bytearray(fill * tl)
        for p, letters in cols.items():
            s[p] = ord(letters[x])
        s0 = start[x] if start else 0
        alns.append((s0 + 1, bytes(s[s0:]), bytes(s[s0:])))
    return alns


def _pat(depth, minor, third=()):
    """A column: C for the reads of `minor`, T for those of `third`, A for the others."""
    return "".join("C" if x in minor else "T" if x in third else "A" for x in range(depth))


def _link(alns, tl, link, sites=SITES, min_len=4, trim=0):
    tw = slt.target(tl, alns, min_len, trim, sites, link_opts=slt.options(*link))
    return tw, tw["partners"], tw["linked"]


def _planted_batch(n):
    """tools/hap_probe.py's batch: the synthetic 10 kb x 40x targets of seed 1000, every second alignment of a target with
    another base at one position in every 1,000 (plant(every=1000, seed=7), copied from there).  Per target its length,
    its alignments and the planted positions."""
    from pbdagcon_amd import synth
    batch = synth.make_batch(n, 10000, 40, seed=1000)
    rng = np.random.default_rng(7)
    other = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        other[a] = b
    out = []
    for t in range(batch.n_targets):
        tl = int(batch.tlen[t])
        pos = np.array([s + int(rng.integers(0, 1000)) for s in range(0, tl - 1000 + 1, 1000)], np.int64)
        for a in range(int(batch.aln_begin[t]) + 1, int(batch.aln_begin[t + 1]), 2):
            o, ln = int(batch.aln_off[a]), int(batch.aln_len[a])
            tcol = np.flatnonzero(batch.tstr[o:o + ln] != GAP)
            k = pos - (int(batch.aln_start[a]) - 1)
            k = k[(k >= 0) & (k < tcol.size)]
            cols = o + tcol[k]
            cols = cols[batch.qstr[cols] != GAP]
            batch.qstr[cols] = other[batch.tstr[cols]]
        alns = []
        for a in range(int(batch.aln_begin[t]), int(batch.aln_begin[t + 1])):
            o, ln = int(batch.aln_off[a]), int(batch.aln_len[a])
            alns.append((int(batch.aln_start[a]), bytes(batch.qstr[o:o + ln]), bytes(batch.tstr[o:o + ln])))
        out.append((tl, alns, pos.tolist()))
    return batch, out


@pytest.fixture(scope="module")
def planted4(oracle_lib):
    """The four planted targets and their twins, plain and linked: computed once, read by the CPU and the GPU test."""
    batch, targets = _planted_batch(4)
    plain = [slt.target(tl, alns, 500, 50, SITES) for tl, alns, _ in targets]
    linked = [slt.target(tl, alns, 500, 50, SITES, link_opts=slt.options()) for tl, alns, _ in targets]
    return batch, targets, plain, linked


# ---- CPU: the rule by hand --------------------------------------------------------------------------------------------

def test_the_rule_by_hand(oracle_lib):
    one = (0, 0, 1, 0)                                                 # the defaults, but one partner links a site
    # the conflict bound, met exactly: ten reads signed at both sites, one of them on the other side
    a10 = _cols(12, 10, {3: _pat(10, {7, 8, 9}), 8: _pat(10, {6, 7, 8, 9})})
    tw, partners, linked = _link(a10, 12, one)
    assert tw["sites"] == [3, 8]
    P, M = slt.rows(tw["ents"], [tw["counts"][p] for p in tw["sites"]])
    assert (P[0], M[0], P[1], M[1]) == (0x07F, 0x380, 0x03F, 0x3C0)
    assert slt.cells(P[0], M[0], P[1], M[1]) == (6, 3, 1, 0)           # 1 * 1000000 == 100000 * 10
    assert partners == [1, 1] and linked == [1, 1]
    assert _link(a10, 12, (99999, 0, 1, 0))[1] == [0, 0]
    # one more conflicting read: 2 of 11
    a11 = _cols(12, 11, {3: _pat(11, {7, 8, 9, 10}), 8: _pat(11, {6, 7, 8, 9})})
    tw, partners, linked = _link(a11, 12, one)
    P, M = slt.rows(tw["ents"], [tw["counts"][p] for p in tw["sites"]])
    assert slt.cells(P[0], M[0], P[1], M[1]) == (6, 3, 1, 1) and partners == [0, 0] and linked == [0, 0]
    assert _link(a11, 12, (181819, 0, 1, 0))[1] == [1, 1] and _link(a11, 12, (181818, 0, 1, 0))[1] == [0, 0]      # 2 / 11
    # cell == min_cell against min_cell - 1: the smaller of the two agreeing cells is the minor allele's
    same3 = _cols(12, 10, {3: _pat(10, {7, 8, 9}), 8: _pat(10, {7, 8, 9})})
    same2 = _cols(12, 10, {3: _pat(10, {7, 8, 9}), 8: _pat(10, {7, 8}, {9})})
    assert _link(same3, 12, one)[1] == [1, 1] and _link(same2, 12, one)[1] == [0, 0]
    assert _link(same2, 12, (0, 2, 1, 0))[1] == [1, 1] and _link(same3, 12, (0, 4, 1, 0))[1] == [0, 0]
    # partners == min_partners against one fewer: three like sites have two partners each, two have one
    three = _cols(12, 10, {2: _pat(10, {7, 8, 9}), 5: _pat(10, {7, 8, 9}), 9: _pat(10, {7, 8, 9})})
    assert _link(three, 12, (0, 0, 0, 0))[1:] == ([2, 2, 2], [1, 1, 1])
    assert _link(same3, 12, (0, 0, 0, 0))[1:] == ([1, 1], [0, 0])
    assert _link(three, 12, (0, 0, 3, 0))[1:] == ([2, 2, 2], [0, 0, 0])
    # a partner need not be linked itself: the middle site has two partners, the outer ones one each (reach 1)
    assert _link(three, 12, (0, 0, 0, 1))[1:] == ([1, 2, 1], [0, 1, 0])
    # same == diff: half the reads signed at both agree; partners only when the bound allows a half, and then the cell
    # is that of the first pair
    half = _cols(12, 8, {3: _pat(8, {4, 5, 6, 7}), 8: _pat(8, {2, 3, 6, 7})})
    tw, partners, _ = _link(half, 12, one)
    P, M = slt.rows(tw["ents"], [tw["counts"][p] for p in tw["sites"]])
    assert slt.cells(P[0], M[0], P[1], M[1]) == (2, 2, 2, 2) and partners == [0, 0]
    assert _link(half, 12, (499999, 2, 1, 0))[1] == [0, 0] and _link(half, 12, (500000, 2, 1, 0))[1] == [1, 1]
    assert _link(half, 12, (1000000, 3, 1, 0))[1] == [0, 0]
    # same == diff == 0: no read is signed at both sites (reads 0 .. 4 end in front of the second, 5 .. 9 begin behind the
    # first): cell 0, below every min_cell
    apart = [(1, s[:20], t[:20]) for _, s, t in _cols(40, 5, {5: "AACCC"})] + [(21, s[20:], t[20:]) for _, s, t in _cols(40, 5, {30: "AACCC"})]
    tw, partners, _ = _link(apart, 40, (1000000, 1, 1, 0))
    assert tw["sites"] == [5, 30] and partners == [0, 0]
    # an insertion site paired with a base site: reads 6 .. 9 insert a T behind base 4 and read C at base 9
    ins = []
    for x, (s0, q, t) in enumerate(_cols(14, 10, {9: _pat(10, {6, 7, 8, 9})})):
        ins.append((s0, q[:5] + b"T" + q[5:], t[:5] + b"-" + t[5:]) if x >= 6 else (s0, q, t))
    tw, partners, linked = _link(ins, 14, one)
    assert tw["sites"] == [4, 9] and srt.kind(tw["counts"][4]) == ("ins",) and srt.kind(tw["counts"][9])[0] == "base"
    P, M = slt.rows(tw["ents"], [tw["counts"][p] for p in tw["sites"]])
    assert slt.cells(P[0], M[0], P[1], M[1]) == (6, 4, 0, 0) and partners == [1, 1] and linked == [1, 1]
    # a site whose k2 does not exist (thresholds 0 / 0: every position is a site, most with one class): row M is empty,
    # the cell of either pair is 0, it has no partners whatever the options
    tw, partners, linked = _link(same3, 12, (1000000, 1, 1, 0), sites=(0, 0))
    assert tw["sites"] == list(range(12)) and srt.kind(tw["counts"][0]) == ("base", 2, None)
    assert partners == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0] and linked == [int(p > 0) for p in partners]
    # the mute: entries at sites that are not linked are unsigned; the entries themselves stay
    plain = srt.target(12, same2, 4, 0, SITES)
    tw, _, _ = _link(same2, 12, one)
    assert plain["hap"] == [1] * 7 + [2] * 3 and plain["signed"] == [2] * 9 + [1]
    assert tw["ents"] == plain["ents"] and tw["hap"] == [0] * 10 and tw["phase"] == [0, 0] and tw["signed"] == [0] * 10
    assert [tw["tally"][k] for k in KEYS] == [0, 0, 10, 0, 0, 0, 0] and tw["tally"]["site_counts"] == [[0] * 4] * 2
    tw, _, _ = _link(same3, 12, one)
    assert tw["hap"] == [1] * 7 + [2] * 3 and tw["phase"] == [1, 1] and tw["tally"]["site_counts"] == [[7, 0, 0, 3]] * 2
    # the options: a 0 is the default
    assert slt.options() == (100000, 3, 2, 256) and slt.options(1, 0, 5, 0) == (1, 3, 5, 256)


def test_the_motivation_on_the_twins(planted4):
    """Four 10 kb x 40x targets with planted haplotypes at --sites' defaults: the reads' own errors outvote the ten
    planted sites and every read gets label 1; with the link rule at its defaults every read is labelled as planted."""
    batch, targets, plain, linked = planted4
    n_linked = n_planted = 0
    for (tl, alns, pos), off, on in zip(targets, plain, linked):
        assert len(off["src"]) == 40 and off["src"] == list(range(40)) and 300 < len(off["sites"]) < 420
        assert off["hap"] == [1] * 40 and not off["tally"]["split"]
        assert on["sites"] == off["sites"] and on["ents"] == off["ents"]
        parity = [1 + x % 2 for x in on["src"]]
        assert on["hap"] in (parity, [3 - h for h in parity]) and on["tally"]["split"] == 1
        assert (on["tally"]["n1"], on["tally"]["n2"], on["tally"]["n0"]) == (20, 20, 0)
        n_linked += sum(on["linked"])
        n_planted += sum(1 for p, l in zip(on["sites"], on["linked"]) if l and p in pos)
    print("linked sites %d, planted among them %d of %d" % (n_linked, n_planted, sum(len(p) for _, _, p in targets)))
    assert n_planted >= 30 and n_linked - n_planted <= 10


# ---- CPU: the twin's invariants, and three wrong versions of the rule ----------------------------------------------------

def _sets(ents, counts):
    """Per site the sets of alignments with M = +1 and M = -1: the rows without bit arithmetic."""
    P, M = [set() for _ in counts], [set() for _ in counts]
    for x, e in enumerate(ents):
        for k, code in e:
            m = srt.sign(code, counts[k])
            if m:
                (P if m > 0 else M)[k].add(x)
    return P, M


def test_twin_invariants_on_random_small_pileups(oracle_lib):
    tes = _tes()
    rng = np.random.default_rng(1301)
    n_partner = n_linked = n_muted = 0
    for k in range(300):
        alns, bb = tes._small_pileup(rng, k)
        sites = (0, 0) if k % 2 else SITES
        opts = slt.options(int(rng.choice([50000, 100000, 300000, 1000000])), 1 + k % 3, 1 + k % 2, int(rng.choice([1, 2, 3, 256])))
        tw = slt.target(len(bb), alns, 4, int(rng.integers(0, 3)), sites, link_opts=opts)
        sc = [tw["counts"][p] for p in tw["sites"]]
        n = len(sc)
        P, M = slt.rows(tw["ents"], sc)
        rel = [[i != j and abs(i - j) <= opts[3] and slt.pair(P[i], M[i], P[j], M[j], opts) for j in range(n)] for i in range(n)]
        assert all(rel[i][j] == rel[j][i] for i in range(n) for j in range(n))                  # symmetric
        assert tw["partners"] == [sum(r) for r in rel]
        assert all(tw["partners"][i] <= min(n - 1, i + opts[3]) - max(0, i - opts[3]) for i in range(n))
        assert tw["linked"] == [int(p >= opts[2]) for p in tw["partners"]]
        # muting only ever turns signs to 0: against the plain split's signs, entry by entry
        plain = srt.target(len(bb), alns, 4, 0, sites)
        for e in tw["ents"]:
            for s, code in e:
                m = srt.sign(code, sc[s])
                assert (m if tw["linked"][s] else 0) in (0, m)
        assert all(a <= b for a, b in zip(tw["signed"], [sum(1 for s, c in e if srt.sign(c, sc[s])) for e in tw["ents"]]))
        assert all(not sg for sg, l in zip(tw["phase"], tw["linked"]) if not l)
        assert all(c == [0, 0, 0, 0] for c, l in zip(tw["tally"]["site_counts"], tw["linked"]) if not l)
        # the loosest options: linked iff a site within reach shares a signed read in both cells of the larger pair
        loose = slt.options(1000000, 1, 1, opts[3])
        _, linked = slt.link(tw["ents"], sc, loose)
        Ps, Ms = _sets(tw["ents"], sc)
        for i in range(n):
            want = False
            for j in range(max(0, i - loose[3]), min(n, i + loose[3] + 1)):
                if j == i:
                    continue
                pp, mm, pm, mp = len(Ps[i] & Ps[j]), len(Ms[i] & Ms[j]), len(Ps[i] & Ms[j]), len(Ms[i] & Ps[j])
                a, b = (pp, mm) if pp + mm >= pm + mp else (pm, mp)
                want = want or (a >= 1 and b >= 1)
            assert linked[i] == int(want)
        n_partner += sum(tw["partners"]); n_linked += sum(tw["linked"]); n_muted += sum(1 for l in tw["linked"] if not l)
        del plain
    print("partners %d, linked %d, muted %d" % (n_partner, n_linked, n_muted))
    assert n_partner > 300 and n_linked > 100 and n_muted > 1000


def _variant(per_target, opts, across=False, by_position=False, wrong_cell=False):
    """The rule written again with one of three mistakes in it.  per_target: [(sites, ents, counts)]."""
    def is_pair(Pi, Mi, Pj, Mj):
        pp, mm, pm, mp = slt.cells(Pi, Mi, Pj, Mj)
        same, diff = pp + mm, pm + mp
        lo, hi = min(same, diff), max(same, diff)
        cell = (min(pm, mp) if same >= diff else min(pp, mm)) if wrong_cell else (min(pp, mm) if same >= diff else min(pm, mp))
        return lo * 1000000 <= opts[0] * (lo + hi) and cell >= opts[1]
    rows, where, tgt = [], [], []
    for t, (sites, ents, counts) in enumerate(per_target):
        P, M = slt.rows(ents, counts)
        rows += list(zip(P, M)); where += list(sites); tgt += [t] * len(sites)
    n = len(rows)
    idx = [i - tgt.index(tgt[i]) for i in range(n)]
    partners = [0] * n
    for i in range(n):
        for j in range(n):
            if i == j or (tgt[i] != tgt[j] and not across):
                continue
            d = abs(where[i] - where[j]) if by_position and tgt[i] == tgt[j] else abs((i - j) if across else (idx[i] - idx[j]))
            if d <= opts[3] and is_pair(*rows[i], *rows[j]):
                partners[i] += 1
    return partners


def test_three_wrong_versions_are_rejected(oracle_lib):
    opts = slt.options(0, 0, 1, 1)
    col = _pat(10, {7, 8, 9})
    # partners counted across a target boundary: two targets, the last site of one and the first of the next alike
    two = [_cols(12, 10, {11: col}), _cols(12, 10, {0: col})]
    tws = [slt.target(12, a, 4, 0, SITES, link_opts=opts) for a in two]
    per = [(tw["sites"], tw["ents"], [tw["counts"][p] for p in tw["sites"]]) for tw in tws]
    assert [tw["sites"] for tw in tws] == [[11], [0]] and [tw["partners"] for tw in tws] == [[0], [0]]
    assert _variant(per, opts) == [0, 0] and _variant(per, opts, across=True) == [1, 1]
    # reach measured in positions: sites at 2, 5, 9 with reach 1 -- the neighbours in the site list are compared
    three = _cols(12, 10, {2: col, 5: col, 9: col})
    tw = slt.target(12, three, 4, 0, SITES, link_opts=opts)
    per = [(tw["sites"], tw["ents"], [tw["counts"][p] for p in tw["sites"]])]
    assert tw["partners"] == [1, 2, 1] == _variant(per, opts) and _variant(per, opts, by_position=True) == [0, 0, 0]
    wide = slt.options(0, 0, 1, 4)
    assert slt.link(per[0][1], per[0][2], wide)[0] == [2, 2, 2] and _variant(per, wide, by_position=True) == [1, 2, 1]
    # the cell taken from the other pair: two like sites have pp 7, mm 3, pm 0, mp 0
    assert _variant(per, opts, wrong_cell=True) == [0, 0, 0]
    half = _cols(12, 8, {3: _pat(8, {4, 5, 6, 7}), 8: _pat(8, {1, 2, 3, 7})})                    # pp 1, mm 1, pm 3, mp 3
    tw = slt.target(12, half, 4, 0, SITES, link_opts=slt.options(300000, 2, 1, 1))
    per = [(tw["sites"], tw["ents"], [tw["counts"][p] for p in tw["sites"]])]
    assert tw["partners"] == [1, 1] and _variant(per, slt.options(300000, 2, 1, 1), wrong_cell=True) == [0, 0]


def test_binding_exports_and_struct_sizes():
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in ("dagcon_set_site_link", "dagcon_fetch_site_link"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(capi.SiteLinkOpts) == 16 and ctypes.sizeof(capi.SiteLink) == 24
    assert [f[0] for f in capi.SiteLinkOpts._fields_] == ["max_conflict_ppm", "min_cell", "min_partners", "reach"]
    assert [f[0] for f in capi.SiteLink._fields_] == ["n_sites", "partners", "linked"]


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _expect(strings, tlens, min_cov, min_len, trim, sites, rounds, link, hap, status, n_given=None, src=None):
    """The arrays the twin expects, as test_site_reads._expect builds them, with partners, linked and the tally.
    link None: the switch off."""
    out = {k: [] for k in ("aln_tgt", "aln_src", "ent_site", "ent_code", "hap", "phase", "pos", "partners", "linked", "site_counts") + KEYS}
    out["ent_begin"], out["site_begin"] = [0], [0]
    base = 0
    for t, (s, tl) in enumerate(zip(strings, tlens)):
        n_al = 0 if s is None else len(s[1])
        if s is not None and not status[t] and n_al >= max(1, min_cov):
            tw = slt.target(tl, s[1], min_len, trim, sites, rounds or srt.ROUNDS, None if link is None else slt.options(*link), hap, min_cov)
            sb = len(out["pos"])
            for i, e, h in zip(tw["src"], tw["ents"], tw["hap"]):
                out["aln_tgt"].append(t); out["aln_src"].append(src[t][i] if src is not None else base + i); out["hap"].append(h)
                out["ent_site"] += [sb + k for k, _ in e]; out["ent_code"] += [c for _, c in e]
                out["ent_begin"].append(len(out["ent_site"]))
            out["pos"] += tw["sites"]; out["phase"] += tw["phase"]
            if link is not None:
                out["partners"] += tw["partners"]; out["linked"] += tw["linked"]
            out["site_counts"] += tw["tally"]["site_counts"]
            for k in KEYS:
                out[k].append(tw["tally"][k])
        else:
            for k in KEYS:
                out[k].append(0)
        out["site_begin"].append(len(out["pos"]))
        base += n_given[t] if n_given is not None else n_al
    return out


def _fetch_all(c, link):
    d = {"sr": c.site_reads(), "ps": c.pileup_sites(), "pu": c.pileup(), "tally": c.hap_tally(), "status": c.target_status.tolist(),
         "reruns": c.timings()["reruns"]}
    if link is not None:
        d["sl"] = c.site_link()
        again = c.site_link()
        assert all(np.array_equal(d["sl"][k], again[k]) for k in again)
    return d


def _link_run(call, strings, tlens, min_cov, min_len, trim, sites=SITES, link=(0, 0, 0, 0), hap=(0, 0), rounds=0, prepare=None, n_given=None, src=None):
    """One context with the pile-up, the split, the tally and the link on; every array against the twin by equality."""
    from pbdagcon_amd import capi
    c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim)
    try:
        if prepare:
            prepare(c)
        c.set_pileup(*sites)
        c.set_site_reads(True, rounds)
        c.set_hap_consensus(*hap)
        if link is not None:
            c.set_site_link(*link)
        got = call(c)
        d = _fetch_all(c, link)
    finally:
        c.close()
    exp = _expect(strings, tlens, min_cov, min_len, trim, sites, rounds, link, hap, d["status"], n_given, src)
    sr, ps = d["sr"], d["ps"]
    assert ps["site_begin"].tolist() == exp["site_begin"] and ps["pos"].tolist() == exp["pos"]
    for k in ("aln_tgt", "aln_src", "ent_begin", "ent_site", "ent_code", "hap", "phase"):
        assert sr[k].tolist() == exp[k], k
    if link is not None:
        assert d["sl"]["partners"].dtype == np.uint16 and d["sl"]["linked"].dtype == np.uint8
        assert d["sl"]["partners"].tolist() == exp["partners"] and d["sl"]["linked"].tolist() == exp["linked"]
    for k in KEYS:
        assert d["tally"][k].tolist() == exp[k], (k, d["tally"][k].tolist(), exp[k])
    assert d["tally"]["site_counts"].tolist() == exp["site_counts"]
    d["got"], d["exp"] = got, exp
    return d


def _strings_call(strings, tlens):
    batch = batch_from_targets([(tl, alns, None) for tl, (_, alns) in zip(tlens, strings)])
    return lambda c: c.consensus(batch, strict=False)


def _deep(n):
    """40 bases under n reads: at positions 5, 17 and 29 the reads 60 .. 70 (those there are; of fewer than 61 reads the
    later half) read C, the others A."""
    minor = set(range(60, 71)) & set(range(n)) if n > 60 else set(range(n - n // 2, n))
    return (b"N" * 40, _cols(40, n, {p: _pat(n, minor) for p in (5, 17, 29)}))


@pytest.mark.gpu
def test_row_word_edges(oracle_lib):
    """Targets of 1, 2, 63, 64, 65, 128 and 129 alignments in one batch: rows of one, two and three words side by side,
    and the one width of the batch.  In the deep ones the minor allele is carried by alignments 60 .. 70, four in the
    first word and the rest in the second, and min_cell is the number of them: a count that misses a word misses the bound."""
    depths = [1, 2, 63, 64, 65, 128, 129]
    strings = [_deep(n) for n in depths]
    tlens = [40] * len(depths)
    # on the twin first
    for n, (_, alns) in zip(depths, strings):
        carried = len(set(range(60, 71)) & set(range(n))) if n > 60 else n // 2
        for cell, want in ((carried, 1), (carried + 1, 0)):
            tw = slt.target(40, alns, 30, 0, (1, 0), link_opts=slt.options(0, cell, 0, 0))
            if n == 1:
                assert tw["sites"] == []
                continue
            assert tw["sites"] == [5, 17, 29] and tw["partners"] == [2 * want] * 3 and tw["linked"] == [want] * 3, (n, cell)
            assert (tw["hap"].count(2) == carried) == bool(want) and (tw["hap"] == [0] * n) == (not want)
    assert [len(set(range(60, 71)) & set(range(n))) for n in (63, 64, 65, 128, 129)] == [3, 4, 5, 11, 11]
    call = _strings_call(strings, tlens)
    r = _link_run(call, strings, tlens, 1, 30, 0, (1, 0), (0, 11, 0, 0), hap=(1, 1))
    assert r["sl"]["linked"].tolist() == [0] * 12 + [1] * 6 and r["status"] == [0] * 7
    r = _link_run(call, strings, tlens, 1, 30, 0, (1, 0), (0, 12, 0, 0), hap=(1, 1))
    assert not r["sl"]["linked"].any() and not r["sr"]["hap"].any()
    r = _link_run(call, strings, tlens, 1, 30, 0, (1, 0), (0, 1, 0, 0), hap=(1, 1))
    assert r["sl"]["linked"].all() and r["tally"]["split"].tolist() == [0, 1, 1, 1, 1, 1, 1]
    # a batch whose deepest target has 2 alignments: the one-word width, with the 1-alignment target in it
    r = _link_run(_strings_call(strings[:2], tlens[:2]), strings[:2], tlens[:2], 1, 30, 0, (1, 0), (0, 1, 0, 0), hap=(1, 1))
    assert r["sl"]["partners"].tolist() == [2, 2, 2]


def _reach_target(reach):
    """Ten reads, three real sites (reads 5 .. 9 read C) at indices 0, reach and 2 * reach + 1 of the site list; every
    position between them is a site of reads 0 and 5 alone, which is nobody's partner: half of its signed reads disagree
    with a real site, and its own cell is 2."""
    n = 2 * reach + 2
    real = {0, reach, 2 * reach + 1}
    cols = {3 + k: _pat(10, set(range(5, 10)) if k in real else {0, 5}) for k in range(n)}
    return (b"N" * (n + 40), _cols(n + 40, 10, cols)), n


@pytest.mark.gpu
@pytest.mark.parametrize("reach", [1, 2, 63, 64, 65])
def test_reach_edges(oracle_lib, reach):
    (bb, alns), n = _reach_target(reach)
    tl = len(bb)
    tw = slt.target(tl, alns, 30, 0, SITES, link_opts=slt.options(0, 0, 1, reach))
    assert tw["sites"] == list(range(3, 3 + n))
    want = [0] * n
    want[0] = want[reach] = 1                                          # index distance reach: partners; reach + 1: not compared
    assert tw["partners"] == want and tw["linked"] == want
    more = slt.target(tl, alns, 30, 0, SITES, link_opts=slt.options(0, 0, 1, reach + 1))
    assert [k for k, p in enumerate(more["partners"]) if p] == [0, reach, 2 * reach + 1] and more["partners"][reach] == 2
    r = _link_run(_strings_call([(bb, alns)], [tl]), [(bb, alns)], [tl], 3, 30, 0, SITES, (0, 0, 1, reach))
    assert r["sl"]["partners"].tolist() == want
    r = _link_run(_strings_call([(bb, alns)], [tl]), [(bb, alns)], [tl], 3, 30, 0, SITES, (0, 0, 1, reach + 1))
    assert r["sl"]["partners"].tolist() == more["partners"]


@pytest.mark.gpu
def test_clipped_candidate_ranges(oracle_lib):
    """700 bases at thresholds 0 / 0, every position a site that splits the six reads three to three: every site is every
    other's partner, so partners[k] is the number of its candidates at the default reach of 256."""
    strings = [_piles(700, 700)]
    tw = slt.target(700, strings[0][1], 30, 0, (0, 0), link_opts=slt.options())
    want = [min(699, k + 256) - max(0, k - 256) for k in range(700)]
    assert tw["partners"] == want and [want[k] for k in (0, 255, 256, 257, 443, 444, 699)] == [256, 511, 512, 512, 512, 511, 256]
    r = _link_run(_strings_call(strings, [700]), strings, [700], 3, 30, 0, (0, 0))
    assert r["sl"]["partners"].tolist() == want and r["sl"]["linked"].all() and r["sr"]["hap"].tolist() == [1, 1, 1, 2, 2, 2]
    assert r["reruns"] >= 1                                            # (4,200 entries in an arena of 4,161: the arenas grew on the way)


@pytest.mark.gpu
def test_target_boundaries(oracle_lib):
    """Neighbouring targets whose last and first sites show the same reads: partners if targets were not kept apart.  With
    them a target without sites, one with a single site and one below min_cov."""
    col = _pat(10, {7, 8, 9})
    strings = [(b"N" * 12, alns) for alns in (_cols(12, 10, {11: col}), _cols(12, 10, {0: col}), _cols(12, 10, {}), _cols(12, 10, {6: col}),
                                              _cols(12, 2, {3: "CC"}), _cols(12, 10, {2: col, 9: col}), _cols(12, 10, {0: col, 11: col}),
                                              _cols(12, 10, {0: col, 5: col}))]
    link = (0, 0, 1, 0)
    tws = [slt.target(12, a, 4, 0, SITES, link_opts=slt.options(*link)) for _, a in strings]
    assert [tw["sites"] for tw in tws] == [[11], [0], [], [6], [], [2, 9], [0, 11], [0, 5]]
    assert [tw["partners"] for tw in tws] == [[0], [0], [], [0], [], [1, 1], [1, 1], [1, 1]]
    r = _link_run(_strings_call(strings, [12] * 8), strings, [12] * 8, 3, 4, 0, SITES, link)
    assert r["status"] == [0] * 8
    assert r["sl"]["partners"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1] and r["ps"]["site_begin"].tolist() == [0, 1, 2, 2, 3, 3, 5, 7, 9]


@pytest.mark.gpu
@pytest.mark.parametrize("sites", [(0, 0), SITES])
def test_random_small_targets_with_a_failed_one(oracle_lib, sites):
    """100 small targets in one batch, one with a non-conforming record between two good ones: none of its sites in the
    arrays, the others intact."""
    tes = _tes()
    rng = np.random.default_rng(300)
    targets = []
    for k in range(100):
        alns, bb = tes._small_pileup(rng, k)
        targets.append((bb, tes._records(bb, alns, eqx=True)))
    bad = 50
    p, q, o = targets[bad][1][1]
    targets[bad][1][1] = (len(targets[bad][0]) + 1, q, o)
    strings = tes._strings(targets)
    assert strings[bad] is None and strings[bad - 1] is not None and strings[bad + 1] is not None
    link = (300000, 1, 1, 3)
    tws = [slt.target(len(s[0]), s[1], 4, 0, sites, link_opts=slt.options(*link)) for s in strings if s is not None and len(s[1]) >= 3]
    n_linked, n_sites = sum(sum(tw["linked"]) for tw in tws), sum(len(tw["linked"]) for tw in tws)
    print("linked %d of %d sites" % (n_linked, n_sites))
    assert n_linked > 50 and n_sites - n_linked > 50                   # on the twin first
    r = _link_run(tes._whole(targets), strings, _tlens(targets), 3, 4, 0, sites, link, hap=(1, 1), n_given=[len(x) for _, x in targets])
    assert r["status"][bad] == NONCONFORMING and sum(1 for s in r["status"] if s) == 1
    assert int(r["ps"]["site_begin"][bad]) == int(r["ps"]["site_begin"][bad + 1]) and r["sl"]["linked"].sum() == n_linked


def _ways_in():
    from test_hap_consensus import _ways_in as ways
    return ways()


LOOSE = (200000, 2, 1, 0)          # for the small noisy targets of the other tests: ten reads deep, variants of a few reads


@pytest.mark.gpu
def test_every_way_in_gives_the_same_arrays(oracle_lib):
    targets, strings, calls = _ways_in()
    tlens = _tlens(targets)
    tws = [slt.target(tl, a, 30, 5, SITES, link_opts=slt.options(*LOOSE)) for tl, (_, a) in zip(tlens, strings)]
    n_linked, n_sites = sum(sum(tw["linked"]) for tw in tws), sum(len(tw["linked"]) for tw in tws)
    plain = [srt.target(tl, a, 30, 5, SITES) for tl, (_, a) in zip(tlens, strings)]
    print("linked %d of %d sites" % (n_linked, n_sites))
    assert 10 <= n_linked < n_sites - 10 and any(a["hap"] != b["hap"] for a, b in zip(tws, plain))      # on the twin first
    ref = None
    for kind, call in calls.items():
        r = _link_run(call, strings, tlens, 3, 30, 5, SITES, LOOSE)
        assert r["status"] == [0] * 12, kind
        if ref is None:
            ref = r
        assert r["got"] == ref["got"] and all(np.array_equal(r["sl"][k], ref["sl"][k]) for k in ref["sl"]), kind


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
                if rng.random() < 0.01:
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
    tws = [slt.target(tl, a, 100, 10, SITES, link_opts=slt.options()) for tl, (_, a) in zip(tlens, strings)]
    assert all(sum(tw["linked"]) >= 4 and tw["tally"]["split"] for tw in tws)
    r = _link_run(lambda c: c.consensus_pre(targets), strings, tlens, 3, 100, 10)
    assert r["tally"]["split"].tolist() == [1, 1] and r["sr"]["aln_src"].max() == 19


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
    tws = [slt.target(tl, a, 30, 5, SITES, link_opts=slt.options(*LOOSE)) for tl, (_, a) in zip(tlens, strings)]
    assert sum(sum(tw["linked"]) for tw in tws) >= 6 and sum(1 for tw in tws for l in tw["linked"] if not l) >= 6
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    _link_run(lambda c: c.consensus_cigar_windows(cb, hw), strings, tlens, 3, 30, 5, SITES, LOOSE, hap=(1, 1), src=src)


@pytest.mark.gpu
def test_under_the_record_filter_aln_src_is_unchanged(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(13, 10, 150, 300)
    depth = 7
    probe = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        probe.set_record_filter(max_depth=depth)
        probe.set_pileup(*SITES); probe.set_site_reads(True)
        probe.consensus_cigar(capi.HostCigarBatch(**ct.records_to_arrays(targets)))
        fate = probe.record_stats()["fate"]
        src_off = probe.site_reads()["aln_src"]
    finally:
        probe.close()
    assert (fate & capi.FATE_MAX_DEPTH).any()
    kept, src, i = [], [], 0
    for bb, recs in targets:
        kept.append((bb, [r for k, r in enumerate(recs) if not fate[i + k]]))
        src.append([i + k for k in range(len(recs)) if not fate[i + k]])
        i += len(recs)
    strings = tes._strings(kept)
    r = _link_run(tes._whole(targets), strings, _tlens(targets), 3, 30, 5, SITES, LOOSE, hap=(1, 2), prepare=lambda c: c.set_record_filter(max_depth=depth), src=src)
    assert np.array_equal(r["sr"]["aln_src"], src_off) and r["sl"]["linked"].any()


@pytest.mark.gpu
def test_arena_growth_a_second_run_and_poisoned_buffers(oracle_lib, monkeypatch):
    """At 0 / 0 the site and entry arenas are outgrown and the batch runs again: the rows are cleared and nothing is
    counted twice.  A second dagcon_run on the same upload gives the same bytes; so does a context whose buffers are
    filled with 0xEE before every run."""
    from pbdagcon_amd import capi
    tes = _tes()
    ((bb, alns),) = tes._strings(tes._variant_targets(5, 1, 1400, 1400, full_span=True))
    second = _piles(5, 40)
    strings, tlens = [(bb, alns), second, (b"N" * 50, _piles(3, 50)[1][:2])], [1400, 40, 50]     # (the last: below min_cov)
    assert sum(tlens) // 8 + 1024 < 1400 - 10 and sum(len(q) for _, q, _ in alns) // 64 + 4096 < len(alns) * 1380      # both arenas are outgrown
    link = LOOSE
    tw = slt.target(1400, alns, 30, 5, (0, 0), link_opts=slt.options(*link))
    print("linked %d of %d, most partners %d" % (sum(tw["linked"]), len(tw["linked"]), max(tw["partners"])))
    assert 5 < sum(tw["linked"]) < len(tw["linked"]) - 100 and max(tw["partners"]) > 2
    r = _link_run(_strings_call(strings, tlens), strings, tlens, 3, 30, 5, (0, 0), link)
    assert r["reruns"] >= 1
    batch = batch_from_targets([(tl, a, None) for tl, (_, a) in zip(tlens, strings)])
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        c.set_pileup(0, 0); c.set_site_reads(True); c.set_hap_consensus(); c.set_site_link(*link)
        c.upload(batch); c.run(); c.sync(); c.fetch()
        one = _fetch_all(c, link)
        c.run(); c.sync(); c.fetch()
        two = _fetch_all(c, link)
    finally:
        c.close()
    for k in ("sl", "sr", "tally", "ps"):
        assert all(np.array_equal(one[k][f], two[k][f]) for f in one[k]), k
        assert all(np.array_equal(one[k][f], r[k][f]) for f in one[k]), k
    monkeypatch.setenv("DAGCON_POISON", "15")
    p = _link_run(_strings_call(strings, tlens), strings, tlens, 3, 30, 5, (0, 0), link)
    assert all(np.array_equal(p["sl"][f], r["sl"][f]) for f in r["sl"])


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 4, 150, 200)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    c = capi.Context(min_cov=3, min_len=30, trim=5)
    try:
        assert _code(c.site_link) == STATE                           # nothing yet
        c.set_site_link(*LOOSE)
        want = c.consensus_cigar(cb)                                 # the switch without the pile-up
        assert _code(c.site_link) == STATE
        c.set_pileup(*SITES)
        assert c.consensus_cigar(cb) == want and _code(c.site_link) == STATE      # without the site reads
        c.set_site_reads(False)
        assert c.consensus_cigar(cb) == want and _code(c.site_link) == STATE      # without phase
        assert c.site_reads()["hap"] is None
        c.set_site_reads(True)
        c.upload_cigar(cb); c.run(); c.sync()
        assert _code(c.site_link) == STATE                           # before a fetch
        assert c.fetch() == want
        sl = c.site_link()
        assert sl["linked"].size == c.pileup_sites()["pos"].size and sl["linked"].any() and not sl["linked"].all()
        with pytest.raises(capi.DagconError) as e:
            c.set_site_link(reach=4097)
        assert e.value.code == INVALID and "4097" in str(e.value)
        assert c.consensus_cigar(cb) == want                         # the switch stayed as it was
        assert all(np.array_equal(c.site_link()[k], sl[k]) for k in sl)
        c.set_site_link(*LOOSE[:3], reach=4096)                      # the largest reach: on these targets every site of a target
        assert c.consensus_cigar(cb) == want and all(np.array_equal(c.site_link()[k], sl[k]) for k in sl)
        muted = c.site_reads()
        c.set_hap_consensus(1, 1)
        c.consensus_cigar(cb)
        c.hap_tally()
        c.upload_haps()                                              # the derived batch has it off
        assert _code(c.site_link) == STATE
        c.run(); c.sync(); c.fetch()
        assert _code(c.site_link) == STATE
        c.set_site_link(None)                                        # off after on
        assert c.consensus_cigar(cb) == want and _code(c.site_link) == STATE
        plain = c.site_reads()
        assert not np.array_equal(plain["phase"], muted["phase"]) and np.array_equal(plain["ent_code"], muted["ent_code"])
        with pytest.raises(capi.DagconError) as e:
            c.site_link()
        assert "dagcon_fetch_site_link without the results of an upload made with dagcon_set_pileup, dagcon_set_site_reads (phase on) and dagcon_set_site_link on" in str(e.value)
    finally:
        c.close()
    for flag in (capi.FLAG_STOP_AFTER_MERGE, capi.FLAG_STOP_AFTER_BUILD):
        stop = capi.Context(min_cov=3, min_len=30, trim=5, flags=flag)
        try:
            stop.set_pileup(*SITES); stop.set_site_reads(True); stop.set_site_link()
            stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
            assert _code(stop.site_link) == STATE
        finally:
            stop.close()


@pytest.mark.gpu
def test_the_switch_changes_nothing_else(oracle_lib):
    """On: the consensus, the edits, the pile-up, the sites, the entries and the alleles (keys and counts) are those of the
    switch off.  Off after on: everything is that of a context that never called it."""
    from pbdagcon_amd import capi
    tes = _tes()
    targets = tes._variant_targets(5, 6, 150, 250)
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))

    def run(mode):
        c = capi.Context(min_cov=3, min_len=30, trim=5, flags=capi.FLAG_BASE_POS)
        try:
            c.set_edits(True); c.set_pileup(*SITES); c.set_site_reads(True); c.set_site_alleles(True); c.set_hap_consensus()
            if mode != "never":
                c.set_site_link(*LOOSE)
            if mode == "off":
                c.set_site_link(None)
            cns, ed = c.consensus_cigar(cb), c.edits()
            # (c_off indexes seq_blob, where the targets lie in the order k_bp_join's waves took their places, which may
            # differ from run to run: it is compared relative to its segment's seq_off)
            ed["c_off"] = ed["c_off"].astype(np.int64) - np.repeat(c._segs[1].astype(np.int64), np.diff(ed["edit_begin"].astype(np.int64)))
            return {"cns": cns, "edits": ed, "pu": c.pileup(), "ps": c.pileup_sites(), "sr": c.site_reads(),
                    "al": c.site_alleles(), "tally": c.hap_tally()}
        finally:
            c.close()
    never, off, on = run("never"), run("off"), run("on")

    def same(a, b, skip=()):
        if isinstance(a, dict):
            return all(same(a[k], b[k]) for k in a if k not in skip)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)
    for k in never:
        assert same(never[k], off[k]), k
    for k in ("cns", "edits", "pu", "ps"):
        assert same(never[k], on[k]), (k, [f for f in never[k] if not same(never[k][f], on[k][f])] if isinstance(never[k], dict) else None)
    assert same(never["sr"], on["sr"], skip=("hap", "phase")) and same(never["al"], on["al"], skip=("hap_count",))
    assert not same(never["sr"], on["sr"])                             # (and the split did change)


@pytest.mark.gpu
def test_the_planted_batch_on_the_device(planted4):
    """Two of the 10 kb x 40x targets: the device's arrays are the twin's.  That the twin's labels are the planted groups
    is test_the_motivation_on_the_twins."""
    batch, targets, plain, linked = planted4
    strings = [(b"N" * tl, alns) for tl, alns, _ in targets[:2]]
    tlens = [tl for tl, _, _ in targets[:2]]
    assert all(tw["tally"]["split"] for tw in linked[:2])
    r = _link_run(_strings_call(strings, tlens), strings, tlens, 6, 500, 50)
    assert r["tally"]["split"].tolist() == [1, 1] and r["tally"]["n0"].tolist() == [0, 0]
    assert r["sl"]["linked"].sum() == sum(sum(tw["linked"]) for tw in linked[:2])
    off = _link_run(_strings_call(strings, tlens), strings, tlens, 6, 500, 50, link=None)
    assert off["sr"]["hap"].tolist() == [1] * 80 and off["tally"]["split"].tolist() == [0, 0]


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    fl, fh = tmp_path / "o.linked", tmp_path / "o.tags"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    tag = ["--haplotag", str(fh)]
    for args in (["--link-sites", str(m5)], ["--linked-sites", str(fl), str(m5)],                  # nothing that splits
                 ["--link-sites", "--site-reads", str(fh), str(m5)], ["--link-sites", "--sites", str(fh), str(m5)],
                 ["--link-sites", "--site-alleles", str(fh), str(m5)],
                 tag + ["--linked-sites", str(m5)],                                                 # no file name: the input is taken for it
                 tag + ["--link-min-cell", "2", str(m5)], tag + ["--link-reach", "9", str(m5)],     # the options without the switch
                 tag + ["--link-max-conflict", "0.2", str(m5)], tag + ["--link-min-partners", "1", str(m5)],
                 tag + ["--link-sites", "--link-reach", "4097", str(m5)], tag + ["--link-sites", "--link-reach", "x", str(m5)],
                 tag + ["--link-sites", "--link-max-conflict", "1.5", str(m5)], tag + ["--link-sites", "--link-max-conflict", "0.1234567", str(m5)],
                 tag + ["--link-sites", "--link-min-cell", str(m5)], tag + ["--link-sites", "--link-min-partners", "-1", str(m5)],
                 rec + ["--window", "200", "--overlap", "120", "--link-sites"] + tag + [str(sam)],  # windows without --phase-windows
                 rec + ["--window", "200", "--overlap", "120", "--linked-sites", str(fl), str(sam)],
                 ["-a", "--link-sites"] + tag + [str(m5)],
                 rec + ["--dump-parsed", "--link-sites"] + tag + [str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not fl.exists() and not fh.exists()
    out = run("--link-sites", str(m5))
    assert b"--link-sites and --linked-sites need --haplotag, --hap-consensus, --hap-sites or --hap-vcf" in out.stderr
    # wherever the split goes, whole targets and phased windows; a file that cannot be written is said before anything runs
    bad = str(tmp_path / "no_such_dir" / "o.txt")
    for args in (["--haplotag", bad, "--link-sites", str(m5)], ["--hap-consensus", bad, "--link-sites", str(m5)], ["--hap-sites", bad, "--link-sites", str(m5)],
                 rec + ["--hap-vcf", bad, "--link-sites", str(sam)], tag + ["--linked-sites", bad, str(m5)],
                 tag + ["--linked-sites", bad, "--link-max-conflict", "0.123456", "--link-min-cell", "1", "--link-min-partners", "3", "--link-reach", "4096", str(m5)],
                 rec + ["--window", "200", "--overlap", "120", "--phase-windows", "--link-sites", "--site-reads", bad, str(sam)],
                 rec + ["--window", "200", "--overlap", "120", "--phase-windows", "--link-sites", "--hap-contigs", bad, str(sam)],
                 rec + ["--window", "200", "--overlap", "120", "--phase-windows", "--hap-windows", str(fh), "--linked-sites", bad, str(sam)]):
        out = run(*args)
        assert out.returncode == 1 and b"cannot write" in out.stderr, (args, out.stderr)
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --contexts N")[1].split(b"\n  --hap-contigs FILE")[0]
    assert b"\n  --link-sites " in text and b"\n  --linked-sites FILE" in text and b"RNAME POS PARTNERS LINKED" in text
    for word in (b"--link-max-conflict", b"default 0.1", b"--link-min-cell", b"default 3", b"--link-min-partners", b"default 2", b"--link-reach", b"default 256",
                 b"at most 4096", b"synthetic reads", b"parity unpinned"):
        assert word in text, word
    usage = h.stdout.split(b"\n")[0]
    assert b"[--hap-windows FILE]] [--link-sites [--link-max-conflict F] [--link-min-cell N] [--link-min-partners N] [--link-reach N]] [--linked-sites FILE] [-v] <input>" in usage


_LINK_MAIN = r"""
#include <iostream>
#include "site_reads.h"
// stdin: "l rname pos0 partners linked" -> the line of --linked-sites | "s code linked n0 .. n7" -> the sign
int main() {
    std::string out, kind, rname;
    while (std::cin >> kind) {
        if (kind == "l") { unsigned long long pos; unsigned p, l; std::cin >> rname >> pos >> p >> l; dg_linked_site_line(out, rname, pos, p, l); }
        else { unsigned code, l, v; uint16_t n[8]; std::cin >> code >> l; for (auto &x : n) { std::cin >> v; x = (uint16_t)v; }
               out += std::to_string(dg_sr_sign((uint8_t)code, n, l)) + "\n"; }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatter_against_python(tmp_path):
    src = tmp_path / "link_main.cpp"; src.write_text(_LINK_MAIN)
    exe = tmp_path / "link_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"), "-o", str(exe), str(src)])
    sites = [("ctg", 0, 0, 0), ("a/b|c", 4294967295, 8192, 1), ("x", 41, 2, 1)]
    signs = [(c, l, n) for c in (0, 1, 5, 9, 13) for l in (0, 1) for n in ([7, 3, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 5, 4, 0], [10, 0, 0, 0, 0, 0, 4, 0])]
    text = "".join("l %s %d %d %d\n" % x for x in sites) + "".join("s %d %d %s\n" % (c, l, " ".join(map(str, n))) for c, l, n in signs)
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    assert out == [slt.linked_sites_line(*x) for x in sites] + [str(srt.sign(c, n) if l else 0) for c, l, n in signs]
    assert out[:2] == ["ctg\t1\t0\t0", "a/b|c\t4294967296\t8192\t1"] and {"1", "-1", "0"} == set(out[3:])


@pytest.mark.gpu
def test_pbdagcon_link_sites(oracle_lib, tmp_path):
    """A planted 600-base target in a SAM file: --haplotag under --link-sites is the twin's lines, --linked-sites the
    formatter's; stdout and --sites do not change."""
    tes = _tes()
    bb, alns, subs, ins_at, n_err = _planted(err=0.02)
    name = "ctg"
    recs = tes._records(bb, alns)
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta([name], [bb]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam([name], [600], [recs]))
    ((_, strings),) = tes._strings([(bb, recs)])

    def lines(link):
        tw = slt.target(600, strings, 500, 50, (2, 80000), link_opts=None if link is None else slt.options(*link))
        tags = [srt.haplotag_line(name, "q0_%d" % i, h, n) for i, h, n in zip(tw["src"], tw["hap"], tw["signed"])]
        linked = [] if link is None else [slt.linked_sites_line(name, p, a, b) for p, a, b in zip(tw["sites"], tw["partners"], tw["linked"])]
        return tw, tags, linked
    off, tags_off, _ = lines(None)
    on, tags_on, linked_on = lines((0, 0, 0, 0))
    tight, tags_tight, linked_tight = lines((50000, 6, 4, 20))
    assert 8 <= sum(on["linked"]) < len(on["linked"]) - 50 and tags_on != tags_off and linked_tight != linked_on and tags_tight != tags_on      # on the twin first
    assert 0 < sum(tight["linked"]) < sum(on["linked"])
    assert on["hap"] == [1] * 12 + [2] * 12
    base = [_cli(), "-c", "6", "-m", "500", "-t", "50", "--site-min-frac", "0.08", "--sam", "--ref", str(ref)]

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    f = {k: tmp_path / k for k in ("h0", "h1", "h2", "h3", "l1", "l2", "l3", "s0", "s1")}
    plain = subprocess.run([x for x in base if x not in ("--site-min-frac", "0.08")] + [str(sam)], capture_output=True, timeout=300)
    assert plain.returncode == 0, plain.stderr.decode()
    got = run("--haplotag", str(f["h0"]), "--sites", str(f["s0"]), str(sam))
    assert got.stdout == plain.stdout and f["h0"].read_text().splitlines() == tags_off
    got = run("--haplotag", str(f["h1"]), "--link-sites", "--linked-sites", str(f["l1"]), "--sites", str(f["s1"]), str(sam))
    assert got.stdout == plain.stdout and f["s1"].read_bytes() == f["s0"].read_bytes()
    assert f["h1"].read_text().splitlines() == tags_on and f["l1"].read_text().splitlines() == linked_on
    run("--haplotag", str(f["h2"]), "--linked-sites", str(f["l2"]), str(sam))                    # the file implies the switch
    assert f["h2"].read_bytes() == f["h1"].read_bytes() and f["l2"].read_bytes() == f["l1"].read_bytes()
    run("--haplotag", str(f["h3"]), "--linked-sites", str(f["l3"]), "--link-max-conflict", "0.05", "--link-min-cell", "6", "--link-min-partners", "4",
        "--link-reach", "20", str(sam))
    assert f["h3"].read_text().splitlines() == tags_tight and f["l3"].read_text().splitlines() == linked_tight


@pytest.mark.gpu
def test_pbdagcon_link_sites_with_phased_windows(oracle_lib, tmp_path):
    """--window --phase-windows --link-sites: the same --haplotag and --linked-sites files whether a batch holds one window
    or four; every position's line once, from the window whose core holds it."""
    from test_window_phase import _planted_records
    bb, recs, groups = _planted_records(chimeras=2)
    name, W, O = "ctg", 150, 70
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta([name], [bb]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam([name], [600], [recs]))
    base = [_cli(), "-c", "6", "-m", "30", "-t", "5", "--sam", "--ref", str(ref), "--window", str(W), "--overlap", str(O), "--phase-windows",
            "--site-min-frac", "0.05"]                                 # (at 0.2 every site of these windows is linked: the reads' errors are few)

    def run(*args):
        r = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r
    out = {}
    for bt in ("1", "4"):
        fh, fl, fs = tmp_path / ("h" + bt), tmp_path / ("l" + bt), tmp_path / ("s" + bt)
        got = run("--haplotag", str(fh), "--link-sites", "--link-min-cell", "2", "--linked-sites", str(fl), "--sites", str(fs), "--batch-targets", bt, str(sam))
        out[bt] = (got.stdout, fh.read_bytes(), fl.read_bytes(), fs.read_bytes())
    assert out["1"] == out["4"]
    linked = [ln.split("\t") for ln in out["1"][2].decode().splitlines()]
    sites = [ln.split("\t") for ln in out["1"][3].decode().splitlines()]
    assert [x[:2] for x in linked] == [x[:2] for x in sites] and len(linked) > 10
    assert {x[3] for x in linked} == {"0", "1"} and all(int(x[3]) == int(int(x[2]) >= 2) for x in linked)
    plain = tmp_path / "h_plain"
    got = run("--haplotag", str(plain), "--sites", str(tmp_path / "s_plain"), str(sam))
    assert got.stdout == out["1"][0] and plain.read_bytes() != out["1"][1]            # stdout never changes; SITES counts only linked sites
