"""Every fixed size behind the site tables' common path, crossed on purpose (inputs and restated schedules: site_table_cases.py).

The alleles at the sites and the joined runs go through five one-block scans that take 1,024 items a round, two deep-table
kernels of 1,024 blocks that loop over a list, a block sort of 128 .. 4,096 keys and a key of 20 bases.  The first part of
this file runs on the CPU alone: it asserts from the twin that every family crosses the size it is built for, prints the
figures, and shows that each of seven wrong versions of the schedules gives arrays that differ from the twin's on them.
The GPU part runs each family through test_site_join's _run: every array of the device equal to the twin's, and the
recounts from the device's own arrays.  The device only ever runs the committed code: no mutation is run on it.
"""
from collections import Counter

import numpy as np
import pytest

import alleles_twin as at
import evidence_twin as ev
import join_twin as jt
import pileup_twin as pt
import site_table_cases as stc
import test_site_join as tsj

gpu = pytest.mark.gpu
ALL_CASES = stc.ROUND_CASES + ("past_the_grid", "sort_sizes_distinct", "sort_sizes_tied", "key_length")


def _run_of(exp, k):
    return int(np.searchsorted(np.asarray(exp["run_begin"]), k, side="right")) - 1


# ---- CPU: the families' figures -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", stc.PADS)
def test_rounds_puts_its_boundary_on_item_1024(oracle_lib, p):
    """Measured, for p = 1008 / 1016 / 1023 / 1024 / 1025: 1,208 / 1,216 / 1,223 / 1,224 / 1,225 sites; items 1,023 and 1,024
    in runs 63 and 64 (a head on 1,024, inside the main target's stretch), 64 and 64 (the run [1016, 1032) straddles the
    round), 64 and 64 (the main target, its stretch and a run begin on 1,023), 63 and 64 (they begin on 1,024), 63 and 64
    (the pad's last run is item 1,024 alone)."""
    c = stc.rounds(p)
    exp, f = c.exp, stc.figures(c.exp)
    n = len(exp["pos"])
    r23, r24 = _run_of(exp, 1023), _run_of(exp, 1024)
    print(c.name, "sites", n, "runs", len(exp["spanning"]), "item 1023 in run", r23, "item 1024 in run", r24, "head on 1024", 1024 in exp["run_begin"],
          "depths in front", sum(f["depth"][:1024]), "alleles in front", sum(f["al_nd"][:1024]), "joined alleles", len(exp["jkey"]))
    assert n == p + stc.MAIN and exp["site_begin"] == [0, p, n] and exp["pos"] == list(range(p)) + list(range(stc.MAIN))
    assert (r23, r24, 1024 in exp["run_begin"]) == stc.ROUNDS_WANT[p]
    assert tsj._runs(exp)[:p // 16] == [16] * (p // 16) and p in exp["run_begin"]
    if p == 1016:
        assert exp["run_begin"][r24:r24 + 2] == [1016, 1032]
    assert sum(f["depth"][:1024]) > 0 and sum(f["al_nd"][:1024]) > 0 and min(f["depth"]) >= 3
    # the read with other bases: two alleles at the sites 1,020 .. 1,028 (normalizeGaps may move one to the site behind) and
    # one everywhere else, and joined tables of two there
    two = [k for k, d in enumerate(f["al_nd"]) if d != 1]
    print(c.name, "sites with two alleles", two)
    assert set(stc.AROUND) - {1028} <= set(two) <= set(stc.AROUND) | {1029} and {f["al_nd"][k] for k in two} == {2}
    assert {f["depth"][k] for k in stc.AROUND} == {4}
    assert {r for r, d in enumerate(f["jn_nd"]) if d != 1} == {_run_of(exp, k) for k in two}
    assert not stc.differs(exp, stc.scans(exp))


def test_past_the_grid_lists_more_than_1024_of_both(oracle_lib):
    """Measured: 1,061 sites (1,050 at even positions, 11 behind one of them), depths 65 .. 70, all deep; 1,039 runs, 11 of
    three sites, 65 .. 70 spanning members each, all deep; 10 partial members; tables of 2, 3 and 4 alleles, no two
    consecutive sites' tables equal, nor two consecutive runs'; 3,173 alleles and 3,151 joined alleles in all."""
    c = stc.past_the_grid()
    exp, (tw,) = c.exp, c.exp["tw"]
    f = stc.figures(exp)
    even = list(range(10, 2110, 2))
    pairs = [x + 1 for x in even if stc._grid_pair(x // 2)]
    deep_s, deep_r = stc.deep_list(f["depth"]), stc.deep_list(exp["spanning"])
    lens = Counter(f["al_nd"])
    print(c.name, "sites", len(tw["sites"]), "runs", len(tw["spanning"]), "deep sites", len(deep_s), "deep runs", len(deep_r), "depths", sorted(Counter(f["depth"]).items()),
          "spanning", sorted(Counter(tw["spanning"]).items()), "partial members", sum(tw["partial"]), "table lengths", sorted(lens.items()),
          "joined table lengths", sorted(Counter(f["jn_nd"]).items()), "alleles", len(exp["key"]), "joined alleles", len(exp["jkey"]))
    assert tw["sites"] == sorted(even + pairs) and len(even) == 1050 and len(pairs) == 11
    assert len(deep_s) == len(tw["sites"]) == 1061 > stc.GRID and len(deep_r) == len(tw["spanning"]) == 1039 > stc.GRID
    assert f["depth"] == [pt.depth(tw["counts"][x]) for x in tw["sites"]] and set(f["depth"]) == set(range(65, 71)) and min(tw["spanning"]) >= 65
    assert sorted(Counter(tsj._runs(exp)).items()) == [(1, 1028), (3, 11)] and sum(tw["partial"]) == 2 * len(stc.GRID_SHORT) and max(tw["partial"]) == 1
    assert set(lens) == {2, 3, 4} and min(lens.values()) > 200
    # which site a block meets on its second trip is the order of execution's to say: every neighbour differs, and so do the
    # two that the ascending list would give one block
    tabs = tw["tables"]
    assert all(a != b for a, b in zip(tabs, tabs[1:])) and all(a != b for a, b in zip(tw["jtables"], tw["jtables"][1:]))
    assert all(tabs[deep_s[w]] != tabs[deep_s[w - stc.GRID]] for w in range(stc.GRID, len(deep_s)))
    assert all(tw["jtables"][deep_r[w]] != tw["jtables"][deep_r[w - stc.GRID]] for w in range(stc.GRID, len(deep_r)))
    assert len({tuple(t) for t in tabs}) > 100
    assert not stc.differs(exp, stc.scans(exp)) and not stc.differs(exp, stc.with_trips(exp))


@pytest.mark.parametrize("pattern", stc.PATTERNS)
def test_sort_sizes_reaches_every_size_from_both_sides(oracle_lib, pattern):
    """Measured, per depth 128, 129, 256, 257, 512, 513, 1,024, 1,025, 2,048, 2,049: site 10's depth and both runs'
    spanning counts are the depth; n2 is 128, 256, 256, 512, 512, 1,024, 1,024, 2,048, 2,048, 4,096.  distinct: site 10's
    table and the run [16, 30)'s joined table are as long as the depth, the run [0, 16)'s has 16 keys.  tied: 20, 21, 30,
    31, 42, 43, 42, 43, 42, 43 alleles at site 10, every count twice (at an odd depth the count 1 three times), the largest
    groups 19, 19, 23, 23, 46, 46, 302, 302, 814 and 814 members."""
    c = stc.sort_sizes(pattern)
    assert [stc.n2_of(d) for d in stc.DEPTHS] == [128, 256, 256, 512, 512, 1024, 1024, 2048, 2048, 4096]
    assert {stc.n2_of(d) for d in stc.DEPTHS} | {stc.N2_MAX} == {128 << k for k in range(6)}
    for depth, tw in zip(stc.DEPTHS, c.exp["tw"]):
        tab, jtab = tw["tables"][stc.SITE], tw["jtables"]
        counts = Counter(cnt for _, cnt, _ in tab)
        print(c.name, "depth", depth, "n2", stc.n2_of(depth), "alleles at site 10", len(tab), "joined alleles", [len(t) for t in jtab],
              "largest group", tab[0][1], "alleles at 18 21 25", [len(tw["tables"][x]) for x in stc.OTHER_RUN])
        assert tw["sites"] == list(range(30)) and tw["run_begin"] == [0, 16, 30]
        assert pt.depth(tw["counts"][stc.SITE]) == depth and tw["spanning"] == [depth, depth] and tw["partial"] == [0, 0]
        assert all(pt.depth(tw["counts"][x]) == depth for x in range(30))
        if pattern == "distinct":
            assert len(tab) == depth and len(jtab[1]) == depth and len(jtab[0]) == 16 and counts == {1: depth}
            assert all(len(tw["tables"][x]) <= 14 for x in stc.OTHER_RUN)
        else:
            sizes = stc.tied_sizes(depth)
            assert sorted((cnt for _, cnt, _ in tab), reverse=True) == sorted(sizes, reverse=True) and len(tab) == len(sizes)
            assert all(n == 2 or (n == 3 and depth % 2 and cnt == 1) for cnt, n in counts.items())
            assert (tab[0][1] > 256) == (depth >= 1024)
            assert len(jtab[0]) == 16 and len(jtab[1]) == min(14, len(sizes))
        # the restated sort builds the twin's table at every size
        assert stc.block_table(tab) == [(kk, cnt) for kk, cnt, _ in tab] and stc.block_table(jtab[1]) == [(kk, cnt) for kk, cnt, _ in jtab[1]]
    assert not stc.differs(c.exp, stc.scans(c.exp))


def test_key_length_has_the_cap_between_its_alleles(oracle_lib):
    """Measured: the site at base 62 has alleles of 19, 19, 20, 21, 21, 21 and 22 bases and the bare base: five keys, counts
    6 (the bare base), 3 (bit 60), 2 (19 bases), 1 (20 bases, no bit 60), 1 (bit 60, another 20th base); its entries stand
    in column 60 of every read.  The site at base 81 has 19 bases twice, once where the run's last column is the
    alignment's last, and 26 bases (bit 60) there too.  Both runs hold joined keys whose text is opaque."""
    c = stc.key_length()
    (tw,) = c.exp["tw"]
    (bb, reads), = c.strings
    cols = ev.columns(reads, c.min_len, c.trim)
    assert len(cols) == len(reads) == 13 and tw["sites"] == list(range(2, 98))
    lens = []
    for s0, q, t in cols:
        tcs, _ = ev.coords(s0, t)
        i = tcs.index(stc.KEY_SITE)
        assert i == stc.KEY_LANE and s0 == 2                             # lane 60 of the first 64-column step
        lens.append(len(at.allele(q, t, i)))
    assert lens == [21, 21, 22, 21, 20, 19, 19, 1, 1, 1, 1, 1, 1]
    # where hi ends the run: the trimmed alignment's last column is the run's last
    ends = [(len(at.allele(q, t, ev.coords(s0, t)[0].index(stc.KEY_END_SITE))), t[-1] == ev.GAP) for s0, q, t in cols[10:]]
    assert ends == [(19, True), (26, True), (19, False)]
    k = tw["sites"].index(stc.KEY_SITE)
    tab = tw["tables"][k]
    bare, long3, k19, k20, long1 = tab
    print(c.name, "table at 62", [(at.text(kk), cnt) for kk, cnt, _ in tab], "table at 81", [(at.text(kk), cnt) for kk, cnt, _ in tw["tables"][tw["sites"].index(stc.KEY_END_SITE)]])
    assert [cnt for _, cnt, _ in tab] == [6, 3, 2, 1, 1]
    assert long3[0] & at.LONG and long1[0] & at.LONG and not k20[0] & at.LONG and not k19[0] & at.LONG and not bare[0] & at.LONG
    assert long3[0] == k20[0] | at.LONG and long1[0] != long3[0] and (long1[0] ^ long3[0]) >> 3 == 0          # they differ in the 20th base alone
    assert [len(at.text(kk).rstrip("+")) for kk, _, _ in tab] == [1, 20, 19, 20, 20]
    ke = tw["sites"].index(stc.KEY_END_SITE)
    assert [(len(at.text(kk)), cnt) for kk, cnt, _ in tw["tables"][ke]] == [(1, 10), (19, 2), (21, 1)] and tw["tables"][ke][2][0] & at.LONG
    # the joined tables: a key over a long allele has no text
    rb = tw["run_begin"]
    opaque = {}
    for site in (k, ke):
        r = _run_of(c.exp, site)
        assert rb[r + 1] - rb[r] > 1
        opaque[r] = [jt.jtext(kk, tw["tables"][rb[r]:rb[r + 1]]) for kk, _, _ in tw["jtables"][r]]
    print(c.name, "joined texts", opaque)
    assert all(("*", True) in texts and any(not o for _, o in texts) for texts in opaque.values())
    assert stc.tables_with_cap(reads, c.min_len, c.trim, tw["sites"]) == [[cnt for _, cnt, _ in t] for t in tw["tables"]]


# ---- CPU: the wrong versions --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mut", stc.MUTATIONS[:2])
def test_a_wrong_carry_is_rejected(oracle_lib, mut):
    """The carry dropped at a round's start, or taken one item early (thread 1,023's offset without its own count), in each of
    the five scans: the arrays differ from the twin's on every case the table names, and which arrays do is printed for all."""
    for scan in stc.SCANS:
        for name in ALL_CASES:
            exp = stc.case(name).exp
            bad = stc.differs(exp, stc.scans(exp, mut, scan))
            print(mut, scan, name, "differs in", bad)
            must = name in stc.CARRY_REJECTS[(mut, scan)]
            assert bad if must else True, (mut, scan, name)
            if len(exp["pos"]) <= stc.ROUND:
                assert not bad                                           # (a batch of one round has no carry to lose)
        assert stc.CARRY_REJECTS[(mut, scan)]


def test_a_run_number_read_for_a_stretch_number_is_rejected(oracle_lib):
    """k_jn_runs reads jn_run[k] as a stretch number and writes the run number over it in the same pass.  Were an item at or
    beyond 1,024 to read the run number, it would look up jn_sfirst under it: a word that no stretch wrote."""
    for stale, names in stc.STRETCH_REJECTS.items():
        for name in stc.ROUND_CASES:
            exp = stc.case(name).exp
            bad = stc.differs(exp, stc.scans(exp, stc.MUTATIONS[2], "k_jn_runs", stale=stale))
            print("run_for_stretch, unwritten words", stale, name, "differs in", bad)
            assert ("run_begin" in bad) if name in names else True, (stale, name)


@pytest.mark.parametrize("mut", stc.MUTATIONS[3:5])
def test_a_wrong_second_trip_is_rejected(oracle_lib, mut):
    """A deep block that stops after its first trip leaves the tables of list entries 1,024 .. unwritten; one that keeps s_nd
    adds its first table's length to its second's.  Both lists of past_the_grid are longer than the grid."""
    exp = stc.past_the_grid().exp
    f = stc.figures(exp)
    for lengths, nd, what in ((f["depth"], f["al_nd"], "al_begin"), (exp["spanning"], f["jn_nd"], "jal_begin")):
        deep = stc.deep_list(lengths)
        got = stc.deep_trips(deep, nd, mut)
        wrong = [k for k in deep if got[k] != nd[k]]
        print(mut, what, "listed", len(deep), "wrong lengths", len(wrong))
        assert len(wrong) == len(deep) - stc.GRID > 0 and stc.deep_trips(deep, nd) == {k: nd[k] for k in deep}
    bad = stc.differs(exp, stc.with_trips(exp, mut))
    print(mut, "differs in", bad)
    assert "al_begin" in bad and "jal_begin" in bad
    # ... and a batch whose lists are shorter than the grid cannot tell
    small = stc.sort_sizes("distinct").exp
    assert not stc.differs(small, stc.with_trips(small, mut))


def test_a_sort_one_power_too_small_is_rejected(oracle_lib):
    """n2 one power too small at depth 2^k + 1: the last key of the stretch is never loaded.  Every such depth rejects it, in
    the site's table and in the run's, in both patterns; at 2^k nothing changes."""
    for pattern in stc.PATTERNS:
        c = stc.sort_sizes(pattern)
        for depth, tw in zip(stc.DEPTHS, c.exp["tw"]):
            for tab in (tw["tables"][stc.SITE], tw["jtables"][0], tw["jtables"][1]):
                want = [(kk, cnt) for kk, cnt, _ in tab]
                got = stc.block_table(tab, stc.MUTATIONS[5])
                assert (got != want) == (depth % 2 == 1), (pattern, depth)
    assert stc.n2_of(129, "n2_small") == 128 and stc.n2_of(257, "n2_small") == 256 and stc.n2_of(2049, "n2_small") == 2048 and stc.n2_of(2048, "n2_small") == 2048


def test_a_cap_of_21_bases_is_rejected(oracle_lib):
    """With 21 bases in a key the alleles of 21, 21 (another 21st base) and 22 bases are three, not one."""
    c = stc.key_length()
    (tw,) = c.exp["tw"]
    (bb, reads), = c.strings
    got = stc.tables_with_cap(reads, c.min_len, c.trim, tw["sites"], 21)
    want = [[cnt for _, cnt, _ in t] for t in tw["tables"]]
    k = tw["sites"].index(stc.KEY_SITE)
    print("cap 21 at site 62:", got[k], "cap 20:", want[k])
    assert got[k] == [6, 2, 1, 1, 1, 1, 1] and want[k] == [6, 3, 2, 1, 1] and [i for i in range(len(want)) if got[i] != want[i]] == [k]
    # and no other family has an allele at the cap: only this one can tell
    for name in ALL_CASES[:-1]:
        cc = stc.case(name)
        assert all(len(at.text(kk).rstrip("+")) < 19 for kk in cc.exp["key"]), name


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _on_the_device(c, phase=True):
    dev, _ = tsj._run(tsj._strings_call(c.strings), c.strings, c.tlens, c.min_cov, c.min_len, c.trim, c.opts, phase, exp=c.exp)
    return dev


@gpu
@pytest.mark.parametrize("p", stc.PADS)
def test_rounds_on_the_device(oracle_lib, p):
    """Item 1,024 of k_al_soff, k_al_tscan, k_jn_stretch and k_jn_runs: a run head on it, a run across it, a target and a
    stretch that begin on it, and the items either side."""
    dev = _on_the_device(stc.rounds(p))
    assert dev["js"]["run_begin"].size > 64 and dev["ps"]["pos"].size == p + stc.MAIN > stc.ROUND


@gpu
@pytest.mark.parametrize("phase", [True, False])
def test_past_the_grid_on_the_device(oracle_lib, phase):
    """1,061 deep sites and 1,039 deep runs on 1,024 blocks each: 37 and 15 blocks take a second trip; 1,039 items for
    k_jn_tscan."""
    dev = _on_the_device(stc.past_the_grid(), phase)
    assert dev["js"]["spanning"].size == 1039 and int(dev["js"]["spanning"].min()) > stc.WAVE
    assert dev["ps"]["pos"].size == 1061 and int(dev["ps"]["counts"][:, :6].sum(axis=1).min()) > stc.WAVE


@gpu
@pytest.mark.parametrize("pattern", stc.PATTERNS)
def test_sort_sizes_on_the_device(oracle_lib, pattern):
    """Every n2 from 128 to 4,096 but 4,096 alone from below (test_the_deepest_site has 4,094), each from 2^k and 2^k + 1."""
    dev = _on_the_device(stc.sort_sizes(pattern))
    depth = dev["ps"]["counts"][:, :6].sum(axis=1).reshape(len(stc.DEPTHS), 30)
    assert (depth == np.asarray(stc.DEPTHS)[:, None]).all()


@gpu
def test_key_length_on_the_device(oracle_lib):
    dev = _on_the_device(stc.key_length())
    keys = dev["sa"]["key"]
    assert int(((keys & np.uint64(at.LONG)) != 0).sum()) >= 3
