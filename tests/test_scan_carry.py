"""The carry of the one-block scan (csrc/k_scan.hip.h) behind three of its eight users, the edits, the pile-up's tiles and
the site entries (the other five, k_al_soff, k_al_tscan, k_jn_stretch, k_jn_runs and k_jn_tscan, are carried past their
1,024th item by test_site_table_limits.py): a round takes 1,024 items, and the small batches of test_edits,
test_edit_support, test_pileup and test_site_reads never reach a second one.  One record upload with all four outputs on, sized so that each of the three scans crosses its 1,024th item:

    k_ed_scan    an item is a target                  1,100 targets
    k_sr_scan    an item is an alignment              3,300 alignments
    k_pile_scan  an item is a tile of 256 positions   264,000 positions, 1,032 tiles

Every array is compared with the twins', as those files' own helpers do.  That the input puts work on both sides of each
scan's 1,024th item is a condition on the input: the CPU test checks it on the twins' output, the GPU test on the device's."""
import functools

import numpy as np
import pytest

import pileup_twin as pt

N_T, TL, DEPTH = 1100, 240, 3
MIN_COV, MIN_LEN, TRIM = 3, 30, 0
OPTS = (1, 200000)                                               # a base that one read of three shows makes a site
ROUND, TILE = 1024, 256


def _mods():
    import test_edit_support as tes
    import test_pileup as tp
    import test_site_reads as tsr
    return tes, tp, tsr


def _other(b):
    return b"CGTA"[b"ACGT".index(b)]


@functools.lru_cache(maxsize=None)
def _case():
    """The input and what the twins make of it, computed once.  A target is 240 bases without a repeated neighbour under
    three full-length reads.  Every 40 bases one read of the three shows another base (a site, and an entry of each read);
    at bases 70 and 190 all three do (an edit: the consensus follows the reads)."""
    tes, tp, tsr = _mods()
    rng = np.random.default_rng(1024)
    # (a step of 1..3 letters from one base to the next: no base equals its neighbour)
    letters = np.frombuffer(b"ACGT", np.uint8)[np.cumsum(rng.integers(1, 4, (N_T, TL)), axis=1) % 4]
    targets = []
    for k in range(N_T):
        bb = letters[k].tobytes()
        reads = [bytearray(bb) for _ in range(DEPTH)]
        for x in range(10 + k % 7, TL, 40):
            reads[(k + x) % DEPTH][x] = _other(bb[x])
        for x in (70, 190):
            for r in reads:
                r[x] = _other(bb[x])
        targets.append((bb, tes._records(bb, [(1, bytes(r), bb) for r in reads], eqx=True)))
    strings = tes._strings(targets)
    tlens = [TL] * N_T
    status = [0] * N_T
    edits = tes._twin_edits(strings, MIN_COV, MIN_LEN, TRIM)
    return dict(targets=targets, strings=strings, tlens=tlens, status=status, edits=edits,
                support=tes._twin_support(strings, edits, MIN_LEN, TRIM),
                counts=tp._twin(strings, tlens, MIN_COV, MIN_LEN, TRIM, status),
                reads=tsr._expect(strings, tlens, MIN_COV, MIN_LEN, TRIM, OPTS, 0, status))


def _both_sides(edits, site_begin, site_pos, ent_begin):
    """Edits of a target below and of one at or above index 1,024; sites below and at or above position 1,024 x 256;
    entries of an alignment below and of one at or above index 1,024."""
    n_ed = [sum(len(e) for _, _, _, e in per) for per in edits]
    assert len(n_ed) > ROUND and sum(n_ed[:ROUND]) > 0 and sum(n_ed[ROUND:]) > 0
    g = np.repeat(np.arange(N_T, dtype=np.int64) * TL, np.diff(np.asarray(site_begin, np.int64))) + np.asarray(site_pos, np.int64)
    assert N_T * TL > ROUND * TILE and (g < ROUND * TILE).any() and (g >= ROUND * TILE).any()
    n_ent = np.diff(np.asarray(ent_begin, np.int64))
    assert n_ent.size == N_T * DEPTH > ROUND and n_ent[:ROUND].sum() > 0 and n_ent[ROUND:].sum() > 0


def test_the_input_crosses_the_1024th_item_of_every_scan(oracle_lib):
    case = _case()
    assert all(s is not None for s in case["strings"])
    assert len(case["reads"]["aln_tgt"]) == N_T * DEPTH                  # every alignment is taken: the device's index is the caller's
    _both_sides(case["edits"], case["reads"]["site_begin"], case["reads"]["pos"], case["reads"]["ent_begin"])
    assert (N_T * TL + TILE - 1) // TILE > ROUND


@pytest.mark.gpu
def test_every_scan_carries_into_its_second_round(oracle_lib):
    from pbdagcon_amd import capi
    tes, tp, tsr = _mods()
    case = _case()
    c = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=capi.FLAG_BASE_POS)
    try:
        c.set_edits(True); c.set_edit_support(True)
        c.set_pileup(*OPTS); c.set_site_reads(True, 0)
        got = tes._whole(case["targets"])(c)
        dev = tes._device(c, got)
        sup = tes._flat(c.edit_support())
        sr, ps, pu = c.site_reads(), c.pileup_sites(), c.pileup()
        status = c.target_status.tolist()
    finally:
        c.close()
    assert status == case["status"]
    assert dev == case["edits"] and sup == case["support"]
    assert pu["pos_begin"].tolist() == list(range(0, N_T * TL + 1, TL))
    want = np.concatenate(case["counts"])
    assert np.array_equal(pu["counts"], want), np.argwhere(pu["counts"] != want)[:5].tolist()
    tsr._check((pu, ps, sr), case["reads"])                          # (the sites' targets and positions among the rest)
    g = np.repeat(pu["pos_begin"][:-1].astype(np.int64), np.diff(ps["site_begin"].astype(np.int64))) + ps["pos"]
    assert np.array_equal(ps["counts"], want[g])
    assert ps["pos"][:int(ps["site_begin"][1])].tolist() == pt.sites(case["counts"][0], *OPTS)
    assert sr["aln_src"].tolist() == list(range(N_T * DEPTH))
    _both_sides(dev, ps["site_begin"], ps["pos"], sr["ent_begin"])
