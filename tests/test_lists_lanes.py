"""k_lists_lanes: a lane per backbone position, a wave per 64 positions (targets of up to 64 reads).

Built graphs (FLAG_STOP_AFTER_BUILD) and merged graphs (FLAG_STOP_AFTER_MERGE) against the oracle, vertex by vertex
and entry by entry, on the shapes at which the lane kernel takes another path: backbones that end just before, on and
just behind a wave's last position; rows with more distinct backbone neighbours than a lane's table (they go to the
wave-wide routine); lists that outgrow their fixed pool slot on the first and on the last lane of a wave; folded
duplicate insertions (counts above one on inserted vertices); a target of 65 reads in the same batch (k_lists beside
k_lists_lanes).  Every batch goes through the oracle first (_oracle_graph asserts merge_nodes() == 0).
"""
import numpy as np
import pytest

from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs, _oracle_graph
from test_lists_growth import _wide_target
from util import batch_from_targets, random_target

pytestmark = pytest.mark.gpu


def _run(ctx_factory, batch, merge, trim=0):
    # (the oracle's merged graph of every target first: merge_nodes() == 0 is asserted in there)
    merged = [_oracle_graph(batch, t, 0, trim, True) for t in range(batch.n_targets)]
    exp = merged if merge else [_oracle_graph(batch, t, 0, trim, False) for t in range(batch.n_targets)]
    flags = capi.FLAG_STOP_AFTER_MERGE if merge else capi.FLAG_STOP_AFTER_BUILD
    ctx = ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=flags)
    ctx.consensus(batch)
    return _check_graphs(ctx, batch, trim, merge, oracle_graphs=exp)


def wave_edge_batch():
    """tlen + 2 = 63, 64, 65, 128, 129, 132 positions; 1, 2, 40, 63, 64 reads; one target of 65 reads."""
    rng = np.random.default_rng(6401)
    targets = []
    for i, tl in enumerate((61, 62, 63, 126, 127, 130)):
        for j, k in enumerate((1, 2, 40, 63, 64)):
            alns, bb = random_target(rng, tl, k, alphabet=[b"ACGT", b"AC", b"A"][(i + j) % 3])
            targets.append((tl, alns, bb))
    alns, bb = random_target(rng, 130, 65)
    targets.append((130, alns, bb))
    return batch_from_targets(targets)


def _ends_everywhere(rng, tl=140, k=64):
    """k reads that start at k different positions and end at k different positions: enter's out-row and exit's in-row
    hold k distinct backbone neighbours."""
    bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl))
    alns = []
    for r in range(k):
        s0, e0 = r, tl - (k - 1) + r
        q, t = bytearray(), bytearray()
        for i in range(s0, e0):
            if s0 < i < e0 - 1 and rng.random() < 0.04:
                q.append(0x2D); t.append(bb[i])
            else:
                q.append(bb[i]); t.append(bb[i])
        alns.append((s0 + 1, bytes(q), bytes(t)))
    return tl, alns, bb


def _wide_in_target(rng, tl, k, end_pos):
    """Deletion runs of k different lengths (0 .. k - 1) that all end in front of base end_pos: the in-row of that
    position holds up to k distinct backbone neighbours."""
    bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl))
    alns = []
    for r in range(k):
        q, t = bytearray(), bytearray()
        for i in range(tl):
            if end_pos - r <= i < end_pos:
                q.append(0x2D); t.append(bb[i])
            else:
                q.append(bb[i]); t.append(bb[i])
        alns.append((1, bytes(q), bytes(t)))
    return tl, alns, bb


def table_overflow_batch():
    """Base i is backbone position i + 1 (position 0 is the enter), lane (i + 1) % 64 of its wave."""
    rng = np.random.default_rng(6402)
    targets = [_ends_everywhere(rng), _ends_everywhere(rng, tl=70, k=40)]
    # out-rows: 4 (the table's edge), 5 (just past it), 15 distinct deletion-run lengths at a position in the middle of
    # a wave, on lane 0 and on lane 63 of one
    for k in (5, 6, 16, 40):
        for del_pos in (30, 63, 62, 126):
            targets.append(_wide_target(rng, 150, k, 100, del_pos))
    # in-rows: the same on the arrival side
    for k in (4, 5, 6, 15):
        for end_pos in (30, 63, 62, 127):
            targets.append(_wide_in_target(rng, 150, k, end_pos))
    return batch_from_targets(targets)


def growth_batch():
    """13, 20 and 64 distinct insertions behind base ins_pos: the out-list of position ins_pos + 1 and the in-list of
    position ins_pos + 2 outgrow their slot.  ins_pos 61, 62, 63 put them on lanes 62 / 63, 63 / 0 and 0 / 1."""
    rng = np.random.default_rng(6403)
    targets = []
    for k in (13, 20, 64):
        for ins_pos in (61, 62, 63, 125, 126):
            targets.append(_wide_target(rng, 140, k, ins_pos, 5))
    return batch_from_targets(targets)


def folded_batch():
    """Groups of reads with the same insertion behind the same base (k_emit folds them: counts above one on inserted
    vertices, `extra` in the departure cells), next to reads with insertions of their own and deletions."""
    rng = np.random.default_rng(6404)
    targets = []
    for tl, k in ((70, 12), (130, 40), (66, 64)):
        bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl))
        spots = {10: [b"AC", b"G", b"ACT"], 62: [b"T", b"TT"], 63: [b"GA", b"C"], 64: [b"A"], tl - 1: [b"CA", b"A"]}
        alns = []
        for r in range(k):
            q, t = bytearray(), bytearray()
            for i in range(tl):
                if 20 <= i < 20 + r % 4:
                    q.append(0x2D); t.append(bb[i])
                else:
                    q.append(bb[i]); t.append(bb[i])
                if i in spots and r % 5 != 4:
                    ins = spots[i][r % len(spots[i])]
                    q += ins; t += b"-" * len(ins)
            alns.append((1, bytes(q), bytes(t)))
        targets.append((tl, alns, bb))
    return batch_from_targets(targets)


@pytest.mark.parametrize("merge", [False, True])
def test_wave_edges(gpu_ctx_factory, merge):
    _run(gpu_ctx_factory, wave_edge_batch(), merge, trim=2)


@pytest.mark.parametrize("merge", [False, True])
def test_rows_past_the_lane_table(gpu_ctx_factory, merge):
    _run(gpu_ctx_factory, table_overflow_batch(), merge)


@pytest.mark.parametrize("merge", [False, True])
def test_growth_region_on_wave_edges(gpu_ctx_factory, merge):
    graphs = _run(gpu_ctx_factory, growth_batch(), merge)
    if not merge:
        assert max(len(v["out"]) for g in graphs for v in g if v["backbone"]) > 12
        assert max(len(v["inn"]) for g in graphs for v in g if v["backbone"]) > 12


def test_folded_duplicates_after_merge(gpu_ctx_factory):
    graphs = _run(gpu_ctx_factory, folded_batch(), True)
    # counts above one on edges into inserted vertices: the folded chains
    assert any(c > 1 and not g[d]["backbone"] for g in graphs for v in g if v["backbone"] and not v["deleted"]
               for d, c in v["out"])


def test_folded_duplicates_after_build_without_fold(gpu_ctx_factory, monkeypatch):
    monkeypatch.setenv("DAGCON_FOLD", "0")
    _run(gpu_ctx_factory, folded_batch(), False)
