"""Insertion-run cells (matC) a byte wide where the cells stay run lengths, 32 bits wide where a run outgrows a byte or a
target has more than 64 reads; and dagcon_fetch's two rounds (the status block, then what it sizes).  Every batch against
the CPU oracle; the re-run with wide cells is counted in timings()["reruns"]."""
import numpy as np
import pytest

import oracle
import support_twin as st
from pbdagcon_amd import capi, synth
from util import batch_from_targets, oracle_batch

pytestmark = pytest.mark.gpu

OPTS = dict(min_cov=3, min_len=100, trim=5)
OARGS = (3, 100, 5)


def _backbone(rng, tlen):
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, tlen))


def _read(bb, runs=(), first=0, last=None, lead=0, trail=0):
    """An alignment that matches bb[first:last] base for base, with an insertion run of n columns in front of target base
    i (0-based) for every (i, n) of runs, `lead` insertion columns in front of its first and `trail` behind its last
    column.  Inserted bases differ from the target base behind the run, so normalizeGaps leaves the run where it is."""
    last = len(bb) if last is None else last
    runs = dict(runs)
    q, t = bytearray(), bytearray()

    def insert(n, nxt):
        two = [c for c in b"ACGT" if c != nxt][:2]
        for k in range(n):
            q.append(two[k & 1]); t.append(0x2D)

    insert(lead, bb[first])
    for i in range(first, last):
        if i in runs and i > first:
            insert(runs[i], bb[i])
        q.append(bb[i]); t.append(bb[i])
    insert(trail, 0)
    return first + 1, bytes(q), bytes(t)


def _target(rng, tlen, n_reads, special):
    """tlen, n_reads full-span plain reads with `special` = {read index: kwargs of _read} replacing some of them."""
    bb = _backbone(rng, tlen)
    return tlen, [_read(bb, **special.get(r, {})) for r in range(n_reads)], bb


def _run(ctx, batch):
    got = ctx.consensus(batch)
    assert got == oracle_batch(batch, *OARGS)
    assert sum(len(s) for segs in got for _, _, s in segs) > 0
    return ctx.timings()["reruns"]


def test_runs_at_the_byte_edge(gpu_ctx_factory):
    """One read of a target carries a run of 254, 255, 256 columns (far beyond both LDS windows of the chunked
    normalizeGaps: dg_finish_alignment's writer).  A byte holds the first two; the third costs one re-run."""
    rng = np.random.default_rng(5)
    targets = [_target(rng, 700 + 3 * k, 8, {3: dict(runs=[(350, n)])}) for k, n in enumerate((254, 255, 256))]
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets(targets[:2])) == 0
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets(targets)) == 1


def test_runs_inside_the_lds_windows(gpu_ctx_factory):
    """Runs of 30 to 90 columns: k_norm_finish2's writer (and its scan of run lengths across lanes and passes)."""
    rng = np.random.default_rng(6)
    special = {0: dict(runs=[(200, 30), (900, 61)]), 2: dict(runs=[(640, 45)]), 5: dict(runs=[(333, 90), (334, 33)]),
               9: dict(runs=[(1400, 64), (1465, 77)])}
    targets = [_target(rng, 1501, 10, special), _target(rng, 777, 7, {6: dict(runs=[(123, 88)])})]
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets(targets)) == 0


def test_stretch_edges_of_k_emit(gpu_ctx_factory):
    """Two stretches of 512 positions.  Runs in front of the positions around 512, in different reads and in one read
    (pfx_entry: a lane enters the second stretch behind a run; pfx_next: the first stretch's look-ahead ends in a run);
    reads that end in a trailing run, at the target's end and right at the stretch edge (checkpoints); reads that start
    at the edge, plain and behind a leading run."""
    rng = np.random.default_rng(7)
    special = {0: dict(runs=[(511, 3)]), 1: dict(runs=[(510, 2)]), 2: dict(runs=[(512, 4)]), 3: dict(runs=[(513, 2)]),
               4: dict(runs=[(510, 1), (511, 2), (512, 3), (513, 1)]), 5: dict(trail=5),
               6: dict(last=511, trail=3), 7: dict(last=512, trail=2), 8: dict(first=511), 9: dict(first=512, lead=3),
               10: dict(first=510, runs=[(511, 2), (512, 2)])}
    batch = batch_from_targets([_target(rng, 1100, 13, special)])
    assert _run(gpu_ctx_factory(**OPTS), batch) == 0
    # the same reads with every target of the batch full-span but these: the other merge path, the same k_emit
    full = {k: v for k, v in special.items() if "first" not in v and "last" not in v}
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets([_target(rng, 1100, 8, full)])) == 0


def test_lane_edges(gpu_ctx_factory):
    """Exactly a wave of reads, long runs in its first and last lane: byte cells.  65 reads: the prefix over the reads is
    taken in place (k_groups), 32-bit cells as before, and a run of 300 columns is nothing special."""
    rng = np.random.default_rng(8)
    t64 = _target(rng, 600, 64, {0: dict(runs=[(100, 200), (300, 255)]), 63: dict(runs=[(300, 255), (500, 120)])})
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets([t64])) == 0
    t65 = _target(rng, 600, 65, {0: dict(runs=[(100, 300)]), 64: dict(runs=[(100, 300), (500, 255)])})
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets([t65])) == 0


def test_wide_batch_then_narrow_batch(gpu_ctx_factory):
    """The mark a run of more than 255 columns leaves on a context lasts until the upload of a batch without such a run."""
    rng = np.random.default_rng(9)
    wide = batch_from_targets([_target(rng, 640, 8, {1: dict(runs=[(320, 400)])}), _target(rng, 500, 6, {})])
    narrow = batch_from_targets([_target(rng, 640, 8, {1: dict(runs=[(320, 255)])}), _target(rng, 900, 9, {4: dict(runs=[(77, 9)])})])
    ctx = gpu_ctx_factory(**OPTS)
    assert _run(ctx, wide) == 1
    assert _run(ctx, narrow) == 0
    assert _run(ctx, wide) == 1


def test_fetch_without_segments(gpu_ctx_factory):
    """Every read under min_len: no alignment reaches the device, no segment and no consensus base come back."""
    rng = np.random.default_rng(10)
    batch = batch_from_targets([_target(rng, 300, 8, {}), _target(rng, 350, 8, {2: dict(runs=[(100, 20)])})])
    ctx = gpu_ctx_factory(min_cov=3, min_len=500, trim=5, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    got = ctx.consensus(batch)
    assert got == oracle_batch(batch, 3, 500, 5) == [[], []]
    assert ctx.fetch_support_raw()[0].size == 0 and ctx.fetch_positions_raw().size == 0
    assert ctx.timings()["reruns"] == 0


def test_fetch_one_target(gpu_ctx_factory):
    rng = np.random.default_rng(11)
    assert _run(gpu_ctx_factory(**OPTS), batch_from_targets([_target(rng, 901, 8, {3: dict(runs=[(450, 12)])})])) == 0


def _twin_positions(tlen, alns, min_len, trim, min_weight):
    """support_twin.consensus_target_support's walk with _bbMap in place of the weights: [(range0, range1, positions)]."""
    g = oracle.Graph(blen=tlen)
    for start, q, t in alns:
        if len(q) < min_len:
            continue
        q, t = oracle.normalize_gaps(q, t)
        q, t, start = oracle.trim_aln(q, t, start, trim)
        g.add_aln(start, q, t)
    assert g.merge_nodes() == 0
    path = g.best_path()
    ends = (st._node(g.L, g.g, 0)[0], st._node(g.L, g.g, tlen + 1)[0])
    bms = [bm for base, _, _, bm in (st._node(g.L, g.g, v) for v in path) if base not in ends]
    return [(r0, r1, bms[r0:r1]) for r0, r1, _ in g.consensus_all(min_weight, min_len)]


def test_fetch_support_and_positions(gpu_ctx_factory):
    """Both per-base outputs ride in the fetch's second round: the twin's values, base for base."""
    batch = synth.make_batch(3, 1300, 12, seed=21)
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)
    got = ctx.consensus(batch)
    assert got == oracle_batch(batch, 6, 500, 50)
    exp = st.batch_support(batch, 6, 500, 50)
    sup, pos = ctx.base_support(), ctx.base_positions()
    n = 0
    for t in range(batch.n_targets):
        assert got[t] == [s[:3] for s in exp[t]]
        assert [(w.tolist(), d.tolist()) for w, d in sup[t]] == [(s[3], s[4]) for s in exp[t]]
        tp = _twin_positions(int(batch.tlen[t]), batch.target_alignments(t), 500, 50, 6)
        assert [(r0, r1) for r0, r1, _ in got[t]] == [(r0, r1) for r0, r1, _ in tp]
        assert [p.tolist() for p in pos[t]] == [p for _, _, p in tp]
        n += sum(len(s) for _, _, s in got[t])
    assert n > 0
