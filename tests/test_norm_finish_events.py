"""k_norm_finish2 visits the events among a lane's columns (csrc/k_norm_fin.hip.h): insertion runs set on the edges the
kernel has -- a 16-byte piece (8 columns), a lane (16 columns), a pass (1,024 columns of a chunk that took its neighbours
in), a chunk (512 input columns) -- against the oracle: consensus, the built graph vertex by vertex, and the literal
loop (k_normalize_slow, FLAG_RAW_ALIGNMENTS) on the same columns.

The reads match a backbone without equal neighbours (norm_cases.plain) base for base, so a chunk starts at every multiple
of 512 input columns and a column of the normalised read is its input column: where a run lands is known here, and
checked against oracle.normalize_gaps before anything runs on the device."""
import numpy as np
import pytest

import oracle
from norm_cases import plain
from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs, _oracle_graph
from test_run_cells import _read
from util import batch_from_targets, oracle_batch, random_target

pytestmark = pytest.mark.gpu

RUNS = (1, 3, 7, 8, 9, 16)
REP0, NREP = 101, 600          # the (AC) x 600 stretch of the first backbone: columns 101 .. 1300


def _ins_runs(q, t):
    """[(first column, length)] of the insertion runs of a normalised alignment."""
    out, k = [], 0
    while k < len(q):
        if t[k] == 0x2D and q[k] != 0x2D:
            s = k
            while k < len(q) and t[k] == 0x2D and q[k] != 0x2D:
                k += 1
            out.append((s, k - s))
        else:
            k += 1
    return out


def _runs_at(edges):
    """_read's runs=[(target base, n)] such that the n-column runs lie on the output columns `edges` = [(first column, n)]
    (in rising order) of a read that starts at target base 0."""
    runs, before = [], 0
    for s, n in edges:
        runs.append((s - before, n))
        before += n
    return runs


def _edge_runs(edge_of, first=0):
    """For every length of RUNS three runs: one that ends on an edge, one that straddles it (a run of 1 cannot: it is the
    edge's first column) and one that begins on it; edge_of(j) = the j-th edge's column."""
    edges, j = [], first
    for n in RUNS:
        for s in (edge_of(j) - n, edge_of(j + 1) - n // 2, edge_of(j + 2)):
            edges.append((s, n))
        j += 3
    return edges


def _big_backbone(rng):
    # 100 plain bases, G, (AC) x 600, T, plain to 2,000: gaps slide through the repeat and through the chunk starts in it
    left = plain(rng, 100, )
    left = left[:-1] + (b"T" if left[-2] != ord("T") else b"C")
    bb = left + b"G" + b"AC" * NREP + b"T"
    return bb + plain(rng, 2000 - len(bb), avoid=ord("T"))


def _hop_read(bb, where, n):
    """The read of norm_cases.pieces' "hop-over AC in t": two inserted bases in front of the repeat, in its phase, whose
    gaps travel through all of it (its chunks take their neighbours in: one chunk of ~1,500 columns from column 0), and
    a run of n columns of G / T, which stays where it is, in front of target base `where`."""
    s, q, t = _read(bb)
    q, t = bytearray(q), bytearray(t)
    ins = bytes(b"GT"[k & 1] for k in range(n))
    q[where:where] = ins; t[where:where] = b"-" * n
    q[REP0:REP0] = b"AC"; t[REP0:REP0] = b"--"
    return s, bytes(q), bytes(t)


def _targets():
    rng = np.random.default_rng(815)
    bb = _big_backbone(rng)
    reads, want = [], []                    # want: per read, the (first column, length) runs it has to show once normalised
    # piece edges that are no lane edges (8, 24, 40 ...), lane edges (16, 32, ...), chunk edges; a run of 16 on each
    for edges in (_edge_runs(lambda j: 8 * (2 * (2 * j + 1) + 1)), _edge_runs(lambda j: 16 * (3 * j + 2)),
                  [(511, 1), (1024 - 3, 7), (1536 - 8, 16)], [(512 - 1, 3), (1024, 8), (1536 - 4, 9)],
                  [(512 - 8, 16), (1024 - 1, 1), (1536, 3)]):
        reads.append(_read(bb, runs=_runs_at(edges)))
        want.append(edges)
    # the pass edge: column 1,024 of the chunk that starts at column 0
    for n in RUNS:
        found = None
        for where in range(1024 - n - 2, 1026):
            r = _hop_read(bb, where, n)
            got = _ins_runs(*oracle.normalize_gaps(r[1], r[2]))
            hit = [(s, m) for s, m in got if m >= n and (s < 1024 < s + m if n > 1 else s in (1023, 1024))]
            # (the two gaps have left column 101 and arrived at the repeat's end, through the chunk starts at 512 and 1,024)
            if hit and got[0] == hit[0] and got[1][0] >= REP0 + 2 * NREP - 2:
                found = (r, hit[0])
                break
        assert found, f"no run of {n} on column 1,024"
        reads.append(found[0]); want.append([found[1]])
    assert len(reads) == 11
    reads.append(_read(bb, runs=_runs_at([(1000, 9)]), trail=7)); want.append([(1000, 9), (2009, 7)])     # ends in a run
    small_bb = plain(rng, 700)
    small = [_read(small_bb, runs=_runs_at([(8 * 7 - 1, 3), (512 - 2, 8)]), trail=3),
             _read(small_bb, first=300, last=360, runs=[(330, 3)]),          # 63 columns: trim 50 leaves none
             _read(small_bb, first=100, last=215, runs=[(157, 7)])]          # 122 columns: trim 50 leaves a window in 3 pieces
    for (s, q, t), w in zip(reads, want):
        got = _ins_runs(*oracle.normalize_gaps(q, t))
        for run in w:
            assert run in got, (run, got[:40])
    return [(2000, reads, bb), (700, small, small_bb)]


@pytest.fixture(scope="module")
def batch():
    targets = _targets()
    assert [len(t[1]) for t in targets] == [12, 3]
    return batch_from_targets(targets)


@pytest.mark.parametrize("trim", [0, 1, 50])
def test_runs_on_the_kernels_edges(gpu_ctx_factory, batch, trim):
    exp = [_oracle_graph(batch, t, 0, trim, False) for t in range(batch.n_targets)]
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(batch)
    _check_graphs(ctx, batch, trim, False, oracle_graphs=exp)
    assert ctx.timings()["reruns"] == 0
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0)
    assert ctx.consensus(batch) == oracle_batch(batch, 0, 0, trim, 0)


def test_random_reads(gpu_ctx_factory):
    """12 random reads on 2,000 positions and 3 on 700, many gaps in flight: the same comparison."""
    rng = np.random.default_rng(816)
    ta, ba = random_target(rng, 2000, 12, alphabet=b"AC", sub=0.04, ins=0.12, dele=0.08, ins_ext=0.4, full_span=True)
    tb, bbb = random_target(rng, 700, 3, alphabet=b"ACGT", sub=0.03, ins=0.15, dele=0.05, ins_ext=0.5, full_span=True)
    b = batch_from_targets([(2000, ta, ba), (700, tb, bbb)])
    for trim in (0, 50):
        ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
        ctx.consensus(b)
        _check_graphs(ctx, b, trim, False)


def _graphs_and_status(gpu_ctx_factory, b, trim, flags):
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=flags | capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(b, strict=False)
    status = ctx.target_status.tolist()
    return [ctx.debug_graph(t) if status[t] == 0 else None for t in range(b.n_targets)], status


@pytest.mark.parametrize("trim", [0, 50])
def test_normalised_columns_against_the_literal_loop(gpu_ctx_factory, trim):
    """The same alignments, already normalised: k_normalize_slow's dg_finish_alignment (raw columns) and the chunked path
    leave the same graphs and the same failure bits.  One read of the small target runs past tlen: that target fails
    (-4) on both paths, the other completes."""
    targets = _targets()
    norm = []
    for tl, alns, bb in targets:
        norm.append((tl, [(s,) + oracle.normalize_gaps(q, t) for s, q, t in alns], bb))
    tl, alns, bb = norm[1]
    over = _read(bb + b"AC" * 32, first=300)               # 464 target bases from position 301 of 700: past tlen with any trim here
    norm[1] = (tl, alns + [(over[0],) + oracle.normalize_gaps(over[1], over[2])], bb)
    b = batch_from_targets(norm)
    raw, raw_status = _graphs_and_status(gpu_ctx_factory, b, trim, capi.FLAG_RAW_ALIGNMENTS)
    got, got_status = _graphs_and_status(gpu_ctx_factory, b, trim, 0)
    assert raw_status == got_status == [0, -4]
    assert got[0] is not None and got == raw
    # and the first target is the oracle's
    one = batch_from_targets(norm[:1])
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(one)
    assert _check_graphs(ctx, one, trim, False) == got[:1]


@pytest.mark.parametrize("n, reruns", [(255, 0), (256, 1), (300, 1)])
def test_long_runs_across_a_lane_edge(gpu_ctx_factory, n, reruns):
    """A run of n columns that begins 5 columns before a lane edge of the first chunk: a byte cell holds 255, a longer run
    costs the re-run with wide cells."""
    rng = np.random.default_rng(817 + n)
    bb = plain(rng, 900)
    reads = [_read(bb) for _ in range(5)]
    reads[2] = _read(bb, runs=_runs_at([(16 * 9 - 5, n), (700, 3)]))
    assert (16 * 9 - 5, n) in _ins_runs(*oracle.normalize_gaps(reads[2][1], reads[2][2]))
    b = batch_from_targets([(900, reads, bb)])
    ctx = gpu_ctx_factory(min_cov=3, min_len=100, trim=5)
    assert ctx.consensus(b) == oracle_batch(b, 3, 100, 5)
    assert ctx.timings()["reruns"] == reruns
    exp = [_oracle_graph(b, 0, 0, 5, False)]
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=5, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(b)
    _check_graphs(ctx, b, 5, False, oracle_graphs=exp)
