"""k_norm_chunk's first pass visits only the columns that hold a gap (dg_norm_run_gc, csrc/k_norm_run.hip.h): the
device against oracle.normalize_gaps and oracle.trim_aln, exactly.

The shapes are the smallest that still cross a refill (16 input columns), a chunk edge (512), the re-run region (a
gap that slides through a chunk start) and the second pass (a look-ahead the 64-column window cannot serve): about
40 alignments of 600 to 3,000 columns with the constructions of tests/norm_cases.py set on chunk edges, a few random
ones with many gaps in flight, and one small target through the graph."""
import numpy as np
import pytest

import oracle
from norm_cases import pieces, plain
from util import batch_from_targets, oracle_batch, random_target

pytestmark = pytest.mark.gpu


def _alignments():
    rng = np.random.default_rng(512)
    alns, names = [], []
    for k, (name, pq, pt) in enumerate(pieces(rng)):
        # the piece starts 500 .. 530 columns into a window of 512 input columns: on or next to the chunk edge
        at = 512 * (1 + k % 2) + 500 + (k * 7) % 31
        left = plain(rng, at - 1) + b"C"                   # (the pieces start with G)
        right = plain(rng, max(80, 600 - at - len(pq)), avoid=pq[-1])
        alns.append((1, left + pq + right, left + pt + right))
        names.append(name)
    # a gap column as the very last column, the alignment ending on a chunk edge
    s = plain(rng, 1024)
    alns.append((1, s, s[:-1] + b"-")); names.append("last column insertion")
    alns.append((1, s[:-1] + b"-", s)); names.append("last column deletion")
    # random alignments, many gaps in flight
    for i in range(6):
        a1, _ = random_target(rng, int(rng.integers(600, 2400)), 1, alphabet=[b"AC", b"ACGT"][i % 2], sub=0.05, ins=0.15,
                              dele=0.10, ins_ext=0.4, full_span=True, dots=(i == 4))
        alns.append(a1[0]); names.append(f"random {i}")
    return alns, names


@pytest.fixture(scope="module")
def cases():
    alns, names = _alignments()
    assert 35 <= len(alns) <= 50 and all(600 <= len(q) <= 3000 for _, q, _ in alns)
    return alns, names, [oracle.normalize_gaps(q, t) for _, q, t in alns]


@pytest.mark.parametrize("trim", [0, 1, 50])
def test_normalize_constructed(gpu_ctx_factory, cases, trim):
    alns, names, normalized = cases
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=0, min_weight=0)
    got = ctx.normalize(alns, trim=trim)
    assert len(got) == len(alns)
    for name, (s, _, _), (qn, tn), (gs, gq, gt) in zip(names, alns, normalized, got):
        assert (gq, gt, gs) == oracle.trim_aln(qn, tn, s, trim), f"{name}, trim {trim}"


def test_consensus_through_the_chunk_results(gpu_ctx_factory):
    """matC, ckpt and the counts k_norm_finish2 derives from the chunk results: 12 reads on 2,000 positions."""
    rng = np.random.default_rng(513)
    tl = 2000
    ta, bb = random_target(rng, tl, 12, alphabet=b"AC", sub=0.04, ins=0.12, dele=0.08, ins_ext=0.4, full_span=True)
    batch = batch_from_targets([(tl, ta, bb)])
    for kw in (dict(min_cov=0, min_len=0, trim=0, min_weight=0), dict(min_cov=4, min_len=100, trim=50, min_weight=-1)):
        ctx = gpu_ctx_factory(**kw)
        got = ctx.consensus(batch)
        exp = oracle_batch(batch, kw["min_cov"], kw["min_len"], kw["trim"], kw["min_weight"])
        assert got == exp
