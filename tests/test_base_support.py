"""Per-base support (DAGCON_FLAG_BASE_SUPPORT, dagcon_fetch_support, Context.base_support) against the CPU twin
(tests/support_twin.py: the oracle's graph after mergeNodes, read along its best path), in every bestPath regime;
the consensus itself unchanged; the call sequence refused where it has no results."""
import numpy as np
import pytest

import oracle
import support_twin as st
from pbdagcon_amd import capi, synth
from util import batch_from_targets, oracle_batch, random_target

pytestmark = pytest.mark.gpu

SUP = capi.FLAG_BASE_SUPPORT


def _check(ctx, got, exp_sup, targets=None):
    """got: the consensus of ctx's last run; exp_sup: batch_support's value (per target); targets: the ones to compare."""
    sup = ctx.base_support()
    assert len(sup) == len(got) == len(exp_sup)
    n = 0
    for t in (range(len(got)) if targets is None else targets):
        exp = exp_sup[t]
        assert got[t] == [s[:3] for s in exp], t
        assert len(sup[t]) == len(exp)
        for (w, d), (_, _, seq, ew, ed) in zip(sup[t], exp):
            assert w.dtype == np.uint16 and d.dtype == np.uint16 and w.size == d.size == len(seq)
            assert w.tolist() == ew and d.tolist() == ed, t
            n += w.size
    return n


@pytest.mark.parametrize("max_segments", [0, 1, 64])
def test_full_span_batches(gpu_ctx_factory, max_segments):
    """synth full-span pileups (k_bp_walk, one piece per target or many)."""
    batch = synth.make_batch(6, 2200, 16, seed=11 + max_segments)
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP, max_segments=max_segments)
    got = ctx.consensus(batch)
    assert got == oracle_batch(batch, 6, 500, 50)
    assert _check(ctx, got, st.batch_support(batch, 6, 500, 50)) > 0


def test_lane_walk(gpu_ctx_factory, monkeypatch):
    """k_bp_walk_r<true>: forced on a small batch, and chosen by itself on a batch of 40,000 pieces (a sample of its
    targets against the twin)."""
    batch = synth.make_batch(5, 3000, 20, seed=5)
    monkeypatch.setenv("DAGCON_BP_LANE", "2")
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP)
    got = ctx.consensus(batch)
    assert _check(ctx, got, st.batch_support(batch, 6, 500, 50)) > 0
    monkeypatch.delenv("DAGCON_BP_LANE")
    big = synth.make_batch(640, 10000, 24, seed=9)
    ctx2 = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP)
    got2 = ctx2.consensus(big)
    sample = [0, 1, 317, 639]
    exp = [st.batch_support(big.select([t]), 6, 500, 50)[0] if t in sample else None for t in range(big.n_targets)]
    assert _check(ctx2, got2, exp, sample) > 0
    # and the whole of it covers every base exactly once
    sup = ctx2.base_support()
    assert sum(w.size for segs in sup for w, _ in segs) == sum(len(s) for segs in got2 for _, _, s in segs)


def test_partial_span_pileups(gpu_ctx_factory):
    """random_target pileups, reads that start and end anywhere (k_cuts2 / k_bp_walk_g and its cns_tmp0 piece)."""
    rng = np.random.default_rng(41)
    targets = []
    for tl, k in ((900, 14), (1400, 20), (2600, 9), (700, 30)):
        alns, bb = random_target(rng, tl, k, sub=0.04, ins=0.08, dele=0.05)
        targets.append((tl, alns, bb))
    batch = batch_from_targets(targets)
    for flags, ms in ((SUP, 0), (SUP, 64), (SUP | capi.FLAG_DEBUG_RESWEEP, 0)):
        ctx = gpu_ctx_factory(min_cov=3, min_len=100, trim=5, flags=flags, max_segments=ms)
        got = ctx.consensus(batch)
        assert got == oracle_batch(batch, 3, 100, 5)
        assert _check(ctx, got, st.batch_support(batch, 3, 100, 5)) > 0


def test_real_backbone_and_resweep(gpu_ctx_factory):
    """dagcon_batch.backbone (dazcon's path: backbone vertices start at weight 1) and DAGCON_FLAG_DEBUG_RESWEEP."""
    batch = synth.make_batch(4, 1800, 14, seed=23, with_backbone=True)
    exp = st.batch_support(batch, 6, 500, 10)
    for flags in (SUP, SUP | capi.FLAG_DEBUG_RESWEEP):
        ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=10, flags=flags)
        got = ctx.consensus(batch)
        assert got == oracle_batch(batch, 6, 500, 10)
        assert _check(ctx, got, exp) > 0


def test_upload_run_fetch_and_min_weight(gpu_ctx_factory):
    """The three-step path, a second run of the same context, min_weight below min_cov."""
    batch = synth.make_batch(5, 1600, 12, seed=3)
    ctx = gpu_ctx_factory(min_cov=6, min_len=300, trim=50, min_weight=3, flags=SUP)
    ctx.upload(batch)
    exp = st.batch_support(batch, 6, 300, 50, 3)
    for _ in range(2):
        ctx.run()
        got = ctx.fetch()
        assert _check(ctx, got, exp) > 0


def _pre_targets(rng, n=4, local_flank=False):
    rc = bytes.maketrans(b"ACGT", b"TGCA")

    def mutate(t, sub=0.03, ins=0.08, dele=0.05):
        q = bytearray()
        for c in t:
            u = rng.random()
            if u < dele:
                continue
            q.append(c if u > dele + sub else b"ACGT"[rng.integers(0, 4)])
            while rng.random() < ins:
                q.append(b"ACGT"[rng.integers(0, 4)])
        return bytes(q)

    targets = []
    for ti in range(n):
        tlen = int(rng.integers(1200, 2400))
        target = bytes(b"ACGT"[j] for j in rng.integers(0, 4, tlen))
        recs = []
        for r in range(9):
            s = int(rng.integers(0, tlen // 4)); e = int(rng.integers(3 * tlen // 4, tlen + 1))
            strand = b"+-"[(r + ti) % 2:(r + ti) % 2 + 1]
            tseq = target[s:e] if strand == b"+" else target[s:e].translate(rc)[::-1]
            qseq = mutate(tseq)
            if local_flank:
                qseq = bytes(b"ACGT"[j] for j in rng.integers(0, 4, 30)) + qseq
            recs.append((s if strand == b"+" else tlen - e, strand, qseq, tseq))
        targets.append((tlen, recs))
    return targets


@pytest.mark.parametrize("local", [False, True])
def test_consensus_pre(gpu_ctx_factory, local):
    """dagcon_consensus_pre, global and local: the support of the graph its own alignments make (the twin takes them
    from dagcon_align / align_ends on a context of the same mode, then the start arithmetic of SimpleAligner.cpp:51-62)."""
    rng = np.random.default_rng(61 + local)
    targets = _pre_targets(rng, local_flank=local)
    flags = SUP | (capi.FLAG_LOCAL_ALIGN if local else 0)
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=flags)
    got = ctx.consensus_pre(targets)
    sup = ctx.base_support()
    actx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_LOCAL_ALIGN if local else 0)
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    n = 0
    for ti, (tlen, recs) in enumerate(targets):
        alns_dev = actx.align([(q, t) for _, _, q, t in recs])
        ends = actx.align_ends()
        alns = []
        for (tstart, strand, q, t), (qa, ta), (_, _, tb, te) in zip(recs, alns_dev, ends):
            st_, en = tstart + tb, tstart + te
            if strand == b"-":
                st_ = tlen - en
                qa, ta = qa.translate(rc)[::-1], ta.translate(rc)[::-1]
            alns.append((st_ + 1, qa, ta))
        exp = st.consensus_target_support(tlen, alns, 500, 50, 6)
        assert got[ti] == [s[:3] for s in exp]
        assert [(w.tolist(), d.tolist()) for w, d in sup[ti]] == [(s[3], s[4]) for s in exp]
        n += sum(len(s[2]) for s in exp)
    assert n > 0


def test_failed_target_has_no_entries(gpu_ctx_factory):
    """One non-conforming target: no segments and no entries for it; the rest exact, at the same offsets as seq_blob."""
    batch = synth.make_batch(4, 1500, 12, seed=19)
    bad = batch.select(range(4))
    bad.aln_start = batch.aln_start.copy()
    bad.aln_start[int(batch.aln_begin[1])] = np.uint32(900)             # an alignment of target 1 runs past tlen
    ctx = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP)
    got = ctx.consensus(bad, strict=False)
    assert ctx.target_status[1] == -4 and got[1] == []
    exp = st.batch_support(batch, 6, 500, 50)
    exp[1] = []
    assert _check(ctx, got, exp) > 0
    w, d = ctx.fetch_support_raw()
    assert w.size == d.size == sum(len(s) for segs in got for _, _, s in segs)


def test_state_errors(gpu_ctx_factory):
    """DAGCON_ERR_STATE: without the flag, before a fetch, under STOP_AFTER_BUILD / STOP_AFTER_MERGE; the flag is
    accepted by dagcon_create, undefined bits still are not."""
    batch = synth.make_batch(2, 1200, 10, seed=2)
    plain = gpu_ctx_factory(min_cov=6, min_len=500, trim=50)
    plain.consensus(batch)
    with pytest.raises(capi.DagconError) as e:
        plain.fetch_support_raw()
    assert e.value.code == -8
    fresh = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP)
    with pytest.raises(capi.DagconError) as e:
        fresh.fetch_support_raw()
    assert e.value.code == -8
    fresh.upload(batch)
    fresh.run()
    with pytest.raises(capi.DagconError) as e:                           # run, not fetched yet
        fresh.fetch_support_raw()
    assert e.value.code == -8
    fresh.fetch()
    assert fresh.fetch_support_raw()[0].size > 0
    for stop in (capi.FLAG_STOP_AFTER_BUILD, capi.FLAG_STOP_AFTER_MERGE):
        c = gpu_ctx_factory(min_cov=6, min_len=500, trim=50, flags=SUP | stop)
        assert c.consensus(batch) == [[], []]
        with pytest.raises(capi.DagconError) as e:
            c.fetch_support_raw()
        assert e.value.code == -8
    for bad in (8, 128, 1 << 20):
        with pytest.raises(capi.DagconError) as e:
            capi.Context(flags=SUP | bad)
        assert e.value.code == -5


def test_support_values_are_bounded(gpu_ctx_factory):
    """Deep pileups (thousands of alignments): depth <= K, weight <= K + 1, and the twin's values exactly."""
    rng = np.random.default_rng(7)
    alns, bb = random_target(rng, 30, 3000, sub=0.05, ins=0.08, dele=0.05, full_span=False)
    batch = batch_from_targets([(30, alns, bb)])
    ctx = gpu_ctx_factory(min_cov=6, min_len=0, trim=0, min_weight=0, flags=SUP)
    got = ctx.consensus(batch)
    assert _check(ctx, got, st.batch_support(batch, 6, 0, 0, 0)) > 0
    for w, d in ctx.base_support()[0]:
        assert int(d.max()) <= 3000 and int(w.max()) <= 3001
    assert oracle.consensus_target(30, alns, 0, 0, 0) == got[0]
