"""One context across entry points, across batch sizes, and closed in every state.

The other GPU tests reuse a context within one entry point.  Here one context goes through all of them in turn (every
named buffer set, the page-locked result buffers and the status block are then shared by calls that size them
differently), grows and shrinks, and is destroyed before an upload, after one, after a run and after a refused call.
Every result is compared with the same call on a context of its own."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import cigar_twin as ct
import cs_twin as cst
import paf_files as pf
from util import oracle_batch

pytestmark = pytest.mark.gpu

MIN_COV, MIN_LEN, TRIM = 6, 500, 50


def _flags():
    from pbdagcon_amd import capi
    return capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS


def _ctx():
    from pbdagcon_amd import capi
    return capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM, flags=_flags())


def _record_targets(batch):
    """[(target bases, [(pos, read bases, ops)])] of a synthetic batch made with its backbone."""
    out = []
    for t in range(batch.n_targets):
        o = int(batch.backbone_off[t])
        bb = batch.backbone[o:o + int(batch.tlen[t])].tobytes()
        out.append((bb, [ct.compress(s, q, tt, bb) for s, q, tt in batch.target_alignments(t)]))
    return out


def _cigar(targets):
    from pbdagcon_amd import capi
    return capi.HostCigarBatch(**ct.records_to_arrays(targets))


def _cs(targets):
    from pbdagcon_amd import capi
    return capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs])
                                          for bb, recs in targets])


def _consensus_result(ctx, got, edits):
    """Everything a consensus call leaves behind, in a form that does not depend on where a target lies in seq_blob."""
    sup = [[(w.tobytes(), d.tobytes()) for w, d in segs] for segs in ctx.base_support()]
    out = {"segments": got, "status": ctx.target_status.tolist(), "support": sup}
    if edits:
        ed = ctx.edits()
        so = ctx._segs[1].astype(np.int64)
        ed["c_off"] = ed["c_off"].astype(np.int64) - np.repeat(so, np.diff(ed["edit_begin"].astype(np.int64)))
        out["edits"] = {k: v.tobytes() for k, v in ed.items()}
    out["positions"] = [[p.tobytes() for p in segs] for segs in ctx.base_positions()]      # (edits on: fetched on demand)
    return out


@pytest.fixture(scope="module")
def calls():
    """(name, edits switch before the call, call) in the order one context takes them."""
    from pbdagcon_amd import capi, synth
    rng = np.random.default_rng(5)
    batch = synth.make_batch(3, 1000, 20, seed=1)
    hb = synth.make_batch(3, 1000, 20, seed=1, with_backbone=True)
    rec = []
    for bb, recs in _record_targets(hb):                            # a few target bases changed under the records' M ops:
        bb = bytearray(bb)                                          # the consensus then differs from its target there
        for x in range(100, len(bb), 170):
            bb[x] = b"ACGT"[(b"ACGT".index(bb[x]) + 1) % 4]
        rec.append((bytes(bb), recs))
    cigar, cs = _cigar(rec), _cs(rec)
    windows = capi.HostWindows.tiled([len(bb) for bb, _ in rec], 600, 100)
    pairs = [(q, t) for _, q, t in ac.tie_pairs_at(rng, 130)] + [(ac.mutate(rng, t), t) for t in (ac.rand(rng, 700), ac.rand(rng, 40))]
    # overlaps of a few trace-point panels each (A bases, B bases per panel), one of them with an empty panel
    p_pairs, p_panels = [], []
    for shapes in ([(100, None)] * 3, [(37, None), (100, None), (0, 5)], [(300, None), (129, None)]):
        ts = [ac.rand(rng, m) for m, _ in shapes]
        qs = [ac.mutate(rng, t) if n is None else ac.rand(rng, n) for t, (_, n) in zip(ts, shapes)]
        p_pairs.append((b"".join(qs), b"".join(ts)))
        p_panels.append([(len(t), len(q)) for t, q in zip(ts, qs)])
    seqs = [ac.rand(rng, 300)]
    seqs += [ac.mutate(rng, seqs[0][20:280]), ac.mutate(rng, seqs[0])[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")), ac.rand(rng, 200)]
    place_pairs = [(1, 0), (2, 0), (3, 0), (1, 2)]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    pre = []
    for ti in range(2):
        target = ac.rand(rng, 900 + 100 * ti)
        recs = []
        for r in range(8):
            s, e = 10 * r, len(target) - 7 * r
            strand = b"+-"[r % 2:r % 2 + 1]
            tseq = target[s:e] if strand == b"+" else target[s:e].translate(rc)[::-1]
            recs.append((s if strand == b"+" else len(target) - e, strand, ac.mutate(rng, tseq), tseq))
        pre.append((len(target), recs))

    def cons(f, edits):
        return lambda ctx: _consensus_result(ctx, f(ctx), edits)
    return [
        ("align", None, lambda ctx: (ctx.align(pairs), ctx.align_ends(), ctx.align_dropped())),
        ("align_panels", None, lambda ctx: ctx.align_panels(p_pairs, p_panels)),
        ("place", None, lambda ctx: {k: bytes(v) if isinstance(v, bytes) else v.tobytes() for k, v in ctx.place(seqs, place_pairs).items()}),
        ("consensus_pre", None, cons(lambda ctx: ctx.consensus_pre(pre), False)),
        ("consensus", None, cons(lambda ctx: ctx.consensus(batch), False)),
        ("consensus_cigar", False, cons(lambda ctx: ctx.consensus_cigar(cigar), False)),
        ("consensus_cigar_windows", True, cons(lambda ctx: ctx.consensus_cigar_windows(cigar, windows), True)),
        ("consensus_cs", True, cons(lambda ctx: ctx.consensus_cs(cs), True)),
        ("consensus again", None, cons(lambda ctx: ctx.consensus(batch), False)),
    ]


def _run(ctx, switch, call):
    if switch is not None:
        ctx.set_edits(switch)
    return call(ctx)


def test_one_context_through_every_entry_point_twice(calls, monkeypatch):
    monkeypatch.setenv("DAGCON_POISON", "15")
    fresh = []
    for name, switch, call in calls:
        ctx = _ctx()
        try:
            fresh.append(_run(ctx, switch, call))
        finally:
            ctx.close()
    assert sum(len(s) for segs in fresh[4]["segments"] for _, _, s in segs) > 2000          # (the inputs do give a consensus)
    assert len(fresh[6]["edits"]["t_pos"]) > 0 and any(fresh[3]["segments"])
    ctx = _ctx()
    try:
        for rnd in range(2):
            for (name, switch, call), want in zip(calls, fresh):
                assert _run(ctx, switch, call) == want, (rnd, name)
    finally:
        ctx.close()


def test_growth_and_shrinking(monkeypatch):
    """Small, about four times the targets and the length, small again: the buffers sized by the batch are allocated
    anew for the second and are larger than needed for the third."""
    from pbdagcon_amd import synth
    monkeypatch.setenv("DAGCON_POISON", "15")
    small = _record_targets(synth.make_batch(2, 600, 12, seed=3, with_backbone=True))
    large = _record_targets(synth.make_batch(8, 2400, 12, seed=4, with_backbone=True))
    batches = [_cigar(small), _cigar(large), _cigar(small)]

    def call(ctx, b):
        ctx.set_edits(True)
        return _consensus_result(ctx, ctx.consensus_cigar(b), True)
    fresh = []
    for b in batches[:2]:
        ctx = _ctx()
        try:
            fresh.append(call(ctx, b))
        finally:
            ctx.close()
    fresh.append(fresh[0])
    assert all(any(segs for segs in f["segments"]) for f in fresh)
    ctx = _ctx()
    try:
        for k, (b, want) in enumerate(zip(batches, fresh)):
            assert call(ctx, b) == want, k
    finally:
        ctx.close()


def test_destroy_in_every_state(oracle_lib):
    from pbdagcon_amd import capi, synth
    batch = synth.make_batch(3, 1000, 20, seed=1)
    _ctx().close()                                                  # created and closed at once
    ctx = _ctx()
    ctx.upload(batch)                                               # an upload without a run
    ctx.close()
    ctx = _ctx()
    ctx.upload(batch)
    ctx.run()                                                       # a run without a fetch (destroy waits for it)
    ctx.close()
    ctx = _ctx()                                                    # a call the host-side checks refuse: nothing launched
    off, ln = np.array([10], np.uint64), np.array([5], np.uint32)
    blob, out = np.zeros(8, np.uint8), np.zeros(32, np.uint8)
    rc = ctx.L.dagcon_align(ctx.h, 1, off.ctypes.data, ln.ctypes.data, off.ctypes.data, ln.ctypes.data, blob.ctypes.data, 8,
                            blob.ctypes.data, 8, np.zeros(1, np.uint64).ctypes.data, out.ctypes.data, out.ctypes.data,
                            np.zeros(1, np.uint32).ctypes.data)
    assert rc == -1 and capi.ERR_NAMES[rc] == "DAGCON_ERR_INVALID_ARG"
    assert ctx.L.dagcon_last_error(ctx.h) == b"pair 0 runs past its blob"
    ctx.close()
    ctx.L.dagcon_destroy(C.c_void_p())                              # NULL is accepted
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=TRIM)
    try:
        assert ctx.consensus(batch) == oracle_batch(batch, MIN_COV, MIN_LEN, TRIM)
    finally:
        ctx.close()
