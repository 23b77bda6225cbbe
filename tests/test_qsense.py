"""bin/qsense (the q-sense.py command line) on synthetic clusters, on the GPU.

Exactness: the CLI's output equals the same steps redone here, twin placement (tests/place_twin.py) -> dagcon_align
with local ends -> the CPU oracle's consensus with the seed as the real backbone.  Accuracy: identity to the true
template.  Coverage: a cluster below --min_cov gets a warning and no record, the others are unaffected."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_twin as tw  # noqa: E402
from test_place import _cluster_reads, _qsense, rand_seq  # noqa: E402
from util import batch_from_targets, oracle_batch  # noqa: E402

MIN_VOTES, FLANK, TRIM = 3, 96, 10


def write_fasta(path, seqs, name="r"):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">%s%d\n%s\n" % (name.encode(), i, s))


def read_fasta(path):
    recs = []
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            recs.append([line[1:].decode(), b""])
        elif line:
            recs[-1][1] += line
    return [(n, s) for n, s in recs]


def pipeline(ctx, clusters, seeds, n_iter, min_cov=8, max_cov=60, max_n_reads=150, min_len=100):
    """qsense's rounds (host/qsense_main.cpp) redone: twin placement, device alignment, oracle consensus."""
    reads = [c[:max_n_reads] for c in clusters]
    G = len(reads)
    if seeds is None:                                    # d: all against all
        seeds = []
        for g in range(G):
            n = len(reads[g])
            pairs = [(j, i) for i in range(n) for j in range(n) if j != i]
            pl = tw.place_pairs(reads[g], pairs)
            score = np.zeros(n, np.int64)
            for a, (_, i) in enumerate(pairs):
                score[i] += max(int(pl["votes_fwd"][a]), int(pl["votes_rev"][a]))
            seeds.append(reads[g][int(np.argmax(score))])
    seed = list(seeds)
    active, cns = [True] * G, [None] * G
    for _ in range(n_iter):
        act = [g for g in range(G) if active[g]]
        if not act:
            break
        jobs = []
        for g in act:
            idx = tw.TargetIndex(seed[g], 12, 4)
            res = [tw.place(r, seed[g], 12, 4, idx) for r in reads[g]]
            keep = [a for a, r in enumerate(res) if r[2] != "." and max(r[0], r[1]) >= MIN_VOTES]
            keep.sort(key=lambda a: -max(res[a][0], res[a][1]))
            keep = keep[:max_cov]
            if len(keep) < min_cov:
                active[g] = False
                continue
            for a in keep:
                q = tw.rc(reads[g][a]) if res[a][2] == "-" else reads[g][a]
                w0, w1 = max(0, res[a][3] - FLANK), min(len(seed[g]), res[a][4] + FLANK)
                if w1 > w0:
                    jobs.append((g, w0, q, seed[g][w0:w1]))
        alns = ctx.align([(q, t) for _, _, q, t in jobs]) if jobs else []
        ends = ctx.align_ends() if jobs else []
        per = {g: [] for g in act if active[g]}
        for (g, w0, _, _), (qa, ta), e in zip(jobs, alns, ends):
            if qa:
                per[g].append((w0 + e[2] + 1, qa, ta))
        tg = []
        for g in list(per):
            if len(per[g]) < min_cov:
                active[g] = False
            else:
                tg.append(g)
        if not tg:
            continue
        batch = batch_from_targets([(len(seed[g]), per[g], seed[g]) for g in tg], with_backbone=True)
        out = oracle_batch(batch, min_cov, min_len, TRIM, min_cov)
        for g, segs in zip(tg, out):
            if not segs:
                active[g] = False
                continue
            best = max(range(len(segs)), key=lambda s: (len(segs[s][2]), -s))
            c = segs[best][2]
            if c == seed[g]:
                active[g] = False
            seed[g] = cns[g] = c
    return seeds, cns


def make_clusters(rng, n, tlen, depth):
    out = []
    for _ in range(n):
        t = rand_seq(rng, tlen)
        out.append((t, _cluster_reads(rng, t, depth)))
    return out


def run_cli(tmp_path, mode, clusters, refs=None, extra=()):
    lines = []
    for g, (_, reads) in enumerate(clusters):
        fa = tmp_path / f"c{g}.fa"
        write_fasta(fa, reads)
        line = str(fa)
        if mode == "r":
            rf = tmp_path / f"c{g}_ref.fa"
            write_fasta(rf, [refs[g]], "ref")
            line += " " + str(rf)
        lines.append(line)
    fofn = tmp_path / "clusters.fofn"
    fofn.write_text("\n".join(lines) + "\n")
    out = subprocess.run([_qsense(), mode, "--fofn", str(fofn), "-d", str(tmp_path), "-o", "cns.fasta", *extra],
                         capture_output=True, text=True, timeout=300)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["d", "r"])
def test_qsense_equals_the_steps_redone(tmp_path, mode, gpu_ctx_factory):
    from pbdagcon_amd import capi
    rng = np.random.default_rng(21 if mode == "d" else 22)
    clusters = make_clusters(rng, 4, 1500, 24)
    refs = [tw.rc(t) if g % 2 else t for g, (t, _) in enumerate(clusters)] if mode == "r" else None
    out = run_cli(tmp_path, mode, clusters, refs, ["--n_iter", "2"])
    assert out.returncode == 0, out.stderr
    ctx = gpu_ctx_factory(min_cov=8, min_len=100, trim=TRIM, flags=capi.FLAG_LOCAL_ALIGN)
    seeds, cns = pipeline(ctx, [r for _, r in clusters], refs, 2)
    assert all(c for c in cns), "every cluster should reach a consensus"
    exp = b"".join(b">consensus/%d\n%s\n" % (g, c) for g, c in enumerate(cns) if c)
    assert (tmp_path / "cns.fa").read_bytes() == exp
    if mode == "d":
        assert (tmp_path / "cns_ref.fa").read_bytes() == b"".join(b">consensus_ref/%d\n%s\n" % (g, s) for g, s in enumerate(seeds))
    else:
        assert not (tmp_path / "cns_ref.fa").exists()


def identity(ctx, c: bytes, template: bytes):
    """Matches per column of the consensus's local alignment (a context with FLAG_LOCAL_ALIGN) to the template, and
    the share of the template it covers.  As qsense aligns a read: oriented and placed first, then aligned inside the
    placed window, so that the band is centred on the consensus's own diagonal (the template's ends, where fewer than
    --min_cov reads start, lie outside the consensus and would pull a band over the whole template off it)."""
    _, _, strand, t0, t1 = tw.place(c, template)
    x = tw.rc(c) if strand == "-" else c
    w0, w1 = max(0, t0 - FLANK), min(len(template), t1 + FLANK)
    (qa, ta), = ctx.align([(x, template[w0:w1])])
    (_, _, a0, a1), = ctx.align_ends()
    q, t = np.frombuffer(qa, np.uint8), np.frombuffer(ta, np.uint8)
    return float((q == t).sum()) / max(len(q), 1), (a1 - a0) / len(template)


@pytest.mark.gpu
def test_qsense_accuracy_3kb_at_40x(tmp_path, gpu_ctx_factory):
    rng = np.random.default_rng(31)
    template, reads = make_clusters(rng, 1, 3000, 40)[0]
    from pbdagcon_amd import capi
    ctx = gpu_ctx_factory(min_cov=8, min_len=100, trim=TRIM, flags=capi.FLAG_LOCAL_ALIGN)
    for mode, want in (("r", 0.99), ("d", 0.98)):
        d = tmp_path / mode
        d.mkdir()
        out = run_cli(d, mode, [(template, reads)], [template])
        assert out.returncode == 0, out.stderr
        (_, c), = read_fasta(d / "cns.fa")
        ident, cover = identity(ctx, c, template)
        print(f"{mode}: consensus of {len(c)} bases, identity {ident:.4f} over {cover:.3f} of the {len(template)}-base template")
        assert ident >= want and cover >= 0.85, (mode, ident, cover)   # trim 10 takes a few bases off each end a round


@pytest.mark.gpu
def test_qsense_cluster_below_min_cov(tmp_path):
    rng = np.random.default_rng(41)
    clusters = make_clusters(rng, 3, 1200, 20)
    clusters[1] = (clusters[1][0], clusters[1][1][:5])
    out = run_cli(tmp_path, "d", clusters, extra=["--n_iter", "2"])
    assert out.returncode == 0, out.stderr
    assert "cluster 1" in out.stderr and "warning" in out.stderr and "cluster 0" not in out.stderr
    got = dict(read_fasta(tmp_path / "cns.fa"))
    assert sorted(got) == ["consensus/0", "consensus/2"]
    alone = tmp_path / "alone"
    alone.mkdir()
    out = run_cli(alone, "d", [clusters[0], clusters[2]], extra=["--n_iter", "2"])
    assert out.returncode == 0, out.stderr
    got2 = dict(read_fasta(alone / "cns.fa"))
    assert got2 == {"consensus/0": got["consensus/0"], "consensus/1": got["consensus/2"]}
