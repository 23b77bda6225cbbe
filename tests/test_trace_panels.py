"""dazcon --trace-panels and dagcon_align_panels: every overlap of a .las re-aligned inside its trace-point panels
(where the reference runs DALIGNER's Compute_Trace_PTS, DazAlnProvider.cpp:304-351; DALIGNER is not in the reference
tree, so the panel aligner's tie-breaks are this build's own and parity is unpinned).  tests/panel_twin.py is the CPU
twin: checked here against a plain scalar DP, then the device against it byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import daz_files
import daz_model as dm
import panel_twin as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pbdagcon_amd", "bin", "dazcon")
MAX_SIDE = 512                                               # DAGCON_PANEL_MAX_SIDE


def _cli():
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return CLI


def _scalar(t: bytes, q: bytes):
    """The panel aligner as a triple loop: the same recurrence and tie rule, one cell at a time."""
    m, n = len(t), len(q)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    K = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(n + 1):
        D[0][j], K[0][j] = j, 1
    for i in range(1, m + 1):
        D[i][0], K[i][0] = i, 2
        for j in range(1, n + 1):
            best, k = None, None
            for cand, kk in ((D[i - 1][j - 1] + (t[i - 1] != q[j - 1]), 0), (D[i][j - 1] + 1, 1), (D[i - 1][j] + 1, 2)):
                if best is None or cand < best:
                    best, k = cand, kk
            D[i][j], K[i][j] = best, k
    qa, ta, i, j = bytearray(), bytearray(), m, n
    while i or j:
        k = K[i][j]
        qa.append(q[j - 1] if k != 2 else 45); ta.append(t[i - 1] if k != 1 else 45)
        i -= k != 1; j -= k != 2
    return bytes(qa[::-1]), bytes(ta[::-1]), D[m][n]


def _seq(rng, n, alpha=b"ACGT"):
    return bytes(alpha[k] for k in rng.integers(0, len(alpha), n))


def _mutate(rng, s: bytes):
    out = bytearray()
    for ch in s:
        u = rng.random()
        if u < 0.04:
            continue
        out.append(ch if u > 0.07 else b"ACGT"[rng.integers(0, 4)])
        if rng.random() < 0.05:
            out.append(b"ACGT"[rng.integers(0, 4)])
    return bytes(out)


# ---------------------------------------------------------------- CPU

def test_twin_equals_scalar_dp():
    rng = np.random.default_rng(5)
    shapes = [(0, 0), (0, 3), (4, 0), (1, 1), (0, 1), (1, 0)]
    for x in range(3000):
        m, n = shapes[x] if x < len(shapes) else (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
        alpha = [b"A", b"AC", b"ACG", b"ACGT"][x % 4]
        t, q = _seq(rng, m, alpha), _seq(rng, n, alpha)
        assert pt.align_panel(t, q) == _scalar(t, q), (t, q)


def test_twin_columns_and_distance():
    """The twin's columns spell the two panels, and their cost is the distance it reports."""
    rng = np.random.default_rng(6)
    for _ in range(300):
        t = _seq(rng, int(rng.integers(0, 60)))
        q = _mutate(rng, t)
        qa, ta, d = pt.align_panel(t, q)
        assert len(qa) == len(ta) and qa.replace(b"-", b"") == q and ta.replace(b"-", b"") == t
        assert sum(x != y for x, y in zip(qa, ta)) == d


@pytest.mark.parametrize("tspace", [100, 37])
def test_twin_distance_at_most_the_known_alignment(tspace):
    """Panels cut from known alignments (daz_model.synth_dataset): an optimal panel costs no more than the known one."""
    rng = np.random.default_rng(7)
    _, _, model = dm.synth_dataset(rng, n_targets=3)
    checked = 0
    for recs in model.values():
        for r in recs:
            # the known columns, cut where the A position crosses a multiple of tspace
            a_pos, cut = r["abpos"], [[]]
            for ct, cq in zip(r["tstr"], r["qstr"]):
                if ct != "-" and a_pos > r["abpos"] and a_pos % tspace == 0 and cut[-1]:
                    cut.append([])
                cut[-1].append((ct, cq))
                a_pos += ct != "-"
            for cols in cut:
                t = "".join(c for c, _ in cols if c != "-").encode()
                q = "".join(c for _, c in cols if c != "-").encode()
                known = sum(x != y for x, y in cols)
                assert pt.align_panel(t, q)[2] <= known
                checked += 1
    assert checked > 100


def _las_with_trace(tmp_path, rng, tspace=100, n_targets=3, cov=8, tlen=1500, comp=True, zero_diffs=False, big_insert=False):
    """Reads + overlaps with TRUE traces: every B read is cut from its A read with known edits, and each trace-point
    panel's B bases and differences are counted as they are made.  Returns reads, overlaps (with B' = the B read as the
    overlap sees it, and its trace), db path, las path."""
    reads, ovl = [], []
    for _ in range(n_targets):
        a = _seq(rng, tlen + int(rng.integers(0, 300)))
        ai = len(reads)
        reads.append(a)
        for k in range(cov):
            abpos = int(rng.integers(0, len(a) // 3))
            if k == 1:
                abpos -= abpos % tspace                             # one overlap starts on a panel boundary
            aepos = int(rng.integers(2 * len(a) // 3, len(a) + 1))
            npan = (aepos - 1) // tspace - abpos // tspace + 1
            bcnt, dcnt, b = [0] * npan, [0] * npan, bytearray()
            for i in range(abpos, aepos):
                p = i // tspace - abpos // tspace
                if big_insert and k == 0 and p == npan // 2 and i % tspace == 0 and i > abpos:
                    ins = _seq(rng, MAX_SIDE + 40 - tspace)         # this panel gets more than MAX_SIDE B bases
                    b += ins; bcnt[p] += len(ins); dcnt[p] += len(ins)
                u = rng.random()
                if u < 0.04:
                    dcnt[p] += 1
                    continue
                ch = a[i] if u > 0.07 else b"ACGT"[rng.integers(0, 4)]
                dcnt[p] += ch != a[i]
                b.append(ch); bcnt[p] += 1
                if rng.random() < 0.05 and i + 1 < aepos:
                    b.append(b"ACGT"[rng.integers(0, 4)]); bcnt[p] += 1; dcnt[p] += 1
            fl, fr = _seq(rng, int(rng.integers(0, 40))), _seq(rng, int(rng.integers(0, 40)))
            whole = fl + bytes(b) + fr
            flag = int(comp and rng.random() < 0.5)
            bi = len(reads)
            reads.append(dm.revcomp(whole.decode()).encode() if flag else whole)
            trace = [v for p in range(npan) for v in (0 if zero_diffs else dcnt[p], bcnt[p])]
            ovl.append(dict(aread=ai, bread=bi, flags=flag, abpos=abpos, aepos=aepos, bbpos=len(fl), bepos=len(fl) + len(b),
                            diffs=sum(dcnt), trace=trace, b_prime=whole))
    db, las = str(tmp_path / "reads.db"), str(tmp_path / "ovl.las")
    daz_files.write_db(db, [r.decode() for r in reads])
    daz_files.write_las(las, ovl, tspace)
    return reads, ovl, db, las


def test_cli_refuses_trace_whose_b_bases_do_not_add_up(tmp_path):
    rng = np.random.default_rng(8)
    reads, ovl, db, las = _las_with_trace(tmp_path, rng, n_targets=1, cov=3)
    ovl[1]["trace"][1] += 1
    daz_files.write_las(las, ovl, 100)
    out = subprocess.run([_cli(), "--trace-panels", "-a", las, "-s", db, "-c", "1"], capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 1 and "overlap 2" in err and "B bases add up to" in err, err


def test_cli_refuses_trace_with_wrong_pair_count(tmp_path):
    rng = np.random.default_rng(9)
    reads, ovl, db, las = _las_with_trace(tmp_path, rng, n_targets=1, cov=3)
    ovl[2]["trace"] = ovl[2]["trace"][:-2]
    ovl[2]["trace"][1] += ovl[2]["bepos"] - ovl[2]["bbpos"] - sum(ovl[2]["trace"][1::2])   # (the B bases still add up)
    daz_files.write_las(las, ovl, 100)
    out = subprocess.run([_cli(), "--trace-panels", "-a", las, "-s", db, "-c", "1"], capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 1 and "overlap 3" in err and "pairs" in err and "panels of 100" in err, err


def test_cli_refuses_trace_panels_with_text_input(tmp_path):
    s, a = tmp_path / "reads.txt", tmp_path / "ovl.txt"
    s.write_text("1 ACGT\n2 ACGT\n")
    a.write_text("O 1 2 0 0 4 0 4 0 ACGT ACGT\n")
    out = subprocess.run([_cli(), "--trace-panels", "-a", str(a), "-s", str(s)], capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 1 and "--trace-panels needs a DALIGNER .las file" in err, err


# ---------------------------------------------------------------- GPU

def _panel_batch(rng):
    """Overlaps of 1 to 500 panels: empty sides, short first panels, panels of exactly MAX_SIDE, every kernel instance."""
    pairs, panels = [], []

    def overlap(shapes, alpha=b"ACGT", related=True):
        qs, ts, ps = [], [], []
        for m, n in shapes:
            t = _seq(rng, m, alpha)
            q = _mutate(rng, t) if related and n is None else _seq(rng, n if n is not None else m, alpha)
            qs.append(q); ts.append(t); ps.append((len(t), len(q)))
        pairs.append((b"".join(qs), b"".join(ts)))
        panels.append(ps)

    overlap([(0, 0)]); overlap([(0, 7)]); overlap([(9, 0)]); overlap([(0, 0), (5, 5), (0, 3), (4, 0)])
    overlap([(MAX_SIDE, MAX_SIDE)], b"AC"); overlap([(MAX_SIDE, MAX_SIDE), (MAX_SIDE, 1)]); overlap([(480, None), (MAX_SIDE, None)]); overlap([(1, MAX_SIDE), (MAX_SIDE, 0)])
    for m, n in [(100, 129), (129, 100), (200, 300), (300, 200), (256, 256), (257, 257), (400, 120), (120, 400), (64, 511)]:
        overlap([(m, n), (m, None)])
    for _ in range(60):                                             # a short first panel, then tspace-sized ones
        k = int(rng.integers(1, 40))
        overlap([(int(rng.integers(1, 100)), None)] + [(100, None)] * k)
    for _ in range(200):                                            # tiny panels with ties everywhere
        overlap([(int(rng.integers(0, 12)), int(rng.integers(0, 12)))] * int(rng.integers(1, 6)), b"AC", related=False)
    overlap([(int(rng.integers(0, 30)), None) for _ in range(500)])
    return pairs, panels


@pytest.mark.gpu
def test_align_panels_equals_twin(gpu_ctx_factory):
    rng = np.random.default_rng(11)
    pairs, panels = _panel_batch(rng)
    big = len(pairs)
    pairs.append((_seq(rng, 600), _seq(rng, 200)))                  # B side of its second panel over MAX_SIDE
    panels.append([(100, 50), (100, MAX_SIDE + 1), (0, 37)])
    assert sum(len(p) for p in panels) >= 2000
    ctx = gpu_ctx_factory(min_cov=1, min_len=0, trim=0)
    got, dists = ctx.align_panels(pairs, panels)
    assert ctx.align_dropped() >= 1
    assert got[big] == (b"", b"") and dists[big] == [-1, -1, -1]
    assert sum(max(max(x, y) for x, y in ps) == MAX_SIDE for ps in panels) >= 3
    for a, ((q, t), ps) in enumerate(zip(pairs, panels)):
        if max(max(x, y) for x, y in ps) > MAX_SIDE:              # not aligned, whatever its other panels are
            assert got[a] == (b"", b"") and dists[a] == [-1] * len(ps), f"overlap {a}"
            continue
        qa, ta, d = pt.align_overlap(q, t, ps)
        assert got[a] == (qa, ta), f"overlap {a}: {ps[:4]}"
        assert dists[a] == d, f"overlap {a}"


@pytest.mark.gpu
def test_align_panels_refuses_panels_that_do_not_add_up(gpu_ctx_factory):
    from pbdagcon_amd import capi
    ctx = gpu_ctx_factory(min_cov=1, min_len=0, trim=0)
    with pytest.raises(capi.DagconError, match="INVALID_ARG"):
        ctx.align_panels([(b"ACGT", b"ACGT")], [[(2, 2), (1, 2)]])
    with pytest.raises(capi.DagconError, match="INVALID_ARG"):
        ctx.align_panels([(b"ACGT", b"ACGT")], [[(2, 2), (2, 1)]])


def _expected_alns(reads, ovl, tspace, max_hits=85):
    """The alignments dazcon --trace-panels hands to the consensus, per A read: hit selection by the model, every record
    aligned by the twin inside its panels -- or, when a panel has more than MAX_SIDE bases on a side, end to end by the
    -a aligner (oracle.banded_align is dagcon_align's twin)."""
    import oracle
    by_a, res = {}, {}
    for o in ovl:
        by_a.setdefault(o["aread"], []).append(o)
    for ai in sorted(by_a):
        a = reads[ai]
        hits = dm.group_hits(by_a[ai], len(a), {o["bread"]: len(reads[o["bread"]]) for o in by_a[ai]})
        alns = []
        for h in dm.sort_hits(hits, len(a), False)[:max_hits]:
            for r in h.records:
                ps = pt.trace_panels(r["abpos"], r["aepos"], r["trace"], tspace)
                q, t = r["b_prime"][r["bbpos"]:r["bepos"]], a[r["abpos"]:r["aepos"]]
                if max(max(x, y) for x, y in ps) > MAX_SIDE:
                    qa, ta = oracle.banded_align(q, t)
                else:
                    qa, ta, _ = pt.align_overlap(q, t, ps)
                alns.append((r["abpos"] + 1, qa, ta, r))
        res[ai] = alns
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("tspace", [100, 500])
def test_dazcon_trace_panels_dump_equals_twin(tmp_path, tspace):
    rng = np.random.default_rng(20 + tspace)
    reads, ovl, db, las = _las_with_trace(tmp_path, rng, tspace=tspace, n_targets=3, cov=8, tlen=1500 if tspace == 100 else 2600)
    assert any(o["flags"] for o in ovl) and any(o["abpos"] % tspace for o in ovl)
    assert any(max(o["trace"][1::2]) <= MAX_SIDE for o in ovl)
    out = subprocess.run([_cli(), "--trace-panels", "--dump-alns", "-a", las, "-s", db, "-c", "1"], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    exp = [b"%d\t%d\t%s\t%s\n" % (ai + 1, st, ta, qa) for ai, alns in _expected_alns(reads, ovl, tspace).items()
           for st, qa, ta, _ in alns]
    assert out.stdout == b"".join(exp)


@pytest.mark.gpu
def test_dazcon_trace_panels_end_to_end():
    """FASTA of dazcon --trace-panels = the CPU composition: twin alignments, the model's hit selection, the oracle's
    real-backbone consensus (as test_dazcon_on_las_and_db composes the end-to-end aligner's)."""
    import tempfile
    import oracle
    rng = np.random.default_rng(31)
    with tempfile.TemporaryDirectory() as d:
        from pathlib import Path
        reads, ovl, db, las = _las_with_trace(Path(d), rng, tspace=100, n_targets=4, cov=12, tlen=2500)
        out = subprocess.run([_cli(), "--trace-panels", "-a", las, "-s", db, "-c", "4", "-l", "500"], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    exp, well = [], 0
    for ai, alns in _expected_alns(reads, ovl, 100).items():
        if len(alns) < 4:
            continue
        for r0, r1, sq in oracle.consensus_target(len(reads[ai]), [(st, qa, ta) for st, qa, ta, _ in alns], 500, 10, 4,
                                                  backbone=reads[ai]):
            exp.append(b">%d/%d/%d_%d\n%s\n" % (ai + 1, well, r0, r1, sq))
            well += 1
    assert len(exp) >= 3 and out.stdout == b"".join(exp)


@pytest.mark.gpu
def test_dazcon_trace_panels_fallback_and_verbose(tmp_path):
    """An overlap with a panel over MAX_SIDE B bases is aligned end to end (dagcon_align, whose twin is
    oracle.banded_align) and counted on stderr; traces that claim 0 differences give a non-zero -v report."""
    import re
    rng = np.random.default_rng(41)
    reads, ovl, db, las = _las_with_trace(tmp_path, rng, tspace=400, n_targets=1, cov=4, tlen=2600, big_insert=True,
                                          zero_diffs=True)
    out = subprocess.run([_cli(), "--trace-panels", "--dump-alns", "-v", "-a", las, "-s", db, "-c", "1"], capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 0, err
    big = sum(max(o["trace"][1::2]) > MAX_SIDE for o in ovl)
    assert big >= 1 and max(ovl[0]["trace"][1::2]) > MAX_SIDE
    assert f"{big} overlaps have a trace-point panel over 512 bases and were aligned end to end" in err, err
    m = re.search(r"(\d+) of (\d+) trace-point panels came out with more differences", err)
    assert m and int(m.group(1)) > 0, err
    rows = out.stdout.split(b"\n")[:-1]
    alns = _expected_alns(reads, ovl, 400)[0]
    assert len(rows) == len(alns)
    for row, (st, qa, ta, r) in zip(rows, alns):
        assert row == b"1\t%d\t%s\t%s" % (st, ta, qa)
