"""Windows against the whole target, on the CPU: the same reads on a 60 kb target, once as windows of 10 kb (twin cut,
oracle per window, twin stitch: tests/window_twin.py) and once whole (the oracle on the expanded strings).  Prints the
number of differing bases between the two by an exact (banded, unit-cost) alignment, where they lie relative to the
joins, and the identity of each to the synthetic truth.

    python tools/window_vs_whole.py [tlen] [W] [O] [coverage] [read_len]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cigar_twin as ct  # noqa: E402
import oracle  # noqa: E402
import test_windows as tw  # noqa: E402
import window_twin as wt  # noqa: E402


def align(a, b, band=200):
    """Unit-cost edit distance of a and b inside a band, and the positions in a of its edits (substitutions,
    deletions from a, insertions counted at the a position in front of them)."""
    a = np.frombuffer(a, np.uint8); b = np.frombuffer(b, np.uint8)
    n, m = a.size, b.size
    assert abs(n - m) < band // 2
    w = 2 * band + 1
    INF = 1 << 30
    idx = np.arange(w)
    prev = np.full(w, INF, np.int64)
    # cell (i, j) lives at column j - i + band
    j0 = idx - band
    prev[(j0 >= 0) & (j0 <= m)] = j0[(j0 >= 0) & (j0 <= m)]
    back = np.zeros((n + 1, w), np.uint8)                          # 0 diag, 1 up (a base alone), 2 left (b base alone)
    back[0] = 2
    for i in range(1, n + 1):
        j = idx - band + i
        ok = (j >= 0) & (j <= m)
        bj = np.where((j >= 1) & (j <= m), b[np.clip(j - 1, 0, m - 1)], 0)
        diag = np.where((j >= 1) & ok, prev + (bj != a[i - 1]), INF)      # (i-1, j-1) is the same column
        up = np.full(w, INF, np.int64); up[:-1] = prev[1:] + 1            # (i-1, j) is one column to the right
        base = np.minimum(diag, up)
        base[~ok] = INF
        cur = np.minimum.accumulate(base - idx) + idx
        cur[~ok] = INF
        back[i] = np.where(cur == diag, 0, np.where(cur == up, 1, 2))
        prev = cur
    i, c = n, m - n + band
    dist = int(prev[c])
    edits = []
    while i > 0 or (c - band + i) > 0:
        mv = back[i, c]
        if mv == 0:
            if a[i - 1] != b[c - band + i - 1]:
                edits.append(i - 1)
            i -= 1
        elif mv == 1:
            edits.append(i - 1); i -= 1; c += 1
        else:
            edits.append(i); c -= 1
    assert len(edits) == dist
    return dist, sorted(edits)


def main():
    tlen, W, O, cov, rl = (int(x) for x in (sys.argv[1:6] + ["60000", "10000", "1000", "30", "2000"][len(sys.argv) - 1:]))
    rng = np.random.default_rng(5)
    truth = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), tlen))
    recs = tw.mapped_reads(rng, truth, tlen * cov // rl, rl)
    win_txt = tw.windowed_expected(["t"], [(truth, recs)], W, O, 6, 500, 50, False)
    lines = win_txt.split(b"\n")
    heads, seqs = lines[0:-1:2], lines[1::2]
    alns = [ct.expand(p, q, truth, ops) for p, q, ops in recs]
    whole = oracle.consensus_target(tlen, alns, 500, 50, 6)
    res = dict(tlen=tlen, W=W, O=O, coverage=cov, read_len=rl, windowed_records=[h.decode() for h in heads],
               whole_segments=[(r0, r1) for r0, r1, _ in whole])
    if len(seqs) == 1 and len(whole) == 1:
        wseq, t0 = seqs[0], int(heads[0].split(b"/")[1].split(b"_")[0])
        hseq = whole[0][2]
        d, edits = align(wseq, hseq)
        # a windowed base's target coordinate, to within the indels in front of it: t0 + its index
        near = [min(abs(t0 + e - k * W) for k in range(1, -(-tlen // W))) for e in edits]
        res.update(windowed_len=len(wseq), whole_len=len(hseq), differing_bases=d,
                   distance_of_each_to_the_nearest_join=near,
                   joins_with_a_difference_within_100=len({round((t0 + e) / W) for e, x in zip(edits, near) if x <= 100}))
        # to the truth: the stretch of it the windowed record names; the whole consensus against the same stretch
        t1 = int(heads[0].split(b"_")[-1])
        dw, _ = align(wseq, truth[t0:t1])
        dh, _ = align(hseq, truth[t0:t1], band=400)
        res.update(windowed_identity=1 - dw / max(len(wseq), t1 - t0), whole_identity=1 - dh / max(len(hseq), t1 - t0),
                   windowed_edits_to_truth=dw, whole_edits_to_truth=dh)
    os.makedirs(os.path.join(ROOT, "profiles", "windows"), exist_ok=True)
    json.dump(res, open(os.path.join(ROOT, "profiles", "windows", "window_vs_whole.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
