"""dagcon_align_panels (dazcon --trace-panels) against dagcon_align (the end-to-end aligner) on the same overlaps:
synthetic A reads, B reads cut from them at ~15 % error (5 % deletions, 5 % substitutions, 5 % insertions) with
their TRUE traces (B bases and differences per panel of tspace A bases).  A sample is checked against the CPU twin
(tests/panel_twin.py) byte for byte, and every panel's distance against the differences its trace records.
Prints one JSON line.  Kernel times: run it under rocprofv3 --kernel-trace --stats.

    python tools/panel_probe.py [--pairs 3840] [--len 50000] [--tspace 100] [--check 6] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

from pbdagcon_amd import capi
import panel_twin

ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_pair(rng, L, tspace):
    """(B interval, A interval, panels [(A bases, B bases)], per-panel differences)."""
    a = ACGT[rng.integers(0, 4, L)]
    u = rng.random(L)
    keep = u >= 0.05
    sub = (u >= 0.05) & (u < 0.10)
    b_main = np.where(sub, ACGT[(np.searchsorted(ACGT, a) + rng.integers(1, 4, L)) % 4], a)
    ins = rng.random(L) < 0.05
    ins[-1] = False
    # per A base: its own B base (if kept), then an inserted one (if any)
    out_n = keep.astype(np.int64) + ins
    pos = np.cumsum(out_n) - out_n
    b = np.empty(int(out_n.sum()), np.uint8)
    b[pos[keep]] = b_main[keep]
    b[pos[ins] + keep[ins]] = ACGT[rng.integers(0, 4, int(ins.sum()))]
    pan = np.arange(L) // tspace
    bcnt = np.bincount(pan, weights=out_n).astype(np.int64)
    diffs = np.bincount(pan, weights=(~keep).astype(np.int64) + sub + ins).astype(np.int64)
    alen = np.bincount(pan).astype(np.int64)
    return b.tobytes(), a.tobytes(), list(zip(alen.tolist(), bcnt.tolist())), diffs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3840)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--tspace", type=int, default=100)
    ap.add_argument("--check", type=int, default=6, help="pairs compared with the CPU twin")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the dagcon_align timing")
    args = ap.parse_args()
    rng = np.random.default_rng(2024)
    t0 = time.perf_counter()
    pairs, panels, diffs = [], [], []
    for _ in range(args.pairs):
        q, t, p, d = make_pair(rng, args.len, args.tspace)
        pairs.append((q, t)); panels.append(p); diffs.append(d)
    gen_s = time.perf_counter() - t0
    ctx = capi.Context(min_cov=1, min_len=0, trim=0)
    res = dict(pairs=args.pairs, len=args.len, tspace=args.tspace, panels=sum(len(p) for p in panels),
               cells=int(sum(x * y for p in panels for x, y in p)), gen_s=round(gen_s, 1))
    try:
        ctx.align_panels(pairs[:4], panels[:4])                 # warm: module load, first allocations
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got, dist = ctx.align_panels(pairs, panels)
            ms.append((time.perf_counter() - t0) * 1e3)
        res["panels_call_ms"] = [round(x, 1) for x in ms]
        res["panels_dropped"] = ctx.align_dropped()
        res["over_trace"] = int(sum(int((np.array(dd) > d).sum()) for dd, d in zip(dist, diffs)))
        bad = 0
        for a in rng.choice(args.pairs, size=min(args.check, args.pairs), replace=False):
            qa, ta, dd = panel_twin.align_overlap(pairs[a][0], pairs[a][1], panels[a])
            bad += got[a] != (qa, ta) or dist[a] != dd
        res["twin_checked"], res["twin_mismatch"] = min(args.check, args.pairs), bad
        res["columns"] = int(sum(len(x) for x, _ in got))
        del got, dist
        if not args.no_end_to_end:
            ctx.align(pairs[:4])
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                e2e = ctx.align(pairs)
                ms.append((time.perf_counter() - t0) * 1e3)
            res["end_to_end_call_ms"] = [round(x, 1) for x in ms]
            res["end_to_end_dropped"] = ctx.align_dropped()
            res["end_to_end_columns"] = int(sum(len(x) for x, _ in e2e))
    finally:
        ctx.close()
    print(json.dumps(res), flush=True)
    return 0 if res.get("twin_mismatch", 1) == 0 and res.get("over_trace", 1) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
