"""The figures DESIGN.md quotes for dagcon_place and qsense (needs a GPU).

  1. dagcon_place all against all for 150 reads x 10 kb (22,350 ordered pairs): wall time of the call, host copies
     included, median of --reps after one warm-up call.
  2. qsense d --fofn on --clusters clusters x 40 reads x 2 kb, 4 rounds: wall seconds and consensus bases per second.

Reads carry tests/util.py's random_target error profile (3 % substitutions, 12 % insertion runs, 6 % deletions) and
both strands.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def reads_of(rng, template, n, sub=0.03, ins=0.12, dele=0.06, ext=0.3):
    """n reads of template (bytes), vectorised: start in the first and end in the last 5 %, either strand."""
    T = np.frombuffer(template, np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for _ in range(n):
        a, b = int(rng.integers(0, len(T) // 20 + 1)), len(T) - int(rng.integers(0, len(T) // 20 + 1))
        x = T[a:b]
        u = rng.random(x.size)
        keep = u >= dele
        base = np.where(u < dele + sub, acgt[rng.integers(0, 4, x.size)], x)
        n_ins = np.where(rng.random(x.size) < ins, rng.geometric(1 - ext, x.size), 0)
        emit = keep.astype(np.int64) + n_ins
        idx = np.repeat(np.arange(x.size), emit)
        within = np.arange(idx.size) - np.repeat(np.cumsum(emit) - emit, emit)
        r = np.where((within == 0) & keep[idx], base[idx], acgt[rng.integers(0, 4, idx.size)]).tobytes()
        out.append(r if rng.random() < 0.5 else r.translate(_RC)[::-1])
    return out


def probe_place(reps):
    from pbdagcon_amd import capi
    rng = np.random.default_rng(5)
    reads = reads_of(rng, rng.choice(list(b"ACGT"), 10000).astype(np.uint8).tobytes(), 150)
    pairs = [(j, i) for i in range(150) for j in range(150) if j != i]
    ctx = capi.Context()
    try:
        ctx.place(reads, pairs)
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            got = ctx.place(reads, pairs)
            ms.append((time.perf_counter() - t) * 1e3)
    finally:
        ctx.close()
    placed = float((np.frombuffer(got["strand"], np.uint8) != ord(".")).mean())
    return {"place_pairs": len(pairs), "place_ms_median": float(np.median(ms)), "place_ms_min": float(min(ms)),
            "place_placed_fraction": placed}


def probe_qsense(n_clusters, depth, tlen, n_iter):
    rng = np.random.default_rng(9)
    with tempfile.TemporaryDirectory() as d:
        lines = []
        for g in range(n_clusters):
            t = rng.choice(list(b"ACGT"), tlen).astype(np.uint8).tobytes()
            path = os.path.join(d, f"c{g}.fa")
            with open(path, "wb") as f:
                for i, r in enumerate(reads_of(rng, t, depth)):
                    f.write(b">r%d\n%s\n" % (i, r))
            lines.append(path)
        fofn = os.path.join(d, "clusters.fofn")
        with open(fofn, "w") as f:
            f.write("\n".join(lines) + "\n")
        cli = os.path.join(ROOT, "pbdagcon_amd", "bin", "qsense")
        t = time.perf_counter()
        out = subprocess.run([cli, "d", "--fofn", fofn, "-d", d, "--n_iter", str(n_iter)], capture_output=True, text=True)
        wall = time.perf_counter() - t
        if out.returncode != 0:
            raise SystemExit(f"qsense failed ({out.returncode}): {out.stderr[-2000:]}")
        seqs = [ln for ln in open(os.path.join(d, "g_consensus.fa")).read().split("\n") if ln and not ln.startswith(">")]
    bases = sum(len(s) for s in seqs)
    return {"qsense_clusters": n_clusters, "qsense_reads_per_cluster": depth, "qsense_template": tlen,
            "qsense_rounds": n_iter, "qsense_wall_s": wall, "qsense_records": len(seqs), "qsense_consensus_bases": bases,
            "qsense_bases_per_s": bases / wall, "qsense_warnings": out.stderr.count("warning")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = probe_place(a.reps)
    res.update(probe_qsense(a.clusters, 40, 2000, 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
