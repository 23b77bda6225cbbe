"""Cost of the per-base support (DAGCON_FLAG_BASE_SUPPORT): the same resident batch through a context without and
one with the flag, alternating, in one process.  Shapes: configs[1] (1,000 targets x 10 kb x 40x, full spans: the lane
walk) and the config-5 shape (400 mixed-length targets of 2-40 kb x 30x, partial spans, real backbones: the piece walk).
Per shape and mode: best device ms_bestpath / ms_total over the reps, and the wall time of dagcon_fetch (plus
dagcon_fetch_support with the flag).  Prints one JSON line per shape.  Kernel times: run it under
rocprofv3 --kernel-trace --stats.
    python tools/support_probe.py [reps] [shape ...]      shapes: c1 c5 (default both)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
shapes = sys.argv[2:] or ["c1", "c5"]


def batch_of(shape):
    if shape == "c1":
        return synth.make_batch(1000, 10000, 40, seed=1000), dict(min_cov=6, min_len=500, trim=50)
    tl = np.random.default_rng(5).integers(2000, 40000, 400)
    return (synth.make_batch(400, 0, 30, seed=8000, min_span=0.6, tlens=tl, with_backbone=True),
            dict(min_cov=6, min_len=500, trim=10))


for shape in shapes:
    batch, kw = batch_of(shape)
    ctxs = {"off": capi.Context(**kw), "on": capi.Context(flags=capi.FLAG_BASE_SUPPORT, **kw)}
    for c in ctxs.values():
        c.upload(batch)
    stats = {k: {"ms_bestpath": [], "ms_total": [], "ms_fetch_wall": []} for k in ctxs}
    seqs = {}
    for rep in range(reps + 1):                              # (rep 0: warm-up, not recorded)
        for k, c in ctxs.items():
            c.run()
            c.sync()
            t0 = time.perf_counter()
            r = capi.Results()
            c._chk(c.L.dagcon_fetch(c.h, C.byref(r)))
            if k == "on":
                s = capi.Support()
                c._chk(c.L.dagcon_fetch_support(c.h, C.byref(s)))
                assert s.n == r.seq_bytes
            wall = (time.perf_counter() - t0) * 1e3
            seqs[k] = capi.Context.results_to_py(r)           # (per target: the blob's layout is the device's order)
            if rep:
                t = c.timings()
                stats[k]["ms_bestpath"].append(t["ms_bestpath"])
                stats[k]["ms_total"].append(t["ms_total"])
                stats[k]["ms_fetch_wall"].append(wall)
    best = {k: {m: round(min(v), 3) for m, v in d.items()} for k, d in stats.items()}
    print(json.dumps({
        "shape": shape, "targets": batch.n_targets, "reps": reps,
        "consensus_bases": sum(len(x) for segs in seqs["on"] for _, _, x in segs),
        "same_consensus": seqs["on"] == seqs["off"], "best": best,
        "bestpath_on_over_off": round(best["on"]["ms_bestpath"] / best["off"]["ms_bestpath"], 3),
        "total_on_over_off": round(best["on"]["ms_total"] / best["off"]["ms_total"], 3),
        "fetch_extra_ms": round(best["on"]["ms_fetch_wall"] - best["off"]["ms_fetch_wall"], 3),
        "all": {k: {m: [round(x, 3) for x in v] for m, v in d.items()} for k, d in stats.items()},
    }), flush=True)
    for c in ctxs.values():
        c.close()
