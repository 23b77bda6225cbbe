"""Cost of rating the records (dagcon_set_record_filter) next to the same call without a filter, copies inside the clock:
configs[1] (1,000 targets x 10 kb x 40x, pbdagcon_amd/synth.py with its backbone as the target sequence) through
dagcon_consensus_cigar with {1000000, 0} set (nothing is left out: the pipeline behind the expansion does the same work)
and with no filter, alternating in one process, `reps` repetitions each after a warm-up, every value kept.  The
no-filter call's own run-to-run spread is the yardstick.  Prints one JSON line.  Kernel times (k_cigar_rate and
k_cigar_rate_sum next to k_cigar_expand): run it under rocprofv3 --kernel-trace --stats, in a run of its own.
    python tools/rate_probe.py [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_twin as ct  # noqa: E402
from pbdagcon_amd import capi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
cb = capi.HostCigarBatch(**ct.compress_batch(batch))
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
c_struct = cb.c_struct()
wall = {"plain": [], "rated": []}
res, stats = {}, None
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for kind in ("plain", "rated"):
        if kind == "rated":
            ctx.set_record_filter(1000000, 0)
        else:
            ctx.set_record_filter(None, None)
        r = capi.Results()
        t0 = time.perf_counter()
        rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(c_struct), C.byref(r))
        dt = (time.perf_counter() - t0) * 1e3
        ctx._chk(rc)
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
            if kind == "rated":
                stats = ctx.record_stats()
        else:
            wall[kind].append(round(dt, 3))
ctx.close()
cols = sum(int(stats[k].sum()) for k in ("match", "mismatch", "ins", "del"))
print(json.dumps({
    "probe": "record_filter", "targets": n, "reps": reps, "records": int(cb.n_records), "ops": int(cb.ops.size),
    "same_consensus": res["plain"] == res["rated"], "columns": cols,
    "error_rate": round(1.0 - int(stats["match"].sum()) / max(cols, 1), 4),
    "wall_ms": wall, "plain_spread_ms": round(max(wall["plain"]) - min(wall["plain"]), 3),
    "rated_minus_plain_ms": [round(a - b, 3) for a, b in zip(wall["rated"], wall["plain"])],
}), flush=True)
