"""Cost of the pile-up (dagcon_set_pileup): the configs[1] batch of bench.py (1,000 targets x 10 kb x 40x as strings),
two contexts alternating in one process, `reps` repetitions each after a warm-up, every value kept:
    off              dagcon_consensus as bench.py calls it
    on               dagcon_set_pileup at the default thresholds of pbdagcon --sites (2 alignments, 0.2 of the depth):
                     the same call, then dagcon_fetch_pileup_sites
Wall time of each, the device pipeline's time (ms_total) and its bestPath stage (ms_bestpath: the memset and the four
pile-up kernels run at its end, so on minus off is what they add), the sites and the bytes they add to the fetch (a
24-byte record per site), the bytes and the wall time of one dagcon_fetch_pileup (16 bytes a position, copied only when
asked for), and whether the two contexts agree on the consensus.  Prints one JSON line (kept as
profiles/pileup/probe.json).  The probe times stages, not kernels: the kernels' own times come from a run of this
script under rocprofv3 --kernel-trace --stats, a run of its own.
    python tools/pileup_probe.py [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
batch = synth.make_batch(n, 10000, 40, seed=1000)
c_struct = batch.c_struct()
ctxs = {k: capi.Context(min_cov=6, min_len=500, trim=50) for k in ("off", "on")}
ctxs["on"].set_pileup(2, 200000)
wall = {k: [] for k in ctxs}
dev = {k: [] for k in ctxs}
stage = {k: [] for k in ctxs}
res, n_sites, reruns = {}, 0, {}
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for kind, ctx in ctxs.items():
        r = capi.Results()
        t0 = time.perf_counter()
        ctx._chk(ctx.L.dagcon_consensus(ctx.h, C.byref(c_struct), C.byref(r)))
        if kind == "on":
            s = capi.PileupSites()
            ctx._chk(ctx.L.dagcon_fetch_pileup_sites(ctx.h, C.byref(s)))
            n_sites = int(s.site_begin[int(s.n_targets)])
        dt = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
            reruns[kind] = ctx.timings()["reruns"]
        else:
            wall[kind].append(round(dt, 3))
            dev[kind].append(round(ctx.timings()["ms_total"], 3))
            stage[kind].append(round(ctx.timings()["ms_bestpath"], 3))
t0 = time.perf_counter()
pu = ctxs["on"].pileup()
t_counts = (time.perf_counter() - t0) * 1e3
depth = pu["counts"][:, :6].sum(axis=1, dtype="int64")
for c in ctxs.values():
    c.close()
print(json.dumps({
    "probe": "pileup", "targets": n, "reps": reps, "same_consensus": res["off"] == res["on"], "reruns_of_the_warm_up": reruns,
    "positions": int(pu["counts"].shape[0]), "positions_with_depth": int((depth > 0).sum()), "mean_depth": round(float(depth.mean()), 2),
    "sites_at_2_and_0.2": n_sites,
    "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage,
    "pileup_kernels_ms": [round(a - b, 3) for a, b in zip(stage["on"], stage["off"])],
    "pileup_wall_ms": [round(a - b, 3) for a, b in zip(wall["on"], wall["off"])],
    "fetched_bytes_for_the_sites": 24 * n_sites,
    "fetch_pileup_bytes": 16 * int(pu["counts"].shape[0]), "fetch_pileup_wall_ms_with_the_python_copy": round(t_counts, 3),
}), flush=True)
