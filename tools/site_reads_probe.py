"""Cost of the site reads (dagcon_set_site_reads): the configs[1] batch of bench.py (1,000 targets x 10 kb x 40x as
strings), one context in one process, `reps` repetitions after a warm-up, every value kept.  The pile-up is on in every
mode, at the default thresholds of pbdagcon --sites (2 alignments, 0.2 of the depth):
    pile             dagcon_set_pileup alone: what the switch is compared with
    reads            and dagcon_set_site_reads without the split
    phase            and the split, 8 rounds
Wall time of dagcon_consensus + dagcon_fetch_pileup_sites, the device pipeline's time (ms_total) and its bestPath stage
(ms_bestpath: the pile-up's and the site reads' kernels run at its end), the sites, and with the switch on the taken
alignments, the entries, how the alignments were labelled, and the wall time of one dagcon_fetch_site_reads.  Prints one
JSON line (kept as profiles/site_reads/probe_<mode>.json).  The probe times stages, not kernels: the kernels' own times
come from a run of this script under rocprofv3 --kernel-trace --stats, one run per mode.
    python tools/site_reads_probe.py [mode] [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "phase"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
assert mode in ("pile", "reads", "phase")
batch = synth.make_batch(n, 10000, 40, seed=1000)
c_struct = batch.c_struct()
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(2, 200000)
if mode != "pile":
    ctx.set_site_reads(mode == "phase")
wall, dev, stage, n_sites, reruns = [], [], [], 0, 0
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    r = capi.Results()
    t0 = time.perf_counter()
    ctx._chk(ctx.L.dagcon_consensus(ctx.h, C.byref(c_struct), C.byref(r)))
    s = capi.PileupSites()
    ctx._chk(ctx.L.dagcon_fetch_pileup_sites(ctx.h, C.byref(s)))
    n_sites = int(s.site_begin[int(s.n_targets)])
    dt = (time.perf_counter() - t0) * 1e3
    if rep == 0:
        reruns = ctx.timings()["reruns"]
    else:
        wall.append(round(dt, 3)); dev.append(round(ctx.timings()["ms_total"], 3)); stage.append(round(ctx.timings()["ms_bestpath"], 3))
out = {"probe": "site_reads", "mode": mode, "targets": n, "reps": reps, "reruns_of_the_warm_up": reruns, "sites_at_2_and_0.2": n_sites,
       "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage}
if mode != "pile":
    t0 = time.perf_counter()
    sr = ctx.site_reads()
    out["fetch_site_reads_wall_ms_with_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["taken_alignments"] = int(sr["aln_tgt"].size)
    out["entries"] = int(sr["ent_site"].size)
    out["entries_with_ins"] = int((sr["ent_code"] >> 3).sum())
    if sr["hap"] is not None:
        out["hap_0_1_2"] = [int((sr["hap"] == k).sum()) for k in range(3)]
        out["phase_minus_0_plus"] = [int((sr["phase"] == k).sum()) for k in (-1, 0, 1)]
ctx.close()
print(json.dumps(out), flush=True)
