"""Cost of the alleles at the sites (dagcon_set_site_alleles): the configs[1] batch of bench.py (1,000 targets x 10 kb x
40x as strings), one context in one process, `reps` repetitions after a warm-up, every value kept.  The pile-up and the
site reads are on in every mode, at the default thresholds of pbdagcon --sites (2 alignments, 0.2 of the depth):
    reads            dagcon_set_site_reads without the split: what the switch is compared with
    alleles          and dagcon_set_site_alleles
    phase            the site reads with the split: what the next mode is compared with
    phase_alleles    and dagcon_set_site_alleles, with the counts per label
Wall time of dagcon_consensus + dagcon_fetch_pileup_sites, the device pipeline's time (ms_total) and its bestPath stage
(ms_bestpath: the pile-up's, the site reads' and the alleles' kernels run at its end), the sites, and with the switch on
the alleles, how many sites have one, two, three and more, the deepest table, and the wall time of one
dagcon_fetch_site_alleles.  Prints one JSON line (kept as profiles/site_alleles/probe_<mode>.json).  The probe times
stages, not kernels: the kernels' own times come from a run of this script under rocprofv3 --kernel-trace --stats, one run
per mode.
    python tools/alleles_probe.py [mode] [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "alleles"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
assert mode in ("reads", "alleles", "phase", "phase_alleles")
batch = synth.make_batch(n, 10000, 40, seed=1000)
c_struct = batch.c_struct()
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(2, 200000)
ctx.set_site_reads(mode.startswith("phase"))
ctx.set_site_alleles(mode.endswith("alleles"))
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
out = {"probe": "site_alleles", "mode": mode, "targets": n, "reps": reps, "reruns_of_the_warm_up": reruns, "sites_at_2_and_0.2": n_sites,
       "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage}
if mode.endswith("alleles"):
    t0 = time.perf_counter()
    sa = ctx.site_alleles()
    out["fetch_site_alleles_wall_ms_with_the_site_reads_and_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
    nd = np.diff(sa["al_begin"]).astype(np.int64)
    out["entries"] = int(sa["ent_allele"].size)
    out["alleles"] = int(sa["key"].size)
    out["sites_with_1_2_3_more_alleles"] = [int((nd == 1).sum()), int((nd == 2).sum()), int((nd == 3).sum()), int((nd > 3).sum())]
    out["most_alleles_at_a_site"] = int(nd.max(initial=0))
    out["entries_of_the_first_allele"] = int((sa["ent_allele"] == 0).sum())
    out["long_alleles"] = int(((sa["key"] >> np.uint64(60)) & np.uint64(1)).sum())
    out["empty_alleles"] = int((sa["key"] == 0).sum())
    if sa["hap_count"] is not None:
        out["entries_by_label_1_2_0"] = [int(x) for x in sa["hap_count"].astype(np.int64).sum(axis=0)]
ctx.close()
print(json.dumps(out), flush=True)
