"""Cost of the joined sites (dagcon_set_site_join): the configs[1] batch of bench.py (1,000 targets x 10 kb x 40x as strings),
one context in one process, `reps` repetitions after a warm-up, every value kept.  The pile-up, the site reads and the
alleles are on in every mode, at the default thresholds of pbdagcon --sites (2 alignments, 0.2 of the depth):
    alleles          dagcon_set_site_alleles without the split: what the switch is compared with
    join             and dagcon_set_site_join
    phase_alleles    the alleles with the split: what the next mode is compared with
    phase_join       and dagcon_set_site_join, with the counts per label
Wall time of dagcon_consensus + dagcon_fetch_pileup_sites, the device pipeline's time (ms_total) and its bestPath stage
(ms_bestpath: the outputs' kernels run at its end), the sites, and with the switch on the runs, the joined alleles, the runs
of more than one site, the opaque alleles, the device bytes the join holds per entry and per site, and the wall time of one
dagcon_fetch_joined_sites.  Prints one JSON line (kept as profiles/site_join/probe_<mode>.json).  The probe times stages, not
kernels: the kernels' own times come from a run of this script under rocprofv3 --kernel-trace --stats, one run per mode.
    python tools/join_probe.py [mode] [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "join"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
assert mode in ("alleles", "join", "phase_alleles", "phase_join")
batch = synth.make_batch(n, 10000, 40, seed=1000)
c_struct = batch.c_struct()
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(2, 200000)
ctx.set_site_reads(mode.startswith("phase"))
ctx.set_site_alleles(True)
ctx.set_site_join(mode.endswith("join"))
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
out = {"probe": "site_join", "mode": mode, "targets": n, "reps": reps, "reruns_of_the_warm_up": reruns, "sites_at_2_and_0.2": n_sites,
       "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage}
if mode.endswith("join"):
    t0 = time.perf_counter()
    js = ctx.joined_sites()
    out["fetch_joined_sites_wall_ms_with_the_alleles_the_site_reads_and_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
    sa = ctx.site_alleles()
    m = np.diff(js["run_begin"]).astype(np.int64)
    nd = np.diff(js["jal_begin"]).astype(np.int64)
    out["entries"] = int(js["ent_joined"].size)
    out["runs"] = int(m.size)
    out["joined_alleles"] = int(js["key"].size)
    out["runs_of_more_than_one_site"] = int((m > 1).sum())
    out["runs_of_16_sites"] = int((m == 16).sum())
    out["longest_run"] = int(m.max(initial=0))
    out["most_joined_alleles_of_a_run"] = int(nd.max(initial=0))
    out["spanning_members"] = int(js["spanning"].astype(np.int64).sum())
    out["partial_members"] = int(js["partial"].astype(np.int64).sum())
    out["entries_of_partial_members"] = int((js["ent_joined"] == 0xFFFF).sum())
    # opaque: a nibble of 15 among the run's m, or a long allele at one of its sites
    which = np.repeat(np.arange(m.size), nd)
    opaque = np.zeros(js["key"].size, bool)
    for j in range(16):
        c = ((js["key"] >> np.uint64(4 * (15 - j))) & np.uint64(15)).astype(np.int64)
        inside = j < m[which]
        site = np.minimum(js["run_begin"][:-1].astype(np.int64)[which] + j, max(sa["al_begin"].size - 2, 0))
        at_ = np.minimum(sa["al_begin"].astype(np.int64)[site] + np.minimum(c, 14), max(sa["key"].size - 1, 0))
        is_long = ((sa["key"][at_] >> np.uint64(60)) & np.uint64(1)).astype(bool) if sa["key"].size else np.zeros(c.size, bool)
        opaque |= inside & ((c == 15) | is_long)
    out["opaque_joined_alleles"] = int(opaque.sum())
    # what a run holds on the device for the join alone (api_outputs.hip.h, join_room), and the compact tables of the fetch
    out["device_bytes_per_entry_of_the_arena"] = 8 + 4 + 4 + 2 + 2
    out["device_bytes_per_site_of_the_arena"] = 4 + 4 + 4 + 8 + 4 + 4 + 8
    out["device_bytes_per_joined_allele_at_the_fetch"] = 16
    if js["hap_count"] is not None:
        out["spanning_members_by_label_1_2_0"] = [int(x) for x in js["hap_count"].astype(np.int64).sum(axis=0)]
ctx.close()
print(json.dumps(out), flush=True)
