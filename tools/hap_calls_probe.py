"""Cost of the hap calls (dagcon_set_hap_calls): the configs[1] batch of bench.py (1,000 targets x 10 kb x 40x) as records,
with planted haplotypes as in tools/hap_probe.py -- every second read of a target gets another base at one position in a
thousand -- and sites of at least 8 alignments and 0.35 of the depth (hap_probe.py says why not the defaults).  Two
contexts in one process, both with edits, edit support, pile-up, site reads, split and tally on; one of them with
dagcon_set_hap_calls.  Per repetition and context: the first run (not timed), then dagcon_upload_haps + run + sync + fetch,
timed, and the device pipeline of that derived run; the contexts alternate, `reps` repetitions after a warm-up, every value
kept.  With the switch off the derived run has no edits at all, so the difference is the edit kernels, their support and
k_hap_calls together; the kernels' own times come from a rocprofv3 --kernel-trace --stats run of this probe.
Prints one JSON line (kept as profiles/hap_calls/probe.json).
    python tools/hap_calls_probe.py [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_twin as ct  # noqa: E402
from pbdagcon_amd import capi, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
GAP = 0x2D


def plant(batch, every=1000, seed=7):
    """Every second alignment of a target reads another base at the target's planted positions (one per `every` bases,
    at a random place of each stretch).  Returns the number of bases changed."""
    rng = np.random.default_rng(seed)
    other = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        other[a] = b
    changed = 0
    for t in range(batch.n_targets):
        tl = int(batch.tlen[t])
        pos = np.array([s + int(rng.integers(0, every)) for s in range(0, tl - every + 1, every)], np.int64)
        for a in range(int(batch.aln_begin[t]) + 1, int(batch.aln_begin[t + 1]), 2):
            o, ln = int(batch.aln_off[a]), int(batch.aln_len[a])
            tcol = np.flatnonzero(batch.tstr[o:o + ln] != GAP)
            k = pos - (int(batch.aln_start[a]) - 1)
            k = k[(k >= 0) & (k < tcol.size)]
            cols = o + tcol[k]
            cols = cols[batch.qstr[cols] != GAP]
            batch.qstr[cols] = other[batch.tstr[cols]]
            changed += int(cols.size)
    return changed


batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
planted = plant(batch)
cb = capi.HostCigarBatch(**ct.compress_batch(batch))
c_struct = cb.c_struct()
ctxs = {}
for mode in ("off", "on"):
    c = capi.Context(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_POS)
    c.set_edits(True); c.set_edit_support(True)
    c.set_pileup(8, 350000); c.set_site_reads(True); c.set_hap_consensus()
    if mode == "on":
        c.set_hap_calls(True)
    ctxs[mode] = c
out = {"probe": "hap_calls", "targets": n, "reps": reps, "planted_bases": planted, "site_min_count_and_ppm": [8, 350000]}
wall = {m: [] for m in ctxs}
dev = {m: [] for m in ctxs}
stage = {m: [] for m in ctxs}
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for mode, c in ctxs.items():
        r = capi.Results()
        c._chk(c.L.dagcon_consensus_cigar(c.h, C.byref(c_struct), C.byref(r)))
        c._chk(c.L.dagcon_fetch_hap_tally(c.h, C.byref(capi.HapTally())))      # (its copies are not the second run's)
        t0 = time.perf_counter()
        c._chk(c.L.dagcon_upload_haps(c.h))
        c._chk(c.L.dagcon_run(c.h)); c._chk(c.L.dagcon_sync(c.h))
        c._chk(c.L.dagcon_fetch(c.h, C.byref(r)))
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            wall[mode].append(round(dt, 3)); dev[mode].append(round(c.timings()["ms_total"], 3)); stage[mode].append(round(c.timings()["ms_bestpath"], 3))
        if mode == "on" and rep == reps:
            t0 = time.perf_counter()
            hc = c.hap_calls()
            out["fetch_hap_calls_wall_ms_with_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
            out["derived_targets"] = int(r.n_targets)
            out["edits"] = int(hc["state"].size)
            out["states_nocover_het_clash_hom"] = np.bincount(hc["state"], minlength=4).tolist()
            out["reruns_of_the_last_derived_run"] = c.timings()["reruns"]
out.update({"second_run_wall_ms": wall, "second_run_device_pipeline_ms": dev, "second_run_bestpath_stage_ms": stage})
for c in ctxs.values():
    c.close()
print(json.dumps(out), flush=True)
