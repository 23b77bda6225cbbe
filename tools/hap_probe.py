"""Cost of the consensus per read group (dagcon_set_hap_consensus): the configs[1] batch of bench.py (1,000 targets x 10 kb
x 40x as strings) with planted haplotypes -- the synthetic reads carry none, so every second read of a target gets another
base at the same positions, about one in a thousand.  One context in one process, one mode a run, `reps` repetitions after
a warm-up, every value kept.  The pile-up, the site reads and the split are on in every mode, with sites of at least 8
alignments and 0.35 of the depth.  At pbdagcon --sites' defaults (2, 0.2) the synthetic reads' own errors make 346,276
sites in the 1,000 targets (profiles/site_reads/probe_phase.json), every read agrees with the seed at most of them, and the
ten planted sites a target are outvoted: a run of this probe at those thresholds gave n1, n2, n0 = 40000, 0, 0 and no
split target (profiles/hap_consensus/probe_tally_default_sites.json).
    off              the tally off: what the switch is compared with
    tally            dagcon_set_hap_consensus on: the device pipeline with k_hap_tally and k_hap_targets at its end
    haps             per repetition the first run (not timed), then dagcon_upload_haps + run + sync + fetch, timed
    host             what a caller does without it: the groups' strings gathered on the host (timed apart) and run through
                     dagcon_consensus, upload included
Prints one JSON line (kept as profiles/hap_consensus/probe_<mode>.json).  The probe times stages and calls, not kernels.
    python tools/hap_probe.py [mode] [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "tally"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
assert mode in ("off", "tally", "haps", "host")
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
            tcol = np.flatnonzero(batch.tstr[o:o + ln] != GAP)              # column of the k-th target base of the alignment
            k = pos - (int(batch.aln_start[a]) - 1)
            k = k[(k >= 0) & (k < tcol.size)]
            cols = o + tcol[k]
            cols = cols[batch.qstr[cols] != GAP]
            batch.qstr[cols] = other[batch.tstr[cols]]
            changed += int(cols.size)
    return changed


def group_batch(batch, hm):
    """The groups of a hap_map as a batch of strings of their own: what a caller gathers on the host today."""
    src = hm["aln_src"].astype(np.int64)
    lens = batch.aln_len[src].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    q = np.empty(int(offs[-1]), np.uint8)
    t = np.empty(int(offs[-1]), np.uint8)
    for i, a in enumerate(src):
        o = int(batch.aln_off[a])
        q[offs[i]:offs[i + 1]] = batch.qstr[o:o + lens[i]]
        t[offs[i]:offs[i + 1]] = batch.tstr[o:o + lens[i]]
    return capi.HostBatch(batch.tlen[hm["src_target"]], hm["aln_begin"], batch.aln_start[src], offs[:-1], lens, q, t)


batch = synth.make_batch(n, 10000, 40, seed=1000)
planted = plant(batch)
c_struct = batch.c_struct()
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(8, 350000)
ctx.set_site_reads(True)
if mode != "off":
    ctx.set_hap_consensus()
out = {"probe": "hap_consensus", "mode": mode, "targets": n, "reps": reps, "planted_bases": planted, "site_min_count_and_ppm": [8, 350000]}
wall, dev, stage = [], [], []


def first_run():
    r = capi.Results()
    t0 = time.perf_counter()
    ctx._chk(ctx.L.dagcon_consensus(ctx.h, C.byref(c_struct), C.byref(r)))
    return (time.perf_counter() - t0) * 1e3


if mode in ("off", "tally"):
    for rep in range(reps + 1):                              # (rep 0: warm-up, not recorded)
        dt = first_run()
        if rep == 0:
            out["reruns_of_the_warm_up"] = ctx.timings()["reruns"]
        else:
            wall.append(round(dt, 3)); dev.append(round(ctx.timings()["ms_total"], 3)); stage.append(round(ctx.timings()["ms_bestpath"], 3))
    out.update({"wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage})
    if mode == "tally":
        t0 = time.perf_counter()
        ht = ctx.hap_tally()
        out["fetch_hap_tally_wall_ms_with_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["split_targets"] = int(ht["split"].sum())
        out["separating_sites"] = int(ht["n_sep"].sum())
        out["agree_disagree"] = [int(ht["agree"].sum()), int(ht["disagree"].sum())]
        out["n1_n2_n0"] = [int(ht[k].sum()) for k in ("n1", "n2", "n0")]
else:
    first_run()
    ctx.upload_haps()
    hm = ctx.hap_map()
    out["groups"] = int(hm["label"].size)
    out["group_alignments"] = int(hm["aln_src"].size)
    bases = 0
    if mode == "host":
        t0 = time.perf_counter()
        gb = group_batch(batch, hm)
        out["gather_on_the_host_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["uploaded_bytes"] = int(2 * gb.qstr.size)
        g_struct = gb.c_struct()
        ctx.set_pileup(None); ctx.set_site_reads(None); ctx.set_hap_consensus(None)
    for rep in range(reps + 1):
        if mode == "haps":
            first_run()
            ctx._chk(ctx.L.dagcon_fetch_hap_tally(ctx.h, C.byref(capi.HapTally())))      # (its copies are not the second run's)
            r = capi.Results()
            t0 = time.perf_counter()
            ctx._chk(ctx.L.dagcon_upload_haps(ctx.h))
            ctx._chk(ctx.L.dagcon_run(ctx.h)); ctx._chk(ctx.L.dagcon_sync(ctx.h))
            ctx._chk(ctx.L.dagcon_fetch(ctx.h, C.byref(r)))
        else:
            r = capi.Results()
            t0 = time.perf_counter()
            ctx._chk(ctx.L.dagcon_consensus(ctx.h, C.byref(g_struct), C.byref(r)))
        dt = (time.perf_counter() - t0) * 1e3
        bases = int(r.seq_bytes)
        if rep:
            wall.append(round(dt, 3)); dev.append(round(ctx.timings()["ms_total"], 3))
    out.update({"second_run_wall_ms": wall, "second_run_device_pipeline_ms": dev, "consensus_bases": bases})
ctx.close()
print(json.dumps(out), flush=True)
