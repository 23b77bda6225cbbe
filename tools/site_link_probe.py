"""Cost and effect of the site link (dagcon_set_site_link): the configs[1] batch of bench.py (1,000 targets x 10 kb x 40x as
strings) with the planted haplotypes of tools/hap_probe.py -- every second read of a target gets another base at one
position in every thousand -- at pbdagcon --sites' default thresholds (2 reads, 0.2 of the depth), where the synthetic reads'
own errors make some 350 sites a target and outvote the ten planted ones.  One context in one process, one mode a run,
`reps` repetitions after a warm-up, every value kept.  The pile-up, the site reads, the split and the tally are on in both
modes.
    off              the switch off: what it is compared with
    on               dagcon_set_site_link at its defaults: k_lk_kind, k_lk_bits and k_lk_pairs in front of k_sr_split
Prints one JSON line (kept as profiles/site_link/probe_<mode>.json).  The probe times stages and calls, not kernels: the
k_lk_* times come from a rocprofv3 --kernel-trace --stats run of their own.
    python tools/site_link_probe.py [mode] [reps] [targets]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "on"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
assert mode in ("off", "on")
GAP = 0x2D


def plant(batch, every=1000, seed=7):
    """tools/hap_probe.py's plant(), which also returns the planted positions of every target."""
    rng = np.random.default_rng(seed)
    other = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        other[a] = b
    changed, where = 0, []
    for t in range(batch.n_targets):
        tl = int(batch.tlen[t])
        pos = np.array([s + int(rng.integers(0, every)) for s in range(0, tl - every + 1, every)], np.int64)
        where.append(pos)
        for a in range(int(batch.aln_begin[t]) + 1, int(batch.aln_begin[t + 1]), 2):
            o, ln = int(batch.aln_off[a]), int(batch.aln_len[a])
            tcol = np.flatnonzero(batch.tstr[o:o + ln] != GAP)
            k = pos - (int(batch.aln_start[a]) - 1)
            k = k[(k >= 0) & (k < tcol.size)]
            cols = o + tcol[k]
            cols = cols[batch.qstr[cols] != GAP]
            batch.qstr[cols] = other[batch.tstr[cols]]
            changed += int(cols.size)
    return changed, where


batch = synth.make_batch(n, 10000, 40, seed=1000)
planted, where = plant(batch)
c_struct = batch.c_struct()
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(2, 200000)
ctx.set_site_reads(True)
ctx.set_hap_consensus()
if mode == "on":
    ctx.set_site_link()
out = {"probe": "site_link", "mode": mode, "targets": n, "reps": reps, "planted_bases": planted, "planted_positions": int(sum(p.size for p in where)),
       "site_min_count_and_ppm": [2, 200000], "link_opts": list((100000, 3, 2, 256)) if mode == "on" else None}
wall, dev, stage = [], [], []
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    r = capi.Results()
    t0 = time.perf_counter()
    ctx._chk(ctx.L.dagcon_consensus(ctx.h, C.byref(c_struct), C.byref(r)))
    dt = (time.perf_counter() - t0) * 1e3
    if rep == 0:
        out["reruns_of_the_warm_up"] = ctx.timings()["reruns"]
    else:
        wall.append(round(dt, 3)); dev.append(round(ctx.timings()["ms_total"], 3)); stage.append(round(ctx.timings()["ms_bestpath"], 3))
out.update({"wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage})
ht = ctx.hap_tally()
ps = ctx.pileup_sites()
out["sites"] = int(ps["pos"].size)
out["n1_n2_n0"] = [int(ht[k].sum()) for k in ("n1", "n2", "n0")]
out["split_targets"] = int(ht["split"].sum())
out["separating_sites"] = int(ht["n_sep"].sum())
out["agree_disagree"] = [int(ht["agree"].sum()), int(ht["disagree"].sum())]
sr = ctx.site_reads()
# reads labelled like their planted group, up to the swap of the two names, target by target
hap, tgt, src = sr["hap"].astype(np.int64), sr["aln_tgt"].astype(np.int64), sr["aln_src"].astype(np.int64)
parity = 1 + (src - batch.aln_begin[tgt].astype(np.int64)) % 2
as_planted = np.bincount(tgt, weights=(hap == parity), minlength=n).astype(np.int64)
swapped = np.bincount(tgt, weights=(hap == 3 - parity), minlength=n).astype(np.int64)
best = np.maximum(as_planted, swapped)
out["reads_labelled_like_their_planted_group"] = int(best.sum())
out["targets_with_all_40_reads_labelled_like_their_planted_group"] = int((best == 40).sum())
if mode == "on":
    t0 = time.perf_counter()
    sl = ctx.site_link()
    out["fetch_site_link_wall_ms_with_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["selected_sites"] = int(sl["linked"].sum())
    out["sites_with_a_partner"] = int((sl["partners"] > 0).sum())
    hit = 0
    for t in range(n):
        a, b = int(ps["site_begin"][t]), int(ps["site_begin"][t + 1])
        hit += int(np.isin(ps["pos"][a:b][sl["linked"][a:b] != 0], where[t]).sum())
    out["planted_positions_linked"] = hit
else:
    out["selected_sites"] = int(np.count_nonzero(sr["phase"]))          # (the sites that sign the split: those with a phase)
ctx.close()
print(json.dumps(out), flush=True)
