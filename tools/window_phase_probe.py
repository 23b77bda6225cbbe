"""Cost of the phase across windows (dagcon_set_window_phase): a windows batch of about the configs[1] volume of bench.py --
1,000 windows with cores of 10 kb at 40x, from 100 contigs of 100 kb cut with an overlap of 1,000 -- with planted haplotypes
as in tools/hap_probe.py (every second read of a contig reads another base at about one position in a thousand).  The
synthetic alignments go in as records (CIGAR ops from the strings' columns), so the records are cut to the windows on the
device as for pbdagcon --window.  One context in one process, one mode a run, `reps` repetitions after a warm-up, every
value kept.  The pile-up, the site reads and the split are on in both modes, with sites of at least 8 alignments and 0.35
of the depth (hap_probe.py says why).
    off              the switch off: what it is compared with
    on               dagcon_set_window_phase on: the device pipeline with k_wl_pairs, k_wl_scan and k_wl_apply behind the split
Prints one JSON line (kept as profiles/window_phase/probe_<mode>.json).  The probe times the pipeline and calls, not
kernels; those come from one rocprofv3 --kernel-trace --stats run of mode `on`.
    python tools/window_phase_probe.py [mode] [reps] [contigs] [contig length]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pbdagcon_amd import capi, synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "on"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 100
tlen = int(sys.argv[4]) if len(sys.argv) > 4 else 100000
assert mode in ("off", "on")
GAP = 0x2D
W, O = 10000, 1000


def plant(batch, every=1000, seed=7):
    """tools/hap_probe.py's: every second alignment of a target reads another base at the target's planted positions."""
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


def records(batch):
    """The batch of strings as the arrays of a dagcon_cigar_batch: M / I / D from the columns, the target from its own side."""
    T = batch.n_targets
    t_off, t_parts, pos, q_off, q_len, op_begin, ops, q_parts = [], [], [], [], [], [0], [], []
    tp = qp = 0
    for t in range(T):
        a0, a1 = int(batch.aln_begin[t]), int(batch.aln_begin[t + 1])
        tl = int(batch.tlen[t])
        tgt = np.full(tl, ord("N"), np.uint8)
        for a in range(a0, a1):
            o, ln = int(batch.aln_off[a]), int(batch.aln_len[a])
            q, ts = batch.qstr[o:o + ln], batch.tstr[o:o + ln]
            code = np.where(ts == GAP, 1, np.where(q == GAP, 2, 0)).astype(np.uint32)     # M 0, I 1, D 2
            cut = np.flatnonzero(np.diff(code)) + 1
            start = np.concatenate([[0], cut])
            run = np.diff(np.concatenate([start, [ln]])).astype(np.uint32)
            ops.append((run << 4) | code[start]); op_begin.append(op_begin[-1] + start.size)
            bases = q[q != GAP]
            s = int(batch.aln_start[a]) - 1
            tb = ts[ts != GAP]
            tgt[s:s + tb.size] = tb
            pos.append(s + 1); q_off.append(qp); q_len.append(bases.size); q_parts.append(bases); qp += bases.size
        t_off.append(tp); t_parts.append(tgt); tp += tl
    return dict(tlen=batch.tlen, t_off=np.array(t_off, np.uint64), rec_begin=batch.aln_begin, pos=np.array(pos, np.uint32),
                q_off=np.array(q_off, np.uint64), q_len=np.array(q_len, np.uint32), op_begin=np.array(op_begin, np.uint64),
                ops=np.concatenate(ops), t_blob=np.concatenate(t_parts), q_blob=np.concatenate(q_parts))


t0 = time.perf_counter()
batch = synth.make_batch(n, tlen, 40, seed=1000)
planted = plant(batch)
cb = capi.HostCigarBatch(**records(batch))
hw = capi.HostWindows.tiled([tlen] * n, W, O)
prep = time.perf_counter() - t0
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
ctx.set_pileup(8, 350000)
ctx.set_site_reads(True)
if mode == "on":
    ctx.set_window_phase()
out = {"probe": "window_phase", "mode": mode, "contigs": n, "contig_length": tlen, "windows": hw.n_windows, "window_and_overlap": [W, O], "reps": reps,
       "planted_bases": planted, "site_min_count_and_ppm": [8, 350000], "host_preparation_s": round(prep, 1)}
wall, dev, stage = [], [], []
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    t0 = time.perf_counter()
    ctx.upload_cigar_windows(cb, hw)
    t1 = time.perf_counter()
    ctx.run(); ctx.sync(); ctx.fetch()
    dt = (time.perf_counter() - t1) * 1e3
    tm = ctx.timings()
    if rep == 0:
        out["reruns_of_the_warm_up"] = tm["reruns"]
    else:
        wall.append(round(dt, 3)); dev.append(round(tm["ms_total"], 3)); stage.append(round(tm["ms_bestpath"], 3))
        out.setdefault("upload_wall_ms", []).append(round((t1 - t0) * 1e3, 3))
out.update({"run_sync_fetch_wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage})
sr = ctx.site_reads()
out["taken_alignments"] = int(sr["aln_tgt"].size)
out["labelled_alignments"] = int((sr["hap"] != 0).sum())
if mode == "on":
    t0 = time.perf_counter()
    wp = ctx.window_phase()
    out["fetch_window_phase_wall_ms_with_the_python_copy"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["blocks"] = int(np.unique(wp["block"]).size)
    out["flipped_windows"] = int(wp["flip"].sum())
    out["same_diff"] = [int(wp["same"].sum()), int(wp["diff"].sum())]
ctx.close()
print(json.dumps(out), flush=True)
