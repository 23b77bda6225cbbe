"""Cost of the kept parts (dagcon_set_window_keep) on the derived batch of pbdagcon --hap-contigs: the windows batch of
tools/window_phase_probe.py -- 1,000 windows with cores of 10 kb plus 1,000 bases either side at 40x, from 100 contigs of
100 kb with planted haplotypes -- is run with the pile-up, the split, the window phase and the tally on; then its split
windows run again as their two read groups (dagcon_upload_haps_swapped with the windows' flip), which is the batch this
probe times.  One context in one process, one mode a run, `reps` repetitions after a warm-up, every value kept.
    off   the switch off.  The stitch's input comes the old way: the positions (4 bytes a base across the bus, copied by
          dagcon_fetch itself on a context without the edits, so their cost is in the run / sync / fetch wall time) and
          a scan over every base of every segment for i0 and i1.  The scan is timed as numpy's (two comparisons and two
          argmax a segment, C loops): DgStitch::add walks the same bases one by one on one thread
    on    the switch on: k_win_keep behind k_bp_join; the positions stay on the device; dagcon_fetch_window_keep (16 bytes a
          segment) and the record join
Both modes time the calls themselves (ctypes, no Python copy of the arrays) and the device pipeline of the derived batch.
Prints one JSON line (kept as profiles/hap_contigs/probe_<mode>.json).  The kernel's own time comes from one
rocprofv3 --kernel-trace --stats run of mode `on`.
    python tools/hap_contigs_probe.py [mode] [reps] [contigs] [contig length]"""
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
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
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
    """tools/window_phase_probe.py's: the batch of strings as the arrays of a dagcon_cigar_batch."""
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
per = -(-tlen // W)
c0 = np.tile(np.arange(per, dtype=np.int64) * W, n)
lo = (c0 - hw.begin).astype(np.uint32)
hi = (np.minimum(c0 + W, tlen) - hw.begin).astype(np.uint32)
prep = time.perf_counter() - t0
ctx = capi.Context(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_POS)
ctx.set_pileup(8, 350000)
ctx.set_site_reads(True)
ctx.set_window_phase()
ctx.set_hap_consensus()
out = {"probe": "hap_contigs", "mode": mode, "contigs": n, "contig_length": tlen, "windows": hw.n_windows, "window_and_overlap": [W, O], "reps": reps,
       "planted_bases": planted, "site_min_count_and_ppm": [8, 350000], "host_preparation_s": round(prep, 1)}
L = ctx.L
first_dev, dev, stage, wall, fetch_ms, join_ms = [], [], [], [], [], []
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    ctx.set_window_keep(None)
    ctx.upload_cigar_windows(cb, hw)
    ctx.run(); ctx.sync(); ctx.fetch()
    first = ctx.timings()["ms_total"]
    wp = ctx.window_phase()
    tally = ctx.hap_tally()
    if mode == "on":
        ctx.set_window_keep(lo, hi)
    t1 = time.perf_counter()
    ctx.upload_haps(swap=wp["flip"])
    t2 = time.perf_counter()
    ctx.run(); ctx.sync()
    r = capi.Results()
    ctx._chk(L.dagcon_fetch(ctx.h, C.byref(r)))
    t3 = time.perf_counter()
    S = int(r.n_segments)
    seq_off = np.ctypeslib.as_array(r.seq_off, shape=(S,)).copy()
    seq_len = np.ctypeslib.as_array(r.seq_len, shape=(S,)).copy()
    seg_begin = np.ctypeslib.as_array(r.seg_begin, shape=(r.n_targets + 1,)).copy()
    src = ctx.hap_map()["src_target"]
    seg_win = np.repeat(src, np.diff(seg_begin.astype(np.int64)))
    if mode == "on":
        wk = capi.WindowKeep()
        ta = time.perf_counter()
        ctx._chk(L.dagcon_fetch_window_keep(ctx.h, C.byref(wk)))
        tb = time.perf_counter()
        i0 = np.ctypeslib.as_array(wk.i0, shape=(S,)); i1 = np.ctypeslib.as_array(wk.i1, shape=(S,))
        tc = time.perf_counter()
        kept = int((i1.astype(np.int64) - i0).sum())             # the record join: O(segments)
        cont = int(((i0 > 0)[1:] & (i1 < seq_len)[:-1]).sum())
        td = time.perf_counter()
        nbytes = 16 * S
    else:
        ptr, cnt = C.POINTER(C.c_uint32)(), C.c_uint64()
        ta = time.perf_counter()
        ctx._chk(L.dagcon_fetch_positions(ctx.h, C.byref(ptr), C.byref(cnt)))
        tb = time.perf_counter()
        pos = np.ctypeslib.as_array(ptr, shape=(max(int(cnt.value), 1),))
        tc = time.perf_counter()
        kept = cont = 0
        prev_cut = False
        for s in range(S):                                      # the scan over every base of every segment
            p = pos[int(seq_off[s]):int(seq_off[s]) + int(seq_len[s])]
            a = p > lo[seg_win[s]]
            k0 = int(a.argmax()) if a.any() else p.size
            b = p[k0:] > hi[seg_win[s]]
            k1 = k0 + int(b.argmax()) if b.any() else p.size
            kept += k1 - k0
            cont += bool(s and k0 > 0 and prev_cut)
            prev_cut = k1 < p.size
        td = time.perf_counter()
        nbytes = 4 * int(cnt.value)
    tm = ctx.timings()
    if rep == 0:
        out.update({"reruns_of_the_warm_up": tm["reruns"], "split_windows": int(tally["split"].sum()), "flipped_windows": int(wp["flip"].sum()),
                    "derived_targets": int(r.n_targets), "derived_segments": S, "derived_consensus_bases": int(tm["consensus_bases"]),
                    "kept_bases": kept, "continuations": cont, "bytes_fetched_for_the_stitch": nbytes})
    else:
        first_dev.append(round(first, 3)); dev.append(round(tm["ms_total"], 3)); stage.append(round(tm["ms_bestpath"], 3))
        wall.append(round((t3 - t2) * 1e3, 3)); fetch_ms.append(round((tb - ta) * 1e3, 3)); join_ms.append(round((td - tc) * 1e3, 3))
        out.setdefault("upload_haps_wall_ms", []).append(round((t2 - t1) * 1e3, 3))
out.update({"first_batch_device_pipeline_ms": first_dev, "derived_device_pipeline_ms": dev, "derived_bestpath_stage_ms": stage,
            "derived_run_sync_fetch_wall_ms": wall,
            ("fetch_window_keep_call_ms" if mode == "on" else "fetch_positions_call_ms"): fetch_ms,
            ("record_join_ms" if mode == "on" else "per_base_scan_numpy_ms"): join_ms})
ctx.close()
print(json.dumps(out), flush=True)
