"""Cost of the edit list next to the per-base positions: the tools/cigar_probe.py batch (configs[1]: 1,000 targets x
10 kb x 40x, synth's backbone as the target sequence) as (position, read, CIGAR) records on DAGCON_FLAG_BASE_POS
contexts, with one target base in a hundred changed to another so that the consensus differs from its target as a
draft does from its polish (third argument: per mille, 0 for none), three calls alternating in one process, `reps` repetitions each after a warm-up, every value kept:
    consensus        dagcon_consensus_cigar, edits off (what the parent commit runs)
    positions        the same call, then dagcon_fetch_positions (4 B a consensus base, copied by the fetch)
    edits            dagcon_set_edits on: the call, then dagcon_fetch_edits (the positions stay on the device)
Wall time of each, the device pipeline's time (ms_total) and its bestPath stage (ms_bestpath: the three edit kernels
run at its end, so edits minus consensus is what they add), the bytes each result fetch brings beyond the consensus
itself, and whether the three agree on the consensus.  Prints one JSON line.  The probe times stages, not kernels: the
times of k_ed_scan_seg and k_ed_scan themselves come from a run of this script under rocprofv3 --kernel-trace --stats
(profiles/edits/kernel_stats.csv).
    python tools/edits_probe.py [reps] [targets] [changed target bases per mille]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
cb = capi.HostCigarBatch(**ct.compress_batch(batch))
per_mille = int(sys.argv[3]) if len(sys.argv) > 3 else 10
if per_mille:
    tb = cb.t_blob.copy()
    at = np.random.default_rng(7).choice(tb.size, size=tb.size * per_mille // 1000, replace=False)
    tb[at] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), tb[at] & 0xDF) % 4]
    cb.t_blob = np.ascontiguousarray(tb)
c_struct = cb.c_struct()
off = capi.Context(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_POS)
on = capi.Context(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_POS)
on.set_edits(True)
kinds = ("consensus", "positions", "edits")
wall = {k: [] for k in kinds}
dev = {k: [] for k in kinds}
stage = {k: [] for k in kinds}
extra = {}
res = {}
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for kind in kinds:
        ctx = on if kind == "edits" else off
        r = capi.Results()
        t0 = time.perf_counter()
        rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(c_struct), C.byref(r))
        ctx._chk(rc)
        if kind == "positions":
            ptr, cnt = C.POINTER(C.c_uint32)(), C.c_uint64()
            ctx._chk(ctx.L.dagcon_fetch_positions(ctx.h, C.byref(ptr), C.byref(cnt)))
            extra[kind] = 4 * int(cnt.value)
        elif kind == "edits":
            e = capi.Edits()
            ctx._chk(ctx.L.dagcon_fetch_edits(ctx.h, C.byref(e)))
            # (what crosses the link: a 32-byte record per segment, a 24-byte record per edit)
            extra[kind] = 32 * int(e.n_segments) + 24 * int(e.n)
            n_edits = int(e.n)
        else:
            extra[kind] = 4 * int(r.seq_bytes)               # (a BASE_POS context without edits copies them in the fetch)
        dt = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
        else:
            wall[kind].append(round(dt, 3))
            dev[kind].append(round(ctx.timings()["ms_total"], 3))
            stage[kind].append(round(ctx.timings()["ms_bestpath"], 3))
bases = sum(len(x) for segs in res["consensus"] for _, _, x in segs)
off.close(); on.close()
print(json.dumps({
    "probe": "edits", "targets": n, "changed_target_bases_per_mille": per_mille, "reps": reps, "consensus_bases": bases, "edits": n_edits,
    "same_consensus": res["consensus"] == res["positions"] == res["edits"],
    "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage,
    "edit_kernels_ms": [round(a - b, 3) for a, b in zip(stage["edits"], stage["consensus"])],
    "fetched_bytes_beyond_the_consensus": extra,
    "consensus_spread_ms": round(max(wall["consensus"]) - min(wall["consensus"]), 3),
    "edits_minus_positions_ms": [round(a - b, 3) for a, b in zip(wall["edits"], wall["positions"])],
}), flush=True)
