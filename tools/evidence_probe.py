"""Cost of the read support per edit: the tools/edits_probe.py batch (configs[1]: 1,000 targets x 10 kb x 40x as
(position, read, CIGAR) records, one target base in a hundred changed), two calls alternating in one process, `reps`
repetitions each after a warm-up, every value kept:
    edits            dagcon_set_edits on: dagcon_consensus_cigar, then dagcon_fetch_edits
    support          dagcon_set_edit_support on as well: the same, then dagcon_fetch_edit_support
Wall time of each, the device pipeline's time (ms_total) and its bestPath stage (ms_bestpath: the edit and the support
kernels run at its end, so support minus edits is what k_ev_windows, k_ev_count and k_ev_spread add), the bytes the
support adds to the fetch, the counts' sums, and whether the two agree on the consensus and the edits.  Prints one JSON
line (kept as profiles/edit_support/probe.json).  The probe times stages, not kernels: the kernels' own times come
from a run of this script under rocprofv3 --kernel-trace --stats.
    python tools/evidence_probe.py [reps] [targets] [changed target bases per mille]"""
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
ctxs = {k: capi.Context(min_cov=6, min_len=500, trim=50, flags=capi.FLAG_BASE_POS) for k in ("edits", "support")}
for c in ctxs.values():
    c.set_edits(True)
ctxs["support"].set_edit_support(True)
wall = {k: [] for k in ctxs}
dev = {k: [] for k in ctxs}
stage = {k: [] for k in ctxs}
res, eds, sums = {}, {}, {}
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for kind, ctx in ctxs.items():
        r = capi.Results()
        t0 = time.perf_counter()
        ctx._chk(ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(c_struct), C.byref(r)))
        e = capi.Edits()
        ctx._chk(ctx.L.dagcon_fetch_edits(ctx.h, C.byref(e)))
        if kind == "support":
            s = capi.EditSupport()
            ctx._chk(ctx.L.dagcon_fetch_edit_support(ctx.h, C.byref(s)))
        dt = (time.perf_counter() - t0) * 1e3
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
            ed = ctx.edits()
            seq_off = np.ctypeslib.as_array(r.seq_off, shape=(int(r.n_segments),)).astype(np.int64)
            so = np.repeat(seq_off, np.diff(ed["edit_begin"].astype(np.int64)))
            eds[kind] = (ed["t_pos"].tolist(), ed["t_len"].tolist(), (ed["c_off"].astype(np.int64) - so).tolist(), ed["c_len"].tolist())
            if kind == "support":
                sp = ctx.edit_support()
                sums = {k: int(sp[k].sum()) for k in ("span", "alt", "ref")}
                sums["edits"] = int(sp["span"].size)
                sums["edits_with_alt_ge_ref"] = int((sp["alt"] >= sp["ref"]).sum())
                sums["windows_longer_than_the_edit"] = int(((sp["w_end"] - sp["w_begin"]) > ed["t_len"]).sum())
        else:
            wall[kind].append(round(dt, 3))
            dev[kind].append(round(ctx.timings()["ms_total"], 3))
            stage[kind].append(round(ctx.timings()["ms_bestpath"], 3))
for c in ctxs.values():
    c.close()
print(json.dumps({
    "probe": "edit_support", "targets": n, "changed_target_bases_per_mille": per_mille, "reps": reps,
    "same_consensus": res["edits"] == res["support"], "same_edits": eds["edits"] == eds["support"], "counts": sums,
    "wall_ms": wall, "device_pipeline_ms": dev, "bestpath_stage_ms": stage,
    "support_kernels_ms": [round(a - b, 3) for a, b in zip(stage["support"], stage["edits"])],
    "support_wall_ms": [round(a - b, 3) for a, b in zip(wall["support"], wall["edits"])],
    "fetched_bytes_for_the_support": 40 * sums.get("edits", 0),
}), flush=True)
