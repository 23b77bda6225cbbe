"""Cost of the local-end mode of the -a stage: the same pairs through dagcon_align on a global and on a local
(DAGCON_FLAG_LOCAL_ALIGN) context, alternating, in one process.  Pairs: nt targets of L bases x cov (synthetic edits,
as tools/align_probe.py).  Prints one JSON line.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
    python tools/align_local_probe.py [L] [cov] [nt] [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbdagcon_amd import capi, synth  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
cov = int(sys.argv[2]) if len(sys.argv) > 2 else 60
nt = int(sys.argv[3]) if len(sys.argv) > 3 else 64
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 2
b = synth.make_batch(nt, L, cov, seed=7000)
pairs = []
for t in range(b.n_targets):
    for start, q, tt in b.target_alignments(t):
        pairs.append((q.replace(b"-", b""), tt.replace(b"-", b"")))
ctxs = {"global": capi.Context(min_cov=8, min_len=500, trim=50),
        "local": capi.Context(min_cov=8, min_len=500, trim=50, flags=capi.FLAG_LOCAL_ALIGN)}
for c in ctxs.values():
    c.align(pairs[:4])
ms = {k: [] for k in ctxs}
res = {}
for rep in range(reps):
    for k, c in ctxs.items():
        t0 = time.perf_counter()
        out = c.align(pairs)
        ms[k].append((time.perf_counter() - t0) * 1e3)
        res[k] = (out, c.align_ends(), c.align_dropped())
g_out, _, g_drop = res["global"]
l_out, l_ends, l_drop = res["local"]
full = sum(e == (0, len(q), 0, len(t)) for e, (q, t) in zip(l_ends, pairs))
print(json.dumps({
    "pairs": len(pairs), "L": L, "cov": cov, "targets": nt,
    "ms_global": [round(x, 1) for x in ms["global"]], "ms_local": [round(x, 1) for x in ms["local"]],
    "local_over_global": round(min(ms["local"]) / min(ms["global"]), 3),
    "dropped_global": g_drop, "dropped_local": l_drop,
    "local_ends_whole": full, "local_equals_global": sum(a == b for a, b in zip(l_out, g_out)),
}), flush=True)
for c in ctxs.values():
    c.close()
