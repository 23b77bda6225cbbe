"""Cost of taking SAM / BAM records without a reference (dagcon_consensus_cigar_md: the targets rebuilt on the device
from the MD:Z texts, no target bases uploaded) next to the CIGAR call on the same records with the true targets uploaded
(dagcon_consensus_cigar), copies inside the clock, pageable memory, alternating in one process, `reps` repetitions each
after a warm-up, every value kept.  Targets of the configs[1] shape (10 kb x 40x, pbdagcon_amd/synth.py with its backbone
as the target sequence) at the bench's error profile and at 1 % error.  Reports the bytes either call carries and whether
the rebuilt targets equal the backbone wherever a record covers it.  Prints one JSON line per profile.  Kernel times:
run it under rocprofv3 --kernel-trace --stats.
    python tools/md_probe.py [reps] [targets] [profile ...]"""
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

PROFILES = {"bench": {}, "one_percent": dict(sub=0.002, ins=0.005, dele=0.003)}


def md_of_strings(qstr, tstr):
    """MD text of one alignment's gapped strings (tests/md_twin.py: encode, in numpy; deleted bases that only an
    insertion separates come out as one ^ group): (text, target bases covered)."""
    qa, ta = np.frombuffer(bytes(qstr), np.uint8), np.frombuffer(bytes(tstr), np.uint8)
    tc = ta != 45
    qa, ta = qa[tc], ta[tc]
    n = ta.size
    if n == 0:
        return b"0", 0
    code = np.where(qa == 45, 2, np.where(qa == ta, 0, 1))
    start = np.ones(n, bool)
    start[1:] = (code[1:] != code[:-1]) | (code[1:] == 1)
    idx = np.flatnonzero(start)
    run = np.diff(np.append(idx, n))
    rc = code[idx]
    z = rc != 0
    z[1:] &= rc[:-1] != 0                                            # a 0 between two letter groups, and in front of a first one
    nd = 1 + sum((run >= 10 ** k).astype(np.int64) for k in range(1, 9))
    rb = np.where(rc == 0, nd, np.where(rc == 1, 1, 1 + run)) + z
    off = np.cumsum(rb) - rb
    tail = int(rc[-1] != 0)
    out = np.empty(int(rb.sum()) + tail, np.uint8)
    if tail:
        out[-1] = 48
    out[off[z]] = 48
    bs = off + z
    m = rc == 0
    for d in range(1, int(nd[m].max()) + 1 if m.any() else 1):
        sel = m & (nd >= d)
        out[bs[sel] + d - 1] = 48 + (run[sel] // 10 ** (nd[sel] - d)) % 10
    s = rc == 1
    out[bs[s]] = ta[idx[s]]
    dl = rc == 2
    out[bs[dl]] = 94
    run_of = np.cumsum(start) - 1
    cols = np.flatnonzero(code == 2)
    r = run_of[cols]
    out[bs[r] + 1 + cols - idx[r]] = ta[cols]
    return out.tobytes(), n


def md_tags(batch):
    """The MD texts of a synth batch (with its backbone), one per alignment, and the positions its records cover."""
    texts = []
    covered = np.zeros(batch.backbone.size, bool)
    for t in range(batch.n_targets):
        o = int(batch.backbone_off[t])
        for start, q, tt in batch.target_alignments(t):
            text, nt = md_of_strings(q, tt)
            texts.append(text)
            covered[o + start - 1:o + start - 1 + nt] = True
    return capi.HostMdTags.from_texts(texts), covered


def probe(name, reps, n):
    batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True, **PROFILES[name])
    arr = ct.compress_batch(batch)
    ref_b = capi.HostCigarBatch(**arr)
    md, covered = md_tags(batch)
    del batch
    md_b = capi.HostCigarBatch(**dict(arr, t_blob=None))
    structs = {"ref": ref_b.c_struct(), "md": md_b.c_struct()}
    tags = md.c_struct()
    wall = {"ref": [], "md": []}
    dev = {"ref": [], "md": []}
    res = {}
    ctx = capi.Context(min_cov=6, min_len=500, trim=50)
    same_targets = None
    for rep in range(reps + 1):                                      # (rep 0: warm-up, not recorded)
        for kind in ("ref", "md"):
            r = capi.Results()
            t0 = time.perf_counter()
            if kind == "ref":
                rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(structs[kind]), C.byref(r))
            else:
                rc = ctx.L.dagcon_consensus_cigar_md(ctx.h, C.byref(structs[kind]), None, C.byref(tags), 0, C.byref(r))
            dt = (time.perf_counter() - t0) * 1e3
            ctx._chk(rc)
            if rep == 0:
                res[kind] = capi.Context.results_to_py(r)
                if kind == "md":
                    t = ctx.md_targets()
                    same_targets = bool(np.array_equal(t[covered], ref_b.t_blob[covered]) and (t[~covered] == ord("N")).all())
            else:
                wall[kind].append(round(dt, 3))
                dev[kind].append(round(ctx.timings()["ms_total"], 3))
    ctx.close()
    print(json.dumps({
        "probe": "md_input", "profile": name, "targets": n, "reps": reps,
        "same_consensus": res["ref"] == res["md"], "rebuilt_targets_equal_the_backbone_where_covered": same_targets,
        "consensus_bases": sum(len(x) for segs in res["md"] for _, _, x in segs),
        "records": ref_b.n_records, "read_bases": int(ref_b.q_len.sum()), "target_bases": int(ref_b.t_blob.size),
        "uncovered_target_bases": int((~covered).sum()), "md_text_bytes": int(md.md_blob.size), "cigar_ops": int(ref_b.ops.size),
        "input_bytes": {"ref": ref_b.nbytes, "md": md_b.nbytes + md.nbytes},
        "wall_ms": wall, "device_pipeline_ms": dev,
        "ref_spread_ms": round(max(wall["ref"]) - min(wall["ref"]), 3),
        "md_minus_ref_ms": [round(p - u, 3) for p, u in zip(wall["md"], wall["ref"])],
    }), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    for name in (sys.argv[3:] or list(PROFILES)):
        probe(name, reps, n)
