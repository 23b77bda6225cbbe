"""Cost of applying the read strand on the device next to reads that are reverse-complemented on the host beforehand,
copies inside the clock, pageable memory: configs[1] (1,000 targets x 10 kb x 40x, pbdagcon_amd/synth.py with its
backbone as the target sequence) with every second record reversed -- its bases lie in q_blob as a reads file would
have them -- through dagcon_consensus_cigar_strand, and the same batch with those records reverse-complemented on the
host (outside the clock) through dagcon_consensus_cigar, alternating in one process, `reps` repetitions each after a
warm-up, every value kept.  The yardstick is the unstranded call and its own spread.  Also what the host-side reverse
complement costs (numpy, one thread), for scale.  Prints one JSON line.  Kernel times: run it under
rocprofv3 --kernel-trace --stats.
    python tools/paf_probe.py [reps] [targets]
    python tools/paf_probe.py e2e [targets]     pbdagcon --sam on SAM text and pbdagcon --paf on PAF + reads FASTA of the
                                                same alignments (half of them '-'): wall time of each, twice"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cigar_twin as ct  # noqa: E402
import paf_files as pf  # noqa: E402
from pbdagcon_amd import capi, synth  # noqa: E402

TABLE = np.frombuffer(pf._TABLE, np.uint8)


def e2e(n):
    b = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    sam, paf, rd, fa = (os.path.join(d, "paf_probe." + x) for x in ("sam", "paf", "reads.fa", "fa"))
    names = ["t%07d" % t for t in range(n)]
    codes = np.frombuffer(ct.OPS.encode(), "S1")
    with open(sam, "wb") as g, open(paf, "wb") as h, open(rd, "wb") as f:
        g.write(ct.to_sam(names, [int(x) for x in b.tlen], [[] for _ in names]))
        for t in range(n):
            o = int(b.backbone_off[t])
            tl = int(b.tlen[t])
            bb = b.backbone[o:o + tl].tobytes()
            for k, (start, q, tt) in enumerate(b.target_alignments(t)):
                pos, qq, ops = ct.compress(start, q, tt, bb)
                ops = np.asarray(ops, np.int64)
                cig = b"".join(np.char.add(np.char.mod("%d", ops >> 4).astype("S"), codes[ops & 15]).tolist())
                qn = b"q%07d_%d" % (t, k)
                rev = k % 2 == 1
                span = pf.tspan(ops.tolist())
                g.write(b"%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (qn, 16 if rev else 0, names[t].encode(), pos, cig, qq))
                f.write(b">%s\n%s\n" % (qn, pf.revcomp(qq) if rev else qq))
                h.write(b"%s\t%d\t0\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:%s\n" % (
                    qn, len(qq), len(qq), b"-" if rev else b"+", names[t].encode(), tl, pos - 1, pos - 1 + span, span, span, cig))
    with open(fa, "wb") as f:
        f.write(ct.to_fasta(names, [b.backbone[int(b.backbone_off[t]):int(b.backbone_off[t]) + int(b.tlen[t])].tobytes() for t in range(n)]))
    exe = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
    runs = {"sam": [], "paf": []}
    outs = {}
    for rep in range(2):
        for kind, args in (("sam", ["--sam", "--ref", fa, sam]), ("paf", ["--paf", "--ref", fa, "--reads", rd, paf])):
            t0 = time.perf_counter()
            out = subprocess.run([exe, "-j", "8", *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            runs[kind].append(round(time.perf_counter() - t0, 3))
            assert out.returncode == 0, out.stderr.decode()[-500:]
            outs[kind] = out.stdout
    print(json.dumps({"probe": "e2e", "targets": n, "sam_bytes": os.path.getsize(sam), "paf_bytes": os.path.getsize(paf),
                      "reads_bytes": os.path.getsize(rd), "fasta_bytes": os.path.getsize(fa), "wall_s": runs,
                      "same_output": outs["sam"] == outs["paf"], "records": outs["sam"].count(b">")}), flush=True)
    for p in (sam, paf, rd, fa):
        os.remove(p)


if len(sys.argv) > 1 and sys.argv[1] == "e2e":
    e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
un = capi.HostCigarBatch(**ct.compress_batch(batch))                 # the bases in the target's orientation
del batch
reverse = (np.arange(un.n_records) % 2).astype(np.uint8)
# the reads as a reads file has them: the reverse records' bases reverse-complemented in place
t0 = time.perf_counter()
blob = un.q_blob.copy()
for r in np.flatnonzero(reverse):
    o, ln = int(un.q_off[r]), int(un.q_len[r])
    blob[o:o + ln] = TABLE[un.q_blob[o:o + ln][::-1]]
host_revcomp_ms = (time.perf_counter() - t0) * 1e3
st = capi.HostCigarBatch(un.tlen, un.t_off, un.t_blob, un.rec_begin, un.pos, un.q_off, un.q_len, blob, un.op_begin, un.ops,
                         reverse=reverse)
structs = {"unstranded": un.c_struct(), "stranded": st.c_struct()}
wall = {"unstranded": [], "stranded": []}
dev = {"unstranded": [], "stranded": []}
res = {}
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
for rep in range(reps + 1):                                          # (rep 0: warm-up, not recorded)
    for kind in ("unstranded", "stranded"):
        r = capi.Results()
        t0 = time.perf_counter()
        if kind == "unstranded":
            rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(structs[kind]), C.byref(r))
        else:
            rc = ctx.L.dagcon_consensus_cigar_strand(ctx.h, C.byref(structs[kind]), None, st.reverse.ctypes.data, C.byref(r))
        dt = (time.perf_counter() - t0) * 1e3
        ctx._chk(rc)
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
        else:
            wall[kind].append(round(dt, 3))
            dev[kind].append(round(ctx.timings()["ms_total"], 3))
ctx.close()
print(json.dumps({
    "probe": "paf_input", "targets": n, "reps": reps,
    "same_consensus": res["unstranded"] == res["stranded"],
    "consensus_bases": sum(len(x) for segs in res["stranded"] for _, _, x in segs),
    "records": un.n_records, "reverse_records": int(reverse.sum()), "read_bases": int(un.q_len.sum()),
    "host_revcomp_numpy_ms": round(host_revcomp_ms, 1),
    "wall_ms": wall, "device_pipeline_ms": dev,
    "unstranded_spread_ms": round(max(wall["unstranded"]) - min(wall["unstranded"]), 3),
    "stranded_minus_unstranded_ms": [round(p - u, 3) for p, u in zip(wall["stranded"], wall["unstranded"])],
}), flush=True)
