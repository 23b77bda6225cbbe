"""Cost of the CIGAR input next to the string input, copies inside the clock: configs[1] (1,000 targets x 10 kb x 40x,
pbdagcon_amd/synth.py with its backbone as the target sequence) through dagcon_consensus on the gapped strings and
through dagcon_consensus_cigar on (position, read, CIGAR) records, alternating in one process, `reps` repetitions each
after a warm-up, every value kept.  The CIGAR form comes from tests/cigar_twin.py (library-independent), outside the
clock.  Also the input bytes of both forms at this error profile and at 1 % error.  Prints one JSON line.  Kernel
times: run it under rocprofv3 --kernel-trace --stats.
    python tools/cigar_probe.py [reps] [targets]
    python tools/cigar_probe.py e2e [targets]     pbdagcon on .m5 text and pbdagcon --sam --ref on SAM text of the same
                                                  alignments: wall time of each, twice, and the file sizes"""
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
from pbdagcon_amd import capi, synth  # noqa: E402


def strings_only(b):
    return capi.HostBatch(b.tlen, b.aln_begin, b.aln_start, b.aln_off, b.aln_len, b.qstr, b.tstr, None, None, b.ids)


def string_bytes(b):
    return int(2 * b.qstr.size + sum(a.nbytes for a in (b.tlen, b.aln_begin, b.aln_start, b.aln_off, b.aln_len)))


def e2e(n):
    b = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    m5, sam, fa = (os.path.join(d, "cigar_probe." + x) for x in ("m5", "sam", "fa"))
    names = ["t%07d" % t for t in range(n)]
    codes = np.frombuffer(ct.OPS.encode(), "S1")
    with open(m5, "wb") as f, open(sam, "wb") as g:
        g.write(b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (names[t].encode(), int(b.tlen[t])) for t in range(n)))
        for t in range(n):
            o = int(b.backbone_off[t])
            bb = b.backbone[o:o + int(b.tlen[t])].tobytes()
            for k, (start, q, tt) in enumerate(b.target_alignments(t)):
                qa, ta = np.frombuffer(q, np.uint8), np.frombuffer(tt, np.uint8)
                nq, nt = int(np.count_nonzero(qa != 45)), int(np.count_nonzero(ta != 45))
                match = np.where(qa == ta, np.uint8(124), np.uint8(42)).tobytes()
                f.write(b"q%07d_%d/0_%d %d 0 %d + %s %d %d %d + -1000 0 0 0 0 254 " % (
                    t, k, nq, nq, nq, names[t].encode(), int(b.tlen[t]), start - 1, start - 1 + nt))
                f.write(q); f.write(b" "); f.write(match); f.write(b" "); f.write(tt); f.write(b"\n")
                pos, qq, ops = ct.compress(start, q, tt, bb)
                ops = np.asarray(ops, np.int64)
                cig = b"".join(np.char.add(np.char.mod("%d", ops >> 4).astype("S"), codes[ops & 15]).tolist())
                g.write(b"q%07d_%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (t, k, names[t].encode(), pos, cig, qq))
    with open(fa, "wb") as f:
        f.write(ct.to_fasta(names, [b.backbone[int(b.backbone_off[t]):int(b.backbone_off[t]) + int(b.tlen[t])].tobytes() for t in range(n)]))
    exe = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
    runs = {"m5": [], "sam": []}
    outs = {}
    for rep in range(2):
        for kind, args in (("m5", [m5]), ("sam", ["--sam", "--ref", fa, sam])):
            t0 = time.perf_counter()
            out = subprocess.run([exe, "-j", "8", *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            runs[kind].append(round(time.perf_counter() - t0, 3))
            assert out.returncode == 0, out.stderr.decode()[-500:]
            outs[kind] = out.stdout
    print(json.dumps({"probe": "e2e", "targets": n, "m5_bytes": os.path.getsize(m5), "sam_bytes": os.path.getsize(sam),
                      "fasta_bytes": os.path.getsize(fa), "wall_s": runs, "same_output": outs["m5"] == outs["sam"],
                      "records": outs["m5"].count(b">")}), flush=True)
    for p in (m5, sam, fa):
        os.remove(p)


if len(sys.argv) > 1 and sys.argv[1] == "e2e":
    e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
sb = strings_only(batch)
cb = capi.HostCigarBatch(**ct.compress_batch(batch))
low = synth.make_batch(max(n // 10, 1), 10000, 40, seed=1000, sub=0.004, ins=0.004, dele=0.002, with_backbone=True)
low_c = capi.HostCigarBatch(**ct.compress_batch(low))
sizes = {"clr_like": {"targets": n, "string_bytes": string_bytes(sb), "cigar_bytes": cb.nbytes, "ops": int(cb.ops.size)},
         "one_percent": {"targets": low.n_targets, "string_bytes": string_bytes(low), "cigar_bytes": low_c.nbytes, "ops": int(low_c.ops.size)}}
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
s_struct, c_struct = sb.c_struct(), cb.c_struct()
wall = {"strings": [], "cigar": []}
dev = {"strings": [], "cigar": []}
res = {}
for rep in range(reps + 1):                                  # (rep 0: warm-up, not recorded)
    for kind in ("strings", "cigar"):
        r = capi.Results()
        t0 = time.perf_counter()
        if kind == "strings":
            rc = ctx.L.dagcon_consensus(ctx.h, C.byref(s_struct), C.byref(r))
        else:
            rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(c_struct), C.byref(r))
        dt = (time.perf_counter() - t0) * 1e3
        ctx._chk(rc)
        if rep == 0:
            res[kind] = capi.Context.results_to_py(r)
        else:
            wall[kind].append(round(dt, 3))
            dev[kind].append(round(ctx.timings()["ms_total"], 3))
ctx.close()
spread = max(wall["strings"]) - min(wall["strings"])
print(json.dumps({
    "probe": "cigar_input", "targets": n, "reps": reps, "same_consensus": res["strings"] == res["cigar"],
    "consensus_bases": sum(len(x) for segs in res["cigar"] for _, _, x in segs),
    "wall_ms": wall, "device_pipeline_ms": dev,
    "strings_spread_ms": round(spread, 3),
    "cigar_minus_strings_ms": [round(c - s, 3) for c, s in zip(wall["cigar"], wall["strings"])],
    "input_bytes": sizes,
}), flush=True)
