"""Cost of packed (BAM 4-bit) read bases next to one byte a base, copies inside the clock, pageable memory: configs[1]
(1,000 targets x 10 kb x 40x, pbdagcon_amd/synth.py with its backbone as the target sequence) and the same shape at
1 % error, each through dagcon_consensus_cigar on the unpacked batch and through dagcon_consensus_cigar_packed on its
packed twin (HostCigarBatch.packed(), outside the clock), alternating in one process, `reps` repetitions each after a
warm-up, every value kept.  Also the bytes both forms carry to the device, counted from the arrays.  Prints one JSON
line.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
    python tools/bam_probe.py [reps] [targets]
    python tools/bam_probe.py e2e [targets]     pbdagcon --sam on SAM text and pbdagcon --bam on the BAM of the same
                                                records (tests/bam_files.py, level 6): wall time of each, twice, the
                                                file sizes and the reader's inflate line (PBDAGCON_TIMING)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_files as bf  # noqa: E402
import cigar_twin as ct  # noqa: E402
from pbdagcon_amd import capi, synth  # noqa: E402


def e2e(n):
    import struct
    b = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    sam, bam, fa = (os.path.join(d, "bam_probe." + x) for x in ("sam", "bam", "fa"))
    names = ["t%07d" % t for t in range(n)]
    refs = [(names[t], int(b.tlen[t])) for t in range(n)]
    codes = np.frombuffer(ct.OPS.encode(), "S1")
    nib = np.full(256, 0, np.uint8)
    nib[np.frombuffer(bf.NT16, np.uint8)] = np.arange(16, dtype=np.uint8)
    pending, pend_bytes = [], 0
    with open(sam, "wb") as g, open(bam, "wb") as h:
        def put(chunk, flush=False):
            # members of 0xFF00 payload bytes, as a writer fills them: records straddle them
            nonlocal pending, pend_bytes
            pending.append(chunk); pend_bytes += len(chunk)
            if pend_bytes >= (1 << 22) or flush:
                data = b"".join(pending)
                cut = len(data) if flush else len(data) - len(data) % 0xFF00
                h.write(bf.bgzf(data[:cut], 6, eof=flush) if cut or flush else b"")
                pending, pend_bytes = [data[cut:]], len(data) - cut
        g.write(bf.sam_text(refs, []))
        put(bf.bam_bytes(refs, []))
        for t in range(n):
            o = int(b.backbone_off[t])
            bb = b.backbone[o:o + int(b.tlen[t])].tobytes()
            for k, (start, q, tt) in enumerate(b.target_alignments(t)):
                pos, qq, ops = ct.compress(start, q, tt, bb)
                ops = np.asarray(ops, np.int64)
                cig = b"".join(np.char.add(np.char.mod("%d", ops >> 4).astype("S"), codes[ops & 15]).tolist())
                qn = b"q%07d_%d" % (t, k)
                g.write(b"%s\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (qn, names[t].encode(), pos, cig, qq))
                # the record, vectorised (bam_files.record_bytes lays out the same fields a base at a time)
                c = nib[np.frombuffer(qq, np.uint8)]
                if c.size % 2:
                    c = np.append(c, np.uint8(0))
                seq = ((c[0::2] << 4) | c[1::2]).tobytes()
                span = bf.ref_span(ops.tolist())
                body = struct.pack("<iiBBHHHiiii", t, pos - 1, len(qn) + 1, 60, bf.reg2bin(pos - 1, pos - 1 + max(span, 1)),
                                   len(ops), 0, len(qq), -1, -1, 0)
                assert len(ops) <= 65535
                body += qn + b"\0" + ops.astype("<u4").tobytes() + seq + b"\xff" * len(qq)
                put(struct.pack("<i", len(body)) + body)
        put(b"", flush=True)
    with open(fa, "wb") as f:
        f.write(ct.to_fasta(names, [b.backbone[int(b.backbone_off[t]):int(b.backbone_off[t]) + int(b.tlen[t])].tobytes() for t in range(n)]))
    exe = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
    runs = {"sam": [], "bam": []}
    outs, inflate = {}, []
    env = dict(os.environ, PBDAGCON_TIMING="1")
    for rep in range(2):
        for kind, args in (("sam", ["--sam", "--ref", fa, sam]), ("bam", ["--bam", "--ref", fa, bam])):
            t0 = time.perf_counter()
            out = subprocess.run([exe, "-j", "8", *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            runs[kind].append(round(time.perf_counter() - t0, 3))
            assert out.returncode == 0, out.stderr.decode()[-500:]
            outs[kind] = out.stdout
            inflate += [ln for ln in out.stderr.decode().splitlines() if "--bam inflate" in ln]
    rate = [float(m.group(1)) for ln in inflate for m in [re.search(r"\(([\d.]+) MB/s", ln)] if m]
    print(json.dumps({"probe": "e2e", "targets": n, "sam_bytes": os.path.getsize(sam), "bam_bytes": os.path.getsize(bam),
                      "fasta_bytes": os.path.getsize(fa), "wall_s": runs, "same_output": outs["sam"] == outs["bam"],
                      "records": outs["sam"].count(b">"), "inflate_MBps_per_thread": rate, "inflate_lines": inflate}), flush=True)
    for p in (sam, bam, fa):
        os.remove(p)


if len(sys.argv) > 1 and sys.argv[1] == "e2e":
    e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
shapes = {"clr_like": synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True),
          "one_percent": synth.make_batch(n, 10000, 40, seed=1000, sub=0.004, ins=0.004, dele=0.002, with_backbone=True)}
out = {"probe": "bam_input", "targets": n, "reps": reps}
ctx = capi.Context(min_cov=6, min_len=500, trim=50)
for name, batch in shapes.items():
    cb = capi.HostCigarBatch(**ct.compress_batch(batch))
    pb = cb.packed()
    del batch
    structs = {"unpacked": cb.c_struct(), "packed": pb.c_struct()}
    wall = {"unpacked": [], "packed": []}
    dev = {"unpacked": [], "packed": []}
    res = {}
    for rep in range(reps + 1):                              # (rep 0: warm-up, not recorded)
        for kind in ("unpacked", "packed"):
            r = capi.Results()
            t0 = time.perf_counter()
            if kind == "unpacked":
                rc = ctx.L.dagcon_consensus_cigar(ctx.h, C.byref(structs[kind]), C.byref(r))
            else:
                rc = ctx.L.dagcon_consensus_cigar_packed(ctx.h, C.byref(structs[kind]), None, C.byref(r))
            dt = (time.perf_counter() - t0) * 1e3
            ctx._chk(rc)
            if rep == 0:
                res[kind] = capi.Context.results_to_py(r)
            else:
                wall[kind].append(round(dt, 3))
                dev[kind].append(round(ctx.timings()["ms_total"], 3))
    out[name] = {
        "same_consensus": res["unpacked"] == res["packed"],
        "consensus_bases": sum(len(x) for segs in res["packed"] for _, _, x in segs),
        "records": cb.n_records, "read_bases": int(cb.q_len.sum()),
        "upload_bytes": {"unpacked": cb.nbytes, "packed": pb.nbytes, "read_bases_unpacked": int(cb.q_blob.size),
                         "read_bases_packed": int(pb.q_blob.size)},
        "wall_ms": wall, "device_pipeline_ms": dev,
        "unpacked_spread_ms": round(max(wall["unpacked"]) - min(wall["unpacked"]), 3),
        "packed_minus_unpacked_ms": [round(p - u, 3) for p, u in zip(wall["packed"], wall["unpacked"])],
    }
    del cb, pb, structs, res
ctx.close()
print(json.dumps(out), flush=True)
