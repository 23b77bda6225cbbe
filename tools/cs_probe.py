"""Cost of taking alignments as cs:Z: text (dagcon_consensus_cs: decoded on the device, no reads uploaded) next to the
stranded CIGAR call on the same alignments (dagcon_consensus_cigar_strand: reads as a reads file has them, every second
record reversed), copies inside the clock, pageable memory, alternating in one process, `reps` repetitions each after a
warm-up, every value kept.  Targets of the configs[1] shape (10 kb x 40x, pbdagcon_amd/synth.py with its backbone as the
target sequence) at the bench's error profile and at 1 % error.  Reports the bytes either call carries.  Prints one
JSON line per profile.  Kernel times: run it under rocprofv3 --kernel-trace --stats.
    python tools/cs_probe.py [reps] [targets]
    python tools/cs_probe.py e2e [targets]      pbdagcon --paf --cs and pbdagcon --paf --reads on one PAF file whose lines
                                                carry both tags (half of them '-'): wall time of each, twice"""
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
PROFILES = {"bench": {}, "one_percent": dict(sub=0.002, ins=0.005, dele=0.003)}
OPC = np.frombuffer(b":*+-", np.uint8)


def cs_of_strings(qstr, tstr):
    """Short-form cs text of one alignment's gapped strings (tests/cs_twin.py: encode, in numpy): (text, read bases,
    target bases)."""
    qa, ta = np.frombuffer(bytes(qstr), np.uint8), np.frombuffer(bytes(tstr), np.uint8)
    gq, gt = qa == 45, ta == 45
    code = np.where(gt, 2, np.where(gq, 3, np.where(qa == ta, 0, 1)))
    n = code.size
    start = np.ones(n, bool)
    start[1:] = (code[1:] != code[:-1]) | (code[1:] == 1)
    idx = np.flatnonzero(start)
    run = np.diff(np.append(idx, n))
    rc = code[idx]
    nd = 1 + sum((run >= 10 ** k).astype(np.int64) for k in range(1, 9))
    rb = np.where(rc == 0, 1 + nd, np.where(rc == 1, 3, 1 + run))
    off = np.cumsum(rb) - rb
    out = np.empty(int(rb.sum()), np.uint8)
    out[off] = OPC[rc]
    m = rc == 0
    for d in range(1, int(nd.max()) + 1 if n else 1):
        sel = m & (nd >= d)
        out[off[sel] + d] = 48 + (run[sel] // 10 ** (nd[sel] - d)) % 10
    s = rc == 1
    out[off[s] + 1] = ta[idx[s]] | 0x20
    out[off[s] + 2] = qa[idx[s]] | 0x20
    run_of = np.cumsum(start) - 1
    for c, src in ((2, qa), (3, ta)):
        cols = np.flatnonzero(code == c)
        r = run_of[cols]
        out[off[r] + 1 + cols - idx[r]] = src[cols] | 0x20
    return out.tobytes(), int((~gq).sum()), int((~gt).sum())


def cs_batch(batch):
    """A synth batch (with its backbone) as a HostCsBatch."""
    pos, q_len, t_span, cs_off, cs_len, texts = [], [], [], [], [], []
    at = 0
    for t in range(batch.n_targets):
        for start, q, tt in batch.target_alignments(t):
            text, nq, nt = cs_of_strings(q, tt)
            pos.append(start); q_len.append(nq); t_span.append(nt); cs_off.append(at); cs_len.append(len(text))
            texts.append(text); at += len(text)
    return capi.HostCsBatch(batch.tlen, batch.backbone_off, batch.backbone, batch.aln_begin, pos, q_len, cs_off, cs_len,
                            b"".join(texts), t_span)


def e2e(n):
    b = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True)
    d = "/dev/shm" if os.access("/dev/shm", os.W_OK) else "/tmp"
    paf, rd, fa = (os.path.join(d, "cs_probe." + x) for x in ("paf", "reads.fa", "fa"))
    names = ["t%07d" % t for t in range(n)]
    codes = np.frombuffer(ct.OPS.encode(), "S1")
    cs_bytes = cg_bytes = 0
    with open(paf, "wb") as h, open(rd, "wb") as f:
        for t in range(n):
            o = int(b.backbone_off[t])
            tl = int(b.tlen[t])
            bb = b.backbone[o:o + tl].tobytes()
            for k, (start, q, tt) in enumerate(b.target_alignments(t)):
                pos, qq, ops = ct.compress(start, q, tt, bb)
                ops = np.asarray(ops, np.int64)
                cig = b"".join(np.char.add(np.char.mod("%d", ops >> 4).astype("S"), codes[ops & 15]).tolist())
                text, nq, span = cs_of_strings(q, tt)
                qn = b"q%07d_%d" % (t, k)
                rev = k % 2 == 1
                f.write(b">%s\n%s\n" % (qn, pf.revcomp(qq) if rev else qq))
                h.write(b"%s\t%d\t0\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\ttp:A:P\tcg:Z:%s\tcs:Z:%s\n" % (
                    qn, len(qq), len(qq), b"-" if rev else b"+", names[t].encode(), tl, pos - 1, pos - 1 + span, span, span, cig, text))
                cs_bytes += len(text); cg_bytes += len(cig)
    with open(fa, "wb") as f:
        f.write(ct.to_fasta(names, [b.backbone[int(b.backbone_off[t]):int(b.backbone_off[t]) + int(b.tlen[t])].tobytes() for t in range(n)]))
    exe = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
    runs = {"reads": [], "cs": []}
    outs = {}
    for rep in range(2):
        for kind, args in (("reads", ["--paf", "--ref", fa, "--reads", rd, paf]), ("cs", ["--paf", "--cs", "--ref", fa, paf])):
            t0 = time.perf_counter()
            out = subprocess.run([exe, "-j", "8", *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            runs[kind].append(round(time.perf_counter() - t0, 3))
            assert out.returncode == 0, out.stderr.decode()[-500:]
            outs[kind] = out.stdout
    print(json.dumps({"probe": "e2e", "targets": n, "paf_bytes": os.path.getsize(paf), "cs_text_bytes": cs_bytes, "cg_text_bytes": cg_bytes,
                      "reads_bytes": os.path.getsize(rd), "fasta_bytes": os.path.getsize(fa), "wall_s": runs,
                      "same_output": outs["reads"] == outs["cs"], "records": outs["cs"].count(b">")}), flush=True)
    for p in (paf, rd, fa):
        os.remove(p)


def probe(name, reps, n):
    batch = synth.make_batch(n, 10000, 40, seed=1000, with_backbone=True, **PROFILES[name])
    un = capi.HostCigarBatch(**ct.compress_batch(batch))
    cs = cs_batch(batch)
    del batch
    reverse = (np.arange(un.n_records) % 2).astype(np.uint8)
    blob = un.q_blob.copy()
    for r in np.flatnonzero(reverse):
        o, ln = int(un.q_off[r]), int(un.q_len[r])
        blob[o:o + ln] = TABLE[un.q_blob[o:o + ln][::-1]]
    st = capi.HostCigarBatch(un.tlen, un.t_off, un.t_blob, un.rec_begin, un.pos, un.q_off, un.q_len, blob, un.op_begin, un.ops,
                             reverse=reverse)
    structs = {"strand": st.c_struct(), "cs": cs.c_struct()}
    wall = {"strand": [], "cs": []}
    dev = {"strand": [], "cs": []}
    res = {}
    ctx = capi.Context(min_cov=6, min_len=500, trim=50)
    for rep in range(reps + 1):                                      # (rep 0: warm-up, not recorded)
        for kind in ("strand", "cs"):
            r = capi.Results()
            t0 = time.perf_counter()
            if kind == "strand":
                rc = ctx.L.dagcon_consensus_cigar_strand(ctx.h, C.byref(structs[kind]), None, st.reverse.ctypes.data, C.byref(r))
            else:
                rc = ctx.L.dagcon_consensus_cs(ctx.h, C.byref(structs[kind]), None, C.byref(r))
            dt = (time.perf_counter() - t0) * 1e3
            ctx._chk(rc)
            if rep == 0:
                res[kind] = capi.Context.results_to_py(r)
            else:
                wall[kind].append(round(dt, 3))
                dev[kind].append(round(ctx.timings()["ms_total"], 3))
    ctx.close()
    print(json.dumps({
        "probe": "cs_input", "profile": name, "targets": n, "reps": reps,
        "same_consensus": res["strand"] == res["cs"],
        "consensus_bases": sum(len(x) for segs in res["cs"] for _, _, x in segs),
        "records": un.n_records, "read_bases": int(un.q_len.sum()), "cs_text_bytes": int(cs.cs_blob.size),
        "cigar_ops": int(un.ops.size),
        "input_bytes": {"strand": st.nbytes + int(reverse.nbytes), "cs": cs.nbytes},
        "wall_ms": wall, "device_pipeline_ms": dev,
        "strand_spread_ms": round(max(wall["strand"]) - min(wall["strand"]), 3),
        "cs_minus_strand_ms": [round(p - u, 3) for p, u in zip(wall["cs"], wall["strand"])],
    }), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "e2e":
        e2e(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    for name in (sys.argv[3:] or list(PROFILES)):
        probe(name, reps, n)
