"""Step time of a DAGCON_FLAG_BASE_POS context against a BASE_SUPPORT-only one (configs[1] shape, inputs resident), and
the windowed CIGAR call against dagcon_consensus_cigar on the same windows given as separate short targets whose
records were cut on the host outside the clock (copies inside the clock for both).  Writes profiles/windows/probe.json.

    python tools/window_probe.py [targets] [read_len] [coverage] [contig_len]     (defaults 1000 10000 30 1000000)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cigar_twin as ct  # noqa: E402
import window_twin as wt  # noqa: E402
from pbdagcon_amd import capi, synth  # noqa: E402


def step_ms(ctx, n=10, warm=2):
    out = []
    for i in range(n + warm):
        t0 = time.perf_counter(); ctx.run(); ctx.sync(); dt = time.perf_counter() - t0
        if i >= warm:
            out.append(dt * 1e3)
    return sorted(out)[len(out) // 2]


def main():
    T, tlen, cov, clen = (int(x) for x in (sys.argv[1:5] + ["1000", "10000", "30", "1000000"][len(sys.argv) - 1:]))
    res = {}
    batch = synth.make_batch(T, tlen, cov, seed=1)
    for name, flags in (("plain", 0), ("sup", capi.FLAG_BASE_SUPPORT), ("pos", capi.FLAG_BASE_POS),
                        ("sup_pos", capi.FLAG_BASE_SUPPORT | capi.FLAG_BASE_POS)):
        ctx = capi.Context(flags=flags)
        ctx.upload(batch)
        res["step_ms_" + name] = step_ms(ctx)
        ctx.fetch()
        ctx.close()
    # one contig of clen bases, reads of tlen bases mapped at random offsets at `cov`x (tests/test_windows.py:
    # mapped_reads), W = 10,000, O = 1,000
    import test_windows as tw
    rng = np.random.default_rng(2)
    contig = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), clen))
    recs = tw.mapped_reads(rng, contig, clen * cov // tlen, tlen)
    targets = [(contig, recs)]
    win = [(0, b, e) for b, e, _, _ in wt.tiled(len(contig), 10000, 1000)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    wo = capi.HostWindows([w[0] for w in win], [w[1] for w in win], [w[2] for w in win])
    # the parent's way: every window a target of its own, records cut on the host (outside the clock)
    spans = [wt.span(p, clen, ops) for p, _, ops in recs]
    sep = []
    for _, b, e in win:
        near = [r for r, (s0, e0) in zip(recs, spans) if s0 < e and e0 > b]
        (_, alns, _), = wt.window_targets([(contig, near)], [(0, b, e)])
        tb = contig[b:e]
        sep.append((tb, [ct.compress(s, q, t, tb) for s, q, t in alns]))
    sb = capi.HostCigarBatch(**ct.records_to_arrays(sep))
    ctx = capi.Context()
    ms_w, ms_s = [], []
    for i in range(5):
        t0 = time.perf_counter(); a = ctx.consensus_cigar_windows(cb, wo); ms_w.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); b = ctx.consensus_cigar(sb); ms_s.append((time.perf_counter() - t0) * 1e3)
        assert a == b
    ctx.close()
    res.update(contig_len=len(contig), windows=len(win), records=len(recs), windowed_call_ms=sorted(ms_w)[2],
               separate_targets_call_ms=sorted(ms_s)[2], pieces=int(sb.n_records), windowed_bytes=cb.nbytes, separate_bytes=sb.nbytes)
    os.makedirs(os.path.join(ROOT, "profiles", "windows"), exist_ok=True)
    json.dump(res, open(os.path.join(ROOT, "profiles", "windows", "probe.json"), "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
