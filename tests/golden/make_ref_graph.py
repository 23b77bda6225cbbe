#!/usr/bin/env python3
"""The inputs on which the oracle's graph stages (addAln, mergeNodes, bestPath, consensus) are held to the REFERENCE's own
AlnGraphBoost.cpp (compiled in place on oracle/bgl_standin into oracle/_ref/libref_graph.so), the one way an answer is
written down, and the fixtures made from the reference's answers:

  tests/golden/ref_graph_hashes.json   SHA-256 per block of BLOCK answers, per group of inputs (test_ref_graph.py)
  tests/golden/ref_graph_gpu.json      the reference's consensus segments of the groups test_ref_graph_gpu.py runs

An input is (tlen, alns, backbone, option sets); it is answered once per option set (min_len, trim, min_weight) with the
N backbone (AlnGraphBoost(tlen), main.cpp:130) and once with the real one (AlnGraphBoost(backbone)).  One answer is

  (segments, longest, path, dangling, adjacency)
    segments   consensus(seqs, min_weight, min_len) behind main.cpp:130-137: [(range0, range1, seq)]
    longest    consensus(min_weight)
    path       bestPath(): (base, weight, coverage, backbone, deleted) per node
    dangling   danglingNodes()
    adjacency  the merged graph per vertex id: (base, weight, coverage, deleted, out list, in list), the lists as
               (vertex, count) in list order (oracle.Graph.adjacency())

or the string "nonconforming" where the oracle refuses the input (the reference's behaviour is undefined there, and it is
not run).  A block's digest is sha256(repr(list of answers)), strings as Python bytes / str reprs.  The bound inputs
(tests/bound_cases.py) are answered by their segments alone.

    python tests/golden/make_ref_graph.py        # rewrites both files; needs the reference (oracle/_ref)
"""
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from util import random_target  # noqa: E402

BLOCK = 100
N_RANDOM = 1500
PLAIN = (0, 0, 0)                          # merge_cases.GRAPH_OPTS as (min_len, trim, min_weight)
TRIMMED = (0, 2, 1)                        # the second of merge_cases.CNS_OPTS
DEFAULT = (500, 50, 6)                     # pbdagcon's defaults, where a read is long enough to pass them
GPU_RANDOM = 60                            # test_ref_graph_gpu.py: the first 60 random inputs with at least 3 reads
GPU_FAMILIES = (("merge", ("widths", "fan32", "span", "partial")), ("bestpath", ("suffix", "waiters", "widths_row")))
BOUND = (("S", "above"), ("P", "above"), ("M", "above"), ("S", "between"))


# ---- the inputs ------------------------------------------------------------------------------------------------------------

def _optsets(alns, sets):
    sets = list(sets)
    if any(len(a[1]) >= DEFAULT[0] for a in alns):
        sets.append(DEFAULT)
    return tuple(dict.fromkeys(sets))


def random_inputs():
    """1,500 seeded pileups: tlen 1 .. 120 (every 50th 300 .. 1,500), 0 .. 14 reads, alphabets ACGT / AC / ACGTN / A in
    rotation, every third full span, every seventh with dots; answered under its own small (min_len 0 .. 7, trim 0 .. 3,
    min_weight 0 .. 3) and under the plain options."""
    rng = np.random.default_rng(20)
    out = []
    for i in range(N_RANDOM):
        tl = int(rng.integers(300, 1501)) if i % 50 == 49 else int(rng.integers(1, 121))
        alph = [b"ACGT", b"AC", b"ACGTN", b"A"][i % 4]
        alns, bb = random_target(rng, tl, int(rng.integers(0, 15)), alphabet=alph, sub=float(rng.uniform(0, 0.1)),
                                 ins=float(rng.uniform(0, 0.3)), dele=float(rng.uniform(0, 0.2)), dots=(i % 7 == 0),
                                 full_span=(i % 3 == 0))
        own = (int(rng.integers(0, 8)), int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        out.append((tl, alns, bb, _optsets(alns, (own, PLAIN))))
    return out


def _as_opts(d):
    return d["min_len"], d["trim"], d["min_weight"]


def family_names():
    """Every group of constructed inputs, as (module, family)."""
    import bestpath_cases as bc
    import build_cases as bu
    import cut_cases as cc
    import merge_cases as mc
    return ([("merge", n) for n in mc.ALL] + [("bestpath", n) for n in bc.ALL] + [("build", n) for n in bu.FAMILIES]
            + [("cut", n) for n in cc.FAMILIES] + [("cut", "mixed")])


def family_inputs(module, name):
    """The inputs of one family: every target of it (carve: the targets of CARVE_GRAPHS), under the option sets its case
    file runs it with."""
    import bestpath_cases as bc
    import build_cases as bu
    import cut_cases as cc
    import merge_cases as mc
    cns = tuple(_as_opts(o) for o in mc.CNS_OPTS)
    assert cns == (PLAIN, TRIMMED)
    if module == "merge":
        targets, sets = mc.case(name).targets, cns
    elif module == "bestpath":
        targets, sets = bc.case(name).targets, cns
    elif module == "build":
        fam = bu.family(name)
        if name == "carve":
            targets = [fam[t] for t in bu.CARVE_GRAPHS if t not in bu.CARVE_INACTIVE and t != bu.CARVE_BAD]
            sets = (_as_opts(bu.CARVE_OPTS), _as_opts(dict(bu.CARVE_OPTS, trim=1)))
        else:
            targets, sets = fam, cns + (_as_opts(dict(mc.GRAPH_OPTS, trim=1)),)
    elif name == "mixed":
        targets, sets = [c.target for c in cc.mixed()[0]], cns
    else:
        targets, sets = [c.target for c in cc.family(name)], cns
    return [(tl, alns, bb, _optsets(alns, sets)) for tl, alns, bb in targets]


def group_names():
    return ["random"] + [f"{m}/{n}" for m, n in family_names()]


def group_inputs(name):
    return random_inputs() if name == "random" else family_inputs(*name.split("/"))


def runs(inputs):
    """(input index, tlen, alns, backbone or None, (min_len, trim, min_weight)) of every answer, in the order of the digests."""
    for i, (tl, alns, bb, sets) in enumerate(inputs):
        for real in (False, True):
            for o in sets:
                yield i, tl, alns, (bb if real else None), o


# ---- the answers -----------------------------------------------------------------------------------------------------------

def oracle_answer(tl, alns, bb, o):
    ml, trim, mw = o
    try:
        segs = oracle.consensus_target(tl, alns, ml, trim, mw, bb)
    except ValueError:
        return "nonconforming"
    g = oracle.Graph(backbone=bb) if bb is not None else oracle.Graph(blen=tl)
    for s, q, t in alns:
        if len(q) < ml:
            continue
        qn, tn = oracle.normalize_gaps(q, t)
        qn, tn, s2 = oracle.trim_aln(qn, tn, s, trim)
        g.add_aln(s2, qn, tn)
    assert g.merge_nodes() == 0
    assert g.consensus_all(mw, ml) == segs
    return segs, g.consensus_longest(mw), oracle.path_nodes(g), g.dangling_nodes(), g.adjacency()


def ref_answer(tl, alns, bb, o, lib=None):
    """The same from the reference (or from a build of it on another stand-in: lib).  Conforming input only."""
    ml, trim, mw = o
    segs = oracle.ref_consensus_target(tl, alns, ml, trim, mw, bb, lib=lib)
    g = oracle.ref_target_graph(tl, alns, ml, trim, bb, lib=lib)
    assert g.consensus_all(mw, ml) == segs
    return segs, g.consensus_longest(mw), g.best_path(), g.dangling_nodes(), g.adjacency()


def kat_answers(graph_cls, path_of):
    """The reference's two known-answer tests (test/cpp/AlnGraphBoostTest.cpp:11-57, inputs in kat_graph.json) on
    oracle.Graph or oracle.RefGraph: (RawConsensus: consensus(), path, adjacency), (DanglingNodes: danglingNodes())."""
    k = json.load(open(os.path.join(HERE, "kat_graph.json")))
    r, d = k["raw_consensus"], k["dangling_nodes"]
    g = graph_cls(backbone=r["backbone"].encode())
    for a in r["alignments"]:
        g.add_aln(r["start"], a["q"].encode(), a["t"].encode())
    assert g.merge_nodes() == 0
    h = graph_cls(blen=d["blen"])
    h.add_aln(d["start"], d["q"].encode(), d["t"].encode())
    return (g.consensus_longest(0), path_of(g), g.adjacency()), h.dangling_nodes()


def digests(answers):
    return [hashlib.sha256(repr(answers[i:i + BLOCK]).encode()).hexdigest() for i in range(0, len(answers), BLOCK)]


def bound_segments(family, band, ref=False):
    """The segments of one input of tests/bound_cases.py under its options: the oracle's fp32 answer, or the reference's."""
    import bound_cases as bd
    c = bd.case(family, band)
    if not ref:
        return c.exp
    b = c.batch
    return oracle.ref_consensus_target_blob(int(b.tlen[0]), b.aln_start, b.aln_off, b.aln_len, b.qstr, b.tstr,
                                            bd.OPTS["min_len"], bd.OPTS["trim"], bd.OPTS["min_cov"])


def segments_digest(segs):
    return hashlib.sha256(repr(segs).encode()).hexdigest()


# ---- the GPU groups --------------------------------------------------------------------------------------------------------

def gpu_groups():
    """{group: (targets, option sets)} of test_ref_graph_gpu.py: the families on which list order decided the answer, and
    the first GPU_RANDOM random inputs with at least 3 reads.  All with the N backbone."""
    out = {}
    for module, names in GPU_FAMILIES:
        for n in names:
            out[f"{module}/{n}"] = ([x[:3] for x in family_inputs(module, n)], (PLAIN, TRIMMED))
    rnd = [x[:3] for x in random_inputs() if len(x[1]) >= 3][:GPU_RANDOM]
    out["random"] = (rnd, (PLAIN, TRIMMED))
    return out


def gpu_expected(consensus_target):
    return {g: {"%d,%d,%d" % o: [[[r0, r1, s.decode()] for r0, r1, s in consensus_target(tl, alns, o[0], o[1], o[2])]
                                 for tl, alns, _ in targets] for o in sets}
            for g, (targets, sets) in gpu_groups().items()}


def main():
    oracle.build()
    assert oracle.ref_graph_lib() is not None, "needs the reference (oracle/_ref/libref_graph.so)"
    doc = dict(source="reference AlnGraphBoost.cpp on oracle/bgl_standin via oracle/_ref/libref_graph.so", block=BLOCK,
               answer="sha256(repr(answers of a block)); an answer is (segments, longest, path, dangling, adjacency) or "
                      "'nonconforming' (make_ref_graph.py)", groups={}, inputs={}, bound={})
    doc["kat"] = segments_digest(kat_answers(oracle.RefGraph, lambda g: g.best_path()))
    for name in group_names():
        t0 = time.perf_counter()
        inputs = group_inputs(name)
        answers = []
        for _, tl, alns, bb, o in runs(inputs):
            a = oracle_answer(tl, alns, bb, o)
            answers.append(a if a == "nonconforming" else ref_answer(tl, alns, bb, o))
        doc["groups"][name] = digests(answers)
        doc["inputs"][name] = [len(inputs), len(answers)]
        print(f"{name}: {len(inputs)} inputs, {len(answers)} answers, {time.perf_counter() - t0:.1f} s")
    for fam, band in BOUND:
        t0 = time.perf_counter()
        doc["bound"][f"{fam}/{band}"] = segments_digest(bound_segments(fam, band, ref=True))
        print(f"bound {fam}/{band}: reference {time.perf_counter() - t0:.1f} s")
    json.dump(doc, open(os.path.join(HERE, "ref_graph_hashes.json"), "w"), indent=1)
    gpu = dict(source=doc["source"], options="min_len,trim,min_weight", groups=gpu_expected(oracle.ref_consensus_target))
    json.dump(gpu, open(os.path.join(HERE, "ref_graph_gpu.json"), "w"), indent=1)
    print("wrote ref_graph_hashes.json and ref_graph_gpu.json")


if __name__ == "__main__":
    main()
