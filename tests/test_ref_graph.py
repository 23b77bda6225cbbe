"""The oracle's graph stages (addAln, mergeNodes, bestPath, consensus) against the reference's own AlnGraphBoost.cpp.

Every parity test of the device ends in oracle/dagcon_oracle.c, a restatement.  Here the restatement is held to the code it
restates: src/cpp/AlnGraphBoost.cpp of the reference, compiled where it lies on a stand-in for the few Boost.Graph containers
and calls it uses (oracle/bgl_standin; its rules stand at the top of its boost/graph/adjacency_list.hpp), with
oracle/ref_graph_glue.cpp as handles (oracle/Makefile, target `ref`: oracle/_ref/libref_graph.so).

  a. the stand-in alone: tests/native/bgl_standin_check.cpp asserts its rules one by one, also under ASan + UBSan, and fails
     on each of the four wrong builds; tests/native/ref_graph_sanitize.cpp walks the reference's loops over its iterators
     under the same sanitizers.
  b. the reference's two known-answer tests through oracle.RefGraph.
  c. oracle == reference on the inputs of tests/golden/make_ref_graph.py (1,500 random pileups and every family of the
     merge, bestPath, build and cut limit tests; the bound inputs on their segments): consensus segments, longest consensus,
     bestPath's nodes, danglingNodes, and the merged graph vertex by vertex with both list orders.
  d. the reference's answers are committed as SHA-256 digests per block (tests/golden/ref_graph_hashes.json): the oracle is
     compared with those everywhere, and live, answer by answer, where oracle/_ref/libref_graph.so exists.
  e. the comparison is sensitive to list order: the reference built on four wrong stand-ins is rejected by named families.

What this leaves unpinned is Boost.Graph itself: that the stand-in's rules are BGL's is read off BGL's documentation, not run.
"""
import ctypes
import functools
import json
import os
import subprocess
import time

import pytest

import oracle
from util import golden_module

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
ORACLE = os.path.dirname(os.path.abspath(oracle.__file__))
STANDIN = os.path.join(ORACLE, "bgl_standin")
REF_SRC = os.path.join(oracle.REFERENCE, "src", "cpp")
REF_FILES = [os.path.join(REF_SRC, "AlnGraphBoost.cpp"), os.path.join(REF_SRC, "Alignment.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

mg = golden_module("make_ref_graph")


def have_reference_source():
    return all(os.path.exists(f) for f in REF_FILES)


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "ref_graph_hashes.json")))


@functools.lru_cache(maxsize=None)
def oracle_answers(group):
    """[(run, answer)] of one group from the oracle, computed once per process."""
    t0 = time.perf_counter()
    rs = list(mg.runs(mg.group_inputs(group)))
    out = [(r, mg.oracle_answer(*r[1:])) for r in rs]
    print(f"{group}: {len(out)} answers from the oracle in {time.perf_counter() - t0:.1f} s")
    return out


def _compile(args, **kw):
    return subprocess.Popen(["g++", "-std=c++14"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)


def _finish(procs):
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out[-3000:]


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))


# ---- a. the stand-in alone ---------------------------------------------------------------------------------------------

def test_standin_keeps_its_rules_and_the_check_sees_each_wrong_build(tmp_path):
    """bgl_standin_check.cpp: exit status 0 plain and under ASan + UBSan; status 1 on each of BGL_STANDIN_WRONG = 1 .. 4, at
    the rule that build breaks (out-list order, in-list order, order after clear_vertex, order of edges())."""
    src = os.path.join(HERE, "native", "bgl_standin_check.cpp")
    exe = {k: str(tmp_path / f"check_{k}") for k in ("plain", "san", 1, 2, 3, 4)}
    procs = [_compile(["-O1", "-g", "-I", STANDIN, src, "-o", exe["plain"]]),
             _compile(["-O1", "-g", *SANITIZE, "-I", STANDIN, src, "-o", exe["san"]])]
    procs += [_compile(["-O0", f"-DBGL_STANDIN_WRONG={v}", "-I", STANDIN, src, "-o", exe[v]]) for v in (1, 2, 3, 4)]
    _finish(procs)
    for k in ("plain", "san"):
        r = _run(exe[k])
        assert r.returncode == 0 and "every rule holds" in r.stdout, (k, r.stdout, r.stderr[-3000:])
    where = {1: "outs(0, g)", 2: "ins(2, g)", 3: "ins(5, h)", 4: "all_edges(g)"}
    for v, expr in where.items():
        r = _run(exe[v])
        assert r.returncode == 1 and r.stdout.startswith("FAILED") and expr in r.stdout, (v, r.stdout, r.stderr[-2000:])


def _parse_pileup(line):
    head, tail = line.split(" => ")
    f = head.split(" ")
    assert f[0] == "pileup" and f[2] == "tlen" and f[10] == "bb"
    tl, trim, mw, ml = int(f[3]), int(f[5]), int(f[7]), int(f[9])
    bb = None if f[11] == "-" else f[11].encode()
    reads = f[12:]
    alns = [(int(reads[i]), reads[i + 1].encode(), reads[i + 2].encode()) for i in range(0, len(reads), 3)]
    t = tail.split(" ")
    assert t[0] == "longest" and t[2] == "dangling" and t[4] == "segments"
    segs = []
    for s in t[5:]:
        r0, r1, seq = s.split("_")
        segs.append((int(r0), int(r1), seq.encode()))
    return (tl, alns, bb, (ml, trim, mw)), (segs, t[1][1:-1].encode(), bool(int(t[3])))


def test_reference_loops_on_the_standin_under_sanitizers(tmp_path, oracle_lib):
    """ref_graph_sanitize.cpp linked with the reference's AlnGraphBoost.cpp and Alignment.cpp, all three under ASan + UBSan:
    the RawConsensus input (and printGraph: reapNodes, remove_vertex) and 24 seeded pileups run clean, the known answer
    comes out, and what the program prints for the pileups is what the oracle answers for the inputs it prints.  Needs the
    reference's source; where that is absent there is nothing to link, and the stand-in's own check above is what runs."""
    if not have_reference_source():
        return
    k = json.load(open(os.path.join(GOLD, "kat_graph.json")))["raw_consensus"]
    exe = str(tmp_path / "ref_graph_sanitize")
    _finish([_compile(["-O1", "-g", *SANITIZE, "-ffp-contract=off", "-I", STANDIN, "-I", REF_SRC,
                       os.path.join(HERE, "native", "ref_graph_sanitize.cpp"), *REF_FILES, "-o", exe])])
    r = _run(exe, k["backbone"], k["expected"], *[a[x] for a in k["alignments"] for x in ("t", "q")])
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0].startswith(f"kat {k['expected']} dot_lines ")
    assert len(lines) == 25
    for line in lines[1:]:
        (tl, alns, bb, o), (segs, longest, dangling) = _parse_pileup(line)
        a = mg.oracle_answer(tl, alns, bb, o)
        assert (a[0], a[1], a[3]) == (segs, longest, dangling), line[:200]


# ---- b. the reference's own known-answer tests -----------------------------------------------------------------------------

def test_reference_known_answers(oracle_lib, gold):
    """RawConsensus and DanglingNodes (test/cpp/AlnGraphBoostTest.cpp:11-57; DanglingNodes starts at 0 on purpose): the
    expected values through oracle.RefGraph, and the oracle's consensus, path and graph equal to the reference's."""
    k = json.load(open(os.path.join(GOLD, "kat_graph.json")))
    mine = mg.kat_answers(oracle.Graph, oracle.path_nodes)
    assert mine[0][0].decode() == k["raw_consensus"]["expected"] and mine[1] is k["dangling_nodes"]["expected"]
    assert mg.segments_digest(mine) == gold["kat"]
    if oracle.ref_graph_lib() is not None:
        ref = mg.kat_answers(oracle.RefGraph, lambda g: g.best_path())
        assert ref[0][0].decode() == k["raw_consensus"]["expected"] and ref[1] is k["dangling_nodes"]["expected"]
        assert ref == mine


# ---- c, d. oracle against reference ------------------------------------------------------------------------------------------

PARTS = ("segments", "longest", "path", "dangling", "adjacency")


@pytest.mark.parametrize("group", mg.group_names())
def test_oracle_equals_reference(group, oracle_lib, gold):
    """Every answer of the group (make_ref_graph.py: each input with the N backbone and with the real one, under each of its
    option sets) from the oracle: its digests equal the reference's, committed; and where the reference is built, every
    part of every answer equals the reference's, live."""
    got = oracle_answers(group)
    n_inputs = len({r[0] for r, _ in got})
    assert [n_inputs, len(got)] == gold["inputs"][group]
    dig = mg.digests([a for _, a in got])
    assert dig == gold["groups"][group], [k for k, (a, b) in enumerate(zip(dig, gold["groups"][group])) if a != b]
    if group == "random":
        assert n_inputs == mg.N_RANDOM
        assert not any(a == "nonconforming" for _, a in got)       # random_target stays inside its target
    if oracle.ref_graph_lib() is None:
        return
    t0 = time.perf_counter()
    for r, a in got:
        if a == "nonconforming":
            continue
        b = mg.ref_answer(*r[1:])
        for part, x, y in zip(PARTS, a, b):
            assert x == y, (f"{group} input {r[0]} backbone {'real' if r[3] is not None else 'N'} options {r[4]}: {part} "
                            f"differs (oracle, reference)", x, y)
    print(f"{group}: {n_inputs} inputs, {len(got)} answers equal the reference's, live; reference {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("family,band", mg.BOUND)
def test_bound_inputs_reference_gives_the_fp32_answer(family, band, oracle_lib, gold):
    """The inputs of bound_cases whose scores pass 2^23 (S, P, M above) and the one between 2^22 and 2^23 (S): the
    reference's segments are the oracle's fp32 answer, and for S and P above not the `wide` (exact) answer, which differs
    there.  Digest of the reference's segments committed; live where the reference is built."""
    import bound_cases as bd
    c = bd.case(family, band)
    assert mg.segments_digest(c.exp) == gold["bound"][f"{family}/{band}"]
    if band == "above" and family in ("S", "P"):
        assert c.wide != c.exp
        assert mg.segments_digest(c.wide) != gold["bound"][f"{family}/{band}"]
    if oracle.ref_graph_lib() is None:
        return
    t0 = time.perf_counter()
    ref = mg.bound_segments(family, band, ref=True)
    print(f"{family}/{band}: {c.columns} columns, reference {time.perf_counter() - t0:.1f} s, oracle {c.oracle_seconds:.1f} s")
    assert ref == c.exp
    if band == "above" and family in ("S", "P"):
        assert ref != c.wide


# ---- e. the comparison is sensitive to list order ----------------------------------------------------------------------------

WRONG = {1: "new out-edges go to the front of the out list", 2: "new in-edges go to the front of the in list",
         3: "clear_vertex fills the hole at the other end with that list's last entry", 4: "edges() walks the global list backwards"}
WRONG_FAMILIES = ("merge/deep", "merge/widths", "merge/span", "merge/partial", "bestpath/widths_row")
# (variant, part) -> the families in which that part of at least one answer must differ from the reference's
REJECTED_BY = {
    (1, "segments"): ("merge/widths", "merge/span", "merge/partial", "bestpath/widths_row"),
    (1, "adjacency"): WRONG_FAMILIES,
    (2, "segments"): ("merge/span",),
    (2, "adjacency"): WRONG_FAMILIES,
    (3, "adjacency"): ("merge/deep", "merge/span", "merge/partial"),
}


@pytest.fixture(scope="module")
def wrong_libs(tmp_path_factory):
    """The reference on each wrong stand-in (-DBGL_STANDIN_WRONG=v, used by this test alone), built into a temporary
    directory; None where the reference's source is absent."""
    if not have_reference_source():
        return None
    d = tmp_path_factory.mktemp("wrong_standins")
    so = {v: str(d / f"libref_graph_wrong{v}.so") for v in WRONG}
    _finish([_compile(["-O2", "-fPIC", "-ffp-contract=off", "-shared", "-Wl,-Bsymbolic", f"-DBGL_STANDIN_WRONG={v}",
                       "-DREF_GRAPH_GLUE_ACCESS", "-I", STANDIN, "-I", REF_SRC, "-o", so[v],
                       os.path.join(ORACLE, "ref_graph_glue.cpp"), *REF_FILES, "-lpthread"]) for v in WRONG])
    return {v: oracle._bind_ref_graph(ctypes.CDLL(so[v])) for v in WRONG}


def test_wrong_standins_are_rejected_by_named_families(wrong_libs, oracle_lib):
    """The reference built on a stand-in that breaks one container rule no longer gives the oracle's answers, and which
    family notices is known:

      1 (out lists reversed)   consensus segments change in widths, span, partial and widths_row (bestPath's first-best
                               choice among equal scores follows out-list order); the graph in every family
      2 (in lists reversed)    segments change in span; the graph in every family
      3 (clear_vertex swaps)   the merged graph changes in deep, span and partial (lists that a merge took a middle entry
                               out of); the segments of these families do not (measured over all inputs of
                               make_ref_graph.py: segments change in 31 of the 6,016 random answers and in no family)
      4 (edges() backwards)    unobservable through this reference code, asserted as such: its one use of edges() is
                               AlnGraphBoost.cpp:377-378, `for (boost::tie(ei, ee) = edges(_g); ei != ee; ++ei)
                               _g[*ei].visited = false;`, which writes the same value to every edge in any order.
                               (printGraph's write_graphviz is the other walk; nothing here reads its text.)

    Needs the reference's source to build from; without it nothing can be built wrongly, and the test has nothing to do."""
    if wrong_libs is None:
        return
    differs = {}                                       # (variant, part) -> {family: answers that differ}
    for fam in WRONG_FAMILIES:
        for r, a in oracle_answers(fam):
            assert a != "nonconforming"
            for v, lib in wrong_libs.items():
                b = mg.ref_answer(*r[1:], lib=lib)
                for part, x, y in zip(PARTS, a, b):
                    if x != y:
                        d = differs.setdefault((v, part), {})
                        d[fam] = d.get(fam, 0) + 1
    for key in sorted(differs):
        print(f"wrong stand-in {key[0]} ({WRONG[key[0]]}): {key[1]} differs in", differs[key])
    for (v, part), fams in REJECTED_BY.items():
        for fam in fams:
            assert differs.get((v, part), {}).get(fam, 0) > 0, f"wrong stand-in {v} ({WRONG[v]}): {part} of {fam} did not notice"
    assert not any(v == 4 for v, _ in differs), {k: d for k, d in differs.items() if k[0] == 4}
    assert (3, "segments") not in differs
