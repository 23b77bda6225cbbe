"""Every fixed size of the normalize stage, crossed on purpose (inputs and the model: norm_limit_cases.py,
tests/native/norm_stage_host.cpp).

The stage: k_norm_chunk (first pass, 64-column window; second pass, 512-column ring; the re-run loop and its region of
the scratch), k_norm_scan (offsets, empty and swallowed windows, the trim by whole chunks), k_norm_finish2 (the copy and
the events, 1,024 columns a pass), k_normalize_slow, and the host's chunk and scratch tables (dg_tmp_main, dg_tmp_cap).

  size                                   where                         behind it                                  family
  -------------------------------------  ----------------------------  -----------------------------------------  ---------
  512 input columns a window (DG_NCH)    dg_chunk_start, upload_impl   windows with and without a chunk start,    starts
                                                                       starts on a window's first / last column,
                                                                       len = 512 k and 512 k + 1, 16 byte phases
  refill while e - o <= 32 of 64         dg_norm_run_gc                overflow: the chunk is flagged 2, RETRY    window64
  refill while (e - i) + 32 <= 512       dg_norm_run<512>              overflow: flag 1, k_normalize_slow         window512
  512-column ring, DG_W                  dg_norm_run<512>              e >= 512 and >= 1,024: the ring comes      window512
                                                                       round once and twice
  `dirty`: a push behind the chunk end   k_norm_chunk's re-run loop    the next window taken in, ovf_top bumped,  reruns
                                                                       ch_next; empty windows skipped by k1 / k2
  max(tmp_main / 16, 2^20) columns       dg_tmp_cap, k_norm_chunk      tmp_main + o + need > tmp_cap: flag 1      scratch
  whole chunks by ch_tb against trim     k_norm_scan                   lbases + tb < trim; o >= lo && rbases +    trim
                                                                       tb < trim; column by column; ends meet
  1,024 columns a pass                   k_norm_finish2                adv_tile / run_tile carried; the window    finish
                                                                       begins in a later pass; 4 passes and more
  8 columns a piece, o & 7               k_norm_finish2's copy         head h = (8 - (o & 7)) & 7, nb = 0, w < h  finish
  1 << emit_shift positions              dg_fin_ckpt                   x == 0 && o > lo; a pass's first lane      finish
  255 a byte cell                        dg_store_run                  DG_E_RUN_WIDE: the run with wide cells     finish,
                                                                                                                  window512
  four routes in one batch, tlen         all of them                   first / second pass, slow by window and    routes
                                                                       by scratch side by side; -4 for one target
  tmp_off (shared strings)               dagcon_upload_haps            second pass, re-run and slow path with     shared
                                                                       the scratch at the columns in front

The CPU part (no marker) builds norm_stage_host.cpp with AddressSanitizer and UBSan and runs it as a program of its
own.  It is the stage's own text around the product's headers and says, per window, which route it took.  Before it is
believed it is checked itself: its columns against oracle.normalize_gaps / trim_aln, its insertion runs and checkpoints
against a literal Python restatement of dg_finish_alignment (norm_limit_cases.finish_literal).  Then every family asserts
on the model that it reaches the path it was built for, and prints the figures.

The GPU part compares the device with the oracle by equality, with the arenas poisoned (DAGCON_POISON=15).  THE ROUTE IS
ASSERTED ON THE MODEL AND NOT ON THE DEVICE: the device offers no read-out of ch_flag, and none is added here.  A device
whose routing differs from the model's is therefore caught only where its result differs.

Two figures of the construction were corrected on the model (it is right, and equal to the oracle, in both):
  * the route of a gap run of 40 columns that STAYS goes by the phase of its first column in a refill's 16 columns: the
    first pass serves it at the phases 0 .. 7 (the 64-column window reaches 48 columns from up to 7 columns in front of
    the run) and hands it to the second pass at 8 .. 15.  window64 has it at all 16 phases, in t and in q, and asserts the
    second pass at 8 .. 15; the phases 0 .. 7 and the staying runs of 33 are recorded.  A sliding 40 and any 64 take the
    second pass at every phase.
  * the second pass's bound is between 480 and 495 columns with the refill phase: 479 and below always fit (plain_need
    <= 480), 496 and above never do; 480 and 495 are recorded (measured: 480 second pass at both phases, 495 second pass
    with the run on a refill boundary and slow 9 columns behind one).

timings()["reruns"] counts every repeat of a batch, also one that grows an arena: the families are kept inside the first
guesses of the vertex and the pool arena (test_no_family_runs_again_for_an_arena; window512 carries sixteen plain reads for that), so that
the count is 0, or 1 where a run of more than 255 columns asks for wide cells.

Measured on the model: the scratch turning point is n = 11,264 (22,592 columns, 45 windows): chunk 0 runs again 43 times
and asks for 1,058,272 of the region's 1,048,576 columns; one chunk shorter, 43 re-runs ask for 1,012,184 and fit.  The
finish family asks for 936,408 columns of the region in one batch, every family but scratch stays inside it.

Measured wall times: the CPU part 10 s in all (2 s of them the build of the model, 3 s the 2,400 random alignments).  GPU
part, on an MI355X: starts 0.50 s, window64 0.13 s, window512 0.30 s, reruns 0.15 s, trim 1.80 s (57 trims, the graph at 33),
scratch 1.20 and 1.11 s (trim 0, 5), finish 0.38 .. 0.47 s a case (six of them), routes 1.53 .. 1.63 s a case, shared
0.24 s; every GPU test prints its time (`-s`).
"""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import norm_limit_cases as nl
import oracle
from pbdagcon_amd import capi
from util import batch_from_targets, oracle_batch

gpu = pytest.mark.gpu

LIMITS = [
    ("512 input columns a window", "starts"), ("first pass: refill while e - o <= 32", "window64"),
    ("second pass: refill while (e - i) + 32 <= 512", "window512"), ("512-column ring", "window512"),
    ("dirty re-runs", "reruns"), ("re-run region", "scratch"), ("trim by whole chunks", "trim"),
    ("1,024 columns a pass", "finish"), ("8 columns a piece", "finish"), ("1 << emit_shift positions", "finish"),
    ("255 a byte cell", "finish"), ("four routes, tlen", "routes"), ("tmp_off", "shared"),
]
FAMILIES = ("starts", "window64", "window512", "reruns", "scratch", "trim", "finish", "routes", "shared")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return nl.build_program(tmp_path_factory.mktemp("norm_stage_host"))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("norm_limits"))


_MODELS = {}


def _model(program, work, fam, trim, shift=9):
    """The model's batch for a family, every alignment of it checked against the oracle and the literal loop."""
    key = (fam.name, trim, shift)
    if key not in _MODELS:
        res = nl.run_model(program, work, [fam.model(trim, shift)], name=fam.name)[0]
        assert len(res["alns"]) == len(fam.alns)
        for k, r in enumerate(res["alns"]):
            nl.check_model(oracle, r, fam.alns[k], fam.tlens[k], trim, shift, f"{fam.name}: {fam.names[k]}, trim {trim}, shift {shift}")
        _MODELS[key] = res
    return _MODELS[key]


def _all_settings(program, work, fam):
    return {(tr, sh): _model(program, work, fam, tr, sh) for tr in fam.trims for sh in fam.shifts}


def _fits(res):
    """Every re-run of the batch found room: the routes do not depend on the order of the atomicAdds."""
    return res["B"]["ovf_top"] <= res["B"]["region"]


def test_every_limit_names_its_family():
    assert {f for _, f in LIMITS} == set(FAMILIES)
    for _, f in LIMITS:
        assert f"  {f}" in __doc__


# ---- CPU: dg_norm_run<512> itself ---------------------------------------------------------------------------------------

def _random_long(n_cases=2400, seed=20250):
    """test_norm_run_host.set_a's alphabets and rates on 600 .. 3,000 input columns, gap runs extended with rate `ext`."""
    rng = np.random.default_rng(seed)
    alphabets = [b"A", b"AC", b"ACGT", b"AC"]
    cases, alph_of = [], []
    for k in range(n_cases):
        ai = k % 4
        alph = np.frombuffer(alphabets[ai], np.uint8)
        n = int(rng.integers(600, 3001))
        ins, dele = rng.uniform(0.10, 0.15), rng.uniform(0.05, 0.15)
        sub, dd, ext = rng.uniform(0.03, 0.12), rng.uniform(0.0, 0.03), rng.uniform(0.0, 0.5)
        u = rng.random(n)
        # an extended run: the column repeats the kind of the column in front
        keep = rng.random(n) < ext
        for i in range(1, n):
            if keep[i] and u[i - 1] < ins + dele:
                u[i] = u[i - 1]
        base = alph[rng.integers(0, len(alph), n)]
        other = alph[rng.integers(0, len(alph), n)]
        q = np.where(rng.random(n) < sub, other, base)
        t = base.copy()
        is_ins = u < ins
        is_del = (u >= ins) & (u < ins + dele)
        is_dd = (u >= ins + dele) & (u < ins + dele + dd)
        t[is_ins | is_dd] = 0x2D
        q[is_del | is_dd] = 0x2D
        if ai == 3:
            q[(q == 0x2D) & (rng.random(n) < 0.3)] = 0x2E
            t[(t == 0x2D) & (rng.random(n) < 0.3)] = 0x2E
        cases.append((q.tobytes(), t.tobytes(), int(rng.integers(0, 16))))
        alph_of.append(ai)
    return cases, alph_of


def _run_runs(program, work, cases):
    path = os.path.join(work, "runs.bin")
    with open(path, "wb") as f:
        for q, t, phase in cases:
            f.write(struct.pack("<II", len(q), phase) + q + t)
    out = subprocess.run([program, "runs", path], capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = [dict() for _ in cases]
    for ln in out.stdout.split(b"\n"):
        if ln:
            f = ln.split(b" ")
            if f[1] == b"need":
                res[int(f[0])]["need"] = int(f[2])
            else:
                strip = lambda s: b"" if s == b"." else s
                res[int(f[0])][f[1].decode()] = (f[2] == b"o", strip(f[3]), strip(f[4]), f[5] == b"1")
    assert all(len(r) == 3 for r in res)
    return res


def test_second_pass_form_with_its_ring_wrapped(program, work, oracle_lib):
    """dg_norm_run<512> as one chunk and cut into chunks on alignments of 600 .. 3,000 input columns (its ring comes round in
    every one of them) and on the families' constructed runs.  No overflow: the output is the oracle's.  Overflow only
    where the plain restatement finds a look-up of more than 480 columns; on the two- and four-letter alphabets no random
    case may report it, on the one-letter alphabet (the pile-up at the end, test_norm_run_host.py) fewer than half."""
    cases, alph_of = _random_long()
    assert len(cases) >= 2000
    built = []
    for fam in (nl.window64(), nl.window512(), nl.reruns(), nl.finish()[0]):
        built += [(q, t, k % 16) for k, (_, q, t) in enumerate(fam.alns) if len(q) >= 600]
    res = _run_runs(program, work, cases + built)
    n_over = n_wrapped = n_over_built = 0
    for k, ((q, t, _), r) in enumerate(zip(cases + built, res)):
        exp = oracle_lib.normalize_gaps(q, t)
        for form in ("whole", "chunks"):
            over, gq, gt, wrapped = r[form]
            n_wrapped += wrapped
            if over:
                assert r["need"] > nl.P2_REFILL, f"case {k} {form}: overflow with need {r['need']}"
                if k < len(cases):
                    assert alph_of[k] == 0, f"case {k} {form}: overflow on alphabet {alph_of[k]}, need {r['need']}"
                    n_over += 1
                else:
                    n_over_built += 1
                continue
            assert (gq, gt) == exp, f"case {k} {form}"
        assert r["whole"][3], f"case {k}: the ring did not come round"
    n_a = 2 * sum(1 for a in alph_of if a == 0)
    print(f"second-pass form: {len(cases)} random and {len(built)} constructed alignments, ring wrapped in {n_wrapped} runs; "
          f"{n_over} of {n_a} one-letter runs and {n_over_built} constructed runs reported overflow")
    assert n_over < n_a // 2 and n_over_built > 0


# ---- CPU: the families on the model -------------------------------------------------------------------------------------

def _k0s(r):
    return [w["k0"] for w in r["W"]]


def test_starts_reaches_windows_without_a_start(program, work, oracle_lib):
    fam = nl.starts()
    for res in _all_settings(program, work, fam).values():
        assert _fits(res)
        by = dict(zip(fam.names, res["alns"]))
        for n in (1, 2, 3):
            assert _k0s(by[f"{n} empty"])[:n + 2] == [0] + [-1] * n + [nl.NCH * (n + 1)], n           # and a start on a window's first column
            assert by[f"{n} empty"]["F"][0]["w"] == nl.NCH * (n + 1)
        k = _k0s(by["empty by mismatches"])
        assert k[:2] == [0, -1] and by["empty by mismatches"]["F"][0]["w"] > 1024 + 200              # 512 + 1.5 x 512 and more: two passes of the finish
        assert _k0s(by["last empty"]) == [0, 512, -1]
        assert _k0s(by["start on last column"])[:3] == [0, 2 * nl.NCH - 1, 2 * nl.NCH]
        assert [len(by[f"length {n}"]["W"]) for n in (1, 2, 3, 511, 512, 513, 1024, 1025)] == [1, 1, 1, 1, 1, 2, 2, 3]
        assert _k0s(by["length 513"]) == [0, 512] and _k0s(by["length 1025"]) == [0, 512, 1024] and by["length 1025"]["F"][-1]["w"] == 1
        for s in ("insertion", "deletion"):
            r = by[f"empty by {s}"]
            assert _k0s(r)[:2] == [0, -1] and _k0s(r)[2] > 505 + 530 and r["A"]["slow"] and nl.routes_of(r)[0] == "slow:window"
        assert all(set(nl.routes_of(r)) == {"p1"} for n, r in by.items() if not n.startswith("empty by "))
        assert all(set(nl.routes_of(by[n])) == {"p1"} for n in by if n == "empty by mismatches")
    offs = nl.blob_of(fam.alns)[2]
    phases = {offs[fam.index(f"phase copy {k}")] % 16 for k in range(16)}
    print("starts: byte phases of the 16 copies", sorted(phases), "windows without a start", sum(k < 0 for r in res["alns"] for k in _k0s(r)))
    assert phases == set(range(16))
    assert fam.alns[fam.index("column 0 gap in q")][1][0] == nl.GAP and fam.alns[fam.index("column 0 gap in t")][2][0] == nl.GAP


def test_window64_crosses_the_first_pass(program, work, oracle_lib):
    fam = nl.window64()
    res = _model(program, work, fam, 0)
    _all_settings(program, work, fam)
    assert _fits(res)
    seen, staying40, staying33 = {}, {}, {}
    for name, r in zip(fam.names, res["alns"]):
        L = int(name.split()[1])
        route = nl.routes_of(r)[0]                       # the run lies in chunk 0
        seen.setdefault((L, "slides" in name), set()).add(route)
        if L == 24:
            assert route == "p1", name
        elif L == 64 or (L == 40 and "slides" in name):
            assert route == "p2", name
        elif L == 40 and "phase" in name:
            # a staying run of 40 leaves the first pass where it begins in the upper half of a refill's 16 columns
            phase = int(name.split()[-1])
            staying40.setdefault(route, []).append(phase)
            if phase >= 8:
                assert route == "p2", name
        elif L == 33 and "phase" in name:
            staying33.setdefault(route, []).append(phase := int(name.split()[-1]))
        assert nl.routes_of(r)[1:] == ["p1"] * (len(nl.routes_of(r)) - 1)
    print("window64: routes of chunk 0 by (run, slides):", sorted((k, sorted(v)) for k, v in seen.items()))
    print("window64: staying 40, phases by route (t and q):", staying40, "staying 33:", staying33)
    assert len(staying40["p2"]) == 16                    # phases 8 .. 15, in t and in q


def test_window512_crosses_the_second_pass_and_wraps_its_ring(program, work, oracle_lib):
    fam = nl.window512()
    res = _model(program, work, fam, 0)
    _all_settings(program, work, fam)
    assert _fits(res)
    assert nl.W512_BOUND + 1 == nl.P2_REFILL            # a staying run of L columns: plain_need = L + 1
    fig = {}
    for name, r in zip(fam.names, res["alns"]):
        if not name.startswith("run "):
            continue
        L = int(name.split()[1])
        route, w0 = nl.routes_of(r)[0], r["W"][0]
        fig.setdefault(L, []).append((route, w0["span"]))
        if L <= nl.W512_BOUND:
            assert route == "p2" and not r["A"]["slow"], name
            assert L + 1 <= w0["span"] <= L + 1 + 16, (name, w0["span"])
        if L in nl.W512_ABOVE or L + 1 > nl.P2_REFILL + 16:
            assert route == "slow:window" and r["A"]["slow"], name
    print("window512: (route, largest e - i) by run length:", sorted(fig.items()))
    once, twice = res["alns"][fam.index("wraps once")], res["alns"][fam.index("wraps twice")]
    print("window512: wraps once", once["W"][0], "wraps twice", twice["W"][0])
    assert once["W"][0]["route"] == "p2" and once["W"][0]["wraps"] == 1 and once["W"][0]["reruns"] == 0
    assert twice["W"][0]["route"] == "p2" and twice["W"][0]["wraps"] == 2 and twice["W"][0]["reruns"] == 2 and twice["W"][0]["next"] == 3
    assert twice["W"][0]["asked"] > 0 and len(twice["F"]) == 1 and twice["F"][0]["passes"] == 2


def test_reruns_takes_neighbours_in(program, work, oracle_lib):
    fam = nl.reruns()
    for res in _all_settings(program, work, fam).values():
        assert _fits(res)
        by = dict(zip(fam.names, res["alns"]))
        for n in (1, 2, 6):
            for s in "qt":
                w0 = by[f"across {n} in {s}"]["W"][0]
                assert (w0["reruns"], w0["next"], w0["route"]) == (n, n + 1, "p1")
                assert w0["asked"] == sum((2 * nl.NCH * (j + 1) + 15) & ~7 for j in range(1, n + 1))
        r = by["across an empty window"]
        assert _k0s(r)[:4] == [0, 512, -1, 1536] and (r["W"][0]["reruns"], r["W"][0]["next"]) == (1, 3) and len(r["F"]) == 2
        r = by["ends on len"]
        assert r["W"][0]["next"] == len(r["W"]) and len(r["F"]) == 1 and r["F"][0]["w"] == len(fam.alns[fam.index("ends on len")][1])
        r = by["two dirty chunks"]
        assert [w["reruns"] for w in r["W"]] == [1, 0, 0, 1, 0] and [f["c"] for f in r["F"]] == [0, 2, 3]
    print("reruns: columns of the re-run region asked for", res["B"]["ovf_top"], "of", res["B"]["region"])


_TURN = {}


def _scratch_turn(program, work):
    """The smallest n, a multiple of 256, at which the model sends G AC (AC) x n T to the slow path for want of scratch."""
    if "n" not in _TURN:
        def slow(k):
            a = nl.scratch_aln(256 * k)
            r = nl.run_model(program, work, [nl.model_batch([a], [nl.tlen_of(a)])], name="turn")[0]
            return r["alns"][0]["W"][0]["route"] == "slow:scratch", r
        lo, hi = 1, 128
        assert slow(hi)[0] and not slow(lo)[0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if slow(mid)[0] else (mid, hi)
        _TURN["n"] = 256 * hi
    return _TURN["n"]


def _scratch_family(program, work):
    n = _scratch_turn(program, work)
    rng = np.random.default_rng(9008)
    big, less = nl.scratch_aln(n), nl.scratch_aln(n - 256)
    fam = nl.Family("scratch", trims=(0, 5))
    short = nl.reruns_short(rng, 1)
    fam.target([short[0], big, short[1], short[2]], ["short before", "turning point", "short behind", "short behind too"])
    fam.target([less], ["one chunk shorter, same batch"])
    alone = nl.Family("scratch_alone", trims=(0, 5)).target([less], ["one chunk shorter"])
    return n, fam, alone


def test_scratch_spends_the_rerun_region(program, work, oracle_lib):
    n, fam, alone = _scratch_family(program, work)
    res, res_alone = _model(program, work, fam, 0), _model(program, work, alone, 0)
    _all_settings(program, work, fam); _all_settings(program, work, alone)
    B = res["B"]
    # the floor, not tmp_main / 16, is the region's size
    assert B["region"] == nl.FLOOR and B["tmp_main"] // 16 < nl.FLOOR and res_alone["B"]["region"] == nl.FLOOR
    big, one_less = res["alns"][fam.index("turning point")], res_alone["alns"][0]
    w0 = big["W"][0]
    # by the formula: re-run j takes the window j + 1 in and asks for (2 * (k2 - k0) + 15) & ~7 columns
    need = lambda j: (2 * min(nl.NCH * (j + 1), len(nl.scratch_aln(n)[1])) + 15) & ~7
    total, j = 0, 0
    while total + need(j + 1) <= nl.FLOOR:
        j += 1
        total += need(j)
    print(f"scratch: n = {n}, {len(fam.alns[fam.index('turning point')][1])} columns, {len(big['W'])} windows; chunk 0 re-ran {w0['reruns']} times and asked for "
          f"{w0['asked']} columns of {B['region']}; one chunk shorter: {one_less['W'][0]['reruns']} re-runs, {one_less['W'][0]['asked']} columns")
    assert w0["route"] == "slow:scratch" and big["A"]["slow"] and w0["reruns"] >= j - 1 and w0["asked"] > nl.FLOOR
    assert one_less["W"][0]["route"] == "p1" and not one_less["A"]["slow"] and one_less["W"][0]["next"] == len(one_less["W"])
    assert one_less["W"][0]["asked"] <= nl.FLOOR < one_less["W"][0]["asked"] + need(one_less["W"][0]["reruns"] + 1)
    assert n % 256 == 0 and 40 <= n // 256 <= 50


def _trim_family(program, work):
    """The three alignments with the trims taken from the model's tb per chunk."""
    alns, names = nl.trim_alns()
    base = nl.Family("trim_base").target(alns, names)
    res = _model(program, work, base, 0)
    trims, inside = {0, 1}, {}
    for name, r in zip(names, res["alns"]):
        tbs = [w["tb"] for w in nl.chunks_of(r)]
        total = sum(tbs)
        for k in (1, 2):
            for s in (sum(tbs[:k]), sum(tbs[-k:])):
                trims |= {s - 1, s, s + 1}
        trims |= {total // 2 - 1, total // 2, total // 2 + 1}
        # the left end stops inside chunk g (front < trim <= front + tb) and the right end would skip it whole (behind + tb < trim)
        for g, tb in enumerate(tbs):
            front, behind = sum(tbs[:g]), sum(tbs[g + 1:])
            t = max(behind + tb + 1, front + 1)
            if t <= front + tb:
                inside.setdefault(name, []).append(t)
                trims.add(t)
    fam = nl.Family("trim", trims=sorted(t for t in trims if t >= 0))
    fam.inside = inside
    return fam.target(alns, names)


def test_trim_fires_every_branch_of_the_scan(program, work, oracle_lib):
    fam = _trim_family(program, work)
    seen, per = set(), {}
    for (trim, _), res in _all_settings(program, work, fam).items():
        assert _fits(res)
        for name, r in zip(fam.names, res["alns"]):
            seen |= set(r["A"]["branches"])
            per.setdefault(name, {})[trim] = r["A"]["branches"] or "-"
    base = _model(program, work, fam, 0)
    for name, r in zip(fam.names, base["alns"]):
        print(f"trim: {name}: tb per chunk {[w['tb'] for w in nl.chunks_of(r)]}, k0 {_k0s(r)}; branches by trim {sorted(per[name].items())}")
    by = dict(zip(fam.names, base["alns"]))
    assert any(w["reruns"] for w in by["swallowed"]["W"]) and len(by["swallowed"]["F"]) < len(by["swallowed"]["W"])
    assert _k0s(by["empty ends"])[1] == -1 and _k0s(by["empty ends"])[-1] == -1
    assert seen == set("LlRrxm"), seen
    # the trims at which the left end stops inside the chunk the right end would skip whole: `o >= lo` is false there
    print("trim: left end inside the chunk the right end would skip:", fam.inside)
    assert len(fam.inside) >= 2 and all("x" in per[name][t] for name, ts in fam.inside.items() for t in ts)
    # a trim that ends exactly on a chunk edge is taken column by column: the chunk's last columns may be insertions
    r = by["ends in a run"]
    tb0 = nl.chunks_of(r)[0]["tb"]
    assert nl.chunks_of(r)[0]["w"] == nl.NCH and tb0 == nl.NCH - 2 and r["t"][nl.NCH - 2:nl.NCH] == b"--"
    at = _model(program, work, fam, tb0)["alns"][fam.index("ends in a run")]
    assert "L" not in at["A"]["branches"] and at["A"]["lo"] == nl.NCH - 2 and at["t"][:2] == b"--"
    assert "L" in _model(program, work, fam, tb0 + 1)["alns"][fam.index("ends in a run")]["A"]["branches"]
    assert len(fam.trims) >= 20


def test_finish_crosses_every_pass_and_piece_edge(program, work, oracle_lib):
    fam, want = nl.finish()
    for name, cols in want.items():
        a = fam.alns[fam.index(name)]
        got = nl.ins_runs(*oracle_lib.normalize_gaps(a[1], a[2]))
        assert all(c in got for c in cols), (name, cols, got[:8])
    fig = {}
    for (trim, shift), res in _all_settings(program, work, fam).items():
        assert _fits(res)
        by = dict(zip(fam.names, res["alns"]))
        assert [by[f"takes {k} in"]["F"][c]["passes"] for k, c in ((0, 6), (1, 5), (3, 3), (5, 1))] == [1, 2, 3, 4]
        assert [by[f"takes {k} in"]["W"][c]["reruns"] for k, c in ((0, 6), (1, 5), (3, 3), (5, 1))] == [0, 1, 3, 5]
        F = [f for r in res["alns"] for f in r["F"]]
        fig[(trim, shift)] = dict(passes=sorted({f["passes"] for f in F}), carried=sum(f["carried"] for f in F), ck_first=sum(f["ck_first"] for f in F),
                                  ck_lane0=sum(f["ck_lane0"] for f in F), h=sorted({f["h"] for f in F}), nb0=sum(f["nb"] == 0 for f in F),
                                  w_lt_h=sum(f["w"] < ((8 - (f["o"] & 7)) & 7) for f in F))
        x = fig[(trim, shift)]
        assert set(x["passes"]) >= {1, 2, 3, 4, 5} and x["carried"] >= (20 if trim < 16 else 10) and x["h"] == list(range(8)) and x["nb0"] >= 15 * 8 - 40 and x["w_lt_h"] >= 8
        assert x["ck_lane0"] >= 1
        if shift == 4 and trim < 16:
            assert x["ck_first"] >= 2              # a checkpoint on a chunk's first column, left to the chunk in front
        # every edge read's runs lie in a chunk from column 0 of more than 3,072 columns, where they were put
        for name, cols in want.items():
            r = by[name]
            assert r["F"][0]["o"] == 0 and r["F"][0]["passes"] >= 4 and r["F"][0]["w"] > cols[-1][0] + cols[-1][1]
            if trim == 0:
                assert list(r["C"].values()).count(cols[0][1]) >= 3 and max(r["C"].values()) == max(2, cols[0][1])
        for rot in range(3):
            r = by[f"deletions {rot}.0"]
            assert r["F"][0]["passes"] == 4 and r["W"][0]["reruns"] == 6
            assert r["A"]["n_del"] == 2 + 9 + 1 + 16 + 8 or trim > nl.PASS_COLS        # (the stretches are 10, 16 and 8 target bases)
        # trim 1,100: the trimmed window of the chunks from column 0 begins in their second pass
        if trim > nl.PASS_COLS:
            for name in want:
                assert by[name]["F"][0]["o"] == 0 and nl.PASS_COLS < by[name]["A"]["lo"] < 2 * nl.PASS_COLS
            assert all(r["A"]["hi"] == r["A"]["lo"] for n, r in by.items() if n.startswith("tail"))
        # the right trim ends inside the tails longer than it and skips the shorter ones whole
        if 0 < trim < 16:
            for rr in range(1, 16):
                A = by[f"tail {rr} at o & 7 = 3"]["A"]
                assert ("R" in A["branches"]) == (rr < trim) and "r" in A["branches"]
    for k, v in sorted(fig.items()):
        print("finish: trim, shift", k, v)
    assert nl.long_runs(oracle_lib, fam.alns, 0, fam.tlens)


def _routes_family(program, work):
    n = _scratch_turn(program, work)
    rng = np.random.default_rng(9009)
    big = nl.scratch_aln(n)
    reads = [nl.Cols(rng).plain(900).aln(1), nl.Cols(rng).plain(200).slide_run(40).plain(700).aln(40),
             nl.Cols(rng).plain(300).ins_run(600).plain(500).aln(100), big, nl.Cols(rng).plain(700).del_run(30).plain(400).aln(2000)]
    fam = nl.Family("routes", trims=(0, 5, 50))
    fam.target(reads, ["first pass", "second pass", "slow by window", "slow by scratch", "first pass too"], nl.tlen_of(big))
    tl, alns, names = nl.overrun_target(rng)
    return fam.target(alns, names, tl)


def test_routes_takes_all_four_in_one_target(program, work, oracle_lib):
    fam = _routes_family(program, work)
    for (trim, _), res in _all_settings(program, work, fam).items():
        by = dict(zip(fam.names, res["alns"]))
        assert set(nl.routes_of(by["first pass"])) == {"p1"} and not by["first pass"]["A"]["slow"]
        assert nl.routes_of(by["second pass"])[0] == "p2" and not by["second pass"]["A"]["slow"]
        assert nl.routes_of(by["slow by window"])[0] == "slow:window" and by["slow by window"]["A"]["slow"]
        assert nl.routes_of(by["slow by scratch"])[0] == "slow:scratch" and by["slow by scratch"]["A"]["slow"]
        assert res["B"]["region"] == nl.FLOOR
        # the read past tlen: conforming up to its last chunk
        r = by["past tlen"]
        assert r["A"]["nonconf"] and len(r["F"]) == 3 and not by["fits"]["A"]["nonconf"] and not by["fits too"]["A"]["nonconf"]
        print("routes: trim", trim, {n: nl.routes_of(r) for n, r in by.items()})
    assert nl.long_runs(oracle_lib, fam.alns[:5], 0, fam.tlens[:5])


def test_no_family_runs_again_for_an_arena(program, work, oracle_lib):
    """timings()["reruns"] counts every repeat of a batch, the ones that grow an arena too.  The GPU part expects 0, and 1
    where a run of more than 255 columns is in the batch: so no family may outgrow the first guess of the vertex arena or of the pool arena."""
    fams = [nl.starts(), nl.window64(), nl.window512(), nl.reruns(), nl.finish()[0], _trim_family(program, work),
            _scratch_family(program, work)[1], _routes_family(program, work)]
    bb, alns, _ = _shared_target()
    fams.append(nl.Family("shared").target(alns, [str(k) for k in range(8)], 1500))
    fams.append(nl.Family("shared groups").target(alns[:4], list("0123"), 1500).target(alns[4:], list("4567"), 1500))
    for fam in fams:
        for trim in fam.trims[:1] + fam.trims[-1:]:
            nodes, node_cap, pool, pool_cap = nl.arenas_fit(oracle_lib, fam, trim)
            print(f"{fam.name}, trim {trim}: {nodes} vertices, first guess {node_cap}; {pool} pool words, first guess {pool_cap}")
            assert nodes <= node_cap and pool <= pool_cap, fam.name


# ---- shared strings -----------------------------------------------------------------------------------------------------

def _shared_target():
    """1,500 positions, 8 full-span reads: two haplotypes that differ by a substitution every 40 .. 60 bases outside an (AC)
    repeat across the chunk start at 512; in either group a read with a staying insertion of 64 columns (second pass), one with AC
    inserted in front of the repeat (a re-run) and one with a staying insertion of 600 columns (slow path, wide cells)."""
    rng = np.random.default_rng(9010)
    left = nl.plain(rng, 420)
    left = left[:-1] + (b"T" if left[-2] != ord("T") else b"C")
    bb = left + b"G" + b"AC" * 100 + b"T"
    bb = bb + nl.plain(rng, 1500 - len(bb), avoid=ord("T"))
    subs, x = {}, 30
    while x < 1480:
        if not 400 <= x <= 640:
            subs[x] = next(b for b in b"ACGT" if b not in (bb[x - 1], bb[x], bb[x + 1]))
        x += int(rng.integers(40, 61))
    alns = []
    for k in range(8):
        second, kind = k >= 4, k % 4
        q, t = bytearray(), bytearray()
        for p in range(1500):
            if kind == 1 and p == 200:
                two = [c for c in b"ACGT" if c not in (bb[p - 1], bb[p])][:2]
                q += bytes(two[j & 1] for j in range(64)); t += b"-" * 64
            if kind == 2 and p == 421:
                q += b"AC"; t += b"--"
            if kind == 3 and p == 900:
                two = [c for c in b"ACGT" if c not in (bb[p - 1], bb[p])][:2]
                q += bytes(two[j & 1] for j in range(600)); t += b"-" * 600
            q.append(subs[p] if second and p in subs else bb[p]); t.append(bb[p])
        alns.append((1, bytes(q), bytes(t)))
    return bb, alns, sorted(subs)


def _shared_model(program, work, alns, order, trim):
    """The derived batch as dagcon_upload_haps builds it: the groups' alignments point into the first batch's strings, the
    scratch lies at the columns in front of each in the derived batch."""
    qb, tb, offs = nl.blob_of(alns)
    sel = [alns[i] for i in order]
    rec = nl.model_batch(sel, [1500] * len(sel), trim, 9, shared=(qb, tb, [offs[i] for i in order]))
    res = nl.run_model(program, work, [rec], name="shared")[0]
    for k, r in enumerate(res["alns"]):
        nl.check_model(oracle, r, sel[k], 1500, trim, 9, f"shared: read {order[k]}")
    return res


def test_shared_model_takes_every_route_at_its_own_scratch(program, work, oracle_lib):
    import site_reads_twin as srt
    bb, alns, subs = _shared_target()
    tw = srt.target(1500, alns, 500, 10, (2, 200000))
    assert tw["hap"] == [1] * 4 + [2] * 4, tw["hap"]
    res = _shared_model(program, work, alns, list(range(8)), 10)
    plain_res = nl.run_model(program, work, [nl.model_batch(alns, [1500] * 8, 10)], name="shared_plain")[0]
    assert res["B"]["tmp_main"] == plain_res["B"]["tmp_main"]              # (all 8 reads once: the same columns in front)
    routes = [nl.routes_of(r) for r in res["alns"]]
    print("shared: routes", routes, "re-runs", [[w["reruns"] for w in r["W"]] for r in res["alns"]])
    for g in (0, 4):
        assert set(routes[g]) == {"p1"}
        assert "p2" in routes[g + 1] and not res["alns"][g + 1]["A"]["slow"]
        assert res["alns"][g + 2]["W"][0]["reruns"] == 1 and not res["alns"][g + 2]["A"]["slow"]
        assert "slow:window" in routes[g + 3] and res["alns"][g + 3]["A"]["slow"]
    # a derived batch of one group alone lies elsewhere in the scratch than the reads do in the blob
    one = _shared_model(program, work, alns, [4, 5, 6, 7], 10)
    assert one["B"]["tmp_main"] < res["B"]["tmp_main"] and [nl.routes_of(r) for r in one["alns"]] == routes[4:]


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _poison(monkeypatch, shift=None):
    monkeypatch.setenv("DAGCON_POISON", "15")
    if shift is None or shift == 9:
        monkeypatch.delenv("DAGCON_EMIT_SHIFT", raising=False)
    else:
        monkeypatch.setenv("DAGCON_EMIT_SHIFT", str(shift))


def _normalize_equals_oracle(gpu_ctx_factory, alns, trim):
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=0, min_weight=0)
    got = ctx.normalize(alns, trim=trim)
    assert len(got) == len(alns)
    for k, ((s, q, t), (gs, gq, gt)) in enumerate(zip(alns, got)):
        qn, tn = oracle.normalize_gaps(q, t)
        assert (gq, gt, gs) == oracle.trim_aln(qn, tn, s, trim), f"alignment {k}, trim {trim}"


def _graph_and_consensus(gpu_ctx_factory, fam, trim, status=None):
    from test_gpu_parity import _check_graphs
    batch = fam.batch()
    want_reruns = 1 if nl.long_runs(oracle, fam.alns, trim, fam.tlens) else 0
    ok = [t for t in range(batch.n_targets) if status is None or status[t] == 0]
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(batch, strict=False)
    assert ctx.target_status.tolist() == (status or [0] * batch.n_targets)
    graphs = _check_graphs(ctx, batch, trim, False, targets=ok)
    assert ctx.timings()["reruns"] == want_reruns
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0)
    got = ctx.consensus(batch, strict=False)
    # (the oracle stops at a non-conforming alignment: it gets the targets that are to complete)
    exp = oracle_batch(batch_from_targets([(tl, al, None) for t, (tl, al, _) in enumerate(fam.targets) if t in ok]), 0, 0, trim, 0)
    assert ctx.target_status.tolist() == (status or [0] * batch.n_targets)
    for k, t in enumerate(ok):
        assert got[t] == exp[k], f"target {t}: consensus differs"
    assert all(got[t] == [] for t in range(batch.n_targets) if t not in ok)
    assert ctx.timings()["reruns"] == want_reruns
    return batch, graphs


def _against_the_literal_loop(gpu_ctx_factory, fam, trim, graphs, status):
    """The same alignments, already normalised, through FLAG_RAW_ALIGNMENTS (k_normalize_slow's dg_finish_alignment alone):
    the same graphs and the same status as the chunked path left."""
    norm = [(tl, [(s,) + oracle.normalize_gaps(q, t) for s, q, t in alns], None) for tl, alns, _ in fam.targets]
    b = batch_from_targets(norm)
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=trim, min_weight=0, flags=capi.FLAG_RAW_ALIGNMENTS | capi.FLAG_STOP_AFTER_BUILD)
    ctx.consensus(b, strict=False)
    st = ctx.target_status.tolist()
    assert st == status
    assert [ctx.debug_graph(t) for t in range(b.n_targets) if st[t] == 0] == graphs


def _timed(name, t0):
    print(f"{name}: {time.time() - t0:.2f} s")


@gpu
@pytest.mark.parametrize("name", ["starts", "window64", "window512", "reruns"])
def test_family_on_the_device(gpu_ctx_factory, monkeypatch, name):
    t0 = time.time()
    _poison(monkeypatch)
    fam = getattr(nl, name)()
    for trim in fam.trims:
        _normalize_equals_oracle(gpu_ctx_factory, fam.alns, trim)
        _graph_and_consensus(gpu_ctx_factory, fam, trim)
    _timed(name, t0)


@gpu
def test_trim_on_the_device(gpu_ctx_factory, monkeypatch, program, work):
    t0 = time.time()
    _poison(monkeypatch)
    fam = _trim_family(program, work)
    for trim in fam.trims:
        _normalize_equals_oracle(gpu_ctx_factory, fam.alns, trim)
    # the graph and the consensus at a trim of every kind: on a chunk edge (the chunk that ends in insertion columns) and
    # one column past it, every trim with `o >= lo` false, the ends met, the largest, and 0 and 1
    r = _model(program, work, fam, 0)["alns"][fam.index("ends in a run")]
    tb0 = nl.chunks_of(r)[0]["tb"]
    some = {0, 1, tb0, tb0 + 1, fam.trims[-1]} | {t for ts in fam.inside.values() for t in ts}
    some |= {t for t in fam.trims if any("m" in x["A"]["branches"] for x in _model(program, work, fam, t)["alns"])
             and not all("m" in x["A"]["branches"] for x in _model(program, work, fam, t)["alns"])}
    print("trim: graph and consensus at", sorted(some))
    assert len(some) >= 10 and some <= set(fam.trims)
    for trim in sorted(some):
        _graph_and_consensus(gpu_ctx_factory, fam, trim)
    _timed("trim", t0)


@gpu
@pytest.mark.parametrize("trim", [0, 5])
def test_scratch_on_the_device(gpu_ctx_factory, monkeypatch, program, work, trim):
    t0 = time.time()
    _poison(monkeypatch)
    n, fam, alone = _scratch_family(program, work)
    _normalize_equals_oracle(gpu_ctx_factory, fam.alns, trim)
    _normalize_equals_oracle(gpu_ctx_factory, alone.alns, trim)
    _graph_and_consensus(gpu_ctx_factory, fam, trim)
    _timed(f"scratch trim {trim}", t0)


@gpu
@pytest.mark.parametrize("shift", [9, 4])
@pytest.mark.parametrize("trim", [0, 7, 1100])
def test_finish_on_the_device(gpu_ctx_factory, monkeypatch, trim, shift):
    t0 = time.time()
    _poison(monkeypatch, shift)
    fam, _ = nl.finish()
    if shift == 9:
        _normalize_equals_oracle(gpu_ctx_factory, fam.alns, trim)
    status = [0] * len(fam.targets)
    _, graphs = _graph_and_consensus(gpu_ctx_factory, fam, trim)
    _against_the_literal_loop(gpu_ctx_factory, fam, trim, graphs, status)
    _timed(f"finish trim {trim} shift {shift}", t0)


@gpu
@pytest.mark.parametrize("trim", [0, 5, 50])
def test_routes_on_the_device(gpu_ctx_factory, monkeypatch, program, work, trim):
    t0 = time.time()
    _poison(monkeypatch)
    fam = _routes_family(program, work)
    _normalize_equals_oracle(gpu_ctx_factory, fam.alns, trim)
    status = [0, -4]
    _, graphs = _graph_and_consensus(gpu_ctx_factory, fam, trim, status)
    _against_the_literal_loop(gpu_ctx_factory, fam, trim, graphs, status)
    _timed(f"routes trim {trim}", t0)


@gpu
def test_shared_on_the_device(oracle_lib, monkeypatch):
    """Through set_hap_consensus / upload_haps: the derived batch of the two groups against a fresh context and the oracle
    on the groups' strings (test_hap_consensus._hap_run), the reads in the model's order."""
    from test_hap_consensus import _hap_run, _strings_call
    t0 = time.time()
    _poison(monkeypatch)
    bb, alns, subs = _shared_target()
    r = _hap_run(_strings_call([(bb, alns)], [1500]), [(bb, alns)], [1500], 3, 500, 10)
    assert r["tally"]["split"].tolist() == [1] and r["map"]["label"].tolist() == [1, 2]
    assert r["map"]["aln_src"].tolist() == list(range(8)) and r["status"] == [0]
    assert r["reruns"] == 1                             # the insertions of 600 columns
    (s1,), (s2,) = r["got"]
    assert s1[2] != s2[2] and len(s1[2]) > 1400 and len(s2[2]) > 1400
    _timed("shared", t0)
