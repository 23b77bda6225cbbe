"""The run loops of k_norm_chunk (csrc/k_norm_run.hip.h) on the CPU, against oracle.normalize_gaps.

tests/native/norm_run_host.cpp includes the header, is built here with the host compiler, AddressSanitizer and
UBSan and -DDG_NCH=32 (a chunk edge every 32 input columns), and runs as a program of its own: the first-pass form
(64-column window, gap columns only) and, as a control for the harness, the unchanged second-pass form (512-column
window), each over the whole alignment as one chunk and cut at dg_chunk_start's columns with the kernel's re-run
driver.  Every comparison is exact.

`overflow` (the first pass hands the chunk to the second pass) and the window.  The first pass refills while its
window spans at most 32 columns; the window starts at most 7 final columns (besides (-, -) columns) in front of the
column it works on.  The program also prints `need`, taken from a plain restatement of normalizeGaps: the longest
stretch from that earliest possible window start to the partner column of a look-up.  need <= 32 therefore means
the first pass can always refill: such a case must not report `overflow`.

Set A and homopolymers: on the one-letter alphabet every gap slides to the end of the alignment, where the surplus of
insertions over deletions piles up into one run of up to ~60 columns, whatever the lengths of the runs that were
drawn.  No 64-column window serves that look-ahead (the previous loop did not either), so on alphabet `A` `overflow`
is accepted exactly where need > 32; on the other three alphabets no case may report it, and nothing is left out.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from norm_cases import plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "norm_run_host.cpp")
WINDOW_SPAN = 32          # the first pass refills while e - o <= 32 (k_norm_run.hip.h)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("norm_run_host") / "norm_run_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-DDG_NCH=32", "-o", exe, SRC])
    return exe


def run_cases(exe, tmp_path, cases):
    """cases: [(q, t, phase)] -> per case {'need': n, ('gc', 'whole'): (flags, q, t), ...}"""
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for q, t, phase in cases:
            assert len(q) == len(t)
            f.write(struct.pack("<II", len(q), phase) + q + t)
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = [dict() for _ in cases]
    for ln in out.stdout.split(b"\n"):
        if not ln:
            continue
        f = ln.split(b" ")
        k = int(f[0])
        if f[1] == b"need":
            res[k]["need"] = int(f[2])
        else:
            strip = lambda s: b"" if s == b"." else s
            res[k][(f[1].decode(), f[2].decode())] = (f[3].decode(), strip(f[4]), strip(f[5]))
    assert all(len(r) == 5 for r in res)
    return res


FORMS = [("gc", "whole"), ("gc", "chunks"), ("big", "whole"), ("big", "chunks")]


# ---- set A ---------------------------------------------------------------------------------------------------------

def set_a(n_cases=20000, seed=20240):
    rng = np.random.default_rng(seed)
    alphabets = [b"A", b"AC", b"ACGT", b"AC"]
    cases, alph_of = [], []
    for k in range(n_cases):
        ai = k % 4
        alph = np.frombuffer(alphabets[ai], np.uint8)
        dots = ai == 3
        n = int(rng.integers(0, 401))
        ins, dele = rng.uniform(0.10, 0.15), rng.uniform(0.05, 0.15)
        sub, dd = rng.uniform(0.03, 0.12), rng.uniform(0.0, 0.03)
        u = rng.random(n)
        base = alph[rng.integers(0, len(alph), n)]
        other = alph[rng.integers(0, len(alph), n)]
        q = np.where(rng.random(n) < sub, other, base)      # a substitution draw (may draw the same base)
        t = base.copy()
        is_ins = u < ins
        is_del = (u >= ins) & (u < ins + dele)
        is_dd = (u >= ins + dele) & (u < ins + dele + dd)
        t[is_ins | is_dd] = 0x2D
        q[is_del | is_dd] = 0x2D
        if dots:
            q[(q == 0x2D) & (rng.random(n) < 0.3)] = 0x2E
            t[(t == 0x2D) & (rng.random(n) < 0.3)] = 0x2E
        cases.append((q.tobytes(), t.tobytes(), int(rng.integers(0, 16))))
        alph_of.append(ai)
    return cases, alph_of


def test_set_a_random_alignments(program, tmp_path, oracle_lib):
    cases, alph_of = set_a()
    assert len(cases) >= 20000
    res = run_cases(program, tmp_path, cases)
    n_over = 0
    for k, ((q, t, _), r) in enumerate(zip(cases, res)):
        exp = oracle_lib.normalize_gaps(q, t)
        for form in FORMS:
            flags, gq, gt = r[form]
            if form[0] == "gc" and flags == "o" and alph_of[k] == 0:
                # one letter: the pile-up at the end of the alignment (see the module docstring)
                assert r["need"] > WINDOW_SPAN, f"case {k} {form}: overflow with need {r['need']}"
                n_over += 1
                continue
            assert flags == "-", f"case {k} {form}: flags {flags!r}, need {r['need']}, alphabet {alph_of[k]}"
            assert (gq, gt) == exp, f"case {k} {form}"
    # most one-letter cases still go through the first pass: the exemption is no way around the comparison
    n_a = 2 * sum(1 for a in alph_of if a == 0)
    print(f"set A: {n_over} of {n_a} one-letter runs reported overflow")
    assert n_over < n_a // 2


# ---- set B ---------------------------------------------------------------------------------------------------------

def set_b():
    """[(name, q, t, phase, expect)]; expect: 'any' (equal or overflow), 'equal' (no overflow), 'overflow', 'badchar'."""
    rng = np.random.default_rng(4711)
    cases = []

    def add(name, q, t, expect="any", phases=range(16)):
        for ph in phases:
            cases.append((f"{name} phase {ph}", bytes(q), bytes(t), ph, expect))

    # gap runs of 20 .. 64 columns in either string.  Random bases: the run stays where it is.  Sliding: the run is a
    # homopolymer in front of 48 more of the same base, so it moves on column by column and meets every refill phase;
    # a run of more than 32 columns then overflows whatever the phase (at some column the window ends exactly at the
    # partner), and one of 64 does not fit the window at all.  A run of 33 that stays put overflows or not with the
    # phase of its first column.
    for L in (20, 24, 26, 30, 33, 64):
        for lead in (5, 12):
            left = plain(rng, lead + 30)
            run = plain(rng, L, avoid=left[-1])
            right = plain(rng, 60, avoid=run[-1])
            stay = "equal" if L <= 24 else "overflow" if L == 64 else "any"
            add(f"run {L} in t, stays", left + run + right, left + b"-" * L + right, stay)
            add(f"run {L} in q, stays", left + b"-" * L + right, left + run + right, stay)
            x = b"ACGT"[(b"ACGT".index(left[-1]) + 1) % 4]
            hp, tail = bytes([x]) * L, bytes([x]) * 48
            right = plain(rng, 40, avoid=x)
            slide = "equal" if L <= 24 else "overflow" if L >= 33 else "any"
            add(f"run {L} in t, slides", left + hp + tail + right, left + b"-" * L + tail + right, slide)
            add(f"run {L} in q, slides", left + b"-" * L + tail + right, left + hp + tail + right, slide)
    # a homopolymer of 200 with a one-base insertion (deletion) in front of it
    left, right = plain(rng, 21, ), plain(rng, 30, avoid=ord("A"))
    left = left[:-1] + (b"C" if left[-2] != ord("C") else b"G")
    add("homopolymer 200, insertion", left + b"A" + b"A" * 200 + right, left + b"-" + b"A" * 200 + right, "equal")
    add("homopolymer 200, deletion", left + b"-" + b"A" * 200 + right, left + b"A" + b"A" * 200 + right, "equal")
    # I(a) I(b) M(a) M(b): the second gap overtakes through the column the first one emptied
    for k in (1, 2, 3, 8, 40):
        for ins in (b"AC", b"A", b"CA", b"ACA"):
            rep = b"AC" * k
            left, right = plain(rng, 17, ) , plain(rng, 25, avoid=ord("C"))
            left = left[:-1] + (b"G" if left[-2] != ord("G") else b"T")
            add(f"hop-over {ins.decode()} x{k} in t", left + ins + rep + right, left + b"-" * len(ins) + rep + right,
                "equal", phases=(0, 3, 9, 15))
            add(f"hop-over {ins.decode()} x{k} in q", left + b"-" * len(ins) + rep + right, left + ins + rep + right,
                "equal", phases=(0, 3, 9, 15))
    # an insertion directly followed by the equal deletion, bursts of 1 .. 9: (-, -) columns in every position of an
    # output group (the lead moves the burst through the eight positions)
    for n in range(1, 10):
        for lead in range(8, 16):
            left = plain(rng, lead)
            burst_q, burst_t = bytearray(), bytearray()
            prev = left[-1]
            for _ in range(n):
                x = plain(rng, 1, avoid=prev)[0]
                burst_q += bytes([x, 0x2D]); burst_t += bytes([0x2D, x])
                prev = x
            right = plain(rng, 40, avoid=prev)
            add(f"ins+del burst {n}, lead {lead}", left + burst_q + right, left + burst_t + right, "equal", phases=(0, 7))
            add(f"del+ins burst {n}, lead {lead}", left + burst_t + right, left + burst_q + right, "equal", phases=(0, 7))
    # mismatches at input offsets 15, 16 and 31 of a 16-byte aligned input: the two columns of one straddle a refill
    for offs in ((15,), (16,), (31,), (15, 16), (15, 16, 31), (14, 15, 16, 17, 30, 31, 32)):
        t = bytearray(plain(rng, 70))
        q = bytearray(t)
        for o in offs:
            q[o] = b"ACGT"[(b"ACGT".index(t[o]) + 2) % 4]
        add(f"mismatch at {offs}", q, t, "equal")
    # a gap column as the very last column, and as the last column of a refill (input offsets 15, 31, 47 of an aligned
    # input), with and without an equal base behind it
    for n in (1, 2, 9, 16, 17, 32, 40):
        s = plain(rng, n)
        add(f"last column insertion, {n}", s[:-1] + s[-1:], s[:-1] + b"-", "equal", phases=(0, 5, 15))
        add(f"last column deletion, {n}", s[:-1] + b"-", s[:-1] + s[-1:], "equal", phases=(0, 5, 15))
        add(f"last column (-,-), {n}", s[:-1] + b"-", s[:-1] + b"-", "equal", phases=(0, 5, 15))
        add(f"last column dots, {n}", s[:-1] + b".", s[:-1] + b".", "equal", phases=(0, 5, 15))
    for at in (15, 31, 47):
        s = bytearray(plain(rng, 80))
        for same in (False, True):
            q, t = bytearray(s), bytearray(s)
            if same:
                q[at + 1] = t[at + 1] = s[at]
                if s[at + 2] == s[at]:
                    q[at + 2] = t[at + 2] = b"ACGT"[(b"ACGT".index(s[at]) + 1) % 4]
            t[at] = 0x2D
            add(f"insertion ends refill at {at}, same={same}", q, t, "equal", phases=(0,))
            add(f"deletion ends refill at {at}, same={same}", t, q, "equal", phases=(0,))
    # lengths around one and two refills, the input pointer at all 16 alignments
    for n in (1, 15, 16, 17, 31, 32, 33):
        for rep in range(3):
            q, t = bytearray(), bytearray()
            while len(q) < n:
                b = b"AC"[rng.integers(0, 2)]
                u = rng.random()
                if u < 0.15:
                    q.append(b); t.append(0x2D)
                elif u < 0.27:
                    q.append(0x2D); t.append(b)
                elif u < 0.35:
                    q.append(b"AC"[rng.integers(0, 2)]); t.append(b)
                else:
                    q.append(b); t.append(b)
            add(f"length {n} #{rep}", q, t, "equal")
    # a byte outside 33..126 at each alignment phase, in either string
    for bad in (0x20, 0x7F, 0x80, 0x0A, 0xFF):
        for at in (0, 7, 20, 40):
            s = bytearray(plain(rng, 41))
            q = bytearray(s); q[at] = bad
            add(f"byte {bad:#x} in q at {at}", q, s, "badchar")
            add(f"byte {bad:#x} in t at {at}", s, q, "badchar")
    return cases


def test_set_b_constructed_cases(program, tmp_path, oracle_lib):
    cases = set_b()
    res = run_cases(program, tmp_path, [(q, t, ph) for _, q, t, ph, _ in cases])
    seen = {"equal": 0, "overflow": 0, "any": 0, "badchar": 0}
    for (name, q, t, _, expect), r in zip(cases, res):
        seen[expect] += 1
        if expect == "badchar":
            for form in FORMS:
                assert "b" in r[form][0], f"{name} {form}: no badchar"
            continue
        exp = oracle_lib.normalize_gaps(q, t)
        for form in FORMS:
            flags, gq, gt = r[form]
            if form[0] == "big":                     # the control: a 512-column window serves all of these
                assert flags == "-" and (gq, gt) == exp, f"{name} {form}: flags {flags!r}"
                continue
            if r["need"] <= WINDOW_SPAN:
                assert flags == "-", f"{name} {form}: overflow with need {r['need']}"
            if expect == "overflow":
                assert flags == "o", f"{name} {form}: flags {flags!r}, an overflow was due"
            elif expect == "equal":
                assert flags == "-" and (gq, gt) == exp, f"{name} {form}: flags {flags!r}"
            else:
                assert flags == "o" or (flags == "-" and (gq, gt) == exp), f"{name} {form}: flags {flags!r}"
    assert all(seen.values()), seen
