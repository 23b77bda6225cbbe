"""The step of k_win_keep (dg_keep_step of csrc/k_keep.hip.h) on the CPU, against hap_contigs_twin.keep.

tests/native/keep_host.cpp includes the header, is built here with the host compiler, AddressSanitizer and UBSan, and runs
as a program of its own on position arrays of exactly n words.  The expected records come from the twin, which is written
from rule 12 of include/dagcon.h and not from the header.  The program also says how many steps of 64 it took: the wave
leaves the loop at the step that holds i1.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import hap_contigs_twin as hct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "keep_host.cpp")
BB = 0x80000000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keep_host") / "keep_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def run_cases(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for pos, lo, hi in cases:
            f.write(struct.pack("<3I", len(pos), lo, hi))
            f.write(np.asarray(pos, np.uint32).tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().splitlines()]
    assert [r[0] for r in res] == list(range(len(cases)))
    return [r[1:] for r in res]


def check(cases, res, names=None):
    for k, ((pos, lo, hi), got) in enumerate(zip(cases, res)):
        tag = "case %d%s" % (k, " (%s)" % names[k] if names else "")
        plain = [int(p) & ~BB for p in pos]
        exp = hct.keep(plain, lo, hi)
        assert got[:4] == exp, (tag, got, exp)
        # the loop ends at the step that holds i1; without one (or without an i0) it reads the whole segment
        n = len(pos)
        i0 = next((i for i in range(n) if plain[i] > lo), None)
        i1 = None if i0 is None else next((i for i in range(i0, n) if plain[i] > hi), None)
        assert got[4] == (-(-n // 64) if i1 is None else i1 // 64 + 1), (tag, got)


def ramp(n, first=1):
    return list(range(first, first + n))


def constructed():
    cases, names = [], []

    def add(name, pos, lo, hi):
        assert lo <= hi
        cases.append((pos, lo, hi)); names.append(name)

    for n in (1, 63, 64, 65, 128, 129):
        add(f"n={n} all kept", ramp(n), 0, n)
        add(f"n={n} all kept, hi far", ramp(n), 0, 10 * n)
        add(f"n={n} nothing over lo", ramp(n), n, n + 5)
        add(f"n={n} last base alone", ramp(n), n - 1, n)
        add(f"n={n} first base alone", ramp(n), 0, 1)
        add(f"n={n} lo == hi at the front", ramp(n), 0, 0)
        add(f"n={n} lo == hi in the middle", ramp(n), n // 2, n // 2)
        add(f"n={n} kind bit set on every base", [p | BB for p in ramp(n)], n // 3, n - 1)
    # i0 at index 0, 63 and 64; i1 at 64, 65 and n (P(i) = i + 1: i0 = lo, i1 = hi)
    for i0 in (0, 63, 64):
        for i1 in (64, 65, 129):
            if i1 > i0:
                add(f"i0={i0} i1={i1 if i1 < 129 else 'n'}", ramp(129), i0, i1 if i1 < 129 else 129)
    add("i0 on lane 63, i1 on lane 0 of the next step", ramp(129), 63, 64)
    add("i0 and i1 in one step", ramp(129), 70, 90)
    add("i0 and i1 on neighbouring lanes", ramp(129), 70, 71)
    add("i0 on the last lane of the last step", ramp(128), 127, 200)
    add("plateau below lo, then a ramp", [1] * 5 + [0] + [1] * 64 + ramp(59, 2), 1, 30)
    add("P(i0) > hi: empty", [1, 2, 3, 50, 4, 5], 3, 10)
    add("P(i0) > hi in the second step: empty", [1] * 64 + [50] + ramp(64), 3, 10)
    # non-monotone positions that cross lo twice: the first crossing counts, and the dip below lo stays in the part
    add("crosses lo twice", [1, 2, 6, 7, 2, 3, 6, 7, 8, 20, 9], 5, 10)
    add("crosses lo twice, over two steps", [1] * 60 + [6, 7, 2, 3] + [2] * 10 + [6, 7, 8, 20, 9], 5, 10)
    add("crosses hi twice: the first crossing ends it", [1, 6, 7, 20, 6, 7, 30], 5, 10)
    add("a dip behind i0, hi in a later step", [1] * 10 + [6] + [2] * 100 + [7, 8, 11, 5], 5, 10)
    return cases, names


def test_constructed_segments(program, tmp_path):
    cases, names = constructed()
    res = run_cases(program, tmp_path, cases)
    check(cases, res, names)
    by = dict(zip(names, res))
    # the boundaries by name, so that a twin that is wrong the same way does not hide them
    assert by["i0 on lane 63, i1 on lane 0 of the next step"] == (63, 64, 64, 64, 2)
    assert by["i0=64 i1=65"] == (64, 65, 65, 65, 2) and by["i0=0 i1=n"] == (0, 129, 1, 129, 3) and by["i0=63 i1=64"][:2] == (63, 64)
    assert by["P(i0) > hi: empty"] == (0, 0, 0, 0, 1) and by["n=1 nothing over lo"] == (0, 0, 0, 0, 1)
    assert by["n=64 lo == hi in the middle"] == (0, 0, 0, 0, 1)                 # P(i0) = lo + 1 > hi
    assert by["crosses lo twice"] == (2, 9, 6, 8, 1)


def test_high_base_in_front_of_i0(program, tmp_path):
    """A base with P > hi in front of i0 must not end the part.  On plain numbers with lo <= hi there is no such base (it
    would be over lo too, so it would be i0 itself, and the part empty: the cases above).  The step takes the two masks
    as they come, though, and the kernel's contract is on the masks: lanes in front of i0 are masked out of the hi ballot
    in the step that finds i0, and the hi bits of earlier steps are never looked at.  The program applies the step to
    whatever thresholds it is given, so lo > hi -- which dagcon_set_window_keep refuses -- makes the masks disagree."""
    same = [1, 2, 7, 8, 3, 11, 4, 4, 13]                       # lo 10, hi 5: i0 = 5; lanes 2 and 3 are over hi in front of it
    early = [7, 8] + [1] * 70 + [11, 3, 12]                    # i0 = 72; the two bases over hi lie in step 0
    behind = [7, 8] + [1] * 70 + [11, 3, 12]                   # lo 10, hi 11: the part runs from 72 to the 12 behind it
    cases = [(same, 10, 5), (early, 10, 5), (behind, 10, 11), ([1, 9, 1, 1, 6, 7, 2, 9, 1], 5, 8)]
    res = run_cases(program, tmp_path, cases)
    check(cases, res)
    assert res[0][:4] == (0, 0, 0, 0) and res[1][:4] == (0, 0, 0, 0)         # P(i0) > hi: empty -- and found at i0, not earlier
    assert res[0][4] == 1 and res[1][4] == 2                                 # (the early bases did not end the loop in step 0)
    assert res[2][:4] == (72, 74, 11, 3) and res[3][:4] == (0, 0, 0, 0)


def test_random_segments(program, tmp_path):
    rng = np.random.default_rng(1201)
    cases = []
    for _ in range(3000):
        n = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, 200, int(rng.integers(1, 300))]))
        kind = int(rng.integers(0, 3))
        if kind == 0:                                           # a path's positions: non-decreasing, runs of equal values (insertions)
            pos = np.cumsum(rng.random(n) < 0.8) + int(rng.integers(0, 3))
        elif kind == 1:                                         # anything
            pos = rng.integers(0, 40, size=n)
        else:                                                   # a ramp with dips
            pos = np.arange(1, n + 1) - (rng.random(n) < 0.1) * rng.integers(0, 30, size=n)
            pos = np.maximum(pos, 0)
        top = int(pos.max()) + 2
        lo = int(rng.integers(0, top))
        hi = int(rng.integers(lo, top + 1))
        if rng.random() < 0.3:
            pos = pos | (BB * (rng.random(n) < 0.5))
        cases.append((pos.astype(np.uint32).tolist(), lo, hi))
    res = run_cases(program, tmp_path, cases)
    check(cases, res)
    kept = sum(1 for r in res if r[1] > r[0])
    assert 500 < kept < 2900
