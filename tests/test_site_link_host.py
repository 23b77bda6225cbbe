"""The pair test of k_lk_pairs (dg_lk_cells / dg_lk_pair / dg_lk_rows of csrc/k_site_link.hip.h) on the CPU, against
site_link_twin.

tests/native/site_link_host.cpp includes the header, is built here with the host compiler, AddressSanitizer and UBSan, and
runs as a program of its own on rows of exactly `words` words.  It counts the four cells twice, by words and bit by bit;
the expected cells and answers here come from the twin, which works on Python ints and is written from rule 13 of
include/dagcon.h, not from the header.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import site_link_twin as slt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "site_link_host.cpp")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("site_link_host") / "site_link_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def run_cases(exe, tmp_path, cases):
    """cases: (words, ppm, min_cell, (Pi, Mi, Pj, Mj) as Python ints)."""
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for words, ppm, cell, rows in cases:
            f.write(struct.pack("<3I", words, ppm, cell))
            for r in rows:
                assert r >> (64 * words) == 0
                f.write(b"".join(struct.pack("<Q", (r >> (64 * w)) & M64) for w in range(words)))
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().splitlines()]
    assert [r[0] for r in res] == list(range(len(cases)))
    return [r[1:] for r in res]


def check(cases, res):
    for k, ((words, ppm, cell, rows), got) in enumerate(zip(cases, res)):
        cells = slt.cells(*rows)
        assert got[:4] == cells, (k, got, cells)
        assert got[4] == int(slt.pair_cells(*cells, (ppm, cell, 0, 0))), (k, got, cells, ppm, cell)


def bits(xs):
    return sum(1 << x for x in xs)


def test_edge_values(program, tmp_path):
    """The edges tests/test_site_link.py names, as rows: the conflict bound met exactly and missed by one read, cell ==
    min_cell and one fewer, same == diff, same == diff == 0, an empty row M (a site without a second class), and the
    largest values: 4,094 alignments all in one cell, the bound's product past 2^32."""
    ten = (bits(range(7)), bits(range(7, 10)), bits(range(6)), bits(range(6, 10)))                  # 6 3 1 0
    eleven = (bits(range(7)), bits(range(7, 11)), bits(list(range(6)) + [10]), bits(range(6, 10)))  # 6 3 1 1
    same3 = (bits(range(7)), bits(range(7, 10)), bits(range(7)), bits(range(7, 10)))
    same2 = (bits(range(7)), bits(range(7, 10)), bits(range(7)), bits(range(7, 9)))
    half = (bits(range(4)), bits(range(4, 8)), bits([0, 1, 4, 5]), bits([2, 3, 6, 7]))
    anti = (bits(range(7)), bits(range(7, 10)), bits(range(7, 10)), bits(range(7)))                 # the two sites name the alleles the other way round
    no_m = (bits(range(10)), 0, bits(range(7)), bits(range(7, 10)))
    full = bits(range(4094))
    cases = [(1, 100000, 3, ten), (1, 99999, 3, ten), (1, 100000, 3, eleven), (1, 181819, 3, eleven), (1, 181818, 3, eleven),
             (1, 100000, 3, same3), (1, 100000, 4, same3), (1, 100000, 3, same2), (1, 100000, 2, same2),
             (1, 499999, 2, half), (1, 500000, 2, half), (1, 1000000, 3, half),
             (1, 1000000, 1, (0, 0, 0, 0)), (1, 1, 1, (3, 0, 0, 3)), (1, 1000000, 1, no_m), (1, 100000, 3, anti), (1, 1, 3, same3), (1, 1, 3, ten),
             (64, 1, 2047, (full, 0, full, 0)), (64, 1000000, 1, (full, 0, 0, full)),
             (64, 1, 2047, (bits(range(2047)), bits(range(2047, 4094)), bits(range(2047)), bits(range(2047, 4094)))),
             (64, 4294967295, 4294967295, (bits(range(2047)), bits(range(2047, 4094)), bits(range(2047, 4094)), bits(range(2047))))]
    res = run_cases(program, tmp_path, cases)
    check(cases, res)
    assert [r[4] for r in res] == [1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    assert res[0][:4] == (6, 3, 1, 0) and res[2][:4] == (6, 3, 1, 1) and res[9][:4] == (2, 2, 2, 2) and res[15][:4] == (0, 0, 7, 3)
    assert res[18][:4] == (4094, 0, 0, 0) and res[20][:4] == (2047, 2047, 0, 0)


@pytest.mark.parametrize("words", [1, 2, 65])
def test_random_rows(program, tmp_path, words):
    """Random rows of one, two and 65 words (65: past the 64 words a target of 4,094 alignments needs) with random bounds:
    a read is in P, in M or in neither at a site, never in both, as the kernel's rows are; some cases break that too."""
    rng = np.random.default_rng(1300 + words)
    n = 64 * words
    cases = []
    for k in range(600):
        rows = []
        for _ in range(2):
            dens = rng.choice([0.02, 0.3, 0.9])
            state = rng.choice(3, size=n, p=[1 - dens, dens * 0.7, dens * 0.3])
            P, M = bits(np.flatnonzero(state == 1).tolist()), bits(np.flatnonzero(state == 2).tolist())
            if k % 50 == 49:
                M |= P & bits(range(0, n, 3))
            rows += [P, M]
        if k % 3 == 0:                                                 # the second site a noisy copy of the first: partners are common
            flip = bits(np.flatnonzero(rng.random(n) < 0.05).tolist())
            rows[2], rows[3] = rows[0] & ~flip | rows[1] & flip, rows[1] & ~flip | rows[0] & flip
            if k % 6 == 0:
                rows[2], rows[3] = rows[3], rows[2]
        ppm = int(rng.choice([1, 50000, 100000, 500000, 1000000, int(rng.integers(1, 1000001))]))
        cases.append((words, ppm, int(rng.choice([1, 2, 3, 10, int(rng.integers(1, 40))])), tuple(rows)))
    res = run_cases(program, tmp_path, cases)
    check(cases, res)
    yes = sum(r[4] for r in res)
    assert 60 < yes < 540
    assert any(r[2] + r[3] > r[0] + r[1] and r[4] for r in res)       # partners through the other pair of cells too
