"""The row scan of k_lists_lanes (csrc/k_lists_row.hip.h) on the CPU, against a plain statement of the list rule.

tests/native/lists_row_host.cpp includes the header, is built here with the host compiler, AddressSanitizer and UBSan,
and runs as a program of its own on rows of exactly K words.  The expected lists come from `model` below, written from
the rule and not from the header:

  entry 0 is the chain neighbour, counted by the reads that hold it; an id in [ulo, uhi) is an inserted vertex of one
  read, an entry of its own with count 1 + extra; any other non-zero id is an entry at its first read, with the number
  of reads that hold it plus the extra of that first read; the order is the order of first reads.  Arrival rows: DEL
  and DUP cells bring no entry, n_cov counts the non-zero cells, n_match those that are no DEL, last_base is the base
  of the last non-zero cell.  More than four distinct "other" ids: the overflow mark, and nothing else is promised.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "lists_row_host.cpp")
DEL, DUP = 0x1FFFFFF, 0x1FFFFFE
TABLE = 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lists_row_host") / "lists_row_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def model(cells, arrival, chain, ulo, uhi):
    entries, others = [], {}
    c0 = n_cov = n_match = last_base = 0
    for c in cells:
        ident, extra = c & 0x1FFFFFF, c >> 25
        if arrival:
            if c != 0:
                n_cov += 1
                last_base = c >> 25
                n_match += ident != DEL
            if ident in (DEL, DUP):
                ident = 0
            extra = 0
        if ident == 0:
            continue
        if ident == chain:
            c0 += 1
        elif ulo <= ident < uhi:
            entries.append([ident, 1 + extra])
        elif ident in others:
            entries[others[ident]][1] += 1
        else:
            others[ident] = len(entries)
            entries.append([ident, 1 + extra])
    return dict(n=1 + len(entries), c0=c0, overflow=len(others) > TABLE, n_cov=n_cov, n_match=n_match,
                last_base=last_base, entries=entries, n_other=len(others))


def run_cases(exe, tmp_path, cases):
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for cells, arrival, chain, ulo, uhi in cases:
            f.write(struct.pack("<5I", len(cells), int(arrival), chain, ulo, uhi))
            f.write(np.asarray(cells, np.uint32).tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = []
    for ln in out.stdout.decode().splitlines():
        f = ln.split()
        assert int(f[0]) == len(res)
        res.append(dict(n=int(f[1]), c0=int(f[2]), overflow=bool(int(f[3])), n_cov=int(f[4]), n_match=int(f[5]),
                        last_base=int(f[6]), entries=[[int(x) for x in e.split(":")] for e in f[7:]]))
    assert len(res) == len(cases)
    return res


def check(cases, res, names=None):
    seen_overflow = seen_fit = 0
    for k, ((cells, arrival, chain, ulo, uhi), got) in enumerate(zip(cases, res)):
        exp = model(cells, arrival, chain, ulo, uhi)
        tag = f"case {k}" + (f" ({names[k]})" if names else "")
        assert got["overflow"] == exp["overflow"], f"{tag}: overflow mark with {exp['n_other']} other ids"
        if arrival:
            assert (got["n_cov"], got["n_match"], got["last_base"]) == (exp["n_cov"], exp["n_match"], exp["last_base"]), tag
        if exp["overflow"]:
            seen_overflow += 1
            continue
        seen_fit += 1
        assert got["n"] == exp["n"] and got["c0"] == exp["c0"], tag
        if arrival:                       # in-lists carry no count
            assert [e[0] for e in got["entries"]] == [e[0] for e in exp["entries"]], tag
        else:
            assert got["entries"] == exp["entries"], tag
    return seen_fit, seen_overflow


# ids of a row: unique ones ulo + read, the chain next to the range as at a backbone position
ULO, CHAIN_IN = 1000, 900


def cell(ident, top=0):
    return (top << 25) | ident


def random_row(rng, K, arrival, n_other):
    uhi = ULO + K + 1
    chain = CHAIN_IN if arrival else uhi
    pool = [int(x) for x in rng.choice(np.r_[1:CHAIN_IN, uhi + 1:uhi + 500], size=max(n_other, 1), replace=False)]
    cells = []
    for r in range(K):
        u = rng.random()
        top = int(rng.integers(0, 4)) if arrival else (int(rng.integers(1, 128)) if rng.random() < 0.2 else 0)
        if u < 0.10:
            cells.append(0)
        elif u < 0.55:
            cells.append(cell(chain, top))
        elif u < 0.75:
            cells.append(cell(ULO + r, top))
        elif u < 0.90 and n_other:
            cells.append(cell(pool[int(rng.integers(0, n_other))], top))
        elif arrival:
            cells.append(cell(DEL if u < 0.96 else DUP, top))
        else:
            cells.append(cell(chain, top))
    return cells, arrival, chain, ULO, uhi


def test_random_rows(program, tmp_path):
    rng = np.random.default_rng(7101)
    cases = []
    for K in (1, 2, 3, 40, 63, 64):
        for arrival in (False, True):
            for n_other in range(0, 8):
                for _ in range(40):
                    cases.append(random_row(rng, K, arrival, n_other))
    fit, over = check(cases, run_cases(program, tmp_path, cases))
    assert fit > 1000 and over > 100, (fit, over)


def constructed():
    cases, names = [], []

    def add(name, cells, arrival, chain=None, ulo=ULO, uhi=None):
        uhi = ULO + 100 if uhi is None else uhi
        chain = (CHAIN_IN if arrival else uhi) if chain is None else chain
        cases.append((cells, arrival, chain, ulo, uhi))
        names.append(name)

    for arrival in (False, True):
        side = "in" if arrival else "out"
        ch = CHAIN_IN if arrival else ULO + 100
        for K in (0, 1, 2, 3, 40, 63, 64):
            add(f"{side} only chain K={K}", [cell(ch, 1)] * K, arrival)
            add(f"{side} only zeros K={K}", [0] * K, arrival)
            add(f"{side} all unique K={K}", [cell(ULO + r, r % 3) for r in range(K)], arrival)
            # K distinct other ids: enter's departures, exit's arrivals
            add(f"{side} K distinct others K={K}", [cell(5000 + 7 * r) for r in range(K)], arrival)
        # 0 .. 6 distinct other ids, each on several reads, between chain and unique cells; the fifth one arrives at
        # the first, at a middle and at the last cell of the row
        for m in range(0, 7):
            row = []
            for r in range(40):
                row.append(cell(3000 + (r % m), 2 if r < m else 0) if m and r % 3 == 0 else cell(ch) if r % 3 == 1 else cell(ULO + r))
            add(f"{side} {m} others", row, arrival)
        for at in (4, 20, 39):
            row = [cell(ch)] * 40
            for i in range(4):
                row[i] = cell(4000 + i)
            row[at] = cell(4999)
            add(f"{side} fifth other at cell {at}", row, arrival)
            row2 = list(row)
            row2[at] = cell(4003)                      # the fourth again: exactly at the table's edge
            add(f"{side} fourth other again at cell {at}", row2, arrival)
        # other ids below the unique range, above it, and next to its bounds
        add(f"{side} others around the range", [cell(ULO - 1), cell(ULO + 100 + 1), cell(1), cell(ULO - 1), cell(1), cell(ULO)], arrival)
    # extra: on unique cells, on the first read of an other entry (counted), on a later read of it (not counted), on chain cells
    add("out extra on unique", [cell(ULO + 0, 5), cell(ULO + 1, 0), cell(ULO + 2, 127)], False)
    add("out extra on first other", [cell(7000, 9), cell(7000, 0), cell(7000, 3), cell(7001, 0), cell(7001, 4)], False)
    add("out extra 127 on first other of 64", [cell(7000, 127)] * 64, False)
    add("out extra on chain", [cell(ULO + 100, 6), cell(ULO + 100, 0)], False)
    # arrival side: DEL / DUP cells with bases, alone and among entries
    add("in only DEL", [cell(DEL, 2)] * 40, True)
    add("in only DUP", [cell(DUP, 3)] * 40, True)
    add("in DEL, DUP, entries", [cell(DEL, 1), cell(ULO + 1, 2), cell(DUP, 3), cell(CHAIN_IN, 0), cell(8000, 1), cell(DEL, 2), cell(8000, 3)], True)
    # the last covering read at cell 0 and at cell K - 1
    for K in (1, 40, 64):
        add(f"in last cover at cell 0, K={K}", [cell(CHAIN_IN, 3)] + [0] * (K - 1), True)
        add(f"in last cover at cell K-1, K={K}", [cell(CHAIN_IN, 1)] * (K - 1) + [cell(DEL, 2)], True)
        add(f"in only cell K-1 covers, K={K}", [0] * (K - 1) + [cell(ULO + K - 1, 3)], True)
    return cases, names


def test_constructed_rows(program, tmp_path):
    cases, names = constructed()
    res = run_cases(program, tmp_path, cases)
    fit, over = check(cases, res, names)
    assert fit and over
    # the overflow mark exactly past the table's edge
    for name, (cells, arrival, chain, ulo, uhi), got in zip(names, cases, res):
        m = model(cells, arrival, chain, ulo, uhi)["n_other"]
        assert got["overflow"] == (m > TABLE), name
