"""The lane functions of k_norm_finish2 (csrc/k_norm_fin.hip.h) on the CPU, against the literal column loop of
dg_finish_alignment.

tests/native/norm_fin_host.cpp includes the header, is built here with the host compiler, AddressSanitizer and UBSan,
and runs as a program of its own.  It makes its cases itself and prints one line of counts a set; a set that found a
difference prints the first few to stderr and the program ends with status 1.  Every comparison is exact and no case is
left out: what the lanes write (matC cells, checkpoints), the flags they raise (a run too long for a byte cell, a
non-conforming read) and the counts they hand on (insertions, deletions, target bases, the run that leaves the chunk)
against the same from the reference loop with the rules at a chunk's edges.

  pieces   all 4^8 class patterns (match, deletion, insertion, neither) of an 8-column piece, run_in in {0, 1, 3, 254,
           255}; each with 54 scenes on the whole piece (start + adv_lane across a checkpoint multiple for emit_shift 4, 7
           and 9, adv_lane across the conformity limit and tlen + 1, start 0, the chunk's first column with o > lo and
           o <= lo, emit_shift 0 and 2) and with every window edge f0 <= f1 in 0..8, the scenes in turn; the piece is the
           lane's lower or upper one
  combine  dg_seg_combine: identity and associativity on 16 values; the 64-lane network of row shifts and row broadcasts
           against the run length counted column by column, 20,000 random waves
  chunks   20,000 random chunks of 1 to 2,300 columns through an emulation of the wave (the lanes in order, the same
           functions, the same network)
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "norm_fin_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("norm_fin_host") / "norm_fin_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def run_set(exe, name):
    out = subprocess.run([exe, name], capture_output=True, timeout=600)
    assert out.returncode == 0, (out.stdout.decode() + out.stderr.decode(errors="replace"))[-4000:]
    f = out.stdout.decode().split()
    assert f[0] == name
    return {k: int(v, 0) for k, v in zip(f[1::2], f[2::2])}


def test_pieces_exhaustive(program):
    r = run_set(program, "pieces")
    assert r["mismatches"] == 0
    # 4^8 patterns x 5 run_in x (the scenes + the 45 windows)
    assert r["scenes"] >= 3 * 10 + 11 + 3 and r["cases"] == 65536 * 5 * (r["scenes"] + 45)


def test_seg_combine(program):
    r = run_set(program, "combine")
    assert r["mismatches"] == 0 and r["cases"] == 16 ** 3 and r["waves"] == 20000


def test_whole_chunks(program):
    r = run_set(program, "chunks")
    assert r["mismatches"] == 0 and r["cases"] == 20000
    # the cases do hold what they were made for
    for key in ("multi_pass", "wide", "nonconf", "empty", "o_gt_lo", "trailing", "raw", "edge_piece", "edge_pass", "edge_chunk",
                "trim_first", "trim_last"):
        assert r[key] >= 100, (key, r)
    assert r["o_mod8"] == 0xFF and r["cells"] > 100000 and r["ckpts"] > 100000
