#!/usr/bin/env python3
"""SHA-256 of the REFERENCE's answers (src/cpp/Alignment.cpp compiled in place into
oracle/_ref/libref_alignment.so) on the seeded fuzz inputs of
test_oracle.py::test_against_live_reference_build (normalizeGaps, trimAln, revcomp) and
test_pre.py::test_parse_pre_against_live_reference_build (parsePre), one digest per block of
100 inputs.  The tests hash the restatement's answers the same way and compare, so they pin it
to the reference on a checkout with no reference to build from; where oracle/_ref exists they
compare with it live as well.

    python tests/golden/make_ref_fuzz.py        # rewrites tests/golden/ref_fuzz_hashes.json
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402

BLOCK = 100
REVCOMP_INPUT = b"ACGTNacgt-ACCGT"
PRE_KEYS = ("id", "sid", "qstr", "tstr", "strand", "tlen", "start", "end")


def a1_inputs():
    """(q, t, trim): normalizeGaps, then trimAln from start 5."""
    rng = np.random.default_rng(99)
    out = []
    for i in range(1500):
        n = int(rng.integers(1, 70))
        al = [b"ACGT-.", b"AC-", b"ACGTN-"][i % 3]
        q = bytes(al[j] for j in rng.integers(0, len(al), n))
        t = bytes(al[j] for j in rng.integers(0, len(al), n))
        out.append((q, t, int(rng.integers(0, 9))))
    return out


def pre_inputs():
    rng = np.random.default_rng(5)
    out = []
    for i in range(200):
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        q = bytes(b"ACGTacgtN-"[j] for j in rng.integers(0, 10, n))
        t = bytes(b"ACGTN"[j] for j in rng.integers(0, 5, m))
        out.append(b" ".join([b"q%d" % i, b"t%d" % (i % 3), b"+-"[i % 2:i % 2 + 1], b"%d" % rng.integers(1, 9999),
                              b"%d" % rng.integers(0, 999), b"%d" % rng.integers(0, 9999), q, t]))
    return out


def a1_answers(normalize_gaps, trim_aln):
    out = []
    for q, t, trim in a1_inputs():
        qn, tn = normalize_gaps(q, t)
        out.append((qn, tn) + tuple(trim_aln(qn, tn, 5, trim)))
    return out


def pre_answers(parse_pre):
    return [tuple(parse_pre(line)[k] for k in PRE_KEYS) for line in pre_inputs()]


def revcomp(fn):
    s = bytearray(REVCOMP_INPUT)
    fn((oracle.C.c_char * len(s)).from_buffer(s), len(s))
    return bytes(s).decode()


def digests(answers):
    return [hashlib.sha256(repr(answers[i:i + BLOCK]).encode()).hexdigest() for i in range(0, len(answers), BLOCK)]


def main():
    oracle.build()
    assert oracle.ref_lib() is not None, "needs the reference (oracle/_ref)"
    doc = dict(source="reference Alignment.cpp via oracle/_ref/libref_alignment.so", block=BLOCK,
               a1=digests(a1_answers(oracle.ref_normalize_gaps, oracle.ref_trim_aln)),
               pre=digests(pre_answers(oracle.ref_parse_pre)),
               revcomp=dict(input=REVCOMP_INPUT.decode(), output=revcomp(oracle.ref_lib().ref_revcomp)))
    json.dump(doc, open(os.path.join(HERE, "ref_fuzz_hashes.json"), "w"), indent=1)
    print(f"wrote ref_fuzz_hashes.json: {len(doc['a1'])} + {len(doc['pre'])} digests")


if __name__ == "__main__":
    main()
