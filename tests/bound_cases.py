"""Pileups whose bestPath scores reach 2^22 and 2^23, for tests/test_bestpath_bound.py.

The device sweeps a target in concurrent pieces with relative fp32 scores (k_bestpath.hip.h), which is the reference's
sweep only while every value is an exact multiple of 0.5, below 2^23; dg_bp_exact (m + |above| + wmax < 2^22) guards
that, and a target that fails it is swept whole, in the reference's own operations and order.  A score grows by about
K / 2 per backbone position (count - coverage * 0.5), so the inputs here are long, and a few hundred reads deep: the
oracle's cost grows with depth, the magnitude is reached with length.

Three families, one target each:
  S  full span, rounding-sensitive: every read is the backbone with 1 % single-base deletions; at the sites 200, 261,
     322, ... a rotating set of (K - 1) / 2 of the K reads inserts one base.  The path through the insertion and the
     direct one differ by 1.5 in exact arithmetic; in fp32 they tie once the score behind them is past 2^23, and the
     first in list order wins.  The oracle's answer (fp32, as the reference) then differs from its `wide` answer
     (double: exact arithmetic), which is what a device that stayed in pieces -- small, exact relative values -- gives.
  P  S with every read cut to a random span of at least 0.6 of the target: the partial-span machinery (p.gcuts).
  M  plain: synth.make_batch at a low error rate.
Three bands per family (s = the oracle's largest |score|, K = reads), each asserted on the CPU by the tests:
  below     0.97 * 2^22 < s, s + K < 2^22        the pieces stand, as closely under the bound as an input gets
  between   2^22 + K < s < 2^23 - K              the bound fails, the values are still exact: pieces and whole sweep agree
  above     s > 2^23 + 2^20, fp32 != wide        only the whole sweep gives the reference's answer
L is the smallest multiple of 100 that meets its band for the family's K and seed (SIZES).  P has the two bands in
which its bound fails.  M above has the magnitude and fp32 scores that differ from the exact ones, but the same
consensus either way: the candidates of a plain pileup are hundreds apart, and a rounding to a multiple of 1 decides
nothing there (test_input_lies_in_its_band has the figures).

Strongly negative totals are left out: they are out of reach.  A pileup where every read keeps 30 % of the bases gives
about -0.044 K per position (-795,827 at 60 kb x 301); crossing -2^22 needs about 100 M columns.

The oracle's results are cached here, per process: the CPU preconditions and the GPU tests share them.
"""
import functools
import time

import numpy as np

import oracle
from pbdagcon_amd import synth
from pbdagcon_amd.capi import HostBatch

OPTS = dict(min_cov=6, min_len=500, trim=50)
T22, T23 = float(1 << 22), float(1 << 23)

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NEXT = np.zeros(256, dtype=np.uint8)          # the next letter of ACGT
_NEXT[_ACGT] = np.roll(_ACGT, -1)
_GAP = 0x2D

# (family, band) -> (L, K, seed); the measured figures are in the docstrings of test_bestpath_bound.py
SIZES = {
    ("S", "below"): (17300, 501, 1),
    ("S", "between"): (17900, 501, 1),
    ("S", "above"): (40000, 501, 1),
    ("M", "below"): (23100, 401, 1),
    ("M", "between"): (23800, 401, 1),
    ("M", "above"): (53400, 401, 1),
    ("P", "between"): (17300, 651, 1),
    ("P", "above"): (39100, 651, 1),
}


def _columns_s(L, K, seed):
    """Family S as flat column arrays: (q, t, offs, lens, sites of each read [a list of K arrays])."""
    assert K % 2 == 1 and L > 400
    rng = np.random.default_rng(seed)
    bb = _ACGT[rng.integers(0, 4, L)]
    q = np.broadcast_to(bb, (K, L)).copy()
    dele = rng.integers(0, 100, (K, L), dtype=np.uint8) == 0       # 1 % single-base deletions ...
    dele[:, :60] = False                                           # ... none in the first and last 60 positions
    dele[:, L - 60:] = False
    q[dele] = _GAP
    t = np.broadcast_to(bb, (K, L)).reshape(-1)
    sites = np.arange(200, L - 61, 61)
    a = (K - 1) // 2
    carry = (np.arange(K)[:, None] + np.arange(sites.size)[None, :]) % K < a       # [read, site]: the rotating set
    r_idx, j_idx = np.nonzero(carry)                               # (by read, then by site: ascending flat indices)
    flat = r_idx.astype(np.int64) * L + sites[j_idx] + 1           # behind the site
    qf = np.insert(q.reshape(-1), flat, _NEXT[bb[sites[j_idx] + 1]])   # never the following backbone base
    tf = np.insert(t, flat, _GAP)
    lens = L + carry.sum(axis=1)
    offs = np.zeros(K, dtype=np.int64)
    offs[1:] = np.cumsum(lens)[:-1]
    return qf, tf, offs, lens, [sites[carry[r]] for r in range(K)]


def _one_target(L, starts, offs, lens, q, t, name):
    K = len(lens)
    return HostBatch(np.array([L], np.uint32), np.array([0, K], np.uint64), np.asarray(starts, np.uint32),
                     np.asarray(offs, np.uint64), np.asarray(lens, np.uint32), q, t, None, None, [f"{name}/0_{L}"])


def family_s(L, K, seed=1):
    q, t, offs, lens, _ = _columns_s(L, K, seed)
    return _one_target(L, np.ones(K, np.uint32), offs, lens, q, t, f"S{K}x{L}")


def family_p(L, K, seed=1):
    """S with read r cut to the target bases [s0, s0 + span), span at least 0.6 L; an inserted base stays with the
    target base in front of it."""
    q, t, offs, lens, sites = _columns_s(L, K, seed)
    rng = np.random.default_rng(seed + 7919)
    span = rng.integers((6 * L + 9) // 10, L + 1, K)
    s0 = (rng.random(K) * (L - span + 1)).astype(np.int64)
    qs, ts = [], []
    for r in range(K):                                             # (a loop over reads, not over columns)
        c0 = int(s0[r]) + int(np.searchsorted(sites[r], s0[r]))    # an insertion behind site p sits at column p + 1 + (sites before p)
        c1 = int(s0[r] + span[r]) + int(np.searchsorted(sites[r], s0[r] + span[r]))
        qs.append(q[offs[r] + c0:offs[r] + c1])
        ts.append(t[offs[r] + c0:offs[r] + c1])
    nl = np.array([x.size for x in qs], dtype=np.int64)
    no = np.zeros(K, dtype=np.int64)
    no[1:] = np.cumsum(nl)[:-1]
    return _one_target(L, s0 + 1, no, nl, np.concatenate(qs), np.concatenate(ts), f"P{K}x{L}")


def family_m(L, K, seed=1):
    return synth.make_batch(1, L, K, seed=seed, ins=0.02, dele=0.01)


FAMILIES = {"S": family_s, "P": family_p, "M": family_m}


def oracle_target(batch, t=0, wide=False):
    """(segments, stats) of target t of a batch under OPTS, from the oracle's fp32 recurrence (the reference's) or, with
    wide, the same in double."""
    a0, a1 = int(batch.aln_begin[t]), int(batch.aln_begin[t + 1])
    return oracle.consensus_target_blob(
        int(batch.tlen[t]), batch.aln_start[a0:a1].copy(), batch.aln_off[a0:a1].copy(), batch.aln_len[a0:a1].copy(),
        batch.qstr, batch.tstr, OPTS["min_len"], OPTS["trim"], OPTS["min_cov"], None, wide=wide, stats=True)


class Case:
    """One input: its batch, the oracle's answer and scores, and for the `above` band the wide answer too."""

    def __init__(self, family, band):
        self.family, self.band = family, band
        self.L, self.K, seed = SIZES[(family, band)]
        self.batch = FAMILIES[family](self.L, self.K, seed)
        self.columns = int(self.batch.qstr.size)
        t0 = time.perf_counter()
        self.exp, self.stats = oracle_target(self.batch)
        self.oracle_seconds = time.perf_counter() - t0
        self.s = max(abs(self.stats["min"]), abs(self.stats["max"]))
        self.wide = self.wide_stats = None
        if band == "above":
            self.wide, self.wide_stats = oracle_target(self.batch, wide=True)

    def __repr__(self):
        return (f"{self.family} {self.band}: L={self.L} K={self.K} columns={self.columns} s={self.s} "
                f"enter={self.stats['enter']} min={self.stats['min']} oracle {self.oracle_seconds:.2f} s")


@functools.lru_cache(maxsize=None)
def case(family, band):
    return Case(family, band)
