"""The device against the reference's own AlnGraphBoost.cpp, without the oracle in between.

The expected consensus segments are the reference's (src/cpp/AlnGraphBoost.cpp compiled in place on oracle/bgl_standin), committed
as tests/golden/ref_graph_gpu.json by tests/golden/make_ref_graph.py; where oracle/_ref/libref_graph.so is present they
are computed live as well.  The groups are the inputs on which list order decided the answer when the reference was built
on wrong containers (test_ref_graph.py::test_wrong_standins_are_rejected_by_named_families): merge_cases' widths, fan32,
span and partial, bestpath_cases' suffix, waiters and widths_row, and the first 60 random pileups with at least 3 reads.
One batch per group, one consensus call under the plain options and one under trim 2 / min_weight 1, default plan.

The bound inputs are not run here again: test_bestpath_bound.py holds the device to the oracle on them, and
test_ref_graph.py holds the oracle to the reference.
"""
import functools
import json
import os

import pytest

import oracle
from util import batch_from_targets, golden_module

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
mg = golden_module("make_ref_graph")
GROUPS = tuple(f"{m}/{n}" for m, names in mg.GPU_FAMILIES for n in names) + ("random",)


@functools.lru_cache(maxsize=None)
def gold():
    return json.load(open(os.path.join(GOLD, "ref_graph_gpu.json")))["groups"]


@functools.lru_cache(maxsize=None)
def groups():
    return mg.gpu_groups()


def _expected(group, o):
    return [[(r0, r1, s.encode()) for r0, r1, s in segs] for segs in gold()[group]["%d,%d,%d" % o]]


def test_fixture_covers_the_groups_and_is_what_the_reference_gives(oracle_lib):
    """ref_graph_gpu.json has every group under both option sets, one answer per target; the random group is 60 inputs of at
    least 3 reads; and where the reference is built, the file is what it answers now."""
    assert tuple(groups()) == GROUPS and set(gold()) == set(GROUPS)
    for g, (targets, sets) in groups().items():
        assert sets == (mg.PLAIN, mg.TRIMMED)
        for o in sets:
            assert len(_expected(g, o)) == len(targets)
    rnd = groups()["random"][0]
    assert len(rnd) == mg.GPU_RANDOM and all(len(alns) >= 3 for _, alns, _ in rnd)
    if oracle.ref_graph_lib() is not None:
        assert mg.gpu_expected(oracle.ref_consensus_target) == gold()


@gpu
@pytest.mark.parametrize("group", GROUPS)
def test_device_equals_reference(group, gpu_ctx_factory):
    targets, sets = groups()[group]
    batch = batch_from_targets(targets)
    for ml, trim, mw in sets:
        exp = _expected(group, (ml, trim, mw))
        if oracle.ref_graph_lib() is not None:
            live = [oracle.ref_consensus_target(tl, alns, ml, trim, mw) for tl, alns, _ in targets]
            assert live == exp
        ctx = gpu_ctx_factory(min_cov=0, min_len=ml, trim=trim, min_weight=mw)
        try:
            got = ctx.consensus(batch)
        finally:
            ctx.close()
        bad = [t for t in range(len(exp)) if got[t] != exp[t]]
        assert not bad, f"{group} options {(ml, trim, mw)}: targets {bad[:8]} differ from the reference"
