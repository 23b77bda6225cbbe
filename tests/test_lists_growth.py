"""Backbone adjacency lists that outgrow their fixed pool slot (more than
min(K + 2, 12) entries) move to the growth region.  Pileups where one position
has an insertion per read and another a deletion run of a different length per
read give out- and in-lists of up to K + 1 entries, on unique neighbours and on
peeled ones, in the middle of a wave's positions and on its edges."""
import numpy as np
import pytest

from pbdagcon_amd import capi
from test_gpu_parity import _check_graphs
from util import batch_from_targets

pytestmark = pytest.mark.gpu


def _wide_target(rng, tl, k, ins_pos, del_pos):
    bb = bytes(b"ACGT"[i] for i in rng.integers(0, 4, tl))
    alns = []
    for r in range(k):
        q, t = bytearray(), bytearray()
        dl = r % 15                                  # deletion run after del_pos: up to 15 distinct targets
        for i in range(tl):
            if del_pos < i <= del_pos + dl:
                q.append(0x2D); t.append(bb[i])
            else:
                q.append(bb[i]); t.append(bb[i])
            if i == ins_pos:                         # one inserted vertex per read: k distinct neighbours
                for _ in range(1 + r % 3):
                    q.append(b"ACGT"[rng.integers(0, 4)]); t.append(0x2D)
        alns.append((1, bytes(q), bytes(t)))
    return tl, alns, bb


@pytest.mark.parametrize("merge", [False, True])
def test_lists_past_the_fixed_slot_match_oracle(gpu_ctx_factory, merge):
    rng = np.random.default_rng(23)
    targets = [
        _wide_target(rng, 40, 64, 10, 20),           # a full wave of reads
        _wide_target(rng, 40, 30, 14, 30),           # on the last position of a wave
        _wide_target(rng, 33, 40, 0, 15),            # insertion behind the enter's first vertex
        _wide_target(rng, 24, 20, 23, 1),            # insertion in front of the exit
    ]
    batch = batch_from_targets(targets)
    flags = capi.FLAG_STOP_AFTER_MERGE if merge else capi.FLAG_STOP_AFTER_BUILD
    ctx = gpu_ctx_factory(min_cov=0, min_len=0, trim=0, min_weight=0, flags=flags)
    ctx.consensus(batch)
    _check_graphs(ctx, batch, 0, merge)
