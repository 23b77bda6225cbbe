"""The C-ABI library loads (without a GPU) and exports every symbol that
include/dagcon.h declares; no compute call is made here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "dagcon.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(dagcon_[a-z_0-9]+)\s*\(", src)
    return sorted(set(names))


def test_header_and_binding_agree():
    from pbdagcon_amd import capi
    assert sorted(capi.EXPORTS) == declared_functions()


def test_library_exports_every_declared_symbol():
    from pbdagcon_amd import capi
    lib = capi.load()
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} is declared in include/dagcon.h but not exported"
    assert lib.dagcon_abi_version() == 2


def test_struct_layouts_match_header():
    """sizes the C compiler gives the ABI structs == the ctypes mirrors."""
    import subprocess
    import tempfile
    from pbdagcon_amd import capi
    prog = r'''
#include <stdio.h>
#include "dagcon.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dagcon_opts), sizeof(dagcon_batch),
 sizeof(dagcon_results), sizeof(dagcon_timings), sizeof(dagcon_graph_dump), sizeof(dagcon_pre_batch)); return 0;}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"),
                               os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    got = [ctypes.sizeof(x) for x in (capi.Opts, capi.Batch, capi.Results, capi.Timings, capi.GraphDump, capi.PreBatch)]
    assert got == [int(x) for x in out]


def test_default_opts_are_pbdagcon_defaults():
    """main.cpp:181-211: -c 6 -m 500 -t 50; min_weight follows min_cov (quirk Q1)."""
    from pbdagcon_amd import capi
    o = capi.default_opts()
    assert (o.min_cov, o.min_len, o.trim, o.min_weight) == (6, 500, 50, -1)


def test_no_device_fails_loudly():
    """Without a GPU the product refuses to run: there is no CPU fallback."""
    from pbdagcon_amd import capi
    from util import gpu_present
    if gpu_present():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.DagconError) as e:
        capi.Context()
    assert e.value.code == -2


def test_product_does_not_import_oracle():
    """The product package never references oracle/ (checker only)."""
    pkg = os.path.join(ROOT, "pbdagcon_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".c", ".cpp")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "import oracle" not in txt and "from oracle" not in txt, fn
                assert "dagcon_oracle" not in txt and "liboracle" not in txt, fn


def test_piece_plan_never_gives_an_empty_grid():
    """dagcon_upload's piece arithmetic (dagcon_debug_plan: host only).  A batch of very many short targets used to
    come out with 0 merge pieces per target (T > 24576 with fewer than 256 positions each: grids of 0 blocks for
    k_merge_q / k_bp_sweep / k_bp_walk); every shape must give 1 <= pieces <= 256, bestPath pieces >= 1, and the
    four-segments-per-wave kernel only with at least two pieces per target."""
    from pbdagcon_amd import capi
    lib = capi.load()
    lib.dagcon_debug_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32 * 4]
    out = (ctypes.c_uint32 * 4)()
    Ts = sorted(set(list(range(1, 70)) + [96, 255, 256, 257, 1000, 4000, 8191, 8192, 8193, 24575, 24576, 24577,
                                          30000, 50000, 65536, 100000]))
    for T in Ts:
        for per in (4, 40, 132, 256, 600, 1004, 10004, 50004):        # positions per target (tlen + 2, rounded)
            for cov in (1, 8, 40, 72, 73, 300):
                for partial in (0, 1):
                    for ms in (0, 1, 3, 64, 500):
                        assert lib.dagcon_debug_plan(T, T * cov, T * per, partial, ms, 0, out) == 0
                        seg_max, seg_min, use_q, bp_max = list(out)
                        assert 1 <= seg_max <= 256 and 1 <= bp_max <= 256 and seg_min >= 1, (T, per, cov, partial, ms, list(out))
                        assert (T * seg_max + 3) // 4 > 0 and T * bp_max > 0
                        if use_q and not ms:
                            assert seg_max >= 2 and not partial, (T, per, cov, list(out))
    # the shape the advice named: 24577 targets below 256 positions each -> not the row kernel with 0 pieces
    lib.dagcon_debug_plan(24577, 24577 * 8, 24577 * 132, 0, 0, 0, out)
    assert out[0] >= 1 and out[3] >= 1
    # the caller's piece length is taken as given, partial spans or not (a floor of 256 stood here for two hours at the end
    # of round 3, until the race it fenced off was understood: k_cuts2's condition (5))
    for partial in (0, 1):
        lib.dagcon_debug_plan(30, 510, 30 * 5000, partial, 64, 4, out)
        assert out[1] == 4, list(out)
    # configs[1]: 1,000 x 10 kb x 40x keeps the choice the round-2 measurements were made with
    lib.dagcon_debug_plan(1000, 40000, 1000 * 10004, 0, 0, 0, out)
    assert list(out) == [49, 128, 1, 64]
