"""dagcon_set_edits / dagcon_fetch_edits (include/dagcon.h, csrc/k_edits.hip.h) and pbdagcon --edits: where the consensus
differs from its target.  One invariant holds everything: the edits applied to the target give the consensus back byte
for byte.  CPU: the twin (tests/edits_twin.py) against that invariant, the binding, the usage errors.  GPU: the device's
arrays equal the twin's field for field, and satisfy the invariant on their own."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import edits_twin as et
import paf_files as pf
import window_twin as wt
from util import random_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBDAGCON = os.path.join(ROOT, "pbdagcon_amd", "bin", "pbdagcon")
MIN_COV, MIN_LEN = 3, 30
NONCONFORMING = -4


def _cli():
    if not os.path.exists(PBDAGCON):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return PBDAGCON


# ---- CPU: the twin ---------------------------------------------------------------------------------------------------

def _check_twin_target(tseq, alns, min_cov, min_len, trim):
    """The invariant and the trim's postcondition on every segment of one target; the number of edits seen."""
    (segs,) = et.batch_edits([(tseq, alns)], min_cov, min_len, trim)
    n = 0
    for seq, t0, t1, edits in segs or []:
        assert et.apply_edits(tseq, t0, t1, edits, seq) == seq
        for t_pos, t_len, c, c_len in edits:
            assert t_len or c_len
            if t_len and c_len:
                assert tseq[t_pos] != seq[c] and tseq[t_pos + t_len - 1] != seq[c + c_len - 1]
        assert all(a[0] + a[1] <= b[0] for a, b in zip(edits, edits[1:]))
        n += len(edits)
    return n


def test_twin_invariant_on_random_small_pileups(oracle_lib):
    """2,000 random small pileups (partial spans, leading insertion runs, two-letter alphabets): the twin's edits applied
    to the target give every segment back, and no edit is left with equal first or last bytes on both sides."""
    rng = np.random.default_rng(20)
    edits = segs = 0
    for k in range(2000):
        tlen = int(rng.integers(8, 70))
        alns, bb = random_target(rng, tlen, int(rng.integers(3, 8)), alphabet=b"AC" if k % 3 == 0 else b"ACGT",
                                 sub=0.06, ins=0.12, dele=0.08, full_span=bool(k % 2))
        if k % 5 == 0:                                          # a soft-masked stretch: case counts in the trim
            a = int(rng.integers(0, tlen)); b = min(tlen, a + 6)
            low = bb[:a] + bb[a:b].lower() + bb[b:]
            alns = [(s, q, _retarget(s, t, low)) for s, q, t in alns]
            bb = low
        n = _check_twin_target(bb, alns, 3, 4, int(rng.integers(0, 3)))
        edits += n; segs += n > 0
    assert edits > 1000 and segs > 500                           # (the case is not vacuous)


def _retarget(start, tstr, tseq):
    """tstr with the bytes of tseq at the positions it consumes."""
    out, x = bytearray(tstr), start - 1
    for i, ch in enumerate(out):
        if ch != ct.GAP:
            out[i] = tseq[x]; x += 1
    return bytes(out)


def test_twin_trim_and_apply_by_hand():
    #          0123456789
    target = b"ACGTACGTAC"
    # bases 0-1 kept, an inserted G, target 2 skipped (a G: the trim drops the edit), target 3 kept, TT inserted, 4-5 skipped
    seq = b"ACGTTTGTAC"
    pos = [1, 2, 3, 4, 7, 7, 7, 8, 9, 10]
    kind = [1, 1, 0, 1, 0, 0, 1, 1, 1, 1]
    t0, t1, edits = et.segment_edits(target, pos, kind, seq, c_base=100)
    assert (t0, t1) == (0, 10) and edits == [(4, 2, 104, 2)]
    assert et.apply_edits(target, t0, t1, [(4, 2, 4, 2)], seq) == seq
    # no backbone base: one insertion at t0 = t1
    assert et.segment_edits(target, [5, 5], [0, 0], b"GG") == (4, 4, [(4, 0, 0, 2)])
    # a leading and a trailing run, and a deletion whose c_off is the base it stands in front of
    assert et.segment_edits(target, [3, 3, 6, 11], [0, 1, 1, 0], b"TGCA") == (2, 6, [(2, 0, 0, 1), (3, 2, 2, 0), (6, 0, 3, 1)])
    with pytest.raises(AssertionError):
        et.apply_edits(target, 0, 10, [(4, 2, 0, 1), (5, 1, 0, 1)], seq)


def test_binding_exports_and_struct_size():
    from pbdagcon_amd import capi
    assert "dagcon_set_edits" in capi.EXPORTS and "dagcon_fetch_edits" in capi.EXPORTS
    lib = capi.load()
    assert hasattr(lib, "dagcon_set_edits") and hasattr(lib, "dagcon_fetch_edits")
    prog = '#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu\\n", sizeof(dagcon_edits)); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = subprocess.check_output([os.path.join(d, "s")]).split()
    assert ctypes.sizeof(capi.Edits) == int(out[0])
    assert callable(capi.Context.set_edits) and callable(capi.Context.edits)


def test_edits_usage_errors(tmp_path):
    """--edits goes with the record inputs only: .m5, .pre (-a), --dump-parsed and a missing file name are usage errors
    (exit 2), said without a device; --help lists the option."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    ed = tmp_path / "e.tsv"

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    for args in (["--edits", str(ed), str(m5)], ["-a", "--edits", str(ed), str(m5)], [str(m5), "--edits"]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
    # --dump-parsed runs nothing: the file would not be written, so the pair is refused, not ignored
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))
    out = run("--sam", "--ref", str(ref), "--dump-parsed", "--edits", str(ed), str(sam))
    assert out.returncode == 2 and b"PARSE ERROR" in out.stderr
    assert not ed.exists()
    h = run("--help")
    assert h.returncode == 0 and b"--edits FILE" in h.stdout


# ---- CPU: the stitch's edit rule (csrc/host/windows.h) ------------------------------------------------------------------

def _random_windows(rng, tlen, W, O, agree):
    """A target and, per window of its tiling, one or two segments with random best paths: kept, dropped and inserted
    bases, inserted bases behind dropped ones, a two-letter alphabet so that the trim moves edits.  agree: every window
    reads its path off one path of the whole target; otherwise every window has a path of its own, so that neighbours
    disagree at their joints as nothing on a device would.  (target, windows for edits_twin.stitch_edits)."""
    target = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), size=tlen).tolist())

    def path(lo, hi):                                           # [(kind, 0-based target position, byte)]
        out = []
        for x in range(lo, hi):
            for _ in range(int(rng.integers(1, 4)) if rng.random() < 0.12 else 0):
                out.append((0, x, int(rng.choice(np.frombuffer(b"AC", np.uint8)))))
            if rng.random() < 0.85:
                out.append((1, x, target[x]))
        return out
    whole = path(0, tlen)
    wins = []
    for begin, end, c0, c1 in wt.tiled(tlen, W, O):
        pth = [v for v in whole if begin <= v[1] < end] if agree else path(begin, end)
        cuts = sorted(rng.integers(0, len(pth) + 1, 2).tolist()) if rng.random() < 0.3 else None
        segs = []
        for part in ([pth] if cuts is None else [pth[:cuts[0]], pth[cuts[1]:]]):
            if not part:
                continue
            kind = [k for k, _, _ in part]
            pos = [x - begin + 1 for _, x, _ in part]
            seq = bytes(b for _, _, b in part)
            t0, _, edits = et.segment_edits(target[begin:end], pos, kind, seq)
            segs.append((seq, pos, t0, edits))
        wins.append((begin, c0, c1, segs))
    return target, wins


def _check_pieces(target, pieces, wins, min_len):
    """The binding condition, the order of the pieces, and the stitch's own records beside them; the number of edits."""
    plain = wt.stitch([(b, c0, c1, [(seq, pos, None) for seq, pos, _, _ in segs]) for b, c0, c1, segs in wins], min_len)
    assert [(t0, t1, seq) for t0, t1, seq, _, _, _ in pieces] == [(t0, t1, seq) for t0, t1, seq, _ in plain]
    end = 0
    for t0, t1, seq, e0, e1, edits in pieces:
        assert end <= e0 <= e1 <= len(target)
        assert et.apply_edits(target, e0, e1, edits, seq) == seq
        assert all(tl or cl for _, tl, _, cl in edits)
        assert all(a[0] + a[1] <= b[0] and a[2] + a[3] <= b[2] and (a[0] + a[1] < b[0] or a[2] + a[3] < b[2])
                   for a, b in zip(edits, edits[1:]))
        end = e1
    return sum(len(p[5]) for p in pieces)


def _window_cases():
    rng = np.random.default_rng(404)
    for k in range(300):
        W = int(rng.integers(8, 40)); O = int(rng.integers(0, W + 10))
        yield (k,) + _random_windows(rng, int(rng.integers(20, 200)), W, O, agree=bool(k % 2)) + (int(rng.integers(1, 12)),)


def test_twin_stitch_edits_rebuild_every_piece():
    """300 random tilings, half with windows that agree and half with windows that do not: every piece is the stitch's own
    record, its edits applied to its span of the target give it back, and the pieces of a target do not overlap."""
    n = 0
    for _, target, wins, min_len in _window_cases():
        n += _check_pieces(target, et.stitch_edits(wins, min_len), wins, min_len)
    assert n > 2000


def test_twin_stitch_of_agreeing_windows_is_the_whole_target_s_list():
    """Windows that read their paths off one path of the whole target, which starts and ends with a kept base: the stitch
    is one piece, and its span and edits are those of the whole path -- no cut leaves a trace."""
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for _ in range(200):
        tlen = int(rng.integers(60, 200)); W = int(rng.integers(10, 40)); O = int(rng.integers(5, W))
        target = bytes(rng.choice(acgt, size=tlen).tolist())
        whole = []
        for x in range(tlen):
            for _ in range(int(rng.integers(1, 4)) if rng.random() < 0.1 else 0):
                whole.append((0, x, int(rng.choice(acgt))))
            if rng.random() < 0.9 or x in (0, tlen - 1):
                whole.append((1, x, target[x]))
        wins = []
        for b, e, c0, c1 in wt.tiled(tlen, W, O):
            part = [v for v in whole if b <= v[1] < e]
            seq, pos = bytes(v[2] for v in part), [v[1] - b + 1 for v in part]
            t0, _, ed = et.segment_edits(target[b:e], pos, [v[0] for v in part], seq)
            wins.append((b, c0, c1, [(seq, pos, t0, ed)]))
        seq = bytes(v[2] for v in whole)
        t0, t1, ed = et.segment_edits(target, [v[1] + 1 for v in whole], [v[0] for v in whole], seq)
        assert et.stitch_edits(wins, 1) == [(t0, t1, seq, t0, t1, ed)]


def test_twin_stitch_edits_by_hand():
    #          0123456789012345
    target = b"ACGTACGTACGTACGT"
    # window 0 = [0, 12), core [0, 8): bases 0-5 kept, TT inserted, 6 kept, 7-8 dropped, 9-11 kept
    seq0, pos0, kind0 = b"ACGTACTTGCGT", [1, 2, 3, 4, 5, 6, 7, 7, 7, 10, 11, 12], [1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1]
    # window 1 = [4, 16), core [8, 16): the same path from base 4 on
    seq1, pos1, kind1 = seq0[4:] + b"ACGT", [p - 4 for p in pos0[4:]] + [9, 10, 11, 12], kind0[4:] + [1, 1, 1, 1]
    segs = []
    for tw, (seq, pos, kind) in ((target[0:12], (seq0, pos0, kind0)), (target[4:16], (seq1, pos1, kind1))):
        t0, _, ed = et.segment_edits(tw, pos, kind, seq)
        segs.append((seq, pos, t0, ed))
    wins = [(0, 0, 8, [segs[0]]), (4, 8, 16, [segs[1]])]
    # the cut lies between base 6 (g 7) and the deletion of 7-8, which goes with base 9 behind it into the second part
    assert et.stitch_edits(wins, 1) == [(0, 16, b"ACGTACTTGCGTACGT", 0, 16, [(6, 0, 6, 2), (7, 2, 9, 0)])]
    # alone, the second part starts at its first kept base: the deletion in front of it is not its own
    assert et.stitch_edits([(4, 8, 16, [segs[1]])], 1) == [(9, 16, b"CGTACGT", 9, 16, [])]
    # a run split by the cut: window 0 ends inside it (its second T has the g of base 9), window 1 begins inside it
    pos0b = [1, 2, 3, 4, 5, 6, 7, 9, 7, 10, 11, 12]
    t0, _, ed0 = et.segment_edits(target[0:12], pos0b, kind0, seq0)
    t1_, _, ed1 = et.segment_edits(target[4:16], [p - 4 for p in pos0b[4:]] + [9, 10, 11, 12], kind1, seq1)
    wins = [(0, 0, 8, [(seq0, pos0b, t0, ed0)]), (4, 8, 16, [(seq1, [p - 4 for p in pos0b[4:]] + [9, 10, 11, 12], t1_, ed1)])]
    (piece,) = et.stitch_edits(wins, 1)
    assert piece[2] == b"ACGTACT" + b"TGCGTACGT" and et.apply_edits(target, piece[3], piece[4], piece[5], piece[2]) == piece[2]


_STITCH_MAIN = r"""
#include <iostream>
#include "windows.h"
// stdin: per segment "wi begin c0 c1 n t0 ne", the bases, n positions, ne edits; stdout: the pieces with their edits
int main() {
    DgStitch st;
    long long wi; uint32_t begin, c0, c1, n, t0; uint64_t ne; unsigned min_len;
    std::cin >> min_len;
    while (std::cin >> wi >> begin >> c0 >> c1 >> n >> t0 >> ne) {
        if (wi < 0) {
            for (const DgStitchPiece &p : st.pieces) {
                if (p.seq.size() < min_len) continue;
                std::cout << "P " << p.t0 << ' ' << p.t1 << ' ' << p.seq << ' ' << p.e0 << ' ' << p.e1 << '\n';
                for (const DgPieceEdit &e : p.edits) std::cout << "E " << e.t_pos << ' ' << e.t_len << ' ' << e.c_off << ' ' << e.c_len << '\n';
            }
            std::cout << "T\n";
            st.reset();
            continue;
        }
        std::string seq; std::cin >> seq;
        std::vector<uint32_t> pos(n), tp(ne), tl(ne), cl(ne); std::vector<uint64_t> co(ne);
        for (auto &x : pos) std::cin >> x;
        for (uint64_t k = 0; k < ne; k++) { std::cin >> tp[k] >> tl[k] >> co[k] >> cl[k]; co[k] += 1000; }
        DgSegEdits se{t0, ne, tp.data(), tl.data(), co.data(), cl.data(), 1000};
        st.add(wi, begin, c0, c1, seq.data(), pos.data(), n, nullptr, nullptr, &se);
    }
    return 0;
}
"""


def test_host_stitch_equals_the_twin(tmp_path):
    """DgStitch itself (csrc/host/windows.h, compiled into a small program) on the 300 tilings: the twin's pieces, spans
    and edits, field for field."""
    src = tmp_path / "stitch_main.cpp"; src.write_text(_STITCH_MAIN)
    exe = tmp_path / "stitch_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"),
                           "-o", str(exe), str(src)])
    cases = list(_window_cases())
    lines = []
    want = []
    for _, target, wins, _ in cases:
        for wi, (begin, c0, c1, segs) in enumerate(wins):
            for seq, pos, t0, edits in segs:
                lines.append("%d %d %d %d %d %d %d %s %s %s" % (wi, begin, c0, c1, len(seq), t0, len(edits), seq.decode(),
                             " ".join(map(str, pos)), " ".join("%d %d %d %d" % e for e in edits)))
        lines.append("-1 0 0 0 0 0 0")
        want.append(et.stitch_edits(wins, 3))
    out = subprocess.run([str(exe)], input=("3\n" + "\n".join(lines) + "\n").encode(), capture_output=True, timeout=120, check=True)
    got, cur = [], []
    for ln in out.stdout.decode().splitlines():
        f = ln.split(" ")
        if f[0] == "T":
            got.append(cur); cur = []
        elif f[0] == "P":
            cur.append((int(f[1]), int(f[2]), f[3].encode(), int(f[4]), int(f[5]), []))
        else:
            cur[-1][5].append(tuple(int(x) for x in f[1:]))
    assert len(got) == len(want) == 300
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, k


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _records(bb, alns, eqx=False):
    return [ct.compress(s, q, t, bb, eqx=eqx and bool(k % 2)) for k, (s, q, t) in enumerate(alns)]


def _strings(targets):
    """[(target bytes, [(start, q, t)])] of record targets; a target with a non-conforming record: None."""
    out = []
    for bb, recs in targets:
        if any(not ct.conforming(p, len(q), len(bb), o) for p, q, o in recs):
            out.append(None)
        else:
            out.append((bb, [ct.expand(p, q, bb, o) for p, q, o in recs]))
    return out


def _twin(strings, min_cov, min_len, trim):
    return [[] if s is None else x for s, x in
            zip(strings, et.batch_edits([s if s is not None else (b"", []) for s in strings], min_cov, min_len, trim))]


def _device(ctx, got):
    """The device's edits in the twin's form, and the invariant straight from its arrays."""
    ed = ctx.edits()
    sb, so, sl = ctx._segs
    assert ed["seg_t0"].size == so.size == ed["edit_begin"].size - 1 and int(ed["edit_begin"][-1]) == ed["t_pos"].size
    out = []
    for t, segs in enumerate(got):
        per = []
        for k, (_, _, seq) in enumerate(segs):
            s = int(sb[t]) + k
            b, e = int(ed["edit_begin"][s]), int(ed["edit_begin"][s + 1])
            per.append((seq, int(ed["seg_t0"][s]), int(ed["seg_t1"][s]),
                        [(int(ed["t_pos"][i]), int(ed["t_len"][i]), int(ed["c_off"][i]) - int(so[s]), int(ed["c_len"][i]))
                         for i in range(b, e)]))
        out.append(per)
    return out


def _assert_invariant(dev, tseqs):
    n = 0
    for per, tseq in zip(dev, tseqs):
        for seq, t0, t1, edits in per:
            assert 0 <= t0 <= t1 <= len(tseq)
            assert all(0 <= c <= len(seq) - (1 if not c_len else c_len) for _, _, c, c_len in edits)
            assert et.apply_edits(tseq, t0, t1, edits, seq) == seq
            n += len(edits)
    return n


def _run_whole(targets, trim, min_len=MIN_LEN):
    """consensus_cigar with edits on: device == twin, invariant from the device's arrays; the device's edits."""
    from pbdagcon_amd import capi
    strings = _strings(targets)
    exp = _twin(strings, MIN_COV, min_len, trim)
    ctx = capi.Context(min_cov=MIN_COV, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
    try:
        ctx.set_edits(True)
        got = ctx.consensus_cigar(capi.HostCigarBatch(**ct.records_to_arrays(targets)), strict=False)
        dev = _device(ctx, got)
        status = ctx.target_status.tolist()
        reruns = ctx.timings()["reruns"]
    finally:
        ctx.close()
    assert dev == exp
    _assert_invariant(dev, [bb for bb, _ in targets])
    return dev, status, reruns


def _designed():
    """Ten identical full-span records per target that agree on designed edits.  Target A (420 bases): a leading run of 3
    inserted bases, a substitution, a 1-base insertion and deletion, a run of 5 that starts exactly at base 64 of the
    segment, a 70-base deletion and a 70-base insertion (each crosses a 64-base step of the scan), a trailing run of 4.
    Target B (200 bases): substitutions in the first and the last 3 bases of its segment.  Returns the record targets
    and per target the expected edits as (t_pos, t_len, replacing bytes)."""
    rng = np.random.default_rng(5)

    def other(*avoid):
        return next(b for b in b"ACGT" if b not in avoid)

    def build(tlen, plan):
        # no base equals its neighbour: nothing normalizeGaps or the trim could slide an edit along
        bb = bytearray()
        while len(bb) < tlen:
            b = int(rng.choice(np.frombuffer(b"ACGT", np.uint8)))
            if not bb or bb[-1] != b:
                bb.append(b)
        # a deleted stretch does not hold the base behind it (normalizeGaps would move that base into the gap, piece by
        # piece), and its last base differs from the base in front of it (the deletion cannot be slid left either)
        for kind, p, n in plan:
            if kind == "del":
                for i in range(p, p + n):
                    bb[i] = other(bb[i - 1], bb[p + n], bb[p - 1] if i == p + n - 1 else 0)
        q, t, exp = bytearray(), bytearray(), []
        x = 0
        for kind, p, n in plan:                                # sorted by p; ins: in front of target base p
            while x < p:
                q.append(bb[x]); t.append(bb[x]); x += 1
            if kind == "ins":
                prev = q[-1] if q else 0
                run = bytearray()
                for i in range(n):
                    run.append(other(run[-1] if run else prev, bb[p] if p < tlen else 0, bb[p - 1] if p else 0))
                q += run; t += b"-" * n
                exp.append((p, 0, bytes(run)))
            elif kind == "del":
                assert bb[p] != bb[p + n] and bb[p + n - 1] != bb[p - 1]
                q += b"-" * n; t += bb[p:p + n]; x = p + n
                exp.append((p, n, b""))
            else:
                sub = other(bb[p], bb[p - 1], bb[p + 1])
                q.append(sub); t.append(bb[p]); x = p + 1
                exp.append((p, 1, bytes([sub])))
        while x < tlen:
            q.append(bb[x]); t.append(bb[x]); x += 1
        recs = [ct.compress(1, bytes(q), bytes(t), bytes(bb), eqx=bool(k % 2)) for k in range(10)]
        return (bytes(bb), recs), exp
    # A: consensus index of target base p: 3 + p up to 50, 4 + p behind the insertion at 51, 3 + p behind the deletion
    # of 55: target base 61 would be base 64 -- the run of 5 in front of it starts there
    a = build(420, [("ins", 0, 3), ("sub", 30, 1), ("ins", 51, 1), ("del", 55, 1), ("ins", 61, 5), ("del", 100, 70),
                    ("ins", 250, 70), ("ins", 420, 4)])
    b = build(200, [("sub", 1, 1), ("sub", 198, 1)])
    return [a[0], b[0]], [a[1], b[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 5])
def test_designed_edits(oracle_lib, trim):
    targets, want = _designed()
    strings = _strings(targets)
    exp = _twin(strings, MIN_COV, MIN_LEN, 0)
    # on the CPU first (oracle + twin, trim 0): one segment per target, every designed edit is in its list and nothing else
    for per, w, (bb, _) in zip(exp, want, targets):
        assert len(per) == 1
        seq, t0, t1, edits = per[0]
        assert (t0, t1) == (0, len(bb))
        assert [(p, n, seq[c:c + cl]) for p, n, c, cl in edits] == w
    seq_a, _, _, ed_a = exp[0][0]
    assert (61, 0, 64, 5) in ed_a and ed_a[0] == (0, 0, 0, 3) and ed_a[-1] == (420, 0, len(seq_a) - 4, 4)
    assert any(n == 70 for _, n, _, _ in ed_a) and any(cl == 70 for _, _, _, cl in ed_a)
    dev, status, _ = _run_whole(targets, trim)
    assert status == [0, 0] and [len(p) for p in dev] == [1, 1]
    if trim == 0:
        assert dev == exp


def _structure_case():
    """Target 0: three stretches of coverage held together by one long read -- [0, 200), the single base 250 and
    [300, 600) -- so three segments, one of one base (min_len 1 lets it out; the issue's min_len 30 cannot).  Target 1:
    below min_cov.  Target 2: a record that runs past its target.  Target 3: a sound pileup behind the failed one."""
    rng = np.random.default_rng(11)
    _, bb = random_target(rng, 600, 1, full_span=True)
    recs = [ct.compress(1, bb, bb, bb)]
    for k in range(5):
        recs.append(ct.compress(1, bb[:200], bb[:200], bb))
        recs.append(ct.compress(251, bb[250:251], bb[250:251], bb))
        q = bytearray(bb[300:600]); q[40] = ord("A") if q[40] != ord("A") else ord("C")
        recs.append(ct.compress(301, bytes(q), bb[300:600], bb))
    alns1, bb1 = random_target(rng, 150, 2, full_span=True)
    alns2, bb2 = random_target(rng, 160, 6, full_span=True)
    recs2 = _records(bb2, alns2)
    p, q, o = recs2[3]
    recs2[3] = (len(bb2) - 10, q, o)
    alns3, bb3 = random_target(rng, 333, 9)
    return [(bb, recs), (bb1, _records(bb1, alns1)), (bb2, recs2), (bb3, _records(bb3, alns3, eqx=True))]


@pytest.mark.gpu
def test_segments_failures_and_the_rerun(oracle_lib, monkeypatch):
    targets = _structure_case()
    assert not ct.conforming(*[(p, len(q), len(targets[2][0]), o) for p, q, o in targets[2][1]][3])
    # (the edit arena starts at two entries: the batch is run again with the size the device asked for)
    monkeypatch.setenv("DAGCON_EDITS_CAP", "2")
    dev, status, reruns = _run_whole(targets, 0, min_len=1)
    assert reruns >= 1
    assert status == [0, 0, NONCONFORMING, 0]
    assert len(dev[0]) >= 3 and any(len(seq) == 1 for seq, _, _, _ in dev[0])
    assert dev[1] == [] and dev[2] == [] and dev[3]
    assert sum(len(e) for _, _, _, e in dev[0]) >= 1 and sum(len(e) for _, _, _, e in dev[3]) > 2


def _with_variants(rng, alns, tlen, n_var):
    """Every read that covers one of n_var random target positions carries the same variant there -- another base, the
    base gone, or one to three bases behind it -- so that the consensus differs from its target, not only the reads."""
    var = {}
    for p in rng.choice(np.arange(2, tlen - 2), size=min(n_var, tlen - 4), replace=False).tolist():
        u = rng.random()
        var[p] = ("sub", b"ACGT"[rng.integers(0, 4)]) if u < 0.4 else ("del",) if u < 0.7 else \
                 ("ins", bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(1, 4)))))
    out = []
    for s, q, t in alns:
        nq, nt, x = bytearray(), bytearray(), s - 1
        for qb, tb in zip(q, t):
            v = var.get(x) if tb != ct.GAP else None
            if v and v[0] == "sub" and qb != ct.GAP:
                qb = v[1]
            if v and v[0] == "del":
                qb = ct.GAP
            nq.append(qb); nt.append(tb)
            if v and v[0] == "ins":
                nq += v[1]; nt += b"-" * len(v[1])
            x += tb != ct.GAP
        out.append((s, bytes(nq), bytes(nt)))
    return out


def _random_targets(seed, n, lo, hi, mask=True, upper_reads=False, full_span=None):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        tlen = int(rng.integers(lo, hi + 1))
        alns, bb = random_target(rng, tlen, int(rng.integers(8, 13)), sub=0.03, ins=0.05, dele=0.04,
                                 full_span=bool(k % 3 == 0) if full_span is None else full_span)
        alns = _with_variants(rng, alns, tlen, 8)
        if mask:                                                # a soft-masked target stretch; half the reads follow it
            a = int(rng.integers(0, tlen - 20)); b = a + int(rng.integers(5, 20))
            low = bb[:a] + bb[a:b].lower() + bb[b:]
            new = []
            for j, (s, q, t) in enumerate(alns):
                t2 = _retarget(s, t, low)
                if j % 2 and not upper_reads:
                    q = bytes(tb if (qb | 0x20) == tb and tb != ct.GAP else qb for qb, tb in zip(q, t2))
                new.append((s, q, t2))
            alns, bb = new, low
        out.append((bb, _records(bb, alns, eqx=True)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 5])
def test_random_targets(oracle_lib, trim):
    targets = _random_targets(31 + trim, 300, 150, 700)
    dev, status, _ = _run_whole(targets, trim)
    assert status == [0] * 300
    n = sum(len(e) for per in dev for _, _, _, e in per)
    both = sum(1 for per in dev for _, _, _, e in per for _, tl, _, cl in e if tl and cl)
    case = sum(1 for per, (bb, _) in zip(dev, targets) for seq, _, _, e in per for p, tl, c, cl in e
               if tl and cl and (bb[p] ^ seq[c]) == 0x20)
    print("edits %d, replacements %d, of which a case change at the first byte %d" % (n, both, case))
    assert n > 1500 and both > 100 and case > 20


@pytest.mark.gpu
@pytest.mark.parametrize("lane", ["0", "2"])
def test_full_span_walks(oracle_lib, monkeypatch, lane):
    """Full-span pileups take the other two walks: a wave per piece (DAGCON_BP_LANE=0) and a row of eight lanes (2)."""
    monkeypatch.setenv("DAGCON_BP_LANE", lane)
    targets = _random_targets(55, 60, 150, 700, full_span=True)
    dev, status, _ = _run_whole(targets, 5)
    assert status == [0] * 60 and sum(len(e) for per in dev for _, _, _, e in per) > 300


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, 5])
def test_windows(oracle_lib, trim):
    from pbdagcon_amd import capi
    targets = _random_targets(77, 40, 250, 600)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 100, 20)
    wins = list(zip(hw.target.tolist(), hw.begin.tolist(), hw.end.tolist()))
    per = wt.window_targets(targets, wins)
    assert not any(f for _, _, f in per)
    wseqs = [targets[g][0][a:b] for g, a, b in wins]
    exp = et.batch_edits([(ws, alns) for ws, (_, alns, _) in zip(wseqs, per)], MIN_COV, MIN_LEN, trim)
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=trim, flags=capi.FLAG_BASE_POS)
    try:
        ctx.set_edits(True)
        got = ctx.consensus_cigar_windows(capi.HostCigarBatch(**ct.records_to_arrays(targets)), hw)
        dev = _device(ctx, got)
    finally:
        ctx.close()
    assert dev == exp
    assert _assert_invariant(dev, wseqs) > 300 and sum(1 for p in dev if p) > 100


@pytest.mark.gpu
def test_packed_stranded_and_cs_give_the_plain_call_s_arrays(oracle_lib):
    """Packed, stranded and cs uploads of the same alignments: the consensus and every edit array of the plain call (c_off
    counted from its segment's seq_off: the place of a target in seq_blob is not fixed from run to run)."""
    from pbdagcon_amd import capi
    targets = _random_targets(91, 30, 150, 500, upper_reads=True)
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 100, 20)
    n = sum(len(recs) for _, recs in targets)
    reverse = (np.arange(n) % 3 == 1).astype(np.uint8)
    as_file, i = [], 0
    for bb, recs in targets:
        as_file.append((bb, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(recs)]))
        i += len(recs)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    forms = {"packed": plain.packed(), "stranded": capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)),
             "cs": capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs])
                                                  for bb, recs in targets])}
    ctx = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=capi.FLAG_BASE_POS)
    try:
        ctx.set_edits(True)

        def arrays(batch, win):
            if isinstance(batch, capi.HostCsBatch):
                got = ctx.consensus_cs(batch, win)
            else:
                got = ctx._intake(batch, win, (batch, win), True)
            # c_off indexes seq_blob, where the targets lie in the order k_bp_join's waves took their places: that order
            # may differ from run to run, so an edit's c_off is compared relative to its segment's seq_off
            ed = ctx.edits()
            so = ctx._segs[1].astype(np.int64)
            per_seg = np.diff(ed["edit_begin"].astype(np.int64))
            ed["c_off"] = ed["c_off"].astype(np.int64) - np.repeat(so, per_seg)
            assert (ed["c_off"] >= 0).all()
            return got, ed
        for win in (None, hw):
            ref_got, ref = arrays(plain, win)
            assert ref["t_pos"].size > 100
            for kind, batch in forms.items():
                got, ed = arrays(batch, win)
                assert got == ref_got, kind
                assert sorted(ed) == sorted(ref)
                for k in ref:
                    assert np.array_equal(ed[k], ref[k]), (kind, k)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_state_rules_and_the_kind_bit_never_leaks(oracle_lib, monkeypatch):
    from pbdagcon_amd import capi
    from util import batch_from_targets
    targets = _random_targets(13, 12, 150, 400) + _structure_case()[:1]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    hw = capi.HostWindows.tiled([len(bb) for bb, _ in targets], 100, 20)
    sb = batch_from_targets([(len(bb), [ct.expand(p, q, bb, o) for p, q, o in recs], None) for bb, recs in targets])
    STATE = -8

    def code(f):
        with pytest.raises(capi.DagconError) as e:
            f()
        return e.value.code
    plain = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5)
    try:
        assert code(lambda: plain.set_edits(True)) == STATE
        assert code(plain.edits) == STATE
    finally:
        plain.close()
    flags = capi.FLAG_BASE_POS | capi.FLAG_BASE_SUPPORT
    off = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=flags)
    on = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=flags)
    stop = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=flags | capi.FLAG_STOP_AFTER_MERGE)
    try:
        assert code(off.edits) == STATE                          # edits off, nothing fetched
        off.consensus_cigar(cb)
        assert code(off.edits) == STATE                          # edits off, after a fetch
        on.set_edits(True)
        assert code(on.edits) == STATE                           # before a fetch
        on.upload_cigar(cb); on.run(); on.sync()
        assert code(on.edits) == STATE                           # run, not fetched
        on.fetch()
        assert on.edits()["t_pos"].size > 0
        on.consensus(sb)
        assert code(on.edits) == STATE                           # dagcon_consensus: no single target on the device
        stop.set_edits(True)
        stop.consensus_cigar(cb)
        assert code(stop.edits) == STATE                         # stopped before bestPath
        # with edits on, segments, positions and support are those of a context that never heard of them; asked for
        # before and after the edits, whole targets and windows (partial spans: the walk in pieces; test_full_span_walks
        # has the other two)
        for win in (None, hw):
            for lane in ("1", "2"):
                monkeypatch.setenv("DAGCON_BP_LANE", lane)
                a = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=flags)
                b = capi.Context(min_cov=MIN_COV, min_len=MIN_LEN, trim=5, flags=flags)
                try:
                    b.set_edits(True)
                    call = (lambda c: c.consensus_cigar(cb)) if win is None else (lambda c: c.consensus_cigar_windows(cb, win))
                    ga, gb = call(a), call(b)
                    assert ga == gb
                    pa, pb_, sa, sb_ = a.base_positions(), b.base_positions(), a.base_support(), b.base_support()
                    b.edits()
                    pb2 = b.base_positions()
                    for x, y, z in zip(pa, pb_, pb2):
                        assert len(x) == len(y) and all(np.array_equal(u, v) and np.array_equal(u, w) for u, v, w in zip(x, y, z))
                        assert all(int(u.max(initial=0)) < 2 ** 31 for u in y)
                    for x, y in zip(sa, sb_):
                        assert all(np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) for u, v in zip(x, y))
                    b.set_edits(False)
                    assert call(b) == ga and code(b.edits) == STATE
                    assert all(np.array_equal(u, v) for x, y in zip(pa, b.base_positions()) for u, v in zip(x, y))
                finally:
                    monkeypatch.undo()
                    a.close(); b.close()
    finally:
        off.close(); on.close(); stop.close()


def _apply_report(text, refs):
    """The pieces of an --edits file, each rebuilt from the reference: [(name, t0, t1, sequence)]."""
    out, cur = [], None
    for ln in text.decode().splitlines():
        if ln.startswith("#piece "):
            _, name, t0, t1 = ln.split(" ")
            cur = [name, int(t0), int(t1), []]
            out.append(cur)
        else:
            name, b, e, ref, alt = ln.split("\t")
            assert cur is not None and name == cur[0]
            ref, alt = ("" if x == "-" else x for x in (ref, alt))
            assert refs[name][int(b):int(e)].decode() == ref and (ref or alt) and int(e) - int(b) == len(ref)
            cur[3].append((int(b), int(e) - int(b), alt.encode()))
    res = []
    for name, t0, t1, edits in out:
        seq, at = b"", t0
        for b, n, alt in edits:
            assert at <= b and b + n <= t1
            seq += refs[name][at:b] + alt; at = b + n
        res.append((name, t0, t1, seq + refs[name][at:t1]))
    return res


@pytest.mark.gpu
def test_pbdagcon_edits_sam_bam_and_paf_cs(oracle_lib, tmp_path):
    """pbdagcon --edits on three targets as SAM, BAM and PAF with cs:Z: tags: stdout is that of the command without
    --edits, and every #piece of the file, its edits applied to the --ref sequence, is the FASTA record beside it."""
    import bam_files as bf
    targets = _random_targets(101, 3, 300, 600, upper_reads=True)
    names = ["ctgA", "ctgB", "ctgC"]
    refs = {n: bb for n, (bb, _) in zip(names, targets)}
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, [len(bb) for bb, _ in targets], [r for _, r in targets]))
    bam = tmp_path / "in.bam"
    bam.write_bytes(bf.bgzf(bf.bam_bytes([(n, len(refs[n])) for n in names],
                                         [dict(qname="q%d_%d" % (g, k), ref=g, pos=p, ops=o, seq=q, flag=0)
                                          for g, (_, recs) in enumerate(targets) for k, (p, q, o) in enumerate(recs)])))
    paf = tmp_path / "in.paf"
    paf.write_text("".join("q%d_%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t0\t0\t60\tcs:Z:%s\n" % (
        g, k, len(q), len(q), names[g], len(bb), p - 1, p - 1 + pf.tspan(o), cst.encode(p, q, bb, o).decode())
        for g, (bb, recs) in enumerate(targets) for k, (p, q, o) in enumerate(recs)))
    outs = []
    for kind, args in (("sam", ["--sam", str(sam)]), ("bam", ["--bam", str(bam)]), ("cs", ["--paf", "--cs", str(paf)])):
        ed = tmp_path / (kind + ".edits")
        base = [_cli(), "--ref", str(ref), "-c", "3", "-m", "30", "-t", "5"]
        plain = subprocess.run(base + args, capture_output=True, timeout=300)
        got = subprocess.run(base + ["-v", "--edits", str(ed)] + args, capture_output=True, timeout=300)
        assert plain.returncode == 0 and got.returncode == 0, (kind, plain.stderr.decode(), got.stderr.decode())
        assert got.stdout == plain.stdout and got.stdout.count(b">") >= 3, kind
        assert b"edits written to" in got.stderr
        pieces = _apply_report(ed.read_bytes(), refs)
        fasta = got.stdout.decode().split("\n")
        assert [">" + p[0] for p in pieces] == [h.split("/")[0] for h in fasta[0::2] if h]
        assert [p[3].decode() for p in pieces] == [x for x in fasta[1::2]], kind
        assert sum(1 for ln in ed.read_bytes().splitlines() if not ln.startswith(b"#")) >= 10
        by_name = {}
        for name, t0, t1, _ in pieces:                           # pieces of a target do not overlap
            assert by_name.get(name, 0) <= t0 <= t1
            by_name[name] = t1
        outs.append((got.stdout, ed.read_bytes()))
    assert outs[0] == outs[1] == outs[2]


def _designed_window_target():
    """450 bases, no base equal to its neighbour, ten identical full-span records that agree on edits at the core
    boundaries of --window 100: a substitution at base 99, one inserted base in front of base 200, bases 300-301
    dropped, three inserted bases in front of base 398.  ((target, records), [(begin, end, REF, ALT)])."""
    rng = np.random.default_rng(8)
    bb = bytearray()
    while len(bb) < 450:
        b = int(rng.choice(np.frombuffer(b"ACGT", np.uint8)))
        if not bb or bb[-1] != b:
            bb.append(b)

    def other(*avoid):
        return next(b for b in b"ACGT" if b not in avoid)
    for i in (300, 301):                                        # the dropped bases cannot slide: unlike both neighbours' bases
        bb[i] = other(bb[i - 1], bb[302], bb[299])
    q, t, want = bytearray(), bytearray(), []
    for x in range(450):
        if x == 200:
            ins = bytes([other(bb[199], bb[200])])
            q += ins; t += b"-"; want.append((200, 200, "-", ins.decode()))
        if x == 398:
            ins = bytes([other(bb[397], bb[398]), other(other(bb[397], bb[398]), bb[398], bb[397]), other(bb[398], bb[397])])
            ins = ins[:1] + bytes([other(ins[0], ins[2])]) + ins[2:] if ins[1] in (ins[0], ins[2]) else ins
            q += ins; t += b"---"; want.append((398, 398, "-", ins.decode()))
        if x == 99:
            sub = other(bb[98], bb[99], bb[100])
            q.append(sub); t.append(bb[x]); want.append((99, 100, chr(bb[99]), chr(sub)))
        elif x in (300, 301):
            q += b"-"; t.append(bb[x])
        else:
            q.append(bb[x]); t.append(bb[x])
    want.append((300, 302, bytes(bb[300:302]).decode(), "-"))
    bb = bytes(bb)
    return (bb, [ct.compress(1, bytes(q), bytes(t), bb, eqx=bool(k % 2)) for k in range(10)]), sorted(want)


@pytest.mark.gpu
def test_pbdagcon_edits_with_windows(oracle_lib, tmp_path):
    """pbdagcon --sam --window 100 --overlap 70 --edits on a 450-base target whose records agree on edits at the core
    boundaries (within 3 bases of one each), and on a 450-base target with random reads: stdout is that of the command
    without --edits, every #piece, its edits applied to the --ref sequence, is the FASTA record beside it, the pieces of
    a target do not overlap.  The designed target is one piece named by its span, with exactly the designed edits."""
    designed, want = _designed_window_target()
    targets = [designed] + _random_targets(202, 1, 450, 450, upper_reads=True)
    names = ["ctgD", "ctgR"]
    refs = {n: bb for n, (bb, _) in zip(names, targets)}
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"
    sam.write_bytes(ct.to_sam(names, [450, 450], [sorted(r, key=lambda x: x[0]) for _, r in targets]))
    ed = tmp_path / "w.edits"
    base = [_cli(), "--sam", "--ref", str(ref), "-c", "3", "-m", "30", "-t", "5", "--window", "100", "--overlap", "70"]
    plain = subprocess.run(base + [str(sam)], capture_output=True, timeout=300)
    got = subprocess.run(base + ["-v", "--edits", str(ed), str(sam)], capture_output=True, timeout=300)
    assert plain.returncode == 0 and got.returncode == 0, (plain.stderr.decode(), got.stderr.decode())
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 2
    assert b"edits written to" in got.stderr
    text = ed.read_bytes()
    print(text.decode())
    pieces = _apply_report(text, refs)
    fasta = got.stdout.decode().split("\n")
    assert [">" + p[0] for p in pieces] == [h.split("/")[0] for h in fasta[0::2] if h]
    assert [p[3].decode() for p in pieces] == [x for x in fasta[1::2]]
    by_name = {}
    for name, t0, t1, _ in pieces:
        assert by_name.get(name, 0) <= t0 <= t1 <= 450
        by_name[name] = t1
    d = [(p, h) for p, h in zip(pieces, [h for h in fasta[0::2] if h]) if p[0] == "ctgD"]
    assert len(d) == 1 and d[0][1] == ">ctgD/%d_%d" % (d[0][0][1], d[0][0][2])
    lines = [ln.split("\t") for ln in text.decode().splitlines() if ln.startswith("ctgD\t")]
    assert [(int(b), int(e), r, a) for _, b, e, r, a in lines] == want
    assert sum(1 for ln in text.splitlines() if ln.startswith(b"ctgR\t")) >= 5
