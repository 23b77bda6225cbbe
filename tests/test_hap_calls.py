"""dagcon_set_hap_calls: the derived batch of dagcon_upload_haps reports its edits, and k_hap_calls pairs the two groups'
edits (include/dagcon.h rule 11).  The rule by hand and against wrong versions of itself on the CPU; on the GPU the device's
arrays against tests/hap_calls_twin.py, the derived batch's edits against a fresh context on each group's records, the
state rules, and pbdagcon --hap-vcf."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cigar_twin as ct
import cs_twin as cst
import hap_calls_twin as hct
import md_twin as mt
import paf_files as pf
import site_reads_twin as srt
from hap_calls_twin import NOCOVER, HET, CLASH, HOM, NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, NONCONFORMING = -8, -4
NAMES = ("dagcon_set_hap_calls", "dagcon_fetch_hap_calls")
SITES = (2, 200000)


def _tes():
    import test_edit_support as tes
    return tes


def _cli():
    return _tes()._cli()


def _code(f):
    from pbdagcon_amd import capi
    with pytest.raises(capi.DagconError) as e:
        f()
    return e.value.code


# ---- CPU: the rule by hand ------------------------------------------------------------------------------------------

def S(p, b=b"G"):
    return (p, 1, b)


def I(p, b=b"G"):
    return (p, 0, b)


def D(p, n=1):
    return (p, n, b"")


# (own edits, partner edits, partner spans or None) -> [(state, mate)]; each is one of the cases the issue lists
CASES = {
    "hom": ([S(10)], [S(10)], [(0, 50)], [(HOM, 0)]),
    "het": ([S(10)], [S(20)], [(0, 50)], [(HET, None)]),
    "clash": ([S(10, b"G")], [S(10, b"T")], [(0, 50)], [(CLASH, 0)]),
    "nocover": ([S(10)], [], [(20, 50)], [(NOCOVER, None)]),
    "ins at the partner's t0": ([I(20)], [], [(20, 50)], [(HET, None)]),
    "ins at the partner's t1": ([I(50)], [], [(20, 50)], [(HET, None)]),
    "ins at p against a substitution of [p, p + 1)": ([I(10)], [S(10)], [(0, 50)], [(CLASH, 0)]),
    "ins at p against a deletion of [p - 1, p)": ([I(10)], [D(9)], [(0, 50)], [(HET, None)]),
    "adjacent substitutions": ([S(10)], [S(11)], [(0, 50)], [(HET, None)]),
    "alt differs in its last byte": ([(10, 2, b"ACGT")], [(10, 2, b"ACGA")], [(0, 50)], [(CLASH, 0)]),
    "alt differs in case": ([(10, 2, b"ACGT")], [(10, 2, b"ACGt")], [(0, 50)], [(CLASH, 0)]),
    "partner without edits": ([S(10), D(30, 3)], [], [(0, 50)], [(HET, None), (HET, None)]),
    "partner without segments": ([S(10), D(30, 3)], [], [], [(NOCOVER, None), (NOCOVER, None)]),
    "partner failed": ([S(10)], [S(10)], None, [(NOCOVER, None)]),
    "deletion that ends at the partner's t1": ([D(47, 3)], [], [(0, 50)], [(HET, None)]),
    "deletion that ends one past the partner's t1": ([D(48, 3)], [], [(0, 50)], [(NOCOVER, None)]),
    "covered by the partner's second segment only": ([S(60)], [S(10)], [(0, 50), (55, 90)], [(HET, None)]),
    "the lowest of two clashing edits": ([D(10, 5)], [S(9), S(11), S(14), S(15)], [(0, 50)], [(CLASH, 1)]),
    "a clash where the cover also holds": ([S(10, b"G")], [D(10, 2)], [(0, 50)], [(CLASH, 0)]),
}


def test_the_rule_by_hand():
    for name, (own, partner, spans, want) in CASES.items():
        assert hct.pair(own, partner, spans) == want, name
    # a whole derived batch: two pairs, the second with a failed label-2 target; states and mates flat, in host order
    t = [([(0, 50)], [S(5), S(10, b"G"), I(20), S(30)]), ([(0, 25)], [S(5), S(10, b"T"), S(22)]),
         ([(0, 50)], [S(7)]), (None, [S(7)])]
    state, mate = hct.calls(t)
    assert state == [HOM, CLASH, HET, NOCOVER, HOM, CLASH, HET, NOCOVER]
    assert mate == [4, 5, NONE, NONE, 0, 1, NONE, NONE]
    assert hct.occupied(I(7)) == (7, 8) and hct.occupied(D(7, 3)) == (7, 10) and hct.occupied(S(7)) == (7, 8)


def _wrong_versions():
    def closed(a, b):
        (a0, a1), (b0, b1) = hct.occupied(a), hct.occupied(b)
        return a0 <= b1 and b0 <= a1

    def no_max(a, b):
        return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]

    def nocase(a, b):
        return a[0] == b[0] and a[1] == b[1] and bytes(a[2]).upper() == bytes(b[2]).upper()

    def strict(e, spans):
        return any(t0 < e[0] and e[0] + e[1] < t1 for t0, t1 in spans)

    def first_only(e, spans):
        return hct.covered(e, spans[:1])

    def no_t_len(e, spans):
        return any(t0 <= e[0] <= t1 for t0, t1 in spans)
    return {"closed intervals": dict(overlap=closed), "no max(t_len, 1)": dict(overlap=no_max), "cover before CLASH": dict(cover_first=True),
            "case-insensitive compare": dict(same=nocase), "cover with <": dict(covered=strict), "the partner's first segment only": dict(covered=first_only),
            "cover without t_len": dict(covered=no_t_len)}


def test_wrong_versions_of_the_rule_are_rejected():
    for name, kw in _wrong_versions().items():
        caught = [c for c, (own, partner, spans, want) in CASES.items() if hct.pair(own, partner, spans, **kw) != want]
        assert caught, name
        print("%-36s rejected by: %s" % (name, "; ".join(caught)))
    # each of them by the case that names its part of the rule
    by = {"closed intervals": "adjacent substitutions", "no max(t_len, 1)": "ins at p against a substitution of [p, p + 1)",
          "cover before CLASH": "a clash where the cover also holds", "case-insensitive compare": "alt differs in case",
          "cover with <": "ins at the partner's t0", "the partner's first segment only": "covered by the partner's second segment only",
          "cover without t_len": "deletion that ends one past the partner's t1"}
    for name, case in by.items():
        own, partner, spans, want = CASES[case]
        assert hct.pair(own, partner, spans, **_wrong_versions()[name]) != want, (name, case)


def _random_group(rng, tlen):
    """Edits with disjoint occupied intervals and rising t_pos, and one to three spans."""
    edits, p = [], int(rng.integers(0, 6))
    while p < tlen - 6:
        kind = int(rng.integers(0, 3))
        n = int(rng.integers(1, 4))
        alt = bytes(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), int(rng.integers(1, 4))).tolist())
        e = (p, 0, alt) if kind == 0 else (p, n, b"") if kind == 1 else (p, n, alt)
        edits.append(e)
        p = hct.occupied(e)[1] + int(rng.integers(0, 5))
    cuts = sorted(set(rng.integers(0, tlen + 1, int(rng.integers(1, 4)) * 2).tolist()))
    spans = list(zip(cuts[0::2], cuts[1::2]))
    return spans, edits if spans else []                                 # (a target without a segment has no edits)


def test_twin_invariants_on_random_small_edit_lists():
    rng = np.random.default_rng(11)
    seen = [0, 0, 0, 0]
    for k in range(400):
        tlen = int(rng.integers(10, 60))
        a, b = _random_group(rng, tlen), _random_group(rng, tlen)
        if k % 3 == 0:                                                   # shared edits: something to be HOM
            b = (b[0], sorted(set(b[1][::2]) | {e for e in a[1][::2] if not any(hct.overlap(e, x) for x in b[1][::2])}) if b[0] else [])
            try:
                hct.check_ascent(b[1])
            except AssertionError:
                continue
        targets = [a, b] if k % 7 else [a, (None, b[1])]
        state, mate = hct.calls(targets)                                 # (asserts the symmetry, the involution and the ascent)
        n1 = len(a[1])
        for i, (s, m) in enumerate(zip(state, mate)):
            seen[s] += 1
            if m != NONE:
                assert (i < n1) != (m < n1)                              # a mate is in the partner's stretch
        assert len(state) == n1 + (len(b[1]) if targets[1][0] is not None else 0)
    print("NOCOVER %d, HET %d, CLASH %d, HOM %d" % tuple(seen))
    assert min(seen) > 50


def test_binding_exports_and_struct_size():
    from pbdagcon_amd import capi
    import test_abi
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == test_abi.declared_functions()
    prog = ('#include <stdio.h>\n#include "dagcon.h"\nint main(void){printf("%zu %d %d %d %d\\n", sizeof(dagcon_hap_calls), DAGCON_HC_NOCOVER, '
            'DAGCON_HC_HET, DAGCON_HC_CLASH, DAGCON_HC_HOM); return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert ctypes.sizeof(capi.HapCalls) == out[0] == 24
    assert out[1:] == [capi.HC_NOCOVER, capi.HC_HET, capi.HC_CLASH, capi.HC_HOM] == [NOCOVER, HET, CLASH, HOM] and capi.HC_NONE == NONE
    assert callable(capi.Context.set_hap_calls) and callable(capi.Context.hap_calls)
    assert lib.dagcon_abi_version() == 2 and capi.ABI_VERSION == 2
    rule = open(os.path.join(ROOT, "include", "dagcon.h")).read().split(" * 11. ")[1].split("*/")[0]
    assert "PARITY UNPINNED" in open(os.path.join(ROOT, "include", "dagcon.h")).read().split(" * 11. ")[0][-400:] and "max(t_len, 1)" in rule


def test_usage_errors_and_help(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    m5 = tmp_path / "in.m5"; m5.write_text("")
    f = tmp_path / "o.vcf"
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(["c"], [b"ACGT" * 100]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(["c"], [400], [[]]))

    def run(*args):
        return subprocess.run([_cli(), *args], capture_output=True, env=env, timeout=120)
    rec = ["--sam", "--ref", str(ref)]
    for args in (rec + [str(sam), "--hap-vcf"], ["--hap-vcf", str(f), str(m5)],
                 rec + ["--window", "200", "--overlap", "120", "--hap-vcf", str(f), str(sam)],
                 ["-a", "--hap-vcf", str(f), str(m5)], ["-a", "--polish", "1", "--hap-vcf", str(f), str(m5)],
                 rec + ["--dump-parsed", "--hap-vcf", str(f), str(sam)],
                 rec + ["--hap-vcf", str(f), "--hap-min-sites", "x", str(sam)], rec + ["--hap-vcf", str(f), "--site-min-frac", "1.5", str(sam)]):
        out = run(*args)
        assert out.returncode == 2 and b"PARSE ERROR" in out.stderr, args
        assert not f.exists()
    out = run(*rec, "--hap-vcf", str(tmp_path / "no_such_dir" / "o.vcf"), "--hap-min-sites", "3", "--site-min-count", "3", str(sam))
    assert out.returncode == 1 and b"cannot write" in out.stderr
    h = run("--help")
    assert h.returncode == 0
    text = h.stdout.split(b"\n  --hap-vcf FILE")[1].split(b"\n  --polish")[0]
    for word in (b"PAIR=UNSPLIT;DP=span;AD=ref,alt", b"1/1", b"PAIR=HOM 1|1", b"PAIR=HET 1|0 or 0|1", b"PAIR=CLASH 1|. and .|1", b"PAIR=NOCOV",
                 b"GT:PS", b"parity unpinned", b"--window"):
        assert word in text, word
    assert b"[--hap-vcf FILE]" in h.stdout.split(b"\n")[0]


_VCF_MAIN = r"""
#include <iostream>
#include "hap_vcf.h"
// stdin: "u name target n" or "s name target n1 n2", then per edit "t_pos t_len alt span ref alt_n state mate" ('-': an empty alt)
int main() {
    std::string out, kind, name, target;
    dg_hap_vcf_header(out, "##contig=<ID=ctg,length=12345>\n");
    auto edits = [](size_t n) {
        std::vector<DgHapVcfEdit> v(n);
        for (auto &e : v) { std::cin >> e.t_pos >> e.t_len >> e.alt >> e.span >> e.n_ref >> e.n_alt >> e.state >> e.mate; if (e.alt == "-") e.alt.clear(); }
        return v;
    };
    while (std::cin >> kind >> name >> target) {
        size_t n1, n2;
        if (kind == "u") { std::cin >> n1; dg_hap_vcf_unsplit(out, name, target.data(), (uint32_t)target.size(), edits(n1)); }
        else { std::cin >> n1 >> n2; const auto a = edits(n1); const auto b = edits(n2); dg_hap_vcf_split(out, name, target.data(), (uint32_t)target.size(), a, b); }
    }
    std::cout << out;
    return 0;
}
"""


def test_the_line_formatter_against_python(tmp_path):
    src = tmp_path / "hap_vcf_main.cpp"; src.write_text(_VCF_MAIN)
    exe = tmp_path / "hap_vcf_main"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "pbdagcon_amd", "csrc", "host"), "-o", str(exe), str(src)])
    T = b"ACGTTTGACA"
    un = [((3, 1, b"C"), (9, 2, 7)), ((6, 0, b"T"), (8, 3, 5)), ((0, 2, b""), (4, 1, 3)), ((10, 0, b"A"), (4, 1, 3))]
    e1 = [(0, 0, b"GG"), (2, 1, b"A"), (4, 2, b""), (7, 1, b"T"), (9, 1, b"G")]
    s1 = [(5, 1, 4), (6, 0, 6), (7, 2, 5), (8, 3, 5), (2, 0, 2)]
    c1 = [(HET, None), (HOM, 0), (CLASH, 1), (NOCOVER, None), (HOM, 3)]
    e2 = [(2, 1, b"A"), (4, 1, b"C"), (6, 0, b"TT"), (9, 1, b"G")]
    s2 = [(7, 1, 6), (9, 4, 5), (4294967295, 4294967295, 0), (3, 1, 2)]
    c2 = [(HOM, 1), (CLASH, 2), (HET, None), (HOM, 4)]

    def row(e, s, c):
        return "%d %d %s %d %d %d %d %d\n" % (e[0], e[1], e[2].decode() or "-", s[0], s[1], s[2], c[0], -1 if c[1] is None else c[1])
    text = "u ctg %s %d\n" % (T.decode(), len(un)) + "".join(row(e, s, (0, None)) for e, s in un)
    text += "s a/b|c %s %d %d\n" % (T.decode(), len(e1), len(e2)) + "".join(map(row, e1, s1, c1)) + "".join(map(row, e2, s2, c2))
    text += "s empty %s 0 0\n" % T.decode()
    out = subprocess.run([str(exe)], input=text.encode(), capture_output=True, check=True, timeout=60).stdout.decode().splitlines()
    want = hct.header([("ctg", 12345)]) + hct.unsplit_lines("ctg", T, [e for e, _ in un], [s for _, s in un])
    want += hct.split_lines("a/b|c", T, e1, s1, c1, e2, s2, c2)
    assert out == want
    body = [ln.split("\t") for ln in out if not ln.startswith("#")]
    assert out[0] == "##fileformat=VCFv4.2" and out[1] == "##contig=<ID=ctg,length=12345>" and sum(ln.startswith("##pbdagcon_note=") for ln in out) == 2
    assert [ln.split(",")[0] for ln in out if ln.startswith("##INFO") or ln.startswith("##FORMAT")] == [
        "##INFO=<ID=PAIR", "##INFO=<ID=DP", "##INFO=<ID=AD", "##INFO=<ID=DP1", "##INFO=<ID=AD1", "##INFO=<ID=DP2", "##INFO=<ID=AD2", "##FORMAT=<ID=GT", "##FORMAT=<ID=PS"]
    assert out[len(hct.header([])) ] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample"
    assert body[0] == ["ctg", "4", ".", "T", "C", ".", ".", "PAIR=UNSPLIT;DP=9;AD=2,7", "GT", "1/1"]
    assert body[1][1:5] == ["6", ".", "T", "TT"] and body[2][1:5] == ["1", ".", "ACG", "G"] and body[3][1:5] == ["10", ".", "A", "AA"]
    sp = body[4:]
    # merged by (t_pos, label), the HOM mates of label 2 left out: 5 + 4 - 2 lines
    assert [(x[1], x[7].split(";")[0], x[9]) for x in sp] == [
        ("1", "PAIR=HET", "1|0:1"), ("3", "PAIR=HOM", "1|1:1"), ("4", "PAIR=CLASH", "1|.:1"), ("5", "PAIR=CLASH", ".|1:1"),
        ("6", "PAIR=HET", "0|1:1"), ("8", "PAIR=NOCOV", "1|.:1"), ("10", "PAIR=HOM", "1|1:1")]
    assert sp[1][7] == "PAIR=HOM;DP1=6;AD1=0,6;DP2=7;AD2=1,6" and sp[3][7] == "PAIR=CLASH;DP2=9;AD2=4,5" and all(x[8] == "GT:PS" for x in sp)
    assert sp[4][7] == "PAIR=HET;DP2=4294967295;AD2=4294967295,0"


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _sub(bb, p, other=b""):
    """A substitution at p by a base that neither neighbour is; `other`: not that one either (bb[p - 1] == bb[p + 1] then)."""
    return ("s", bytes([next(b for b in b"ACGT" if b not in (bb[p - 1], bb[p], bb[p + 1]) and b not in other)]))


def _reads(bb, events, spans):
    """Gapped strings of error-free reads of the haplotype `events` describes ({target position: ('s', base) | ('i', bases
    in front of it) | ('d',)}), one per (begin, end) of spans; events at a read's first and last two bases are left out."""
    out = []
    for s, e in spans:
        q, t = bytearray(), bytearray()
        for p in range(s, e):
            kind = events.get(p, (None,)) if s + 2 <= p < e - 2 else (None,)
            if kind[0] == "i":
                q += kind[1]; t += b"-" * len(kind[1])
            if kind[0] == "d":
                q.append(ct.GAP); t.append(bb[p]); continue
            q.append(kind[1][0] if kind[0] == "s" else bb[p]); t.append(bb[p])
        out.append((s + 1, bytes(q), bytes(t)))
    return out


def _as_edits(events, lo, hi):
    """The edits a consensus that equals the haplotype over [lo, hi) has against the target."""
    out = []
    for p in sorted(events):
        k = events[p]
        if lo <= p < hi:
            out.append((p, 1, k[1]) if k[0] == "s" else (p, 0, bytes(k[1])) if k[0] == "i" else (p, 1, b""))
    return out


def _target(bb, ev1, ev2, spans1, spans2):
    """(target bases, records): the reads of haplotype 1 first."""
    tes = _tes()
    alns = _reads(bb, ev1, spans1) + _reads(bb, ev2, spans2)
    return bb, tes._records(bb, alns)


def _planted_target(seed=3):
    """A 600-base target and two haplotypes of 12 reads each: het substitutions on haplotype 2 every 40 to 60 bases, one
    het inserted base at 305, two changes both carry (HOM, at 100 and 200), one position where they carry different
    substitutions (CLASH, at the first place from 240 on whose neighbours are equal, so that two other bases are left),
    and one change both carry at 560 -- where no read of haplotype 2 reaches: they end at 450."""
    tes = _tes()
    rng = np.random.default_rng(seed)
    bb = tes._nonrep(rng, 600)
    pc = next(p for p in range(240, 290) if bb[p - 1] == bb[p + 1])
    ev1, ev2, x = {}, {}, int(rng.integers(20, 40))
    while x < 440:
        if all(abs(x - p) > 3 for p in (100, 200, pc, 305)):
            ev2[x] = _sub(bb, x)
        x += int(rng.integers(40, 61))
    het = sorted(ev2)
    for p in (100, 200, 560):
        ev1[p] = ev2[p] = _sub(bb, p)
    ev1[pc] = _sub(bb, pc)
    ev2[pc] = _sub(bb, pc, other=ev1[pc][1])
    ev2[305] = ("i", bytes([next(b for b in b"ACGT" if b not in (bb[305], bb[304]))]))
    return _target(bb, ev1, ev2, [(0, 600)] * 12, [(0, 450)] * 12), ev1, ev2, het, pc


class _Run:
    """One context with every switch --hap-vcf turns on; the first batch by `call`, then the derived batch: its results,
    its edits in the twin's form, their support, the positions, the map and the calls."""

    def __init__(self, call, min_cov, min_len, trim, hap=(0, 0), calls=True, support=True, opts=SITES, prepare=None):
        from pbdagcon_amd import capi
        tes = _tes()
        c = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
        try:
            if prepare:
                prepare(c)
            c.set_edits(True)
            if support:
                c.set_edit_support(True)
            c.set_pileup(*opts); c.set_site_reads(True); c.set_hap_consensus(*hap)
            if calls:
                c.set_hap_calls(True)
            self.first = call(c)
            self.first_status = c.target_status.tolist()
            self.first_dev = tes._device(c, self.first)
            self.first_sup = tes._flat(c.edit_support()) if support else None
            self.sr, self.tally = c.site_reads(), c.hap_tally()
            assert _code(c.hap_calls) == STATE                          # the first batch has none
            c.upload_haps()
            self.map = c.hap_map()
            assert _code(c.hap_calls) == STATE and _code(c.edits) == STATE      # before the derived fetch
            c.run(); c.sync()
            self.got = c.fetch(strict=False)
            self.status = c.target_status.tolist()
            self.reruns = c.timings()["reruns"]
            if calls:
                self.dev = tes._device(c, self.got)
                self.sup = tes._flat(c.edit_support()) if support else None
                self.pos = c.base_positions()
                self.calls = c.hap_calls()
                again = c.hap_calls()
                assert all(np.array_equal(self.calls[k], again[k]) for k in again)
            else:
                assert _code(c.edits) == STATE and _code(c.hap_calls) == STATE and _code(c.edit_support) == STATE
        finally:
            c.close()

    def check_twin(self, tseqs):
        """(b) the edits INVARIANT from the device's own arrays against the source targets, (c) the calls against the twin."""
        import test_edits as te
        src = self.map["src_target"].tolist()
        n = te._assert_invariant(self.dev, [tseqs[t] for t in src])
        state, mate = hct.calls(hct.from_device(self.dev, self.status))
        assert self.calls["state"].tolist() == state and self.calls["mate"].tolist() == mate
        assert len(state) == n
        return state, mate

    def group(self, d):
        """[(t_pos, t_len, alt, state)] of derived target d."""
        flat = [(tp, tl, bytes(seq[c:c + cl])) for per in self.dev[:d] for seq, _, _, ed in per for tp, tl, c, cl in ed]
        own = [(tp, tl, bytes(seq[c:c + cl])) for seq, _, _, ed in self.dev[d] for tp, tl, c, cl in ed]
        st = self.calls["state"][len(flat):len(flat) + len(own)].tolist()
        return [e + (s,) for e, s in zip(own, st)]


def _whole(targets):
    return _tes()._whole(targets)


def _fresh_groups(run, targets, min_cov, min_len, trim):
    """(a) a fresh context on each group's records alone, edits and support on: the consensus, the edits, the support and
    the positions of the derived batch, byte for byte (c_off from its segment's seq_off)."""
    from pbdagcon_amd import capi
    tes = _tes()
    recs = [r for _, rs in targets for r in rs]
    b = run.map["aln_begin"].tolist()
    groups = [(targets[t][0], [recs[i] for i in run.map["aln_src"][b[d]:b[d + 1]].tolist()]) for d, t in enumerate(run.map["src_target"].tolist())]
    fresh = capi.Context(min_cov=min_cov, min_len=min_len, trim=trim, flags=capi.FLAG_BASE_POS)
    try:
        fresh.set_edits(True); fresh.set_edit_support(True)
        want = fresh.consensus_cigar(capi.HostCigarBatch(**ct.records_to_arrays(groups)), strict=False)
        assert run.got == want and run.status == fresh.target_status.tolist()
        assert run.dev == tes._device(fresh, want) and run.sup == tes._flat(fresh.edit_support())
        wp = fresh.base_positions()
        assert [len(x) for x in run.pos] == [len(x) for x in wp] and all(np.array_equal(a, b) for x, y in zip(run.pos, wp) for a, b in zip(x, y))
    finally:
        fresh.close()
    return groups


@pytest.mark.gpu
def test_the_planted_diploid_target(oracle_lib):
    tes = _tes()
    (bb, recs), ev1, ev2, het, pc = _planted_target()
    (_, alns), = tes._strings([(bb, recs)])
    tw = srt.target(600, alns, 100, 10, SITES)
    assert tw["hap"] == [1] * 12 + [2] * 12 and len(het) >= 6           # on the twin first: the planted groups come back
    r = _Run(_whole([(bb, recs)]), 6, 100, 10)
    assert r.first_status == [0] and r.tally["split"].tolist() == [1] and r.status == [0, 0]
    assert r.map["label"].tolist() == [1, 2] and r.map["aln_src"].tolist() == list(range(24))
    _fresh_groups(r, [(bb, recs)], 6, 100, 10)                          # (a)
    r.check_twin([bb])                                                   # (b), (c)
    # (d) the planted events with their planted states: group 1 reaches to 590, group 2 to 440
    g1, g2 = r.group(0), r.group(1)
    assert [e[:3] for e in g1] == _as_edits(ev1, 10, 590) and [e[:3] for e in g2] == _as_edits(ev2, 10, 440)
    assert [(tp, s) for tp, _, _, s in g1] == [(100, HOM), (200, HOM), (pc, CLASH), (560, NOCOVER)]
    assert ev1[pc] != ev2[pc] and ev1[pc][0] == ev2[pc][0] == "s"
    want2 = {100: HOM, 200: HOM, pc: CLASH}
    assert [(tp, s) for tp, _, _, s in g2] == [(p, want2.get(p, HET)) for p in sorted(ev2) if p < 440]
    assert (305, 0) in [(tp, tl) for tp, tl, _, _ in g2]
    # the support is the group's own: every read of a group carries its haplotype
    assert all(x[2] == 12 and x[3] == 12 and x[4] == 0 for x in r.sup)
    assert [per[0][1:3] for per in r.dev] == [(10, 590), (10, 440)]


def _grid_target(rng, n1, n2):
    """Haplotype 2 carries n2 substitutions at 20 + 4 k; haplotype 1 carries n1 changes: at every fifth k the same one
    (HOM), at the k behind it that base dropped instead (CLASH), else a substitution two bases further (HET)."""
    tes = _tes()
    tl = 40 + 4 * max(n1, n2) + 20
    bb = tes._nonrep(rng, tl)
    ev1, ev2 = {}, {}
    for k in range(n2):
        ev2[20 + 4 * k] = _sub(bb, 20 + 4 * k)
    for k in range(n1):
        p = 20 + 4 * k
        if k % 5 == 0 and k < n2:
            ev1[p] = ev2[p]
        elif k % 5 == 1 and k < n2:
            ev1[p] = ("d",)
        else:
            ev1[p + 2] = _sub(bb, p + 2)
    return _target(bb, ev1, ev2, [(0, tl)] * 8, [(0, tl)] * 8), ev1, ev2


def _segments_target(rng):
    """Groups of two and of three segments: three whole reads a haplotype carry the labels across, too few for min_cov,
    so each group's consensus breaks where only they cover.  Haplotype 2 has a substitution every 25 bases."""
    tes = _tes()
    bb = tes._nonrep(rng, 600)
    ev2 = {p: _sub(bb, p) for p in range(15, 590, 25)}
    ev1 = {p: ev2[p] for p in (140, 390)}                               # two the haplotypes share
    return _target(bb, ev1, ev2, [(0, 600)] * 3 + [(0, 250)] * 8 + [(300, 600)] * 8, [(0, 600)] * 3 + [(0, 180)] * 8 + [(220, 400)] * 8 + [(440, 600)] * 8)


def _long_insertion_target(rng):
    """Both haplotypes insert the same 70 bases at 100 and 70 bases that differ in the 70th at 200; haplotype 2 has
    substitutions besides, for the split.  The target is ACAC.. and the inserted bases are G and T, so that normalizeGaps
    finds no target base to move an inserted one to and each run stays one edit."""
    bb = b"AC" * 150
    ev2 = {p: _sub(bb, p) for p in range(30, 280, 40)}
    a, b = b"GT" * 35, b"TG" * 35
    ev1 = {100: ("i", a), 200: ("i", b)}
    ev2[100] = ("i", a)
    ev2[200] = ("i", b[:-1] + b"T")
    return _target(bb, ev1, ev2, [(0, 300)] * 8, [(0, 300)] * 8), ev1, ev2


def _size_targets():
    """The batch of the size tests: a failed target in front, two unsplit ones between the split ones."""
    tes = _tes()
    rng = np.random.default_rng(17)
    plain = tes._nonrep(rng, 200)
    failed = _target(plain, {}, {60: _sub(plain, 60), 120: _sub(plain, 120)}, [(0, 200)] * 6, [(0, 200)] * 6)
    p, q, o = failed[1][1]
    failed[1][1] = (len(plain) + 1, q, o)
    un1 = _target(plain, {50: _sub(plain, 50)}, {50: _sub(plain, 50)}, [(0, 200)] * 6, [(0, 200)] * 6)      # every read the same change: no site
    un2 = _target(plain, {}, {}, [(0, 200)] * 6, [(0, 200)] * 6)
    grids = [_grid_target(rng, n1, n2) for n1, n2 in ((63, 64), (65, 129), (0, 65))]
    segs = _segments_target(rng)
    ins = _long_insertion_target(rng)
    targets = [failed, grids[0][0], un1, grids[1][0], grids[2][0], un2, segs, ins[0]]
    return targets, grids, ins


N1 = [6, 8, 6, 8, 8, 6, 19, 8]                                           # the reads of haplotype 1 in each of them, in front


@pytest.mark.gpu
def test_sizes_where_the_kernel_can_go_wrong(oracle_lib):
    tes = _tes()
    targets, grids, ins = _size_targets()
    strings = tes._strings(targets)
    assert strings[0] is None
    for t in (1, 3, 4, 6, 7):                                            # on the twin first: the haplotypes come back as the labels
        hap = srt.target(len(targets[t][0]), strings[t][1], 100, 5, SITES)["hap"]
        assert set(hap[:N1[t]]) == {1} and set(hap[N1[t]:]) == {2}, t
    r = _Run(_whole(targets), 6, 100, 5)
    assert r.first_status == [NONCONFORMING] + [0] * 7 and r.tally["split"].tolist() == [0, 1, 0, 1, 1, 0, 1, 1]
    assert r.map["src_target"].tolist() == [1, 1, 3, 3, 4, 4, 6, 6, 7, 7] and r.status == [0] * 10
    # the first batch's own edits are those of the unsplit targets too: the failed one has none
    assert r.first_dev[0] == [] and len(r.first_dev[2][0][3]) == 1 and r.first_dev[5][0][3] == []
    state, mate = r.check_twin([bb for bb, _ in targets])
    _fresh_groups(r, targets, 6, 100, 5)
    # 64 lanes a step: the groups' edit counts, and the states by design
    for d, ((_, ev1, ev2), (n1, n2)) in zip((0, 2, 4), zip(grids, ((63, 64), (65, 129), (0, 65)))):
        g1, g2 = r.group(d), r.group(d + 1)
        assert (len(g1), len(g2)) == (n1, n2)
        assert [e[:3] for e in g1] == _as_edits(ev1, 0, 10 ** 6) and [e[:3] for e in g2] == _as_edits(ev2, 0, 10 ** 6)
        assert [s for *_, s in g1] == [HOM if k % 5 == 0 and k < n2 else CLASH if k % 5 == 1 and k < n2 else HET for k in range(n1)]
        assert [s for *_, s in g2] == [HOM if k % 5 == 0 and k < n1 else CLASH if k % 5 == 1 and k < n1 else HET for k in range(n2)]
    # two and three segments, a coverage gap in the middle: every state occurs, NOCOVER where the partner has the gap
    spans = [[(t0, t1) for _, t0, t1, _ in per] for per in r.dev[6:8]]
    assert [len(s) for s in spans] == [2, 3] and spans[0][0][1] < spans[0][1][0] and spans[1][0][1] < spans[1][1][0]
    g1, g2 = r.group(6), r.group(7)
    assert sorted(set(s for *_, s in g2)) == [NOCOVER, HET, HOM] and [s for *_, s in g1] == [HOM, HOM]
    for tp, tl, _, s in g2:
        assert (s == NOCOVER) == (not any(t0 <= tp and tp + tl <= t1 for t0, t1 in spans[0])), tp
    assert any(spans[0][1][0] <= tp for tp, _, _, s in g2 if s == HET)   # covered by the partner's second segment only
    # alt bytes past 64: the same 70 and 70 that differ in the last
    g1, g2 = r.group(8), r.group(9)
    long1, long2 = [e for e in g1 if len(e[2]) == 70], [e for e in g2 if len(e[2]) == 70]
    assert [(e[0], e[3]) for e in long1] == [(100, HOM), (200, CLASH)] == [(e[0], e[3]) for e in long2]
    assert long1[0][2] == long2[0][2] and long1[1][2][:69] == long2[1][2][:69] and long1[1][2][69] != long2[1][2][69]
    assert sorted(set(state)) == [NOCOVER, HET, CLASH, HOM]


@pytest.mark.gpu
def test_a_derived_batch_of_no_targets(oracle_lib):
    targets = [t for k, t in enumerate(_size_targets()[0]) if k in (2, 5)]
    r = _Run(_whole(targets), 6, 100, 5)
    assert r.tally["split"].tolist() == [0, 0] and r.got == [] and r.dev == [] and r.sup == []
    assert r.calls["state"].size == 0 and r.calls["mate"].size == 0


def _same(a, b):
    assert a.got == b.got and a.dev == b.dev and a.sup == b.sup and a.status == b.status
    assert all(np.array_equal(a.calls[k], b.calls[k]) for k in a.calls)
    assert all(np.array_equal(a.map[k], b.map[k]) for k in a.map)


@pytest.mark.gpu
def test_arena_growth_and_poisoned_buffers(oracle_lib, monkeypatch):
    targets = [t for k, t in enumerate(_size_targets()[0]) if k in (0, 1, 2, 6)]
    ref = _Run(_whole(targets), 6, 100, 5)
    assert ref.reruns == 0 and ref.calls["state"].size > 100
    monkeypatch.setenv("DAGCON_EDITS_CAP", "2")
    grown = _Run(_whole(targets), 6, 100, 5)
    assert grown.reruns > 0
    _same(grown, ref)
    monkeypatch.delenv("DAGCON_EDITS_CAP")
    monkeypatch.setenv("DAGCON_POISON", "15")
    poisoned = _Run(_whole(targets), 6, 100, 5)
    _same(poisoned, ref)
    poisoned.check_twin([bb for bb, _ in targets])


@pytest.mark.gpu
def test_every_way_in_gives_the_same_calls(oracle_lib):
    from pbdagcon_amd import capi
    from util import batch_from_targets
    tes = _tes()
    targets = [t for k, t in enumerate(_size_targets()[0]) if k in (1, 2, 6, 7)]
    strings = tes._strings(targets)
    n = sum(len(recs) for _, recs in targets)
    reverse = (np.arange(n) % 3 == 1).astype(np.uint8)
    as_file, i = [], 0
    for bb, recs in targets:
        as_file.append((bb, [(p, pf.revcomp(q) if reverse[i + k] else q, o) for k, (p, q, o) in enumerate(recs)]))
        i += len(recs)
    plain = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    arr = ct.records_to_arrays(targets); arr["t_blob"] = None
    md = capi.HostMdTags.from_texts([mt.encode(p, q, bb, o) for bb, recs in targets for p, q, o in recs])
    cs = capi.HostCsBatch.from_records([(bb, [(p, len(q), pf.tspan(o), cst.encode(p, q, bb, o)) for p, q, o in recs]) for bb, recs in targets])
    hw = capi.HostWindows(np.arange(len(targets), dtype=np.uint32), np.zeros(len(targets), np.uint32), np.asarray([len(bb) for bb, _ in targets], np.uint32))
    calls = {"plain": lambda c: c.consensus_cigar(plain), "packed": lambda c: c._intake(plain.packed(), None, plain, True),
             "stranded": lambda c: c._intake(capi.HostCigarBatch(reverse=reverse, **ct.records_to_arrays(as_file)), None, None, True),
             "cs": lambda c: c.consensus_cs(cs), "md": lambda c: c.consensus_cigar_md(capi.HostCigarBatch(**arr), md),
             "windows": lambda c: c.consensus_cigar_windows(plain, hw)}
    ref = None
    for kind, call in calls.items():
        r = _Run(call, 6, 100, 5)
        assert r.tally["split"].tolist() == [1, 0, 1, 1], kind
        if ref is None:
            ref = r
            ref.check_twin([bb for bb, _ in targets])
            assert ref.calls["state"].size > 100
        _same(r, ref)
    # a string first batch: the switch is without effect, the derived batch is what it is without it
    sb = batch_from_targets([(len(bb), alns, None) for bb, alns in strings])
    for on in (True, False):
        c = capi.Context(min_cov=6, min_len=100, trim=5, flags=capi.FLAG_BASE_POS)
        try:
            c.set_edits(True); c.set_pileup(*SITES); c.set_site_reads(True); c.set_hap_consensus()
            if on:
                c.set_hap_calls(True)
            c.consensus(sb)
            c.upload_haps(); c.run(); c.sync()
            assert c.fetch() == ref.got
            assert _code(c.edits) == STATE and _code(c.hap_calls) == STATE
        finally:
            c.close()


@pytest.mark.gpu
def test_state_rules(oracle_lib):
    from pbdagcon_amd import capi
    targets = [t for k, t in enumerate(_size_targets()[0]) if k in (1, 2)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    c = capi.Context(min_cov=6, min_len=100, trim=5, flags=capi.FLAG_BASE_POS)
    try:
        assert _code(lambda: c.set_hap_calls(True)) == STATE             # without the edits
        assert _code(c.hap_calls) == STATE
        c.set_edits(True); c.set_hap_calls(True)
        c.set_edits(False)                                               # ... which clears it
        c.set_pileup(*SITES); c.set_site_reads(True); c.set_hap_consensus()
        c.set_edits(True)
        c.consensus_cigar(cb)
        c.upload_haps(); c.run(); c.sync()
        want = c.fetch()
        assert _code(c.edits) == STATE and _code(c.hap_calls) == STATE   # the switch off: the derived batch has no edits, as before
        c.set_hap_calls(True)
        first = c.consensus_cigar(cb)
        assert _code(c.hap_calls) == STATE                               # the first batch
        c.upload_haps()
        assert _code(c.hap_calls) == STATE                               # before the run
        c.run(); c.sync()
        assert _code(c.hap_calls) == STATE                               # before the fetch
        assert c.fetch() == want
        hc = c.hap_calls()
        assert hc["state"].size == c.edits()["t_pos"].size > 100
        assert _code(c.edit_support) == STATE                            # not latched for the first batch: not for the derived one
        c.run(); c.sync()
        assert _code(c.hap_calls) == STATE                               # a run alone drops the results
        assert c.fetch() == want and np.array_equal(c.hap_calls()["state"], hc["state"])
        assert c.consensus_cigar(cb) == first and _code(c.hap_calls) == STATE      # after the next upload
        # edits off at the first upload, on at dagcon_upload_haps: without effect
        c.set_edits(False)
        c.consensus_cigar(cb)
        c.set_edits(True); c.set_hap_calls(True)
        c.upload_haps(); c.run(); c.sync()
        assert c.fetch() == want and _code(c.edits) == STATE and _code(c.hap_calls) == STATE
    finally:
        c.close()
    stop = capi.Context(min_cov=6, min_len=100, trim=5, flags=capi.FLAG_BASE_POS | capi.FLAG_STOP_AFTER_MERGE)
    try:
        stop.set_edits(True); stop.set_hap_calls(True); stop.set_pileup(*SITES); stop.set_site_reads(True); stop.set_hap_consensus()
        stop.upload_cigar(cb); stop.run(); stop.sync(); stop.fetch()
        assert _code(stop.hap_calls) == STATE and _code(stop.upload_haps) == STATE
    finally:
        stop.close()


@pytest.mark.gpu
def test_the_switch_changes_nothing_else(oracle_lib):
    from pbdagcon_amd import capi
    targets = [t for k, t in enumerate(_size_targets()[0]) if k in (0, 1, 2, 7)]
    cb = capi.HostCigarBatch(**ct.records_to_arrays(targets))
    out = []
    for on in (False, True):
        c = capi.Context(min_cov=6, min_len=100, trim=5, flags=capi.FLAG_BASE_POS)
        try:
            c.set_edits(True); c.set_edit_support(True); c.set_pileup(*SITES); c.set_site_reads(True)
            c.set_site_alleles(True); c.set_site_join(True); c.set_hap_consensus()
            if on:
                c.set_hap_calls(True)
            first = c.consensus_cigar(cb, strict=False)
            outs = [c.edits(), c.edit_support(), c.pileup(), c.pileup_sites(), c.site_reads(), c.site_alleles(), c.joined_sites(), c.hap_tally()]
            so = c._segs[1].astype(np.int64)
            outs[0]["c_off"] = outs[0]["c_off"].astype(np.int64) - np.repeat(so, np.diff(outs[0]["edit_begin"].astype(np.int64)))
            c.upload_haps(); c.run(); c.sync()
            out.append((first, outs, c.fetch(), c.hap_map()))
        finally:
            c.close()
    (f0, o0, d0, m0), (f1, o1, d1, m1) = out
    assert f0 == f1 and d0 == d1 and all(np.array_equal(m0[k], m1[k]) for k in m0)
    for a, b in zip(o0, o1):
        assert sorted(a) == sorted(b)
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


def _vcf_from_api(run, names, targets):
    """The file pbdagcon --hap-vcf writes, from the API's arrays of one run over all targets."""
    lines = hct.header([(n, len(bb)) for n, (bb, _) in zip(names, targets)])
    src = run.map["src_target"].tolist()
    at1 = at2 = 0
    flat1 = [(tp, tl, bytes(seq[c:c + cl])) for per in run.first_dev for seq, _, _, ed in per for tp, tl, c, cl in ed]
    for t, (name, (bb, _)) in enumerate(zip(names, targets)):
        n_first = sum(len(ed) for _, _, _, ed in run.first_dev[t])
        if t not in src:
            if not run.first_status[t]:
                lines += hct.unsplit_lines(name, bb, flat1[at1:at1 + n_first], [(x[2], x[4], x[3]) for x in run.first_sup[at1:at1 + n_first]])
        else:
            d = src.index(t)
            g = [run.group(d), run.group(d + 1)]
            n = [len(g[0]), len(g[1])]
            sup = [[(x[2], x[4], x[3]) for x in run.sup[at2:at2 + n[0]]], [(x[2], x[4], x[3]) for x in run.sup[at2 + n[0]:at2 + n[0] + n[1]]]]
            mate = run.calls["mate"][at2:at2 + n[0] + n[1]].tolist()
            c1 = [(e[3], None if m == NONE else m - at2 - n[0]) for e, m in zip(g[0], mate[:n[0]])]
            c2 = [(e[3], None if m == NONE else m - at2) for e, m in zip(g[1], mate[n[0]:])]
            lines += hct.split_lines(name, bb, [e[:3] for e in g[0]], sup[0], c1, [e[:3] for e in g[1]], sup[1], c2)
            at2 += n[0] + n[1]
        at1 += n_first
    return lines


@pytest.mark.gpu
def test_pbdagcon_hap_vcf(oracle_lib, tmp_path):
    import bam_files as bf
    all_targets = _size_targets()[0]
    targets = [all_targets[k] for k in (1, 2, 6, 7)]                     # four small targets, one unsplit
    names = ["ctg%d" % i for i in range(4)]
    tl = [len(bb) for bb, _ in targets]
    r = _Run(_whole(targets), 6, 100, 5)
    assert r.tally["split"].tolist() == [1, 0, 1, 1]
    want = _vcf_from_api(r, names, targets)
    body = [ln for ln in want if not ln.startswith("#")]
    assert len(body) > 100 and {ln.split("\t")[7].split(";")[0] for ln in body} == {"PAIR=UNSPLIT", "PAIR=HET", "PAIR=HOM", "PAIR=CLASH", "PAIR=NOCOV"}
    ref = tmp_path / "ref.fa"; ref.write_bytes(ct.to_fasta(names, [bb for bb, _ in targets]))
    sam = tmp_path / "in.sam"; sam.write_bytes(ct.to_sam(names, tl, [rs for _, rs in targets]))
    bam = tmp_path / "in.bam"
    bam.write_bytes(bf.bgzf(bf.bam_bytes(list(zip(names, tl)), [dict(qname="q%d_%d" % (g, k), ref=g, pos=p, ops=o, seq=q, flag=0)
                                                               for g, (_, recs) in enumerate(targets) for k, (p, q, o) in enumerate(recs)])))
    paf = tmp_path / "in.paf"
    paf.write_text("".join("q%d_%d\t%d\t0\t%d\t+\t%s\t%d\t%d\t%d\t0\t0\t60\tcs:Z:%s\n" % (
        g, k, len(q), len(q), names[g], len(bb), p - 1, p - 1 + pf.tspan(o), cst.encode(p, q, bb, o).decode())
        for g, (bb, recs) in enumerate(targets) for k, (p, q, o) in enumerate(recs)))
    base = [_cli(), "--ref", str(ref), "-c", "6", "-m", "100", "-t", "5"]

    def run(*args):
        x = subprocess.run(base + list(args), capture_output=True, timeout=300)
        assert x.returncode == 0, x.stderr.decode()
        return x
    f = {k: tmp_path / k for k in ("F", "G", "V", "G0", "V0", "Fb", "Fc", "Fj")}
    plain = run("--sam", "--hap-consensus", str(f["G0"]), "--vcf", str(f["V0"]), str(sam))
    got = run("--sam", "--hap-vcf", str(f["F"]), "--hap-consensus", str(f["G"]), "--vcf", str(f["V"]), str(sam))
    assert f["F"].read_text().splitlines() == want
    assert got.stdout == plain.stdout and got.stdout.count(b">") >= 4
    assert f["G"].read_bytes() == f["G0"].read_bytes() and f["V"].read_bytes() == f["V0"].read_bytes() and f["G"].stat().st_size > 1000
    run("--bam", "--hap-vcf", str(f["Fb"]), str(bam))
    run("--paf", "--cs", "--hap-vcf", str(f["Fc"]), str(paf))
    assert f["Fb"].read_bytes() == f["F"].read_bytes() == f["Fc"].read_bytes()
    got = run("--sam", "--hap-vcf", str(f["Fj"]), "-j", "2", "--batch-targets", "2", str(sam))
    assert f["Fj"].read_bytes() == f["F"].read_bytes() and got.stdout == plain.stdout
