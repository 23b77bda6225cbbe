"""dagcon_place (k-mer diagonal placement, include/dagcon.h) and the qsense command line's argument handling.

CPU: tests/place_twin.py against a brute-force O(|q||t|) reading of the contract, and qsense's exits that never reach
the device.  GPU: the device against the twin, bit for bit on every output array."""
import os
import subprocess
import sys
import time
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_twin as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


def brute(q: bytes, t: bytes, k=12, max_occ=4):
    """The contract read literally: every (i, j) compared base by base."""
    q, t = q.decode("latin-1"), t.decode("latin-1")

    def kmer(x, i):
        v = 0
        for ch in x[i:i + k]:
            if ch not in CODE:
                return None
            v = v * 4 + CODE[ch]
        return v

    tk = [kmer(t, j) for j in range(len(t) - k + 1)]
    occ = Counter(v for v in tk if v is not None)
    lq, lt = len(q), len(t)
    per = []
    for x in (q, "".join(COMP.get(ch, ch) for ch in reversed(q))):
        votes = []
        for i in range(len(x) - k + 1):
            v = kmer(x, i)
            if v is None or occ[v] > max_occ:
                continue
            votes.extend((i, j) for j in range(len(tk)) if tk[j] == v)
        bins = Counter((j - i + lq) // 64 for i, j in votes)
        V = max(bins.values(), default=0)
        B = min((b for b, n in bins.items() if n == V), default=0)
        per.append((votes, V, B))
    if per[0][1] == 0 and per[1][1] == 0:
        return 0, 0, ".", 0, 0
    s = 0 if per[0][1] >= per[1][1] else 1
    votes, _, B = per[s]
    R = 2 + (lq + 511) // 512
    ends = []
    for quarter in (0, 3):
        c = Counter(b for b in ((j - i + lq) // 64 for i, j in votes if (4 * i) // lq == quarter) if abs(b - B) <= R)
        top = max(c.values(), default=0)
        ends.append(min((b for b, n in c.items() if n == top), default=B) if c else B)
    t0 = min(max(64 * ends[0] + 32 - lq, 0), lt)
    t1 = min(max(64 * ends[1] + 32, 0), lt)
    return per[0][1], per[1][1], "+-"[s], t0, t1


def mutate(rng, x: bytes, err=0.1):
    out = bytearray()
    for b in x:
        u = rng.random()
        if u < err / 3:
            continue
        out.append(b"ACGT"[rng.integers(0, 4)] if u < 2 * err / 3 else b)
        if rng.random() < err / 3:
            out.append(b"ACGT"[rng.integers(0, 4)])
    return bytes(out)


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def adversarial_pairs(rng, scale=1):
    """(q, t, k, max_occ) on the contract's edges."""
    out = []
    t = rand_seq(rng, 300 * scale)
    out.append((t[50:250].replace(b"A", b"N", 3), t, 12, 4))                     # a few Ns
    out.append((t[:100] + b"N" * 40 + t[140:260], t, 12, 4))                     # a run of N
    out.append((t[20:200].lower(), t, 12, 4))                                     # lower case query
    out.append((t[20:200], t.lower(), 12, 4))                                     # lower case target
    rep = rand_seq(rng, 12)
    for occ in (4, 5, 8, 9):                                                      # k-mers at max_occ and max_occ + 1
        tt = bytearray(rand_seq(rng, 400 * scale))
        for m in range(occ):
            tt[30 + 41 * m:42 + 41 * m] = rep
        for mo in (4, 8):
            out.append((rep + bytes(tt[100:180]), bytes(tt), 12, mo))
    out.append((t[:7], t, 8, 4))                                                  # query shorter than k
    out.append((t[:11], t, 12, 4))
    out.append((t, t[:11], 12, 4))                                                # target shorter than k
    out.append((b"", t, 12, 4))
    pal = rand_seq(rng, 30)
    pal += tw.rc(pal)                                                             # its own reverse complement: equal support
    out.append((pal, rand_seq(rng, 40) + pal + rand_seq(rng, 40), 8, 8))
    half = rand_seq(rng, 60)
    out.append((half + tw.rc(half), rand_seq(rng, 30) + half + rand_seq(rng, 50) + half, 12, 4))
    out.append((rand_seq(rng, 900 * scale), t, 12, 4))                            # read longer than the target
    out.append((mutate(rng, t + rand_seq(rng, 200)), t, 12, 4))
    out.append((tw.rc(mutate(rng, t[30:290])), t, 12, 4))                        # '-' strand
    out.append((rand_seq(rng, 300, b"AC"), rand_seq(rng, 300, b"AC"), 8, 8))      # low complexity: many masked
    out.append((t[100:200], t, 16, 1))
    return out


def test_twin_matches_the_contract_read_literally():
    rng = np.random.default_rng(7)
    cases = adversarial_pairs(rng)
    for _ in range(40):
        lt = int(rng.integers(8, 400))
        t = rand_seq(rng, lt, b"ACGT" if rng.random() < 0.7 else b"ACGN")
        if rng.random() < 0.5 and lt > 20:
            a = int(rng.integers(0, lt - 10))
            q = mutate(rng, t[a:a + int(rng.integers(10, 300))], 0.05)
            if rng.random() < 0.5:
                q = tw.rc(q)
        else:
            q = rand_seq(rng, int(rng.integers(0, 300)))
        cases.append((q, t, int(rng.integers(8, 17)), int(rng.integers(1, 9))))
    seen = set()
    for q, t, k, mo in cases:
        exp = brute(q, t, k, mo)
        assert tw.place(q, t, k, mo) == exp, (q, t, k, mo)
        seen.add(exp[2])
    assert seen == {"+", "-", "."}


def test_equal_support_goes_to_plus():
    x = rand_seq(np.random.default_rng(2), 40)
    q = x + tw.rc(x)                                                            # its own reverse complement
    vf, vr, s, _, _ = tw.place(q, b"TTTT" + q + b"GGGG", 12, 4)
    assert vf == vr > 0 and s == "+"
    assert brute(q, b"TTTT" + q + b"GGGG", 12, 4)[:3] == (vf, vr, "+")


def _qsense():
    path = os.path.join(ROOT, "pbdagcon_amd", "bin", "qsense")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "pbdagcon_amd", "csrc"), "all"])
    return path


def test_qsense_usage_and_refusals(tmp_path):
    cli = _qsense()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")       # none of these may get as far as the device
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=60, env=env, cwd=tmp_path)
    h = run("--help")
    assert h.returncode == 0 and "parity unpinned" in h.stdout and "--fofn" in h.stdout and "--min_len" in h.stdout
    assert "not optimized for larger templates" in h.stdout
    assert run().returncode == 2
    assert run("x").returncode == 2
    assert run("d").returncode == 2                                      # input.fasta is required
    assert run("r", "in.fa").returncode == 2                             # and ref.fasta in r mode
    assert run("d", "in.fa", "--bogus").returncode == 2
    assert run("d", "in.fa", "--n_iter", "x").returncode == 2
    fa = tmp_path / "in.fa"
    fa.write_text(">r\nACGT\n")
    for opt in (["--enable_hp_correction"], ["--hp_correction_th", "0.5"], ["--mark_lower_case"], ["--dump_dag_info"]):
        r = run("d", str(fa), *opt)
        assert r.returncode == 2 and opt[0] in r.stderr and "not built" in r.stderr, r.stderr
    r = run("d", str(tmp_path / "missing.fa"))
    assert r.returncode == 1 and "missing.fa" in r.stderr
    r = run("r", str(fa), str(tmp_path / "missing_ref.fa"))
    assert r.returncode == 1 and "missing_ref.fa" in r.stderr
    r = run("d", "--fofn", str(tmp_path / "missing.fofn"))
    assert r.returncode == 1
    bad = tmp_path / "bad.fa"
    bad.write_text("ACGT\n>r\nACGT\n")
    assert run("d", str(bad)).returncode == 1
    assert not list(tmp_path.glob("*.fa.*")) and not (tmp_path / "g_consensus.fa").exists()


# ---------------------------------------------------------------------------------------------------------------- GPU

def _check(got, exp, label):
    for name in ("votes_fwd", "votes_rev", "t0", "t1"):
        bad = np.flatnonzero(np.asarray(got[name]) != np.asarray(exp[name]))
        assert bad.size == 0, (label, name, bad[:10], np.asarray(got[name])[bad[:10]], np.asarray(exp[name])[bad[:10]])
    assert got["strand"] == exp["strand"], label


@pytest.mark.gpu
def test_place_matches_twin_random_and_adversarial(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    rng = np.random.default_rng(11)
    seqs, pairs = [], []
    for _ in range(2000):
        lt = int(np.exp(rng.uniform(np.log(8), np.log(65536))))
        t = rand_seq(rng, lt)
        u = rng.random()
        if u < 0.6:
            a = int(rng.integers(0, lt))
            q = mutate(rng, t[a:a + int(np.exp(rng.uniform(np.log(8), np.log(65536))))], float(rng.uniform(0, 0.2)))
            q = q[:65536] if len(q) >= 8 else q + rand_seq(rng, 8)
            if rng.random() < 0.5:
                q = tw.rc(q)
        else:
            q = rand_seq(rng, int(np.exp(rng.uniform(np.log(8), np.log(65536)))))
        seqs += [q, t]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
    got = ctx.place(seqs, pairs)
    _check(got, tw.place_pairs(seqs, pairs), "random")
    # the adversarial set, by (k, max_occ)
    by = {}
    for q, t, k, mo in adversarial_pairs(rng, scale=3):
        by.setdefault((k, mo), []).append((q, t))
    for (k, mo), qt in by.items():
        s = [x for pr in qt for x in pr]
        p = [(2 * a, 2 * a + 1) for a in range(len(qt))]
        _check(ctx.place(s, p, k=k, max_occ=mo), tw.place_pairs(s, p, k, mo), ("adversarial", k, mo))
    # a target shared by many pairs, the same sequence on both sides of a pair
    t = rand_seq(rng, 20000)
    s = [t] + [mutate(rng, t[a:a + 5000]) for a in range(0, 15000, 1000)]
    p = [(i, 0) for i in range(len(s))] + [(0, i) for i in range(1, len(s))]
    _check(ctx.place(s, p), tw.place_pairs(s, p), "shared")


def _cluster_reads(rng, template, n, err=(0.03, 0.12, 0.06, 0.3)):
    """Reads of both strands with util.random_target's error profile (sub, ins, del, ins_ext), starting in the first
    and ending in the last 5 % of the template."""
    sub, ins, dele, ext = err
    L = len(template)
    reads = []
    for _ in range(n):
        a, b = int(rng.integers(0, L // 20 + 1)), L - int(rng.integers(0, L // 20 + 1))
        out = bytearray()
        for x in template[a:b]:
            u = rng.random()
            if u < dele:
                pass
            elif u < dele + sub:
                out.append(b"ACGT"[rng.integers(0, 4)])
            else:
                out.append(x)
            if rng.random() < ins:
                while True:
                    out.append(b"ACGT"[rng.integers(0, 4)])
                    if rng.random() >= ext:
                        break
        reads.append(bytes(out) if rng.random() < 0.5 else tw.rc(bytes(out)))
    return reads


@pytest.mark.gpu
def test_place_all_against_all_150_reads_of_10kb(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    rng = np.random.default_rng(5)
    reads = _cluster_reads(rng, rand_seq(rng, 10000), 150)
    pairs = [(j, i) for i in range(150) for j in range(150) if j != i]
    t = time.perf_counter()
    got = ctx.place(reads, pairs)
    print(f"dagcon_place: {len(pairs)} pairs of 10 kb in {(time.perf_counter() - t) * 1e3:.1f} ms (first call)")
    # the twin takes milliseconds a pair: every twentieth pair, which covers every target and query
    sample = list(range(0, len(pairs), 20))
    exp = tw.place_pairs(reads, [pairs[a] for a in sample])
    _check({n: (v[sample] if n != "strand" else bytes(v[a] for a in sample)) for n, v in got.items()}, exp, "all-against-all")
    assert (np.maximum(got["votes_fwd"], got["votes_rev"]) >= 3).mean() > 0.95     # they are reads of one template


@pytest.mark.gpu
def test_place_size_limit(gpu_ctx_factory):
    from pbdagcon_amd import capi
    ctx = gpu_ctx_factory()
    rng = np.random.default_rng(3)
    t = rand_seq(rng, capi.PLACE_MAX_LEN)
    got = ctx.place([t[:5000], t], [(0, 1), (1, 0)])                   # at the limit: fine
    assert got["strand"] == b"++"
    with pytest.raises(capi.DagconError) as e:
        ctx.place([t[:5000], t + b"A"], [(0, 1)])
    assert e.value.code == -5
    with pytest.raises(capi.DagconError) as e:
        ctx.place([t + b"A", t[:5000]], [(0, 1)])
    assert e.value.code == -5
    for k, mo in ((7, 4), (17, 4), (12, 0), (12, 9)):
        with pytest.raises(capi.DagconError) as e:
            ctx.place([t[:100], t[:200]], [(0, 1)], k=k, max_occ=mo)
        assert e.value.code == -1
