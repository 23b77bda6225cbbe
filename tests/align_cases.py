"""Pair families for the -a aligner's edge tests (test_align_edges.py), shared by the global flavour (against
oracle.banded_align) and the local one (against align_local_twin.align): tie-dense sequence (homopolymers, tandem
repeats, two letters, no base in common, a repeat with one foreign base, N and lower-case bytes), lengths on the
kernels' own periods (k_align.hip.h: windows of 64 characters, 16 staged rows, 64 path codes), the lengths at which
dg_align_cells steps to the next kernel instance, and block indels that hand a pair from one band to the next."""
import numpy as np

import align_local_twin as twin


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[j] for j in rng.integers(0, len(alphabet), int(n)))


def mutate(rng, t, sub=0.03, ins=0.08, dele=0.05, alphabet=b"ACGT"):
    q = bytearray()
    for c in t:
        u = rng.random()
        if u < dele:
            continue
        q.append(c if u > dele + sub else alphabet[rng.integers(0, len(alphabet))])
        while rng.random() < ins:
            q.append(alphabet[rng.integers(0, len(alphabet))])
    return bytes(q)


def fit(rng, q, n, alphabet=b"ACGT"):
    """q cut or padded (random bases behind it) to exactly n."""
    return q[:n] + rand(rng, max(n - len(q), 0), alphabet)


def mutated_to(rng, t, n, alphabet=b"ACGT", **rates):
    return fit(rng, mutate(rng, t, alphabet=alphabet, **rates), n, alphabet)


def n_lower(rng, t):
    """t with a tenth of its bases N and a tenth lower-case (a != A: the aligner compares bytes)."""
    b = bytearray(t)
    for x in range(len(b)):
        u = rng.random()
        if u < 0.1:
            b[x] = ord("N")
        elif u < 0.2:
            b[x] = b[x] | 0x20
    return bytes(b)


FAMILIES = ("homopolymer", "tandem2", "tandem3", "two_letter", "disjoint", "foreign", "n_lower")


def tie_pair(rng, family, a, b):
    """One pair (q, t) of the family, q of a bases and t of b."""
    L = max(a, b)
    if family == "homopolymer":
        return b"G" * a, b"G" * b
    if family == "tandem2":
        return (b"AC" * L)[:a], (b"AC" * L)[:b]
    if family == "tandem3":
        return (b"CGA" * L)[:a], (b"ACG" * L)[:b]                 # (the two sides start at different phases)
    if family == "two_letter":
        t = rand(rng, b, b"AG")
        return mutated_to(rng, t, a, b"AG", sub=0.05, ins=0.04, dele=0.04), t
    if family == "disjoint":
        return b"A" * a, b"C" * b
    if family == "foreign":
        q = bytearray((b"AC" * L)[:a])
        q[int(rng.integers(0, a))] = ord("G")
        return bytes(q), (b"AC" * L)[:b]
    if family == "n_lower":
        t = n_lower(rng, rand(rng, b))
        q = bytearray(mutated_to(rng, t, a, sub=0.02, ins=0.03, dele=0.03))
        for x in rng.integers(0, a, max(a // 20, 1)):              # the same base in the other case: a mismatch
            q[x] ^= 0x20 if chr(q[x]).upper() in "ACGT" else 0
        return bytes(q), t
    raise ValueError(family)


def tie_pairs_at(rng, L, diffs=(0, 1, 20, 61)):
    """Every family at scale L with the length differences `diffs`, the shorter side alternating -> [(family, q, t)]."""
    out = []
    for f, fam in enumerate(FAMILIES):
        for x, d in enumerate(diffs):
            a, b = (L, L - d) if (f + x) % 2 else (L - d, L)
            out.append((fam, *tie_pair(rng, fam, a, b)))
    return out


def small_tie_pairs(rng):
    """The families on pairs of at most 40 bases a side (the full band holds the whole matrix) -> [(family, q, t)]."""
    out = []
    for n in range(1, 13):                                          # homopolymers: every n, m in 1 .. 12
        for m in range(1, 13):
            out.append(("homopolymer", b"T" * n, b"T" * m))
    for n, m in ((40, 40), (40, 39), (39, 40), (40, 1), (1, 40), (40, 20), (17, 40), (33, 36), (36, 37), (38, 31)):
        out.append(("homopolymer", b"A" * n, b"A" * m))
    for unit in (b"AC", b"GT", b"ACG", b"TTG", b"AAC"):             # tandem repeats, different copy numbers
        for ca in range(1, 14):
            for cb in range(1, 14):
                if (ca + cb) % 3 == 0 or ca == cb or abs(ca - cb) == 1:
                    for ph in (0, 1):                               # (and a side that starts inside the unit)
                        out.append(("tandem", (unit * ca)[ph:][:40], (unit * cb)[:40]))
    for k in range(260):                                            # two letters, random: unrelated and mutated
        ab = (b"AC", b"AT", b"GC")[k % 3]
        t = rand(rng, rng.integers(1, 41), ab)
        q = rand(rng, rng.integers(1, 41), ab) if k % 2 else mutate(rng, t, 0.1, 0.1, 0.1, ab)[:40] or b"A"
        out.append(("two_letter", q, t))
    for k in range(120):                                            # no base in common
        x = int(rng.integers(0, 4))
        q = b"ACGT"[x:x + 1] * int(rng.integers(1, 41))
        t = rand(rng, rng.integers(1, 41), bytes(c for c in b"ACGT" if c != q[0])) if k % 2 else \
            b"ACGT"[(x + 1) % 4:(x + 1) % 4 + 1] * int(rng.integers(1, 41))
        out.append(("disjoint", q, t))
    for unit, n, m in ((b"AC", 24, 24), (b"AC", 31, 27), (b"ACG", 30, 33), (b"A", 20, 22), (b"GT", 40, 38)):
        base = (unit * 40)[:n]
        for p in range(n):                                          # one foreign base, at every position
            f = bytearray(base)
            f[p] = ord("T") if unit != b"GT" else ord("A")
            out.append(("foreign", bytes(f), (unit * 40)[:m]))
            if p % 2:
                out.append(("foreign", (unit * 40)[:m], bytes(f)))
    for k in range(200):                                            # N and lower case
        t = n_lower(rng, rand(rng, rng.integers(1, 41)))
        q = mutate(rng, t, 0.05, 0.08, 0.08)[:40] or b"n"
        if k % 4 == 0:
            q = q.swapcase()
        elif k % 4 == 1:
            q = t.lower()
        out.append(("n_lower", q, t))
    return out


PERIOD_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257)


def window_lengths():
    """Target lengths m with m - W in 63 .. 65 and 127 .. 129, W the first band's half-width of a pair that long: the
    t window's first / second refill then falls where t runs out."""
    out = []
    for m in range(64, 400):
        if m - twin.halfwidth_first(m, m) in (63, 64, 65, 127, 128, 129):
            out.append(m)
    return out


def period_pairs(rng):
    """Lengths on the kernels' periods -> [(q, t)]: n from PERIOD_LENGTHS against m = n - 2 .. n + 2 and against the two
    extremes of the set, q a mutated t cut or padded to n; identical pairs whose path is a multiple of 64 long, or one
    off; targets that end where the t window refills."""
    pairs = []
    for n in PERIOD_LENGTHS:
        for m in sorted({m for m in range(n - 2, n + 3) if m >= 1} | {PERIOD_LENGTHS[0], PERIOD_LENGTHS[-1]}):
            t = rand(rng, m)
            pairs.append((mutated_to(rng, t, n), t))
    for n in (63, 64, 65, 128, 192):
        t = rand(rng, n)
        pairs.append((t, t))
    for m in window_lengths():
        t = rand(rng, m)
        pairs.append((mutated_to(rng, t, m, sub=0.02, ins=0.03, dele=0.03), t))
        pairs.append((mutated_to(rng, t, m - 3, sub=0.02, ins=0.03, dele=0.03), t))
    return pairs


def cells(w):
    """dg_align_cells (k_align.hip.h): cells per lane of the kernel instance that takes a band of half-width w."""
    c = (2 * w + 1 + 63) // 64
    return next(k for k in (2, 4, 6, 8, 12, 16) if c <= k or k == 16)


def instance_steps(width, max_w=twin.MAXW):
    """The smallest L at which each step of dg_align_cells(width(L, L)) is crossed, and the L at which the width
    reaches the cap, for L up to the cap of the full band -> [(L, width at L - 1, width at L)]."""
    out = []
    L = 2
    while True:
        a, b = width(L - 1, L - 1), width(L, L)
        if b > max_w:
            break
        if cells(a) != cells(b) or (b == twin.MAXW and a < b):
            out.append((L, a, b))
        if twin.halfwidth(L, L) == twin.MAXW:
            break
        L += 1
    return out


def block_pair(t, d, swapped):
    """q = t without its middle d bases; swapped: the roles the other way round."""
    h = (len(t) - d) // 2
    q = t[:h] + t[h + d:]
    return (t, q) if swapped else (q, t)
