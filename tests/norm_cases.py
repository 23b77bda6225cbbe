"""Constructed normalizeGaps inputs shared by test_norm_run_host.py and test_norm_gapcols.py."""


def plain(rng, n, avoid=None):
    """n matching columns over ACGT without two equal neighbours (nothing slides through them); the first base
    differs from `avoid`."""
    out = bytearray()
    prev = avoid
    for _ in range(n):
        b = b"ACGT"[rng.integers(0, 4)]
        while b == prev:
            b = b"ACGT"[rng.integers(0, 4)]
        out.append(b)
        prev = b
    return bytes(out)


def pieces(rng):
    """[(name, q, t)]: short stretches of columns that exercise one thing each; every piece starts and ends with a
    column that holds a base in both strings, so it can be set between two plain() stretches."""
    out = []
    for L in (20, 24, 26, 30, 33, 64, 300):
        run = plain(rng, L, avoid=ord("G"))
        out.append((f"run {L} in t", b"G" + run + b"T", b"G" + b"-" * L + b"T"))
        out.append((f"run {L} in q", b"G" + b"-" * L + b"T", b"G" + run + b"T"))
    for L in (24, 33):
        out.append((f"sliding run {L} in t", b"G" + b"A" * (L + 48) + b"T", b"G" + b"-" * L + b"A" * 48 + b"T"))
        out.append((f"sliding run {L} in q", b"G" + b"-" * L + b"A" * 48 + b"T", b"G" + b"A" * (L + 48) + b"T"))
    out.append(("homopolymer 200, insertion", b"G" + b"A" * 201 + b"T", b"G-" + b"A" * 200 + b"T"))
    out.append(("homopolymer 200, deletion", b"G-" + b"A" * 200 + b"T", b"G" + b"A" * 201 + b"T"))
    # I(a) I(b) M(a) M(b): a later gap overtakes through the column an earlier one emptied; 600 repeats carry the gaps
    # through chunk starts (the re-run region)
    for ins, k in ((b"AC", 3), (b"A", 20), (b"CA", 600), (b"ACA", 600)):
        rep = b"AC" * k
        out.append((f"hop-over {ins.decode()} x{k} in t", b"G" + ins + rep + b"T", b"G" + b"-" * len(ins) + rep + b"T"))
        out.append((f"hop-over {ins.decode()} x{k} in q", b"G" + b"-" * len(ins) + rep + b"T", b"G" + ins + rep + b"T"))
    # an insertion directly followed by the equal deletion: (-, -) columns
    for n in (1, 4, 9):
        bq, bt = bytearray(b"G"), bytearray(b"G")
        prev = ord("G")
        for _ in range(n):
            x = plain(rng, 1, avoid=prev)[0]
            bq += bytes([x, 0x2D]); bt += bytes([0x2D, x])
            prev = x
        tail = plain(rng, 1, avoid=prev)
        out.append((f"ins+del burst {n}", bytes(bq) + tail, bytes(bt) + tail))
        out.append((f"del+ins burst {n}", bytes(bt) + tail, bytes(bq) + tail))
    # mismatches side by side
    t = plain(rng, 12)
    q = bytearray(t)
    for o in (3, 4, 5, 9):
        q[o] = b"ACGT"[(b"ACGT".index(t[o]) + 2) % 4]
    out.append(("mismatches", bytes(q), t))
    return out
