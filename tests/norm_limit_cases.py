"""Inputs and the model for test_norm_limits.py: alignments built to cross one fixed size of the normalize stage each,
and tests/native/norm_stage_host.cpp, which runs the stage's own text on the CPU and says which route every chunk takes.

An alignment is (start, q, t); a model batch adds each alignment's tlen.  Columns are put together from norm_cases.plain
(matches without equal neighbours: nothing slides through them, and every window of 512 starts a chunk on its first
column) and a few constructions that make columns move or windows lose their start on purpose."""
import os
import struct
import subprocess

import numpy as np

from norm_cases import plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "norm_stage_host.cpp")
NCH = 512                  # DG_NCH: input columns per window
P2_REFILL = 480            # dg_norm_run<512> refills while (e - i) + 32 <= 512
PASS_COLS = 1024           # k_norm_finish2: 64 lanes x DG_FIN_NP 2 pieces x 8 columns a pass
FLOOR = 1 << 20            # the re-run region's least size, columns
GAP = 0x2D


def build_program(out_dir):
    exe = os.path.join(str(out_dir), "norm_stage_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


# ---- the model ---------------------------------------------------------------------------------------------------------

def blob_of(alns):
    """The strings one behind the other, as util.batch_from_targets and Context.normalize lay them out."""
    offs, pos = [], 0
    for _, q, _ in alns:
        offs.append(pos)
        pos += len(q)
    return b"".join(a[1] for a in alns), b"".join(a[2] for a in alns), offs


def model_batch(alns, tlens, trim=0, emit_shift=9, shared=None):
    """One batch for run_model.  shared = (qblob, tblob, offs): the alignments share strings (dagcon_upload_haps)."""
    if shared is None:
        qb, tb, offs = blob_of(alns)
    else:
        qb, tb, offs = shared
    assert len(qb) == len(tb)
    rec = struct.pack("<5I", len(alns), trim, emit_shift, 0 if shared is None else 1, len(qb)) + qb + tb
    for (s, q, t), tl, off in zip(alns, tlens, offs):
        assert len(q) == len(t) and qb[off:off + len(q)] == q and tb[off:off + len(q)] == t
        rec += struct.pack("<4I", off, len(q), s, tl)
    return rec


def _pairs(fields):
    return {} if fields == ["."] else {int(a): int(b) for a, b in (f.split(":") for f in fields)}


def run_model(exe, tmp_path, batches, name="stage"):
    """-> per batch {"B": {...}, "alns": [{"W": [window dicts], "F": [chunk dicts], "A": {...}, "q", "t", "C", "K"}]}"""
    path = os.path.join(str(tmp_path), name + ".bin")
    with open(path, "wb") as f:
        for b in batches:
            f.write(b)
    out = subprocess.run([exe, "stage", path], capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-4000:]
    res = [{"B": None, "alns": []} for _ in batches]

    def aln(bi, a):
        al = res[bi]["alns"]
        while len(al) <= a:
            al.append({"W": [], "F": [], "A": None, "q": None, "t": None, "C": None, "K": None})
        return al[a]
    for ln in out.stdout.decode().split("\n"):
        if not ln:
            continue
        f = ln.split(" ")
        bi, tag = int(f[0]), f[1]
        if tag == "B":
            res[bi]["B"] = dict(zip(("tmp_main", "tmp_cap", "region", "ovf_top"), map(int, f[2:])))
            continue
        r = aln(bi, int(f[2]))
        if tag == "W":
            r["W"].append({"c": int(f[3]), "k0": int(f[4]), "route": f[5], "reruns": int(f[6]), "next": int(f[7]), "w": int(f[8]),
                           "tb": int(f[9]), "span": int(f[10]), "wraps": int(f[11]), "asked": int(f[12])})
        elif tag == "F":
            r["F"].append(dict(zip(("c", "o", "w", "passes", "h", "nb", "carried", "ck_first", "ck_lane0"), map(int, f[3:]))))
        elif tag == "A":
            r["A"] = {"slow": f[3] == "1", "lo": int(f[4]), "hi": int(f[5]), "start": int(f[6]), "n_lb": int(f[7]), "m": int(f[8]),
                      "branches": "" if f[9] == "-" else f[9], "n_ins": int(f[10]), "n_del": int(f[11]), "nonconf": f[12] == "1"}
        elif tag in ("Q", "T"):
            r[tag.lower()] = b"" if f[3] == "." else f[3].encode()
        else:
            r[tag] = _pairs(f[3:])
    return res


def chunks_of(r):
    """The windows of a model alignment that k_norm_scan keeps: a start, and not swallowed by the chunk in front."""
    kept = {f["c"] for f in r["F"]}
    return [w for w in r["W"] if w["c"] in kept]


def routes_of(r):
    """The routes of the chunks that make up the result (every window with a start when the alignment goes slow)."""
    if r["A"]["slow"]:
        out, c = [], 0
        ws = r["W"]
        while c < len(ws):
            if ws[c]["k0"] < 0:
                c += 1
                continue
            out.append(ws[c]["route"])
            c = max(ws[c]["next"], c + 1)
        return out
    return [w["route"] for w in chunks_of(r)]


def finish_literal(qn, tn, start, trim, tlen, emit_shift):
    """dg_finish_alignment (k_build.hip.h), literally, on the normalised columns of an alignment:
    lo, hi, start, {position: run}, {slot: column}, n_ins, n_del, conforming."""
    m = len(qn)
    lb = rb = lo = 0
    hi = m
    while lb < trim and lo < m:
        if tn[lo] != GAP:
            lb += 1
        lo += 1
    while rb < trim and hi > lo:
        hi -= 1
        if tn[hi] != GAP:
            rb += 1
    start += lb
    cells, ck = {}, {}
    n_ins = n_del = adv = run = 0
    conf = start >= 1
    mask = (1 << emit_shift) - 1
    for i in range(lo, hi):
        qb, tb = qn[i], tn[i]
        if qb == tb or qb == GAP:
            if conf and ((start + adv) & mask) == 0 and start + adv <= tlen + 1:
                ck[(start + adv) >> emit_shift] = i - run
            if run:
                if conf and start + adv <= tlen + 1:
                    cells[start + adv] = run
                run = 0
            adv += 1
            n_del += qb != tb
            if start - 1 + adv > tlen:
                conf = False
        elif tb == GAP:
            n_ins += 1
            run += 1
    if run and conf and ((start + adv) & mask) == 0 and start + adv <= tlen + 1:
        ck[(start + adv) >> emit_shift] = hi - run
    if run and conf and start + adv <= tlen + 1:
        cells[start + adv] = run
    return lo, hi, start, cells, ck, n_ins, n_del, (conf or hi == lo)


def check_model(oracle, r, aln, tlen, trim, emit_shift, what=""):
    """The model is checked itself before it is believed: its columns against the oracle's, its runs and checkpoints
    against the literal loop.  Nothing is compared for an alignment the model sends to the slow path."""
    if r["A"]["slow"]:
        return None
    s, q, t = aln
    qn, tn = oracle.normalize_gaps(q, t)
    eq, et, es = oracle.trim_aln(qn, tn, s, trim)
    A = r["A"]
    assert (r["q"], r["t"], A["start"]) == (eq, et, es), f"{what}: the model's columns differ from the oracle's"
    lo, hi, st, cells, ck, n_ins, n_del, conf = finish_literal(qn, tn, s, trim, tlen, emit_shift)
    assert (A["lo"], A["hi"], A["m"]) == (lo, hi, len(qn)), f"{what}: window {A['lo']}..{A['hi']} of {A['m']}, literal {lo}..{hi} of {len(qn)}"
    assert r["C"] == cells, f"{what}: insertion runs"
    assert r["K"] == ck, f"{what}: checkpoints"
    assert (A["n_ins"], A["n_del"], A["nonconf"]) == (n_ins, n_del, not conf), f"{what}: totals"
    return cells


def long_runs(oracle, alns, trim, tlens):
    """Does a read of the batch hold an insertion run a byte cell cannot hold (the device then runs again with wide cells)."""
    for (s, q, t), tl in zip(alns, tlens):
        qn, tn = oracle.normalize_gaps(q, t)
        cells = finish_literal(qn, tn, s, trim, tl, 9)[3]
        if cells and max(cells.values()) > 255:
            return True
    return False


# ---- building blocks -----------------------------------------------------------------------------------------------------

def _other(*avoid):
    return next(c for c in b"ACGT" if c not in avoid)


class Cols:
    """An alignment under construction: q and t grow side by side; `bb` collects the target's bases."""

    def __init__(self, rng):
        self.rng, self.q, self.t = rng, bytearray(), bytearray()

    def __len__(self):
        return len(self.q)

    def last(self):
        for c in reversed(self.t):
            if c != GAP:
                return c
        return None

    def plain(self, n, avoid=None):
        s = plain(self.rng, n, avoid=self.last() if avoid is None else avoid)
        self.q += s; self.t += s
        return self

    def plain_to(self, col):
        assert col >= len(self.q), (col, len(self.q))
        return self.plain(col - len(self.q))

    def match(self, s):
        self.q += s; self.t += s
        return self

    def ins(self, s):
        self.q += s; self.t += b"-" * len(s)
        return self

    def dele(self, s):
        self.q += b"-" * len(s); self.t += s
        return self

    def ins_run(self, n):
        """n inserted bases that stay where they are, and the matching column behind them: two letters in turn, neither
        the base in front nor the one behind."""
        nxt = _other(self.last())
        two = [c for c in b"ACGT" if c not in (self.last(), nxt)][:2]
        return self.ins(bytes(two[k & 1] for k in range(n))).match(bytes([nxt]))

    def del_run(self, n):
        """n deleted target bases that stay where they are, and the matching column behind them: three letters in turn,
        none of them the base behind the run, the first not the base in front."""
        nxt = _other(self.last())
        three = [c for c in b"ACGT" if c != nxt]
        while three[0] == self.last():
            three = three[1:] + three[:1]
        return self.dele(bytes(three[k % 3] for k in range(n))).match(bytes([nxt]))

    def slide_run(self, n, in_q=False):
        """norm_cases.pieces' sliding run: n gap columns in front of 48 columns of the same base, which they move through."""
        b = _other(self.last())
        (self.dele if in_q else self.ins)(bytes([b]) * n)
        return self.match(bytes([b]) * 48)

    def homopolymer(self, n):
        """n matching columns of one base (no chunk starts inside a homopolymer)."""
        b = _other(self.last())
        return self.match(bytes([b]) * n)

    def mismatches(self, n):
        """n columns, match and mismatch in turn (no three matches in a row: no chunk start), nothing slides: the read's
        base differs from the target's bases at, in front of and behind the column."""
        s = plain(self.rng, n + 1, avoid=self.last())
        for k in range(n):
            if k & 1:
                self.q.append(_other(s[k - 1], s[k], s[k + 1])); self.t.append(s[k])
            else:
                self.q.append(s[k]); self.t.append(s[k])
        return self

    def hop(self, reps, in_q=False, tail=True):
        """norm_cases.pieces' hop-over: G, AC inserted, (AC) x reps, T -- the two gaps travel to the end of the repeat."""
        self.match(b"G" if self.last() != ord("G") else b"TG")
        (self.dele if in_q else self.ins)(b"AC")
        self.match(b"AC" * reps)
        if tail:
            self.match(b"T")
        return self

    def aln(self, start=1):
        return start, bytes(self.q), bytes(self.t)

    def tbases(self):
        return bytes(c for c in self.t if c != GAP)


def tlen_of(aln):
    s, _, t = aln
    return s - 1 + sum(1 for c in t if c not in (GAP, 0x2E))


# ---- families --------------------------------------------------------------------------------------------------------------

class Family:
    """targets = [(tlen, [(start, q, t)], names)]: one batch; the alignments one behind the other are the model's batch and
    the argument of Context.normalize."""

    def __init__(self, name, trims=(0,), shifts=(9,)):
        self.name, self.targets, self.trims, self.shifts = name, [], tuple(trims), tuple(shifts)

    def target(self, alns, names, tlen=None):
        assert len(alns) == len(names)
        self.targets.append((max(tlen_of(a) for a in alns) if tlen is None else tlen, list(alns), list(names)))
        return self

    @property
    def alns(self):
        return [a for _, al, _ in self.targets for a in al]

    @property
    def names(self):
        return [n for _, _, nm in self.targets for n in nm]

    @property
    def tlens(self):
        return [tl for tl, al, _ in self.targets for _ in al]

    def index(self, name):
        return self.names.index(name)

    def batch(self):
        from util import batch_from_targets
        return batch_from_targets([(tl, al, None) for tl, al, _ in self.targets])

    def model(self, trim, shift=9):
        return model_batch(self.alns, self.tlens, trim, shift)


def _pad16(c):
    """The alignment's length a multiple of 16: the next one's strings begin on a 16-byte boundary again."""
    return c.plain(-len(c) % 16)


def starts():
    """Windows with and without a chunk start.  Measured on the model (k0 per window, -1: none):
      one / two / three empty windows (homopolymer)   [0, -1, 1024 ..] / [0, -1, -1, 1536 ..] / [0, -1, -1, -1, 2048 ..]
      empty by alternating mismatches                  [0, -1, 1028]: the chunk of window 0 is 1,286 columns, first pass
      empty by a gap run of 530 columns, in t / in q   [0, -1, 1037]: chunk 0 is too long a look-up for both passes, the
                                                       alignment goes to the slow path (and, in t, asks for wide cells)
      last window empty                                [0, 512, -1]
      a start on a window's last column                [0, 1023, 1024]; on its first: every plain window
      lengths 1, 2, 3, 511, 512, 513, 1024, 1025      1, 1, 1, 1, 1, 2 (w = 1), 2, 3 windows (w = 1)
      16 copies of a 1,024-column alignment behind alignments of 1 .. 15 columns: all 16 byte phases of the strings."""
    rng = np.random.default_rng(9001)
    f = Family("starts", trims=(0, 3))
    alns, names = [], []

    def add(name, c, start=1):
        alns.append(c.aln(start)); names.append(name)
    for n in (1, 2, 3):
        add(f"{n} empty", Cols(rng).plain(511).homopolymer(NCH * n + 1).plain(700))
    add("empty by mismatches", Cols(rng).plain(510).mismatches(517).plain(400))
    add("empty by insertion", Cols(rng).plain(505).ins_run(530).plain(500))
    add("empty by deletion", Cols(rng).plain(505).del_run(530).plain(500))
    add("last empty", Cols(rng).plain(1023).homopolymer(400))
    add("start on last column", Cols(rng).plain(511).homopolymer(512).plain(600))
    add("column 0 gap in q", Cols(rng).dele(b"G").plain(600, avoid=ord("G")))
    add("column 0 gap in t", Cols(rng).ins(b"G").plain(600, avoid=ord("G")))
    f.target(alns, names)
    alns, names = [], []
    for n in (1, 2, 3, 511, 512, 513, 1024, 1025):
        c = Cols(rng).plain(n)
        if n >= 3:
            c.q[n // 3] = GAP
        add(f"length {n}", c)
    f.target(alns, names)
    alns, names = [], []
    for k in range(16):
        if k:
            c = Cols(rng).plain(k)
            if k >= 3:
                c.t[1] = GAP
            add(f"short {k}", c)
        add(f"phase copy {k}", Cols(rng).plain(300).ins_run(3).plain_to(511).homopolymer(512).plain(1))
    f.target(alns, names)
    return f


WINDOW64_RUNS = (24, 33, 40, 64)


def window64():
    """Runs of 24, 33, 40 and 64 gap columns, staying and sliding, in t and in q, beginning on a refill boundary (column 96 of
    strings that begin on a 16-byte boundary) and ending three columns in front of the chunk start at column 512.
    A staying run's route goes by the phase of its first column in the 16 columns of a refill, so staying runs of 33 and 40
    also begin on every column 96 .. 111 ("phase k").
    Measured on the model: 24 first pass everywhere; 64, and 33 and 40 that slide, second pass everywhere.  Staying 40:
    first pass at the phases 0 .. 7 (the refill boundary and the chunk-edge placement among them), second pass at 8 .. 15,
    in t and in q alike.  Staying 33: second pass at phase 15 alone.  Staying runs of 48 and more never fit the first
    pass (the window reaches 48 columns from the output cursor)."""
    rng = np.random.default_rng(9002)
    f = Family("window64", trims=(0, 5))
    alns, names = [], []
    for L in WINDOW64_RUNS:
        for in_q in (False, True):
            for slide in (False, True):
                for edge in (False, True):
                    c = Cols(rng)
                    c.plain_to((NCH - 2 - L - (48 if slide else 0)) if edge else 96)
                    if slide:
                        c.slide_run(L, in_q)
                    elif in_q:
                        c.del_run(L)
                    else:
                        c.ins_run(L)
                    c.plain(640 - len(c) if len(c) < 640 else 16)
                    alns.append(_pad16(c).aln())
                    names.append(f"run {L} in {'q' if in_q else 't'}, {'slides' if slide else 'stays'}, {'chunk edge' if edge else 'refill'}")
    for L in (33, 40):
        for in_q in (False, True):
            for k in range(16):
                c = Cols(rng).plain_to(96 + k)
                (c.del_run if in_q else c.ins_run)(L)
                alns.append(_pad16(c.plain_to(640)).aln())
                names.append(f"run {L} in {'q' if in_q else 't'}, stays, phase {k}")
    f.target(alns, names)
    return f


W512_BELOW, W512_ABOVE = (300, 400), (520, 600)
W512_BOUND = P2_REFILL - 1          # a staying run of L columns asks for e - i = L + 1 (plain_need in norm_stage_host.cpp)
W512_AROUND = (W512_BOUND - 16, W512_BOUND - 1, W512_BOUND, W512_BOUND + 1, W512_BOUND + 16)


def window512():
    """Staying gap runs around the second pass's bound, in t and in q, the run's first column on a refill boundary (column 96)
    and 9 columns behind one (105); and two second-pass chunks whose 512-column ring comes round once and twice.
    Measured on the model (the same in t and in q; route, largest e - i at column 96 / 105):
      300  second pass 304 / 311      400  second pass 416 / 407      463  second pass 464 / 465
      478  second pass 480 / 480      479  second pass 480 / 481      480  second pass 482 / 482
      495  second pass 496 at column 96, slow by window at 105 (487)  520, 600  slow by window (496 / 487)
    479 and below are second pass by plain_need <= 480, 496 and above can never be; 480 and 495 are recorded.
    "wraps once": a sliding run of 40 in front of 80 mismatches in chunk 0 (582 columns): second pass, ring round once, no
    re-run.  "wraps twice": the same with a hop-over across the chunk starts at 512 and 1,024: second pass, 2 re-runs,
    5,040 columns of the re-run region, one chunk of 1,528 columns, ring round twice."""
    rng = np.random.default_rng(9003)
    f = Family("window512", trims=(0, 5))
    alns, names = [], []
    for L in W512_BELOW + W512_AROUND + W512_ABOVE:
        for in_q in (False, True):
            for col in (96, 105):
                c = Cols(rng).plain_to(col - 1)          # (the run's first column is `col`: ins_run / del_run put a column behind it)
                c.plain(1)
                (c.del_run if in_q else c.ins_run)(L)
                alns.append(_pad16(c.plain(700)).aln())
                names.append(f"run {L} in {'q' if in_q else 't'} at {col}")
    c = Cols(rng).plain(16).slide_run(40)
    for _ in range(80):
        c.plain(4).mismatches(2)
    alns.append(_pad16(c.plain_to(700)).aln()); names.append("wraps once")
    c = Cols(rng).plain(16).slide_run(40)
    for _ in range(40):
        c.plain(4).mismatches(2)
    c.hop(420).plain(300)
    alns.append(_pad16(c).aln()); names.append("wraps twice")
    # (sixteen plain reads: the first guesses of the vertex and the pool arena go by the input columns, and with them they hold
    # the 8,000 inserted bases of the runs above -- the batch runs again for the wide cells only: test_norm_limits.py,
    # test_no_family_runs_again_for_an_arena)
    for k in range(16):
        alns.append(_pad16(Cols(rng).plain(1400)).aln()); names.append(f"plain {k}")
    f.target(alns, names)
    return f


def reruns():
    """norm_cases.pieces' hop-over (AC inserted in front of an (AC) repeat: two gaps travel to its end) across chunk starts.
    Measured on the model, chunk 0 of each: across 1 / 2 / 6 starts: 1 / 2 / 6 re-runs, next = 2 / 3 / 7; across an empty
    window: 1 re-run that takes windows 1 and 2 in (next = 3); ending on len: 2 re-runs, k2 = len; two dirty chunks with a
    clean one between: chunks 0 and 3 with one re-run each, chunk 2 with none."""
    rng = np.random.default_rng(9004)
    f = Family("reruns", trims=(0, 5))
    alns, names = [], []
    for n in (1, 2, 6):
        for in_q in (False, True):
            alns.append(Cols(rng).plain(300).hop(106 + 256 * n - 50, in_q).plain(300).aln())      # the repeat ends 100 columns behind the n-th start
            names.append(f"across {n} in {'q' if in_q else 't'}")
    alns.append(Cols(rng).plain(300).hop(150).plain_to(1023).homopolymer(513).plain(300).aln()); names.append("across an empty window")
    alns.append(Cols(rng).plain(300).hop(400, tail=False).aln()); names.append("ends on len")
    alns.append(Cols(rng).plain(300).hop(150).plain_to(1800).hop(200).plain(300).aln()); names.append("two dirty chunks")
    f.target(alns, names)
    return f


def reruns_short(rng, k):
    """Three short alignments of the reruns kind."""
    return [Cols(rng).plain(300 + 16 * j).hop(150 + 8 * k).plain(200).aln() for j in range(3)]


def scratch_aln(n):
    """G, AC inserted, (AC) x n, T: chunk 0 runs again with one more window taken in at every one of the repeat's starts."""
    c = Cols(np.random.default_rng(9005)).hop(n)
    return c.plain(60).aln()


def trim_alns():
    """Alignments for the trims: plain with short indels; with swallowed windows (a hop-over across two starts in front of a
    short tail chunk); with empty windows at both ends; with a chunk that ends in insertion columns."""
    rng = np.random.default_rng(9006)
    c = Cols(rng)
    for _ in range(14):
        c.plain(70).ins_run(2).plain(60).del_run(3)
    plain_a = c.plain(40).aln(7)
    swallowed = Cols(rng).plain(200).hop(500).plain(400).aln(3)
    c = Cols(rng).plain(511).homopolymer(513).plain(400).ins_run(5).plain_to(2047).homopolymer(500)
    empty = c.aln(1)
    # chunk 0 ends in the two insertion columns that travelled to the repeat's end, column 511: at trim = its tb the left end
    # stops in front of them (`lbases + tb < trim`, not `<=`: the whole chunk would take them along)
    ends_in_run = Cols(rng).plain(200).hop(154, tail=False)
    assert len(ends_in_run) == NCH
    ends_in_run = ends_in_run.match(b"G").plain(699).aln(5)           # (G: neither travelling base finds its like behind the repeat)
    return [plain_a, swallowed, empty, ends_in_run], ["plain", "swallowed", "empty ends", "ends in a run"]


FIN_RUNS = (1, 8, 16, 255)
FIN_EDGES = (1024, 2048, 3072)
FIN_REP0, FIN_NREP = 101, 1650             # the (AC) repeat of the finish backbone: columns 101 .. 3,400 (into window 6)


def _finish_backbone(rng):
    left = plain(rng, 100)
    left = left[:-1] + (b"T" if left[-2] != ord("T") else b"C")
    bb = left + b"G" + b"AC" * FIN_NREP + b"T"
    return bb + plain(rng, 3700 - len(bb), avoid=ord("T"))


def _finish_read(bb, hop_at, runs=(), first=0, last=None, mism=()):
    """bb[first:last] base for base, AC inserted in front of target base hop_at (inside the repeat, in its phase; None: not),
    a run of n columns of G / T, which stays where it is, in front of target base i for (i, n) of runs, and another base
    than the target's (and its neighbours') at the target bases `mism`: two columns each once normalised."""
    last = len(bb) if last is None else last
    runs = dict(runs)
    q, t = bytearray(), bytearray()
    for i in range(first, last):
        if i in runs:
            n = runs[i]
            q += bytes(b"GT"[k & 1] for k in range(n)); t += b"-" * n
        if i == hop_at:
            assert bb[i:i + 2] == b"AC"
            q += b"AC"; t += b"--"
        q.append(_other(bb[i - 1], bb[i], bb[i + 1]) if i in mism else bb[i]); t.append(bb[i])
    return first + 1, bytes(q), bytes(t)


def ins_runs(q, t):
    """[(first column, length)] of the insertion runs of a normalised alignment."""
    out, k = [], 0
    while k < len(q):
        if t[k] == GAP and q[k] != GAP:
            s = k
            while k < len(q) and t[k] == GAP and q[k] != GAP:
                k += 1
            out.append((s, k - s))
        else:
            k += 1
    return out


def finish():
    """k_norm_finish2's passes, copy and events.  Returns the family and `want`: per name the (first column, length) runs the
    read has to show once normalised (checked against the oracle by the test).
    Measured on the model: chunks of 1, 2, 3 and 4 passes from the hop-overs at columns 3,101 / 2,601 / 1,601 / 601 (0, 1, 3, 5
    windows taken in, 514 / 1,026 / 2,050 / 3,074 columns); the edge reads are one chunk from column 0 of 3,586 + runs columns, 4 or 5 passes."""
    rng = np.random.default_rng(9007)
    bb = _finish_backbone(rng)
    f = Family("finish", trims=(0, 7, 1100), shifts=(9, 4))
    want = {}
    alns, names = [], []
    for hop_at, taken in ((3101, 0), (2601, 1), (1601, 3), (601, 5)):
        # (two mismatches behind the repeat, in the chunk's last window: 512 x (taken + 1) + 2 columns, one pass more than 1,024 x passes)
        alns.append(_finish_read(bb, hop_at, mism=(3450, 3460))); names.append(f"takes {taken} in")
    # insertion runs that end on, straddle and begin on columns 1,024, 2,048 and 3,072 of the chunk that begins at column 0
    for n in FIN_RUNS + (256, 300):
        for kind in ("ends on", "straddles", "begins on"):
            if n == 1 and kind == "straddles":
                continue
            cols, runs, before = [], [], 0
            for e in FIN_EDGES:
                s = e - n if kind == "ends on" else e - n // 2 if kind == "straddles" else e
                cols.append((s, n)); runs.append((s - before - 2, n)); before += n      # (the two travelling gaps jump over the run: it keeps its input column)
            name = f"runs of {n} {kind} the pass edges"
            alns.append(_finish_read(bb, FIN_REP0, runs)); names.append(name); want[name] = cols
    f.target(alns[:16], names[:16], 3700).target(alns[16:], names[16:], 3700)
    # deletion runs across the same edges: a travelling deletion (AC deleted in front of the repeat) through stretches of G / T
    # in the target that the read does not have
    for rot in range(3):
        kinds = [("ends on", 9), ("straddles", 16), ("begins on", 8)]
        kinds = kinds[rot:] + kinds[:rot]
        t_all = bytearray(bb)
        dels = []
        for e, (kind, d) in zip(FIN_EDGES, kinds):
            s = e - d if kind == "ends on" else e - d // 2 if kind == "straddles" else e
            s -= s & 1                                     # (whole AC pairs are replaced: the repeat goes on in phase behind the stretch)
            s += 1
            t_all[s:s + d + (d & 1)] = bytes(b"GT"[k & 1] for k in range(d + (d & 1)))
            dels.append((s, d + (d & 1)))
        tb = bytes(t_all)
        reads = []
        for r in range(3):
            q, t = bytearray(), bytearray()
            for i in range(len(tb)):
                if i == FIN_REP0:
                    q += b"--"; t += b"AC"
                if any(s <= i < s + d for s, d in dels):
                    q.append(GAP)
                else:
                    q.append(tb[i])
                t.append(tb[i])
            reads.append((1, bytes(q), bytes(t)))
        f.target(reads, [f"deletions {rot}.{r}" for r in range(3)], len(tb) + 2)
    # tail chunks of 1 .. 15 columns at every o & 7, and first reads whose chunk at column 512 begins on a multiple of 16
    small = plain(rng, 600)
    for j0 in (0, 4):
        alns, names = [], []
        for r in range(1, 16):
            for j in range(j0, j0 + 4):
                alns.append(_finish_read(small, None, (), 0, NCH + r, mism=range(10, 10 + 5 * j, 5))); names.append(f"tail {r} at o & 7 = {j}")
        alns.append(_finish_read(small, None, (), 15, 15 + NCH + 40)); names.append(f"chunk start on a checkpoint {j0}")
        f.target(alns, names, 600)
    return f, want


def overrun_target(rng):
    """A target of 1,100 with a read that runs past tlen in its last chunk only (target base 1,101 is column 1,069 of the
    chunk that starts at column 1,024), beside two that fit."""
    bb = plain(rng, 1300)
    c = Cols(rng).match(bb[30:1300])
    return 1100, [(1, bb[:1100], bb[:1100]), (31, bytes(c.q), bytes(c.t)), (1, bb[:900], bb[:900])], ["fits", "past tlen", "fits too"]


def arenas_fit(oracle, fam, trim):
    """The first guesses of the vertex and the pool arena (upload_impl: node_cap = sum_bb + sum_len / 7 + 1024, pool_cap =
    8 node_cap + 80 sum_bb + 1024 T) against what k_carve will ask for (dg_pool_words at growth_pct 100): a batch inside
    both runs again for wide cells only.  -> (vertices, node_cap, pool words, pool_cap)"""
    nodes = pool = sum_bb = 0
    for tl, alns, _ in fam.targets:
        ins = dele = 0
        for s, q, t in alns:
            qn, tn = oracle.normalize_gaps(q, t)
            f = finish_literal(qn, tn, s, trim, tl, 9)
            ins += f[5]; dele += f[6]
        k = len(alns)
        capb = min(k + 2, 12)
        fixed = 3 * ins + (tl + 2) * 3 * capb
        pool += fixed + fixed * 100 // 100 + 3 * (ins + dele + 2 * k) + 64 + 256
        nodes += tl + 2 + ins
        sum_bb += (tl + 2 + 3) & ~3
    node_cap = sum_bb + sum(len(q) for _, q, _ in fam.alns) // 7 + 1024
    return nodes, node_cap, pool, 8 * node_cap + 80 * sum_bb + 1024 * len(fam.targets)
