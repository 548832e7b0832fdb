"""Constructed pairs for the batch traceback (tb_walk_pair, tb_walk_pair_wave, aln_traceback_expand_kernel); tests/tb_batch_model.py
states the geometry they are aimed at.  Not a test module.

The block notation, the builder and the flank rule (L / 2 + 100 residues around a gap of L where the semantics are local) are those
of tests/tb_single_cases.py; its Case class is imported.  On top of it the residues at both ends of a gap block are chosen so that the
gap cannot slide along its flank (a gap whose first residue equals the first residue after it has two equally good places).  Global
paths are forced, so the window, last-block and thin cases, whose strips are too short for those flanks, are core global; the
cases that have room are core local as well.

Every case names its aim as a dict of predicates over the model's step records (check_aim); GROUP_AIMS are those a whole group has
to meet between its cases.  tests/test_tb_batch_model_cpu.py holds every case to its aim on the oracle's path.

Schemes: "int" BLOSUM62 11 / 2 (the batch fast kernel); "real" BLOSUM62 x 0.37 with 11.3 / 2.1 (aln_fill_f64_kernel); "off" BLOSUM62
with one entry of 33, beyond the fast kernels' int8 profile (the generic integer kernel); "dna" +5 / -4 over four letters, 11 / 2 (the
two-pairs-per-wave kernel's LDS holds 8 rows a lane with 1024 columns only for so small a matrix).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tb_batch_model as bm  # noqa: E402
import tb_single_cases as sc  # noqa: E402
from scheme_limits import FAST_SMAX  # noqa: E402

CORE_GLOBAL, CORE_LOCAL, LEGACY_GLOBAL, LEGACY_LOCAL = sc.CORE_GLOBAL, sc.CORE_LOCAL, sc.LEGACY_GLOBAL, sc.LEGACY_LOCAL
SEMS = (("cg", CORE_GLOBAL), ("cl", CORE_LOCAL), ("lg", LEGACY_GLOBAL), ("ll", LEGACY_LOCAL))
FORBIDDEN = (sc.W, 13, 18, sc.P, sc.G)          # residues a gap's edge never takes: W, F, Y (no_w) and the two prefix letters


def scheme(kind):
    from aligner_amd.matrices import get_blosum62
    b = np.asarray(get_blosum62(), dtype=np.float64)
    if kind == "real":
        return b * 0.37, 11.3, 2.1
    if kind == "dna":
        return np.where(np.eye(4, dtype=bool), 5.0, -4.0), 11.0, 2.0
    if kind == "off":
        b = b.copy()
        i = int(np.argmax(np.diag(b)))
        b[i, i] = FAST_SMAX + 1
        return b, 11.0, 2.0
    return b, 11.0, 2.0


class Case(sc.Case):
    """group: which list of the issue the case belongs to; subset: it also runs on the real-valued and the off-fast-path scheme and
    on the row-major fallback."""

    def __init__(self, group, name, sem, blocks, aim, no_w=False, subset=False, pure=None, kind="int"):
        sc.Case.__init__(self, name, "batch", sem, 0, blocks, aim, no_w)
        self.group, self.subset, self.kind = group, subset, kind
        self.pure = group == "window" if pure is None else pure

    @property
    def id(self):
        return "%s/%s" % (self.group, self.name)

    def seqs(self):
        """The builder's sequences with the gaps made unambiguous.  pure (the window group, whose aims count the steps of a run): a gap
        block is all W (query) or all P (target) and no flank holds W, F, Y or P, so no residue of a gap scores above -1 anywhere and
        the run is one piece.
        Otherwise the residues at both ends of a gap block differ from both flank residues beside it.
        kind "dna" (a 4-letter scheme): the flanks are over codes 0 .. 2 and every gap block is all 3."""
        q, t = sc.Case.seqs(self)
        q, t = q.copy(), t.copy()
        if self.kind == "dna":
            assert self.pure and all(k in ("m", "q", "t") for k, _ in self.blocks)
            q %= 3
            t %= 3
        qi = ti = 0
        for n_blk, (kind, n) in enumerate(self.blocks):
            inner = 0 < n_blk < len(self.blocks) - 1 and self.blocks[n_blk - 1][0] in ("m", "w") and self.blocks[n_blk + 1][0] in ("m", "w")
            if kind in ("q", "t") and self.pure:
                if kind == "q":
                    q[qi:qi + n] = 3 if self.kind == "dna" else sc.W
                else:
                    t[ti:ti + n] = 3 if self.kind == "dna" else sc.P
            elif kind in ("q", "t") and inner:
                s, i = (q, qi) if kind == "q" else (t, ti)
                for pos in (i, i + n - 1):                          # the gap block s[i : i + n] between s[i - 1] and s[i + n]
                    bad = {int(s[i - 1]), int(s[i + n])} | set(FORBIDDEN)
                    s[pos] = min(v for v in range(20) if v not in bad)
            elif kind == "m" and self.pure and self.kind != "dna":
                for s, i in ((q, qi), (t, ti)):
                    blk = s[i:i + n]
                    blk[(blk == sc.W) | (blk == 13) | (blk == 18) | (blk == sc.P)] = 0
            if kind in ("m", "w", "q", "jq", "qW"):
                qi += n
            if kind in ("m", "w", "t", "jt", "tG"):
                ti += n
        return q, t

    def shape(self):
        q, t = self.seqs()
        return len(t), len(q)


def kinds_of(case):
    """The schemes a case runs with.  The legacy semantics are integer only, so their subset cases skip the real-valued scheme."""
    if not case.subset:
        return (case.kind,)
    return ("int", "off") if case.legacy() else ("int", "real", "off")


def oracle(orc, case, kind="int", want_matrices=False):
    q, t = case.seqs()
    S, dele, ext = scheme(kind)
    return orc.align(case.sem, q, t, dele, ext, S, want_matrices=want_matrices)


def moves_of(case, ref):
    return bm.path_from_alignment(case.legacy(), ref["end"], ref["start"], ref["qa"], ref["ta"])


def _q(R):
    return 4 * bm.spb(R)


def _place(M, R, L, kind, want_mod):
    """(a, b, d) of [("m", a), (kind, L), ("m", b)] for a single strip of M rows such that step k of the run's first cell (walk order)
    is want_mod modulo the steps of a quad; d = 0 wherever a placement with flanks of three residues or more reaches it, else 1.  The run's length ties the first cell's
    column to its row (x - y is L or -L less the other flank), so k0 = x - 1 + (y - 1) / R moves in steps of 1 and 2 as a grows and
    skips residues: with R = 1 it is 2 a + L - 2, one parity only; with R = 3 every fourth value is left out."""
    Q = _q(R)
    rows = M - (L if kind == "t" else 0)
    best = None
    for a in sorted(range(3, rows - 2), key=lambda v: abs(v - rows // 2)):
        b = rows - a
        # walk order: b diagonal steps from (M, N), then the run; its first cell is (M - b, N - b)
        y, x = M - b, (a + L if kind == "q" else a)
        k0 = x - 1 + (y - 1) // R
        d = min((k0 - want_mod) % Q, (want_mod - k0) % Q)
        if best is None or d < best[0]:
            best = (d, a, b)
        if d == 0:
            break
    assert best[0] <= 1, (M, R, L, kind, want_mod, best)
    return best[1], best[2], best[0]


def cases():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    # ---- tag counts, all four semantics.  Core global has no pair with 0 tags (both sequences hold a residue), nor has core local:
    for sn, sem in SEMS:
        legacy = sem in (LEGACY_GLOBAL, LEGACY_LOCAL)
        glob = sem in (CORE_GLOBAL, LEGACY_GLOBAL)
        if sem == CORE_LOCAL:
            # (no 0 tags either: a pair without a positive cell is an error, and a positive end cell is a step of its own; 1 tag is
            # the end cell whose predecessor is a Beginning)
            add("tags", "1_%s" % sn, sem, [("jq", 5), ("jt", 4), ("w", 1)], dict(tags=1))
        elif sem == LEGACY_LOCAL:
            add("tags", "0_%s" % sn, sem, [("jq", 5), ("jt", 4), ("w", 1)], dict(tags=0))
            add("tags", "0_row1_%s" % sn, sem, [("w", 1), ("qW", 60), ("tG", 70)], dict(tags=0, end_row=1))
            add("tags", "1_%s" % sn, sem, [("jq", 5), ("jt", 4), ("w", 2)], dict(tags=1))
        elif sem == LEGACY_GLOBAL:
            add("tags", "0_%s" % sn, sem, [("w", 1)], dict(tags=0))
            add("tags", "1_%s" % sn, sem, [("w", 2)], dict(tags=1))
        else:
            add("tags", "1_%s" % sn, sem, [("w", 1)], dict(tags=1))
        for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 385):
            steps = n + (1 if legacy else 0)
            gap = ("q", 2) if n % 2 else ("t", 2)
            a = steps // 2 - 1
            add("tags", "%d_%s" % (n, sn), sem, [("m", a), gap, ("m", steps - 2 - a)], dict(tags=n, gap=n > 64),
                subset=sem in (CORE_LOCAL, CORE_GLOBAL) and n in (64, 65, 129, 257))
    # ---- start cells on the borders: legacy global keeps to the border when the residue that opens the match occurs nowhere earlier
    for kind in ("q", "t"):
        for B in (63, 64, 65, 200):
            for inner, tag in ((41, "i40"), (65, "i64")):            # w + m - 1 interior tags (legacy: the end cell's own step is the seed)
                add("border", "%s%d_%s" % (kind, B, tag), LEGACY_GLOBAL, [(kind, B), ("w", 1), ("m", inner - 1)],
                    dict(border=("L" if kind == "q" else "T", B), interior=inner - 1), no_w=True, subset=B in (64, 65) and tag == "i64")
    # ---- the window: one strip of 64 R - 1 rows, Q = 4 spb steps a quad
    for R in (1, 2, 3, 8):
        Q, M = _q(R), 64 * R - 1
        for L in (Q - 1, Q, Q + 1, 2 * Q, 2 * Q + 1, 3 * Q + 1):
            for pn, mod in (("first", Q - 1), ("last", 0)):
                a, b, d = _place(M, R, L, "q", mod)
                aim = dict(run=("L", L), run_mod=("L", Q, mod, d), R=R)
                if L == 3 * Q + 1:
                    aim["reasons"] = {"dq"}
                add("window", "R%d_left%d_%s" % (R, L, pn), CORE_GLOBAL, [("m", a), ("q", L), ("m", b)], aim, subset=L in (Q + 1, 3 * Q + 1) and pn == "first")
                if M - L < 2 * max(R, 4) + 8:
                    continue                                        # (no room for a Top run of L rows: R = 1 has 63 rows and Q = 64)
                a, b, d = _place(M, R, L, "t", mod)
                aim = dict(run=("T", L), run_mod=("T", Q, mod, d), R=R)
                if L >= 2 * Q + 1 and R >= 3:
                    aim["reasons"] = {"wrap"}
                add("window", "R%d_top%d_%s" % (R, L, pn), CORE_GLOBAL, [("m", a), ("t", L), ("m", b)], aim, subset=L == 2 * Q + 1 and pn == "first")
        if R == 1:                                                  # the Top runs a strip of 63 rows has room for
            for L in (20, 40):
                add("window", "R1_top%d" % L, CORE_GLOBAL, [("m", (63 - L) // 2), ("t", L), ("m", 63 - L - (63 - L) // 2)], dict(run=("T", L), R=1))
    # R = 8 with local flanks (the rule fits in 511 rows), and the R = 8 strip as the first of two (M = 575: the last strip has R = 1)
    for L in (7, 8, 9, 16, 17, 25):
        add("window", "R8_left%d_local" % L, CORE_LOCAL, [("m", 250), ("q", L), ("m", 261)], dict(run=("L", L), R=8), subset=L == 25)
        add("window", "R8_top%d_local" % L, CORE_LOCAL, [("m", 240), ("t", L), ("m", 271 - L)], dict(run=("T", L), R=8), subset=L == 25)
        add("window", "R8_left%d_two" % L, CORE_GLOBAL, [("m", 250), ("q", L), ("m", 325)], dict(run=("L", L), strips={0, 1}, run_strip=0), subset=L == 17)
        add("window", "R8_top%d_two" % L, CORE_GLOBAL, [("m", 240), ("t", L), ("m", 335 - L)], dict(run=("T", L), strips={0, 1}, run_strip=0))
    # a staircase of runs that each carry the path out of the window (runs of 3 between flanks of 2 never move it more than three
    # steps off the prediction, and no oracle keeps to them): five rounds or more in the one strip
    stair = [("m", 52)]
    for _ in range(3):
        stair += [("q", 26), ("m", 52), ("t", 30), ("m", 52)]
    add("window", "R8_staircase", CORE_GLOBAL, stair, dict(rounds_in_strip=5, reasons={"dq", "wrap"}, R=8), subset=True)
    # ---- strip changes
    for M in (513, 576, 1030, 1100):
        add("strips", "diag_%d" % M, CORE_LOCAL, [("m", M // 2), ("q", 3), ("m", M - M // 2)], dict(strips=set(range(bm.num_strips(M))), gap=True),
            subset=M in (513, 1100))
        add("strips", "diag_%d_global" % M, CORE_GLOBAL, [("m", M // 2), ("t", 3), ("m", M - 3 - M // 2)], dict(strips=set(range(bm.num_strips(M))), gap=True))
    for M in (513, 576, 1030, 1100):
        # (M = 513: the last strip is row 513 alone and nothing lies below the runs, so the path is a forced global one)
        sem = CORE_GLOBAL if M == 513 else CORE_LOCAL
        T = min(31, M - 499)                                        # the Top run holds rows 500 .. 530, or .. 513
        add("strips", "top_500_%d_%d" % (499 + T, M), sem, [("m", 499), ("t", T)] + ([("m", M - 499 - T)] if M > 499 + T else []),
            dict(run=("T", T), run_rows=(500, 499 + T)), subset=M == 576, pure=True)
        add("strips", "left_row513_%d" % M, sem, [("m", 513), ("q", 20)] + ([("m", M - 513)] if M > 513 else []),
            dict(run=("L", 20), run_row=513, run_lane_r=(0, 0)), pure=True)
        add("strips", "left_row512_%d" % M, sem, [("m", 512), ("q", 20), ("m", M - 512)], dict(run=("L", 20), run_row=512, run_lane_r=(63, 7)),
            subset=M == 576, pure=True)
    # leaves strip 1 at column 1: the rest of the path is the Top run of column 1 (core global: interior cells), and at column N
    add("strips", "leave_col1", CORE_GLOBAL, [("t", 520), ("w", 1), ("m", 150)], dict(leave_x=1, strips={0, 1}), no_w=True, subset=True)
    add("strips", "leave_colN", CORE_GLOBAL, [("m", 150), ("t", 520)], dict(leave_x=150, strips={0, 1}, last_block=8), subset=True, pure=True)
    for R in range(1, 9):
        M = 512 + 64 * R - 5
        add("strips", "last_R%d" % R, CORE_LOCAL, [("m", 300), ("q", 9), ("m", M - 300 - 31), ("t", 7), ("m", 24)], dict(last_R=R, gap_in_last=True, strips={0, 1}),
            subset=R in (3, 5, 8))
    # ---- the last block of a lane: Top runs in column N, where k | bmask > lend
    for L in (1, 2, 7, 8, 9, 70):
        # the Top steps of column N whose block ends with the lane's last step lend = lane + N - 1 and not with a full block
        R = bm.pick_r(120 + L)
        partial = sum(((y - 1) // R + 119) % bm.spb(R) != bm.spb(R) - 1 for y in range(121, 121 + L))
        add("lastblock", "top%d" % L, CORE_GLOBAL, [("m", 120), ("t", L)], dict(run=("T", L), last_block=partial, last_block_exact=True), subset=L in (2, 9, 70),
            pure=True)
    for N in range(33, 49):                                         # R = 1 (M <= 64): N mod 16 takes every residue
        add("lastblock", "N%d" % N, CORE_GLOBAL, [("m", N), ("t", 9)], dict(last_block=1, R=1), subset=N in (33, 40, 48))
    for L in (3, 70):
        add("lastblock", "col1_top%d" % L, CORE_GLOBAL, [("t", L), ("w", 1), ("m", 60)], dict(col1=2), no_w=True, subset=L == 70)
    # ---- thin pairs
    for N in (1, 2, 3):
        for M in (64, 65, 513):
            # core global: the path keeps off the border (an interior gap cell costs ext, a border cell del), so all M steps are
            # interior, none beyond column N, through every strip; local: the N steps of the last N rows, M = 513: the second one in
            # another strip
            strips = dict(strips={0, 1}) if M == 513 else {}
            add("thin", "N%d_M%d" % (N, M), CORE_GLOBAL, [("t", M - N), ("m", N)], dict(interior=M, x_max=N, **strips), subset=(N, M) in ((1, 65), (2, 513)))
            add("thin", "N%d_M%d_local" % (N, M), CORE_LOCAL, [("jt", M - N), ("m", N)], dict(interior=N, x_max=N, **(strips if N > 1 else {})))
    for M in (1, 2):
        for N in (64, 65, 700):
            # lanes 0 .. M - 1 only (R = 1), the first step at column N in the highest quad row of the strip; core global: all N steps
            # interior (as above), through every quad row
            aim = dict(lanes_max=M - 1, first_qrow=(N - 1 + M - 1) // 64)
            add("thin", "M%d_N%d" % (M, N), CORE_GLOBAL, [("q", N - M), ("m", M)], dict(aim, interior=N), subset=(M, N) in ((1, 65), (2, 700)))
            add("thin", "M%d_N%d_local" % (M, N), CORE_LOCAL, [("jq", N - M), ("m", M)], dict(aim, interior=M))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


# what a group has to meet between its cases (every window register serves a step, both reasons of a re-centre, a clamped kj)
GROUP_AIMS = {"window": dict(served={"wa", "wb", "wc"}, reasons={"first", "dq", "wrap"}, clamp=True)}


# ---- the two-pairs-per-wave kernel's regions: core global, R = ceil(rows / 32), a Left and a Top run of 2 Q + 1 each
def ubatch_cases():
    out = []
    for rows in (32, 33, 150, 225, 256):
        R = (rows + 31) // 32
        L = 2 * _q(R) + 1
        for cols in (60, 150, 1024):
            # rows = a + L + b + c, cols = a + b + L + c
            rest = min(rows, cols) - L
            if rest < 12:
                L = max(min(rows, cols) - 12, 1)                    # (32 and 33 rows at R = 1, 2: no room for 2 Q + 1)
                rest = min(rows, cols) - L
            a = rest // 3
            b = rest // 3
            c = rest - a - b
            blocks = [("m", a), ("t", L + max(rows - cols, 0)), ("m", b), ("q", L + max(cols - rows, 0)), ("m", c)]
            out.append(Case("ubatch", "r%d_c%d" % (rows, cols), CORE_GLOBAL, blocks, dict(shape=(rows, cols), gap=True, runs=("L", "T")), pure=True,
                            kind="dna" if rows >= 150 and cols == 1024 else "int"))
    return out


def ubatch_r(rows):
    return (rows + 31) // 32


# ---- PWM windows: a 4 x 130 PWM built as tb_single_cases.pwm_case builds its motif; windows that lack 40 motif columns or carry 40
# extra residues, paths that cross 64 and 128 positions
PWM_COLS = 130


def pwm_cases(real):
    rng = np.random.default_rng([sc.SEED, PWM_COLS, int(real)])
    motif = rng.integers(0, 4, PWM_COLS).astype(np.uint8)
    if real:
        pwm = np.round(rng.normal(-4.0, 0.5, (4, PWM_COLS)), 2)
        pwm[motif, np.arange(PWM_COLS)] = np.round(rng.normal(6.0, 0.25, PWM_COLS), 2)
        dele, ext = 11.3, 2.1
    else:
        pwm = np.full((4, PWM_COLS), -4.0)
        pwm[motif, np.arange(PWM_COLS)] = 6.0
        dele, ext = 11.0, 2.0
    junk = lambda n: rng.integers(0, 4, n).astype(np.uint8)  # noqa: E731
    wins = [
        ("short50", motif[40:90].copy()),
        ("len64", motif[:64].copy()),
        ("len65", motif[:65].copy()),
        ("lacks40", np.concatenate([motif[:45], motif[85:]])),
        ("extra40", np.concatenate([motif[:70], junk(40), motif[70:]])),
        ("len128", motif[:128].copy()),
        ("len129", motif[1:].copy()),
        ("whole", np.concatenate([junk(30), motif, junk(25)])),
    ]
    return pwm, dele, ext, wins


# ---- aims
def runs_of(recs, tag):
    """Maximal runs of one tag among the interior steps: lists of records."""
    out, cur = [], []
    for r in recs:
        if r["tag"] == tag:
            cur.append(r)
        elif cur:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def check_aim(case, ref, moves, recs, rounds):
    """recs, rounds: the wave walk's.  Returns the list of misses (empty: the construction holds)."""
    a, miss = case.aim, []
    steps = [r for r in recs if r["tag"] != 3]
    if "tags" in a and len(moves) != a["tags"]:
        miss.append("%d tags, built for %d" % (len(moves), a["tags"]))
    if a.get("gap") and not ("L" in moves or "T" in moves):
        miss.append("no gap in the path")
    if "end_row" in a and ref["end"][0] != a["end_row"]:
        miss.append("end cell in row %d" % ref["end"][0])
    if "interior" in a and len(steps) != a["interior"]:
        miss.append("%d interior steps, built for %d" % (len(steps), a["interior"]))
    if "border" in a:
        kind, n = a["border"]
        tail = moves[len(steps):]
        if len(tail) != n or any(m != kind for m in tail):
            miss.append("border run of %d (%s), built for %d %s" % (len(tail), set(tail), n, kind))
    if "R" in a and not all(r["R"] == a["R"] for r in recs):
        miss.append("rows per lane %s" % {r["R"] for r in recs})
    if "shape" in a and case.shape() != a["shape"]:
        miss.append("shape %s" % (case.shape(),))
    for kind in a.get("runs", ()):
        if not runs_of(recs, bm.TAG[kind]):
            miss.append("no %s run" % kind)
    run = None
    if "run" in a:
        kind, L = a["run"]
        sel = [r for r in runs_of(recs, bm.TAG[kind]) if len(r) == L]
        if not sel:
            miss.append("no %s run of %d: %s" % (kind, L, [len(r) for r in runs_of(recs, bm.TAG[kind])]))
        else:
            run = sel[0]
    if run is not None:
        if "run_mod" in a:
            _, Q, mod, tol = a["run_mod"]
            got = run[0]["k"] % Q
            if min((got - mod) % Q, (mod - got) % Q) > tol:
                miss.append("the run starts at step %d of its quad, built for %d" % (got, mod))
        if "run_row" in a and {r["y"] for r in run} != {a["run_row"]}:
            miss.append("the run lies in rows %s" % {r["y"] for r in run})
        if "run_lane_r" in a and {(r["lane"], r["r"]) for r in run} != {a["run_lane_r"]}:
            miss.append("the run lies in (lane, row) %s" % {(r["lane"], r["r"]) for r in run})
        if "run_rows" in a and not (min(r["y"] for r in run) <= a["run_rows"][0] and max(r["y"] for r in run) >= a["run_rows"][1]):
            miss.append("the run spans rows %d .. %d" % (min(r["y"] for r in run), max(r["y"] for r in run)))
        if "run_strip" in a and {r["strip"] for r in run} != {a["run_strip"]}:
            miss.append("the run lies in strips %s" % {r["strip"] for r in run})
    if "reasons" in a and not a["reasons"] <= {r["reason"] for r in rounds}:
        miss.append("fetch rounds for %s only" % {r["reason"] for r in rounds})
    if "rounds_in_strip" in a:
        most = max([sum(1 for r in rounds if r["strip"] == s) for s in {r["strip"] for r in rounds}] or [0])
        if most < a["rounds_in_strip"]:
            miss.append("%d rounds in one strip" % most)
    if "strips" in a and not a["strips"] <= {r["strip"] for r in recs}:
        miss.append("strips %s visited" % {r["strip"] for r in recs})
    if "leave_x" in a:
        first0 = [r for r in recs if r["strip"] == 0][:1]
        if not first0 or first0[0]["x"] != a["leave_x"]:
            miss.append("strip 0 is entered at column %s" % (first0[0]["x"] if first0 else None))
    if "last_R" in a:
        M = case.shape()[0]
        last = bm.num_strips(M) - 1
        if bm.pick_r(M - last * bm.STRIP_ROWS) != a["last_R"] or not any(r["strip"] == last and r["tag"] in (1, 2) for r in recs):
            miss.append("no gap in a last strip of R = %d" % a["last_R"])
    if a.get("last_block_exact") and sum(1 for r in recs if r["last_block"] and r["tag"] == 2) != a["last_block"]:
        miss.append("%d Top steps in a lane's last block, built for %d" % (sum(1 for r in recs if r["last_block"] and r["tag"] == 2), a["last_block"]))
    if "last_block" in a and sum(1 for r in recs if r["last_block"] and r["tag"] == 2) < a["last_block"]:
        miss.append("%d Top steps in a lane's last block" % sum(1 for r in recs if r["last_block"] and r["tag"] == 2))
    if "x_max" in a and max(r["x"] for r in recs) > a["x_max"]:
        miss.append("column %d" % max(r["x"] for r in recs))
    if "lanes_max" in a and max(r["lane"] for r in recs) > a["lanes_max"]:
        miss.append("lane %d" % max(r["lane"] for r in recs))
    if "first_qrow" in a and recs[0]["qrow"] != a["first_qrow"]:
        miss.append("the first step is in quad row %d" % recs[0]["qrow"])
    if "col1" in a and sum(1 for r in steps if r["x"] == 1) < a["col1"]:
        miss.append("%d interior steps in column 1" % sum(1 for r in steps if r["x"] == 1))
    return miss


AIM_NAMES = ("tags", "gap", "end_row", "interior", "border", "run", "run_mod", "run_row", "run_lane_r", "run_rows", "run_strip", "reasons",
             "rounds_in_strip", "strips", "leave_x", "last_R", "last_block", "col1", "runs", "x_max", "lanes_max", "first_qrow")


# ---- batches that run in a child process (tests/test_tb_batch_gpu.py: the route line of ALN_TRACE_PLAN goes to the child's stderr)
def _filler(rng, n, lo, hi):
    out = []
    for _ in range(n):
        N, M = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        q = rng.integers(0, 20, N).astype(np.uint8)
        t = rng.integers(0, 20, M).astype(np.uint8)
        L = min(N, M) * 2 // 3
        t[:L] = q[:L]
        out.append((q, t))
    return out


UBATCH_MODES = ("ubatch_a", "ubatch_b", "ubatch_c")


def ubatch_mode(case):
    rows, cols = case.aim["shape"]
    return "ubatch_c" if case.kind == "dna" else "ubatch_a" if rows >= 150 else "ubatch_b"


def duo_halves(pairs):
    """Which half of a wave (0: lanes 0 .. 31, 1: lanes 32 .. 63) fills each pair of a two-pairs-per-wave batch: the work queue is the
    pairs by falling cost, equal costs by rising position (aln_pair_cost and aln_plan_order's sort keys, aln_plan_rules.h), and item i of the queue
    takes its positions 2 i and 2 i + 1 (aln_fill_duo_kernel).  Every pair here has one strip."""
    def cost(q, t):
        N, M = len(q), len(t)
        R = bm.pick_r(M)
        return (N + (M + R - 1) // R - 1) * (24 + 21 * R)
    order = sorted(range(len(pairs)), key=lambda i: (-cost(*pairs[i]), i))
    half = [0] * len(pairs)
    for qpos, i in enumerate(order):
        half[i] = qpos & 1
    return half


def batch_of(mode):
    """(pairs, {position: case}, semantics, scheme).  The two-pairs-per-wave kernel's LDS (S, four waves' profiles of 64 x 1 / 2 / 4 / 8
    bytes a code, four staged queries) decides which shapes one batch can hold:
      ubatch_a  rows 150, 225, 256 against 60 and 150 columns among 3 100 fillers of 150 x 150, 20 letters;
      ubatch_b  rows 32, 33 against 60, 150 and 1024 columns among 3 100 fillers of 100 x 100, 20 letters (4 bytes a code);
      ubatch_c  rows 150, 225, 256 against 1024 columns among 3 100 fillers of 150 x 150, the 4-letter scheme (8 bytes a code).
    Every case stands twice, at positions chosen so that duo_halves puts one copy in each half of a wave.
    overlap: the core local cases of the subset among 4 200 fillers of 20 .. 60 residues."""
    rng = np.random.default_rng([sc.SEED, len(mode), ord(mode[-1])])
    b, dele, ext = scheme("int")
    if mode.startswith("ubatch"):
        sel = [c for c in ubatch_cases() if ubatch_mode(c) == mode]
        size = 100 if mode == "ubatch_b" else 150
        pairs = _filler(rng, 3100, size, size)
        S = b[:20, :20].copy()
        if mode == "ubatch_c":
            pairs = [(q % 4, t % 4) for q, t in pairs]
            S, dele, ext = scheme("dna")
        at = {}
        for i, c in enumerate(sel):
            first, second = 200 + 404 * i, 301 + 404 * i
            pairs[first] = c.seqs()
            at[first] = c
            while True:                                             # the second copy: the nearest position that lands in the other half
                saved, pairs[second] = pairs[second], c.seqs()
                half = duo_halves(pairs)
                if half[first] != half[second]:
                    break
                pairs[second] = saved
                second += 1
            at[second] = c
        return pairs, at, CORE_GLOBAL, (S, dele, ext)
    sel = [c for c in cases() if c.subset and c.sem == CORE_LOCAL]
    pairs = _filler(rng, 4200, 20, 60)
    at = {}
    for i, c in enumerate(sel):
        pos = 100 + 333 * i
        pairs[pos] = c.seqs()
        at[pos] = c
    return pairs, at, CORE_LOCAL, (b, dele, ext)


def main(argv):
    """argv: mode, report (.npz).  Summaries of every pair and both strings of every pair, as the batch call returned them."""
    from aligner_amd.batch import PairBatch, align_batch
    mode, report = argv
    pairs, _, sem, (S, dele, ext) = batch_of(mode)
    pb = PairBatch.from_pairs(pairs)
    got = align_batch(pb, sem, dele, ext, S)
    strings, off = [], [0]
    for i in range(len(pb)):
        qa, ta = got.aligned(i) if int(got.results["status"][i]) == 0 else (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        strings += [qa, ta]
        off.append(off[-1] + len(qa) + len(ta))
    np.savez(report, results=got.results, strings=np.concatenate(strings), off=np.array(off))


if __name__ == "__main__":
    main(sys.argv[1:])
