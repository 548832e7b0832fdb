"""CPU model of the row-1 speculation of the fast batch kernel, and the catalogue of pairs that
tests/test_row1_repair_gpu.py sends through it.  Plain Python / numpy; test infrastructure only: nothing under aligner_amd/
imports this module.

Core local with del != ext: the penalty of cell (1, x) is del iff H[M][x-1] == 0, a cell a wavefront has not computed yet.  The
kernel fills with advice bits b[x] instead, reads the bottom row back (z), and repairs strip 0 or fills again where b != z.
The model restates that at the level of H matrices:

* spec_fill      the fill under a given advice; equals the reference's fill iff the advice is self-consistent
* observe        what adopt_advice_zdw (aln_kernels.hip) reads back after a pass: z and last_flip
* classify       the two fills a hazard pair sees first (b = 0, then b = z) compared cell by cell
* predict        the decisions of fast_work / FastStrip::run (which checkpoint, which escalation, how many passes) from the
                 model's matrices alone -- every rule carries the line of the kernel source it restates
* decode_passes  the fields of aln_pair_result.passes

All scores are integers (the fast kernels' domain)."""
import numpy as np

STRIP_ROWS = 512          # ALN_STRIP_ROWS
FULL_R = 8                # ALN_FULL_R
CK_FIRST = 16             # ALN_CK_FIRST
CK_LAST = 1024            # ALN_CK_LAST
REPAIR_ROUNDS = 8         # fast_work: while (!converged && !failed && repairs < 8)


# ---------------------------------------------------------------- geometry (aln_device.h)
def pick_r(rows):
    """aln_pick_r: rows per lane of a pair's last strip, the smallest R with 64 R >= rows."""
    return min(FULL_R, max(1, (rows + 63) // 64))


def spb(R):
    """aln_spb: steps per direction word, the largest power of two <= 16 / R."""
    return 2 if R >= 5 else 4 if R >= 3 else 16 // R


def checkpoint_steps(R, ck_last=CK_LAST):
    """Steps at which strip 0 of a hazard pair saves its lane state (FastStrip::run: "checkpoints sit on quad boundaries: the
    first at max(16, one quad of 4 * SPB steps), then doubling")."""
    quad = 4 * spb(R)
    c = (CK_FIRST + quad - 1) // quad * quad
    out = []
    while c <= ck_last:
        out.append(c)
        c *= 2
    return out


class Geometry:
    """Strip 0 of an M x N pair in the batch kernel's skewed layout."""

    def __init__(self, M, N):
        self.M, self.N = M, N
        self.ns = (M + STRIP_ROWS - 1) // STRIP_ROWS
        self.rows = min(M, STRIP_ROWS)                       # real rows of strip 0
        self.R = pick_r(M) if self.ns == 1 else FULL_R
        self.spb = spb(self.R)
        self.lanes = (self.rows + self.R - 1) // self.R
        self.nsteps = N + self.lanes - 1                     # FastStrip::run: nsteps = N + L - 1
        self.total = (((self.nsteps + self.spb - 1) // self.spb + 3) & ~3) * self.spb      # aln_strip_blocks, in steps
        # every one of the 64 lanes runs its R rows (rows beyond M score against residue code 0: tc[r] = 0) and every lane's
        # registers are compared at a checkpoint, so the model fills 64 R rows of a single-strip pair
        self.fill_rows = 64 * self.R if self.ns == 1 else M

    def step_of(self, y, x):
        """Wave step at which strip 0 computes cell (y, x): lane (y-1) // R runs column x at step x - 1 + lane."""
        return (x - 1) + (y - 1) // self.R


def decode_passes(word):
    """aln_pair_result.passes (include/aligner_hip.h)."""
    word = int(word)
    return dict(full=word & 0x7f, fallback=bool(word & 0x80), repairs=(word >> 8) & 0xff, slot=(word >> 16) & 0xf,
                reason=(word >> 20) & 0xf)


# ---------------------------------------------------------------- the fill under an advice
def _int_matrix(S):
    S = np.asarray(S, dtype=np.float64)
    Si = S.astype(np.int64)
    assert (Si == S).all(), "integer scores only"
    return Si


def spec_fill(q, t, S, del_, ext, b):
    """H of the core-local fill under advice b (index x = 1 .. N; b[1] is ignored): p(1, x) = del iff x == 1 or b[x];
    p(y, x) = del iff H[y-1][x] == 0 for y >= 2; borders 0, no clamp.  Every input of a cell is explicit, so the reference's
    column-major visiting order and any other topological order give the same matrix: this one walks anti-diagonals (one numpy
    expression each); spec_fill_colmajor below is the literal loop nest, and the CPU test holds the two against each other."""
    q = np.asarray(q, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    S = _int_matrix(S)
    N, M = len(q), len(t)
    de, ex = int(del_), int(ext)
    assert de == del_ and ex == ext
    b = np.asarray(b).astype(bool)
    pen1 = np.where(b[:N + 1], de, ex)
    pen1[1] = de
    # K[d][y] = H[y][d - y]: the three inputs of an anti-diagonal are contiguous slices of the two before it
    K = np.zeros((M + N + 1, M + 1), dtype=np.int64)
    for d in range(2, M + N + 1):
        y0, y1 = max(1, d - N), min(M, d - 1)
        top = K[d - 1, y0 - 1:y1]
        left = K[d - 1, y0:y1 + 1]
        diag = K[d - 2, y0 - 1:y1]
        p = np.where(top == 0, de, ex)
        if y0 == 1:
            p[0] = pen1[d - 1]
        sub = S[t[y0 - 1:y1], q[d - y1 - 1:d - y0][::-1]]
        K[d, y0:y1 + 1] = np.maximum(np.maximum(top, left) - p, diag + sub)
    H = np.zeros((M + 1, N + 1), dtype=np.int64)
    yy, xx = np.meshgrid(np.arange(1, M + 1), np.arange(1, N + 1), indexing="ij")
    H[1:, 1:] = K[yy + xx, yy]
    return H


def spec_fill_colmajor(q, t, S, del_, ext, b):
    """The same in the reference's loop nest (simple/mod.rs:187-188: query outer, target inner), cell by cell."""
    S = _int_matrix(S)
    N, M = len(q), len(t)
    H = [[0] * (N + 1) for _ in range(M + 1)]
    for x in range(1, N + 1):
        for y in range(1, M + 1):
            if y == 1:
                p = del_ if (x == 1 or b[x]) else ext
            else:
                p = del_ if H[y - 1][x] == 0 else ext
            H[y][x] = max(H[y - 1][x] - p, H[y][x - 1] - p, H[y - 1][x - 1] + int(S[t[y - 1]][q[x - 1]]))
    return np.array(H, dtype=np.int64)


def no_advice(N):
    return np.zeros(N + 2, dtype=bool)


def observe(H, M=None):
    """(z, last_flip): z[x] = (H[M][x-1] == 0) for x in 2 .. N, last_flip the largest x with z[x] (0: none) -- adopt_advice_zdw:
    "if (z != 0) lf = x" over x = 2 + lane .. N."""
    M = H.shape[0] - 1 if M is None else M
    N = H.shape[1] - 1
    z = no_advice(N)
    z[2:N + 1] = H[M, 1:N] == 0
    nz = np.flatnonzero(z)
    return z, (int(nz[-1]) if len(nz) else 0)


def fixed_point(q, t, S, del_, ext, limit=64):
    """Iterates b := z until the advice is self-consistent: then the fill IS the reference's (induction over its visiting order).
    Returns (H, fills made)."""
    b = no_advice(len(q))
    for n in range(1, limit + 1):
        H = spec_fill(q, t, S, del_, ext, b)
        z, _ = observe(H)
        if (z == b).all():
            return H, n
        b = z
    raise AssertionError("no self-consistent advice within %d fills" % limit)


def classify(q, t, S, del_, ext):
    """The first two fills of a pair: b = 0, then b = z."""
    M, N = len(t), len(q)
    g = Geometry(M, N)
    H0 = spec_fill(q, t, S, del_, ext, no_advice(N))
    z0, last_flip = observe(H0)
    H1 = spec_fill(q, t, S, del_, ext, z0) if last_flip else H0
    z1, _ = observe(H1)
    diff = H0[1:g.rows + 1, 1:] != H1[1:g.rows + 1, 1:]
    ys, xs = np.nonzero(diff)
    return dict(consistent=last_flip == 0, last_flip=last_flip, cells=int(diff.sum()),
                last_step=int(((xs) + (ys // g.R)).max()) if len(ys) else -1,       # (x-1) + (y-1)//R, 0-based indices here
                bottom_row_differs=bool(diff[g.rows - 1].any()), consistent_after=bool((z1 == z0).all()),
                end0=_argmax(H0), end1=_argmax(H1))


def _argmax(H):
    """First maximum in row-major order (ndarray-stats argmax, simple/mod.rs:212)."""
    i = int(np.argmax(H))
    return (i // H.shape[1], i % H.shape[1])


# ---------------------------------------------------------------- the kernel's decisions, from the model's matrices
def _state_same(g, Ha, Hb, c):
    """FastStrip::checkpoint(save = false) at step c, for all 64 lanes: after steps 0 .. c-1 lane l holds Tl[r] = H[lR+1+r][x]
    with x = c - l its newest column (its last one, N, once it has run out of columns; nothing before its first step), hdiag =
    H[lR][x-1] (step(): hdiag = topIn) and bottom = Tl[R-1]."""
    R, N = g.R, g.N
    for l in range(64):
        x = min(c - l, N)
        if x < 1:
            break
        y0 = l * R
        if y0 + 1 > Ha.shape[0] - 1:
            break
        if not np.array_equal(Ha[y0 + 1:y0 + R + 1, x], Hb[y0 + 1:y0 + R + 1, x]):
            return False
        if l and Ha[y0, x - 1] != Hb[y0, x - 1]:
            return False
    return True


def _lane_of_row(M):
    """Lane that owns row y (1-based) in the skewed layout, for every strip of the pair."""
    lane = np.zeros(M + 1, dtype=np.int64)
    ns = (M + STRIP_ROWS - 1) // STRIP_ROWS
    for s in range(ns):
        y0 = s * STRIP_ROWS
        rows = min(M - y0, STRIP_ROWS)
        R = pick_r(rows) if s == ns - 1 else FULL_R
        lane[y0 + 1:y0 + rows + 1] = np.arange(rows) // R
    return lane


def _better(a, b):
    """better_i, core local: greater value, then first in row-major order.  Candidates are (value, y, x) or None."""
    if b is None:
        return a is not None
    if a is None:
        return False
    return a[0] > b[0] or (a[0] == b[0] and (a[1], a[2]) < (b[1], b[2]))


def _row_best(H, y, x_hi):
    """A row's tracker register over columns 1 .. x_hi: the greatest value, the earliest step among equals."""
    if x_hi < 1:
        return None
    row = H[y, 1:x_hi + 1]
    x = int(np.argmax(row))
    return (int(row[x]), y, x + 1)


def predict(q, t, S, del_, ext, ck_last=CK_LAST, no_repair=False, max_passes=4):
    """What fast_work (aln_kernels.hip) does with this pair, as a passes word's fields plus what the decision rested on.
    `exact_stale`: the stale test gave the same answer against the lane's own winner and against the pair's winner (a wave that
    runs the pair alone holds the former, the owner of a shared first pass the latter)."""
    M, N = len(t), len(q)
    g = Geometry(M, N)
    t_fill = np.concatenate([np.asarray(t, dtype=np.int64), np.zeros(g.fill_rows - M, dtype=np.int64)])

    def fill(b):
        return spec_fill(q, t_fill, S, del_, ext, b)

    out = dict(full=1, fallback=False, repairs=0, slot=0, reason=0, last_flip=0, exact_stale=True, ck_step=0, rounds=[])
    H0 = fill(no_advice(N))
    advice, last_flip = observe(H0, M)
    out["last_flip"] = last_flip
    if last_flip == 0:                                           # adopt_advice_zdw returned true: "if (converged) break;"
        out["H"] = H0[:M + 1]
        return out
    converged = False
    if not no_repair:                                            # can_repair = hazard && !no_repair && (one strip || three rows)
        lane_of = _lane_of_row(M)
        lane_best = [None] * 64                                  # FastOut o after the first pass, lane by lane
        for y in range(1, M + 1):
            cand = _row_best(H0, y, N)
            if _better(cand, lane_best[lane_of[y]]):
                lane_best[lane_of[y]] = cand
        pair_best = None
        for c in lane_best:
            if _better(c, pair_best):
                pair_best = c
        comp = H0.copy()
        steps = np.add.outer((np.arange(1, g.fill_rows + 1) - 1) // g.R, np.arange(N))      # step of cell (y, x), rows 1.., columns 1..
        while not converged and out["repairs"] < REPAIR_ROUNDS:
            out["repairs"] += 1
            if last_flip > ck_last:                              # "if (last_flip > a.ck_last) { failed = true; passes |= 0x100000u; break; }"
                out["reason"] = 1
                break
            Hn = fill(advice)
            lim = 512 if last_flip <= 512 else ck_last           # "lim = (in.ck_mode == 2 && in.last_flip <= 512u) ? 512u : in.ck_last"
            stop = None
            for s, c in enumerate(checkpoint_steps(g.R, ck_last)):
                if c >= g.total or c > lim:                      # "kb < nkb && kb * SPB == next_ck"; "next_ck < lim ? next_ck * 2u : none"
                    break
                if last_flip <= c and _state_same(g, H0, Hn, c):  # "__all(checkpoint(...)) && in.last_flip <= next_ck"
                    stop = (s, c)
                    break
            if stop is None:                                     # "if (!__any(ro.repaired)) { ... passes |= 0x300000u; break; }"
                out["reason"] = 3
                break
            s, c = stop
            # the tracker: candidates of the re-run prefix against the saved ones (checkpoint(): old != rbv[r] -> tracker; stale
            # when the saved candidate is the running winner)
            stale_lane = stale_pair = False
            merged = list(lane_best)
            for y in range(1, g.rows + 1):
                l = (y - 1) // g.R
                x_hi = min(c - l, N)
                old, new = _row_best(H0, y, x_hi), _row_best(Hn, y, x_hi)
                if old != new:
                    if old == lane_best[l]:
                        stale_lane = True
                    if old == pair_best:
                        stale_pair = True
                if _better(new, merged[l]):
                    merged[l] = new
            out["exact_stale"] = out["exact_stale"] and stale_lane == stale_pair
            if stale_lane:                                       # "if (!__any(stale)) { ... o.repaired = true; ... } return o;"
                out["reason"] = 3
                out["stale"] = True
                break
            if g.ns > 1 and not np.array_equal(H0[STRIP_ROWS, 1:], Hn[STRIP_ROWS, 1:]):
                out["reason"] = 2                                # "if (ro.c_out != 0) { failed = true; passes |= 0x200000u; break; }"
                break
            out["slot"] = s + 1                                  # "passes = (passes & ~0xf0000u) | ((ro.ck_slot + 1u) << 16)"
            out["ck_step"] = c
            out["rounds"].append((last_flip, c))
            lane_best = merged
            pair_best = None
            for cand in lane_best:
                if _better(cand, pair_best):
                    pair_best = cand
            mask = steps < c
            comp[1:, 1:][mask] = Hn[1:, 1:][mask]                # what memory holds now: the re-run prefix over the pass before
            if g.ns > 1:                                         # "if (ns_skew > 1) { converged = true; break; }"
                converged = True
                break
            z, lf = observe(comp, M)
            converged = bool((z == advice).all())
            advice, last_flip = z, lf
        if converged:
            out["H"] = comp[:M + 1]
            out["end"] = (pair_best[1], pair_best[2])
            return out
        if out["reason"] == 0:                                   # "if (!(passes & 0xf00000u)) passes |= 0x400000u;"
            out["reason"] = 4
    # full passes under the advice adopted last, until one is self-consistent or max_passes is reached ("if ((passes & 0xffu) >=
    # max_passes) break;" sits behind the repair: a pair whose repair converges never reaches the strict-order kernel)
    while True:
        if out["full"] >= max_passes:
            out["fallback"] = True
            break
        Hn = fill(advice)
        out["full"] += 1
        z, _ = observe(Hn, M)
        if (z == advice).all():
            out["H"] = Hn[:M + 1]
            break
        advice = z
    return out


# ---------------------------------------------------------------- constructions
def planted_scheme():
    """Four letters; letter 0 matches itself (+1) and is neutral against everything else, letters 1..3 score 0 on a match and -1
    otherwise: a copy of the target inside the query walks the diagonal at 0 and leaves a zero in the bottom row."""
    S = -np.ones((4, 4))
    S[0] = [1, 0, 0, 0]
    for a in range(1, 4):
        S[a][a] = 0
    return S


def pm1_scheme():
    return np.where(np.eye(4) > 0, 1.0, -1.0)


def planted_pair(M, N, end, seed):
    """(q, t) with exactly one bottom-row zero, in column `end` (so last_flip == end + 1), under planted_scheme() and gaps 2/1 or
    3/1: random letters 1..3, t[0] = q[0] = 0, and t[1:] copied into q[end-M+1 : end]."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4, N).astype(np.uint8)
    t = rng.integers(1, 4, M).astype(np.uint8)
    t[0] = 0
    q[0] = 0
    q[end - M + 1:end] = t[1:]
    return q, t


def random_pair(M, N, seed, letters=4):
    rng = np.random.default_rng(seed)
    return rng.integers(0, letters, N).astype(np.uint8), rng.integers(0, letters, M).astype(np.uint8)


def rider_scheme(boost=10):
    """Eleven letters for pairs whose flip DOES change cells.  1..3 as in planted_scheme (match 0, mismatch -1).  4 is the
    target's first letter only: row 1 scores -3 against everything, except +2 against 5 (a positive cell the row-1 penalty acts
    on), 0 against 6 (the zero a planted copy starts from) and +30 against 10.  5 ends the target (match 0).  8 / 9: target row 2
    against one query column scores +boost: 10 lifts the perturbed cell above the background so that it rides a planted
    diagonal.  10 in the query's last column scores +30 in every row: every lane's end-cell candidate then lies outside any
    re-run prefix."""
    S = -np.ones((11, 11))
    for a in (1, 2, 3, 5, 8):
        S[a][a] = 0
    S[4, :] = -3
    S[4][5], S[4][6] = 2, 0
    S[8][9] = boost
    S[:, 10] = 30
    S[7][7] = 0                    # 7: the query's first letter in crossing_pair -- +1 against 1..3 down column 1, so every
    for a in (1, 2, 3, 8):         # lane's end-cell candidate sits in column 1, ahead of anything a flip can move
        S[a][7] = 1
    S[4][7] = -3
    return S


def rider_pair(M, N, seed, end=0, border=0, boost=False, ride=0, wall=False, period=0):
    """Random letters 1..3 under rider_scheme(); t[0] = 4, t[M-1] = 5.
    end: a copy of t[1:] in q[end-M+1 : end] behind a 6 -- a bottom-row zero in column `end`, and H[1][end] = 2, so the flip at
    column end + 1 changes cell (1, end + 1).  border = k: q[0:k] = t[M-k:M] -- the same at column k off the left border.
    boost: t[1] = 8 and a 9 in the column behind the flip; ride = K: t[2 : 2+K] copied behind that column; wall: 10 in the last
    column; period: t[2 : M-1] repeats with this period (copies at two offsets can then overlap)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4, N).astype(np.uint8)
    t = rng.integers(1, 4, M).astype(np.uint8)
    if period:
        t[2:M - 1] = np.resize(t[2:2 + period], M - 3)
    t[0], t[M - 1] = 4, 5
    if boost:
        t[1] = 8
    flip = 0
    if end:
        q[end - M] = 6
        q[end - M + 1:end] = t[1:]
    if border:
        q[0:border] = t[M - border:]
        flip = border + 1
    elif end:
        flip = end + 1
    if boost:
        q[flip] = 9
    if ride:
        q[flip + 1:flip + 1 + ride] = t[2:2 + ride]
    if wall:
        q[N - 1] = 10
    return q, t


def crossing_pair(M, N, seed, period, start, ride):
    """A multi-strip pair under rider_scheme() whose repair re-joins the checkpointed state although strip 0's bottom row has
    moved.  q[0:3] = t[M-3:M] puts a bottom-row zero in column 3 (flip at 4, and H[1][3] = 2 makes it change cell (1, 4): 1
    becomes 0); q[4 : 4+ride] = t[1 : 1+ride] lets that difference ride a diagonal of matches down through row 512, after which it
    dies out; a whole copy of t[1:] behind a 6 at column `start` adds a flip beyond column 512, so that the repair may run on to
    the checkpoint at 1024.  t repeats with `period`, which start - 4 is a multiple of: the two copies overlap."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4, N).astype(np.uint8)
    t = rng.integers(1, 4, M).astype(np.uint8)
    t[1:M - 3] = np.resize(t[1:1 + period], M - 4)
    t[0], t[M - 1], t[M - 3] = 4, 5, 7
    q[0:3] = t[M - 3:]
    q[4:4 + ride] = t[1:1 + ride]
    q[start - 1] = 6
    q[start:start + M - 1] = t[1:M]
    return q, t


def border_pair(M, N, k, seed):
    """planted_pair's counterpart for flips in the first M columns: q[0:k] = t[M-k:M] runs a diagonal of zeros off the left
    border into H[M][k], so last_flip == k + 1; the +1 cell of planted_scheme() sits in the last column instead."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4, N).astype(np.uint8)
    t = rng.integers(1, 4, M).astype(np.uint8)
    t[0] = 0
    q[N - 1] = 0
    q[0:k] = t[M - k:]
    return q, t


def plain_pair(M, N, seed):
    """planted_pair without the copy: no bottom-row zero at all."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 4, N).astype(np.uint8)
    t = rng.integers(1, 4, M).astype(np.uint8)
    t[0] = 0
    q[0] = 0
    return q, t


# ---------------------------------------------------------------- the catalogue
SCHEMES = {"planted": planted_scheme, "pm1": pm1_scheme, "rider": rider_scheme, "rider2": lambda: rider_scheme(2)}
BUILDERS = {"plain": plain_pair, "planted": planted_pair, "border": border_pair, "random": random_pair, "rider": rider_pair,
            "crossing": crossing_pair}

# (name, class, builder, arguments, scheme, (del, ext), route of the default run: (full passes, repairs, slot, reason)).
# Classes: consistent | harmless (a flip, no cell changes) | dies_out (cells change, the repair re-joins) | beyond (a flip past
# the last checkpoint) | bottom_row (strip 0's bottom row moves) | no_rejoin (last_flip <= 512, cells still differ at step 512
# although the strip has a checkpoint at 1024) | unsettled (single strip, the second advice is not self-consistent either) |
# rounds (single strip, two repair rounds) | stale (the repair re-joins, but the pair's old end cell is gone).
# tests/test_advice_model_cpu.py certifies every line with classify / predict.
CATALOGUE = [
    ("c64", "consistent", "plain", (64, 200, 1), "planted", (2, 1), (1, 0, 0, 0)),
    ("c600", "consistent", "plain", (600, 300, 2), "planted", (3, 1), (1, 0, 0, 0)),
    # harmless flips, last_flip at and just behind a checkpoint step: every R of aln_pick_r, every slot of every R's sequence
    ("h64_64", "harmless", "border", (64, 200, 63, 1), "planted", (2, 1), (1, 1, 1, 0)),          # R 1: 64
    ("h64_66", "harmless", "planted", (64, 260, 64, 1), "planted", (2, 1), (1, 1, 2, 0)),         #      128
    ("h128_32", "harmless", "border", (128, 200, 31, 1), "planted", (3, 1), (1, 1, 1, 0)),        # R 2: 32
    ("h128_33", "harmless", "border", (128, 200, 32, 1), "planted", (2, 1), (1, 1, 2, 0)),        #      64
    ("h192_16", "harmless", "border", (192, 200, 15, 1), "planted", (2, 1), (1, 1, 1, 0)),        # R 3: 16
    ("h192_17", "harmless", "border", (192, 200, 16, 1), "planted", (3, 1), (1, 1, 2, 0)),        #      32
    ("h256_128", "harmless", "border", (256, 400, 127, 1), "planted", (2, 1), (1, 1, 4, 0)),      # R 4: 128
    ("h256_129", "harmless", "border", (256, 400, 128, 1), "planted", (2, 1), (1, 1, 5, 0)),      #      256
    ("h320_256", "harmless", "border", (320, 400, 255, 1), "planted", (2, 1), (1, 1, 5, 0)),      # R 5: 256
    ("h384_257", "harmless", "border", (384, 700, 256, 1), "planted", (3, 1), (1, 1, 6, 0)),      # R 6: 512
    ("h448_512", "harmless", "planted", (448, 700, 511, 1), "planted", (2, 1), (1, 1, 6, 0)),     # R 7: 512
    ("h448_513", "harmless", "planted", (448, 1200, 512, 1), "planted", (2, 1), (1, 1, 7, 0)),    #      1024
    ("h512_1024", "harmless", "planted", (512, 1200, 1023, 1), "planted", (2, 1), (1, 1, 7, 0)),  # R 8: 1024
    ("h513_2", "harmless", "border", (513, 200, 1, 1), "planted", (2, 1), (1, 1, 1, 0)),          # two strips: 16
    ("h513_600", "harmless", "planted", (513, 1200, 599, 1), "planted", (3, 1), (1, 1, 7, 0)),
    ("h600_40", "harmless", "border", (600, 200, 39, 1), "planted", (2, 1), (1, 1, 3, 0)),        #      64
    ("h600_901", "harmless", "planted", (600, 1200, 900, 1), "planted", (2, 1), (1, 1, 7, 0)),
    ("h1100_300", "harmless", "border", (1100, 700, 299, 1), "planted", (2, 1), (1, 1, 6, 0)),    # three strips: 512
    ("b512_1025", "beyond", "planted", (512, 1200, 1024, 1), "planted", (2, 1), (2, 1, 0, 1)),
    ("b1100_1251", "beyond", "planted", (1100, 1300, 1250, 1), "planted", (2, 1), (2, 1, 0, 1)),
    ("b64_1101", "beyond", "planted", (64, 1300, 1100, 1), "planted", (3, 1), (2, 1, 0, 1)),
    ("d128", "dies_out", "rider", (128, 300, 1, 140), "rider", (3, 1), (1, 1, 4, 0)),
    ("d448", "dies_out", "rider", (448, 1250, 3, 600), "rider", (2, 1), (1, 1, 7, 0)),
    ("d600", "dies_out", "rider", (600, 1300, 0, 900), "rider", (2, 1), (1, 1, 7, 0)),            # end cell (1, 900): in the re-run prefix
    ("d1100", "dies_out", "random", (1100, 1300, 4), "pm1", (2, 1), (1, 1, 3, 0)),
    ("m1100", "bottom_row", "random", (1100, 1300, 1), "pm1", (2, 1), (2, 1, 0, 3)),              # 43 526 cells, never re-joins
    ("m513", "bottom_row", "crossing", (513, 1200, 1, 100, 404, 511), "rider", (2, 1), (2, 1, 0, 2)),
    ("n600", "no_rejoin", "rider", (600, 1300, 0, 0, 3, True, 540, True), "rider", (2, 1), (2, 1, 0, 3)),
    ("u40_1", "unsettled", "random", (40, 300, 1), "pm1", (2, 1), (3, 1, 0, 3)),
    ("u40_2", "unsettled", "random", (40, 300, 2), "pm1", (2, 1), (3, 1, 0, 3)),
    ("r100", "rounds", "random", (100, 300, 29), "pm1", (2, 1), (1, 2, 4, 0)),
    ("r40", "rounds", "random", (40, 300, 13), "pm1", (1, 2), (1, 2, 3, 0)),                      # del < ext
    ("s600", "stale", "rider", (600, 1200, 3, 700, 0, True), "rider2", (2, 1), (2, 1, 0, 3)),     # end cell (2, 702) -> (1, 700)
]


def entry_pair(entry):
    """(q, t, S, del, ext) of a catalogue line."""
    name, cls, builder, args, scheme, gaps, route = entry
    q, t = BUILDERS[builder](*args)
    return q, t, SCHEMES[scheme](), gaps[0], gaps[1]
