"""CPU model of the row-1 advice passes of the generic kernels (do_pair and aln_fill_wgpipe_kernel around
adopt_advice_checked, aln_kernels.hip), and the catalogue of pairs that tests/test_advice_generic_gpu.py sends through every
route of that family.  Plain Python / numpy; test infrastructure only: nothing under aligner_amd/ imports this module.

Core local with del != ext: the penalty of cell (1, x) is del iff H[M][x-1] == 0.  A pass fills under advice bits b, records row 1
(value and direction tag) and the bottom row's zeros z, and adopt_advice_checked then decides: no bit differs -- the pass stands;
some differ, but cell (1, x) recomputed under the new bit keeps value and tag at every such x -- the pass stands as well (by
induction over the reference's visiting order the fill under z is this very fill); otherwise fill again under z.

* spec_fill         H and the 2-bit direction tag of every cell under a given advice, f64 arithmetic in the cell's own order
                    (integer schemes are exact in f64 far beyond the sizes used here, and |m - x| < EPSILON is == for them)
* predict_generic   the expected aln_pair_result.passes word and how it came about, pass by pass; `defect` plants one wrong
                    rule (test_advice_generic_cpu.py shows that the catalogue sees each of them)
* CATALOGUE         constructed and seeded pairs, each line naming the outcome or edge it exists for

The three recorders (run_strip, the lean f64 strip, wg_strip) differ in how they write row1 / row1tag / zrow, not in what: the
model has one record, and every route is held to it."""
import numpy as np

import advice_model as am

EPS = 2.0 ** -52                                  # f64::EPSILON (enums.rs:21-25; DBL_EPSILON in the kernels)
TAG_DIAG, TAG_LEFT, TAG_TOP, TAG_BEG = 0, 1, 2, 3  # cell_tag: "0 Diagonal, 1 Left, 2 Top, 3 Beginning"
TAG_TO_D = np.array([2, 1, 0, 3], dtype=np.uint8)  # the oracle's D codes (TOP, LEFT, DIAGONAL, BEGINNING = 0, 1, 2, 3)

DEFECTS = ("no_tag", "end_n_minus_1", "start_3", "stride_mix", "old_penalty", "row1_x", "lean_unswapped", "lean_row_r",
           "b_partial")


def cell_f(top, left, diag, s, p):
    """cell_tag / cell_tag_f64 / the lean blocks (ALN_F64_CELL_HEAD + _LOCAL_TAIL), on scalars or arrays:
    "a = topH - p, b = leftH - p, c = diagH + s; m = vmax(vmax(a, b), c)" -- three roundings, no FMA (numpy fuses nothing);
    "tag = eq(m, b) ? 1 : 0; tag = eq(m, a) ? 2 : tag" with eq = |m - x| < EPSILON (ScOps<double>::eq; the asm forms compute
    m - a >= 0 and compare "eps > da"); "tag = (m == 0) ? 3 : tag" (the lean blocks: Z = (0 == m) is or-ed into both tag bits).
    All three agree on tag 3: exactly the cells with m == 0, whatever the distances say."""
    a, b, c = top - p, left - p, diag + s
    m = np.maximum(np.maximum(a, b), c)
    tag = np.where(np.abs(m - b) < EPS, TAG_LEFT, TAG_DIAG)
    tag = np.where(np.abs(m - a) < EPS, TAG_TOP, tag)
    tag = np.where(m == 0, TAG_BEG, tag)
    return m, tag


def spec_fill(q, t, S, del_, ext, b, pwm=False):
    """(H, T) of the core-local fill under advice b (index x = 1 .. N; b[1] is ignored): p(1, x) = del iff x == 1 or b[x]
    (run_strip: "if (r == 0 && y == 1) p = (x == 1 || adv != 0) ? del : ext"), p(y, x) = del iff H[y-1][x] == 0 for y >= 2
    ("p = (top == 0) ? del : ext"); borders 0.  pwm: the score of column x is S[t[y-1]][x-1] ("pwm ? (int)(x - 1) : q[x - 1]").
    Anti-diagonals, one numpy expression each, as advice_model.spec_fill."""
    t = np.asarray(t, dtype=np.int64)
    S = np.asarray(S, dtype=np.float64)
    M = len(t)
    N = S.shape[1] if pwm else len(q)
    qq = np.arange(N) if pwm else np.asarray(q, dtype=np.int64)
    de, ex = float(del_), float(ext)
    b = np.asarray(b).astype(bool)
    pen1 = np.where(b[:N + 1], de, ex)
    if N >= 1:
        pen1[1] = de
    K = np.zeros((M + N + 1, M + 1))
    KT = np.zeros((M + N + 1, M + 1), dtype=np.uint8)
    for d in range(2, M + N + 1):
        y0, y1 = max(1, d - N), min(M, d - 1)
        top = K[d - 1, y0 - 1:y1]
        left = K[d - 1, y0:y1 + 1]
        diag = K[d - 2, y0 - 1:y1]
        p = np.where(top == 0, de, ex)
        if y0 == 1:
            p[0] = pen1[d - 1]
        sub = S[t[y0 - 1:y1], qq[d - y1 - 1:d - y0][::-1]]
        K[d, y0:y1 + 1], KT[d, y0:y1 + 1] = cell_f(top, left, diag, sub, p)
    H = np.zeros((M + 1, N + 1))
    T = np.full((M + 1, N + 1), TAG_BEG, dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(1, M + 1), np.arange(1, N + 1), indexing="ij")
    H[1:, 1:] = K[yy + xx, yy]
    T[1:, 1:] = KT[yy + xx, yy]
    return H, T


def observe(H, M):
    """z[x] = (H[M][x-1] == 0) for x = 2 .. N: what the last strip leaves in zrow ("w.zrow[x] = (hb == 0) ? 1 : 0", hb the row rb of
    lane lb; the lean strip reads the same cell's tag == 3) as adopt_advice_checked reads it ("z = zrow[x - 1]")."""
    N = H.shape[1] - 1
    z = np.zeros(N + 2, dtype=bool)
    if N >= 2:
        z[2:N + 1] = H[M, 1:N] == 0
    return z


def _walked(N, nthreads, defect):
    """Columns adopt_advice_checked visits: "for (x = 2 + tid; x <= N; x += nthreads)" over tid = 0 .. nthreads-1 -- every x of
    2 .. N, whatever the stride."""
    lo, hi = 2, N
    if defect == "start_3":
        lo = 3
    if defect == "end_n_minus_1":
        hi = N - 1
    cols = set(range(lo, hi + 1))
    if defect == "stride_mix":
        # the one-wave walk (x = 2 + lane) under the workgroup's stride (x += blockDim.x): with more than 64 threads columns
        # 66 .. 1 + nthreads (mod nthreads) are never looked at.  (Stride 64 from every thread's own 2 + tid would only visit
        # columns twice; this is the mix of the two walks that loses some.)
        cols = {x for lane in range(64) for x in range(2 + lane, N + 1, max(nthreads, 64))}
    return cols


def predict_generic(q, t, S, del_, ext, max_passes=4, pwm=False, defect=None, nthreads=64, check=True):
    """What do_pair / aln_fill_wgpipe_kernel do with this pair.  Returns dict(word = the expected passes & 0xff, passes, fallback,
    outcome = no_hazard | consistent | same | fallback, moves = per unconverged-or-last pass "value" / "tag" / None, movers =
    per pass the columns whose cell moved, flips = per pass the flipped columns, H, T, z of the last pass).
    nthreads matters to a planted defect only.  defect "lean_row_r" reads nthreads as the strip's rows per lane."""
    assert defect is None or defect in DEFECTS
    t = np.asarray(t, dtype=np.int64)
    S = np.asarray(S, dtype=np.float64)
    M = len(t)
    N = S.shape[1] if pwm else len(q)
    qq = np.arange(N) if pwm else np.asarray(q, dtype=np.int64)
    de, ex = float(del_), float(ext)
    out = dict(passes=1, fallback=False, outcome="no_hazard", moves=[], movers=[], flips=[])
    b = np.zeros(N + 2, dtype=bool)                              # do_pair: "w.advice[x] = 0" for every x
    if N < 2 or de == ex:                                        # "w.hazard = (SEM == ALN_CORE_LOCAL) && (w.del != w.ext) && N >= 2"
        out["H"], out["T"] = spec_fill(q, t, S, de, ex, b, pwm)  # "if (!w.hazard) { converged = true; break; }"
        out["z"] = observe(out["H"], M)
        out["word"] = 1
        return out
    max_passes = max_passes or 4                                 # "max_passes = a.max_passes ? a.max_passes : 4u"
    walked = _walked(N, nthreads, defect)
    k = 0
    while True:
        H, T = spec_fill(q, t, S, de, ex, b, pwm)
        k += 1                                                   # "++passes"
        z = observe(H, M)
        flips = [x for x in range(2, N + 1) if b[x] != z[x] and x in walked]       # "if (advice[x] != z) { mismatch = 1; ..."
        rec = T[1].copy()                                        # row1tag as the strip recorded it
        if defect == "lean_unswapped":                           # "(t & 1) << 1 | (t >> 1)" left out: Top and Left trade places
            rec = np.array([0, 2, 1, 3], dtype=np.uint8)[rec]
        if defect == "lean_row_r":                               # the tag of the lane's LAST row: bits 0..1, not 2 (R - 1)..
            rec = T[min(nthreads, M)].copy()
        movers, kinds = [], set()
        nb = b.copy()
        for x in flips:
            p = de if z[x] else ex                               # "z ? del : ext"
            if defect == "old_penalty":
                p = de if b[x] else ex
            left = H[1, x] if defect == "row1_x" else H[1, x - 1]          # "row1[x - 1]"
            h, tag = cell_f(0.0, left, 0.0, S[t[0], qq[x - 1]], p)          # "cell_tag((SC)0, row1[x - 1], (SC)0, S[t0 + ...], ...)"
            vm = not (h == H[1, x])                              # "if (!(h == row1[x]) || tag != row1tag[x]) moved = 1"
            tm = int(tag) != int(rec[x]) and defect != "no_tag"
            if vm or tm:
                movers.append(x)
                kinds.add("value" if vm else "tag")
            if defect != "b_partial" or vm or tm:
                nb[x] = z[x]                                     # "advice[x] = z"
        out["flips"].append(flips)
        out["movers"].append(movers)
        out["moves"].append("value" if "value" in kinds else "tag" if kinds else None)
        out.update(passes=k, H=H, T=T, z=z)
        if not flips:                                            # "converged = !__any(!unchanged) || ..."
            out["outcome"] = "consistent"
            break
        if not movers:                                           # "... || !__any(!same)"
            out["outcome"] = "same"
            if check and defect is None:
                # the induction the kernel's comment claims, executed: the fill under the new advice IS this fill
                H2, T2 = spec_fill(q, t, S, de, ex, nb, pwm)
                assert np.array_equal(H2, H) and np.array_equal(T2, T), "a pass accepted as 'same' is not the fill under its own zeros"
                assert np.array_equal(observe(H2, M), z)
            break
        b = nb
        if k >= max_passes:                                      # "while (!converged && passes < max_passes)"; "passes |= 0x80u"
            out["outcome"] = "fallback"
            out["fallback"] = True
            break
    out["word"] = out["passes"] | (0x80 if out["fallback"] else 0)
    return out


def near_tie_cells_row1(H, q, t, S, del_, ext, z, pwm=False):
    """Cells (1, x) of a converged fill in which a candidate lies strictly inside (m - EPS, m): the tag is decided by the tolerance,
    not by equality."""
    N = H.shape[1] - 1
    qq = np.arange(N) if pwm else np.asarray(q, dtype=np.int64)
    n = 0
    for x in range(1, N + 1):
        p = float(del_) if (x == 1 or z[x]) else float(ext)
        a, b, c = 0.0 - p, H[1, x - 1] - p, 0.0 + S[t[0], qq[x - 1]]
        m = max(max(a, b), c)
        n += int(any(0 < m - v < EPS for v in (a, b)))
    return n


# ---------------------------------------------------------------- geometry of the routes
def lean_r(M):
    """Rows per lane of strip 0 in the batch kernels' skewed layout: aln_pick_r for a one-strip pair, ALN_FULL_R else."""
    return am.pick_r(M) if M <= am.STRIP_ROWS else am.FULL_R


def wg_route(M, N):
    """(R, threads) of the one-workgroup route, None when aln_wg_route_r refuses the pair: "pc >= (1 << 14) && d.N >= 16 && d.N <=
    8192 && d.M >= 65 && d.M <= 2048", "R = d.M > 1024 ? 4 : d.M > 512 ? 2 : 1", one wave per strip of 64 R rows."""
    if not (M * N >= (1 << 14) and 16 <= N <= 8192 and 65 <= M <= 2048):
        return None
    R = 4 if M > 1024 else 2 if M > 512 else 1
    return R, 64 * ((M + 64 * R - 1) // (64 * R))


# ---------------------------------------------------------------- schemes
def blosum62():
    from aligner_amd.matrices import get_blosum62
    return np.asarray(get_blosum62(), dtype=np.float64)


def tenths_scheme():
    """Scores in tenths with gaps 0.2 / 0.1 (the near-tie scheme of test_value_limits_gpu.py): sums of tenths miss each other by an
    ulp, so tags are decided inside f64::EPSILON."""
    return np.array([[0.3, -0.1, -0.2, -0.2], [-0.1, 0.3, -0.2, -0.2], [-0.2, -0.2, 0.3, -0.1], [-0.2, -0.2, -0.1, 0.3]])


def pwm_int_scheme(W=60, seed=60):
    return np.random.default_rng(seed).integers(-2, 3, (4, W)).astype(np.float64)


SCHEMES = {
    "pm1": (am.pm1_scheme, 4, True),                  # name: (matrix, letters, integer-valued)
    "blosum": (blosum62, 20, True),
    "blosum_half": (lambda: blosum62() * 0.5, 20, False),
    "blosum_037": (lambda: blosum62() * 0.37, 20, False),
    "tenths": (tenths_scheme, 4, False),
    "pwm_int": (pwm_int_scheme, 4, True),
    "pwm_real": (lambda: pwm_int_scheme() * 0.5, 4, False),
}


def seeded_pair(M, N, seed, letters):
    rng = np.random.default_rng(seed)
    return rng.integers(0, letters, N).astype(np.uint8), rng.integers(0, letters, M).astype(np.uint8)


def column_pair(M, N, col, seed=0):
    """A pair under advice_model.rider_scheme() whose only bottom-row zero sits in column col - 1 and whose flip at `col` moves
    cell (1, col) by value (advice_model.rider_pair: a copy of the target's tail behind a 6, or off the left border)."""
    return am.rider_pair(M, N, seed, end=col - 1) if col - 1 >= M else am.rider_pair(M, N, seed, border=col - 1)


SCHEMES["rider"] = (am.rider_scheme, 11, True)

# (name, what the line is there for, builder, M, N, seed or column, scheme, (del, ext), outcome, passes, declared properties).
# Properties (certified by tests/test_advice_generic_cpu.py from the oracle and the model alone):
#   first = "tag" | "value"   what forced the second pass: a direction alone (an exact tie between left - p and diag + s), or a value
#   sole = x                  pass 1 has exactly one flipped column whose cell moves, x: skip it and the prediction is one pass
#   flips                     the first advice was wrong somewhere
#   near                      a cell of row 1 has a candidate strictly inside (m - EPSILON, m)
CATALOGUE = [
    # ---- outcomes
    ("c1", "1 pass, consistent", "seed", 3, 40, 18, "pm1", (2, 1), "consistent", 1, {}),
    ("s1", "1 pass, wrong and harmless advice", "seed", 3, 20, 45, "pm1", (1.5, 0.5), "same", 1, {"flips": 1}),
    ("c2", "2 passes, consistent; the second forced by a tag alone", "seed", 3, 40, 0, "pm1", (3, 1), "consistent", 2, {"first": "tag"}),
    ("v2", "2 passes, consistent; the second forced by a value", "seed", 3, 40, 4, "pm1", (3, 1), "consistent", 2, {"first": "value"}),
    ("c3", "3 passes, consistent", "seed", 3, 40, 1, "pm1", (1, 2), "consistent", 3, {}),
    ("c4", "4 passes, consistent", "seed", 3, 40, 298, "pm1", (1, 2), "consistent", 4, {}),
    ("s2", "2 passes, the second wrong and harmless", "seed", 3, 40, 6, "pm1", (1, 2), "same", 2, {}),
    ("s3", "3 passes, the third wrong and harmless", "seed", 3, 40, 11, "pm1", (1.5, 0.5), "same", 3, {}),
    ("s4", "4 passes, the fourth wrong and harmless", "seed", 3, 40, 128, "pm1", (1.5, 0.5), "same", 4, {}),
    ("fb", "not converged in 4 passes, integers", "seed", 3, 40, 363, "pm1", (2, 1), "fallback", 4, {}),
    ("fbf", "not converged in 4 passes, halves", "seed", 3, 40, 32, "pm1", (1.5, 0.5), "fallback", 4, {}),
    # ---- loop edges of adopt_advice_checked
    ("x2", "the only deciding flip at x = 2", "seed", 3, 20, 328, "pm1", (3, 1), "consistent", 2, {"sole": 2, "first": "tag"}),
    ("xN", "the only deciding flip at x = N", "seed", 3, 20, 60, "pm1", (2, 1), "consistent", 2, {"sole": 20, "first": "tag"}),
    ("n2", "N = 2, the smallest hazard pair", "seed", 2, 2, 21, "pm1", (2, 1), "consistent", 2, {"sole": 2}),
    ("n1", "N = 1: no hazard", "seed", 3, 1, 4, "pm1", (2, 1), "no_hazard", 1, {}),
    ("eq", "del == ext: no hazard", "seed", 3, 40, 363, "pm1", (2, 2), "no_hazard", 1, {}),
    ("k63", "deciding flip at column 63", "col", 65, 300, 63, "rider", (2, 1), "consistent", 2, {"sole": 63}),
    ("k64", "deciding flip at column 64", "col", 65, 300, 64, "rider", (2, 1), "consistent", 2, {"sole": 64}),
    ("k65", "deciding flip at column 65", "col", 65, 300, 65, "rider", (2, 1), "consistent", 2, {"sole": 65}),
    ("k66", "deciding flip at column 66: lane 0's second column", "col", 65, 300, 66, "rider", (2, 1), "consistent", 2, {"sole": 66}),
    ("k127", "deciding flip at column 127", "col", 65, 300, 127, "rider", (2, 1), "consistent", 2, {"sole": 127}),
    ("k128", "deciding flip at column 128", "col", 65, 300, 128, "rider", (2, 1), "consistent", 2, {"sole": 128}),
    ("k129", "deciding flip at column 129: the workgroup's last thread (64 ns + 1)", "col", 65, 300, 129, "rider", (2, 1), "consistent", 2, {"sole": 129}),
    ("k130", "deciding flip at column 130: thread 0's second column", "col", 65, 300, 130, "rider", (2, 1), "consistent", 2, {"sole": 130}),
    # ---- recording edges: row 1 is the bottom row, M = 2, every R of a one-strip pair, two strips
    ("m1", "M = 1: row 1 is the bottom row", "seed", 1, 40, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("m2", "M = 2", "seed", 2, 40, 0, "pm1", (1.5, 0.5), "consistent", 4, {}),
    ("r1_63", "R = 1, 63 rows", "seed", 63, 48, 0, "pm1", (2, 1), "consistent", 2, {}),
    ("r1_64", "R = 1, 64 rows", "seed", 64, 48, 0, "pm1", (3, 1), "consistent", 2, {"first": "tag"}),
    ("r2_65", "R = 2, 65 rows", "seed", 65, 48, 1, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r2_127", "R = 2, 127 rows", "seed", 127, 48, 0, "pm1", (3, 1), "consistent", 2, {"first": "tag"}),
    ("r2_128", "R = 2, 128 rows", "seed", 128, 48, 0, "pm1", (1, 2), "consistent", 2, {"first": "tag"}),
    ("r3_129", "R = 3, 129 rows", "seed", 129, 48, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("r3_191", "R = 3, 191 rows", "seed", 191, 48, 0, "pm1", (1, 2), "consistent", 2, {"first": "tag"}),
    ("r3_192", "R = 3, 192 rows", "seed", 192, 48, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r4_193", "R = 4, 193 rows", "seed", 193, 48, 0, "pm1", (3, 1), "consistent", 2, {"first": "tag"}),
    ("r4_255", "R = 4, 255 rows", "seed", 255, 48, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r4_256", "R = 4, 256 rows", "seed", 256, 48, 0, "pm1", (2, 1), "consistent", 2, {}),
    ("r5_257", "R = 5, 257 rows", "seed", 257, 48, 0, "pm1", (1, 2), "consistent", 2, {"first": "tag"}),
    ("r5_319", "R = 5, 319 rows", "seed", 319, 48, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("r5_320", "R = 5, 320 rows", "seed", 320, 48, 0, "pm1", (3, 1), "consistent", 2, {}),
    ("r6_321", "R = 6, 321 rows", "seed", 321, 48, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r6_383", "R = 6, 383 rows", "seed", 383, 48, 0, "pm1", (3, 1), "consistent", 2, {"first": "tag"}),
    ("r6_384", "R = 6, 384 rows", "seed", 384, 48, 0, "pm1", (1, 2), "consistent", 2, {}),
    ("r7_385", "R = 7, 385 rows", "seed", 385, 48, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("r7_447", "R = 7, 447 rows", "seed", 447, 48, 0, "pm1", (1, 2), "consistent", 2, {"first": "tag"}),
    ("r7_448", "R = 7, 448 rows", "seed", 448, 48, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r8_449", "R = 8, 449 rows", "seed", 449, 48, 0, "pm1", (3, 1), "consistent", 2, {}),
    ("r8_511", "R = 8, 511 rows", "seed", 511, 48, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("r8_512", "R = 8, 512 rows", "seed", 512, 48, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("t513", "two strips: row 1 from strip 0, the zero row from a one-row strip 1", "seed", 513, 40, 0, "pm1", (2, 1), "consistent", 2, {"first": "tag"}),
    ("t600", "two strips, 600 rows; one workgroup: R = 2, N = 40", "seed", 600, 40, 0, "pm1", (3, 1), "consistent", 2, {}),
    # ---- the one-workgroup route: two waves of R = 1, R = 2, R = 4; a ring that wraps (N = 300) and one that does not
    ("w65", "one workgroup: two waves, R = 1, the ring wraps", "seed", 65, 300, 0, "pm1", (1.5, 0.5), "consistent", 2, {}),
    ("w600", "one workgroup: R = 2, the ring wraps", "seed", 600, 300, 0, "pm1", (1, 2), "consistent", 2, {}),
    ("w1100s", "one workgroup: R = 4, N = 40", "seed", 1100, 40, 0, "pm1", (1.5, 0.5), "consistent", 2, {"sole": 2}),
    ("w1100", "one workgroup: R = 4, the ring wraps", "seed", 1100, 300, 0, "pm1", (3, 1), "consistent", 2, {}),
    # ---- score families
    ("bi2", "BLOSUM62 integers off the fast path, two passes", "seed", 20, 60, 1, "blosum", (11, 2), "consistent", 2, {}),
    ("bi1", "BLOSUM62 integers, wrong and harmless advice", "seed", 20, 60, 10, "blosum", (11, 2), "same", 1, {"flips": 1}),
    ("bh1", "BLOSUM62 x 0.5, 11.5 / 2.25: wrong and harmless advice", "seed", 20, 60, 1, "blosum_half", (11.5, 2.25), "same", 1, {"flips": 1}),
    ("bh2", "BLOSUM62 x 0.5, 11.5 / 2.25: two passes", "seed", 20, 60, 19, "blosum_half", (11.5, 2.25), "consistent", 2, {"sole": 21}),
    ("b37", "BLOSUM62 x 0.37, 11.3 / 2.1: no zero in the bottom row", "seed", 33, 70, 0, "blosum_037", (11.3, 2.1), "consistent", 1, {}),
    ("b37f", "BLOSUM62 x 0.37: a zero after all, harmless", "seed", 20, 60, 2, "blosum_037", (11.3, 2.1), "same", 1, {"flips": 1}),
    ("rx", "BLOSUM62 with del < ext: a deciding flip whose cell moves through H[1][x-1] alone", "seed", 3, 60, 46, "blosum", (2, 11), "consistent", 2, {}),
    ("bp", "BLOSUM62 with del < ext: harmless flips beside a deciding one, all adopted", "seed", 2, 60, 107, "blosum", (1, 4), "consistent", 2, {}),
    ("l100", "R = 2: harmless flips only, the recorded tags of row 1 are what the recheck finds", "seed", 100, 48, 32, "pm1", (2, 1), "same", 1, {"flips": 1}),
    ("te1", "tenths: a row-1 tag decided inside f64::EPSILON, second pass by a tag", "seed", 5, 60, 60, "tenths", (0.2, 0.1), "consistent", 2, {"first": "tag", "near": 1}),
    ("te2", "tenths: deciding flip at x = N", "seed", 5, 60, 99, "tenths", (0.2, 0.1), "consistent", 2, {"sole": 60, "near": 1}),
    ("te3", "tenths: second pass by a value", "seed", 5, 60, 171, "tenths", (0.2, 0.1), "consistent", 2, {"first": "value", "near": 1}),
    ("pi2", "integer PWM 4 x 60, two passes", "seed", 30, 60, 0, "pwm_int", (2, 1), "consistent", 2, {"first": "value"}),
    ("pi2t", "integer PWM 4 x 60, second pass by a tag", "seed", 30, 60, 2, "pwm_int", (2, 1), "consistent", 2, {"first": "tag"}),
    ("pi1", "integer PWM 4 x 60, wrong and harmless advice", "seed", 30, 60, 4, "pwm_int", (2, 1), "same", 1, {"flips": 1}),
    ("pr2", "real-valued PWM 4 x 60, two passes", "seed", 30, 60, 0, "pwm_real", (1.5, 0.5), "consistent", 2, {}),
    ("pr2b", "real-valued PWM 4 x 60, one deciding flip", "seed", 30, 60, 1, "pwm_real", (1.5, 0.5), "consistent", 2, {"sole": 9}),
    ("pr1", "real-valued PWM 4 x 60, wrong and harmless advice", "seed", 30, 60, 4, "pwm_real", (1.5, 0.5), "same", 1, {"flips": 1}),
]
IDS = [e[0] for e in CATALOGUE]


def is_pwm(entry):
    return entry[6].startswith("pwm")


def entry_pair(entry):
    """(q, t, S, del, ext, pwm) of a catalogue line; q is None for a PWM (the columns of S are the query)."""
    name, _, builder, M, N, arg, scheme, gaps = entry[:8]
    make, letters, _ = SCHEMES[scheme]
    if builder == "col":
        q, t = column_pair(M, N, arg)
    else:
        q, t = seeded_pair(M, N, arg, letters)
    S = make()
    if is_pwm(entry):
        assert S.shape[1] == N
        q = None
    return q, t, S, gaps[0], gaps[1], is_pwm(entry)


_predictions = {}


def prediction(entry, max_passes=0):
    """predict_generic of a catalogue line, computed once per (line, max_passes) and left unchanged."""
    key = (entry[0], max_passes or 4)
    if key not in _predictions:
        q, t, S, de, ex, pwm = entry_pair(entry)
        _predictions[key] = predict_generic(q, t, S, de, ex, max_passes=max_passes, pwm=pwm)
    return _predictions[key]
