"""The scheme limits of call_init (aligner_amd/csrc/aln_scheme_rules.h) as figures, shared by the CPU test of the rules
(test_scheme_rules_cpu.py) and the GPU tests at the limits (test_value_limits_gpu.py), and an exact integer restatement of the
recurrences that shows how far |H| and the candidates of a cell actually go; and a count of the cells where the f64 tie rules
decide (candidates within f64::EPSILON of the maximum, H within 1e-12 of zero)."""
import numpy as np

EPS = 2.0 ** -52               # the reference's tie tolerance (enums.rs)
BEGIN = 3                      # direction code of a Beginning cell
INT_BOUND = 1 << 30            # integer kernels: maxabs * max_span < 2^30
FAST_BOUND = 1 << 28           # fast kernels (keys 4*H + tag in i32): maxabs * max_span < 2^28
FAST_SMIN, FAST_SMAX = -31, 32  # int8 profile 4*s - 2
FULL_R = 8                     # ALN_FULL_R: rows per lane of a full strip (a wave's profile is cols x 512 bytes)
MAX_DYADIC_K = 8

# the lopsided global pair of the penalty limits: N (query) much longer than M, so that the border -(N + 1) * del and H(M, N)
# come to about 0.99 of maxabs * span
LOPSIDED = (2000, 12)
# a wider pair that, in the same call, takes max_span past the last fast penalty of LOPSIDED but not past its last integer one
WIDE = (4000, 12)


def span(N, M):
    return N + M + 2


def last_below(bound, sp):
    """The largest integer d with d * sp < bound."""
    return (bound - 1) // sp


def fast_lds(rows, cols, pwm=False):
    """LDS bytes of S (as i32) and four waves' query profiles."""
    return ((rows * cols * 4 + 15) & ~15) + (0 if pwm else 4 * cols * 64 * FULL_R)


def int_extremes(q, t, dele, ext, S, local, legacy=False):
    """Largest |H| and largest |candidate| (top - p, left - p, diag + s) over every cell of the reference's recurrence, in
    Python integers (exact at any size).  Core: the penalty carried in visiting order (column by column), del after a
    Beginning cell (local only) and ext otherwise; global borders -x del, -y del and -(N + 1) del / -(M + 1) del at the two
    corners.  Legacy: del everywhere, local clamps at 0."""
    N, M = len(q), len(t)
    col = [0] * (M + 1)
    if not local:
        col = [-y * dele for y in range(M + 1)]
        col[M] = -(M + 1) * dele
    hmax = max(abs(v) for v in col)
    cmax = 0
    p = dele
    for x in range(1, N + 1):
        top = 0 if local else (-(N + 1) * dele if x == N else -x * dele)
        hmax = max(hmax, abs(top))
        new = [top]
        for y in range(1, M + 1):
            s = int(S[t[y - 1]][q[x - 1]])
            pen = dele if legacy else p
            a, b, c = new[y - 1] - pen, col[y] - pen, col[y - 1] + s
            cmax = max(cmax, abs(a), abs(b), abs(c))
            m = max(a, b, c)
            if legacy:
                if local:
                    m = max(m, 0)
            elif local:
                p = dele if m == 0 else ext
            else:
                p = ext
            new.append(m)
            hmax = max(hmax, abs(m))
        col = new
    return hmax, cmax


def tie_counts(H, D, q, t, dele, ext, S, local):
    """(cells with a candidate in (m - EPS, m), cells with 0 < |H| < 1e-12) of one pair, from the oracle's H and D.  Also checks
    that the recurrence re-evaluated here from H reproduces H: the penalty of a cell is del after a Beginning cell in visiting
    order (column by column) and ext otherwise."""
    M, N = len(t), len(q)
    prev = np.empty((M, N), dtype=np.int64)
    prev[1:, :] = D[1:M, 1:]
    prev[0, 1:] = D[M, 1:N]
    prev[0, 0] = BEGIN
    p = np.where(prev == BEGIN, float(dele), float(ext))
    top, left = H[:-1, 1:] - p, H[1:, :-1] - p
    diag = H[:-1, :-1] + S[np.ix_(t, q)]
    m = np.maximum(np.maximum(top, left), diag)
    assert (m == H[1:, 1:]).all()
    near = ((m > top) & (m - top < EPS)) | ((m > left) & (m - left < EPS))
    tiny = (m != 0) & (np.abs(m) < 1e-12)
    return int(near.sum()), int(tiny.sum())
