"""Every kernel route at the limits that decide it (aln_scheme_rules.h), against the CPU oracle: status, f, score, end and start
cells, aln_len and both aligned strings of every pair; for single pairs the whole D matrix too (and H where the generic kernels
serve it).  Every case also asserts the route it ran through flags (include/aligner_hip.h): bit 0 integer kernels, bit 1 the
single-pair route, bit 2 one workgroup per pair, bit 3 the fast integer kernels.
* int8 profile: entries -31 / 32 fast, -32 or 33 generic integer -- cooperative and lean batch builds, two pairs per wave, the
  single-pair route, both batch walks, PWM pair and windows;
* i32 keys / i32 H: del = ext at the last fast, first generic, last integer and first f64 value of a lopsided global pair whose
  border reaches 0.99 of maxabs * span; a wide pair moving a whole batch; zero and negative penalties;
* dyadic schemes: k = 8 against k = 9, the scaled bound on either side, a scaled scheme on exactly [-31, 32];
* LDS and size: alphabets of 30 and 31, 64 x 64 against 64 x 65, PWMs of 4 x 2000 (integer and real) against 4 x 2001;
* f64 ties: schemes whose cells hold candidates within f64::EPSILON of the maximum and H within 1e-12 of zero, counted here so
  that the test cannot pass vacuously, on the lean f64 batch strip, the generic kernels and a real-valued PWM."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from aligner_amd import _ffi, runtime
from aligner_amd.batch import PairBatch, align_batch
from aligner_amd.pwm import align_window_offsets
from scheme_limits import FAST_BOUND, INT_BOUND, LOPSIDED, WIDE, int_extremes, last_below, span, tie_counts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST, INT, F64 = "fast", "int", "f64"


def route_of(flags):
    flags = int(flags)
    if flags & _ffi.FLAG_FAST:
        assert flags & _ffi.FLAG_INTEGER, flags
        return FAST
    return INT if flags & _ffi.FLAG_INTEGER else F64


def scheme(lo, hi, A=4):
    """hi on the diagonal, lo everywhere else."""
    S = np.full((A, A), float(lo))
    np.fill_diagonal(S, float(hi))
    return S


def related(rng, n, m, A=4):
    """A query of n letters and a target of m letters made of runs copied from it (so that the matches add up) with some
    letters changed and random letters between the runs."""
    q = rng.integers(0, A, n).astype(np.uint8)
    t = []
    while len(t) < m:
        L = int(rng.integers(20, 120))
        s = int(rng.integers(0, max(1, n - L)))
        run = q[s:s + L].copy()
        mut = rng.random(len(run)) < 0.05
        run[mut] = rng.integers(0, A, int(mut.sum()))
        t.extend(run.tolist())
        t.extend(rng.integers(0, A, int(rng.integers(0, 6))).tolist())
    return q, np.array(t[:m], dtype=np.uint8)


def check_pair(orc, sem, q, t, dele, ext, S, route, want_h=False, **kw):
    """One pair through aln_align_pair against the oracle: summary, strings and the whole D (and H) matrix."""
    ref = orc.align(sem, q, t, dele, ext, S, want_matrices=True)
    assert ref["status"] == 0
    res, qa, ta, D, H = runtime.align_pair(sem, q, t, dele, ext, S, want_directions=True, want_h=want_h, **kw)
    assert res.status == 0
    assert route_of(res.flags) == route, (res.flags, route)
    assert (res.score, res.f) == (ref["score"], ref["f"])
    assert (res.end_y, res.end_x) == ref["end"] and (res.start_y, res.start_x) == ref["start"]
    assert res.aln_len == len(ref["qa"])
    assert qa.tolist() == ref["qa"].tolist() and ta.tolist() == ref["ta"].tolist()
    bad = np.argwhere(D != ref["D"])
    assert len(bad) == 0, "D differs first at (y,x)=%s" % (bad[0],)
    if want_h:
        bad = np.argwhere(H != ref["H"])
        assert len(bad) == 0, "H differs first at (y,x)=%s: gpu %r ref %r" % (bad[0], H[tuple(bad[0])], ref["H"][tuple(bad[0])])
    return res, ref


def check_results(orc, b, sem, dele, ext, S, results, strings_of, route):
    """A batch's summaries and strings (strings_of(i) -> (qa, ta)) against the oracle, and every pair's route."""
    ref, tb, tb_off = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, dele, ext, S, n_threads=8)
    for i in range(len(b)):
        r, g = ref[i], results[i]
        assert g["status"] == r.status == 0, i
        assert route_of(g["flags"]) == route, (i, g["flags"], route)
        assert (g["score"], g["f"], g["end_y"], g["end_x"], g["start_y"], g["start_x"], g["aln_len"]) == \
               (r.score, r.f, r.end_y, r.end_x, r.start_y, r.start_x, r.aln_len), i
        cap = int(b.q_len[i] + b.t_len[i]) + 2
        o = int(tb_off[i])
        qa, ta = strings_of(i)
        assert (qa == tb[o:o + r.aln_len]).all() and (ta == tb[o + cap:o + cap + r.aln_len]).all(), i
    return ref


def check_batch(orc, b, sem, dele, ext, S, route, **kw):
    got = align_batch(b, sem, dele, ext, S, **kw)
    check_results(orc, b, sem, dele, ext, S, got.results, got.aligned, route)
    return got


def check_pwm_pair(orc, seq, dele, ext, pwm, route, want_h):
    ref = orc.align_pwm(seq, dele, ext, pwm, want_matrices=True)
    res, numbered, qal, D, H = runtime.align_pwm(seq, dele, ext, pwm, want_directions=True, want_h=want_h)
    assert res.status == 0 and route_of(res.flags) == route, (res.flags, route)
    assert res.f == ref["f"]
    assert numbered.tolist() == ref["numbered"].tolist() and qal.tolist() == ref["qal"].tolist()
    assert (D == ref["D"]).all()
    if want_h:
        assert (H == ref["H"]).all()
    return ref


def check_windows(orc, seq, starts, lens, dele, ext, pwm, route):
    res, alns = align_window_offsets(seq, starts, lens, dele, ext, pwm)
    for i in range(len(starts)):
        s, L = int(starts[i]), int(lens[i])
        ref = orc.align_pwm(seq[s:s + L], dele, ext, pwm)
        assert res["status"][i] == 0 and route_of(res["flags"][i]) == route, (i, res["flags"][i], route)
        assert res["f"][i] == ref["f"] and alns[i].coords == ref["coords"], i
        assert alns[i].numbered.tolist() == ref["numbered"].tolist() and alns[i].query.tolist() == ref["qal"].tolist(), i
    return res


def unsupported(fn):
    with pytest.raises(ValueError, match="ERR_UNSUPPORTED"):
        fn()


# ---------------------------------------------------------------- int8 query profile: -31 .. 32
INT8_CASES = [((-31, 32), FAST), ((-32, 32), INT), ((-31, 33), INT)]

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[2])
from aligner_amd import _ffi
from aligner_amd.batch import PairBatch, align_batch
b = PairBatch(*[np.load(sys.argv[3])[k] for k in ("seqs", "q_off", "q_len", "t_off", "t_len")])
out = {}
for j, (lo, hi) in enumerate(((-31, 32), (-32, 32), (-31, 33))):
    S = np.full((4, 4), float(lo)); np.fill_diagonal(S, float(hi))
    r = align_batch(b, _ffi.CORE_LOCAL, 40, 3, S)
    out["results%d" % j] = r.results
    out["strings%d" % j] = np.concatenate([np.concatenate(r.aligned(i)) for i in range(len(b))])
np.savez(sys.argv[1], **out)
"""
PLAN = re.compile(r"aln plan: .* build (\w+)")


def large_pairs_batch(rng, n=24):
    """Few multi-strip pairs (M > 512): the fast batch kernel shares their strips (cooperative passes)."""
    return PairBatch.from_pairs([related(rng, int(rng.integers(600, 800)), int(rng.integers(900, 1200))) for _ in range(n)])


@pytest.mark.parametrize("lean", [0, 1])
def test_int8_profile_cooperative_and_lean_builds(orc, tmp_path, lean):
    """The cooperative build and the lean build (forced with ALN_COOP_LEAN, in a fresh process: the setting is read once)."""
    b = large_pairs_batch(np.random.default_rng(31))
    np.savez(tmp_path / "batch.npz", seqs=b.seqs, q_off=b.q_off, q_len=b.q_len, t_off=b.t_off, t_len=b.t_len)
    out = tmp_path / "out.npz"
    env = dict(os.environ, ALN_COOP_LEAN=str(lean), ALN_TRACE_PLAN="1")
    p = subprocess.run([sys.executable, "-c", CHILD, str(out), ROOT, str(tmp_path / "batch.npz")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    builds = PLAN.findall(p.stderr)
    # the plan is traced for calls that could share: the fast ones (the generic kernels have no cooperative build)
    assert builds == [("lean" if lean else "coop")], p.stderr
    got = np.load(out)
    for j, ((lo, hi), route) in enumerate(INT8_CASES):
        res, strings = got["results%d" % j], got["strings%d" % j]
        offs = np.concatenate([[0], np.cumsum(2 * res["aln_len"].astype(np.int64))])

        def strings_of(i):
            s = strings[offs[i]:offs[i + 1]]
            return s[:len(s) // 2], s[len(s) // 2:]
        assert ((res["flags"] & _ffi.FLAG_SINGLE) == 0).all()
        check_results(orc, b, _ffi.CORE_LOCAL, 40, 3, scheme(lo, hi), res, strings_of, route)


@pytest.mark.parametrize("lohi,route", INT8_CASES)
def test_int8_profile_duo_single_walks_and_pwm(orc, monkeypatch, lohi, route):
    lo, hi = lohi
    S = scheme(lo, hi)
    rng = np.random.default_rng(hi * 100 - lo)
    cus = runtime.device_info()["compute_units"]
    # two pairs per wave: core global, more than cus * 12 pairs of at most 256 x 1024
    pairs = [related(rng, int(rng.integers(100, 200)), int(rng.integers(100, 200))) for _ in range(cus * 12 + 100)]
    check_batch(orc, PairBatch.from_pairs(pairs), _ffi.CORE_GLOBAL, 40, 40, S, route)
    # the single-pair route (bit 1) -- with the fast kernels only; the others take the generic kernels
    q, t = related(rng, 900, 700)
    for sem in (_ffi.CORE_GLOBAL, _ffi.CORE_LOCAL):
        res, _ = check_pair(orc, sem, q, t, 40, 3 if sem == _ffi.CORE_LOCAL else 40, S, route)
        assert bool(res.flags & _ffi.FLAG_SINGLE) == (route == FAST)
    res, _ = check_pair(orc, _ffi.LEGACY_GLOBAL, q, t, 40, 40, S, route)
    # the batch walks: one wave per pair (few pairs) and one lane per pair (ALN_TB_WAVE=0)
    b = PairBatch.from_pairs([related(rng, int(rng.integers(50, 700)), int(rng.integers(50, 700))) for _ in range(300)])
    check_batch(orc, b, _ffi.CORE_LOCAL, 40, 3, S, route)
    monkeypatch.setenv("ALN_TB_WAVE", "0")
    check_batch(orc, b, _ffi.CORE_LOCAL, 40, 3, S, route)
    check_batch(orc, b, _ffi.LEGACY_LOCAL, 40, 40, S, route)
    monkeypatch.delenv("ALN_TB_WAVE")
    # PWM: one pair and a window batch; the PWM holds both extremes in every column
    W = 300
    pwm = np.full((4, W), float(lo))
    motif = rng.integers(0, 4, W)
    pwm[motif, np.arange(W)] = float(hi)
    seq = np.concatenate([rng.integers(0, 4, 200), motif, rng.integers(0, 4, 300)]).astype(np.uint8)
    ref = check_pwm_pair(orc, seq, 40, 3, pwm, route, want_h=False)
    assert ref["f"] == hi * W
    starts = np.arange(0, len(seq) - 330, 45, dtype=np.uint64)
    check_windows(orc, seq, starts, np.full(len(starts), 330, np.uint64), 40, 3, pwm, route)


# ---------------------------------------------------------------- i32 keys and i32 H
def lopsided(rng, n_pairs=1, N=LOPSIDED[0], M=LOPSIDED[1]):
    return [(rng.integers(0, 20, N).astype(np.uint8), rng.integers(0, 20, M).astype(np.uint8)) for _ in range(n_pairs)]


def penalty_limits():
    sp = span(*LOPSIDED)
    f, i = last_below(FAST_BOUND, sp), last_below(INT_BOUND, sp)
    return [(f, FAST), (f + 1, INT), (i, INT), (i + 1, F64)]


@pytest.mark.parametrize("d,route", penalty_limits())
@pytest.mark.parametrize("sem", [_ffi.CORE_GLOBAL, _ffi.CORE_LOCAL, _ffi.LEGACY_GLOBAL])
def test_penalty_limits_on_a_lopsided_pair(orc, blosum62, sem, d, route):
    """del = ext = d on 2000 x 12: the global border -(N + 1) d and H(M, N) reach 0.99 of d * span."""
    rng = np.random.default_rng(d % 1000)
    (q, t), = lopsided(rng)
    legacy = sem == _ffi.LEGACY_GLOBAL
    if legacy and route == F64:
        unsupported(lambda: runtime.align_pair(sem, q, t, d, d, blosum62))
        b = PairBatch.from_pairs(lopsided(rng, 3))
        unsupported(lambda: align_batch(b, sem, d, d, blosum62))
        return
    res, ref = check_pair(orc, sem, q, t, d, d, blosum62, route)
    if sem != _ffi.CORE_LOCAL:
        assert abs(ref["H"]).max() >= 0.99 * d * span(*LOPSIDED)
        assert abs(res.score) >= 0.98 * d * span(*LOPSIDED)
    # the generic kernels with the H dump (integer up to the last integer value, f64 past it)
    check_pair(orc, sem, q, t, d, d, blosum62, F64 if route == F64 else INT, want_h=True)
    # a batch of such pairs
    b = PairBatch.from_pairs(lopsided(rng, 40))
    check_batch(orc, b, sem, d, d, blosum62, route)


def test_one_wide_pair_moves_the_whole_batch(orc, blosum62):
    rng = np.random.default_rng(4014)
    d = last_below(FAST_BOUND, span(*LOPSIDED))
    pairs = lopsided(rng, 30)
    check_batch(orc, PairBatch.from_pairs(pairs), _ffi.CORE_GLOBAL, d, d, blosum62, FAST)
    wide = lopsided(rng, 1, *WIDE)
    assert d * span(*WIDE) >= FAST_BOUND and last_below(INT_BOUND, span(*WIDE)) >= d
    check_batch(orc, PairBatch.from_pairs(pairs + wide), _ffi.CORE_GLOBAL, d, d, blosum62, INT)
    di = last_below(INT_BOUND, span(*WIDE))
    hmax, _ = int_extremes(wide[0][0].tolist(), wide[0][1].tolist(), di, di, blosum62.tolist(), False)
    assert hmax >= 0.99 * di * span(*WIDE)
    check_batch(orc, PairBatch.from_pairs(pairs + wide), _ffi.CORE_GLOBAL, di, di, blosum62, INT)
    check_batch(orc, PairBatch.from_pairs(pairs + wide), _ffi.CORE_GLOBAL, di + 1, di + 1, blosum62, F64)


@pytest.mark.parametrize("sem", [_ffi.CORE_GLOBAL, _ffi.CORE_LOCAL, _ffi.LEGACY_GLOBAL, _ffi.LEGACY_LOCAL])
def test_zero_penalties(orc, blosum62, sem):
    rng = np.random.default_rng(0)
    q, t = rng.integers(0, 20, 300).astype(np.uint8), rng.integers(0, 20, 250).astype(np.uint8)
    check_pair(orc, sem, q, t, 0, 0, blosum62, FAST)
    check_pair(orc, sem, q, t, 0, 0, blosum62, INT, want_h=True)
    b = PairBatch.from_pairs([(rng.integers(0, 20, int(rng.integers(5, 400))).astype(np.uint8),
                               rng.integers(0, 20, int(rng.integers(5, 400))).astype(np.uint8)) for _ in range(50)])
    check_batch(orc, b, sem, 0, 0, blosum62, FAST)


def test_negative_penalties(orc, blosum62):
    """del = -1 (a gap is a reward): the reference accepts it and maxabs takes |del|.  Core local with del != ext runs the
    multi-pass route."""
    rng = np.random.default_rng(1)
    q, t = rng.integers(0, 20, 300).astype(np.uint8), rng.integers(0, 20, 250).astype(np.uint8)
    b = PairBatch.from_pairs([(rng.integers(0, 20, int(rng.integers(5, 400))).astype(np.uint8),
                               rng.integers(0, 20, int(rng.integers(5, 400))).astype(np.uint8)) for _ in range(50)])
    for sem, dele, ext in ((_ffi.CORE_GLOBAL, -1, -1), (_ffi.LEGACY_GLOBAL, -1, -1), (_ffi.CORE_LOCAL, -1, -1),
                           (_ffi.CORE_LOCAL, -1, 2), (_ffi.CORE_LOCAL, 2, -1)):
        check_pair(orc, sem, q, t, dele, ext, blosum62, FAST)
        check_pair(orc, sem, q, t, dele, ext, blosum62, INT, want_h=True)
        check_batch(orc, b, sem, dele, ext, blosum62, FAST)


# ---------------------------------------------------------------- dyadic schemes
def test_dyadic_limits(orc, blosum62):
    rng = np.random.default_rng(256)
    (q, t), = lopsided(rng)
    # k = 8 is filled by the integer kernels (scaled by 256), k = 9 by the f64 kernels; both equal the oracle on the real numbers
    S8, S9 = blosum62 + 2.0 ** -8, blosum62 + 2.0 ** -9
    for sem in (_ffi.CORE_GLOBAL, _ffi.CORE_LOCAL):
        check_pair(orc, sem, q, t, 11.5, 2.25, S8, INT)
        check_pair(orc, sem, q, t, 11.5, 2.25, S9, F64)
    # the scaled bound: X / 256 with X * span just under 2^30 stays integer, one step more goes to f64
    X = last_below(INT_BOUND, span(*LOPSIDED))
    for d, route in ((X / 256, INT), ((X + 1) / 256, F64)):
        for sem in (_ffi.CORE_GLOBAL, _ffi.CORE_LOCAL):
            check_pair(orc, sem, q, t, d, d, S8, route)
        check_batch(orc, PairBatch.from_pairs(lopsided(rng, 20)), _ffi.CORE_GLOBAL, d, d, S8, route)
    # ... and the fast bound on the scaled figures, with a scheme that scales onto [-31, 32]
    Sf = scheme(-31, 32) / 256
    Sf[0, 1] = 1.0 / 256
    Xf = last_below(FAST_BOUND, span(*LOPSIDED))
    qa = rng.integers(0, 4, LOPSIDED[0]).astype(np.uint8)
    ta = rng.integers(0, 4, LOPSIDED[1]).astype(np.uint8)
    check_pair(orc, _ffi.CORE_GLOBAL, qa, ta, Xf / 256, Xf / 256, Sf, FAST)
    check_pair(orc, _ffi.CORE_GLOBAL, qa, ta, (Xf + 1) / 256, (Xf + 1) / 256, Sf, INT)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_dyadic_scheme_on_the_int8_edges(orc, k):
    """A real-valued scheme that is -31 / 32 once scaled by 2^k runs fast; one step past either edge runs generic."""
    rng = np.random.default_rng(k)
    sc = 2.0 ** -k
    q, t = related(rng, 900, 700)
    b = PairBatch.from_pairs([related(rng, int(rng.integers(50, 600)), int(rng.integers(50, 600))) for _ in range(100)])
    for lo, hi, route in ((-31, 32, FAST), (-32, 32, INT), (-31, 33, INT)):
        S = scheme(lo, hi) * sc
        check_pair(orc, _ffi.CORE_LOCAL, q, t, 40 * sc + sc, 3 * sc, S, route)
        check_batch(orc, b, _ffi.CORE_LOCAL, 40 * sc + sc, 3 * sc, S, route)
        check_batch(orc, b, _ffi.CORE_GLOBAL, 5 * sc, 5 * sc, S, route)


# ---------------------------------------------------------------- LDS and matrix size
@pytest.mark.parametrize("A,route", [(30, FAST), (31, INT)])
def test_alphabet_30_and_31(orc, A, route):
    rng = np.random.default_rng(A)
    S = rng.integers(-6, 9, (A, A)).astype(np.float64)
    np.fill_diagonal(S, 12.0)
    q, t = related(rng, 800, 600, A)
    for sem in (_ffi.CORE_LOCAL, _ffi.CORE_GLOBAL, _ffi.LEGACY_LOCAL):
        check_pair(orc, sem, q, t, 7, 7 if sem != _ffi.CORE_LOCAL else 2, S, route)
    check_pair(orc, _ffi.CORE_LOCAL, q, t, 7, 2, S, INT, want_h=True)
    b = PairBatch.from_pairs([related(rng, int(rng.integers(5, 400)), int(rng.integers(5, 900)), A) for _ in range(60)])
    check_batch(orc, b, _ffi.CORE_LOCAL, 7, 2, S, route)
    check_batch(orc, b, _ffi.CORE_GLOBAL, 7, 7, S, route)


def test_matrix_size_limits(orc):
    rng = np.random.default_rng(64)
    S = rng.integers(-4, 6, (64, 64)).astype(np.float64)
    q, t = rng.integers(0, 64, 300).astype(np.uint8), rng.integers(0, 64, 200).astype(np.uint8)
    check_pair(orc, _ffi.CORE_LOCAL, q, t, 7, 2, S, INT)
    check_batch(orc, PairBatch.from_pairs([(q, t), (t, q)]), _ffi.CORE_GLOBAL, 7, 7, S, INT)
    S65 = np.zeros((64, 65))
    unsupported(lambda: runtime.align_pair(_ffi.CORE_LOCAL, q, t, 7, 2, S65))
    unsupported(lambda: align_batch(PairBatch.from_pairs([(q, t)]), _ffi.CORE_LOCAL, 7, 2, S65))


@pytest.mark.parametrize("kind,route", [("int", FAST), ("real", F64)])
def test_pwm_4_by_2000(orc, kind, route):
    """The widest PWM: S is 32 000 bytes as i32, 64 000 as f64 (next to nothing else in LDS).  One pair (fast / f64, and the
    generic kernels with H), a window batch and a scan score pass."""
    from aligner_amd.repeats import ScanBackend
    W = 2000
    rng = np.random.default_rng(2000)
    pwm = rng.integers(-3, 4, (4, W)).astype(np.float64) if kind == "int" else np.round(rng.normal(0, 1.2, (4, W)), 3)
    motif = np.argmax(pwm, axis=0).astype(np.uint8)
    seq = np.concatenate([rng.integers(0, 4, 300), motif[100:700], rng.integers(0, 4, 400)]).astype(np.uint8)
    check_pwm_pair(orc, seq, 5, 2, pwm, route, want_h=False)
    check_pwm_pair(orc, seq, 5, 2, pwm, INT if kind == "int" else F64, want_h=True)
    first, step, width = 0, 250, 600
    starts = np.arange(first, len(seq), step, dtype=np.uint64)
    lens = np.minimum(starts + np.uint64(width), np.uint64(len(seq))) - starts
    res = check_windows(orc, seq, starts, lens, 5, 2, pwm, route)
    with ScanBackend().scan(seq) as sc:
        f = sc.score(pwm, 5, 2, first, step, width)
    assert np.array_equal(f.view(np.uint64), res["f"].view(np.uint64))
    wide = np.zeros((4, W + 1))
    unsupported(lambda: runtime.align_pwm(seq, 5, 2, wide))
    unsupported(lambda: align_window_offsets(seq, starts, lens, 5, 2, wide))


# ---------------------------------------------------------------- f64 ties
def tie_schemes(blosum62):
    tenths = np.array([[0.3, -0.1, -0.2, -0.2], [-0.1, 0.3, -0.2, -0.2], [-0.2, -0.2, 0.3, -0.1], [-0.2, -0.2, -0.1, 0.3]])
    return [("tenths", tenths, 0.2, 0.1, 4), ("blosum62x0.3", blosum62 * 0.3, 3.3, 0.6, 20)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("sem", [_ffi.CORE_LOCAL, _ffi.CORE_GLOBAL])
def test_f64_near_ties(orc, blosum62, sem, which):
    name, S, dele, ext, A = tie_schemes(blosum62)[which]
    local = sem == _ffi.CORE_LOCAL
    rng = np.random.default_rng(which * 10 + sem)
    q, t = related(rng, 200, 200, A)
    # the generic kernels (one pair, H and D)
    _, ref = check_pair(orc, sem, q, t, dele, ext, S, F64, want_h=True)
    near, tiny = tie_counts(ref["H"], ref["D"], q, t, dele, ext, S, local)
    assert near > 0, name
    if local:
        assert tiny > 0, name
    # the lean f64 strip: a batch (more than four pairs: one wave per pair)
    pairs = [related(rng, int(rng.integers(100, 300)), int(rng.integers(100, 300)), A) for _ in range(40)]
    check_batch(orc, PairBatch.from_pairs(pairs), sem, dele, ext, S, F64)
    near = tiny = 0
    for qq, tt in pairs[:8]:
        r = orc.align(sem, qq, tt, dele, ext, S, want_matrices=True)
        n_, t_ = tie_counts(r["H"], r["D"], qq, tt, dele, ext, S, local)
        near, tiny = near + n_, tiny + t_
    assert near > 0 and (tiny > 0 or not local), name


def test_f64_near_ties_pwm(orc):
    """A real-valued PWM in tenths: one pair (generic kernels with H) and a window batch."""
    rng = np.random.default_rng(10)
    W = 200
    pwm = rng.choice([0.3, -0.1, -0.2], size=(4, W))
    motif = np.argmax(pwm, axis=0).astype(np.uint8)
    seq = np.concatenate([rng.integers(0, 4, 100), motif, rng.integers(0, 4, 150)]).astype(np.uint8)
    ref = check_pwm_pair(orc, seq, 0.2, 0.1, pwm, F64, want_h=True)
    check_pwm_pair(orc, seq, 0.2, 0.1, pwm, F64, want_h=False)
    near, tiny = tie_counts(ref["H"], ref["D"], np.arange(W), seq, 0.2, 0.1, pwm, True)
    assert near > 0 and tiny > 0
    starts = np.arange(0, len(seq) - 220, 10, dtype=np.uint64)
    check_windows(orc, seq, starts, np.full(len(starts), 220, np.uint64), 0.2, 0.1, pwm, F64)
