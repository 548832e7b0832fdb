"""Which kernel family a scoring scheme runs on (aln_scheme_rules.h, the arithmetic of call_init; no GPU): both sides of every
limit, at the exact threshold values -- computed here from max_span, not copied from the header.
* int8 query profile: entries -31 .. 32 fast, -32 or 33 not;
* i32 keys of the fast kernels: maxabs * max_span < 2^28; i32 H of the integer kernels: < 2^30 (past it core goes to f64 and
  legacy has no exact form);
* dyadic schemes: the smallest 2^k, k <= 8, kept only if the scaled scheme stays under 2^30;
* LDS: S and four waves' profiles in 64 KiB (alphabets of 30 fast, 31 not); matrix size: 4096 entries, PWMs 4 x 2000;
* force_f64, want_h, force_generic, force_serial.
And the claim behind the integer bounds: on the integer side of each limit, |H| and every candidate of the recurrence stay inside
i32 (for the fast kernels: 4 |H| + 3 does), evaluated exactly in Python integers on the shapes the GPU tests use."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from scheme_limits import (FAST_BOUND, FAST_SMAX, FAST_SMIN, INT_BOUND, LOPSIDED, MAX_DYADIC_K, WIDE, fast_lds, int_extremes,
                           last_below, span)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "aln_scheme_rules.h"
int main(int argc, char **argv)
{
    // <cases file> -> one line per case: fits all_int scale is_int fast maxabs smin smax fast_lds
    // a case: core pwm rows cols del ext max_span force_f64 want_h force_serial force_generic no_dyadic, then rows x cols values
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 3;
    int core, pwm, f64, wh, fs, fg, nd;
    unsigned rows, cols;
    double del, ext;
    unsigned long long sp;
    while (fscanf(f, "%d %d %u %u %lf %lf %llu %d %d %d %d %d", &core, &pwm, &rows, &cols, &del, &ext, &sp, &f64, &wh, &fs, &fg, &nd) == 12) {
        std::vector<double> md((size_t)rows * cols);
        for (double &v : md)
            if (fscanf(f, "%lf", &v) != 1) return 4;
        const bool fits = aln_matrix_fits(pwm != 0, rows, cols);
        AlnScheme s = aln_scheme_scan(core != 0, del, ext, md.data(), md.size());
        aln_scheme_dyadic(s, core != 0, f64 != 0, wh != 0, nd != 0, del, ext, md.data(), md.size(), sp);
        aln_scheme_route(s, pwm != 0, rows, cols, sp, f64 != 0, wh != 0, fs != 0, fg != 0, 8u);   // ALN_FULL_R
        printf("%d %d %.17g %d %d %.17g %.17g %.17g %llu\n", fits ? 1 : 0, s.all_int ? 1 : 0, s.scale, s.is_int ? 1 : 0, s.fast ? 1 : 0,
               s.maxabs, s.smin, s.smax, (unsigned long long)s.fast_lds);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def classify(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the scheme-rule driver" % cxx)
    d = tmp_path_factory.mktemp("scheme_rules")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), str(src), "-o", str(exe)])
    counter = [0]

    def call(S, dele, ext, max_span, core=True, pwm=False, force_f64=False, want_h=False, force_serial=False,
             force_generic=False, no_dyadic=False):
        S = np.atleast_2d(np.asarray(S, dtype=np.float64))
        counter[0] += 1
        path = d / ("case%d.txt" % counter[0])
        flags = [int(bool(v)) for v in (force_f64, want_h, force_serial, force_generic, no_dyadic)]
        head = [int(core), int(pwm), S.shape[0], S.shape[1], repr(float(dele)), repr(float(ext)), int(max_span)] + flags
        path.write_text(" ".join(map(str, head)) + "\n" + " ".join(repr(float(v)) for v in S.ravel()) + "\n")
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 9, out
        return dict(fits=out[0] == "1", all_int=out[1] == "1", scale=float(out[2]), is_int=out[3] == "1", fast=out[4] == "1",
                    maxabs=float(out[5]), smin=float(out[6]), smax=float(out[7]), fast_lds=int(out[8]))
    return call


def route(r):
    return "fast" if r["fast"] else "int" if r["is_int"] else "f64"


SMALL = np.array([[5.0, -4.0], [-4.0, 5.0]])


def test_penalty_bounds_on_the_lopsided_pair(classify, blosum62):
    """Pairs of 2000 x 12 (span 2014): del = ext = 133284 fast, 133285 generic integer, 533138 integer, 533139 f64 (core) and
    UNSUPPORTED (legacy, which has no f64 form: call_init answers it for every scheme that is not is_int)."""
    sp = span(*LOPSIDED)
    assert sp == 2014
    last_fast, last_int = last_below(FAST_BOUND, sp), last_below(INT_BOUND, sp)
    assert (last_fast, last_int) == (133284, 533138)
    for core in (True, False):
        want = {last_fast: "fast", last_fast + 1: "int", last_int: "int", last_int + 1: "f64"}
        for d, w in want.items():
            r = classify(blosum62, d, d, sp, core=core)
            assert route(r) == w, (core, d, r)
            assert r["maxabs"] == d
    # only the largest |value| counts, whichever of del, ext and S it is -- and its sign does not matter
    assert route(classify(blosum62, 11, last_fast + 1, sp)) == "int"
    assert route(classify(blosum62, -(last_fast + 1), 2, sp)) == "int"
    assert route(classify(blosum62, -last_fast, -last_fast, sp)) == "fast"
    assert route(classify(blosum62, 0, 0, sp)) == "fast"
    assert route(classify(blosum62, -1, 0, sp)) == "fast"
    # one wide pair decides for the whole call: a 4000 x 12 pair next to the lopsided ones
    wide = span(*WIDE)
    assert route(classify(blosum62, last_fast, last_fast, wide)) == "int"
    assert route(classify(blosum62, last_below(FAST_BOUND, wide), last_below(FAST_BOUND, wide), wide)) == "fast"
    assert route(classify(blosum62, last_below(INT_BOUND, wide), last_below(INT_BOUND, wide), wide)) == "int"
    assert route(classify(blosum62, last_int, last_int, wide)) == "f64"
    # the bound is strict: d * span == 2^28 exactly is not fast (span 2^12 + 2 + 2, d = 2^16)
    assert route(classify(SMALL, 1 << 16, 1 << 16, 1 << 12)) == "int"
    assert route(classify(SMALL, (1 << 16) - 1, (1 << 16) - 1, 1 << 12)) == "fast"
    assert route(classify(SMALL, 1 << 18, 1 << 18, 1 << 12)) == "f64"
    assert route(classify(SMALL, (1 << 18) - 1, (1 << 18) - 1, 1 << 12)) == "int"


def test_int8_profile_range(classify):
    sp = span(300, 400)
    for lo, hi, w in ((FAST_SMIN, FAST_SMAX, "fast"), (FAST_SMIN - 1, FAST_SMAX, "int"), (FAST_SMIN, FAST_SMAX + 1, "int"),
                      (-32, 33, "int")):
        S = np.full((4, 4), float(lo))
        np.fill_diagonal(S, float(hi))
        r = classify(S, 11, 2, sp)
        assert route(r) == w, (lo, hi, r)
        assert (r["smin"], r["smax"]) == (lo, hi)
    # a matrix of positive entries only: smin counts from 0 (and smax for a negative one)
    r = classify(np.full((4, 4), 32.0), 0, 0, sp)
    assert route(r) == "fast" and r["smin"] == 0.0
    r = classify(np.full((4, 4), -31.0), 40, 40, sp)
    assert route(r) == "fast" and r["smax"] == 0.0


def test_lds_and_matrix_size(classify):
    sp = span(300, 400)
    assert fast_lds(30, 30) <= 65536 < fast_lds(31, 31)
    for A, w in ((30, "fast"), (31, "int")):
        r = classify(np.eye(A) * 6 - 2, 11, 2, sp)
        assert route(r) == w and r["fast_lds"] == fast_lds(A, A)
    # the profiles take 2 KiB per column: 31 columns fit beside a small S, 32 do not
    assert route(classify(np.ones((4, 31)), 3, 1, sp)) == "fast" and route(classify(np.ones((4, 32)), 3, 1, sp)) == "int"
    assert fast_lds(1, 31) <= 65536 < fast_lds(1, 32)
    assert route(classify(np.ones((1, 31)), 3, 1, sp)) == "fast" and route(classify(np.ones((1, 32)), 3, 1, sp)) == "int"
    assert classify(np.ones((64, 64)), 3, 1, sp)["fits"]
    assert not classify(np.ones((64, 65)), 3, 1, sp)["fits"]
    assert not classify(np.ones((4097, 1)), 3, 1, sp)["fits"]
    # position-weight matrices: no profiles in LDS -- 4 x 2000 fits (S as i32: 32 000 bytes), 4 x 2001 is refused
    pw = span(2000, 500)
    r = classify(np.ones((4, 2000)), 3, 1, pw, pwm=True)
    assert r["fits"] and route(r) == "fast" and r["fast_lds"] == fast_lds(4, 2000, pwm=True) == 32000
    assert route(classify(np.full((4, 2000), 0.25), 3, 1, pw, pwm=True)) == "fast"      # dyadic k = 2
    assert route(classify(np.full((4, 2000), 0.3), 3, 1, pw, pwm=True)) == "f64"
    assert not classify(np.ones((4, 2001)), 3, 1, pw, pwm=True)["fits"]
    # as a substitution matrix 4 x 2000 is too large
    assert not classify(np.ones((4, 2000)), 3, 1, pw)["fits"]


def test_dyadic_scale(classify, blosum62):
    sp = span(*LOPSIDED)
    for k in range(1, MAX_DYADIC_K + 1):
        r = classify(blosum62 + 2.0 ** -k, 11, 2, sp)
        assert r["scale"] == 2.0 ** k and r["all_int"] and r["is_int"] and r["maxabs"] == 11 * 2 ** k + 1, k
    # k = 8 is the last: a scheme in 2^-9 stays real-valued (f64)
    S8 = np.array([[1.0 + 2.0 ** -8, -1.0], [-1.0, 1.0]])
    S9 = np.array([[1.0 + 2.0 ** -9, -1.0], [-1.0, 1.0]])
    r8, r9 = classify(S8, 2, 1, span(300, 300)), classify(S9, 2, 1, span(300, 300))
    assert r8["scale"] == 256.0 and r8["is_int"] and r8["maxabs"] == 2 * 256
    assert r9["scale"] == 1.0 and not r9["all_int"] and route(r9) == "f64"
    # the smallest k wins: a scheme in quarters is scaled by 4, not 8
    assert classify(np.array([[0.25, -0.5]]), 1.5, 0.75, 100)["scale"] == 4.0
    # the scaled bound: del = X / 256 with X * span just under 2^30 is kept (generic integer), one step more is not (f64)
    X = last_below(INT_BOUND, sp)
    S = np.array([[1.0 + 2.0 ** -8, -1.0], [-1.0, 1.0]])
    r = classify(S, X / 256, X / 256, sp)
    assert r["scale"] == 256.0 and r["maxabs"] == X and route(r) == "int"
    r = classify(S, (X + 1) / 256, (X + 1) / 256, sp)
    assert r["scale"] == 1.0 and route(r) == "f64"
    # ... and the fast bound on the scaled figures
    Xf = last_below(FAST_BOUND, sp)
    S = np.array([[32.0, -31.0], [-31.0, 1.0]]) / 256           # scaled: on [-31, 32]
    assert route(classify(S, Xf / 256, Xf / 256, sp)) == "fast"
    assert route(classify(S, (Xf + 1) / 256, (Xf + 1) / 256, sp)) == "int"
    # a scaled scheme that lands exactly on [-31, 32] runs fast; one step further out does not
    for k in (1, 2, 3):
        lo, hi = FAST_SMIN / 2 ** k, FAST_SMAX / 2 ** k
        S = np.array([[hi, lo], [lo, hi]])
        r = classify(S, 1.5, 0.5, span(500, 500))
        assert r["scale"] == 2.0 ** k and (r["smin"], r["smax"]) == (FAST_SMIN, FAST_SMAX) and route(r) == "fast", k
        S = np.array([[hi + 2.0 ** -k, lo], [lo, hi]])
        assert route(classify(S, 1.5, 0.5, span(500, 500))) == "int", k
        S = np.array([[hi, lo - 2.0 ** -k], [lo, hi]])
        assert route(classify(S, 1.5, 0.5, span(500, 500))) == "int", k
    # legacy semantics have no dyadic form: ext is not looked at, but del and S must be integral (call_init: INVALID_ARGUMENT)
    r = classify(np.array([[1.5, -1.0], [-1.0, 1.0]]), 2, 0.5, 100, core=False)
    assert not r["all_int"] and r["scale"] == 1.0
    assert classify(SMALL, 3, 0.5, 100, core=False)["all_int"]


def test_switches(classify, blosum62):
    sp = span(300, 400)
    half = blosum62 / 2
    assert route(classify(blosum62, 11, 2, sp)) == "fast"
    assert route(classify(blosum62, 11, 2, sp, force_f64=True)) == "f64"
    r = classify(half, 5.5, 1, sp, force_f64=True)
    assert r["scale"] == 1.0 and route(r) == "f64"
    # want_h: the integer kernels that can dump H (generic), and no dyadic scale (the dump is what the kernels computed)
    r = classify(blosum62, 11, 2, sp, want_h=True)
    assert route(r) == "int"
    r = classify(half, 5.5, 1, sp, want_h=True)
    assert r["scale"] == 1.0 and route(r) == "f64"
    assert route(classify(half, 5.5, 1, sp)) == "fast"
    assert route(classify(half, 5.5, 1, sp, no_dyadic=True)) == "f64"
    assert route(classify(blosum62, 11, 2, sp, force_generic=True)) == "int"
    assert route(classify(blosum62, 11, 2, sp, force_serial=True)) == "int"
    # a call without a pair (max_span 0) is classified by its numbers alone
    assert route(classify(blosum62, 11, 2, 0)) == "fast"


@pytest.mark.parametrize("sem", ["core_global", "core_local", "legacy_global", "legacy_local"])
def test_integer_side_stays_inside_i32(blosum62, sem):
    """At the last fast and the last integer penalty of the lopsided pair the exact recurrence stays inside what the kernels
    hold: every candidate and |H| below 2^31 on the integer kernels, 4 |H| + 3 (the fast kernels' keys) below 2^31 -- and the
    global pair does come close to the bound (|H| at least 0.99 of maxabs * span), so the bound has no slack to hide in."""
    local, legacy = sem.endswith("local"), sem.startswith("legacy")
    N, M = LOPSIDED
    sp = span(N, M)
    rng = np.random.default_rng(2014)
    q = rng.integers(0, 20, N).tolist()
    t = q[:M] if local else rng.integers(0, 20, M).tolist()
    for d, bound in ((last_below(FAST_BOUND, sp), FAST_BOUND), (last_below(INT_BOUND, sp), INT_BOUND)):
        hmax, cmax = int_extremes(q, t, d, d, blosum62.tolist(), local, legacy)
        assert hmax < bound and cmax < 2 ** 31, (d, hmax, cmax)
        if bound == FAST_BOUND:
            assert 4 * hmax + 3 < 2 ** 31 and 4 * cmax + 3 < 2 ** 31
        if not local:
            assert hmax >= 0.99 * d * sp, (d, hmax)
        else:
            assert hmax <= 11 * M
    # the wide pair of the mixed batch moves the whole call to the bound of its own span
    wide = span(*WIDE)
    d = last_below(INT_BOUND, wide)
    if not local:
        hmax, cmax = int_extremes(rng.integers(0, 20, WIDE[0]).tolist(), t, d, d, blosum62.tolist(), local, legacy)
        assert 0.99 * d * wide <= hmax < INT_BOUND and cmax < 2 ** 31
