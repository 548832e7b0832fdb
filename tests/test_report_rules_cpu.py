"""The rule of aln_seqset_held_report / aln_seqset_held_filter (aln_report_rules.h; no GPU): the header compiled into a driver with
the host compiler and checked against the numpy restatement in report_ref.py, the model tied to Alignment.get_alignment, the filter
at exact ties, the invariants of the counts on oracle alignments, the constructed cases of the GPU test shown to be what they claim,
the records' layouts, the exports and their argument types, the refusals that need no device and those of `allpairs`."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle  # noqa: E402
import report_ref  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import allpairs  # noqa: E402
from aligner_amd import seqset as seqset_module  # noqa: E402
from aligner_amd.alignment import Alignment  # noqa: E402
from aligner_amd.enums import Protein  # noqa: E402
from aligner_amd.matrices import get_blosum62  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["columns", "identical", "positive", "mismatch", "q_gap", "t_gap", "q_gap_open", "t_gap_open", "status", "reserved"]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <vector>
#include "aln_report_rules.h"
typedef unsigned long long ull;
static_assert(sizeof(aln_hit_report) == 40, "aln_hit_report");
static_assert(sizeof(aln_hit_filter) == 32, "aln_hit_filter");
static double from_bits(ull b) { uint64_t x = b; double v; memcpy(&v, &x, 8); return v; }
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "layout")) {
        printf("%u %u\n", (unsigned)sizeof(aln_hit_report), (unsigned)sizeof(aln_hit_filter));
        printf("%u %u %u %u %u %u %u %u %u %u\n", (unsigned)offsetof(aln_hit_report, columns), (unsigned)offsetof(aln_hit_report, identical),
               (unsigned)offsetof(aln_hit_report, positive), (unsigned)offsetof(aln_hit_report, mismatch), (unsigned)offsetof(aln_hit_report, q_gap),
               (unsigned)offsetof(aln_hit_report, t_gap), (unsigned)offsetof(aln_hit_report, q_gap_open), (unsigned)offsetof(aln_hit_report, t_gap_open),
               (unsigned)offsetof(aln_hit_report, status), (unsigned)offsetof(aln_hit_report, reserved));
        printf("%u %u %u %u %u\n", (unsigned)offsetof(aln_hit_filter, min_identity), (unsigned)offsetof(aln_hit_filter, min_q_cover),
               (unsigned)offsetof(aln_hit_filter, min_t_cover), (unsigned)offsetof(aln_hit_filter, min_columns), (unsigned)offsetof(aln_hit_filter, reserved));
        return 0;
    }
    if (!strcmp(argv[1], "count")) {
        // stdin: <rows> <cols> <row_stride>, rows * row_stride entries as bits; then per case <flags> <status> <blank> <len>, the
        // query's codes, the target's codes
        unsigned rows, cols, stride;
        if (scanf("%u %u %u", &rows, &cols, &stride) != 3) return 3;
        std::vector<double> m((size_t)rows * stride);
        for (double &v : m) { ull b; if (scanf("%llx", &b) != 1) return 3; v = from_bits(b); }
        if ((ull)rows * cols > ALN_REPORT_MAX_BITS) return 6;
        std::vector<uint32_t> bits(aln_report_words(rows, cols) + 1, 0xdeadbeefu);
        aln_report_table(m.data(), rows, cols, stride, bits.data());
        if (bits.back() != 0xdeadbeefu) return 7;
        unsigned flags, blank, len; int status;
        while (scanf("%u %d %u %u", &flags, &status, &blank, &len) == 4) {
            std::vector<uint8_t> x(len + 1), y(len + 1);
            for (unsigned j = 0; j < len; ++j) { unsigned v; if (scanf("%u", &v) != 1) return 4; x[j] = (uint8_t)v; }
            for (unsigned j = 0; j < len; ++j) { unsigned v; if (scanf("%u", &v) != 1) return 4; y[j] = (uint8_t)v; }
            const aln_hit_report a = aln_report_count(x.data(), y.data(), len, status, flags, blank, bits.data(), rows, cols);
            // the same from 64 accumulators, accumulator l taking columns l, l + 64, ..., folded at 32 .. 1 (the kernel's shape)
            aln_hit_report lane[64];
            const uint32_t n = aln_report_columns(len, flags);
            for (unsigned l = 0; l < 64; ++l) {
                lane[l] = aln_report_empty(status);
                for (uint32_t j = l; status == ALN_OK && j < n; j += 64) {
                    const uint32_t prev = j ? aln_report_class_of(x[j - 1], y[j - 1], blank, bits.data(), rows, cols) : (uint32_t)ALN_REPORT_NONE;
                    aln_report_take(&lane[l], aln_report_class_of(x[j], y[j], blank, bits.data(), rows, cols), prev);
                }
            }
            for (unsigned w = 32; w >= 1; w >>= 1) for (unsigned l = 0; l < w; ++l) lane[l] = aln_report_fold(lane[l], lane[l + w]);
            if (memcmp(&a, &lane[0], sizeof a)) return 5;
            printf("%u %u %u %u %u %u %u %u %d %u\n", a.columns, a.identical, a.positive, a.mismatch, a.q_gap, a.t_gap, a.q_gap_open, a.t_gap_open,
                   a.status, a.reserved);
        }
        return 0;
    }
    if (!strcmp(argv[1], "keep")) {
        // stdin per case: the record's ten words, N, M, the three thresholds as bits, min_columns
        aln_hit_report r; aln_hit_filter f; unsigned N, M; ull a, b, c;
        while (scanf("%u %u %u %u %u %u %u %u %d %u %u %u %llx %llx %llx %u", &r.columns, &r.identical, &r.positive, &r.mismatch, &r.q_gap, &r.t_gap,
                     &r.q_gap_open, &r.t_gap_open, &r.status, &r.reserved, &N, &M, &a, &b, &c, &f.min_columns) == 16) {
            f.min_identity = from_bits(a); f.min_q_cover = from_bits(b); f.min_t_cover = from_bits(c); f.reserved = 0;
            printf("%d\n", aln_report_keep(r, f, N, M) ? 1 : 0);
        }
        return 0;
    }
    return 2;
}
"""

C99 = r"""
#include <stddef.h>
#include "aligner_hip.h"
#define PIN(name, cond) typedef char pin_##name[(cond) ? 1 : -1]
PIN(size, sizeof(aln_hit_report) == 40);
PIN(status, offsetof(aln_hit_report, status) == 32);
PIN(filter, sizeof(aln_hit_filter) == 32);
PIN(min_columns, offsetof(aln_hit_filter, min_columns) == 24);
PIN(flag, ALN_REPORT_SKIP_SEED == 1u);
int (*const held_report)(aln_seqset *, const aln_params *, uint32_t, const uint32_t *, uint64_t, aln_hit_report *) = aln_seqset_held_report;
int (*const held_filter)(aln_seqset *, const aln_params *, uint32_t, const aln_hit_filter *, uint32_t *, aln_hit_report *, uint64_t,
                         uint64_t *) = aln_seqset_held_filter;
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the report-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("report_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src,
                           "-o", exe])
    return exe


def bits(f):
    return struct.unpack("<Q", struct.pack("<d", float(f)))[0]


def run_count(drv, matrix, cases, stride=None):
    """cases: (qa, ta, flags, status, blank) -> records as report_ref.RECORD"""
    m = np.asarray(matrix, dtype=np.float64)
    stride = m.shape[1] if stride is None else stride
    padded = np.full((m.shape[0], stride), -7.0)
    padded[:, :m.shape[1]] = m
    text = ["%d %d %d" % (m.shape[0], m.shape[1], stride), " ".join("%x" % bits(v) for v in padded.ravel())]
    for qa, ta, flags, status, blank in cases:
        text.append("%d %d %d %d" % (flags, status, blank, len(qa)))
        text.append(" ".join(str(int(v)) for v in qa))
        text.append(" ".join(str(int(v)) for v in ta))
    out = subprocess.run([drv, "count"], check=True, capture_output=True, text=True, input="\n".join(text) + "\n").stdout.splitlines()
    assert len(out) == len(cases)
    rec = np.zeros(len(cases), dtype=report_ref.RECORD)
    for i, line in enumerate(out):
        rec[i] = tuple(int(v) for v in line.split())
    return rec


def run_keep(drv, cases):
    """cases: (record, N, M, min_identity, min_q_cover, min_t_cover, min_columns) -> bools"""
    text = []
    for r, N, M, a, b, c, mc in cases:
        text.append(" ".join(str(int(r[n])) for n in FIELDS) + " %d %d %x %x %x %d" % (N, M, bits(a), bits(b), bits(c), mc))
    out = subprocess.run([drv, "keep"], check=True, capture_output=True, text=True, input="\n".join(text) + "\n").stdout.split()
    assert len(out) == len(cases)
    return np.array([v == "1" for v in out])


def awkward_matrix(rng, rows, cols):
    """entries 0.0, -0.0, NaN, negative and positive in equal parts"""
    pool = np.array([0.0, -0.0, float("nan"), -1.0, -0.25, 3.0, float("-inf"), float("inf"), 5e-324, -5e-324])
    return pool[rng.integers(0, len(pool), (rows, cols))]


def random_strings(rng, n, volume, blank):
    """two strings over {residues, blank}: runs of gaps on either side, both-blank columns, matches"""
    x = rng.integers(0, volume, n)
    y = np.where(rng.random(n) < 0.4, x, rng.integers(0, volume, n))
    for s in (x, y):
        j = 0
        while j < n:
            if rng.random() < 0.12:
                run = int(rng.integers(1, 6))
                s[j:j + run] = blank
                j += run
            j += 1
    return x.astype(np.uint8), y.astype(np.uint8)


# ---------------------------------------------------------------- the rule as code against the model
def test_layouts(driver, tmp_path):
    out = subprocess.run([driver, "layout"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ["40", "32"]
    assert [int(v) for v in out[1].split()] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    assert [int(v) for v in out[2].split()] == [0, 8, 16, 24, 28]
    assert C.sizeof(_ffi.HitReport) == seqset_module.REPORT_DTYPE.itemsize == report_ref.RECORD.itemsize == 40
    assert C.sizeof(_ffi.HitFilter) == 32
    assert [n for n, _ in _ffi.HitReport._fields_] == list(seqset_module.REPORT_DTYPE.names) == list(report_ref.RECORD.names) == FIELDS
    assert [getattr(_ffi.HitReport, n).offset for n in FIELDS] == [seqset_module.REPORT_DTYPE.fields[n][1] for n in FIELDS]
    assert [(n, getattr(_ffi.HitFilter, n).offset) for n, _ in _ffi.HitFilter._fields_] == \
        [("min_identity", 0), ("min_q_cover", 8), ("min_t_cover", 16), ("min_columns", 24), ("reserved", 28)]
    assert _ffi.REPORT_SKIP_SEED == report_ref.SKIP_SEED == 1
    # the public header alone, as C99: the same pins, and the exports' types
    cc = os.environ.get("CC", "gcc")
    src = str(tmp_path / "pin.c")
    with open(src, "w") as fh:
        fh.write(C99)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "pin.o")])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_driver_equals_model_on_random_strings(driver, seed):
    """1 200 string pairs per seed over {residues, blank}, lengths 0 .. 200, both flag values, matrices holding 0.0, -0.0, NaN and
    negative entries (one of them with a row stride beyond its columns); every class occurs, and both kinds of gap open."""
    rng = np.random.default_rng(seed)
    seen = np.zeros(8, dtype=np.int64)
    for rows, cols, stride, blank in ((24, 24, 24, 98), (5, 7, 11, 98), (90, 91, 91, 255)):
        m = awkward_matrix(rng, rows, cols)
        volume = min(rows, cols) + (2 if rows < 10 else 0)            # (the small one: some codes beyond the matrix)
        cases = []
        for i in range(400):
            n = int(rng.integers(0, 201)) if i >= 8 else (0, 1, 2, 63, 64, 65, 128, 200)[i]
            x, y = random_strings(rng, n, volume, blank)
            cases.append((x, y, i & 1, 0, blank))
            if i % 50 == 0:
                cases.append((x, y, i & 1, _ffi.ERR_NO_POSITIVE_CELL, blank))
        got = run_count(driver, m, cases, stride)
        for (x, y, flags, status, b), g in zip(cases, got):
            want = report_ref.report(x, y, m, flags, status, b)
            assert g.tobytes() == want.tobytes(), (len(x), flags, status, g, want)
            seen[:7] += [int(g[n]) for n in FIELDS[1:8]]
            seen[7] += 1
    assert (seen > 0).all()


def test_zero_minus_zero_and_nan_entries(driver):
    """S[y][x] >= 0.0 as a plain compare: 0.0 and -0.0 are positive, NaN and -5e-324 are not; element [t][q] is row t, column q"""
    m = np.array([[9.0, 0.0, -0.0], [float("nan"), 9.0, -5e-324], [5e-324, -1.0, 9.0]])
    x = np.array([1, 2, 0, 2, 0, 1], dtype=np.uint8)                  # query codes: columns
    y = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint8)                  # target codes: rows
    got = run_count(driver, m, [(x[i:i + 1], y[i:i + 1], 0, 0, 98) for i in range(6)])
    assert got["positive"].tolist() == [1, 1, 0, 0, 1, 0] and got["mismatch"].tolist() == [0, 0, 1, 1, 0, 1]
    assert report_ref.classes(x, y, m).tolist() == [1, 1, 2, 2, 1, 2]


def test_model_counts_the_reference_midline():
    """without the flag, identical / positive are the residue / Pos symbols of Alignment.get_alignment on the same strings, and
    every other column is a Blank of it"""
    rng = np.random.default_rng(7)
    blank, pos = Protein.blank(), Protein.pos()
    for m in (get_blosum62(), awkward_matrix(rng, 24, 24)):
        for _ in range(300):
            x, y = random_strings(rng, int(rng.integers(0, 201)), 24, blank)
            mid = Alignment(Protein, x, y, ((1, 1), (1, 1)), 0.0).get_alignment(m)
            r = report_ref.report(x, y, m, 0)
            both_blank = int(((x == blank) & (y == blank)).sum())
            assert int(r["identical"]) == int(((mid != pos) & (mid != blank)).sum())
            assert int(r["positive"]) == int((mid == pos).sum())
            assert int(r["mismatch"]) + int(r["q_gap"]) + int(r["t_gap"]) + both_blank == int((mid == blank).sum())


# ---------------------------------------------------------------- the filter rule at exact ties
def rec(**kw):
    r = np.zeros((), dtype=report_ref.RECORD)
    for k, v in kw.items():
        r[k] = v
    return r


def test_filter_at_exact_ties(driver):
    nan, up = float("nan"), float(np.nextafter(0.5, 1.0))
    r = rec(columns=8, identical=4, q_gap=2, t_gap=1)
    cases = [
        (r, 12, 14, 0.5, 0.0, 0.0, 0, True),                          # 4 >= 0.5 * 8
        (r, 12, 14, up, 0.0, 0.0, 0, False),
        (r, 12, 14, nan, 0.0, 0.0, 0, False),
        (r, 12, 14, 0.0, nan, 0.0, 0, False),
        (r, 12, 14, 0.0, 0.0, nan, 0, False),
        (r, 12, 14, 0.0, 0.5, 0.0, 0, True),                          # 8 - 2 >= 0.5 * 12
        (r, 12, 14, 0.0, up, 0.0, 0, False),
        (r, 12, 14, 0.0, 0.0, 0.5, 0, True),                          # 8 - 1 >= 0.5 * 14
        (r, 12, 14, 0.0, 0.0, up, 0, False),
        (r, 12, 14, 0.0, 0.0, 0.0, 8, True),
        (r, 12, 14, 0.0, 0.0, 0.0, 9, False),
        (r, 12, 14, 0.0, 0.0, 0.0, 7, True),
        (r, 12, 14, 0.5, 0.5, 0.5, 8, True),
        (r, 12, 14, float("-inf"), -1.0, -0.0, 0, True),
        (rec(columns=8, identical=8, status=_ffi.ERR_NO_POSITIVE_CELL), 8, 8, 0.0, 0.0, 0.0, 0, False),
        (rec(), 5, 5, 0.0, 0.0, 0.0, 0, True),                        # no column: 0 >= 0 * 0
        (rec(), 5, 5, 0.1, 0.0, 0.0, 0, True),                        # 0 >= 0.1 * 0
        (rec(), 5, 5, 0.0, 0.1, 0.0, 0, False),
        (rec(), 0, 0, float("inf"), 0.0, 0.0, 0, False),              # inf * 0 is NaN
        (rec(columns=3, identical=1), 3, 3, 1.0 / 3.0, 1.0, 1.0, 3, True),   # (1/3) * 3 rounds to 1.0
    ]
    got = run_keep(driver, [c[:7] for c in cases])
    assert got.tolist() == [c[7] for c in cases]
    for c in cases:
        assert bool(report_ref.keep(np.array([c[0]]), [c[1]], [c[2]], c[3], c[4], c[5], c[6])[0]) == c[7], c


def test_filter_driver_equals_model_on_random_records(driver):
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(2000):
        cols = int(rng.integers(0, 60))
        ident = int(rng.integers(0, cols + 1))
        qg = int(rng.integers(0, cols - ident + 1))
        tg = int(rng.integers(0, cols - ident - qg + 1))
        r = rec(columns=cols, identical=ident, q_gap=qg, t_gap=tg, status=0 if rng.random() < 0.95 else 4)
        th = [float(rng.choice([0.0, 0.25, 1.0 / 3.0, 0.5, 0.7, 1.0, 1.1, float("nan")], p=[.3, .1, .1, .2, .1, .1, .05, .05])) for _ in range(3)]
        cases.append((r, int(rng.integers(0, 60)), int(rng.integers(0, 60)), th[0], th[1], th[2], int(rng.integers(0, 40))))
    got = run_keep(driver, cases)
    want = [bool(report_ref.keep(np.array([c[0]]), [c[1]], [c[2]], c[3], c[4], c[5], c[6])[0]) for c in cases]
    assert got.tolist() == want and 200 < sum(want) < 1800


# ---------------------------------------------------------------- oracle alignments: invariants, and the GPU test's cases
@pytest.fixture(scope="module")
def small():
    oracle.build()
    S = get_blosum62()
    seqs, where = report_ref.small_set(S)
    return S, seqs, [Protein.str_to_vec(s) for s in seqs], where


def test_invariants_on_oracle_alignments(small):
    """With SKIP_SEED the counted columns are the walk's: core local, identical + positive + mismatch + t_gap == end_x - start_x (the
    query residues the walk passes) and the same with q_gap == end_y - start_y; core global, columns - q_gap == N and columns - t_gap
    == M.  Without the flag every count is one column more, of the class of the end cell's pair."""
    S, seqs, codes, where = small
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(60):
        i, j = (int(v) for v in rng.choice(len(codes), 2, replace=False))
        o = oracle.align(oracle.CORE_LOCAL, codes[i], codes[j], 11, 2, S)
        if o["status"] == 0:
            r = report_ref.report(o["qa"], o["ta"], S, report_ref.SKIP_SEED)
            aligned = int(r["identical"]) + int(r["positive"]) + int(r["mismatch"])
            assert aligned + int(r["t_gap"]) == o["end"][1] - o["start"][1]
            assert aligned + int(r["q_gap"]) == o["end"][0] - o["start"][0]
            full = report_ref.report(o["qa"], o["ta"], S, 0)
            assert int(full["columns"]) == int(r["columns"]) + 1 == len(o["qa"])
            n += 1
        g = oracle.align(oracle.CORE_GLOBAL, codes[i], codes[j], 11, 2, S)
        assert g["status"] == 0
        r = report_ref.report(g["qa"], g["ta"], S, report_ref.SKIP_SEED)
        assert int(r["columns"]) - int(r["q_gap"]) == len(codes[i]) and int(r["columns"]) - int(r["t_gap"]) == len(codes[j])
    assert n >= 30


def test_an_aln_len_of_one_does_not_exist():
    """why the lengths case starts at 2: the shortest alignment there is -- one residue against itself -- has aln_len 2 under both
    semantics (the seed pair and the walk's one column), and a local pair without a positive cell fails, so it is never held"""
    S = get_blosum62()
    w, g = Protein.str_to_vec("W"), Protein.str_to_vec("G")
    for sem in (oracle.CORE_LOCAL, oracle.CORE_GLOBAL):
        o = oracle.align(sem, w, w, 11, 2, S)
        assert o["status"] == 0 and len(o["qa"]) == 2
    assert oracle.align(oracle.CORE_LOCAL, w, g, 11, 2, S)["status"] == _ffi.ERR_NO_POSITIVE_CELL
    assert len(oracle.align(oracle.CORE_GLOBAL, w, g, 11, 2, S)["qa"]) == 2


def test_the_gpu_cases_are_what_they_claim(small):
    S, seqs, codes, where = small
    assert 36 <= len(seqs) <= 44
    assert all(q < t for q, t in where.values())
    for n in report_ref.LENGTHS:
        q, t = where["len%d" % n]
        o = oracle.align(oracle.CORE_LOCAL, codes[q], codes[t], 11, 2, S)
        assert o["status"] == 0 and len(o["qa"]) == n
        assert (report_ref.classes(o["qa"], o["ta"], S) == report_ref.IDENTICAL).all()
        assert seqs[q].startswith("WWW") and seqs[q].endswith("WWW") and seqs[t].startswith("GGG") and seqs[t].endswith("GGG")
    assert report_ref.LENGTHS == [2, 63, 64, 65, 66, 128, 129, 130]
    for sem in (oracle.CORE_LOCAL, oracle.CORE_GLOBAL):
        q, t = where["seam0"]
        o = oracle.align(sem, codes[q], codes[t], 11, 2, S)
        c = report_ref.classes(o["qa"], o["ta"], S)
        assert np.flatnonzero(c == report_ref.T_GAP).tolist() == list(range(60, 70))          # covers columns 63 and 64
        r = report_ref.report(o["qa"], o["ta"], S, report_ref.SKIP_SEED)
        assert (int(r["t_gap"]), int(r["t_gap_open"]), int(r["q_gap"]), int(r["q_gap_open"])) == (10, 1, 0, 0)
        q, t = where["seam1"]
        o = oracle.align(sem, codes[q], codes[t], 11, 2, S)
        c = report_ref.classes(o["qa"], o["ta"], S)
        assert np.flatnonzero(c == report_ref.Q_GAP).tolist() == [64, 65, 66]                 # starts at column 64
        r = report_ref.report(o["qa"], o["ta"], S, report_ref.SKIP_SEED)
        assert (int(r["q_gap"]), int(r["q_gap_open"]), int(r["t_gap"])) == (3, 1, 0)


def test_the_tile_case_is_what_it_claims():
    oracle.build()
    S = get_blosum62()
    seqs = report_ref.tile_set()
    codes = [Protein.str_to_vec(s) for s in seqs]
    assert 66 <= len(seqs) <= 90 and all(12 <= len(s) <= 40 for s in seqs)
    strings, ql, tl = [], [], []
    for i in range(len(codes)):
        for j in range(i + 1, len(codes)):
            o = oracle.align(oracle.CORE_GLOBAL, codes[i], codes[j], 11, 2, S)
            assert o["status"] == 0 and o["f"] == 0.0                 # every pair is a hit of f_min = 0
            strings.append((o["qa"], o["ta"]))
            ql.append(len(codes[i]))
            tl.append(len(codes[j]))
    assert 2049 <= len(strings) <= 4000
    assert report_ref.upper_pair(len(seqs), 0) == (0, 1) and report_ref.upper_pair(len(seqs), len(strings) - 1) == (len(seqs) - 2, len(seqs) - 1)
    rep = report_ref.reports(strings, S, report_ref.SKIP_SEED)
    kept = np.flatnonzero(report_ref.keep(rep, ql, tl, min_identity=report_ref.TILE_MIX))
    assert 2047 in kept and 2048 in kept and 2 <= len(kept) < 50


# ---------------------------------------------------------------- the library and the Python layer
@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def test_library_exports_both_calls_with_the_headers_arguments(lib):
    text = open(os.path.join(ROOT, "include", "aligner_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    want = {
        "aln_seqset_held_report": ["aln_seqset *set", "const aln_params *params", "uint32_t flags", "const uint32_t *keep", "uint64_t n_keep",
                                   "aln_hit_report *reports"],
        "aln_seqset_held_filter": ["aln_seqset *set", "const aln_params *params", "uint32_t flags", "const aln_hit_filter *filter",
                                   "uint32_t *positions", "aln_hit_report *reports", "uint64_t capacity", "uint64_t *count"],
    }
    rust = open(os.path.join(ROOT, "rust", "aligner-core-hip", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym, args in want.items():
        assert sym in _ffi.EXPORTS and hasattr(lib, sym)
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl
        assert [" ".join(a.split()) for a in decl.group(1).split(",") if a.strip()] == args
        assert len(getattr(lib, sym).argtypes) == len(args)
        assert "pub fn %s(" % sym in rust and sym in integration
    at = lib.aln_seqset_held_report.argtypes
    assert at[1] == C.POINTER(_ffi.Params) and at[2] is C.c_uint32 and at[4] is C.c_uint64
    at = lib.aln_seqset_held_filter.argtypes
    assert at[1] == C.POINTER(_ffi.Params) and at[2] is C.c_uint32 and at[3] == C.POINTER(_ffi.HitFilter) and at[6] is C.c_uint64
    assert "pub struct AlnHitReport" in rust and "pub struct AlnHitFilter" in rust
    body = hdr[hdr.index("typedef struct aln_hit_report {"):hdr.index("} aln_hit_report;")]
    assert re.findall(r"(\w+)\s*;", body) == FIELDS
    body = hdr[hdr.index("typedef struct aln_hit_filter {"):hdr.index("} aln_hit_filter;")]
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in _ffi.HitFilter._fields_]
    assert "#define ALN_REPORT_SKIP_SEED 1u" in hdr and lib.aln_abi_version() == 2
    from aligner_amd import build as native_build
    assert "aln_report.hip" in native_build.SOURCES and "aln_report_rules.h" in native_build.HEADERS


def test_null_arguments_are_refused_without_a_device(lib):
    rep = np.full(2 * 40, 7, dtype=np.uint8).view(seqset_module.REPORT_DTYPE)
    pos = np.full(2, 7, dtype=np.uint32)
    keep = np.array([0, 1], dtype=np.uint32)
    count = C.c_uint64(77)
    p, flt = _ffi.Params(), _ffi.HitFilter()
    assert lib.aln_seqset_held_report(None, C.byref(p), 1, keep.ctypes.data, 2, rep.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_report(None, None, 0, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_filter(None, C.byref(p), 1, C.byref(flt), pos.ctypes.data, rep.ctypes.data, 2, C.byref(count)) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_filter(None, None, 0, None, None, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert rep.tobytes() == bytes([7]) * 80 and pos.tolist() == [7, 7] and count.value == 77
    for cls in (seqset_module.HeldHits, seqset_module.BestHits):
        assert callable(cls.report) and callable(cls.filter)


def test_report_fractions():
    r = np.zeros(3, dtype=seqset_module.REPORT_DTYPE)
    r[0] = (10, 4, 2, 1, 2, 1, 1, 1, 0, 0)
    r[1] = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)                             # no column: 0 / 0
    r[2] = (0, 0, 0, 0, 0, 0, 0, 0, _ffi.ERR_NO_POSITIVE_CELL, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            x = seqset_module.report_fractions(r, [16, 5, 0], [9, 5, 0])
    assert x.dtype.names == ("identity", "positives", "q_cover", "t_cover", "gap_opens", "gaps")
    assert x["identity"][0] == 0.4 and x["positives"][0] == 0.6 and x["q_cover"][0] == 0.5 and x["t_cover"][0] == 1.0
    assert x["gap_opens"].tolist() == [2, 0, 0] and x["gaps"].tolist() == [3, 0, 0]
    assert np.isnan(x["identity"][1]) and np.isnan(x["positives"][1]) and x["q_cover"][1] == 0.0 and x["t_cover"][1] == 0.0
    assert np.isnan(x["q_cover"][2]) and np.isnan(x["t_cover"][2])
    assert len(seqset_module.report_fractions(r[:0], [], [])) == 0


@pytest.mark.parametrize("argv", [
    ["--report"],                                                     # no held pass
    ["--min-identity", "0.5"],
    ["--min-q-cover", "0.5"],
    ["--min-t-cover", "0.5"],
    ["--report", "--heuristic", "--kd", "1", "--r-squared", "1"],
    ["--min-identity", "0.5", "--best", "3", "--heuristic"],
])
def test_allpairs_refuses_before_anything_is_read(argv, capsys):
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", os.path.join(ROOT, "no", "such.fasta")] + argv)
    assert e.value.code == 2
    assert "--report" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--report", "--best", "3"], ["--min-identity", "0.5", "--report", "--f-min", "30"],
                                  ["--min-q-cover", "0.5", "--min-t-cover", "0.5", "--best", "2", "--shuffles", "10"]])
def test_allpairs_accepts_the_flags_with_a_held_pass(argv):
    """Accepted arguments get as far as the input file (which is not there); no device is asked for."""
    with pytest.raises(OSError):
        allpairs.main(["-i", os.path.join(ROOT, "no", "such.fasta")] + argv)


def test_the_help_says_that_best_selects_before_it_filters(capsys):
    with pytest.raises(SystemExit):
        allpairs.main(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "the K best are selected first, then filtered" in out
