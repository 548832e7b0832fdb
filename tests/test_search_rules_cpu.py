"""The k best per record over a candidate list without a GPU: aligner_amd/csrc/aln_search_rules.h driven through a small C++ program
(row_first against numpy.searchsorted; touched rows, pieces, segments and runs of every chunk of small lists against a clipping
restatement written here; a host replay of "sort pieces by (row, order), fold runs into running lists" against numpy.lexsort per row);
the companion header include/aligner_hip_search.h against its mirrors; the refusals that need no device; the command's argument
errors."""
import ctypes as C
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 2048

DRIVER = r"""
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "aln_search_rules.h"
static std::vector<uint64_t> read_list(uint64_t count)
{
    std::vector<uint64_t> list(count + 1);
    for (uint64_t i = 0; i < count; ++i) if (scanf("%" SCNu64, &list[i]) != 1) exit(2);
    return list;
}
struct Entry { uint64_t key; uint32_t t, row; };
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    uint64_t T, rows, count;
    if (!strcmp(argv[1], "rowfirst")) {       // cases `T n_r C L[C] r[n_r]` -> row_first of the listed rows
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &T, &rows, &count) == 3) {
            const std::vector<uint64_t> list = read_list(count);
            for (uint64_t i = 0; i < rows; ++i) {
                uint64_t r;
                if (scanf("%" SCNu64, &r) != 1) return 2;
                printf("%" PRIu64 " ", aln_search_row_first(list.data(), count, r, T));
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "geom")) {
        // cases `T q_count C L[C]` -> for every chunk (c0, n) of the list one line:
        // c0 n row0 row1 pieces { piece: start len } { touched row: seg_len [start piece0 n_pieces { run: start len }] } { position: run_start }
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &T, &rows, &count) == 3) {
            const std::vector<uint64_t> list = read_list(count);
            std::vector<uint64_t> first(rows + 1);
            for (uint64_t r = 0; r <= rows; ++r) first[r] = aln_search_row_first(list.data(), count, r, T);
            for (uint64_t c0 = 0; c0 < count; ++c0)
                for (uint64_t n = 1; c0 + n <= count; ++n) {
                    const uint64_t row0 = aln_search_row(list[c0], T), row1 = aln_search_row(list[c0 + n - 1], T), pieces = aln_search_pieces(n);
                    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, c0, n, row0, row1, pieces);
                    for (uint64_t p = 0; p < pieces; ++p) {
                        uint64_t s, l;
                        aln_search_piece(c0, n, p, &s, &l);
                        printf(" %" PRIu64 " %" PRIu64, s, l);
                    }
                    for (uint64_t r = row0; r <= row1; ++r) {
                        uint64_t s = 0, p0 = 0, np = 0;
                        const uint64_t len = aln_search_row_segment(first[r], first[r + 1], c0, n, &s, &p0, &np);
                        printf(" %" PRIu64, len);
                        if (!len) continue;
                        printf(" %" PRIu64 " %" PRIu64 " %" PRIu64, s, p0, np);
                        for (uint64_t p = p0; p < p0 + np; ++p) {
                            uint64_t rs, rl;
                            aln_search_run(s, len, c0, p, &rs, &rl);
                            printf(" %" PRIu64 " %" PRIu64, rs, rl);
                        }
                    }
                    for (uint64_t at = c0; at < c0 + n; ++at) printf(" %" PRIu64, aln_search_run_start(first[aln_search_row(list[at], T)], c0, at));
                    printf("\n");
                }
        }
        return 0;
    }
    if (!strcmp(argv[1], "edge")) {
        // the same closed forms at list positions near 2048 without a list that long: lines `first next c0 n` (a row's range and a
        // chunk) -> seg_len [start piece0 n_pieces { run: start len }]
        uint64_t first, next, c0, n;
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &first, &next, &c0, &n) == 4) {
            uint64_t s = 0, p0 = 0, np = 0;
            const uint64_t len = aln_search_row_segment(first, next, c0, n, &s, &p0, &np);
            printf("%" PRIu64, len);
            if (len) {
                printf(" %" PRIu64 " %" PRIu64 " %" PRIu64, s, p0, np);
                for (uint64_t p = p0; p < p0 + np; ++p) {
                    uint64_t rs, rl;
                    aln_search_run(s, len, c0, p, &rs, &rl);
                    printf(" %" PRIu64 " %" PRIu64 " %" PRIu64, rs, rl, aln_search_run_start(first, c0, rs + rl - 1));
                }
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "replay")) {
        // one case: `T q_count q_first t_first flags f_min k C  { pair f status } x C  chunks  n[chunks]` (doubles as 16 hex digits)
        // -> per row `n { t f }`: pieces sorted by (row, order), the first `slots` of each run kept (the rest overwritten with
        // rubbish: nobody may read it), runs folded into running lists with aln_best_fold
        uint64_t q_first, t_first, flags, fm, k, chunks;
        if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNx64 " %" SCNu64 " %" SCNu64, &T, &rows, &q_first, &t_first, &flags, &fm,
                  &k, &count) != 8) return 2;
        double f_min;
        memcpy(&f_min, &fm, 8);
        std::vector<uint64_t> list(count + 1);
        std::vector<double> f(count + 1);
        std::vector<int32_t> status(count + 1);
        for (uint64_t i = 0; i < count; ++i) {
            uint64_t bits;
            int st;
            if (scanf("%" SCNu64 " %" SCNx64 " %d", &list[i], &bits, &st) != 3) return 2;
            memcpy(&f[i], &bits, 8);
            status[i] = st;
        }
        if (scanf("%" SCNu64, &chunks) != 1) return 2;
        const uint32_t slots = aln_best_slots((uint32_t)k, T);
        std::vector<uint64_t> first(rows + 1);
        for (uint64_t r = 0; r <= rows; ++r) first[r] = aln_search_row_first(list.data(), count, r, T);
        std::vector<uint64_t> run_key(rows * slots + 1), tmp_key(slots + 1);
        std::vector<uint32_t> run_t(rows * slots + 1), run_n(rows + 1, 0), tmp_t(slots + 1);
        uint64_t c0 = 0;
        for (uint64_t c = 0; c < chunks; ++c) {
            uint64_t n;
            if (scanf("%" SCNu64, &n) != 1 || !n || c0 + n > count) return 2;
            std::vector<uint64_t> piece_key(n);
            std::vector<uint32_t> piece_t(n);
            for (uint64_t p = 0; p < aln_search_pieces(n); ++p) {
                uint64_t s, l;
                aln_search_piece(c0, n, p, &s, &l);
                std::vector<Entry> e(l);
                for (uint64_t i = 0; i < l; ++i) {
                    const uint64_t row = aln_search_row(list[s + i], T), t = t_first + aln_search_column(list[s + i], T);
                    e[i].row = (uint32_t)row; e[i].key = 0; e[i].t = 0xFFFFFFFFu;
                    if (aln_best_candidate(status[s + i], f[s + i], f_min, q_first + row, t, (uint32_t)flags)) { e[i].key = aln_best_key(f[s + i]); e[i].t = (uint32_t)t; }
                }
                std::sort(e.begin(), e.end(), [](const Entry &a, const Entry &b) { return a.row < b.row || (a.row == b.row && aln_best_before(a.key, a.t, b.key, b.t)); });
                for (uint64_t i = 0; i < l; ++i) {
                    if (e[i].row != aln_search_row(list[s + i], T)) { printf("a run moved\n"); return 1; }
                    const bool lead = s + i - aln_search_run_start(first[e[i].row], c0, s + i) < slots;
                    piece_key[s + i - c0] = lead ? e[i].key : 0xDEADDEADDEADDEADull;
                    piece_t[s + i - c0] = lead ? e[i].t : 0xDEADu;
                }
            }
            for (uint64_t r = aln_search_row(list[c0], T); r <= aln_search_row(list[c0 + n - 1], T); ++r) {
                uint64_t s = 0, p0 = 0, np = 0;
                const uint64_t len = aln_search_row_segment(first[r], first[r + 1], c0, n, &s, &p0, &np);
                if (!len) continue;
                for (uint64_t p = p0; p < p0 + np; ++p) {
                    uint64_t rs, rl;
                    aln_search_run(s, len, c0, p, &rs, &rl);
                    uint32_t nb = 0;
                    while (nb < rl && nb < slots && piece_key[rs - c0 + nb] != 0) ++nb;
                    const uint32_t got = aln_best_fold(&run_key[r * slots], &run_t[r * slots], run_n[r], &piece_key[rs - c0], &piece_t[rs - c0], nb, slots,
                                                       tmp_key.data(), tmp_t.data());
                    for (uint32_t i = 0; i < got; ++i) { run_key[r * slots + i] = tmp_key[i]; run_t[r * slots + i] = tmp_t[i]; }
                    run_n[r] = got;
                }
            }
            c0 += n;
        }
        if (c0 != count) return 2;
        for (uint64_t r = 0; r < rows; ++r) {
            printf("%u", run_n[r]);
            for (uint32_t i = 0; i < run_n[r]; ++i) {
                const double v = aln_best_unkey(run_key[r * slots + i]);
                uint64_t bits;
                memcpy(&bits, &v, 8);
                printf(" %u %016" PRIx64, run_t[r * slots + i], bits);
            }
            printf("\n");
        }
        return 0;
    }
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    tmp = tmp_path_factory.mktemp("search_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe])
    return exe


def run(drv, what, text):
    return subprocess.run([drv, what], check=True, capture_output=True, text=True, input=text).stdout.splitlines()


def random_list(rng, T, rows, fill, empty_rows=()):
    """ascending pair numbers of a rows x T rectangle: every pair of a non-empty row with probability `fill`"""
    out = []
    for r in range(rows):
        if r in empty_rows:
            continue
        cols = [c for c in range(T) if rng.random() < fill] if T <= 64 else sorted(rng.sample(range(T), max(1, int(fill * min(T, 40)))))
        out += [r * T + c for c in cols]
    return out


# ---------------------------------------------------------------- row_first
def test_row_first_against_searchsorted(driver):
    rng = random.Random(17)
    cases = []
    for T in (1, 7, 2047, 2048, 2049):
        for rows, empty in ((9, ()), (9, (0, 1)), (9, (4, 5)), (9, (7, 8)), (9, (0, 3, 4, 8)), (1, ()), (3, (0, 1, 2))):
            for fill in (0.2, 0.9):
                cases.append((T, rows, random_list(rng, T, rows, fill, empty)))
        # the first and the last pair of rows, and nothing else: the bounds r * T themselves
        cases.append((T, 6, sorted({r * T for r in range(6)} | {r * T + T - 1 for r in range(6)})))
    big = 2 ** 40
    for T in (7, 2049, 2 ** 20 + 1):                     # pair numbers near 2^40: the product r * T needs 64 bits
        r0 = big // T
        rows = r0 + 6
        lst = sorted({(r0 + d) * T + c for d in (0, 2, 3, 5) for c in (0, 1, T // 2, T - 1)})
        cases.append((T, rows, lst, [0, 1] + list(range(r0 - 2, rows + 1))))
    text = ""
    for c in cases:
        rr = list(range(c[1] + 1)) if len(c) == 3 else c[3]
        text += "%d %d %d %s %s\n" % (c[0], len(rr), len(c[2]), " ".join(map(str, c[2])), " ".join(map(str, rr)))
    out = run(driver, "rowfirst", text)
    assert len(out) == len(cases)
    for c, line in zip(cases, out):
        T, rows, lst = c[0], c[1], np.array(c[2], dtype=np.uint64)
        rr = list(range(rows + 1)) if len(c) == 3 else c[3]
        got = np.array(line.split(), dtype=np.uint64)
        bounds = np.array([r * T for r in rr], dtype=np.uint64)                      # (exact: Python integers below 2^64)
        assert np.array_equal(got, np.searchsorted(lst, bounds, side="left")), (T, rows)
        assert got[0] == 0 and got[-1] == len(lst) and np.all(np.diff(got.astype(np.int64)) >= 0)
        assert len(c) == 3 or (int(bounds[-1]) > 2 ** 40 and len(set(got.tolist())) >= 4)


# ---------------------------------------------------------------- geometry: every chunk of small lists
def clip(a0, a1, b0, b1):
    """the intersection of [a0, a1) and [b0, b1) as (start, len); len 0 if empty"""
    lo, hi = max(a0, b0), min(a1, b1)
    return (lo, hi - lo) if hi > lo else (lo, 0)


def expect_geometry(lst, T, c0, n, piece=PIECE):
    """Restated by clipping: rows from the list itself, pieces, segments and runs as interval intersections."""
    rows = [x // T for x in lst]
    row0, row1 = rows[c0], rows[c0 + n - 1]
    pieces = [clip(c0 + p * piece, c0 + (p + 1) * piece, c0, c0 + n) for p in range((n + piece - 1) // piece)]
    tok = [c0, n, row0, row1, len(pieces)]
    for s, l in pieces:
        tok += [s, l]
    for r in range(row0, row1 + 1):
        pos = [i for i in range(len(lst)) if rows[i] == r]
        first, nxt = (pos[0], pos[-1] + 1) if pos else (0, 0)
        s, l = clip(first, nxt, c0, c0 + n)
        tok.append(l)
        if not l:
            continue
        over = [p for p, (ps, pl) in enumerate(pieces) if clip(s, s + l, ps, ps + pl)[1]]
        assert over == list(range(over[0], over[-1] + 1))
        tok += [s, over[0], len(over)]
        for p in over:
            tok += list(clip(s, s + l, *[pieces[p][0], pieces[p][0] + pieces[p][1]]))
    for at in range(c0, c0 + n):
        p = (at - c0) // piece
        first = min(i for i in range(len(lst)) if rows[i] == rows[at])
        tok.append(max(first, pieces[p][0]))
    return tok


def test_geometry_of_every_chunk_of_small_lists(driver):
    rng = random.Random(5)
    cases = []
    for T, rows, fill, empty in ((1, 40, 0.8, (3, 4)), (7, 8, 0.6, (0,)), (7, 8, 0.9, (7,)), (5, 12, 0.5, (5, 6, 7)), (60, 1, 0.7, ()),
                                 (2049, 10, 0.1, (2, 9)), (3, 20, 1.0, ())):
        lst = random_list(rng, T, rows, fill, empty)[:60]
        assert 0 < len(lst) <= 60
        cases.append((T, rows, lst))
    text = "".join("%d %d %d %s\n" % (T, rows, len(lst), " ".join(map(str, lst))) for T, rows, lst in cases)
    out = iter(run(driver, "geom", text))
    checked = 0
    for T, rows, lst in cases:
        for c0 in range(len(lst)):
            for n in range(1, len(lst) - c0 + 1):
                got = [int(x) for x in next(out).split()]
                assert got == expect_geometry(lst, T, c0, n), (T, c0, n)
                checked += 1
    assert checked > 3000 and next(out, None) is None


def test_segments_and_runs_at_the_2047_2048_position_edge(driver):
    """A row's range and a chunk, cut at, before and after the row's edges and the edge between two pieces."""
    cases = []
    for c0 in (0, 1, 5, 2047, 2048, 2049, 10 ** 10):
        for n in (1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5):
            edges = sorted({c0 + d for d in (0, 1, 2046, 2047, 2048, 2049, 4095, 4096, 4097, n - 1, n, n + 1) if c0 + d >= 0} | {max(c0 - 1, 0), max(c0 - 3, 0)})
            for first in edges:
                for nxt in edges:
                    if nxt >= first:
                        cases.append((first, nxt, c0, n))
    out = run(driver, "edge", "".join("%d %d %d %d\n" % c for c in cases))
    assert len(out) == len(cases) > 4000
    crossing = 0
    for (first, nxt, c0, n), line in zip(cases, out):
        got = [int(x) for x in line.split()]
        s, l = clip(first, nxt, c0, c0 + n)
        assert got[0] == l, (first, nxt, c0, n)
        if not l:
            assert len(got) == 1
            continue
        pieces = [clip(c0 + p * PIECE, c0 + (p + 1) * PIECE, c0, c0 + n) for p in range((n + PIECE - 1) // PIECE)]
        over = [p for p, (ps, pl) in enumerate(pieces) if clip(s, s + l, ps, ps + pl)[1]]
        want = [l, s, over[0], len(over)]
        for p in over:
            rs, rl = clip(s, s + l, pieces[p][0], pieces[p][0] + pieces[p][1])
            want += [rs, rl, rs]                                      # the run's last position names the run's start
        assert got == want, (first, nxt, c0, n)
        assert sum(want[5::3]) == l
        crossing += len(over) > 1
    assert crossing > 500


# ---------------------------------------------------------------- host replay against lexsort per row
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def reference_rows(T, rows, q_first, t_first, skip_self, f_min, k, lst, f, status):
    out = []
    slots = min(k, T)
    pair = np.array(lst, dtype=np.int64)
    f = np.array(f, dtype=np.float64)
    status = np.array(status)
    with np.errstate(invalid="ignore"):
        ok = (status == 0) & (f == f) & (f >= f_min)
    row, t = pair // T, t_first + pair % T
    if skip_self:
        ok &= (q_first + row) != t
    for r in range(rows):
        m = np.flatnonzero(ok & (row == r))
        order = m[np.lexsort((t[m], -f[m]))][:slots]
        out.append([(int(t[i]), float(f[i])) for i in order])
    return out


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_host_replay_matches_lexsort_per_row(driver, k):
    rng = random.Random(1000 + k)
    for trial in range(6):
        T, rows = rng.choice([(70, 90), (200, 40), (5000, 3), (64, 64), (1, 50)])
        q_first, t_first = rng.choice([(0, 0), (3, 3), (10, 2)])
        skip_self = trial % 2 == 0
        lst = random_list(rng, T, rows, rng.choice([0.3, 0.95]), empty_rows=(0, rows // 2, rows - 1) if trial % 3 == 0 else ())
        if T == 5000:
            lst = sorted(set(lst) | {r * T + c for r in range(rows) for c in rng.sample(range(T), 2300)})     # rows that span pieces
        # heavy ties: few distinct values, both zeros, a NaN, failed pairs
        values = [0.0, -0.0, 1.0, 1.0, 2.5, -3.0, float("nan"), float("inf"), 7.0]
        f = [rng.choice(values) for _ in lst]
        status = [rng.choice([0] * 9 + [-3]) for _ in lst]
        f_min = rng.choice([float("-inf"), 1.0, float("nan")]) if trial else float("-inf")
        # random chunk cuts (none aligned to rows or pieces on purpose)
        cuts, left = [], len(lst)
        while left:
            n = min(left, rng.choice([1, 3, 17, 100, 2047, 2049, 5000]))
            cuts.append(n)
            left -= n
        text = "%d %d %d %d %d %016x %d %d\n" % (T, rows, q_first, t_first, 1 if skip_self else 0, bits(f_min), k, len(lst))
        text += "".join("%d %016x %d\n" % (p, bits(v), s) for p, v, s in zip(lst, f, status))
        text += "%d %s\n" % (len(cuts), " ".join(map(str, cuts)))
        out = run(driver, "replay", text)
        want = reference_rows(T, rows, q_first, t_first, skip_self, f_min, k, lst, f, status)
        assert len(out) == rows
        for r, line in enumerate(out):
            tok = line.split()
            got = [(int(tok[1 + 2 * i]), struct.unpack("<d", struct.pack("<Q", int(tok[2 + 2 * i], 16)))[0]) for i in range(int(tok[0]))]
            assert [t for t, _ in got] == [t for t, _ in want[r]], (trial, r)
            assert all(a == b for (_, a), (_, b) in zip(got, want[r])), (trial, r)       # (-0.0 == +0.0: the key folds them)


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_search_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_search.h")) == sorted(_ffi.SEARCH_EXPORTS) == ["aln_seqset_candidate_best"]
    for other in (_ffi.EXPORTS, _ffi.CLUSTER_EXPORTS, _ffi.PREFILTER_EXPORTS):
        assert not set(_ffi.SEARCH_EXPORTS) & set(other)
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61 and len(_ffi.PREFILTER_EXPORTS) == 5     # the others are as they were
    assert '#include "aligner_hip_prefilter.h"' in open(os.path.join(ROOT, "include", "aligner_hip_search.h")).read()
    assert "aln_search.hip" in native_build.SOURCES and "aln_search_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_search.h") for h in native_build.HEADERS)


def test_the_library_exports_it_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.SEARCH_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and len(fn.argtypes) == 6 and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_the_header_compiles_as_c99_and_the_caller_calls_it(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_search.h"\nint main(void) { return aln_seqset_candidate_best(0, 0, 1, 0.0, 0, 0) == ALN_OK; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    caller = strip_comments(open(os.path.join(ROOT, "tests", "abi_search.c")).read())
    for sym in _ffi.SEARCH_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, caller), sym
    exe = native_build.build_search_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["best_max", str(_ffi.SEQSET_BEST_MAX), "skip_self", str(_ffi.BEST_SKIP_SELF)]


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    count = C.c_uint64(99)
    p = _ffi.Params()
    assert lib.aln_seqset_candidate_best(None, C.byref(p), 3, 0.0, 0, C.byref(count)) == _ffi.ERR_INVALID_ARGUMENT and count.value == 99
    assert b"null" in lib.aln_last_error()
    assert lib.aln_seqset_candidate_best(None, None, 0, float("nan"), 7, None) == _ffi.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the command's argument errors
@pytest.mark.parametrize("extra,word", [
    (["--best-candidates", "3"], "--kmer"),                                                       # without --kmer
    (["--kmer", "3", "--best-candidates", "3", "--best", "2"], "--best"),                          # together with --best
    (["--kmer", "3", "--best-candidates", "3", "--heuristic", "--kd", "1", "--r-squared", "0.5"], "--heuristic"),
    (["--kmer", "3", "--best-candidates", "0"], "--best-candidates"), (["--kmer", "3", "--best-candidates", "65"], "--best-candidates"),
    (["--kmer", "3", "--best-candidates", "-1"], "--best-candidates"),
    (["--kmer", "3", "--best", "2"], "--best-candidates"),                                         # the old refusal points to the new flag
    (["--kmer", "3", "--report"], "--best-candidates"), (["--kmer", "3", "--cluster", "greedy"], "--best-candidates"),
    (["--kmer", "3", "--shuffles", "5"], "--best-candidates"),
])
def test_the_commands_argument_errors(tmp_path, capsys, extra, word):
    from aligner_amd import allpairs
    fa = tmp_path / "x.fasta"
    fa.write_text(">a\nACDEFGHIK\n>b\nACDEFGHIK\n")
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", str(fa)] + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err
