"""The pair order of aln_seqset_* (aln_seqset_rules.h; no GPU): the header compiled into a driver with the host compiler against the
independent restatement in seqset_ref.py -- every pair of every small block, rank as the inverse of unrank, the row boundaries of
squares up to n = 2^32 - 1 (where a floating-point square root would round wrongly), the upper order against a literal restatement
of generate_pairs -- plus the exported symbols and the C layout of aln_seqset_block against the ctypes struct.  The header's chunk
cutter (aln_seqset_cut) runs in the same driver against select_cases.chunk_counts, the restatement of the forced rule."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import select_cases as SC  # noqa: E402
import seqset_ref  # noqa: E402

from aligner_amd import _ffi  # noqa: E402
from aligner_amd import seqset as seqset_module  # noqa: E402,F401  (the feature's module: absent on the parent commit)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aln_seqset_create", "aln_seqset_destroy", "aln_seqset_pairs", "aln_seqset_score", "aln_seqset_hits", "aln_seqset_held_list",
       "aln_seqset_held_strings", "aln_seqset_stats"]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "aln_seqset_rules.h"
static aln_seqset_block blk(char **a)
{
    aln_seqset_block b;
    b.q_first = strtoull(a[0], 0, 10); b.q_count = strtoull(a[1], 0, 10); b.t_first = strtoull(a[2], 0, 10); b.t_count = strtoull(a[3], 0, 10);
    b.upper = (uint32_t)strtoul(a[4], 0, 10); b.reserved = (uint32_t)strtoul(a[5], 0, 10);
    return b;
}
int main(int argc, char **argv)
{
    // pairs <n_seqs> <block: 6 numbers>                  -> the number of pairs
    // all <n_seqs> <block>                               -> per pair "q t rank(q, t)", by unrank and, on the same line, by next
    // at <n_seqs> <block> <k> ...                        -> per k "q t rank(q, t)"
    // cut <target> <forced> <cap>, cells on stdin        -> the chunk counts of aln_seqset_cut over those positions, on one line
    if (argc == 5 && !strcmp(argv[1], "cut")) {
        std::vector<double> cells;
        double v, total = 0;
        while (scanf("%lf", &v) == 1) { cells.push_back(v); total += v; }
        size_t at = 0;
        std::vector<uint64_t> counts;
        aln_seqset_cut([&]() { return cells[at++]; }, cells.size(), total, atof(argv[2]), atoi(argv[3]) != 0, strtoull(argv[4], 0, 10), counts);
        for (uint64_t c : counts) printf("%llu ", (unsigned long long)c);
        printf("\n");
        return 0;
    }
    if (argc < 9) return 2;
    const uint64_t n_seqs = strtoull(argv[2], 0, 10);
    const aln_seqset_block b = blk(argv + 3);
    const uint64_t pairs = aln_seqset_block_pairs(n_seqs, b);
    if (!strcmp(argv[1], "pairs")) { printf("%llu\n", (unsigned long long)pairs); return 0; }
    if (!strcmp(argv[1], "all")) {
        uint64_t cq = 0, ct = 0;
        if (pairs) aln_seqset_unrank(b, 0, &cq, &ct);
        for (uint64_t k = 0; k < pairs; ++k) {
            uint64_t q, t;
            aln_seqset_unrank(b, k, &q, &t);
            printf("%llu %llu %llu %llu %llu\n", (unsigned long long)q, (unsigned long long)t, (unsigned long long)aln_seqset_rank(b, q, t),
                   (unsigned long long)cq, (unsigned long long)ct);
            aln_seqset_next(b, &cq, &ct);
        }
        return 0;
    }
    if (!strcmp(argv[1], "at")) {
        for (int i = 9; i < argc; ++i) {
            const uint64_t k = strtoull(argv[i], 0, 10);
            if (k >= pairs) return 3;
            uint64_t q, t;
            aln_seqset_unrank(b, k, &q, &t);
            printf("%llu %llu %llu\n", (unsigned long long)q, (unsigned long long)t, (unsigned long long)aln_seqset_rank(b, q, t));
        }
        return 0;
    }
    return 2;
}
"""

ABI = r"""
#include <stddef.h>
#include <stdio.h>
#include "aligner_hip.h"
int main(void)
{
    printf("%u %u %u %u %u %u %u\n", (unsigned)sizeof(aln_seqset_block), (unsigned)offsetof(aln_seqset_block, q_first),
           (unsigned)offsetof(aln_seqset_block, q_count), (unsigned)offsetof(aln_seqset_block, t_first),
           (unsigned)offsetof(aln_seqset_block, t_count), (unsigned)offsetof(aln_seqset_block, upper),
           (unsigned)offsetof(aln_seqset_block, reserved));
    return 0;
}
"""


def _compile(tmp, name, src, cmd):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as fh:
        fh.write(src)
    exe = os.path.join(str(tmp), name.split(".")[0])
    subprocess.check_call(cmd + [path, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the seqset-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("seqset_rules")
    return _compile(tmp, "drv.cpp", DRIVER, [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc")])


def _run(drv, *args):
    out = subprocess.run([drv] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    return [[int(v) for v in line.split()] for line in out.splitlines()]


def _blocks():
    """Every square with n <= 40 at three positions, rectangles of assorted shapes (overlapping ranges, ranges that do not start at 0)."""
    upper = [(first, n) for n in range(2, 41) for first in (0, 1, 7)]
    rect = [(qf, qc, tf, tc) for qc in (1, 2, 3, 17, 40) for tc in (1, 2, 5, 40) for qf, tf in ((0, 0), (3, 0), (2, 9), (5, 4))]
    return upper, rect


def test_every_pair_of_every_small_block(driver):
    upper, rect = _blocks()
    for first, n in upper:
        want = seqset_ref.generate_pairs(first, n)
        got = _run(driver, "all", first + n, first, n, first, n, 1, 0)
        assert [(g[0], g[1]) for g in got] == want, (first, n)
        assert [g[2] for g in got] == list(range(len(want))), (first, n)                 # rank(unrank(k)) == k
        assert [(g[3], g[4]) for g in got] == want, (first, n)                          # the host's cursor walks the same order
        assert _run(driver, "pairs", first + n, first, n, first, n, 1, 0) == [[n * (n - 1) // 2]]
    for qf, qc, tf, tc in rect:
        want = seqset_ref.rectangle_pairs(qf, qc, tf, tc)
        n_seqs = max(qf + qc, tf + tc) + 2
        got = _run(driver, "all", n_seqs, qf, qc, tf, tc, 0, 0)
        assert [(g[0], g[1]) for g in got] == want, (qf, qc, tf, tc)
        assert [g[2] for g in got] == list(range(len(want)))
        assert [(g[3], g[4]) for g in got] == want


def test_upper_order_is_generate_pairs():
    """The restatement's closed form against the literal double loop, so that the large-n test below rests on it."""
    for first, n in ((0, 2), (0, 3), (5, 9), (1, 64), (0, 65)):
        want = seqset_ref.generate_pairs(first, n)
        assert [seqset_ref.upper_unrank(first, n, k) for k in range(len(want))] == want
        assert [seqset_ref.upper_rank(first, n, q, t) for q, t in want] == list(range(len(want)))


@pytest.mark.parametrize("n", [2, 3, 65535, 65536, 2 ** 32 - 1])
def test_first_and_last_pair_of_rows(driver, n):
    """First and last pair of every row (of the rows at both ends, around every power of two and around n / sqrt(2) for the largest
    squares: 2^32 rows do not fit a test)."""
    if n <= 65536:
        rows = range(n - 1)
    else:
        rows = sorted({r for c in [0, n - 2, n // 2, int(n * 0.2928932), 3037000499 % n] + [2 ** e for e in range(1, 32)]
                       for r in range(max(0, c - 3), min(n - 2, c + 3) + 1)})
    ks, want = [], []
    for r in rows:
        s = seqset_ref.row_start(n, r)
        ks += [s, s + (n - 1 - r) - 1]
        want += [(r, r + 1), (r, n - 1)]
    total = n * (n - 1) // 2
    assert ks[-1] == total - 1 or n > 65536
    got = []
    for a in range(0, len(ks), 2000):
        got += _run(driver, "at", n, 0, n, 0, n, 1, 0, *ks[a:a + 2000])
    assert [(g[0], g[1]) for g in got] == want
    assert [g[2] for g in got] == ks
    assert [seqset_ref.upper_unrank(0, n, k) for k in ks[:400]] == want[:400]
    assert _run(driver, "pairs", n, 0, n, 0, n, 1, 0) == [[total]]


def test_invalid_blocks_have_no_pairs(driver):
    for n_seqs, b in [(10, (0, 11, 0, 11, 1, 0)), (10, (5, 6, 0, 1, 0, 0)), (10, (0, 1, 10, 1, 0, 0)), (10, (0, 4, 1, 4, 1, 0)),
                      (10, (0, 4, 0, 5, 1, 0)), (10, (0, 4, 0, 4, 1, 1)), (10, (0, 4, 0, 4, 2, 0)), (10, (0, 0, 0, 4, 0, 0)),
                      (10, (0, 1, 0, 1, 1, 0)), (10, (2 ** 64 - 1, 2, 0, 1, 0, 0)), (10, (1, 2 ** 64 - 1, 0, 1, 0, 0))]:
        assert _run(driver, "pairs", n_seqs, *b) == [[0]], b
        assert seqset_ref.block_pairs(n_seqs, *b) == 0, b
    assert _run(driver, "pairs", 10, 0, 10, 0, 10, 0, 0) == [[100]]


# ---------------------------------------------------------------- where a pass is cut (aln_seqset_cut)
CAP = 1 << 22                 # the pair limit of a chunk (ALN_SEQSET_CHUNK_PAIRS)


def _cut(drv, cells, target, forced=True, cap=CAP):
    text = "\n".join(str(int(c)) for c in cells) + "\n"
    out = subprocess.run([drv, "cut", repr(float(target)), str(int(forced)), str(cap)], input=text, check=True, capture_output=True, text=True).stdout
    return [int(v) for v in out.split()]


def _restated(cells, target, cap=None):
    """select_cases.chunk_counts over a hand-made cell list: position i is the pair (sequence i, a sequence of length 1)"""
    n = len(cells)
    lengths = np.array(list(cells) + [1], dtype=np.int64)
    return SC.chunk_counts(lengths, np.arange(n), np.full(n, n), float(target), cap)


@pytest.mark.parametrize("block", [("full",), ("upper", 0, SC.S), ("rect",) + SC.RECT_INNER], ids=lambda b: b[0])
def test_cut_of_the_select_cases_set(driver, block):
    """The header's cutter against the restatement at chunk_cells(): the block's own order, and every third pair of it as an ascending
    sublist, as a candidate list is one."""
    L = SC.set_lengths()
    target = SC.chunk_cells()
    q, t = SC.block_pairs_qt(block)
    for step in (1, 3):
        qs, ts = q[::step], t[::step]
        want = SC.chunk_counts(L, qs, ts, float(target))
        got = _cut(driver, L[qs] * L[ts], target)
        assert got == want and sum(got) == len(qs), (block, step)
        assert got == SC.chunk_counts(L, qs, ts, float(target), CAP)            # the cap is far away: it changes nothing
    if block[0] != "rect":
        assert len(SC.chunk_counts(L, q, t, float(target))) >= 3                # (the inner rectangle fits one chunk)


CUT_EDGES = [
    # name, cells, target, expected counts (worked out by hand from the rule)
    ("total_is_1.5_targets", [10] * 15, 100, [15]),
    ("one_cell_more", [10] * 14 + [11], 100, [10, 5]),
    ("tail_under_a_quarter", [50, 50, 50, 50, 24], 100, [2, 3]),
    ("tail_a_quarter", [50, 50, 50, 50, 25], 100, [2, 2, 1]),
    ("first_pair_exceeds_the_target", [500] + [10] * 12, 100, [1, 12]),
    ("last_position_reaches_the_target", [60, 60, 30, 30, 40], 100, [2, 3]),
]


@pytest.mark.parametrize("name,cells,target,want", CUT_EDGES, ids=[c[0] for c in CUT_EDGES])
def test_cut_edges(driver, name, cells, target, want):
    assert len(cells) <= 20
    assert _restated(cells, target) == want
    assert _cut(driver, cells, target) == want


def test_cut_unforced_and_capped(driver):
    cells = [10] * 20
    # not forced and under 2e10 cells: one chunk whatever the target; forced, the target rules
    for target in (1, 25, 1000):
        assert _cut(driver, cells, target, forced=False) == [20]
        assert _cut(driver, cells, target, forced=True) == _restated(cells, target)
    assert _cut(driver, cells, 25) == [3, 3, 3, 3, 3, 3, 2]
    # a cap of 7: it cuts where the cells alone would not (they fit one chunk, or reach the target only at 9 pairs), and stays out of
    # the way where the cells cut sooner
    for target, want in ((1000, [7, 7, 6]), (90, [7, 7, 6]), (30, [3, 3, 3, 3, 3, 3, 2])):
        got = _cut(driver, cells, target, cap=7)
        assert got == want == _restated(cells, target, cap=7)
        assert max(got) <= 7 and sum(got) == 20
    assert _cut(driver, [], 100) == []


@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def test_library_exports_the_seqset_symbols_with_the_headers_argument_counts(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aligner_hip.h")).read(), flags=re.S)
    for sym in NEW:
        assert sym in _ffi.EXPORTS and hasattr(lib, sym), sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl, sym
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert len(getattr(lib, sym).argtypes) == n_args, sym
    assert lib.aln_abi_version() == 2


def test_seqset_argument_validation_without_a_device(lib):
    st = C.c_int(-1)
    assert not lib.aln_seqset_create(None, None, None, None, 0, C.byref(st))
    assert st.value == _ffi.ERR_INVALID_ARGUMENT
    b = _ffi.SeqsetBlock(0, 2, 0, 2, 1, 0)
    assert lib.aln_seqset_pairs(None, C.byref(b)) == 0
    assert lib.aln_seqset_score(None, None, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_hits(None, None, None, 0.0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_list(None, 0, 0, None, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_held_strings(None, None, 0, None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_stats(None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    lib.aln_seqset_destroy(None)


def test_block_layout_c99_equals_ctypes(tmp_path):
    cc = os.environ.get("CC", "gcc")
    if shutil.which(cc) is None:
        pytest.fail("no C compiler (%s)" % cc)
    exe = _compile(tmp_path, "abi.c", ABI, [cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")])
    size, *offs = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    S = _ffi.SeqsetBlock
    assert size == 40 == C.sizeof(S)
    assert offs == [S.q_first.offset, S.q_count.offset, S.t_first.offset, S.t_count.offset, S.upper.offset, S.reserved.offset] == [0, 8, 16, 24, 32, 36]
