"""The rule of aln_seqset_best (aln_best_rules.h; no GPU): the header compiled into a driver with the host compiler and checked against
restatements in Python integers and numpy -- the key's order over the awkward doubles, who is a candidate, the rows and pieces of
every small chunk and of chunks cut at, one before and one after a row or piece edge (also near pair number 2^40), and a host replay
of piece-then-fold, the way the kernels of aln_best.hip run it, against numpy.lexsort -- plus the export, its argument types and the
refusals that need no device."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd import seqset as seqset_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 2048
M64 = (1 << 64) - 1

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "aln_best_rules.h"
typedef unsigned long long ull;
static void geometry(uint64_t k0, uint64_t n, uint64_t tc)
{
    const aln_best_chunk g = aln_best_chunk_geometry(k0, n, tc);
    printf("G %llu %llu %llu %llu %llu %llu\n", (ull)k0, (ull)n, (ull)tc, (ull)g.row0, (ull)g.rows, (ull)g.pieces);
    for (uint64_t j = 0; j < g.rows; ++j) {
        uint64_t s, l, p0, np;
        aln_best_row_segment(g, tc, j, &s, &l, &p0, &np);
        printf("R %llu %llu %llu %llu\n", (ull)s, (ull)l, (ull)p0, (ull)np);
    }
    for (uint64_t p = 0; p < g.pieces; ++p) {
        uint64_t j, s, l;
        aln_best_piece(g, tc, p, &j, &s, &l);
        printf("P %llu %llu %llu\n", (ull)j, (ull)s, (ull)l);
    }
}
// one row through the kernels' steps: per segment of the row (a chunk's share), per piece of <= ALN_BEST_PIECE pairs: the
// candidates ranked by counting, the first min(cap, candidates) folded into the running list
static void replay(void)
{
    ull cap, fmin_bits, flags, q, t_first, T, ncuts;
    while (scanf("%llu %llx %llu %llu %llu %llu %llu", &cap, &fmin_bits, &flags, &q, &t_first, &T, &ncuts) == 7) {
        std::vector<ull> cuts(ncuts);
        for (ull i = 0; i < ncuts; ++i) if (scanf("%llu", &cuts[i]) != 1) exit(4);
        std::vector<int32_t> status(T);
        std::vector<double> f(T);
        for (ull i = 0; i < T; ++i) {
            int st; ull bits;
            if (scanf("%d %llx", &st, &bits) != 2) exit(4);
            status[i] = st; uint64_t b = bits; memcpy(&f[i], &b, 8);
        }
        double f_min; { uint64_t b = fmin_bits; memcpy(&f_min, &b, 8); }
        std::vector<uint64_t> run_key(cap), out_key(cap), pk, sk(cap);
        std::vector<uint32_t> run_t(cap), out_t(cap), pt, st_(cap);
        uint32_t run_n = 0;
        cuts.push_back(T);
        ull lo = 0;
        for (ull c = 0; c < cuts.size(); ++c) {
            const ull hi = cuts[c];
            for (ull a = lo; a < hi; a += ALN_BEST_PIECE) {
                const ull b = a + ALN_BEST_PIECE < hi ? a + ALN_BEST_PIECE : hi;
                pk.clear(); pt.clear();
                for (ull i = a; i < b; ++i)
                    if (aln_best_candidate(status[i], f[i], f_min, q, t_first + i, (uint32_t)flags)) { pk.push_back(aln_best_key(f[i])); pt.push_back((uint32_t)(t_first + i)); }
                uint32_t nb = 0;
                for (size_t i = 0; i < pk.size(); ++i) {
                    const uint32_t at = aln_best_count_before(pk.data(), pt.data(), (uint32_t)pk.size(), pk[i], pt[i]);
                    if (at < cap) { sk[at] = pk[i]; st_[at] = pt[i]; ++nb; }
                }
                run_n = aln_best_fold(run_key.data(), run_t.data(), run_n, sk.data(), st_.data(), nb, (uint32_t)cap, out_key.data(), out_t.data());
                run_key.swap(out_key); run_t.swap(out_t);
            }
            lo = hi;
        }
        printf("N %u", run_n);
        for (uint32_t i = 0; i < run_n; ++i) {
            const double v = aln_best_unkey(run_key[i]);
            uint64_t b; memcpy(&b, &v, 8);
            printf(" %u %llx", run_t[i], (ull)b);
        }
        printf("\n");
    }
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "key")) {              // key <f bits in hex> ...  -> key, bits of unkey(key)
        for (int i = 2; i < argc; ++i) {
            uint64_t b = strtoull(argv[i], 0, 16); double f; memcpy(&f, &b, 8);
            const uint64_t k = aln_best_key(f);
            const double back = aln_best_unkey(k); uint64_t bb; memcpy(&bb, &back, 8);
            printf("%llu %llu\n", (ull)k, (ull)bb);
        }
        return 0;
    }
    if (!strcmp(argv[1], "cand")) {             // cand <status> <f bits> <f_min bits> <q> <t> <flags> (repeated)
        for (int i = 2; i + 5 < argc; i += 6) {
            uint64_t a = strtoull(argv[i + 1], 0, 16), b = strtoull(argv[i + 2], 0, 16); double f, m; memcpy(&f, &a, 8); memcpy(&m, &b, 8);
            printf("%d\n", (int)aln_best_candidate(atoi(argv[i]), f, m, strtoull(argv[i + 3], 0, 10), strtoull(argv[i + 4], 0, 10), (uint32_t)atoi(argv[i + 5])));
        }
        return 0;
    }
    if (!strcmp(argv[1], "before")) {           // before <key a> <t a> <key b> <t b> (repeated)
        for (int i = 2; i + 3 < argc; i += 4)
            printf("%d\n", (int)aln_best_before(strtoull(argv[i], 0, 10), (uint32_t)strtoul(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10), (uint32_t)strtoul(argv[i + 3], 0, 10)));
        return 0;
    }
    if (!strcmp(argv[1], "sweep")) {            // sweep <max t_count> <max k0 + n>: every chunk
        const uint64_t tmax = strtoull(argv[2], 0, 10), kmax = strtoull(argv[3], 0, 10);
        for (uint64_t tc = 1; tc <= tmax; ++tc)
            for (uint64_t k0 = 0; k0 < kmax; ++k0)
                for (uint64_t n = 1; k0 + n <= kmax; ++n) geometry(k0, n, tc);
        return 0;
    }
    if (!strcmp(argv[1], "geom")) {             // geom <k0> <n> <t_count> (repeated)
        for (int i = 2; i + 2 < argc; i += 3) geometry(strtoull(argv[i], 0, 10), strtoull(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10));
        return 0;
    }
    if (!strcmp(argv[1], "slots")) { printf("%u\n", aln_best_slots((uint32_t)atoi(argv[2]), strtoull(argv[3], 0, 10))); return 0; }
    if (!strcmp(argv[1], "replay")) { replay(); return 0; }
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the best-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("best_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe])
    return exe


def _run(drv, *args, stdin=None):
    return subprocess.run([drv] + [str(a) for a in args], check=True, capture_output=True, text=True, input=stdin).stdout.splitlines()


def bits(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def unbits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def awkward():
    """+-0, +-denormals, +-1, values one ulp apart, +-inf (NaN apart)."""
    one = bits(1.0)
    pos = [0, 1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, one - 1, one, one + 1, bits(12.0), bits(12.0) + 1, bits(1e300), 0x7FEFFFFFFFFFFFFF,
           0x7FF0000000000000]
    return pos + [b | (1 << 63) for b in pos]


NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF]


def test_key_order_is_the_order_of_the_doubles(driver):
    vals = awkward()
    out = [[int(v) for v in line.split()] for line in _run(driver, "key", *["%x" % b for b in vals])]
    keys = [o[0] for o in out]
    for a, ka in zip(vals, keys):
        for b, kb in zip(vals, keys):
            fa, fb = unbits(a), unbits(b)
            assert (ka < kb) == (fa < fb) and (ka == kb) == (fa == fb), (hex(a), hex(b))
    assert keys[vals.index(0)] == keys[vals.index(1 << 63)]                       # -0.0 is folded onto +0.0
    assert all(k != 0 for k in keys)                                             # key 0 is free for the kernels' sentinel
    for b, o in zip(vals, out):                                                  # the key gives the double back (+0.0 for either zero)
        assert o[1] == (0 if b == 1 << 63 else b), hex(b)
    # before(): higher key first, equal keys by the lower target
    quads, want = [], []
    for ka in (keys[0], keys[3], keys[-1]):
        for kb in (keys[0], keys[3], keys[-1]):
            for ta, tb in ((5, 7), (7, 5), (0, 2 ** 32 - 1)):
                quads += [ka, ta, kb, tb]
                want.append(int(ka > kb or (ka == kb and ta < tb)))
    assert [int(v) for v in _run(driver, "before", *quads)] == want


def test_candidates(driver):
    """status, NaN on either side, the threshold as a plain compare, -0.0 against +0.0, the self pair."""
    inf = float("inf")
    cases = []
    for status in (0, 2, 4):
        for f in [unbits(b) for b in awkward()] + [unbits(b) for b in NANS]:
            for f_min in (-inf, -0.0, 0.0, 1.0, 12.0, inf, unbits(NANS[0])):
                for q, t, flags in ((3, 3, 0), (3, 3, 1), (3, 4, 1)):
                    cases.append((status, f, f_min, q, t, flags))
    want = [int(st == 0 and f == f and f >= m and not (flags & 1 and q == t)) for st, f, m, q, t, flags in cases]
    got = []
    for a in range(0, len(cases), 500):
        args = []
        for st, f, m, q, t, flags in cases[a:a + 500]:
            args += [st, "%x" % bits(f), "%x" % bits(m), q, t, flags]
        got += [int(v) for v in _run(driver, "cand", *args)]
    assert got == want
    assert sum(want) > 100 and not any(w for w, c in zip(want, cases) if c[1] != c[1] or c[2] != c[2])    # a NaN selects nothing
    by = {c: w for c, w in zip(cases, want)}
    assert by[(0, -0.0, 0.0, 3, 4, 1)] == 1 and by[(0, 0.0, -0.0, 3, 4, 1)] == 1


def py_geometry(k0, n, tc):
    """Rows and pieces of pair numbers k0 .. k0 + n - 1, by clipping every touched row's range: (row0, rows, [row segments], [pieces])."""
    row0, row1 = k0 // tc, (k0 + n - 1) // tc
    rows, pieces = [], []
    for r in range(row0, row1 + 1):
        lo, hi = max(k0, r * tc), min(k0 + n, (r + 1) * tc)
        cut = list(range(lo, hi, PIECE))
        rows.append((lo - k0, hi - lo, len(pieces), len(cut)))
        for a in cut:
            pieces.append((r - row0, a - k0, min(PIECE, hi - a)))
    return row0, row1 - row0 + 1, rows, pieces


def check_geometry(lines):
    """Every chunk of a driver output against py_geometry; returns the number of chunks."""
    i, chunks = 0, 0
    while i < len(lines):
        head = lines[i].split()
        assert head[0] == "G"
        k0, n, tc, row0, n_rows, n_pieces = [int(v) for v in head[1:]]
        w_row0, w_rows, rows, pieces = py_geometry(k0, n, tc)
        assert (row0, n_rows, n_pieces) == (w_row0, w_rows, len(pieces)), (k0, n, tc)
        got_rows = [tuple(int(v) for v in lines[i + 1 + j].split()[1:]) for j in range(n_rows)]
        assert all(lines[i + 1 + j][0] == "R" for j in range(n_rows)) and got_rows == rows, (k0, n, tc)
        got_pieces = [tuple(int(v) for v in lines[i + 1 + n_rows + j].split()[1:]) for j in range(n_pieces)]
        assert all(lines[i + 1 + n_rows + j][0] == "P" for j in range(n_pieces)) and got_pieces == pieces, (k0, n, tc)
        assert sum(p[2] for p in pieces) == n
        i += 1 + n_rows + n_pieces
        chunks += 1
    return chunks


def test_rows_and_pieces_of_every_small_chunk(driver):
    assert check_geometry(_run(driver, "sweep", 9, 60)) == 9 * 60 * 61 // 2


def test_rows_and_pieces_at_row_and_piece_edges(driver):
    """t_count 1, 2047, 2048, 2049 (and 4200: three pieces per row): chunks that begin and end on, one before and one after a row
    or piece edge; the same around pair number 2^40."""
    args = []
    for tc in (1, 2047, 2048, 2049, 4200):
        edges = sorted({e + d for r in (0, 1, 2, 3) for e in (r * tc, r * tc + PIECE, r * tc + 2 * PIECE) if e <= 3 * tc for d in (-1, 0, 1) if e + d >= 0})
        for base in (0, (2 ** 40 // tc) * tc, (2 ** 40 // tc) * tc + 5):
            for a in edges:
                for b in edges:
                    if b > a:
                        args += [base + a, b - a, tc]
    n = 0
    for a in range(0, len(args), 3000):
        n += check_geometry(_run(driver, "geom", *args[a:a + 3000]))
    assert n == len(args) // 3 > 2000
    for k, tc, want in ((64, 1, 1), (64, 63, 63), (64, 64, 64), (64, 10 ** 12, 64), (1, 5, 1)):
        assert _run(driver, "slots", k, tc) == [str(want)]


def lexsort_best(status, f, f_min, q, t_first, flags, cap):
    """numpy's answer: the candidates of the row by descending f (-0.0 == +0.0), equal f by ascending target, the first cap."""
    t = t_first + np.arange(len(f), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = (status == 0) & (f == f) & (f >= f_min)
    if flags & 1:
        ok &= t != q
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((t[idx], -(f[idx] + 0.0)))][:cap]
    return t[order], f[order] + 0.0


def test_host_replay_of_piece_then_fold(driver):
    """Random rows with heavy ties (a handful of distinct f, -0.0 and +0.0, NaN, failed pairs), random chunk cuts, k in 1, 2, 63, 64;
    rows of up to three pieces; the self pair skipped or not."""
    rng = np.random.default_rng(20261018)
    levels = np.array([-3.5, -0.0, 0.0, 0.37, 5.0, 5.0 + 2 ** -50, 12.0, float("inf"), float("-inf"), float("nan")])
    text, want = [], []
    for case in range(48):
        cap = (1, 2, 63, 64)[case % 4]
        T = int(rng.choice([1, 2, 5, 63, 64, 65, 130, 2047, 2048, 2049, 4200, 5000])) if case >= 8 else (1, 2, 64, 65, 2048, 2049, 4097, 4200)[case]
        f = levels[rng.integers(0, len(levels) if case % 3 else 4, T)]
        status = np.where(rng.random(T) < 0.15, rng.choice([2, 3, 4], T), 0).astype(np.int32)
        if case % 5 == 0:
            status[:] = np.where(rng.random(T) < 0.995, 4, 0)                      # fewer candidates than k
        t_first = int(rng.choice([0, 7, 2 ** 32 - 1 - T]))
        q = t_first + int(rng.integers(0, T))
        flags = case % 2
        f_min = [float("-inf"), 0.0, 5.0, float("nan")][case % 4 if case % 7 else 0]
        cuts = sorted(set(rng.integers(1, T, int(rng.integers(0, 6))).tolist())) if T > 1 else []
        text.append("%d %x %d %d %d %d %d %s" % (min(cap, T), bits(f_min), flags, q, t_first, T, len(cuts), " ".join(str(c) for c in cuts)))
        text.append(" ".join("%d %x" % (s, bits(v)) for s, v in zip(status.tolist(), f.tolist())))
        want.append(lexsort_best(status, f, f_min, q, t_first, flags, min(cap, T)))
    out = _run(driver, "replay", stdin="\n".join(text) + "\n")
    assert len(out) == len(want)
    sizes = set()
    for line, (wt, wf) in zip(out, want):
        tok = line.split()
        n = int(tok[1])
        got_t = [int(v) for v in tok[2::2]]
        got_f = [int(v, 16) for v in tok[3::2]]
        assert n == len(wt) and got_t == wt.tolist() and got_f == [bits(v) for v in wf.tolist()]
        sizes.add(n)
    assert {0, 1, 2, 63, 64} <= sizes


def test_python_ranks_follow_the_rule():
    q = np.array([4, 4, 4, 4, 2, 2, 9], dtype=np.uint32)
    t = np.array([0, 1, 2, 3, 7, 8, 1], dtype=np.uint32)
    f = np.array([5.0, 7.0, 5.0, -0.0, 0.0, -0.0, 3.0])
    assert seqset_module.best_ranks(q, t, f).tolist() == [1, 0, 2, 3, 0, 1, 0]
    assert seqset_module.best_ranks(q[:0], t[:0], f[:0]).tolist() == []


@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def test_library_exports_best_with_the_headers_arguments(lib):
    text = open(os.path.join(ROOT, "include", "aligner_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "aln_seqset_best" in _ffi.EXPORTS and hasattr(lib, "aln_seqset_best")
    decl = re.search(r"\baln_seqset_best\s*\(([^;]*)\)\s*;", hdr)
    assert decl
    args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    at = lib.aln_seqset_best.argtypes
    assert len(at) == len(args) == 7
    assert at[3] is C.c_uint32 and at[4] is C.c_double and at[5] is C.c_uint32 and at[6] == C.POINTER(C.c_uint64)
    assert args[3].startswith("uint32_t") and args[4].startswith("double") and args[5].startswith("uint32_t") and args[6].startswith("uint64_t *")
    assert re.search(r"#define\s+ALN_SEQSET_BEST_MAX\s+64u", hdr) and _ffi.SEQSET_BEST_MAX == 64
    assert re.search(r"#define\s+ALN_BEST_SKIP_SELF\s+1u", hdr) and _ffi.BEST_SKIP_SELF == 1
    assert lib.aln_abi_version() == 2


def test_best_refusals_without_a_device(lib):
    count = C.c_uint64(0xABCDEF)
    b = _ffi.SeqsetBlock(0, 2, 0, 2, 0, 0)
    assert lib.aln_seqset_best(None, None, None, 1, 0.0, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_best(None, None, C.byref(b), 1, 0.0, 0, C.byref(count)) == _ffi.ERR_INVALID_ARGUMENT
    assert count.value == 0xABCDEF
    assert callable(seqset_module.SeqSet.best) and issubclass(seqset_module.BestHits, seqset_module.HeldHits)
