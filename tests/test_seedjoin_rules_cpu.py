"""The seed join without a GPU: aligner_amd/csrc/aln_seedjoin_rules.h driven through a small C++ program and compared with
seedjoin_ref.py (the A^k cap at 2^32 for k up to 16, the sort key and the diagonal's bias at the ends of int32_t, the band count on
hand-made multisets of diagonals, the cut of row totals into chunks and the cut at 2^32 pairs), the same program once more built as a
stand-alone program with the address and undefined-behaviour sanitizers; the companion header include/aligner_hip_seedjoin.h against its
mirrors (_ffi.SEEDJOIN_EXPORTS, the ctypes classes, tests/abi_seedjoin.c) and compiled as C99; the refusals that need no device; the
command's new argument errors."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedjoin_ref as R  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_seedjoin_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "cap")) {            // lines `k A` -> A^k or 0
        uint32_t k, a;
        while (scanf("%" SCNu32 " %" SCNu32, &k, &a) == 2) printf("%" PRIu64 "\n", aln_seedjoin_words(k, a));
        return 0;
    }
    if (!strcmp(argv[1], "word")) {           // lines `k A c0 .. c(k-1)` -> the word's number or -
        uint32_t k, a;
        while (scanf("%" SCNu32 " %" SCNu32, &k, &a) == 2) {
            std::vector<uint8_t> s(k + 1);
            for (uint32_t i = 0; i < k; ++i) { unsigned c; if (scanf("%u", &c) != 1) return 2; s[i] = (uint8_t)c; }
            uint32_t w;
            if (aln_prefilter_word(s.data(), k, a, &w)) printf("%" PRIu32 "\n", w); else printf("-\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "key")) {            // lines `rel_pair pq pt` -> d key, after the way back has been checked
        uint64_t rel;
        uint32_t pq, pt;
        while (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &rel, &pq, &pt) == 3) {
            const int32_t d = aln_seedjoin_diag(pq, pt);
            const uint64_t key = aln_seedjoin_key(rel, d);
            if (aln_seedjoin_key_pair(key) != rel || aln_seedjoin_key_diag(key) != d || aln_seedjoin_unbias(aln_seedjoin_bias(d)) != d) return 3;
            printf("%" PRId32 " %" PRIu64 "\n", d, key);
        }
        return 0;
    }
    if (!strcmp(argv[1], "window")) {         // lines `rel_pair band n d0 .. d(n-1)` -> seeds diag
        uint64_t rel, n;
        uint32_t band;
        while (scanf("%" SCNu64 " %" SCNu32 " %" SCNu64, &rel, &band, &n) == 3) {
            std::vector<uint64_t> keys(n);
            for (uint64_t i = 0; i < n; ++i) { int64_t d; if (scanf("%" SCNd64, &d) != 1) return 2; keys[i] = aln_seedjoin_key(rel, (int32_t)d); }
            std::sort(keys.begin(), keys.end());
            uint64_t seeds;
            int32_t diag;
            aln_seedjoin_best_window(keys.data(), n, band, &seeds, &diag);
            printf("%" PRIu64 " %" PRId32 "\n", seeds, diag);
        }
        return 0;
    }
    if (!strcmp(argv[1], "cut")) {            // lines `cap q_count t_count upper seeds0 .. seeds(q_count-1)` -> `first rows` per chunk, or `over <row>`
        uint64_t cap;
        aln_seqset_block b;
        memset(&b, 0, sizeof b);
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu32, &cap, &b.q_count, &b.t_count, &b.upper) == 4) {
            std::vector<uint64_t> seeds(b.q_count);
            for (uint64_t i = 0; i < b.q_count; ++i) if (scanf("%" SCNu64, &seeds[i]) != 1) return 2;
            bool over = false;
            for (uint64_t first = 0; first < b.q_count && !over;) {
                const uint64_t n = aln_seedjoin_cut(seeds.data(), b, first, cap);
                if (!n) { printf(" over %" PRIu64, first); over = true; }
                else {
                    if (aln_seedjoin_row_pairs(b, first, n) > ALN_SEEDJOIN_MAX_CHUNK_PAIRS) return 3;
                    printf(" %" PRIu64 " %" PRIu64, first, n); first += n;
                }
            }
            printf("\n");
        }
        return 0;
    }
    return 2;
}
"""


def compile_driver(tmp, name, extra):
    cxx = os.environ.get("CXX", "g++")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the plain driver, and the same source as a stand-alone program under the address and undefined-behaviour sanitizers"""
    tmp = tmp_path_factory.mktemp("seedjoin_rules")
    return [compile_driver(tmp, "drv", []), compile_driver(tmp, "drv_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def run(drivers, what, lines):
    """Both programs on the same input: the sanitized one must end clean and print the same."""
    outs = []
    for drv in drivers:
        p = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=120)
        assert p.returncode == 0, (drv, p.returncode, p.stderr[-2000:])
        outs.append(p.stdout.splitlines())
    assert outs[0] == outs[1]
    return outs[0]


# ---------------------------------------------------------------- the rules header against the reference
def test_the_cap_at_two_to_the_32_for_k_up_to_16(drivers):
    cases = [(k, a) for k in range(0, 19) for a in (0, 1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 20, 21, 23, 24, 255, 256, 257, 1625, 1626, 65535, 65536, 65537, 2 ** 32 - 1)]
    out = run(drivers, "cap", ["%d %d" % c for c in cases])
    assert len(out) == len(cases)
    for (k, a), line in zip(cases, out):
        assert int(line) == R.n_word_numbers(k, a), (k, a)
    # at the cap and past it: 4^16 = 16^8 = 256^4 = 65536^2 = 2^32 are taken; one code more is not; k = 17 is not whatever A
    for k, a in ((16, 4), (8, 16), (4, 256), (2, 65536)):
        assert R.n_word_numbers(k, a) == 2 ** 32 and R.n_word_numbers(k, a + 1) == 0
    assert R.n_word_numbers(16, 5) == 0 and R.n_word_numbers(17, 1) == 0 and R.n_word_numbers(17, 4) == 0 and R.n_word_numbers(16, 1) == 1
    assert R.n_word_numbers(7, 20) == 20 ** 7 and R.n_word_numbers(8, 20) == 0 and R.n_word_numbers(13, 5) == 5 ** 13 and R.n_word_numbers(14, 5) == 0
    assert R.n_word_numbers(16, 3) == 3 ** 16 and R.n_word_numbers(15, 4) == 2 ** 30


def test_word_numbers_of_sixteen_residues(drivers):
    rng = random.Random(16)
    cases = [(16, 4, [3] * 16), (16, 4, [0] * 16), (16, 4, [3] * 15 + [4]), (16, 4, [2, 0] * 8), (7, 20, [19] * 7), (7, 20, [19] * 6 + [20]), (13, 5, [4] * 13)]
    cases += [(k, a, [rng.randrange(a + (rng.random() < 0.1)) for _ in range(k)]) for k, a in ((16, 4), (12, 4), (15, 4), (7, 20), (16, 3)) for _ in range(40)]
    out = run(drivers, "word", ["%d %d %s" % (k, a, " ".join(map(str, s))) for k, a, s in cases])
    for (k, a, s), line in zip(cases, out):
        w = R.word(s, a)
        assert line == ("-" if w is None else str(w)), (k, a, s)
    assert out[0] == str(2 ** 32 - 1) and out[1] == "0" and out[2] == "-"


def test_the_key_and_the_bias_at_the_ends_of_int32(drivers):
    top = 2 ** 31 - 1
    cases = [(0, 0, 0), (0, top, 0), (0, 0, top), (2 ** 32 - 1, top, 0), (2 ** 32 - 1, 0, top), (7, 5, 4), (7, 4, 5), (1, top, top), (2 ** 31, 1, 0)]
    rng = random.Random(3)
    cases += [(rng.randrange(2 ** 32), rng.randrange(2 ** 31), rng.randrange(2 ** 31)) for _ in range(200)]
    out = run(drivers, "key", ["%d %d %d" % c for c in cases])
    keys = []
    for (rel, pq, pt), line in zip(cases, out):
        d, key = [int(x) for x in line.split()]
        assert d == pt - pq and key == R.sort_key(rel, d) and 0 <= key < 2 ** 64, (rel, pq, pt)
        keys.append((key, rel, d))
    # ascending keys are ascending by (pair, diagonal), the negative diagonals first
    assert [(rel, d) for _k, rel, d in sorted(keys)] == sorted((rel, d) for _k, rel, d in keys)
    assert R.sort_key(0, -top) == 1 and R.sort_key(0, top) == 2 ** 32 - 1 and R.sort_key(2 ** 32 - 1, top) == 2 ** 64 - 1


def test_the_band_count_on_hand_made_multisets(drivers):
    lo, hi = -(2 ** 31), 2 ** 31 - 1
    cases = [
        (0, [5]), (0, [5, 5, 5]), (0, [1, 2, 2, 3, 3, 3]), (0, [3, 3, 1, 1]),                      # band 0: the fullest diagonal, the least of equals
        (4, [10, 14]), (4, [10, 15]), (4, [10, 14, 15]), (4, [10, 10, 15, 15, 15]),                # d0 + band is in, d0 + band + 1 is out
        (3, [0, 1, 10, 11]), (3, [10, 11, 0, 1]), (3, [0, 0, 9, 9]),                               # equal counts: the least d0
        (2, [-7, -6, -5, 1]), (2, [-1, 0, 1]), (1, [-3, -3, -1, -1, -1]), (5, [-100, 100]),        # negative diagonals
        (0, [lo]), (0, [hi]), (hi, [lo, -1, hi]), (hi, [0, hi]), (hi, [lo, hi]), (hi, [1, hi]), (1, [hi - 1, hi]), (1, [lo, lo + 1, lo + 2]),
        (hi, [-1, hi - 1, hi]), (2, [hi - 1, hi, hi]),                                             # a band that would pass the largest diagonal
    ]
    rng = random.Random(11)
    for _ in range(300):
        span = rng.choice([3, 10, 50, 2000])
        cases.append((rng.choice([0, 1, 2, 5, 16, 100]), [rng.randrange(-span, span + 1) for _ in range(rng.randrange(1, 40))]))
    pairs = [rng.choice([0, 1, 77, 2 ** 32 - 1]) for _ in cases]
    out = run(drivers, "window", ["%d %d %d %s" % (p, band, len(ds), " ".join(map(str, ds))) for p, (band, ds) in zip(pairs, cases)])
    assert len(out) == len(cases)
    for (band, ds), line in zip(cases, out):
        assert tuple(int(x) for x in line.split()) == R.best_window(ds, band), (band, ds)
    # the edges, spelled out
    assert R.best_window([10, 14], 4) == (2, 10) and R.best_window([10, 15], 4) == (1, 10) and R.best_window([10, 14, 15], 4) == (2, 10)
    assert R.best_window([10, 10, 15, 15, 15], 4) == (3, 15) and R.best_window([10, 11, 0, 1], 3) == (2, 0) and R.best_window([3, 3, 1, 1], 0) == (2, 1)
    assert R.best_window([lo, -1, hi], hi) == (2, lo) and R.best_window([-1, hi - 1, hi], hi) == (2, -1) and R.best_window([lo, hi], hi) == (1, lo)


def test_chunk_cutting(drivers):
    rng = random.Random(7)
    cases = [(10, 3, 0, [10]), (10, 3, 0, [11]), (10, 3, 0, [0, 0, 0]), (10, 4, 0, [0, 10, 0, 0, 10, 1]), (10, 2, 0, [3, 3, 3, 3, 3]),
             (10, 9, 1, [5, 5, 5, 6, 4, 0, 0, 0, 0]), (10, 1, 0, [0, 0, 11]), (1, 1, 0, [1, 1, 0, 1]), (2 ** 26, 5, 0, [2 ** 26, 1, 2 ** 26 - 1, 1]),
             (2 ** 26, 5, 0, [2 ** 40])]
    cases += [(rng.randrange(20, 41), rng.randrange(1, 50), 0, [rng.choice([0, 0, 1, 2, 5, 9, 20] * 8 + [39, 40]) for _ in range(rng.randrange(1, 30))]) for _ in range(150)]
    for _ in range(50):
        n = rng.randrange(2, 30)
        cases.append((rng.randrange(20, 41), n, 1, [rng.choice([0, 0, 1, 2, 5, 9, 20]) for _ in range(n - 1)] + [0]))
    # the cut at 2^32 pairs: rows of 2^31 pairs go two by two, rows of one pair more one by one, whatever the seeds allow
    cases += [(100, 2 ** 31, 0, [0] * 7), (100, 2 ** 31 + 1, 0, [1] * 5), (100, 2 ** 32 - 1, 0, [0] * 3), (100, 2 ** 30, 0, [1] * 9), (3, 2 ** 30, 0, [1] * 9),
              (100, 2 ** 31, 0, [0, 0, 0, 101, 0]), (1, 100000, 1, [0] * 100000), (2 ** 26, 150000, 1, [1] * 149999 + [0])]
    out = run(drivers, "cut", ["%d %d %d %d %s" % (cap, len(seeds), tc, up, " ".join(map(str, seeds))) for cap, tc, up, seeds in cases])
    assert len(out) == len(cases)
    seen_over = seen_pairs = 0
    for (cap, tc, up, seeds), line in zip(cases, out):
        tok = line.split()
        block = (0, len(seeds), 0, len(seeds) if up else tc, up)
        want = R.cut(seeds, cap, block)
        if want is None:
            assert "over" in tok and seeds[int(tok[tok.index("over") + 1])] > cap and tok.index("over") == len(tok) - 2
            seen_over += 1
            continue
        got = list(zip([int(x) for x in tok[0::2]], [int(x) for x in tok[1::2]]))
        assert got == want, (cap, tc, up, seeds[:20])
        assert [f for f, n in got] == [sum(n for _f, n in got[:i]) for i in range(len(got))] and sum(n for _f, n in got) == len(seeds)
        for f, n in got:
            assert n >= 1 and sum(seeds[f:f + n]) <= cap and R.row_pairs(block, f, n) <= 2 ** 32
            if f + n < len(seeds):
                by_pairs = R.row_pairs(block, f, n + 1) > 2 ** 32
                assert sum(seeds[f:f + n + 1]) > cap or by_pairs
                seen_pairs += by_pairs
    assert seen_over > 5 and seen_pairs > 5
    assert R.cut([0] * 7, 100, (0, 7, 0, 2 ** 31, 0)) == [(0, 2), (2, 2), (4, 2), (6, 1)]
    assert R.cut([1] * 5, 100, (0, 5, 0, 2 ** 31 + 1, 0)) == [(k, 1) for k in range(5)]
    assert len(R.cut([0] * 100000, 1, (0, 100000, 0, 100000, 1))) == 2


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_seedjoin_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_seedjoin.h")) == sorted(_ffi.SEEDJOIN_EXPORTS)
    assert _ffi.SEEDJOIN_EXPORTS == ["aln_seqset_candidate_diags", "aln_seqset_seed_index", "aln_seqset_seed_join"]
    # the pinned ones are as they were
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61 and len(_ffi.PREFILTER_EXPORTS) == 5
    assert _ffi.WORDJOIN_EXPORTS == ["aln_seqset_word_index", "aln_seqset_word_join"]
    others = [getattr(_ffi, name) for name in dir(_ffi) if name.endswith("EXPORTS") and name != "SEEDJOIN_EXPORTS"]
    assert len(others) >= 9
    for lst in others:
        assert not set(_ffi.SEEDJOIN_EXPORTS) & set(lst)
    assert "aln_seedjoin.hip" in native_build.SOURCES and "aln_seedjoin_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_seedjoin.h") for h in native_build.HEADERS)
    text = strip_comments(open(os.path.join(ROOT, "include", "aligner_hip_seedjoin.h")).read())
    assert '#include "aligner_hip_wordjoin.h"' in text


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.SEEDJOIN_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_seedjoin.c")).read())
    for sym in _ffi.SEEDJOIN_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_seedjoin.h"\nint main(void) { return (int)sizeof(aln_seedjoin_spec) - 32 + (int)sizeof(aln_seedjoin_summary) - 32; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_seedjoin_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_seedjoin_spec", "aln_seedjoin_summary"]
    for l, cls in zip(lines, (_ffi.SeedjoinSpec, _ffi.SeedjoinSummary)):
        assert int(l[2]) == C.sizeof(cls) == 32
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert [name for name, _t in _ffi.SeedjoinSpec._fields_] == ["k", "alphabet", "min_seeds", "band", "max_occ", "chunk_seeds", "flags", "reserved"]
    assert [name for name, _t in _ffi.SeedjoinSummary._fields_] == ["seeds", "pairs_with_seed", "words_dropped", "chunks"]
    assert (_ffi.SEEDJOIN_MAX_K, _ffi.SEEDJOIN_MAX_WORDS, _ffi.SEEDJOIN_MAX_BAND) == (R.MAX_K, R.MAX_WORDS, R.MAX_BAND)
    assert (_ffi.SEEDJOIN_CHUNK_SEEDS, _ffi.SEEDJOIN_MAX_CHUNK_SEEDS) == (R.CHUNK_SEEDS, R.MAX_CHUNK_SEEDS)


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    occ = C.c_uint64(99)
    count = C.c_uint64(99)
    diag = (C.c_int32 * 4)(7, 7, 7, 7)
    summ = _ffi.SeedjoinSummary(5, 5, 5, 5)
    spec = _ffi.SeedjoinSpec(12, 4, 1, 0, 0, 0, 0, 0)
    blk = _ffi.SeqsetBlock(0, 2, 0, 2, 1, 0)

    def untouched():
        return occ.value == 99 and count.value == 99 and list(diag) == [7] * 4 and (summ.seeds, summ.pairs_with_seed, summ.words_dropped, summ.chunks) == (5, 5, 5, 5)

    assert lib.aln_seqset_seed_index(None, 12, 4, C.byref(occ)) == INV and untouched()
    assert lib.aln_seqset_seed_index(None, 12, 4, None) == INV and untouched()
    assert lib.aln_seqset_seed_join(None, C.byref(spec), C.byref(blk), C.byref(summ), C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_seed_join(None, None, C.byref(blk), None, C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_seed_join(None, C.byref(spec), None, C.byref(summ), None) == INV and untouched()
    assert lib.aln_seqset_candidate_diags(None, 0, 4, diag) == INV and untouched()
    assert b"null" in lib.aln_last_error()


# ---------------------------------------------------------------- the command's new argument errors
@pytest.mark.parametrize("extra,message", [
    (["--seed-join"], "error: --seed-join is a route of the prefilter: give --kmer K"),
    (["--kmer", "5", "--seed-join", "--word-join"], "error: --seed-join with --word-join: both name the route"),
    (["--kmer", "5", "--seed-join", "--min-shared", "2"], "error: --min-shared / --min-shared-per-1024 count distinct shared words"),
    (["--kmer", "5", "--seed-join", "--min-shared-per-1024", "10"], "error: --min-shared / --min-shared-per-1024 count distinct shared words"),
    (["--kmer", "8", "--seed-join"], "error: --kmer with --seed-join: K must lie in 1 .. 16 and A^K may not exceed 2^32"),        # 20^8 > 2^32
    (["--kmer", "17", "--dna", "--seed-join"], "error: --kmer with --seed-join: K must lie in 1 .. 16 and A^K may not exceed 2^32"),
    (["--kmer", "5", "--seed-join", "--min-seeds", "0"], "error: --min-seeds: N must lie in 1 .. 2^32 - 1"),
    (["--kmer", "5", "--seed-join", "--band", "-1"], "error: --band: B must lie in 0 .. 2^31 - 1"),
    (["--kmer", "5", "--seed-join", "--band", str(2 ** 31)], "error: --band: B must lie in 0 .. 2^31 - 1"),
    (["--kmer", "5", "--seed-join", "--max-occ", "-1"], "error: --max-occ: C must lie in 0 .. 2^32 - 1"),
    (["--kmer", "5", "--min-seeds", "2"], "error: --min-seeds / --band / --max-occ are the thresholds of --seed-join"),
    (["--kmer", "5", "--word-join", "--band", "2"], "error: --min-seeds / --band / --max-occ are the thresholds of --seed-join"),
    (["--max-occ", "2"], "error: --min-seeds / --band / --max-occ are the thresholds of --seed-join"),
    (["--kmer", "5", "--seed-join", "--best", "2"], "error: --kmer with --best: --best aligns every pair"),
    (["--kmer", "5", "--seed-join", "--heuristic", "--kd", "1", "--r-squared", "0.5"], "error: --kmer with --heuristic: the matrix loop"),
])
def test_the_commands_argument_errors(tmp_path, capsys, extra, message):
    """The refusal's own message, not an option's name: argparse prints every option's name in the usage line of any error."""
    from aligner_amd import allpairs
    fa = tmp_path / "x.fasta"
    fa.write_text(">a\nACDEFGHIK\n>b\nACDEFGHIK\n")
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", str(fa)] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err and "unrecognized arguments" not in err


def test_k_goes_up_to_16_on_this_route_only(tmp_path, capsys):
    """--kmer 16 --dna gets past the check of K with --seed-join (the error is the next check's, the band's), and with neither of the
    other two routes."""
    from aligner_amd import allpairs
    fa = tmp_path / "x.fasta"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n>b\nACGTACGTACGTACGTACGT\n")
    for extra, message in ((["--seed-join", "--band", "-1"], "error: --band: B must lie in 0 .. 2^31 - 1"),
                           (["--word-join"], "error: --kmer with --word-join: K must lie in 1 .. 8"),
                           ([], "error: --kmer: K must lie in 1 .. 8")):
        with pytest.raises(SystemExit) as e:
            allpairs.main(["-i", str(fa), "--dna", "--kmer", "16"] + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err and "unrecognized arguments" not in err
