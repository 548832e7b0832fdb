"""The word join without a GPU: aligner_amd/csrc/aln_wordjoin_rules.h driven through a small C++ program and compared with
wordjoin_ref.py (word numbers beyond the bitmap cap, the A^k cap at 2^32, the bits a sort needs, the keys, the cut of row totals into
chunks), the same program once more built with the address and undefined-behaviour sanitizers; the companion header
include/aligner_hip_wordjoin.h against its mirrors (_ffi.WORDJOIN_EXPORTS, the ctypes class, tests/abi_wordjoin.c); the refusals that
need no device; the new argument errors of the command."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wordjoin_ref as R  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_wordjoin_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "cap")) {            // lines `k A` -> A^k or 0
        uint32_t k, a;
        while (scanf("%" SCNu32 " %" SCNu32, &k, &a) == 2) printf("%" PRIu64 "\n", aln_wordjoin_words(k, a));
        return 0;
    }
    if (!strcmp(argv[1], "bits")) {           // lines `n` -> bits needed
        uint64_t n;
        while (scanf("%" SCNu64, &n) == 1) printf("%" PRIu32 "\n", aln_wordjoin_bits_needed(n));
        return 0;
    }
    if (!strcmp(argv[1], "sortbits")) {       // lines `words n_seqs` -> seq_end word_end
        uint64_t w, n;
        while (scanf("%" SCNu64 " %" SCNu64, &w, &n) == 2) {
            uint32_t se, we;
            aln_wordjoin_sort_bits(w, n, &se, &we);
            printf("%" PRIu32 " %" PRIu32 "\n", se, we);
        }
        return 0;
    }
    if (!strcmp(argv[1], "words")) {          // lines `k A seq n c0 .. c(n-1)` -> windows, then per window `word key` or `- -`
        uint32_t k, a, seq, n;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &k, &a, &seq, &n) == 4) {
            std::vector<uint8_t> s(n + 1);
            for (uint32_t i = 0; i < n; ++i) { unsigned c; if (scanf("%u", &c) != 1) return 2; s[i] = (uint8_t)c; }
            const uint64_t windows = aln_prefilter_windows(n, k);
            printf("%" PRIu64, windows);
            for (uint64_t i = 0; i < windows; ++i) {
                uint32_t w;
                if (aln_prefilter_word(s.data() + i, k, a, &w)) {
                    const uint64_t key = aln_wordjoin_key(w, seq);
                    if (aln_wordjoin_key_word(key) != w || aln_wordjoin_key_seq(key) != seq || key == ALN_WORDJOIN_NO_KEY) return 3;
                    printf(" %" PRIu32 " %" PRIu64, w, key);
                } else printf(" - -");
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "cut")) {            // lines `cap rows occ0 .. occ(rows-1)` -> `first rows` per chunk, or `over <row>`
        uint64_t cap, rows;
        while (scanf("%" SCNu64 " %" SCNu64, &cap, &rows) == 2) {
            std::vector<uint64_t> occ(rows);
            for (uint64_t i = 0; i < rows; ++i) if (scanf("%" SCNu64, &occ[i]) != 1) return 2;
            bool over = false;
            for (uint64_t first = 0; first < rows && !over;) {
                const uint64_t n = aln_wordjoin_cut(occ.data(), rows, first, cap);
                if (!n) { printf(" over %" PRIu64, first); over = true; }
                else { printf(" %" PRIu64 " %" PRIu64, first, n); first += n; }
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "pwords")) {         // lines `k A max_k` -> A^k or 0
        uint32_t k, a, max_k;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &k, &a, &max_k) == 3) printf("%" PRIu64 "\n", aln_postings_words(k, a, max_k));
        return 0;
    }
    if (!strcmp(argv[1], "bounds")) {         // lines `x n a0 .. a(n-1)` (ascending) -> lower upper, over 64-bit and over 32-bit elements
        uint64_t x, n;
        while (scanf("%" SCNu64 " %" SCNu64, &x, &n) == 2) {
            std::vector<uint64_t> a(n);
            for (uint64_t i = 0; i < n; ++i) if (scanf("%" SCNu64, &a[i]) != 1) return 2;
            printf("%" PRIu64 " %" PRIu64, aln_postings_lower_bound(a.data(), n, x), aln_postings_upper_bound(a.data(), n, x));
            bool narrow = true;
            for (uint64_t v : a) narrow = narrow && v <= 0xFFFFFFFFull;
            if (narrow) {
                std::vector<uint32_t> b(a.begin(), a.end());
                printf(" %" PRIu64 " %" PRIu64, aln_postings_lower_bound(b.data(), n, x), aln_postings_upper_bound(b.data(), n, x));
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "misc")) {           // -> `name first words` of every named range of the set's counter words, then the total
        printf("compact %u 1\nword %u %u\nseed %u %u\ntotal %u\n", ALN_SEQSET_MISC_COMPACT, ALN_SEQSET_MISC_WORD, ALN_SEQSET_MISC_WORD_WORDS,
               ALN_SEQSET_MISC_SEED, ALN_SEQSET_MISC_SEED_WORDS, ALN_SEQSET_MISC_WORDS);
        printf("offsets %u %u %u %u %u\n", ALN_JOIN_MISC_KEPT, ALN_JOIN_MISC_NO_PAIR, ALN_JOIN_MISC_SCANNED, ALN_JOIN_MISC_PAIRS_SEEN, ALN_JOIN_MISC_DROPPED);
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
    tmp = tmp_path_factory.mktemp("wordjoin_rules")
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
def test_the_cap_at_two_to_the_32(drivers):
    cases = [(k, a) for k in range(0, 11) for a in (0, 1, 2, 3, 4, 5, 15, 16, 17, 20, 21, 23, 24, 40, 41, 255, 256, 257, 1625, 1626, 65535, 65536, 65537,
                                                     2 ** 32 - 1)]
    out = run(drivers, "cap", ["%d %d" % c for c in cases])
    assert len(out) == len(cases)
    for (k, a), line in zip(cases, out):
        assert int(line) == R.n_word_numbers(k, a), (k, a)
    # 2^32 itself is taken, 2^32 + 1 and everything above is not: 16^8 = 65536^2 = 2^32; 65537^2 = 2^32 + 2^17 + 1; 4^8 beside 4^... k <= 8
    assert R.n_word_numbers(8, 16) == 2 ** 32 and R.n_word_numbers(2, 65536) == 2 ** 32 and R.n_word_numbers(2, 65537) == 0
    assert R.n_word_numbers(8, 17) == 0 and R.n_word_numbers(1, 2 ** 32 - 1) == 2 ** 32 - 1
    assert R.n_word_numbers(7, 20) == 20 ** 7 and R.n_word_numbers(8, 20) == 0 and R.n_word_numbers(8, 4) == 65536 and R.n_word_numbers(9, 4) == 0
    # the cap as a number: the largest product the loop may see before it refuses is 2^32 * (2^32 - 1) < 2^64
    assert (2 ** 32) * (2 ** 32 - 1) < 2 ** 64


def test_bits_needed(drivers):
    ns = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 20 ** 5, 20 ** 7, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1]
    out = run(drivers, "bits", [str(n) for n in ns])
    assert [int(x) for x in out] == [R.bits_needed(n) for n in ns]
    assert R.bits_needed(2 ** 32) == 32 and R.bits_needed(2 ** 32 + 1) == 33 and R.bits_needed(1) == 0 and R.bits_needed(2 ** 64 - 1) == 64
    # the two ranges of the key sort: the bits each field needs and one more for the all-ones key, capped by the field
    cases = [(20 ** 5, 2000), (4, 1), (2 ** 32, 2 ** 32 - 1), (2 ** 31, 2 ** 31), (2 ** 31 + 1, 2 ** 31 + 1), (1, 300)]
    out = run(drivers, "sortbits", ["%d %d" % c for c in cases])
    for (w, n), line in zip(cases, out):
        se, we = [int(x) for x in line.split()]
        assert se == min(32, R.bits_needed(n) + 1) and we == 32 + min(32, R.bits_needed(w) + 1), (w, n)


@pytest.mark.parametrize("k,a", [(5, 20), (6, 20), (7, 20), (8, 4), (8, 16)])
def test_word_numbers_beyond_the_bitmap_cap(drivers, k, a):
    """Word numbers of up to 32 bits: random sequences with codes beyond A mixed in, the largest word of all (every code A - 1, which
    at (8, 16) is 2^32 - 1), and what a key gives back."""
    rng = random.Random(1000 * k + a)
    seqs = [[rng.choice(list(range(a)) * 8 + [a, a + 1, 98, 255]) for _ in range(rng.randrange(0, 60))] for _ in range(120)]
    seqs += [[a - 1] * (k + 3), [a - 1] * k, [0] * k, [a - 1] * (k - 1)]
    ids = [rng.choice([0, 1, 77, 2 ** 31, 2 ** 32 - 2]) for _ in seqs]
    out = run(drivers, "words", ["%d %d %d %d %s" % (k, a, i, len(s), " ".join(map(str, s))) for s, i in zip(seqs, ids)])
    assert len(out) == len(seqs)
    top = 0
    for s, i, line in zip(seqs, ids, out):
        tok = line.split()
        windows = max(len(s) - k + 1, 0)
        assert int(tok[0]) == windows and len(tok) == 1 + 2 * windows
        got = set()
        for j in range(windows):
            w = R.word(s[j:j + k], a)
            if w is None:
                assert tok[1 + 2 * j:3 + 2 * j] == ["-", "-"], (s, j)
            else:
                assert [int(x) for x in tok[1 + 2 * j:3 + 2 * j]] == [w, w << 32 | i], (s, j)
                assert 0 <= w < a ** k <= 2 ** 32
                got.add(w)
        assert got == R.words(s, k, a)
        top = max([top] + list(got))
    assert top == a ** k - 1 > 2 ** 15


def test_chunk_cutting(drivers):
    rng = random.Random(7)
    cases = [(10, [10]), (10, [11]), (10, [0, 0, 0]), (10, [0, 10, 0, 0, 10, 1]), (10, [3, 3, 3, 3, 3]), (10, [5, 5, 5, 6, 4, 0, 0, 11, 1]),
             (10, [0, 0, 11]), (1, [1, 1, 0, 1]), (2 ** 26, [2 ** 26, 1, 2 ** 26 - 1, 1]), (2 ** 26, [2 ** 40]), (5, [])]
    cases += [(rng.randrange(20, 41), [rng.choice([0, 0, 1, 2, 5, 9, 20] * 8 + [39, 40]) for _ in range(rng.randrange(1, 30))]) for _ in range(200)]
    out = run(drivers, "cut", ["%d %d %s" % (cap, len(occ), " ".join(map(str, occ))) for cap, occ in cases])
    assert len(out) == len(cases)
    seen_over = seen_equal = seen_empty = 0
    for (cap, occ), line in zip(cases, out):
        tok = line.split()
        want = R.cut(occ, cap)
        if want is None:
            assert "over" in tok and occ[int(tok[tok.index("over") + 1])] > cap and tok.index("over") == len(tok) - 2
            assert all(v <= cap for v in occ[:int(tok[-1])])
            seen_over += 1
            continue
        got = list(zip([int(x) for x in tok[0::2]], [int(x) for x in tok[1::2]]))
        assert got == want, (cap, occ)
        # whole rows, in order, every row once; within the cap; no chunk could take the next row as well
        assert [r for f, n in got for r in range(f, f + n)] == list(range(len(occ)))
        for f, n in got:
            assert n >= 1 and sum(occ[f:f + n]) <= cap
            assert f + n == len(occ) or sum(occ[f:f + n + 1]) > cap
        seen_equal += any(sum(occ[f:f + n]) == cap for f, n in got)
        seen_empty += any(v == 0 for v in occ)
    assert seen_over > 10 and seen_equal > 10 and seen_empty > 10


# ---------------------------------------------------------------- what the word join and the seed join share
def test_the_shared_cap_at_max_k_8_and_16(drivers):
    cases = [(k, a, max_k) for max_k in (8, 16) for k in range(0, 19) for a in (0, 1, 2, 3, 4, 5, 16, 17, 20, 256, 257, 65536, 65537, 2 ** 32 - 1)]
    out = run(drivers, "pwords", ["%d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for (k, a, max_k), line in zip(cases, out):
        want = a ** k if 1 <= k <= max_k and a >= 1 and a ** k <= 2 ** 32 else 0
        assert int(line) == want, (k, a, max_k)
    assert (9, 4, 8) in cases and (9, 4, 16) in cases and (16, 4, 16) in cases and (17, 1, 16) in cases      # k between and beyond the two caps


def test_lower_and_upper_bound(drivers):
    import bisect
    top = 2 ** 64 - 1
    cases = [(5, []), (0, []), (top, []),                                        # n = 0
             (4, [5]), (5, [5]), (6, [5]), (top, [5]), (top, [top]), (0, [0]),   # one element
             (7, [7] * 9), (6, [7] * 9), (8, [7] * 9), (top, [top] * 3),         # all equal
             (0, [1, 3, 3, 9]), (10, [1, 3, 3, 9]), (top, [1, 3, 3, 9]),         # below the first, above the last
             (9, [1, 3, 9, 9, 9]), (3, [1, 3, 3]), (top, [1, top, top]),         # a run that ends at n
             (2 ** 32, [1, 2 ** 32 - 1]), (2 ** 32 - 1, [1, 2 ** 32 - 1]), (2 ** 40, [2 ** 40 - 1, 2 ** 40, 2 ** 40, 2 ** 63, top])]
    rng = random.Random(64)
    for _ in range(200):
        span = rng.choice([4, 50, 2 ** 32, 2 ** 64])
        a = sorted(rng.randrange(span) for _ in range(rng.randrange(0, 70)))
        cases.append((rng.choice(a + [rng.randrange(span)]), a))
    out = run(drivers, "bounds", ["%d %d %s" % (x, len(a), " ".join(map(str, a))) for x, a in cases])
    assert len(out) == len(cases)
    for (x, a), line in zip(cases, out):
        got = [int(v) for v in line.split()]
        want = [bisect.bisect_left(a, x), bisect.bisect_right(a, x)]
        assert got == want * (2 if all(v < 2 ** 32 for v in a) else 1), (x, a)


def test_the_sets_counter_words_do_not_overlap(drivers):
    out = run(drivers, "misc", [])
    ranges = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in out[:3]}
    total = int(out[3].split()[1])
    assert ranges == {"compact": (16, 1), "word": (20, 3), "seed": (24, 5)} and total == 64
    used = [w for first, n in list(ranges.values()) + [(0, 4), (8, 2)] for w in range(first, first + n)]      # (the passes' and the k best's words)
    assert len(used) == len(set(used)) and max(used) < total
    offsets = [int(v) for v in out[4].split()[1:]]
    assert offsets == [0, 1, 2, 3, 4] and max(offsets) < ranges["seed"][1] and max(offsets[:3]) < ranges["word"][1]


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_wordjoin_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_wordjoin.h")) == sorted(_ffi.WORDJOIN_EXPORTS)
    assert _ffi.WORDJOIN_EXPORTS == ["aln_seqset_word_index", "aln_seqset_word_join"]
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61 and len(_ffi.PREFILTER_EXPORTS) == 5      # as they were
    others = [getattr(_ffi, name) for name in dir(_ffi) if name.endswith("EXPORTS") and name != "WORDJOIN_EXPORTS"]
    assert len(others) >= 7
    for lst in others:
        assert not set(_ffi.WORDJOIN_EXPORTS) & set(lst)
    assert "aln_wordjoin.hip" in native_build.SOURCES and "aln_wordjoin_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_wordjoin.h") for h in native_build.HEADERS)
    text = strip_comments(open(os.path.join(ROOT, "include", "aligner_hip_wordjoin.h")).read())
    assert '#include "aligner_hip_prefilter.h"' in text


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.WORDJOIN_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_wordjoin.c")).read())
    for sym in _ffi.WORDJOIN_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layout_matches(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_wordjoin.h"\nint main(void) { return (int)sizeof(aln_wordjoin_spec) - 32; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_wordjoin_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_wordjoin_spec"]
    l, cls = lines[0], _ffi.WordjoinSpec
    assert int(l[2]) == C.sizeof(cls) == 32
    fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
    assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert [f[0] for f in fields] == ["k", "alphabet", "min_shared", "min_per_1024", "chunk_occurrences", "flags", "reserved"]
    assert (_ffi.WORDJOIN_MAX_K, _ffi.WORDJOIN_MAX_WORDS) == (R.MAX_K, R.MAX_WORDS)
    assert (_ffi.WORDJOIN_CHUNK_OCCURRENCES, _ffi.WORDJOIN_MAX_CHUNK_OCCURRENCES) == (R.CHUNK_OCCURRENCES, R.MAX_CHUNK_OCCURRENCES)


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    words = (C.c_uint32 * 4)(7, 7, 7, 7)
    count = C.c_uint64(99)
    spec = _ffi.WordjoinSpec(5, 20, 1, 0, 0, 0, 0)
    blk = _ffi.SeqsetBlock(0, 2, 0, 2, 1, 0)

    def untouched():
        return list(words) == [7] * 4 and count.value == 99

    assert lib.aln_seqset_word_index(None, 5, 20, words) == INV and untouched()
    assert lib.aln_seqset_word_index(None, 5, 20, None) == INV and untouched()
    assert lib.aln_seqset_word_join(None, C.byref(spec), C.byref(blk), C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_word_join(None, None, C.byref(blk), C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_word_join(None, C.byref(spec), None, None) == INV and untouched()
    assert b"null" in lib.aln_last_error()


# ---------------------------------------------------------------- the command's new argument errors
@pytest.mark.parametrize("extra,message", [
    (["--word-join"], "error: --word-join is a route of the prefilter: give --kmer K"),           # the route without the prefilter
    (["--kmer", "8", "--word-join"], "error: --kmer with --word-join: K must lie in 1 .. 8 and A^K may not exceed 2^32"),      # 20^8 > 2^32
    (["--kmer", "9", "--kmer-alphabet", "4", "--word-join"], "error: --kmer with --word-join: K must lie in 1 .. 8 and A^K may not exceed 2^32"),
    (["--kmer", "5", "--word-join", "--min-shared", "0"], "error: --min-shared with --word-join: N must be at least 1"),
    (["--kmer", "5", "--word-join", "--best", "2"], "error: --kmer with --best: --best aligns every pair"),
    (["--kmer", "5", "--word-join", "--heuristic", "--kd", "1", "--r-squared", "0.5"], "error: --kmer with --heuristic: the matrix loop"),
    (["--kmer", "5", "--word-join", "--min-shared-per-1024", "1025"], "error: --min-shared-per-1024: P must lie in 0 .. 1024"),
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
