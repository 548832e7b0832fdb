"""The k-mer prefilter without a GPU: aligner_amd/csrc/aln_prefilter_rules.h driven through a small C++ program and compared with
prefilter_ref.py (word numbers, rejected windows, the bitmap's element and bit, the candidate predicate and its edges, the closed-form
rank against aln_seqset_unrank); the companion header include/aligner_hip_prefilter.h against its mirrors (_ffi.PREFILTER_EXPORTS,
the ctypes class, tests/abi_prefilter.c); the refusals that need no device; the argument errors of the command."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prefilter_ref as R  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_prefilter_rules.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "bits")) {           // lines `k A` -> bits elements stride
        uint32_t k, a;
        while (scanf("%" SCNu32 " %" SCNu32, &k, &a) == 2) {
            const uint32_t b = aln_prefilter_bits(k, a);
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", b, aln_prefilter_elements(b), aln_prefilter_stride(b));
        }
        return 0;
    }
    if (!strcmp(argv[1], "words")) {          // lines `k A n c0 .. c(n-1)` -> windows, then per window `word element bit` or `- - -`
        uint32_t k, a, n;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &k, &a, &n) == 3) {
            std::vector<uint8_t> s(n + 1);
            for (uint32_t i = 0; i < n; ++i) { unsigned c; if (scanf("%u", &c) != 1) return 2; s[i] = (uint8_t)c; }
            const uint64_t windows = aln_prefilter_windows(n, k);
            printf("%" PRIu64, windows);
            for (uint64_t i = 0; i < windows; ++i) {
                uint32_t w;
                if (aln_prefilter_word(s.data() + i, k, a, &w)) printf(" %" PRIu32 " %" PRIu32 " %" PRIu32, w, aln_prefilter_element(w), aln_prefilter_bit(w));
                else printf(" - - -");
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "cand")) {           // lines `shared n_q n_t min_shared min_per_1024` -> 0 / 1
        uint32_t sh, nq, nt, ms, mp;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &sh, &nq, &nt, &ms, &mp) == 5)
            printf("%d\n", (int)aln_prefilter_candidate(sh, nq, nt, ms, mp));
        return 0;
    }
    if (!strcmp(argv[1], "rank")) {           // lines `n_seqs q_first q_count t_first t_count upper` -> pairs, mismatches, then q t per pair
        uint64_t ns, qf, qc, tf, tc, up;
        while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &ns, &qf, &qc, &tf, &tc, &up) == 6) {
            aln_seqset_block b;
            b.q_first = qf; b.q_count = qc; b.t_first = tf; b.t_count = tc; b.upper = (uint32_t)up; b.reserved = 0;
            const uint64_t pairs = aln_seqset_block_pairs(ns, b);
            uint64_t bad = 0;
            std::vector<uint64_t> qs, ts;
            for (uint64_t k = 0; k < pairs; ++k) {
                uint64_t q, t;
                aln_seqset_unrank(b, k, &q, &t);
                if (aln_prefilter_rank(b, q, t) != k) ++bad;
                qs.push_back(q); ts.push_back(t);
            }
            printf("%" PRIu64 " %" PRIu64, pairs, bad);
            for (uint64_t k = 0; k < pairs; ++k) printf(" %" PRIu64 " %" PRIu64, qs[k], ts[k]);
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
    tmp = tmp_path_factory.mktemp("prefilter_rules")
    src = os.path.join(str(tmp), "drv.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(str(tmp), "drv")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", exe])
    return exe


def run(drv, what, lines):
    return subprocess.run([drv, what], check=True, capture_output=True, text=True, input="\n".join(lines) + "\n").stdout.splitlines()


# ---------------------------------------------------------------- the rules header against the reference
def test_parameter_limits(driver):
    cases = [(k, a) for k in range(0, 11) for a in (0, 1, 2, 3, 4, 5, 8, 20, 21, 22, 23, 64, 65, 512, 513, 2 ** 18, 2 ** 18 + 1, 2 ** 32 - 1)]
    out = run(driver, "bits", ["%d %d" % c for c in cases])
    for (k, a), line in zip(cases, out):
        b, e, s = [int(x) for x in line.split()]
        assert b == R.bits(k, a), (k, a)
        assert e == (b + 31) // 32 and s == (e + 3) // 4 * 4
    assert R.bits(4, 20) == 160000 and R.bits(5, 20) == 0 and R.bits(8, 4) == 65536 and R.bits(9, 4) == 0 and R.bits(1, 2 ** 18) == 2 ** 18


@pytest.mark.parametrize("k,a", list(itertools.product((1, 2, 3), (2, 4, 5))))
def test_words_windows_and_bitmap(driver, k, a):
    """Every (k, A): every sequence of up to k + 2 codes over 0 .. A (A itself being the code outside), and random longer ones with
    codes up to 255: the windows' numbers, which windows are no words, and where each word's bit lives."""
    rng = random.Random(100 * k + a)
    seqs = [list(s) for n in range(0, k + 3) for s in itertools.product(range(a + 1), repeat=n)] if (a + 1) ** (k + 2) <= 8000 else []
    seqs += [[rng.choice(list(range(a)) * 6 + [a, a + 1, 98, 255]) for _ in range(rng.randrange(0, 40))] for _ in range(200)]
    out = run(driver, "words", ["%d %d %d %s" % (k, a, len(s), " ".join(map(str, s))) for s in seqs])
    assert len(out) == len(seqs)
    for s, line in zip(seqs, out):
        tok = line.split()
        windows = max(len(s) - k + 1, 0)
        assert int(tok[0]) == windows and len(tok) == 1 + 3 * windows
        got = set()
        for i in range(windows):
            w = R.word(s[i:i + k], a)
            if w is None:
                assert tok[1 + 3 * i:4 + 3 * i] == ["-", "-", "-"], (s, i)
            else:
                assert [int(x) for x in tok[1 + 3 * i:4 + 3 * i]] == [w, w >> 5, w & 31], (s, i)
                assert 0 <= w < a ** k
                got.add(w)
        assert got == R.words(s, k, a)
        bm = R.bitmap(got, k, a)
        assert sum(bin(e).count("1") for e in bm) == len(got) and len(bm) == (a ** k + 31) // 32
        assert a ** k % 32 == 0 or bm[-1] >> (a ** k % 32) == 0                                          # tail bits are zero


def test_the_candidate_predicate_and_its_edges(driver):
    cases = []
    for nq, nt in itertools.product((0, 1, 2, 3, 7, 100, 1000, 2 ** 18), repeat=2):
        m = min(nq, nt)
        for per in (0, 1, 128, 256, 511, 512, 1023, 1024):
            # the smallest shared that meets the share threshold, and its neighbours: shared * 1024 == per * min(n) where that divides
            edge = (per * m + 1023) // 1024
            for sh in {0, 1, m, max(edge - 1, 0), edge, edge + 1}:
                for ms in (0, 1, sh, sh + 1):
                    cases.append((sh, nq, nt, ms, per))
    cases += [(2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 1024), (2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32 - 1, 0, 1024),
              (2 ** 22, 2 ** 32 - 1, 2 ** 32 - 1, 0, 1)]                                    # products beyond 32 bits
    out = run(driver, "cand", ["%d %d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for c, line in zip(cases, out):
        assert bool(int(line)) == R.candidate(*c), c
    exact = [c for c in cases if c[0] * 1024 == c[4] * min(c[1], c[2]) and c[4] and min(c[1], c[2])]
    assert len(exact) > 50 and all(R.candidate(*c) == (c[0] >= c[3]) for c in exact)          # equality passes
    assert R.candidate(0, 0, 5, 0, 1024) and not R.candidate(0, 0, 5, 1, 0)                  # min(n) == 0: only min_shared decides
    assert all(R.candidate(sh, nq, nt, 0, 0) for sh, nq, nt, _, _ in cases)                   # thresholds 0: every pair


def test_rank_is_the_inverse_of_unrank(driver):
    """Every pair of every block with n <= 40: the upper triangles of every n, and rectangles whose ranges start off zero."""
    blocks = [(n + 3, 3, n, 3, n, 1) for n in range(2, 41)] + [(n, 0, n, 0, n, 1) for n in (2, 3, 40)]
    blocks += [(90, qf, qc, tf, tc, 0) for qf, qc, tf, tc in ((0, 1, 0, 1), (5, 1, 7, 40), (5, 40, 7, 1), (2, 17, 30, 23), (0, 40, 0, 40),
                                                              (11, 40, 50, 40))]
    out = run(driver, "rank", ["%d %d %d %d %d %d" % b for b in blocks])
    for (ns, qf, qc, tf, tc, up), line in zip(blocks, out):
        tok = [int(x) for x in line.split()]
        want = R.block_pairs((qf, qc, tf, tc, up))
        assert tok[0] == len(want) > 0 and tok[1] == 0
        assert list(zip(tok[2::2], tok[3::2])) == want


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_prefilter_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_prefilter.h")) == sorted(_ffi.PREFILTER_EXPORTS)
    assert len(_ffi.PREFILTER_EXPORTS) == 5
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61         # the main header is as it was
    assert not set(_ffi.PREFILTER_EXPORTS) & set(_ffi.EXPORTS) and not set(_ffi.PREFILTER_EXPORTS) & set(_ffi.CLUSTER_EXPORTS)
    assert "aln_prefilter.hip" in native_build.SOURCES and "aln_prefilter_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_prefilter.h") for h in native_build.HEADERS)


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.PREFILTER_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_prefilter.c")).read())
    for sym in _ffi.PREFILTER_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layout_matches(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_prefilter.h"\nint main(void) { return (int)sizeof(aln_prefilter_spec) - 32; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_prefilter_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_prefilter_spec"]
    l, cls = lines[0], _ffi.PrefilterSpec
    assert int(l[2]) == C.sizeof(cls) == 32
    fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
    assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert [f[0] for f in fields] == ["k", "alphabet", "min_shared", "min_per_1024", "chunk_pairs", "flags", "reserved"]
    assert (_ffi.PREFILTER_MAX_K, _ffi.PREFILTER_MAX_BITS, _ffi.PREFILTER_CHUNK_PAIRS) == (R.MAX_K, R.MAX_BITS, 1 << 22)


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    words = (C.c_uint32 * 4)(7, 7, 7, 7)
    count = C.c_uint64(99)
    idx = (C.c_uint64 * 2)(5, 5)
    a, b, c = (C.c_uint32 * 2)(5, 5), (C.c_uint32 * 2)(5, 5), (C.c_uint32 * 2)(5, 5)
    f = (C.c_double * 2)(1.5, 1.5)
    spec = _ffi.PrefilterSpec(2, 4, 0, 0, 0, 0, 0)
    blk = _ffi.SeqsetBlock(0, 2, 0, 2, 1, 0)
    p = _ffi.Params()

    def untouched():
        return list(words) == [7] * 4 and count.value == 99 and list(idx) == [5, 5] and list(a) + list(b) + list(c) == [5] * 6 and list(f) == [1.5, 1.5]

    # a null set
    assert lib.aln_seqset_kmer_index(None, 2, 4, words) == INV and untouched()
    assert lib.aln_seqset_prefilter(None, C.byref(spec), C.byref(blk), C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_candidates(None, 0, 2, idx, a, b, c) == INV and untouched()
    assert lib.aln_seqset_candidate_scores(None, C.byref(p), f, None) == INV and untouched()
    assert lib.aln_seqset_candidate_hits(None, C.byref(p), 0.0, C.byref(count)) == INV and untouched()
    # a null set and a null spec
    assert lib.aln_seqset_prefilter(None, None, C.byref(blk), C.byref(count)) == INV and untouched()
    assert b"null" in lib.aln_last_error()


# ---------------------------------------------------------------- the command's argument errors
@pytest.mark.parametrize("extra", [
    ["--min-shared", "3"], ["--min-shared-per-1024", "100"], ["--kmer-alphabet", "20"],           # thresholds without --kmer
    ["--kmer", "3", "--best", "2"], ["--kmer", "3", "--heuristic", "--kd", "1", "--r-squared", "0.5"],
    ["--kmer", "0"], ["--kmer", "9"], ["--kmer", "5"], ["--kmer", "3", "--kmer-alphabet", "0"], ["--kmer", "2", "--kmer-alphabet", "513"],
    ["--kmer", "3", "--min-shared-per-1024", "1025"], ["--kmer", "3", "--min-shared", "-1"],
])
def test_the_commands_argument_errors(tmp_path, capsys, extra):
    from aligner_amd import allpairs
    fa = tmp_path / "x.fasta"
    fa.write_text(">a\nACDEFGHIK\n>b\nACDEFGHIK\n")
    with pytest.raises(SystemExit) as e:
        allpairs.main(["-i", str(fa)] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--kmer" in err or "--min-shared" in err
