"""The shuffled copies of aln_shuffle_* (aln_shuffle_rules.h; no GPU): the header compiled into a driver with the host compiler
against the independent restatement in shuffle_ref.py -- trims and permutations for many (seed, pair, copy, L, max_trim), raw
bounded draws where rejection is frequent -- plus properties of the copies (permutations of the trimmed prefix; fixed-seed chi-square
tests of the 24 orders of L = 4 and of the 7 trims), and the C layout of aln_shuffle_spec against the ctypes struct."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shuffle_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "aln_shuffle_rules.h"
int main(int argc, char **argv)
{
    // copy <cases>: lines "seed pair s max_trim L r_0 .. r_L-1" -> "trim c_0 .. c_L'-1"
    // bounded <seed> <pair> <s> <n> <count>: count draws of bounded(n) on the stream of (seed, pair, s)
    // count4 <seed> <copies> <max_trim>: copies of [0 1 2 3] on (seed, 0, s): per line "trim perm" where perm = the four codes
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "copy")) {
        FILE *f = fopen(argv[2], "r");
        if (!f) return 3;
        unsigned long long seed, pair, s;
        unsigned mt, L;
        while (fscanf(f, "%llu %llu %llu %u %u", &seed, &pair, &s, &mt, &L) == 5) {
            std::vector<unsigned char> a(L);
            for (unsigned j = 0; j < L; ++j) { unsigned v; if (fscanf(f, "%u", &v) != 1) return 4; a[j] = (unsigned char)v; }
            uint64_t st = aln_shuffle_state(seed, pair, s);
            const uint32_t trim = aln_shuffle_trim(st, mt);
            if (trim != aln_shuffle_trim_of(seed, pair, s, mt)) return 5;
            const uint32_t len = L - trim;
            aln_shuffle_permute(st, a.data(), len);
            printf("%u", trim);
            for (uint32_t j = 0; j < len; ++j) printf(" %u", a[j]);
            printf("\n");
        }
        fclose(f);
        return 0;
    }
    if (!strcmp(argv[1], "bounded")) {
        uint64_t st = aln_shuffle_state(strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10));
        const uint32_t n = (uint32_t)strtoull(argv[5], 0, 10);
        const unsigned count = (unsigned)strtoul(argv[6], 0, 10);
        for (unsigned i = 0; i < count; ++i) printf("%u\n", aln_shuffle_bounded(st, n));
        return 0;
    }
    if (!strcmp(argv[1], "count4")) {
        const uint64_t seed = strtoull(argv[2], 0, 10);
        const unsigned copies = (unsigned)strtoul(argv[3], 0, 10), mt = (unsigned)strtoul(argv[4], 0, 10);
        for (unsigned s = 0; s < copies; ++s) {
            uint64_t st = aln_shuffle_state(seed, 0, s);
            const uint32_t trim = aln_shuffle_trim(st, mt);
            unsigned char a[4] = {0, 1, 2, 3};
            aln_shuffle_permute(st, a, 4);
            printf("%u %u%u%u%u\n", trim, a[0], a[1], a[2], a[3]);
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
    printf("%u %u %u %u %u\n", (unsigned)sizeof(aln_shuffle_spec), (unsigned)offsetof(aln_shuffle_spec, seed),
           (unsigned)offsetof(aln_shuffle_spec, pair_base), (unsigned)offsetof(aln_shuffle_spec, per_pair),
           (unsigned)offsetof(aln_shuffle_spec, max_trim));
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
        pytest.fail("no C++ compiler (%s) to build the shuffle-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("shuffle_rules")
    return _compile(tmp, "drv.cpp", DRIVER, [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                                              os.path.join(ROOT, "aligner_amd", "csrc")])


def _run(drv, *args):
    return subprocess.run([drv] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout


def _cases():
    rng = np.random.default_rng(20261016)
    out = []
    seeds = [0, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, int(rng.integers(0, 2 ** 63))]
    for seed in seeds:
        for L, mt in [(0, 0), (1, 0), (1, 1), (6, 6), (7, 6), (2, 0), (3, 2), (30, 6), (350, 6), (257, 100), (64, 63)]:
            for pair, s in [(0, 0), (1, 0), (0, 4998), (12345, 17), (2 ** 40 + 3, 2 ** 20 - 1)]:
                t = rng.integers(0, 24, L).astype(np.uint8)
                out.append((seed, pair, s, mt, t))
    return out


def test_copies_equal_restatement(driver, tmp_path):
    cases = _cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as fh:
        for seed, pair, s, mt, t in cases:
            fh.write("%d %d %d %d %d %s\n" % (seed, pair, s, mt, len(t), " ".join(str(int(v)) for v in t)))
    lines = _run(driver, "copy", path).splitlines()
    assert len(lines) == len(cases)
    lengths_seen = set()
    for (seed, pair, s, mt, t), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        trim, copy = shuffle_ref.copy_of(t, seed, pair, s, mt)
        assert got[0] == trim and 0 <= trim <= mt, (seed, pair, s, mt, len(t))
        assert got[1:] == copy.tolist(), (seed, pair, s, mt, len(t))
        # a permutation of the trimmed prefix
        assert sorted(got[1:]) == sorted(t[:len(t) - trim].tolist())
        lengths_seen.add(len(t) - trim)
    assert {0, 1} <= lengths_seen          # empty and one-residue copies occur


@pytest.mark.parametrize("n", [3 * 2 ** 30, 2 ** 32 - 1, 2 ** 31 + 1, 7, 1])
def test_bounded_draws_equal_restatement(driver, n):
    """n = 3 * 2^30 rejects a quarter of the first draws' low words below 2^30; n = 2^32 - 1 rejects rarely but at the far end."""
    count = 2000
    got = [int(v) for v in _run(driver, "bounded", 99, 5, 3, n, count).split()]
    r = shuffle_ref.Stream(99, 5, 3)
    want = [r.bounded(n) for _ in range(count)]
    assert got == want
    assert all(0 <= v < n for v in got)


def _chi2(counts, expected):
    counts = np.asarray(counts, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


def test_chi_square_orders_and_trims(driver):
    """Fixed seeds, so deterministic: 24 000 copies of [0 1 2 3] with max_trim 6 for each of seeds 1..8.  Per seed, the trims over
    0..6 and the orders of the copies whose trim is 0 over the 24 permutations stay below the chi-square critical values at
    p = 0.001 (22.46 for 6 degrees of freedom, 49.73 for 23); over all seeds the sums stay below those of 48 and 184 degrees of
    freedom (84.04, 251.6)."""
    tot_trims = tot_orders = 0.0
    for seed in range(1, 9):
        lines = _run(driver, "count4", seed, 24000, 6).split("\n")
        trims = np.zeros(7, dtype=np.int64)
        orders = {"".join(map(str, p)): 0 for p in itertools.permutations(range(4))}
        for line in lines:
            if not line:
                continue
            tr, perm = line.split()
            trims[int(tr)] += 1
            if int(tr) == 0:
                orders[perm] += 1
        assert trims.sum() == 24000
        c_trims = _chi2(trims, 24000 / 7)
        n0 = sum(orders.values())
        assert n0 == trims[0]
        c_orders = _chi2(list(orders.values()), n0 / 24)
        assert c_trims < 22.46 and c_orders < 49.73, (seed, trims, orders)
        tot_trims += c_trims
        tot_orders += c_orders
        # the first draws are the restatement's trims
        assert shuffle_ref.trims(seed, 0, 50, 6).tolist() == [int(l.split()[0]) for l in lines[:50]]
    assert tot_trims < 84.04 and tot_orders < 251.6, (tot_trims, tot_orders)


def test_package_trims_equal_restatement():
    """statistics._trims (the lengths shuffle_targets reports) against the scalar restatement, including rejection-prone bounds."""
    from aligner_amd import statistics
    for seed, pair, mt in [(0, 0, 6), (7, 2 ** 40, 6), (0xFFFFFFFFFFFFFFFF, 3, 0), (5, 1, 3 * 2 ** 30 - 1), (11, 9, 2 ** 32 - 2)]:
        assert statistics._trims(seed, pair, 300, mt).tolist() == shuffle_ref.trims(seed, pair, 300, mt).tolist()


def test_spec_layout_c99_equals_ctypes(tmp_path):
    cc = os.environ.get("CC", "gcc")
    if shutil.which(cc) is None:
        pytest.fail("no C compiler (%s)" % cc)
    exe = _compile(tmp_path, "abi.c", ABI, [cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")])
    size, *offs = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    from aligner_amd import _ffi
    S = _ffi.ShuffleSpec
    assert size == 24 == __import__("ctypes").sizeof(S)
    assert offs == [S.seed.offset, S.pair_base.offset, S.per_pair.offset, S.max_trim.offset] == [0, 8, 16, 20]
    assert {"aln_shuffle_scores", "aln_shuffle_targets"} <= set(_ffi.EXPORTS)
