"""Seed chains without a GPU: aligner_amd/csrc/aln_seedchain_rules.h driven through a small C++ program and compared with
seedchain_ref.py (hand-made anchor sets fed in several orders of their equal-pq anchors, every tie of the rule, v at k and k + 1, gaps
and skews at their limits, gap_scale 0 and 255, the drift at the ends of what 2^31 - 1 positions give, f at k * 2^20, the spec's
ranges, the filter), the same program once more built as a stand-alone program with the address and undefined-behaviour sanitizers; the
reference's fast path against its plain one; the companion header include/aligner_hip_seedchain.h against its mirrors
(_ffi.SEEDCHAIN_EXPORTS, the ctypes classes, tests/abi_seedchain.c) and compiled as C99; the refusals that need no device; the command's
new argument errors."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedchain_ref as R  # noqa: E402
from aligner_amd import _ffi  # noqa: E402
from aligner_amd import build as native_build  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2 ** 31 - 1

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aln_seedchain_rules.h"
static void print(const aln_chain_record &r)
{
    printf("%" PRId32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", r.score, r.anchors, r.q_start, r.q_end,
           r.t_start, r.t_end, r.seeds, r.flags);
}
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    aln_seedchain_spec sp;
    memset(&sp, 0, sizeof sp);
    if (!strcmp(argv[1], "chain")) {          // lines `k G B g max_pair_seeds n pq0 pt0 ..`, ascending in pq -> the record
        uint64_t n;
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64, &sp.k, &sp.max_gap, &sp.max_skew, &sp.gap_scale,
                     &sp.max_pair_seeds, &n) == 6) {
            std::vector<uint64_t> anchors(n);
            std::vector<aln_seedchain_state> state(n);
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t pq, pt;
                if (scanf("%" SCNu32 " %" SCNu32, &pq, &pt) != 2) return 2;
                anchors[i] = aln_seedchain_anchor(pq, pt);
                if (aln_seedchain_pq(anchors[i]) != pq || aln_seedchain_pt(anchors[i]) != pt) return 3;
            }
            print(aln_seedchain_pair(anchors.data(), n, sp, state.data()));
        }
        return 0;
    }
    if (!strcmp(argv[1], "ladder")) {         // lines `k n`: n anchors k apart on one diagonal from (5, 9) -> the record
        uint64_t n;
        while (scanf("%" SCNu32 " %" SCNu64, &sp.k, &n) == 2) {
            sp.max_gap = sp.k; sp.max_skew = 0; sp.gap_scale = 255; sp.max_pair_seeds = (uint32_t)n;
            std::vector<uint64_t> anchors(n);
            std::vector<aln_seedchain_state> state(n);
            for (uint64_t i = 0; i < n; ++i) anchors[i] = aln_seedchain_anchor((uint32_t)(5u + i * sp.k), (uint32_t)(9u + i * sp.k));
            print(aln_seedchain_pair(anchors.data(), n, sp, state.data()));
        }
        return 0;
    }
    if (!strcmp(argv[1], "none")) {           // lines `A max_pair_seeds` -> what chains, and the record of a pair that is not chained
        uint64_t a;
        uint32_t cap;
        while (scanf("%" SCNu64 " %" SCNu32, &a, &cap) == 2) {
            printf("%" PRIu64 " ", aln_seedchain_chained(a, cap));
            print(aln_seedchain_record_none(a, cap));
        }
        return 0;
    }
    if (!strcmp(argv[1], "spec")) {           // lines `G B g max_pair_seeds chunk_anchors flags r0 r1 r2` -> the refusal, 0 for none
        while (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &sp.max_gap, &sp.max_skew,
                     &sp.gap_scale, &sp.max_pair_seeds, &sp.chunk_anchors, &sp.flags, &sp.reserved[0], &sp.reserved[1], &sp.reserved[2]) == 9)
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", aln_seedchain_spec_refusal(sp), aln_seedchain_pair_seeds(sp), aln_seedchain_chunk_anchors(sp));
        return 0;
    }
    if (!strcmp(argv[1], "keep")) {           // lines `score q_start q_end t_start t_end flags min_score min_span` -> 0 / 1
        aln_chain_record r;
        memset(&r, 0, sizeof r);
        int32_t min_score;
        uint32_t min_span;
        while (scanf("%" SCNd32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNd32 " %" SCNu32, &r.score, &r.q_start, &r.q_end, &r.t_start,
                     &r.t_end, &r.flags, &min_score, &min_span) == 8)
            printf("%d\n", aln_seedchain_keep(r, min_score, min_span) ? 1 : 0);
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
    tmp = tmp_path_factory.mktemp("seedchain_rules")
    return [compile_driver(tmp, "drv", []), compile_driver(tmp, "drv_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def run(drivers, what, lines):
    """Both programs on the same input: the sanitized one must end clean and print the same."""
    outs = []
    for drv in drivers:
        p = subprocess.run([drv, what], capture_output=True, text=True, input="\n".join(lines) + "\n", timeout=300)
        assert p.returncode == 0, (drv, p.returncode, p.stderr[-2000:])
        outs.append(p.stdout.splitlines())
    assert outs[0] == outs[1]
    return outs[0]


def orders(anchors, rng, most=6):
    """the anchors ascending in pq, in several orders of those that share a pq: ascending pt, descending pt, shuffled"""
    by_pq = {}
    for pq, pt in anchors:
        by_pq.setdefault(pq, []).append(pt)
    out = []
    for how in range(most):
        seq = []
        for pq in sorted(by_pq):
            pts = sorted(by_pq[pq], reverse=(how == 1))
            if how >= 2:
                rng.shuffle(pts)
            seq += [(pq, pt) for pt in pts]
        if seq not in out:
            out.append(seq)
    return out


def chain_lines(cases, rng):
    """(the driver's input lines, the case each line belongs to)"""
    lines, owner = [], []
    for c, (k, G, B, g, cap, anchors) in enumerate(cases):
        for seq in orders(anchors, rng):
            lines.append("%d %d %d %d %d %d %s" % (k, G, B, g, cap, len(seq), " ".join("%d %d" % x for x in seq)))
            owner.append(c)
    return lines, owner


def check_chains(drivers, cases, seed=1):
    lines, owner = chain_lines(cases, random.Random(seed))
    out = run(drivers, "chain", lines)
    assert len(out) == len(lines)
    want = [R.chain_plain(anchors, k, G, B, g, cap) for k, G, B, g, cap, anchors in cases]
    for line, c in zip(out, owner):
        assert tuple(int(x) for x in line.split()) == want[c], (cases[c], line)
    return want


# ---------------------------------------------------------------- the rules header against the reference
def test_ties_of_the_rule(drivers):
    k = 4
    cases = [
        # two predecessors of equal v at different pq: the greater pq wins, and with it its start
        (k, 100, 100, 0, 0, [(0, 0), (10, 10), (11, 1), (20, 20)]),
        (k, 100, 100, 0, 0, [(0, 50), (3, 3), (30, 60)]),
        # ... at equal pq with different pt: the greater pt wins
        (k, 100, 100, 0, 0, [(5, 1), (5, 2), (20, 20)]),
        (k, 100, 100, 0, 0, [(5, 7), (5, 2), (5, 4), (20, 20), (20, 30)]),
        # two end anchors of equal f: the least pq, then the least pt
        (k, 3, 0, 0, 0, [(0, 0), (50, 50)]),
        (k, 100, 0, 0, 0, [(0, 0), (4, 4), (50, 10), (54, 14)]),
        (k, 100, 0, 0, 0, [(7, 9), (7, 3), (7, 5)]),
        (k, 100, 0, 0, 0, [(0, 30), (4, 34), (0, 10), (4, 14)]),
    ]
    want = check_chains(drivers, cases)
    assert want[0] == (12, 3, 0, 24, 0, 24, 4, 0)          # by (10, 10): (0, 0) is its start; (11, 1) has the same v and no history
    assert want[2] == (8, 2, 5, 24, 2, 24, 3, 0)
    assert want[4] == (4, 1, 0, 4, 0, 4, 2, 0)
    assert want[5] == (8, 2, 0, 8, 0, 8, 4, 0)
    assert want[6] == (4, 1, 7, 11, 3, 7, 3, 0)
    assert want[7] == (8, 2, 0, 8, 10, 18, 4, 0)


def test_v_at_k_and_one_above(drivers):
    k = 5
    cases = [
        # gain 1, cost 1: v = k: no predecessor is taken; cost 0: v = k + 1: taken
        (k, 100, 100, 16, 0, [(0, 0), (1, 2)]),
        (k, 100, 100, 0, 0, [(0, 0), (1, 2)]),
        (k, 100, 100, 8, 0, [(0, 0), (1, 3)]),             # |dd| = 2 at half a point each: cost 1, v = k
        (k, 100, 100, 7, 0, [(0, 0), (1, 3)]),             # (2 * 7) >> 4 = 0: v = k + 1
        (k, 100, 100, 255, 0, [(0, 0), (9, 10)]),          # 255 >> 4 = 15 > gain: v < k
    ]
    want = check_chains(drivers, cases)
    assert [w[:2] for w in want] == [(5, 1), (6, 2), (5, 1), (6, 2), (5, 1)]
    assert want[0][2:6] == (0, 5, 0, 5) and want[1][2:6] == (0, 6, 0, 7)


def test_gaps_and_skews_at_their_limits(drivers):
    k, G, B = 3, 20, 6
    cases = [
        (k, G, 100, 0, 0, [(0, 0), (G, G)]), (k, G, 100, 0, 0, [(0, 0), (G + 1, G + 1)]),              # the gap on both records
        (k, G, 100, 0, 0, [(0, 0), (G, 5)]), (k, G, 100, 0, 0, [(0, 0), (G + 1, 5)]),                  # ... on the query alone
        (k, G, 100, 0, 0, [(0, 0), (5, G)]), (k, G, 100, 0, 0, [(0, 0), (5, G + 1)]),                  # ... on the target alone
        (k, 100, B, 0, 0, [(0, 0), (10, 10 + B)]), (k, 100, B, 0, 0, [(0, 0), (10, 10 + B + 1)]),      # the skew, target ahead
        (k, 100, B, 0, 0, [(0, 0), (10 + B, 10)]), (k, 100, B, 0, 0, [(0, 0), (10 + B + 1, 10)]),      # ... query ahead
        (k, 100, 0, 0, 0, [(0, 0), (10, 10)]), (k, 100, 0, 0, 0, [(0, 0), (10, 11)]),                  # B = 0
        (k, 100, 100, 0, 0, [(0, 0), (0, 5)]), (k, 100, 100, 0, 0, [(0, 0), (5, 0)]),                  # not before it on both records
        (k, 1, 0, 0, 0, [(0, 0), (1, 1), (2, 2), (4, 4)]),                                             # G = 1: overlapping words gain 1
        (k, 100, 100, 255, 0, [(0, 0), (50, 50), (60, 61), (70, 70)]),                                 # gap_scale 255: a drift of 1 costs 15
        (k, 100, 100, 0, 0, [(0, 0), (50, 50), (60, 61), (70, 70)]),                                   # gap_scale 0: drift is free
    ]
    want = check_chains(drivers, cases)
    assert [w[1] for w in want[:14]] == [2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1, 1, 1]
    assert want[14][:2] == (5, 3) and want[14][2:6] == (0, 5, 0, 5)
    assert want[15][:2] == (9, 3) and want[16][:2] == (12, 4)


def test_the_drift_at_the_ends_of_the_positions(drivers):
    k = 16
    cases = [
        (k, TOP, TOP, 255, 0, [(0, 0), (1, TOP)]),                 # dd = 2^31 - 2: cost far above int32
        (k, TOP, TOP, 255, 0, [(0, 0), (TOP, 1)]),                 # dd = -(2^31 - 2)
        (k, TOP, TOP, 0, 0, [(0, 0), (1, TOP)]), (k, TOP, TOP, 0, 0, [(0, 0), (TOP, 1)]),
        (k, TOP, TOP - 1, 0, 0, [(0, 0), (1, TOP)]), (k, TOP, TOP - 2, 0, 0, [(0, 0), (1, TOP)]),      # |dd| = B and B + 1
        (k, TOP, 0, 0, 0, [(0, 0), (TOP, TOP)]), (k, TOP - 1, 0, 0, 0, [(0, 0), (TOP, TOP)]),
        (k, TOP, TOP, 1, 0, [(TOP - 40, 0), (TOP, TOP)]),
    ]
    want = check_chains(drivers, cases)
    assert [w[1] for w in want] == [1, 1, 2, 2, 2, 1, 2, 1, 1]
    assert want[2] == (17, 2, 0, 1 + k, 0, TOP + k, 2, 0) and want[6] == (32, 2, 0, TOP + k, 0, TOP + k, 2, 0)


def test_random_anchor_sets_in_every_order(drivers):
    rng = random.Random(5)
    cases = []
    for _ in range(250):
        k = rng.choice([1, 3, 8, 15, 16])
        span = rng.choice([6, 20, 200])
        n = rng.randrange(1, 40)
        anchors = list({(rng.randrange(span), rng.randrange(span)) for _ in range(n)})
        if rng.random() < 0.4:                                     # a run on one diagonal among the noise
            d, at = rng.randrange(span), rng.randrange(span)
            anchors = list(set(anchors) | {(at + i * rng.choice([1, k]), at + d + i * k) for i in range(rng.randrange(2, 12))})
        cases.append((k, rng.choice([1, 3, 10, 50, 1000]), rng.choice([0, 1, 5, 200]), rng.choice([0, 1, 2, 16, 255]), rng.choice([0, 0, 0, 5, 20]), anchors))
    want = check_chains(drivers, cases, seed=9)
    assert sum(1 for w in want if w[7]) > 5 and sum(1 for w in want if w[1] > 2) > 50
    # the reference's fast path gives the plain one's records
    for k, G, B, g, cap, anchors in cases:
        assert R.chain(anchors, k, G, B, g, cap) == R.chain_plain(anchors, k, G, B, g, cap)
    for _ in range(12):
        anchors = {(rng.randrange(60), rng.randrange(60)) for _ in range(rng.randrange(65, 400))}
        args = (rng.choice([1, 4]), rng.choice([3, 8, 30]), rng.choice([0, 2, 50]), rng.choice([0, 2, 40]))
        assert R.chain(anchors, *args) == R.chain_plain(anchors, *args)


def test_f_at_k_times_two_to_the_twenty(drivers):
    out = run(drivers, "ladder", ["16 %d" % 2 ** 20, "16 1000", "1 %d" % 2 ** 20])
    got = [tuple(int(x) for x in line.split()) for line in out]
    n = 2 ** 20
    assert got[0] == (16 * n, n, 5, 5 + 16 * n, 9, 9 + 16 * n, n, 0) and 16 * n == _ffi.SEEDJOIN_MAX_K * _ffi.SEEDCHAIN_MAX_PAIR_SEEDS < 2 ** 31
    assert got[1] == R.chain([(5 + 16 * i, 9 + 16 * i) for i in range(1000)], 16, 16, 0, 255, 1000)
    assert got[2] == (n, n, 5, 5 + n, 9, 9 + n, n, 0)


def test_pairs_that_are_not_chained(drivers):
    cases = [(0, 0), (0, 7), (7, 7), (8, 7), (2 ** 16, 2 ** 16), (2 ** 16 + 1, 2 ** 16), (2 ** 20 + 1, 2 ** 20), (2 ** 32 - 1, 9), (2 ** 32, 9), (2 ** 40, 2 ** 20)]
    out = run(drivers, "none", ["%d %d" % c for c in cases])
    for (a, cap), line in zip(cases, out):
        tok = [int(x) for x in line.split()]
        assert tok[0] == (0 if a > cap else a)
        assert tuple(tok[1:]) == (R.none_record(a, cap) if (a == 0 or a > cap) else (0,) * 8), (a, cap)
    assert R.none_record(2 ** 40, 2 ** 20) == (0, 0, 0, 0, 0, 0, 2 ** 32 - 1, 1) and R.none_record(8, 7) == (0, 0, 0, 0, 0, 0, 8, 1)
    assert R.chain_plain([(i, i) for i in range(8)], 3, 10, 0, 0, 7) == (0, 0, 0, 0, 0, 0, 8, 1)


def test_the_specs_ranges(drivers):
    good = dict(max_gap=1000, max_skew=200, gap_scale=2, max_pair_seeds=0, chunk_anchors=0, flags=0, reserved=(0, 0, 0))
    edits = [{}, dict(max_gap=0), dict(max_gap=1), dict(max_gap=TOP), dict(max_gap=TOP + 1), dict(max_gap=2 ** 32 - 1), dict(max_skew=0), dict(max_skew=TOP),
             dict(max_skew=TOP + 1), dict(gap_scale=0), dict(gap_scale=255), dict(gap_scale=256), dict(max_pair_seeds=1), dict(max_pair_seeds=2 ** 20),
             dict(max_pair_seeds=2 ** 20 + 1), dict(chunk_anchors=1), dict(chunk_anchors=2 ** 26), dict(chunk_anchors=2 ** 26 + 1), dict(flags=1),
             dict(reserved=(1, 0, 0)), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 1)),
             # max_pair_seeds may not exceed chunk_anchors, each as given or as its default
             dict(chunk_anchors=2 ** 16), dict(chunk_anchors=2 ** 16 - 1), dict(max_pair_seeds=5, chunk_anchors=5), dict(max_pair_seeds=6, chunk_anchors=5),
             dict(max_pair_seeds=2 ** 20, chunk_anchors=2 ** 20 - 1), dict(max_pair_seeds=1, chunk_anchors=1)]
    specs = [dict(good, **e) for e in edits]
    out = run(drivers, "spec", ["%d %d %d %d %d %d %d %d %d" % ((s["max_gap"], s["max_skew"], s["gap_scale"], s["max_pair_seeds"], s["chunk_anchors"], s["flags"]) + s["reserved"])
                                for s in specs])
    refused = 0
    for s, line in zip(specs, out):
        why, pair_seeds, chunk = [int(x) for x in line.split()]
        assert (why == 0) == R.spec_ok(**s), s
        assert pair_seeds == (s["max_pair_seeds"] or R.PAIR_SEEDS) and chunk == (s["chunk_anchors"] or R.CHUNK_ANCHORS)
        refused += why != 0
    assert refused == 15
    assert (R.MAX_GAP, R.MAX_SKEW, R.MAX_GAP_SCALE) == (_ffi.SEEDCHAIN_MAX_GAP, _ffi.SEEDCHAIN_MAX_SKEW, _ffi.SEEDCHAIN_MAX_GAP_SCALE)
    assert (R.PAIR_SEEDS, R.MAX_PAIR_SEEDS, R.CHUNK_ANCHORS, R.MAX_CHUNK_ANCHORS) == (_ffi.SEEDCHAIN_PAIR_SEEDS, _ffi.SEEDCHAIN_MAX_PAIR_SEEDS,
                                                                                     _ffi.SEEDCHAIN_CHUNK_ANCHORS, _ffi.SEEDCHAIN_MAX_CHUNK_ANCHORS)
    assert R.OVERFLOW == _ffi.CHAIN_OVERFLOW == 1


def test_the_filter(drivers):
    cases = []
    for score, qs, qe, ts, te, flags in ((10, 0, 8, 5, 12, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1), (-5, 3, 4, 3, 4, 0), (2 ** 24, 0, TOP, 0, TOP + 16, 0)):
        for min_score, min_span in itertools.product((-(2 ** 31), -5, 0, 1, 10, 11, 2 ** 24, TOP), (0, 1, 7, 8, TOP, 2 ** 32 - 1)):
            cases.append((score, qs, qe, ts, te, flags, min_score, min_span))
    out = run(drivers, "keep", ["%d %d %d %d %d %d %d %d" % c for c in cases])
    for c, line in zip(cases, out):
        score, qs, qe, ts, te, flags, min_score, min_span = c
        assert int(line) == R.keep((score, 0, qs, qe, ts, te, 0, flags), min_score, min_span), c
    assert R.keep((10, 2, 0, 8, 5, 12, 9, 0), 10, 7) and not R.keep((10, 2, 0, 8, 5, 12, 9, 0), 11, 7) and not R.keep((10, 2, 0, 8, 5, 12, 9, 0), 10, 8)
    assert R.keep((0, 0, 0, 0, 0, 0, 70000, 1), TOP, TOP)          # an overflowed pair is never lost


def test_the_approximate_paf_line():
    rec = (40, 3, 10, 60, 110, 175, 9, 0)
    assert R.paf_line("a", 100, "b", 300, rec, 15) == "a\t100\t10\t60\t+\tb\t300\t110\t175\t45\t65\t255\tcs:i:40\tcn:i:3"
    assert R.paf_line("a", 100, "b", 300, rec, 15, minus=True) == "a\t100\t10\t60\t-\tb\t300\t125\t190\t45\t65\t255\tcs:i:40\tcn:i:3"
    assert R.paf_line("a", 100, "b", 300, (40, 9, 10, 60, 110, 175, 9, 0), 15).split("\t")[9] == "50"     # capped at the shorter span


# ---------------------------------------------------------------- the companion header and its mirrors
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declared(path):
    return sorted(set(re.findall(r"\b(aln_[a-z_0-9]+)\s*\(", strip_comments(open(path).read()))))


def test_the_companion_header_declares_the_seedchain_exports():
    assert declared(os.path.join(ROOT, "include", "aligner_hip_seedchain.h")) == sorted(_ffi.SEEDCHAIN_EXPORTS)
    assert _ffi.SEEDCHAIN_EXPORTS == ["aln_seqset_candidate_chain_filter", "aln_seqset_candidate_chain_records", "aln_seqset_candidate_chains"]
    # the pinned ones are as they were
    assert len(declared(os.path.join(ROOT, "include", "aligner_hip.h"))) == 61
    assert _ffi.SEEDJOIN_EXPORTS == ["aln_seqset_candidate_diags", "aln_seqset_seed_index", "aln_seqset_seed_join"]
    others = [getattr(_ffi, name) for name in dir(_ffi) if name.endswith("EXPORTS") and name != "SEEDCHAIN_EXPORTS"]
    assert len(others) >= 10
    for lst in others:
        assert not set(_ffi.SEEDCHAIN_EXPORTS) & set(lst)
    assert "aln_seedchain.hip" in native_build.SOURCES and "aln_seedchain_rules.h" in native_build.HEADERS
    assert any(h.endswith("aligner_hip_seedchain.h") for h in native_build.HEADERS)
    text = strip_comments(open(os.path.join(ROOT, "include", "aligner_hip_seedchain.h")).read())
    assert '#include "aligner_hip_seedjoin.h"' in text


def test_the_library_exports_them_with_argtypes():
    native_build.build()
    lib = _ffi.load()
    for sym in _ffi.SEEDCHAIN_EXPORTS:
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is C.c_int, sym
    assert lib.aln_abi_version() == 2


def test_every_export_is_called_from_c99():
    src = strip_comments(open(os.path.join(ROOT, "tests", "abi_seedchain.c")).read())
    for sym in _ffi.SEEDCHAIN_EXPORTS:
        assert re.search(r"\b%s\s*\(" % sym, src), sym


def test_the_header_compiles_as_c99_and_the_layouts_match(tmp_path):
    native_build.build()
    src = str(tmp_path / "only.c")
    with open(src, "w") as fh:
        fh.write('#include "aligner_hip_seedchain.h"\nint main(void) { return (int)sizeof(aln_seedchain_spec) - 48 + (int)sizeof(aln_chain_record) - 32 + '
                 '(int)sizeof(aln_seedchain_summary) - 32; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                           str(tmp_path / "only.o")])
    exe = native_build.build_seedchain_harness()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("layout ")]
    assert [l[1] for l in lines] == ["aln_seedchain_spec", "aln_chain_record", "aln_seedchain_summary"]
    for l, cls, size in zip(lines, (_ffi.SeedchainSpec, _ffi.ChainRecord, _ffi.SeedchainSummary), (48, 32, 32)):
        assert int(l[2]) == C.sizeof(cls) == size
        fields = [(l[k], int(l[k + 1]), int(l[k + 2])) for k in range(3, len(l), 3)]
        assert fields == [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, _t in cls._fields_]
    assert [name for name, _t in _ffi.SeedchainSpec._fields_] == ["k", "alphabet", "max_occ", "max_gap", "max_skew", "gap_scale", "max_pair_seeds", "chunk_anchors",
                                                                  "flags", "reserved"]
    assert all(getattr(_ffi.SeedchainSpec, name).size == 4 for name, _t in _ffi.SeedchainSpec._fields_[:-1]) and _ffi.SeedchainSpec.reserved.size == 12
    assert tuple(name for name, _t in _ffi.ChainRecord._fields_) == R.FIELDS
    assert [name for name, _t in _ffi.SeedchainSummary._fields_] == ["anchors", "with_anchor", "overflowed", "chunks"]
    # the numpy records of the Python layer and of the reference are the C record
    from aligner_amd.seqset import CHAIN_RECORD
    assert CHAIN_RECORD == R.RECORD and CHAIN_RECORD.itemsize == 32
    assert [CHAIN_RECORD.fields[name][1] for name in R.FIELDS] == [getattr(_ffi.ChainRecord, name).offset for name in R.FIELDS]


# ---------------------------------------------------------------- refusals that need no device
def test_refusals_without_a_device():
    native_build.build()
    lib = _ffi.load()
    INV = _ffi.ERR_INVALID_ARGUMENT
    count = C.c_uint64(99)
    recs = np.full(4, 7, dtype=np.uint8).repeat(32)
    summ = _ffi.SeedchainSummary(5, 5, 5, 5)
    spec = _ffi.SeedchainSpec(12, 4, 0, 1000, 200, 2, 0, 0, 0, (C.c_uint32 * 3)(0, 0, 0))

    def untouched():
        return count.value == 99 and bool((recs == 7).all()) and (summ.anchors, summ.with_anchor, summ.overflowed, summ.chunks) == (5, 5, 5, 5)

    assert lib.aln_seqset_candidate_chains(None, C.byref(spec), 0, 4, recs.ctypes.data, C.byref(summ)) == INV and untouched()
    assert lib.aln_seqset_candidate_chains(None, None, 0, 0, None, None) == INV and untouched()
    assert lib.aln_seqset_candidate_chain_filter(None, C.byref(spec), 0, 0, C.byref(summ), C.byref(count)) == INV and untouched()
    assert lib.aln_seqset_candidate_chain_filter(None, None, 0, 0, None, None) == INV and untouched()
    assert lib.aln_seqset_candidate_chain_records(None, 0, 4, recs.ctypes.data) == INV and untouched()
    assert b"null" in lib.aln_last_error()


# ---------------------------------------------------------------- the command's new argument errors
@pytest.mark.parametrize("extra,message", [
    (["--chain"], "error: --chain chains the seeds of a join's candidates: give --kmer K with --seed-join or --word-join"),
    (["--kmer", "3", "--chain"], "error: --chain chains the seeds of a join's candidates: give --kmer K with --seed-join or --word-join"),
    (["--kmer", "3", "--seed-join", "--chain-paf", "x.paf"], "error: --chain-paf writes the chains of --chain: give --chain"),
    (["--chain-paf", "x.paf"], "error: --chain-paf writes the chains of --chain: give --chain"),
    (["--kmer", "3", "--seed-join", "--max-gap", "5"], "error: --max-gap / --max-skew / --min-chain-score / --min-chain-span are the parameters of --chain"),
    (["--kmer", "3", "--seed-join", "--min-chain-score", "5"], "error: --max-gap / --max-skew / --min-chain-score / --min-chain-span are the parameters of --chain"),
    (["--kmer", "3", "--seed-join", "--chain", "--max-gap", "0"], "error: --max-gap: G must lie in 1 .. 2^31 - 1"),
    (["--kmer", "3", "--seed-join", "--chain", "--max-gap", str(2 ** 31)], "error: --max-gap: G must lie in 1 .. 2^31 - 1"),
    (["--kmer", "3", "--seed-join", "--chain", "--max-skew", "-1"], "error: --max-skew: B must lie in 0 .. 2^31 - 1"),
    (["--kmer", "3", "--seed-join", "--chain", "--min-chain-span", "-1"], "error: --min-chain-span: L must lie in 0 .. 2^32 - 1"),
    (["--kmer", "3", "--seed-join", "--chain", "--min-chain-score", str(2 ** 31)], "error: --min-chain-score: S must fit 32 signed bits"),
    (["--kmer", "9", "--word-join", "--chain"], "error: --kmer with --word-join: K must lie in 1 .. 8"),
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
