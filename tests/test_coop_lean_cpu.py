"""Which build of the fast batch kernel a chunk that could share strips runs (aln_coop_lean_plan, aligner_amd/csrc/aln_plan_rules.h;
no GPU): the lean build (no cooperative machinery) for C5's 100 000 pairs, the cooperative one where sharing pays -- the 12 500-pair
shard, batches of large pairs, a batch of short pairs with a few long ones -- and the ALN_COOP_LEAN setting overriding either way.
The queue costs are modelled here with aln_plan_rules.h's aln_pair_cost (tests/test_plan_rules_cpu.py checks the restatement); tests/test_coop_lean_gpu.py checks the figures the library itself
plans with (ALN_TRACE_PLAN)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from aligner_amd import workloads
from aligner_amd.distributed import lpt_shards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                                 # MI355X
RESIDENT_WGS = CUS * 3                    # three workgroups of four waves per CU
FULL_WGS = CUS * 4                        # the grid without the overlapped traceback (chunk_plan: at most four workgroups per CU)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "aln_plan_rules.h"
int main(int argc, char **argv)
{
    // <costs file: one u64 per line, LPT order> grid cus setting -> lean waves resident tail
    if (argc != 5) return 2;
    std::vector<unsigned long long> cost;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 3;
    unsigned long long v;
    double total = 0;
    while (fscanf(f, "%llu", &v) == 1) { cost.push_back(v); total += (double)v; }
    fclose(f);
    const AlnLeanPlan p = aln_coop_lean_plan(cost.size(), (uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), total,
                                             [&](size_t j) { return cost.at(j); }, atoi(argv[4]));
    printf("%d %llu %llu %llu\n", p.lean ? 1 : 0, (unsigned long long)p.waves, (unsigned long long)p.resident, (unsigned long long)p.tail);
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the plan-rule driver" % cxx)
    d = tmp_path_factory.mktemp("plan_rules")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), str(src), "-o", str(exe)])
    counter = [0]

    def call(costs, grid, setting=-1):
        counter[0] += 1
        path = d / ("costs%d.txt" % counter[0])
        np.savetxt(path, np.asarray(costs, dtype=np.uint64), fmt="%d")
        out = subprocess.run([str(exe), str(path), str(grid), str(CUS), str(setting)], capture_output=True, text=True, check=True).stdout.split()
        return out[0] == "1", int(out[1]), int(out[2]), int(out[3])
    return call


def pair_cost(N, M):
    """aln_plan_rules.h's aln_pair_cost: steps x (24 + 21 R) over the pair's strips (512 rows; the last picks R by its rows)."""
    c = 0
    ns = (M + 511) // 512
    for s in range(ns):
        rows = min(M - s * 512, 512)
        R = max(1, min(8, (rows + 63) // 64)) if s + 1 == ns else 8
        c += (N + (rows + R - 1) // R - 1) * (24 + 21 * R)
    return c


def lpt_costs(qlen, tlen):
    return np.sort(np.array([pair_cost(int(n), int(m)) for n, m in zip(qlen, tlen)], dtype=np.int64))[::-1]


def test_c5_runs_the_lean_build(rule):
    q, t = workloads.c5_lengths(100000)
    cost = lpt_costs(q, t)
    # a staged C5 batch with traceback runs the walk beside the fill: grid = the resident workgroups, 3072 waves
    lean, waves, resident, tail = rule(cost, RESIDENT_WGS)
    assert lean and waves == 3072 and resident == 3072 and tail == 100000 - 2 * 3072
    share = cost.sum() / 3072
    assert cost[tail] * 100 < share and cost[0] * 8 < share              # the tail's longest pair < 1 %, the longest < 1/8
    # without the walk waves (score only): 1024 workgroups, 4096 kernel waves, the share still per resident wave
    lean, waves, resident, tail = rule(cost, FULL_WGS)
    assert lean and waves == 4096 and resident == 3072 and tail == 100000 - 2 * 4096


def test_sharing_batches_keep_the_cooperative_build(rule):
    q, t = workloads.c5_lengths(100000)
    shard = lpt_shards(q * t, 8)[0]                                      # the 8-way shard: ~12 500 pairs, 4 per wave
    assert 12000 < len(shard) < 13000
    assert not rule(lpt_costs(q[shard], t[shard]), FULL_WGS)[0]
    big = np.full(256, 4200)                                             # large_pairs_batch: one workgroup per 4 pairs
    assert not rule(lpt_costs(big, big), 64)[0]
    # many pairs per wave, every one of them long: the tail is a long re-fill
    assert not rule(lpt_costs(np.full(60000, 1900), np.full(60000, 2000)), FULL_WGS)[0]
    # many short pairs and a few very long multi-strip pairs: a re-fill of one of those could end in the tail
    qs = np.concatenate([np.full(32, 20000), np.full(60000, 100)])
    ts = np.concatenate([np.full(32, 8000), np.full(60000, 100)])
    cost = lpt_costs(qs, ts)
    share = cost.sum() / 3072
    assert cost[len(cost) - 2 * 4096] * 64 <= share and cost[0] * 4 > share     # the tail alone would pass, the longest does not
    assert not rule(cost, FULL_WGS)[0]


def test_rule_edges(rule):
    w = RESIDENT_WGS * 4
    n = 16 * w
    base = np.full(n, 100, dtype=np.int64)
    # below 16 pairs per resident wave never
    assert not rule(base[:n - 1], RESIDENT_WGS)[0]
    # at 16 it is the tail's share that decides: with its 2 w pairs at X the share is 1400 + 2 X, and X <= share / 64 up to X = 22
    c = base.copy(); c[-2 * w:] = 22
    assert rule(c, RESIDENT_WGS)[0]
    c[-2 * w:] = 23
    assert not rule(c, RESIDENT_WGS)[0]
    # the longest pair: at most a quarter of the share (tail pairs at 1: share = 1402 + (c0 - 100) / w, a quarter of it 350.5)
    c = base.copy(); c[-2 * w:] = 1; c[0] = 350
    assert rule(c, RESIDENT_WGS)[0]
    c[0] = 352
    assert not rule(c, RESIDENT_WGS)[0]
    # ALN_COOP_LEAN: 0 never, 1 always
    q, t = workloads.c5_lengths(100000)
    assert not rule(lpt_costs(q, t), RESIDENT_WGS, setting=0)[0]
    assert rule(lpt_costs(np.full(256, 4200), np.full(256, 4200)), 64, setting=1)[0]
