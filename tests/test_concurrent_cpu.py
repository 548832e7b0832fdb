"""What tests/test_concurrent_gpu.py stands on, without a GPU: the schedule covers every pair of jobs, every exported family that takes
a context or a handle has a job, the LDS group asks one kernel for two sizes above 64 KiB (by the layout and plan rules compiled for
the host), every expectation comes from the CPU alone and is stable, and the runner's comparison reports what it is fed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import concurrent_cases as CC  # noqa: E402
from aligner_amd import _ffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def names():
    return [j.name for j in CC.jobs()]


def test_the_catalogue_holds_every_entry_without_knobs():
    import call_history as CH
    have = names()
    for e in CH.catalogue():
        assert (e.name in have) == (not e.env), e.name
    assert sorted(e.name for e in CH.catalogue() if e.env) == sorted(CC.LEFT_OUT)
    for n in ("staged_batch", "seqset_held", "pairset_walk", "transform_device", "refusal_scan", "refusal_null") + sum(CC.LDS_PAIRS, ()):
        assert n in have


def test_the_schedule_covers_every_pair_of_jobs():
    rounds = CC.rounds()
    n = len(names())
    want = CC.all_pairs(names())
    assert len(want) == n * (n + 1) // 2 and all((a, a) in want for a in names())
    assert CC.covered(rounds) >= want, sorted(want - CC.covered(rounds))[:5]
    assert all(len(r) == CC.ROUND and set(r) <= set(names()) for r in rounds)
    assert CC.ROUND > 4, "more threads than the pool has slots (ALN_POOL_SLOTS): a lease waits in every round"
    assert rounds == CC.rounds(), "deterministic"
    # the dedicated rounds: the two members alternate, nothing else beside them
    lds = CC.lds_rounds()
    assert len(lds) == len(CC.LDS_PAIRS) == 2
    for r, (a, b) in zip(lds, CC.LDS_PAIRS):
        assert len(r) == CC.ROUND and r.count(a) == r.count(b) == CC.ROUND // 2 and CC.pair_key(a, b) in CC.covered([r])
    r = CC.refusal_round()
    assert len(r) == len(set(r)) == CC.ROUND and r[:2] == ["refusal_scan", "refusal_null"] and set(r) <= set(names())
    assert CC.join_timeout(rounds[0], CC.REPS) >= CC.JOIN_FLOOR_S == 30.0 and CC.LDS_REPS >= 200 and CC.REPS == 3


# the context's own: made before and destroyed after every caller, never beside one
CONTEXT_ITSELF = {"aln_destroy", "aln_device_count", "aln_device_info"}


def test_every_family_that_takes_a_context_or_a_handle_has_a_job():
    """The families are read off the bound prototypes: aln_<family>_... whose first argument is a pointer (the context, or a handle made
    from one)."""
    lib = _ffi.load()
    bound = _ffi.EXPORTS + _ffi.CLUSTER_EXPORTS + _ffi.PREFILTER_EXPORTS + _ffi.WORDJOIN_EXPORTS + _ffi.SEEDJOIN_EXPORTS + _ffi.SEARCH_EXPORTS + \
        _ffi.PROFILE_EXPORTS + _ffi.MSA_EXPORTS + _ffi.CIGAR_EXPORTS + _ffi.STRAND_EXPORTS
    families = {}
    for sym in bound:
        args = getattr(lib, sym).argtypes
        if args and args[0] is C.c_void_p and sym not in CONTEXT_ITSELF:
            families.setdefault(sym.split("_")[1], []).append(sym)
    assert {"align", "batch", "scan", "shuffle", "pairset", "transform", "seqset", "cluster"} <= set(families), sorted(families)
    called = set().union(*(j.calls for j in CC.jobs()))
    assert called <= set(bound), sorted(called - set(bound))
    for fam, syms in sorted(families.items()):
        assert called & set(syms), "no job calls any of %s" % syms


DRIVER = r"""
#include <cstdio>
#define __host__
#define __device__
struct uint4;
#include "aln_device.h"
#include "aln_plan_rules.h"
int main(int argc, char **argv)
{
    printf("shuffle %u %u\n", (unsigned)ALN_SHUFFLE_THREADS, (unsigned)ALN_SHUFFLE_LDS_MAX);
    for (int i = 1; i + 1 < argc; i += 2) {
        AlnPlanCall c;
        c.fast = true; c.is_int = true; c.hazard = true; c.semantics = ALN_CORE_LOCAL; c.rows = 24; c.cols = 24;
        AlnPlanKnobs kn;
        Chunk k;
        k.n = 1;
        k.descs.resize(1);
        PairDesc &d = k.descs[0];
        d.N = (uint32_t)atoi(argv[i]); d.M = (uint32_t)atoi(argv[i + 1]); d.status = ALN_OK;
        const bool big = aln_big_pair(d, 1), to_single = aln_big_to_single(256, c, kn, k);
        const uint32_t R = aln_single_route_r(c, kn, d), ns = R ? aln_uniform_strips(d.M, R) : 0;
        // aln_single_waves (aln_kernels.hip): four strips per workgroup where the steady state exists and the LDS fits
        const uint32_t W = (R && R <= 2 && ns >= 2 && aln_single_lds_bytes(c.rows, c.cols, R, d.N, 4) <= 150u * 1024u) ? 4u : 1u;
        printf("single %u %u big %d to_single %d R %u ns %u W %u lds %u\n", d.N, d.M, big ? 1 : 0, to_single ? 1 : 0, R, ns, W,
               R ? aln_single_lds_bytes(c.rows, c.cols, R, d.N, W) : 0u);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """the layout and plan rules of the LDS group's single pairs (and one row short of the smallest target), compiled for the host"""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the rules driver" % cxx)
    d = tmp_path_factory.mktemp("concurrent_rules")
    src, exe = d / "rules.cpp", d / "rules"
    src.write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "aligner_amd", "csrc"), str(src), "-o", str(exe)])
    singles = [j.lds for j in CC.jobs() if j.lds and j.lds["kind"] == "single"]
    argv = [str(x) for s in singles for x in (s["N"], s["M"])] + [str(x) for s in singles for x in (s["N"], s["M"] - 1)]
    lines = [l.split() for l in subprocess.check_output([str(exe)] + argv, text=True).splitlines()]
    assert lines[0][0] == "shuffle"
    out = dict(threads=int(lines[0][1]), lds_max=int(lines[0][2]), single={})
    for l in lines[1:]:
        out["single"][(int(l[1]), int(l[2]))] = {l[k]: int(l[k + 1]) for k in range(3, len(l), 2)}
    return out


def lds_bytes(job, rules):
    if job.lds["kind"] == "single":
        return rules["single"][(job.lds["N"], job.lds["M"])]["lds"]
    return ((job.lds["t_len"] + 15) & ~15) * rules["threads"]           # shuffle_lds_slot (aln_host.hip) x the workgroup's threads


def test_the_lds_group_asks_one_kernel_for_two_sizes_above_64_kib(rules):
    table = CC.by_name()
    assert rules["threads"] == CC.SHUFFLE_THREADS and rules["lds_max"] == 2048
    for a, b in CC.LDS_PAIRS:
        x, y = lds_bytes(table[a], rules), lds_bytes(table[b], rules)
        assert min(x, y) > CC.LDS_FLOOR and abs(x - y) >= CC.LDS_APART, (a, x, b, y)
        assert {k: v for k, v in table[a].lds.items() if k not in ("N", "t_len")} == {k: v for k, v in table[b].lds.items() if k not in ("N", "t_len")}
    assert [lds_bytes(table[n], rules) for n in sum(CC.LDS_PAIRS, ())] == [120800, 150800, 70656, 131072]
    assert max(table[n].lds["t_len"] for n in CC.LDS_PAIRS[1]) == rules["lds_max"]
    # the plan puts both long pairs on the single-pair route, on the same kernel (rows per lane and waves per workgroup), and a target
    # one row shorter would leave the route: 128 rows is the smallest
    routes = []
    for n in CC.LDS_PAIRS[0]:
        s = table[n].lds
        r = rules["single"][(s["N"], s["M"])]
        assert r["big"] == 1 and r["to_single"] == 1 and r["R"] >= 1 and s["N"] * s["M"] >= 1 << 18, (n, r)
        assert rules["single"][(s["N"], s["M"] - 1)]["big"] == 0
        routes.append((r["R"], r["W"]))
    assert routes == [(1, 4), (1, 4)]


@pytest.fixture(scope="module")
def wants(orc):
    return CC.expectations(orc)


def test_expectations_need_no_gpu_and_are_stable(orc, wants):
    assert sorted(wants) == sorted(names())
    for j in CC.jobs():
        again = {k: np.asarray(v) for k, v in j.expected(orc).items()}
        assert CC.digest(again) == CC.digest(wants[j.name]), j.name
        assert any(not k.startswith("_") for k in wants[j.name]), j.name
    # the refusals differ in status and in text
    a, b = wants["refusal_scan"], wants["refusal_null"]
    assert a["status"][0] == _ffi.ERR_UNSUPPORTED and b["status"][0] == _ffi.ERR_INVALID_ARGUMENT and a["text"].tobytes() != b["text"].tobytes()
    # the pair-set walk holds no refusal, and its runs hold failed pairs beside aligned ones
    st = wants["pairset_walk"]["1:run_all/res.status"]
    assert (st == 0).any() and (st != 0).any()
    assert int(wants["seqset_held"]["count"]) > 256


def test_the_comparison_is_not_vacuous(wants):
    job = CC.by_name()["fast_local_short"]
    want = wants[job.name]
    good = {k: np.array(v, copy=True) for k, v in want.items() if not k.startswith("_") and k != "strings"}
    tb = np.zeros(int(want["_idx"].max()) + 1, dtype=np.uint8)
    tb[want["_idx"]] = want["strings"]
    good.update(_tb=tb, _flags=np.full(len(want["score"]), _ffi.FLAG_FAST | _ffi.FLAG_INTEGER, dtype=np.uint32), _passes=np.zeros(len(want["score"]), np.uint32))
    assert CC.compare(job, good, want) == []
    bad = dict(good, score=good["score"].copy(), _tb=tb.copy())
    bad["score"][7] += 1.0
    bad["_tb"][want["_idx"][11]] ^= 1
    found = CC.compare(job, bad, want)
    assert len(found) == 2 and any(d.startswith("score differs first at [7]") for d in found) and any(d == "strings differ first at byte 11 of %d" % len(want["strings"])
                                                                                                      for d in found), found
    off_route = dict(good, _flags=good["_flags"] | _ffi.FLAG_SINGLE)
    assert len(CC.compare(job, off_route, want)) == 1 and "route" in CC.compare(job, off_route, want)[0]
    # per-family bytes, and the bit-for-bit job
    want = wants["seqset_held"]
    bad = {k: np.array(v, copy=True) for k, v in want.items()}
    bad["words"][3] += 16
    bad["aligned"][5] ^= 1
    assert len(CC.compare(CC.by_name()["seqset_held"], bad, want)) == 2
    want = wants["transform_device"]
    bad = {k: np.array(v, copy=True) for k, v in want.items()}
    bad["0/out"].view(np.uint64)[0, 0, 0] ^= 1
    assert CC.compare(CC.by_name()["transform_device"], bad, want) == ["0/out: not the same bits"]
    # the overlap rule
    assert CC._overlap([(0, 10, "a")], [(9, 12, "b")]) and not CC._overlap([(0, 10, "a"), (20, 30, "a")], [(10, 20, "b"), (30, 31, "b")])


def test_a_stuck_round_stops_every_later_one(wants):
    assert not CC.STUCK
    CC.STUCK.append("made_up")
    try:
        with pytest.raises(RuntimeError, match="nothing more is started"):
            CC.run_round(["refusal_null"], wants, 1)
    finally:
        CC.STUCK.clear()
