"""The batch plan (aligner_amd/csrc/aln_plan_rules.h over aln_layout_rules.h) run on the CPU: tests/plan_rules_driver.cpp, built with
g++, plans the cases of tests/plan_cases.py and must reproduce tests/golden/plan_cases.json exactly -- every scalar of the Chunk, a
64-bit FNV-1a hash of its descriptors, its queue and its route lists, the bounds of the range (aln_plan_bounds), the bytes the fill
stores (aln_batch_direction_bytes) and the chunks of the whole list (aln_make_chunks).

The fixture was recorded from the parent of the commit that moved the plan into the header, 22ec53a748c3fe93e7de190439fbcb4a5661c4b2:
its chunk_plan, the `Need` loop of aln_align_batch, make_chunks and aln_batch_direction_bytes, run on the host through a dump
function that was added to a copy of that commit's aln_host.hip and never committed (a DevCtx of 256 CUs, the call analysed by
call_init from the case's scheme, the knobs set in the environment).  It holds specs of lengths, knobs and recorded values only.

The n >= 2^24 stable_sort fallback of aln_plan_order has no case: a fixture of that size does not belong in the repository.

The Python restatements that the GPU tests expect routes and orders from are tied to the same driver here: route_cases.plan(),
test_coop_lean_cpu.pair_cost and tb_batch_cases.duo_halves."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import plan_cases as pc
import route_cases as rc
import tb_batch_cases as tc
from test_coop_lean_cpu import pair_cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        doc = json.load(f)
    assert doc["cus"] == pc.CUS and tuple(doc["call_fields"]) == pc.FACTS and tuple(doc["plan_fields"]) == pc.SCALARS
    return {c["name"]: c for c in doc["cases"]}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the plan-rule driver" % cxx)
    d = tmp_path_factory.mktemp("plan_rules")
    exe = d / "drv"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "aligner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "plan_rules_driver.cpp"), "-o", str(exe)])
    counter = [0]

    def run(cases_and_facts, lists=False):
        """[(case, call facts)] -> {name: parsed line}, and with lists {name: {list: [int]}}"""
        lines, paths = [], {}
        for c, facts in cases_and_facts:
            counter[0] += 1
            tab = d / ("t%d.bin" % counter[0])
            np.stack(pc.tables(c), axis=1).astype(np.uint64).tofile(tab)
            paths[c["name"]] = d / ("l%d.txt" % counter[0]) if lists else "-"
            lines.append(pc.case_line(c, facts, tab, paths[c["name"]]))
        src = d / ("cases%d.txt" % counter[0])
        src.write_text("\n".join(lines) + "\n")
        out = dict(pc.parse_line(ln) for ln in subprocess.run([str(exe), str(src)], capture_output=True, text=True, check=True).stdout.splitlines())
        assert list(out) == [c["name"] for c, _ in cases_and_facts]
        if not lists:
            return out
        got = {}
        for name, path in paths.items():
            got[name] = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in open(path).read().splitlines()}
        return out, got
    return run


@pytest.fixture(scope="module")
def planned(driver, golden):
    """every case of the fixture through the driver, once"""
    cs = pc.cases()
    assert [c["name"] for c in cs] == list(golden)
    for c in cs:
        g = golden[c["name"]]
        assert g["spec"] == c["spec"] and g["env"] == c["env"], c["name"]
    return driver([(c, dict(zip(pc.FACTS, golden[c["name"]]["call"]))) for c in cs], lists=True)


def test_the_driver_reproduces_the_parents_plans(planned, golden):
    out, _ = planned
    for name, g in golden.items():
        got = out[name]
        for key, want in zip(pc.SCALARS, g["plan"]):
            assert got[key] == want, (name, key, got[key], want)
        assert got["chunks"] == g["chunks"], (name, got["chunks"], g["chunks"])


def test_the_cases_turn_the_rules_they_name(golden):
    """The recorded values themselves: each pair of neighbouring cases lies on the two sides of its rule."""
    def p(name):
        return dict(zip(pc.SCALARS, golden[name]["plan"]))
    assert p("n16")["n_single"] == 16 and p("n17")["n_single"] == 0                        # a sizeable pair in a chunk of at most 16
    assert p("real4")["n_wg"] == 4 and p("real5")["n_wg"] == 0                             # one workgroup per pair: at most four pairs
    assert p("not_alone/overlap")["overlap"] == 0 and p("block/overlap/held/base")["overlap"] == 1
    assert p("block/coop/held/base")["coop"] == 1 and p("many_chunks/coop")["coop"] == 0
    assert p("not_alone/coop")["coop_linger"] == 0 and p("block/coop/held/base")["coop_linger"] == 1
    # single route: R = 1 up to 2560 rows; beyond 4096 strips R doubles; ALN_SINGLE_R=3 runs as 2
    fnv = {v: p("single/m2560" if v == 1 else "single/m2561")["h_single_r"] for v in (1, 2)}
    assert fnv[1] != fnv[2] and p("single/r3")["h_single_r"] == fnv[2] and p("single/m262144")["h_single_r"] == fnv[1]
    assert p("single/m262145")["h_single_r"] == fnv[2] and p("single/m262145")["n_single"] == 1
    # (the staged query's LDS refuses a pair long before the limit of 100 000 columns does)
    assert p("single/lds_in")["n_single"] == 1 and p("single/lds_out")["n_single"] == 0 and p("single/off")["n_single"] == 0
    assert p("single/n100000")["n_single"] == 0 and p("single/n100001")["n_single"] == 0
    # one workgroup: 65 .. 2048 rows; R = 1 / 2 / 4 by rows; ALN_WG_R within 16 strips
    assert [p("wg/m%d" % M)["n_wg"] for M in (64, 65, 2048, 2049)] == [0, 1, 1, 0]
    r = {M: p("wg/m%d" % M)["h_wg_r"] for M in (65, 512, 513, 1024, 1025, 2048)}
    assert r[65] == r[512] != r[513] == r[1024] != r[1025] == r[2048] != r[65]
    assert p("wg/r1_16_strips")["h_wg_r"] == r[65] and p("wg/r1_17_strips")["h_wg_r"] == r[1025] and p("wg/r4")["h_wg_r"] == r[2048]
    assert p("wg/h_dump")["n_wg"] == 1 and p("wg/h_dump")["hmat_elems"] == 301 * 301
    assert p("scattered")["seq_direct"] == 0 and p("packed")["seq_direct"] == 1 and p("scattered")["seq_span"] == p("packed")["seq_span"]
    # the lean edges
    assert [p("lean/pairs_%d" % n)["coop_lean"] for n in (pc.LEAN_N - 1, pc.LEAN_N)] == [0, 1]
    assert [p("lean/tail_" + w)["coop_lean"] for w in ("in", "out")] == [1, 0] and [p("lean/head_" + w)["coop_lean"] for w in ("in", "out")] == [1, 0]
    assert p("lean/tail_out")["coop"] == 1 and p("c5/held")["coop_lean"] == 1 and p("c5/shard")["coop"] == 1
    assert p("share/coop_tail")["coop_tail"] == 21 - 5 and p("share/fill_wgs")["grid"] == 1
    assert p("share/chain")["grid"] == 2 * pc.CUS < p("share/no_chain")["grid"]
    # order: equal pairs keep their index order without a sort
    assert p("order/sorted")["h_order"] != p("order/unsorted")["h_order"]


def test_equal_costs_keep_index_order(planned):
    _, lists = planned
    for name in ("order/sorted", "order/unsorted", "order/equal", "block/duo/held/base", "c5/shard"):
        order, cost = np.array(lists[name]["order"]), np.array(lists[name]["cost"])
        assert np.array_equal(order, order[np.lexsort((order, -cost[order]))]), name
    assert lists["order/sorted"]["order"] == list(range(1000))
    c = np.array(lists["order/equal"]["cost"])
    assert len(np.unique(c)) < len(c) and (np.diff(c[np.array(lists["order/equal"]["order"])]) <= 0).all() and (np.diff(c) > 0).any()


def test_statuses_of_empty_sequences(planned, golden):
    """An empty query and an empty target fail (ALN_ERR_EMPTY_SEQUENCE); PWM scoring of an empty target succeeds with nothing to do."""
    out, lists = planned
    for name in ("empty/query", "empty/target", "empty/pwm_target"):
        assert lists[name]["cost"][1] == 0 and lists[name]["cost"][0] > 0 and out[name]["n_small"] == 3
    assert out["empty/query"]["h_descs"] != out["empty/target"]["h_descs"] and out["pwm/8"]["n_small"] == 8


def test_bounds_hold_for_every_chunk_of_a_forced_chunking(planned):
    """aln_plan_bounds raised over the ranges of a pipelined call is at least what slot_ensure sizes from each range's own plan."""
    out, _ = planned
    multi = [name for name, o in out.items() if "," in o["chunks"]]
    assert {n.split("/")[1] for n in multi if n.startswith("chunks/")} == {"c5_300", "real", "n17", "mixed", "global", "pwm"}
    assert all(any(n.endswith(cells) for n in multi) for cells in pc.FORCED_CELLS)
    for name in multi:
        assert out[name]["bounds"] == "hold", (name, out[name]["bounds"])


def test_route_cases_plan_is_the_headers_plan(planned):
    """route_cases.plan(), which the GPU route tests expect `aln route:` lines from, against the driver on every block and variant."""
    out, lists = planned
    checked = 0
    for c in pc.cases():
        if not c["name"].startswith("block/"):
            continue
        b = rc.block(c["spec"].split(":")[1])
        N, M = pc.lengths(c["spec"])
        _, dele, ext, kind = rc.schemes()[b.scheme]
        want = rc.plan(N, M, kind, b.local(), dele, ext, c["held"], c["env"])
        o, l = out[c["name"]], lists[c["name"]]
        got = dict(pairs=o["n"], small=o["n_small"], single=o["n_single"], wg=o["n_wg"], duo=int(o["duo_qo"] != 0), overlap=o["overlap"],
                   share="coop" if o["coop"] else "lean" if o["coop_lean"] else "none")
        assert got == {k: want[k] for k in got}, (c["name"], got, want)
        assert l["single"] == list(np.flatnonzero(want["single_mask"])) and l["wg"] == list(np.flatnonzero(want["wg_mask"])), c["name"]
        checked += 1
    assert checked == 9 * 2 * 7


def test_restated_costs_and_queue_orders_are_the_headers(planned, driver, golden):
    _, lists = planned
    # test_coop_lean_cpu.pair_cost on the lengths it is used with: C5, the 8-way shard, the large pairs, the mixed batch
    for name in ("c5/held", "c5/shard", "share/chain", "lean/tail_in"):
        N, M = pc.lengths(next(c["spec"] for c in pc.cases() if c["name"] == name))
        assert lists[name]["cost"] == [pair_cost(int(a), int(b)) for a, b in zip(N, M)], name
    extra = [pc.case("coop_lean/long", "1900x2000*50"), pc.case("coop_lean/few_long", "20000x8000*32+100x100*600")]
    _, got = driver([(c, dict(zip(pc.FACTS, golden["c5/held"]["call"]))) for c in extra], lists=True)
    for c in extra:
        N, M = pc.lengths(c["spec"])
        assert got[c["name"]]["cost"] == [pair_cost(int(a), int(b)) for a, b in zip(N, M)]
    # tb_batch_cases.duo_halves: the queue's order (cost, then position) of its two-pairs-per-wave batches
    modes = ("ubatch_a", "ubatch_b", "ubatch_c")
    batches = {m: tc.batch_of(m)[0] for m in modes}
    cs = []
    for m in modes:
        spec = "+".join("%dx%d" % (len(q), len(t)) for q, t in batches[m])
        cs.append(pc.case("duo/" + m, spec, "INT44", local=False))
    out, got = driver([(c, dict(zip(pc.FACTS, golden["block/duo/held/base"]["call"]))) for c in cs], lists=True)
    for m in modes:
        half = [0] * len(batches[m])
        for qpos, i in enumerate(got["duo/" + m]["order"]):
            half[i] = qpos & 1
        assert half == tc.duo_halves(batches[m]), m
