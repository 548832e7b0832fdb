"""The helper of the set-route tests (tests/route_cases.py), without a GPU: every block's lengths meet the restated precondition of
its route in chunk_plan, the oracle gives every pair the status the GPU test relies on (ALN_OK everywhere but the pairs of the
sequence that ends in code 24), the long pairs' alignments are longer than 256 columns and cross a strip boundary, the schedule
holds every ordered pair of blocks once, and the schemes are on the kernel family the table says (aln_scheme_rules.h, through the
driver of test_scheme_rules_cpu.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as ch  # noqa: E402
import route_cases as rc  # noqa: E402
from test_scheme_rules_cpu import classify, route  # noqa: E402,F401  (classify: the fixture that builds and runs the rule driver)

ENV = rc.CHILD_ENV


def lengths_of(b, ok_only=False):
    L = rc.set_lengths()
    q, t = b.pairs()
    if ok_only:
        keep = np.array([rc.LAYOUT[a] != rc.BAD and rc.LAYOUT[c] != rc.BAD for a, c in zip(q, t)])
        q, t = q[keep], t[keep]
    return L[q], L[t]


def planned(b, traceback, env=ENV, ok_only=None):
    N, M = lengths_of(b, traceback if ok_only is None else ok_only)
    _, dele, ext, kind = rc.schemes()[b.scheme]
    return rc.plan(N, M, kind, b.local(), dele, ext, traceback, env)


def test_the_set_and_the_ranges():
    p = rc.pool()
    assert len(p) == 102 and len(set(rc.LAYOUT)) == 102 and rc.LAYOUT[:rc.N_SHORT] == rc.SHORTS
    shorts = [p[n] for n in rc.SHORTS]
    assert all(20 <= len(s) <= 120 and (s == 0).any() and s.max() < 20 for s in shorts)
    assert len(p["s0"]) == 30 and len(p["s91"]) == 40 and len({len(s) for s in shorts}) > 40
    assert [len(p["L%d" % n]) for n in rc.LONG_LENGTHS] == list(rc.LONG_LENGTHS) and all(p["L%d" % n].max() < 20 for n in rc.LONG_LENGTHS)
    assert len(p[rc.BAD]) == 600 and p[rc.BAD][-1] == 24 and p[rc.BAD][:-1].max() < 20
    rc._pool.clear()                                                                   # the same every time
    again = rc.pool()
    assert all(np.array_equal(p[n], again[n]) for n in p)
    names = [b.name for b in rc.blocks()]
    assert names[:rc.SCHEDULE_BLOCKS] == ["duo", "overlap", "single_alone", "single_mixed", "coop", "wg_real", "wg_mixed", "wg_int"]
    for b in rc.blocks():
        assert b.q0 + b.qn <= len(rc.LAYOUT) and b.t0 + b.tn <= len(rc.LAYOUT)
        if b.names:
            assert rc.LAYOUT[b.q0:b.q0 + b.qn] == b.names[0] and rc.LAYOUT[b.t0:b.t0 + b.tn] == b.names[1], b.name
        q, t = b.pairs()
        assert len(q) == (b.qn * (b.qn - 1) // 2 if b.upper else b.qn * b.tn)
    assert set(rc.LAYOUT[:60]) | set(rc.LAYOUT[32:92]) <= set(rc.SHORTS)               # duo: shorts against shorts


def test_every_block_meets_the_precondition_of_its_route():
    L = rc.set_lengths()
    for b in rc.blocks():
        held = planned(b, True)
        for key, v in b.want.items():
            assert held[key] == v, (b.name, key, held[key], v)
    # duo: more pairs than 12 per CU and fewer than the overlapped traceback's 4096; rows <= 256, columns <= 1024; also the score pass
    b = rc.block("duo")
    N, M = lengths_of(b)
    assert 12 * rc.CUS < len(N) == 3600 < 4096 and M.max() <= 256 and N.max() <= 1024 and b.semantics == rc.CORE_GLOBAL
    assert planned(b, False)["duo"] == 1 and planned(b, True, dict(ENV, ALN_NO_DUO="1"))["duo"] == 0
    # overlap: at least 4096 single-strip pairs that fill three workgroups per CU; a score pass walks nothing
    b = rc.block("overlap")
    N, M = lengths_of(b)
    assert len(N) == 4186 >= 4096 and (len(N) + 3) // 4 >= 3 * rc.CUS and int((N * M).sum()) < 2000000000 and "ALN_TB_OVERLAP_ANY" in ENV
    assert planned(b, False)["overlap"] == 0 and planned(b, True, dict(ENV, ALN_TB_OVERLAP="0"))["overlap"] == 0
    assert planned(b, True, {k: v for k, v in ENV.items() if k != "ALN_TB_OVERLAP_ANY"})["overlap"] == 0
    # single_alone: 2^18 cells in a chunk of one, and the time rule alone sends it (no ALN_BIG_TO_SINGLE)
    b = rc.block("single_alone")
    N, M = lengths_of(b)
    assert (N[0], M[0]) == (600, 640) and N[0] * M[0] >= 1 << 18 and N[0] >= 64 and M[0] >= 128
    assert planned(b, True, {"ALN_TRACE_PLAN": "1"})["single"] == 1 and M[0] <= 2560              # one row per lane
    # single_mixed: the four big pairs of the score pass, two of them of the failing query; 2600 rows take two rows per lane;
    # five pairs stay with the batch kernel, so the device's identity queue is replaced
    for name in ("single_mixed", "single_mixed_global"):
        b = rc.block(name)
        q, t = b.pairs()
        sc = planned(b, False)
        big = [(rc.LAYOUT[a], rc.LAYOUT[c]) for a, c in zip(q[sc["single_mask"]], t[sc["single_mask"]])]
        assert big == [("L520", "L640"), ("L520", "L2600"), (rc.BAD, "L640"), (rc.BAD, "L2600")]
        assert sc["small"] == 5 != sc["pairs"] == 9 and L[t].max() == 2600 > 2560
        assert planned(b, True)["single"] == 2 and planned(b, True)["pairs"] == 6
    # coop: multi-strip pairs, too few to send any to the single-pair route by size, far fewer than resident waves
    b = rc.block("coop")
    N, M = lengths_of(b)
    assert 16 < len(N) == 21 and (N * M).max() < 1 << 24 and (M > rc.STRIP_ROWS).all() and planned(b, False)["share"] == "coop"
    assert planned(b, True, dict(ENV, ALN_NO_COOP="1"))["share"] == "none" and planned(b, True, dict(ENV, ALN_NO_COOP="1"))["single"] == 0
    # one workgroup per pair: at most four pairs off the fast path, 65 .. 2048 rows; 40 rows stay with the batch kernel
    for name, n in (("wg_real", 4), ("wg_mixed", 3), ("wg_int", 2)):
        b = rc.block(name)
        N, M = lengths_of(b)
        p = planned(b, True)
        assert len(N) == n <= 4 and np.array_equal(p["wg_mask"], (M >= 65) & (M <= 2048)) and (N * M)[p["wg_mask"]].min() >= 1 << 14
        assert planned(b, False)["wg"] == p["wg"] and planned(b, True, dict(ENV, ALN_NO_WGPIPE="1"))["wg"] == 0
    assert sorted(lengths_of(rc.block("wg_mixed"))[1]) == [40, 130, 1100]


def test_the_oracle_gives_every_pair_the_status_the_gpu_test_relies_on(orc):
    L = rc.set_lengths()
    crossing = 0
    for b in rc.blocks():
        want = rc.expected(orc, b)
        q, t = b.pairs()
        bad = np.array([rc.LAYOUT[a] == rc.BAD or rc.LAYOUT[c] == rc.BAD for a, c in zip(q, t)])
        assert np.array_equal(want["pair_status"], np.where(bad, rc.ERR_CODE_OUT_OF_RANGE, rc.OK)), b.name
        assert bad.sum() == (3 if b.name.startswith("single_mixed") else 0)
        assert len(want["index"]) == (~bad).sum() and ch.compare(want, want) is None
        f = want["score"]
        assert len(np.unique(f)) > min(len(f), 40) // 2, b.name                            # f varies
        # the long pairs (both sequences of 600 and more): long alignments that cross a strip boundary of the batch kernels
        N, M = L[q][~bad], L[t][~bad]
        for i in np.flatnonzero((N >= 600) & (M >= 600)):
            assert want["aln_len"][i] > 256, (b.name, i)
            first, last = (0, M[i] - 1) if not b.local() else (want["start_y"][i], want["end_y"][i])
            assert first < rc.STRIP_ROWS <= last, (b.name, int(N[i]), int(M[i]), int(first), int(last))
            crossing += 1
        if b.name == "single_mixed":
            k = rc.best_rule(q, t, want["pair_f"], want["pair_status"], b.tn, 2)
            assert len(k) == 4 and not bad[k].any() and rc.subset(want, k)["index"].tolist() == k.tolist()
    assert crossing >= 12


def test_the_schedule_holds_every_ordered_pair_of_blocks_once():
    names = rc.schedule_names()
    assert len(names) == 65 and len(ch.transitions(names)) == 64
    assert ch.transitions(names) == {(a.name, b.name) for a in rc.blocks()[:8] for b in rc.blocks()[:8]}


def test_the_schemes_run_on_the_kernel_family_the_table_says(classify):
    L = rc.set_lengths()
    sch = rc.schemes()
    for b in rc.blocks():
        S, dele, ext, kind = sch[b.scheme]
        N, M = lengths_of(b)
        r = classify(S, dele, ext, int((N + M).max()) + 2)
        assert route(r) == kind == b.want["kernels"], (b.name, r)
    S, dele, ext, _ = sch["REAL"]
    r = classify(S, dele, ext, 1300)
    assert r["scale"] == 1.0 and not r["all_int"]                                          # not dyadic: the f64 kernels fill it
    S, dele, ext, _ = sch["OFF_FAST"]
    r = classify(S, dele, ext, 700)
    assert r["is_int"] and not r["fast"] and r["smax"] == 33.0 and route(classify(sch["INT"][0], dele, ext, 700)) == "fast"
    assert L.max() == 2600
