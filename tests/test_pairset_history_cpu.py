"""The pair-set call-history test without a GPU (helpers: tests/pairset_history.py): the schedule over the catalogue, the conditions the
pair list and the catalogue's order are built for -- asserted from the oracle and the rule restatements alone -- and the walker itself,
which must pass over a backend that answers from the references and must catch each of ten planted defects.

The plan is the circuit and a tail (pairset_history.tail) that puts every transition the header allows into a state that accepts both
calls.  One condition is asserted as its opposite, and says so where it stands: cause 2 (no root after a run) cannot occur in any walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as CH  # noqa: E402
import pairset_history as H  # noqa: E402
import set_loop_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def refs(orc):
    return H.Refs(orc)


@pytest.fixture(scope="module")
def plan(refs):
    return H.dry_run(refs)


def test_the_schedule_puts_a_step_directly_after_every_entry():
    k = len(H.CATALOGUE)
    seq = H.the_schedule()
    assert 14 <= k <= 18 and len(seq) == k * k + 1
    pairs = list(zip(seq[:-1], seq[1:]))
    assert len(set(pairs)) == k * k == len(pairs) and CH.transitions(seq) == {(a, b) for a in range(k) for b in range(k)}
    names = {(H.CATALOGUE[a], H.CATALOGUE[b]) for a, b in pairs}
    # best and the going list are observed only through the next step's answers
    assert all((e, "loop_step") in names for e in H.CATALOGUE)
    assert set(H.CHANGERS) < set(H.CATALOGUE) and "set_pass" in H.CATALOGUE


def test_the_plan_meets_the_conditions(plan):
    k = len(H.CATALOGUE)
    n = len(plan)
    assert n == k * k + 1 + len(H.tail()) and [x["entry"] for x in plan[k * k + 1:]] == H.tail()
    kinds = {kd: sum(1 for x in plan if x["kind"] == kd) for kd in H.KINDS}
    refused = sum(kinds.values())
    circuit = plan[:k * k + 1]
    refused_circuit = sum(1 for x in circuit if x["kind"])
    steps = [x for x in plan if x["entry"] == "loop_step" and not x["kind"]]
    going = [x for x in steps if x["facts"]["going"] > 0]
    causes = sorted(set(c for x in steps for c in x["facts"]["causes"]))
    odd = [x["step"] for x in going if x["facts"].get("begun_after_odd")]
    # directly: the entry is the very next call after the state-changing one, and both are accepted
    direct = {(a["entry"], b["entry"]) for a, b in zip(plan[:-1], plan[1:]) if not a["kind"] and not b["kind"]}
    missing = {(a, b) for a in H.CHANGERS for b in H.CATALOGUE if (a, b) not in direct}
    # a step that follows a step (cur == 1, best not zero) directly after every entry that may stand between two steps
    second = {b["entry"] for a, b, c in zip(plan[:-2], plan[1:-1], plan[2:]) if c["entry"] == "loop_step" and not c["kind"] and c["facts"]["going"] > 0
              and not b["kind"] and a["entry"] == "loop_step" and not a["kind"] and a["facts"]["going"] > 0}
    third = sum(1 for a, b, c in zip(going[:-2], going[1:-1], going[2:]) if a["step"] + 1 == b["step"] == c["step"] - 1)
    print("calls %d (circuit %d, refused there %d), refused %d %s, steps with pairs going %d of %d, causes %s, steps after a second loop_begin at "
          "cur == 1: %d, entries between a first and a going second step: %d, third steps in a row: %d, ruled out by the header: %d" % (
              n, len(circuit), refused_circuit, refused, kinds, len(going), len(steps), causes, len(odd), len(second), third, len(H.IMPOSSIBLE)))
    assert all(v >= 1 for v in kinds.values()), kinds
    assert 3 * refused <= n and 3 * refused_circuit <= len(circuit), (refused, n, refused_circuit)
    assert len(going) >= 8
    # cause 2 after a run cannot occur: whether the transform has a root depends on kd, r_squared and the frequencies alone (the linear
    # coefficient is 2 b sum(p * base) / den and sum(p * base) is zero by construction), so a pair without one never enters the going
    # list (tests/test_set_heuristic_gpu.py says the same of the device); what loop_begin refuses is in its status array instead
    assert causes == [cases.DONE, cases.FAILED], causes
    assert odd, "no step after cur flipped an odd number of times and loop_begin ran again"
    # every entry is accepted directly after every entry that changes state, but for what the header itself rules out
    assert missing == set(H.IMPOSSIBLE), (sorted(missing - H.IMPOSSIBLE), sorted(H.IMPOSSIBLE - missing))
    assert second >= set(H.CATALOGUE) - {"heur_a", "heur_b", "loop_begin", "run_none"} and third >= 1, sorted(second)       # (a loop reaches a third going step)
    # a going step directly after the 4 x 4 run, and a fetch of the 4 x 4 run's counts
    assert any(a["entry"] == "run_dna" and b["entry"] == "loop_step" and not b["kind"] and b["facts"]["going"] > 0 for a, b in zip(plan[:-1], plan[1:]))
    assert ("run_dna", "freq_dna") in direct and ("run_all", "strings_out") in direct and ("run_subset", "strings_out") in H.IMPOSSIBLE
    # the stale entry_of form: a pair that an earlier run of every pair held is refused after run_subset
    at = [i for i, x in enumerate(plan) if x["entry"] == "strings_out" and x["prev"] == "run_subset" and x["kind"] == "not_in_last_run"]
    assert at and any(x["entry"] in ("run_all", "run_chunked") for x in plan[:at[0]])
    # every observation of the store and the held run is there after every call that can change them
    assert sum(len(x["obs"]) for x in plan) >= n


def test_loop_begin_reports_the_pair_without_a_root(refs):
    m = H.Model(refs)
    m.step("heur_b")
    _kind, spec, _f = m.step("loop_begin")
    assert spec[1][H.NO_ROOT_PAIR] == 1 and sum(spec[1]) == 1 and H.NO_ROOT_PAIR not in m.going and H.NO_ROOT_PAIR not in m.store
    m.step("heur_a")
    _kind, spec, _f = m.step("loop_begin")
    assert sum(spec[1]) == 0 and len(m.going) == H.N_PAIRS


def test_the_pairs_are_what_they_are_built_for(refs, orc):
    from aligner_amd import _ffi
    from aligner_amd.seqset import window
    assert len(refs.pairs) == H.N_PAIRS == 13
    # the block's own numbering gives the list, and the window starts and ends inside a row
    q, t = window(_ffi.SeqsetBlock(*H.BLOCK, 0), H.FIRST, H.N_PAIRS)
    assert list(zip(q.tolist(), t.tolist())) == H.window() and H.FIRST % H.BLOCK[3] and (H.FIRST + H.N_PAIRS) % H.BLOCK[3]
    run_all = {p: refs.aln(p, "L", ("P", 0))[0] for p in H.ALL}
    for p, n in H.PLANTED.items():
        assert int(run_all[p]["status"]) == 0 and int(run_all[p]["aln_len"]) == n, (p, n, run_all[p])
    assert sorted(H.PLANTED.values()) == [63, 64, 65, 127, 128, 129]
    assert (len(refs.pairs[H.PAIR_ONE][0]), len(refs.pairs[H.PAIR_ONE][1])) == (1, 1) and int(run_all[H.PAIR_ONE]["status"]) == 0
    assert (len(refs.pairs[H.PAIR_STRIPS][0]), len(refs.pairs[H.PAIR_STRIPS][1])) == (300, 520) and 520 > CH.STRIP_ROWS
    assert int(run_all[H.PAIR_EMPTY]["status"]) == _ffi.ERR_EMPTY_SEQUENCE
    assert int(run_all[H.PAIR_BAD]["status"]) == _ffi.ERR_CODE_OUT_OF_RANGE
    assert int(run_all[H.PAIR_NOPOS]["status"]) == _ffi.ERR_NO_POSITIVE_CELL
    assert sum(int(r["status"]) != 0 for r in run_all.values()) == 3
    # the 4 x 4 run's subset is the pairs whose codes are all below 4
    small = [p for p in H.ALL if all(len(s) and int(s.max()) < 4 for s in refs.pairs[p])]
    assert sorted(small) == sorted(H.DNA_SUBSET) and H.SCHEMES["N"][3] != H.SCHEMES["L"][3]
    # run_chunked is cut into three chunks or more
    assert H.planned_chunks(refs.q_len, refs.t_len, H.CHUNK_CELLS) >= 3
    # the column count restated here is the oracle's (an alignment with gaps and mismatches: the orientation shows)
    _res, qa, ta = refs.aln(H.PAIR_STRIPS, "L", ("P", 0))
    c = np.array(H.count_columns(qa, ta, 24, 24, 98)).reshape(24, 24)
    assert (c != c.T).any() and (c == orc.frequency_matrix(qa, ta, 24)).all() and (qa == 98).any() and (ta == 98).any()
    # heur_b's pair has no root, every other pair of both sets has one
    for name in ("a", "b"):
        st = [refs.matrix(p, ("T", name, "B62"))[0] for p in H.ALL]
        assert st == [1 if (name == "b" and p == H.NO_ROOT_PAIR) else 0 for p in H.ALL]


def test_the_chunk_rule_restated_is_the_library_s(refs):
    """the restated cut against aln_plan_chunks (host arithmetic, no GPU) under the same forced target"""
    import ctypes as C
    from aligner_amd import _ffi
    from aligner_amd import build as native_build
    native_build.build()
    p = _ffi.Params(H.CORE_LOCAL, 0, 11.0, 2.0, None, 24, 24, 24, 3, 98, 0, 0, 0, 0)
    ql, tl = refs.q_len.astype(np.uint64), refs.t_len.astype(np.uint64)
    for target in (H.CHUNK_CELLS, 10000, 150000, 10 ** 7):
        with CH.knobs({"ALN_CHUNK_CELLS": str(target)}):
            got = int(_ffi.load().aln_plan_chunks(C.byref(p), ql.ctypes.data, tl.ctypes.data, len(ql), 1, None, None, 0))
        assert got == H.planned_chunks(refs.q_len, refs.t_len, target), target


def test_the_walk_passes_over_the_references(refs, plan):
    out = H.walk(H.FakeBackend(refs), plan, refs.memo)
    assert out["failures"] == [], out["failures"][:3]
    assert out["calls"] == len(plan) + sum(len(x["obs"]) for x in plan) and all(v >= 1 for v in out["refusals"].values())
    assert len(out["log"]) == len(plan) and None not in out["log"]


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_the_walker_catches_a_defect(refs, plan, defect):
    fake = H.FakeBackend(refs, defect)
    out = H.walk(fake, plan, refs.memo, stop_at_first=True)
    assert fake.first_effect is not None, "the schedule never meets the defect"
    assert len(out["failures"]) == 1, defect
    fail = out["failures"][0]
    print(defect, "first effect at step", fake.first_effect, "->", fail["message"][:160])
    assert fail["step"] >= fake.first_effect and "held=" in fail["message"]
    if defect in ("refused_call_writes", "chunked_differs", "strings_serves_previous_run", "heuristics_keeps_written"):
        assert fail["step"] == fake.first_effect              # (seen by the call itself or by the observation behind it)


def test_plan_and_expected_values_survive_their_files(refs, plan, tmp_path):
    import json
    path = str(tmp_path / "expected.npz")
    CH.save_expected(path, refs.memo)
    again = CH.load_expected(path)
    plan2 = json.loads(json.dumps(plan))
    names = {x["name"] for x in plan if x["name"]} | {o["name"] for x in plan for o in x["obs"] if o["name"]}
    assert names <= set(again)
    for name in names:
        for key, v in refs.memo[name].items():
            assert np.array_equal(np.asarray(v), again[name][key]), (name, key)
    assert H.walk(H.FakeBackend(refs), plan2, again)["failures"] == []
