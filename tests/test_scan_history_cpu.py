"""The window-scan call-history test without a GPU (helpers: tests/scan_history.py): the schedule over the catalogue, the conditions the
chromosome and the catalogue are built for -- asserted from the oracle alone --, the plan keys that must overflow the cache of 8, and the
walker itself, which must pass over a fake scan that answers from the oracle and must catch each of four planted faults at the call
that commits it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as CH  # noqa: E402
import scan_history as H  # noqa: E402


@pytest.fixture(scope="module")
def refs(orc):
    return H.Refs(orc)


@pytest.fixture(scope="module")
def plan(refs):
    return H.dry_run(refs)


def test_the_schedule_holds_every_ordered_pair_of_entries_once():
    k = len(H.CATALOGUE)
    seq = CH.schedule(k)
    pairs = list(zip(seq[:-1], seq[1:]))
    assert 18 <= k <= 24 and len(seq) == k * k + 1
    assert len(set(pairs)) == k * k == len(pairs) and CH.transitions(seq) == {(a, b) for a in range(k) for b in range(k)}
    names = H.the_schedule()
    assert CH.transitions(names) == {(a, b) for a in H.CATALOGUE for b in H.CATALOGUE}


def test_the_model_predicts_every_kind_of_refusal(plan):
    kinds = {kd: sum(1 for x in plan if x["kind"] == kd) for kd in H.KINDS}
    held_after = sum(1 for x in plan if x["obs"][0]["entry"] == "obs_list")
    print("calls %d, with observations %d, refused %s, calls after which hits are held %d" % (len(plan), H.expected_calls(plan), kinds, held_after))
    assert all(v >= 1 for v in kinds.values()), kinds
    # a fetch meets both states often: held hits after about half the calls
    assert 3 * held_after >= len(plan) and 3 * (len(plan) - held_after) >= len(plan)
    # every fetch is answered after every held pass, and refused after every other pass
    direct = {(a["entry"], b["entry"]): b["kind"] for a, b in zip(plan[:-1], plan[1:])}
    for p, (call, _k, _g, _r, _rule, _cap) in H.PASSES.items():
        for f in H.FETCHES:
            want = "keep_beyond" if f == "keep_beyond" and call == "hits" else None if call == "hits" else "no_held"
            assert direct[(p, f)] == want, (p, f, direct[(p, f)])
    # a refused pass directly after a held pass, with the hits observed behind it; and a fetch behind that
    for r in H.REFUSED:
        assert any(a["entry"] in H.PASSES and H.PASSES[a["entry"]][0] == "hits" and b["entry"] == r and b["obs"][0]["entry"] == "obs_list"
                   for a, b in zip(plan[:-1], plan[1:]))
    # the other scan's pass between a held pass and a fetch
    assert any(b["entry"] == "other_hits" and b["obs"][0]["entry"] == "obs_list" and c["entry"] in H.FETCHES and c["kind"] is None
               for b, c in zip(plan[:-1], plan[1:]))
    # a reverse pass is the first pass on the reversed strand in some walk: the first reverse pass of this one follows forward passes
    first_rev = next(i for i, x in enumerate(plan) if x["entry"] in H.PASSES and H.PASSES[x["entry"]][3])
    assert any(x["entry"] in H.PASSES for x in plan[:first_rev]), first_rev


def test_the_catalogue_meets_its_own_conditions(refs):
    assert refs.length == H.LEN == 3001 and all(H.LEN % d for d in range(2, 55))
    assert len(refs.chroms[0]) == len(refs.chroms[1]) and (refs.chroms[0] != refs.chroms[1]).any()
    for name, (call, kind, gname, reverse, rule, cap) in H.PASSES.items():
        a = refs.args(name)
        recs = refs.aligned(kind, gname, reverse, 0)
        assert len(recs) == a["n"] and all(r["status"] == 0 for r in recs), name
        if call == "score":
            continue
        hits = len(refs.hit_idx(name))
        print(name, "windows", a["n"], "hits", hits)
        if name in H.SOME_HITS:
            assert 0 < hits < a["n"], (name, hits)
        elif name in H.EVERY_HIT:
            assert hits == a["n"] > 0, (name, hits)
        else:
            assert name in H.NO_HIT and hits == 0, (name, hits)
        assert hits <= 430
    assert len(refs.hit_idx("select_cap")) > refs.args("select_cap")["cap"] == 3
    assert refs.args("hits_no_window")["n"] == 0 and refs.args("hits_none")["n"] > 0
    a = refs.args("hits_few_fwd")
    assert a["n"] == 4 and H.window_lengths(H.LEN, a["first"], a["step"], a["width"], np.arange(4)).tolist() == [100, 70, 40, 10]
    a = refs.args("hits_two_strip")
    lengths = H.window_lengths(H.LEN, a["first"], a["step"], a["width"], np.arange(a["n"]))
    assert a["n"] == 12 and lengths.max() >= CH.STRIP_ROWS + 1 and lengths.min() < a["width"]
    # windows shorter than the PWM, and a truncated tail among the hits of the pass that every window passes
    a = refs.args("hits_all")
    assert a["width"] < a["W"] and refs.hit_lengths("hits_all")[-1] < a["width"]
    # sd = 0: the rule is the division's (inf passes, NaN and -inf fail)
    f, a = refs.f("select_sd0"), refs.args("select_sd0")
    assert a["sd"] == 0.0 and refs.hit_idx("select_sd0").tolist() == np.flatnonzero(f > a["mean"]).tolist() and (f == a["mean"]).any()
    # the strand matters: a reverse pass differs from the forward pass of the same PWM and geometry
    assert (refs.f("hits_few_fwd") != refs.f("hits_few_rev")).any()
    assert (refs.f("hits_all") != np.array([r["f"] for r in refs.aligned("int", "g50", 0, 0)])).any()
    # and so do the residues: the other scan's answers are not the first scan's
    assert (refs.f(H.OTHER_PASS, 0) != refs.f(H.OTHER_PASS, 1)).any() and len(refs.hit_idx(H.OTHER_PASS, 1)) > 0
    # the other scan's pass uses plan keys the first scan uses as well
    assert H.PASSES[H.OTHER_PASS][2] == "g50" and H.OTHER_PASS in H.CATALOGUE
    # a fetch's lists: a position listed twice, not in ascending order, an inner range
    for count in (5, 40, 429):
        keep = H.fetch_args("freq_subset", count)["keep"]
        assert len(set(keep)) == len(keep) - 1 and sorted(keep) != keep and max(keep) < count
        keep = H.fetch_args("strings_subset", count)["keep"]
        assert sorted(keep) != keep and max(keep) < count
        inner = H.fetch_args("list_inner", count)
        assert 0 < inner["first"] and inner["first"] + inner["n"] < count


def test_the_catalogue_overflows_the_plan_cache(refs):
    keys = {k for name in H.PASSES for k in H.plan_keys(refs, name)}
    print("distinct plan keys:", len(keys))
    assert len(keys) >= 9                       # an LRU of 8: the walk must evict and plan again
    # two entries of equal key on different strands, and a few-window plan (host descriptors are kept) used on both strands
    assert H.plan_keys(refs, "hits_few_fwd") == H.plan_keys(refs, "hits_few_rev") and len(H.plan_keys(refs, "hits_few_fwd")) == 2
    assert H.plan_keys(refs, "hits_all")[0] == H.plan_keys(refs, "score_fwd_int")[0]
    assert H.plan_keys(refs, "hits_no_window") == [] and len(H.plan_keys(refs, "hits_none")) == 1


def fake(refs, fault=None):
    abi = H.FakeAbi(refs.chroms, fault)
    return abi, H.Backend(abi)


def test_the_walk_passes_over_the_oracle_scan(refs, plan):
    _abi, backend = fake(refs)
    out = H.walk(backend, plan, refs.memo)
    assert out["failures"] == [], [f["message"] for f in out["failures"][:3]]
    assert out["calls"] == H.expected_calls(plan) and all(v >= 1 for v in out["refusals"].values())
    assert CH.transitions(out["entries"]) == {(a, b) for a in H.CATALOGUE for b in H.CATALOGUE}


@pytest.mark.parametrize("fault", H.FAULTS)
def test_the_walker_catches_a_planted_fault_at_the_culprit_call(refs, plan, fault):
    abi, backend = fake(refs, fault)
    out = H.walk(backend, plan, refs.memo, stop_at_first=True)
    assert abi.first_effect is not None, "the schedule never meets the fault"
    assert len(out["failures"]) == 1, fault
    fail = out["failures"][0]
    print(fault, "first effect at step", abi.first_effect, "->", fail["message"][:200])
    assert fail["step"] == abi.first_effect and "held=" in fail["message"]
    culprit = {"score_keeps_held": ("score_fwd_int", "score_rev_real"), "select_keeps_held": ("select_rev", "select_cap", "select_none", "select_sd0"),
               "refused_pass_drops_held": tuple(H.REFUSED),
               "strings_ignore_keep_order": ("strings_subset",)}[fault]
    assert fail["entry"] in culprit


def test_a_scan_that_answers_what_it_must_refuse_is_reported_to_the_end_of_the_walk(refs, plan):
    """the whole walk over a scan whose held hits survive a select pass: every fetch it answers where it must refuse -- from a held pass of
    any PWM width and window width of the catalogue -- finds room in the buffers and is reported; the walker neither stops nor breaks"""
    abi, backend = fake(refs, "select_keeps_held")
    out = H.walk(backend, plan, refs.memo)
    assert out["calls"] == H.expected_calls(plan)
    answered = [f for f in out["failures"] if f["observed"] in H.FETCHES and "want the refusal" in f["message"]]
    print("failures", len(out["failures"]), "fetches answered that must be refused", len(answered))
    assert len(answered) >= 4 and {f["observed"] for f in answered} >= {"freq_subset", "strings_subset", "list_all"}
    assert max(g[0] for g in H.GEOMS.values()) == H.MAX_W and max(g[6] for g in H.GEOMS.values()) == H.MAX_WIDTH


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
    _abi, backend = fake(refs)
    assert H.walk(backend, plan2, again)["failures"] == []


def test_the_wrap_job_has_three_references_and_wraps_the_salt(orc):
    args, wants = H.wrap_args(orc)
    assert len(args) == 3 and len(wants) == 6
    assert len({wants["score-%d" % k]["f"].tobytes() for k in range(3)}) == 3
    launches = 0
    for n in range(H.WRAP_PASSES):
        launches += 1 if n % 2 == 0 else (2 if int(wants["hits-%d" % (n % 3)]["count"]) else 1)
    assert all(0 < int(wants["hits-%d" % k]["count"]) < args[k]["n"] for k in range(3))
    assert H.WRAP_PASSES >= 1100 and launches > 1024 + 50 and 1024 % 3 and {(n % 3, n % 2) for n in range(6)} == {(k, c) for k in range(3) for c in range(2)}
