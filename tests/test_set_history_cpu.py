"""The sequence-set call-history test without a GPU (helpers: tests/set_history.py): the schedule over the catalogue, the conditions the
two sets are built for -- asserted from the oracle and the rule restatements alone -- and the walker itself, which must pass over a
backend that answers from the references and must catch each of five planted defects at the first transition that can show it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import call_history as CH  # noqa: E402
import cigar_ref  # noqa: E402
import set_history as H  # noqa: E402


@pytest.fixture(scope="module")
def refs(orc):
    r = H.Refs(H.set_a(), H.set_b(), orc)
    for name in H.needed():
        r.get(name)
    return r


def test_the_schedule_holds_every_transition_once():
    k = len(H.CATALOGUE)
    seq = H.rotated_schedule()
    assert 16 <= k <= 24 and len(seq) == k * k + 1 and len(set(H.CATALOGUE)) == k
    pairs = list(zip(seq[:-1], seq[1:]))
    assert len(set(pairs)) == k * k == len(pairs) and CH.transitions(seq) == {(a, b) for a in range(k) for b in range(k)}
    assert H.CATALOGUE[seq[0]] in H.PRODUCERS
    assert set(H.B_ROTATION) == set(H.B_CATALOGUE)
    # the counter word the prefilter and the filter share is written in both orders
    names = [(H.CATALOGUE[a], H.CATALOGUE[b]) for a, b in pairs]
    assert ("pf1", "filter") in names and ("filter", "pf1") in names and ("pf2", "filter") in names and ("filter", "pf2") in names


def test_the_sets_are_what_they_are_built_for(refs):
    a = refs.a
    lens = sorted(len(s) for s in a)
    assert len(a) == H.N_A == 48 and set(H.SPECIAL) <= set(lens) and all(30 <= n <= 200 for n in lens if n not in H.SPECIAL)
    held = {p: refs.held(p) for p in ("hits_large", "hits_small", "best3", "hits_global")}
    held.update({"cand_hits:" + c: refs.held("cand_hits:" + c) for c in ("pf1", "pf2", "wj")})
    sizes = {p: len(h) for p, h in held.items()}
    assert sizes["hits_large"] > 512, sizes                      # more than two 256-hit scan tiles
    assert 1 <= sizes["hits_small"] <= 8, sizes
    assert max(sizes.values()) >= 8 * min(sizes.values()) and min(sizes.values()) >= 1, sizes
    lists = [(h.index.tobytes(), h.q.tobytes(), h.t.tobytes()) for h in held.values()]
    assert len(set(lists)) == len(lists), "no two held passes are equal"
    assert 0 in H.block_nodes(H.PRODUCERS["hits_global"]["block"]) and len(a[0]) == 0
    # the cluster model: families
    comp = refs.get("cluster_components@hits_large")
    assert int(comp["summary.clusters"]) >= 3 and int(comp["records"][:, 1].max()) >= 4
    small = refs.get("cluster_components@hits_small")
    assert int(small["records"][:, 1].max()) >= 2
    assert any(int(refs.get("msa@" + p)["records"][:, 3].sum()) > 0 for p in held), "an MSA with insert columns"
    ops = set(int(w) & 15 for w in refs.get("cigars@hits_large")["words"])
    assert {cigar_ref.I, cigar_ref.D, cigar_ref.EQ, cigar_ref.X, cigar_ref.S} <= ops
    # the candidate lists
    got = {}
    for entry in ("pf1", "pf2", "word_join"):
        want = refs.get(entry + "@-")
        block = H.PREFILTERS[entry]["block"] if entry in H.PREFILTERS else H.WORDJOIN["block"]
        assert 0 < int(want["count"]) < len(H.block_pairs(block)), entry
        got[entry] = (want["q"].tobytes(), want["t"].tobytes())
    assert len(set(got.values())) == 3
    assert 4 ** 0 and 20 ** H.WORD_K > 2 ** 18
    assert not np.array_equal(refs.get("kmer2@-")["n_words"], refs.get("kmer3@-")["n_words"])
    # B: hits on both strands
    b = refs.held("b_hits")
    n = len(refs.recs_b)
    assert any(t >= n for t in b.t.tolist()) and any(t < n for t in b.t.tolist()) and len(b) >= 3
    assert not np.array_equal(refs.get("b_scig@-")["words"], refs.get("b_pcig@-")["words"])


def test_the_walk_meets_every_refusal_and_every_consumer_after_every_producer():
    plan = H.dry_run()
    k = len(H.CATALOGUE)
    assert len(plan) == 2 * (k * k + 1)
    kinds = dict.fromkeys(H.KINDS, 0)
    for _i, _w, _p, _e, _want, kind, _a, _b in plan:
        if kind:
            kinds[kind] += 1
    assert all(v >= 3 for v in kinds.values()), kinds
    accepted = {(want.split("@")[1].split(":")[0], entry) for _i, which, _p, entry, want, _k, _a, _b in plan
                if which == "A" and want and entry in H.CONSUMERS + H.FILLS}
    for producer in H.PRODUCERS:
        for consumer in H.CONSUMERS:
            assert (producer, consumer) in accepted, (producer, consumer)
    assert any(e == "cigar_fill" for _p, e in accepted) and any(e == "msa_fill" for _p, e in accepted)
    # both chunk counts of the chunked walk, from the plan rule
    lens = [len(s) for s in H.set_a()]
    assert H.planned_chunks(lens, H.BIG, H.CHUNK_CELLS) >= 3


def test_the_walk_passes_over_the_references(refs):
    out = H.walk(H.FakeBackend(refs), refs)
    assert out["failures"] == [] and out["calls"] == 2 * (len(H.CATALOGUE) ** 2 + 1)
    assert all(v >= 3 for v in out["refusals"].values()), out["refusals"]


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_the_walker_catches_a_defect_at_its_first_transition(refs, defect):
    fake = H.FakeBackend(refs, defect)
    out = H.walk(fake, refs, stop_at_first=True)
    assert len(out["failures"]) == 1, defect
    fail = out["failures"][0]
    assert fake.first_effect is not None and fail["step"] == fake.first_effect, (defect, fail, fake.first_effect)
    assert "%s -> %s" % (fail["prev"], fail["entry"]) in fail["message"] and "held=" in fail["message"]
    where = {"tail": H.PRODUCERS, "count": ("filter",), "stale_fill": ("cigar_fill",), "old_index": ("pf1", "pf2"), "leak": ("b_sfill",)}[defect]
    assert fail["entry"] in where and fail["which"] == ("B" if defect == "leak" else "A")


def test_expected_values_survive_the_file(refs, tmp_path):
    path = str(tmp_path / "expected.npz")
    refs.save(path)
    again = H.Refs(H.set_a(), H.set_b()).load(path)
    assert sorted(again.memo) == sorted(refs.memo)
    for name, want in refs.memo.items():
        assert sorted(want) == sorted(again.memo[name])
        for key, v in want.items():
            assert np.array_equal(np.asarray(v), again.memo[name][key]), (name, key)
    assert H.walk(H.FakeBackend(again), again)["failures"] == []
