"""Seed chains in the call history of a resident sequence set: the chaining calls after and before every one of the 24 call kinds of
tests/set_history.py's CATALOGUE, on one handle of its 48-protein set.

Per kind E: the calls that put the handle where E is accepted; the chaining round; E, whose answer is held against the catalogue's
expected value (the CPU oracle and the rule restatements) exactly as the set-history walk holds it; the chaining round again.  A
chaining round is: `chains` over the list that is live, if one is (a prefilter's or the word join's: it must stay as it is), exact
against seedchain_ref; then a seed join, `chains` over it and `chain_filter`, exact against seedchain_ref -- list, diagonals, records
and summaries -- after which the list is dropped, so that the state model of set_history stays true.  Before `cand_hits` the round
leaves the prefilter's list alone, so that the pass runs on a list that a chaining call has just read.  So every kind runs directly
after a chaining call and every chaining call directly after every kind, and the held hits, the plans of both fills, the three other
indexes and the counter words are seen from both sides."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedchain_ref as R  # noqa: E402
import seedjoin_ref as SJ  # noqa: E402
import set_history as H  # noqa: E402
from aligner_amd.seqset import Candidates  # noqa: E402

pytestmark = pytest.mark.gpu
K, A = 3, 20
CHAIN = dict(max_gap=40, max_skew=6, gap_scale=4, max_occ=60)
MIN_SCORE, MIN_SPAN = 12, 10
# what makes a fresh state accept the kind
BEFORE = dict(pf1=["kmer2"], pf2=["kmer3"], word_join=["word5"], cand_hits=["kmer2", "pf1"], cigar_fill=["hits_small", "cigars"], msa_fill=["hits_small", "msa"])
BEFORE.update({c: ["hits_small"] for c in H.CONSUMERS})


def tuples(recs):
    return [tuple(int(x) for x in r) for r in recs]


@pytest.fixture(scope="module")
def refs(orc):
    return H.Refs(H.set_a(), H.set_b(), orc)


@pytest.fixture(scope="module")
def own(refs):
    """the chaining round's own list and what it must give, from the references alone"""
    seqs = refs.a
    lists, summary, _rows = SJ.seed_join(seqs, K, A, min_seeds=2, band=2, max_occ=CHAIN["max_occ"], block=H.BIG)
    recs, chain_summary = R.chains(seqs, K, A, list(zip(lists[1], lists[2])), **CHAIN)
    keep = [c for c, r in enumerate(recs) if R.keep(r, MIN_SCORE, MIN_SPAN)]
    assert 10 < len(keep) < len(recs) and chain_summary["with_anchor"] == len(recs)
    return dict(lists=[list(x) for x in lists], summary=summary, recs=recs, chain_summary=chain_summary, keep=keep)


def chaining_round(ss, seqs, own, live, replace=True):
    """live: (count, q, t) of the list the model says is there, or None"""
    if live is not None:
        count, q, t = live
        cand = Candidates(ss, count)
        assert cand.q.tolist() == q and cand.t.tolist() == t
        want, _summary = R.chains(seqs, K, A, list(zip(q, t)), **CHAIN)
        assert tuples(cand.chains(k=K, alphabet_size=A, **CHAIN)) == want
        again = Candidates(ss, count)                      # chains changed nothing
        assert again.index.tolist() == cand.index.tolist() and again.shared.tolist() == cand.shared.tolist()
    if not replace:
        return
    cand = ss.seed_join(K, A, min_seeds=2, band=2, max_occ=CHAIN["max_occ"])           # (the whole upper triangle: H.BIG)
    assert [cand.index.tolist(), cand.q.tolist(), cand.t.tolist(), cand.shared.tolist(), cand.diag.tolist()] == own["lists"] and cand.summary == own["summary"]
    assert tuples(cand.chains(**CHAIN)) == own["recs"]
    assert {k: v for k, v in cand.chain_summary.items() if k != "chunks"} == own["chain_summary"]
    kept = cand.chain_filter(MIN_SCORE, MIN_SPAN, **CHAIN)
    keep = own["keep"]
    for got, was in zip((kept.index, kept.q, kept.t, kept.shared, kept.diag), own["lists"]):
        assert got.tolist() == [was[c] for c in keep]
    assert tuples(kept.chain) == [own["recs"][c] for c in keep]
    assert {k: v for k, v in kept.summary.items() if k != "chunks"} == own["chain_summary"]
    ss.seed_index(K, A)                                    # drops the list: the model's `cand` is None again


def test_chaining_after_and_before_every_catalogued_kind(refs, own):
    backend = H.GpuBackend(refs.a, refs.recs_b)
    try:
        ss = backend.sets["A"]
        assert H.BIG == H.upper(0, len(ss)) and len(H.CATALOGUE) == 24
        model = H.Model("A")
        live = [None]
        seen_accepted = set()

        def call(entry):
            want, kind, args = model.step(entry)
            got = backend.call("A", entry, refs.get(args))
            diff = H.check(got, refs.get(want) if want else None)
            assert diff is None, "%s: %s [%s]" % (entry, diff, model.s.text())
            if entry in H.KMERS or entry == "word5":
                live[0] = None
            if entry in H.LISTS and kind is None:
                live[0] = (int(got["count"]), got["q"].tolist(), got["t"].tolist())
            return kind

        def round_(replace=True):
            chaining_round(ss, refs.a, own, live[0], replace)
            if replace:
                live[0], model.s.cand = None, None

        ss.seed_index(K, A)
        round_()
        for entry in H.CATALOGUE:
            for pre in BEFORE.get(entry, []):
                assert call(pre) is None
            round_(replace=entry != "cand_hits")
            if call(entry) is None:
                seen_accepted.add(entry)
            round_()
        assert seen_accepted == set(H.CATALOGUE)           # no kind was only ever refused
    finally:
        backend.close()
