"""Seed chains on the GPU (aln_seqset_candidate_chains / _chain_filter / _chain_records): every record, every filtered list and every
PAF line exact against seedchain_ref.py.  Predecessor windows at the lane stride and its tail, the expand rounds at 63, 64 and 65 window
starts, runs separated by exactly the skew and the gap and by one more, the end tie, max_occ at its threshold, homopolymers at the
default max_pair_seeds and one past it, lists of the other two routes against a seed index of another k, chunks, the filter with the
candidate passes on top, both strands, the refusals, the C99 caller, call history and the command.

Sets hold a handful of records of at most a few hundred residues."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedchain_ref as R                                                       # noqa: E402
import seedjoin_ref as SJ                                                       # noqa: E402
from aligner_amd import _ffi                                                    # noqa: E402
from aligner_amd import build as native_build                                   # noqa: E402
from aligner_amd.enums import DNA                                               # noqa: E402
from aligner_amd.matrices import nucleotide_matrix                              # noqa: E402
from aligner_amd.seqset import CHAIN_RECORD, SeqSet, both, rectangle, upper    # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _ffi.ERR_INVALID_ARGUMENT


def rnd(rng, n, a=4):
    return rng.integers(0, a, n).astype(np.uint8)


def want_records(seqs, k, a, cand, **kw):
    recs, summary = R.chains(seqs, k, a, list(zip(cand.q.tolist(), cand.t.tolist())), **kw)
    return recs, summary


def check(cand, seqs, k, a, chunk_anchors=0, named=False, **kw):
    """one chaining call held against the reference, record for record; returns the reference's tuples"""
    extra = dict(k=k, alphabet_size=a) if named else {}
    got = cand.chains(chunk_anchors=chunk_anchors, **kw, **extra)
    want, summary = want_records(seqs, k, a, cand, **kw)
    assert got.dtype == CHAIN_RECORD and len(got) == len(cand)
    assert [tuple(int(x) for x in r) for r in got] == want
    per = [0 if r[7] else r[6] for r in want]
    chunks = R.cut(per, chunk_anchors or R.CHUNK_ANCHORS)
    assert cand.chain_summary == dict(summary, chunks=len(chunks))
    return want


# ---------------------------------------------------------------- predecessor windows and expand rounds
def test_predecessor_windows_at_the_lane_stride_and_its_tail():
    """k = 1: a query of N ones and a two sees the target `1 2` with N anchors (i, 0) and one more, (N, 1), whose window is all N"""
    sizes = (63, 64, 65, 129, 1)
    seqs = [np.array([1] * n + [2], dtype=np.uint8) for n in sizes] + [np.array([1, 2], dtype=np.uint8), np.array([2, 2, 2], dtype=np.uint8)]
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(1, 4, block=rectangle(0, len(sizes), len(sizes), 2))
        want = check(cand, seqs, 1, 4, max_gap=1000, max_skew=1000, gap_scale=0)
        by_pair = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), want))
        for i, n in enumerate(sizes):
            # the last anchor takes the nearest one before it: (n - 1, 0), a chain of two that starts there
            assert by_pair[(i, len(sizes))] == (2, 2, n - 1, n + 1, 0, 2, n + 1, 0)
            assert by_pair[(i, len(sizes) + 1)] == (1, 1, n, n + 1, 0, 1, 3, 0)        # every window empty: pq is the same throughout
        # a drift that costs: the cheapest predecessor of each is still found among all 129
        check(cand, seqs, 1, 4, max_gap=1000, max_skew=1000, gap_scale=255)
        check(cand, seqs, 1, 4, max_gap=64, max_skew=64, gap_scale=1)


def test_expand_rounds_at_63_64_and_65_window_starts():
    rng = np.random.default_rng(2)
    k = 8
    base = rnd(rng, k + 64)
    seqs = [base[:k + 62].copy(), base[:k + 63].copy(), base.copy(), base.copy(), np.concatenate([base[:30], rnd(rng, 3), base[30:]]), np.tile(base[:k + 2], 9)]
    with SeqSet(seqs, DNA) as ss:
        for block in (upper(0, len(seqs)), rectangle(0, len(seqs), 0, len(seqs))):
            cand = ss.seed_join(k, 4, block=block)
            want = check(cand, seqs, k, 4)
            check(cand, seqs, k, 4, max_gap=20, max_skew=2, gap_scale=16)
        assert max(r[6] for r in want) > 64 and (k + 64, 65, 0, k + 64, 0, k + 64, 65, 0) in want


# ---------------------------------------------------------------- chain structure
def test_runs_separated_by_the_skew_the_gap_and_one_more():
    rng = np.random.default_rng(3)
    k, B, G = 8, 5, 30
    r1, r2 = rnd(rng, 40), rnd(rng, 40)
    q = np.concatenate([r1, r2])
    seqs = [q, np.concatenate([r1, rnd(rng, B), r2]), np.concatenate([r1, rnd(rng, B + 1), r2])]
    # a run 8 + gap behind the other on both records: G and G + 1
    x, y = rnd(rng, G - 7), rnd(rng, G - 7)
    y[::3] = (x[::3] + 1) % 4
    seqs += [np.concatenate([r1, x[:G - 8], r2]), np.concatenate([r1, y[:G - 8], r2]), np.concatenate([r1, x, r2]), np.concatenate([r1, y, r2])]
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(k, 4)
        want = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), check(cand, seqs, k, 4, max_gap=1000, max_skew=B, gap_scale=0)))
        assert want[(0, 1)][1] == 66 and want[(0, 1)][2:6] == (0, 80, 0, 80 + B)          # one chain across the insertion
        assert want[(0, 2)][1] == 33 and want[(0, 2)][2:6] == (0, 40, 0, 40)              # two: the first of equals
        want = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), check(cand, seqs, k, 4, max_gap=G, max_skew=0, gap_scale=0)))
        assert want[(3, 4)][1] > 33 and want[(3, 4)][3] == 80 + G - 8
        assert want[(5, 6)][1] <= 34 and want[(5, 6)][3] < 80


def test_two_equal_chains_and_the_end_tie():
    rng = np.random.default_rng(4)
    k = 6
    r = rnd(rng, 30)
    seqs = [r, np.concatenate([rnd(rng, 11), r, rnd(rng, 50), r, rnd(rng, 7)]), np.concatenate([r, r])]
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(k, 4, block=rectangle(0, 3, 0, 3))
        want = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), check(cand, seqs, k, 4, max_gap=100, max_skew=0, gap_scale=0)))
        assert want[(0, 1)][:6] == (30, 25, 0, 30, 11, 41)                                # both copies score 30: the one at the least pt
        assert want[(2, 0)][:6] == (30, 25, 0, 30, 0, 30)                                 # ... at the least pq
        check(cand, seqs, k, 4, max_gap=100, max_skew=100, gap_scale=1)


def test_max_occ_at_its_threshold():
    rng = np.random.default_rng(5)
    k = 8
    r, s = rnd(rng, 20), rnd(rng, 30)
    seqs = [np.concatenate([r, s]), np.concatenate([s, r]), r.copy(), rnd(rng, 25)]       # r's words occur 3 times, s's twice
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(k, 4)
        all_ = check(cand, seqs, k, 4, max_occ=0)
        assert check(cand, seqs, k, 4, max_occ=3) == all_
        two = check(cand, seqs, k, 4, max_occ=2)
        assert two != all_ and sum(x[6] for x in two) == 23 and [x for x in two if x[6]][0][:2] == (30, 23)
        assert all(x == (0,) * 8 for x in check(cand, seqs, k, 4, max_occ=1))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_homopolymers_at_the_default_max_pair_seeds(n):
    seqs = [np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)]
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(1, 4)
        assert len(cand) == 1 and int(cand.shared[0]) == n
        got = [tuple(int(x) for x in r) for r in cand.chains(max_gap=8)]
        if n == 257:
            assert got == [(0, 0, 0, 0, 0, 0, n * n, R.OVERFLOW)] == R.chains(seqs, 1, 4, [(0, 1)], max_gap=8)[0]
            for min_score, min_span in ((0, 0), (2 ** 31 - 1, 2 ** 32 - 1)):
                kept = ss.seed_join(1, 4).chain_filter(min_score, min_span, max_gap=8)
                assert len(kept) == 1 and tuple(int(x) for x in kept.chain[0]) == got[0] and kept.summary["overflowed"] == 1
        else:
            assert n * n <= R.PAIR_SEEDS and got == R.chains(seqs, 1, 4, [(0, 1)], max_gap=8)[0]
            assert got == [(n, n, 0, n, 0, n, n * n, 0)]                                  # the main diagonal, a point a step
            assert cand.chain_summary == dict(anchors=n * n, with_anchor=1, overflowed=0, chunks=1)


# ---------------------------------------------------------------- lists of the other routes, chunks
def family(seed=6, k=8):
    rng = np.random.default_rng(seed)
    parent = rnd(rng, 160)
    seqs = []
    for m in range(6):
        s = parent[rng.integers(0, 40):160 - rng.integers(0, 40)].copy()
        flip = rng.random(len(s)) < 0.05
        s[flip] = rnd(rng, int(flip.sum()))
        if m % 2:
            cut = int(rng.integers(20, len(s) - 20))
            s = np.concatenate([s[:cut], rnd(rng, 4), s[cut:]])
        seqs.append(s)
    seqs += [rnd(rng, 90), np.zeros(0, dtype=np.uint8), parent[:k - 1].copy(), np.tile(parent[:k + 3], 7)]
    return seqs


def test_prefilter_and_word_join_lists_against_a_seed_index_of_another_k():
    seqs = family()
    with SeqSet(seqs, DNA) as ss:
        ss.seed_index(8, 4)
        for make in (lambda: ss.prefilter(3, 4, min_shared=0), lambda: ss.word_join(3, 4, min_shared=2)):
            cand = make()                                                                 # (each replaces the list before it)
            want = check(cand, seqs, 8, 4, named=True)
            assert sum(1 for r in want if r[6] == 0) > 3 and sum(1 for r in want if r[1] > 5) > 5
            with pytest.raises(TypeError):
                cand.chains()
            with pytest.raises(ValueError):
                cand.chains(k=7, alphabet_size=4)                                         # another index would drop this list
            assert ss.lib.aln_seqset_candidate_diags(ss.handle, 0, 1, np.zeros(1, dtype=np.int32).ctypes.data) == INV


def test_chunks_of_one_two_and_many_give_the_same_records():
    seqs = family(7)
    with SeqSet(seqs, DNA) as ss:
        cand = ss.seed_join(8, 4, block=rectangle(0, len(seqs), 0, len(seqs)))
        want = check(cand, seqs, 8, 4)
        per = [r[6] for r in want]
        total, most = sum(per), max(per)
        seen = set()
        for chunk in (total, (total + 1) // 2 + most, most, most + 1):
            assert check(cand, seqs, 8, 4, chunk_anchors=chunk, max_pair_seeds=most) == want
            seen.add(cand.chain_summary["chunks"])
        assert 1 in seen and 2 in seen and max(seen) > 4
        # one anchor fewer allowed per pair: the fullest pairs overflow, no chunk is short of room
        over = check(cand, seqs, 8, 4, chunk_anchors=most - 1, max_pair_seeds=most - 1)
        assert sum(1 for r in over if r[7]) >= 1


# ---------------------------------------------------------------- the filter
def test_the_filter_keeps_the_list_exact_and_the_passes_run_on_it():
    seqs = family(8)
    matrix = nucleotide_matrix()
    with SeqSet(seqs, DNA) as ss:
        block = rectangle(0, len(seqs), 0, len(seqs))
        cand = ss.seed_join(8, 4, block=block, band=3)
        full = [a.copy() for a in (cand.index, cand.q, cand.t, cand.shared, cand.diag)]
        want = check(cand, seqs, 8, 4)
        f_all, st_all = cand.score(matrix, 11.0, 2.0)
        held = cand.hits(matrix, 11.0, 2.0, 40.0)
        hits_all = dict(zip(held.index.tolist(), held.f.tolist()))
        min_score, min_span = 90, 80
        keep = np.array([R.keep(r, min_score, min_span) for r in want])
        assert 3 < keep.sum() < len(keep)
        kept = cand.chain_filter(min_score, min_span)
        for got, was in zip((kept.index, kept.q, kept.t, kept.shared, kept.diag), full):
            assert got.dtype == was.dtype and got.tolist() == was[keep].tolist()
        assert [tuple(int(x) for x in r) for r in kept.chain] == [r for r, k_ in zip(want, keep) if k_]
        assert kept.summary["with_anchor"] == sum(1 for r in want if r[6]) and kept.summary["anchors"] == sum(r[6] for r in want)
        # the resident list is the filtered one: the C calls and the passes see it
        again = type(kept)(ss, len(kept), diags=True, chain=True)
        assert again.index.tolist() == kept.index.tolist() and again.diag.tolist() == kept.diag.tolist() and (again.chain == kept.chain).all()
        f, st = kept.score(matrix, 11.0, 2.0)
        assert f.tobytes() == f_all[keep].tobytes() and st.tolist() == st_all[keep].tolist()
        held = kept.hits(matrix, 11.0, 2.0, 40.0)
        assert dict(zip(held.index.tolist(), held.f.tolist())) == {i: v for i, v in hits_all.items() if i in set(kept.index.tolist())}
        # the 2 best per query among the kept pairs, by the unfiltered list's scores: higher f first, equal f by the lower target
        best = kept.best(matrix, 11.0, 2.0, 2, skip_self=True)
        per_q = {}
        for i, q_, t_, v, ok in zip(full[0][keep].tolist(), full[1][keep].tolist(), full[2][keep].tolist(), f_all[keep].tolist(), st_all[keep].tolist()):
            if q_ != t_ and ok == _ffi.OK:
                per_q.setdefault(q_, []).append((-v, t_, i))
        want_best = sorted((q_, r, i, -v) for q_, rows in per_q.items() for r, (v, _t, i) in enumerate(sorted(rows)[:2]))
        assert sorted(zip(best.q.tolist(), best.rank.tolist(), best.index.tolist(), best.f.tolist())) == want_best and len(want_best) > 8
        # filtering the filtered list once more with the same thresholds keeps it all; a second filter is a filter too
        twice = kept.chain_filter(min_score, min_span)
        assert twice.index.tolist() == kept.index.tolist() and (twice.chain == kept.chain).all() and twice.diag.tolist() == kept.diag.tolist()
        none = twice.chain_filter(2 ** 31 - 1)
        assert len(none) == 0 and none.chain.shape == (0,) and none.diag.shape == (0,)
        # a word-join list: filtered, it still has no diagonals, and its records are there
        wj = ss.word_join(4, 4, min_shared=3, block=block)
        w_want = want_records(seqs, 8, 4, wj)[0]
        w_kept = wj.chain_filter(min_score, min_span, k=8, alphabet_size=4)
        w_keep = [R.keep(r, min_score, min_span) for r in w_want]
        assert w_kept.index.tolist() == wj.index[np.array(w_keep, dtype=bool)].tolist() and w_kept.diag is None
        assert [tuple(int(x) for x in r) for r in w_kept.chain] == [r for r, k_ in zip(w_want, w_keep) if k_]
        assert ss.lib.aln_seqset_candidate_diags(ss.handle, 0, 0, None) == INV


# ---------------------------------------------------------------- both strands
def test_a_reverse_complement_partner_in_the_mirrors_frame():
    rng = np.random.default_rng(9)
    a = rnd(rng, 150)
    comp = DNA.complement_map()
    piece = comp[a[40:120][::-1]]                                                        # the reverse complement of a[40:120]
    seqs = [a, np.concatenate([rnd(rng, 9), piece, rnd(rng, 14)]), rnd(rng, 70)]
    with SeqSet.stranded(seqs, DNA) as ss:
        resident = ss.residues()
        assert len(resident) == 6 and resident[4].tolist() == comp[seqs[1][::-1]].tolist()
        cand = ss.seed_join(10, 4, block=both(rectangle(0, 3, 0, 3), 3))
        want = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), check(cand, resident, 10, 4)))
        # record 0 against the mirror of record 1: a[40:120] lies at 14 .. 94 of the mirror
        # (three more residues happen to match behind it)
        assert want[(0, 4)][:6] == (83, 74, 40, 123, 14, 97)
        assert want[(1, 3)][:6] == (83, 74, 6, 89, 27, 110)


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_everything_as_it_was():
    seqs = family(10)
    with SeqSet(seqs, DNA) as ss:
        lib, h = ss.lib, ss.handle
        recs = np.full(64 * 32, 7, dtype=np.uint8)
        summ = _ffi.SeedchainSummary(5, 5, 5, 5)
        count = C.c_uint64(99)

        def spec(**kw):
            f = dict(k=8, alphabet=4, max_occ=0, max_gap=1000, max_skew=200, gap_scale=2, max_pair_seeds=0, chunk_anchors=0, flags=0, reserved=(0, 0, 0))
            f.update(kw)
            return _ffi.SeedchainSpec(f["k"], f["alphabet"], f["max_occ"], f["max_gap"], f["max_skew"], f["gap_scale"], f["max_pair_seeds"], f["chunk_anchors"],
                                      f["flags"], (C.c_uint32 * 3)(*f["reserved"]))

        def untouched():
            return count.value == 99 and bool((recs == 7).all()) and (summ.anchors, summ.with_anchor, summ.overflowed, summ.chunks) == (5, 5, 5, 5)

        def both_refuse(sp, n=1):
            assert lib.aln_seqset_candidate_chains(h, C.byref(sp), 0, n, recs.ctypes.data, C.byref(summ)) == INV and untouched()
            assert lib.aln_seqset_candidate_chain_filter(h, C.byref(sp), 0, 0, C.byref(summ), C.byref(count)) == INV and untouched()

        both_refuse(spec())                                                               # no seed index
        ss.seed_index(8, 4)
        both_refuse(spec())                                                               # no candidate list
        cand = ss.seed_join(8, 4)
        state = [x.copy() for x in (cand.index, cand.q, cand.t, cand.shared, cand.diag)]
        n = len(cand)
        assert 1 < n <= 64
        for sp in (spec(k=7), spec(alphabet=5), spec(k=17), spec(max_gap=0), spec(max_gap=2 ** 31), spec(max_skew=2 ** 31), spec(gap_scale=256),
                   spec(max_pair_seeds=2 ** 20 + 1), spec(chunk_anchors=2 ** 26 + 1), spec(flags=1), spec(reserved=(0, 0, 1)), spec(reserved=(1, 0, 0)),
                   # ALN_ERR_CAPACITY cannot be reached through a valid spec: a pair that is chained always fits a chunk
                   spec(chunk_anchors=2 ** 16 - 1), spec(max_pair_seeds=10, chunk_anchors=9)):
            both_refuse(sp)
        good = spec()
        assert lib.aln_seqset_candidate_chains(h, C.byref(good), 0, n + 1, recs.ctypes.data, None) == INV and untouched()
        assert lib.aln_seqset_candidate_chains(h, C.byref(good), n + 1, 0, recs.ctypes.data, None) == INV and untouched()
        assert lib.aln_seqset_candidate_chains(h, C.byref(good), 0, n, None, C.byref(summ)) == INV and untouched()
        assert lib.aln_seqset_candidate_chains(h, None, 0, n, recs.ctypes.data, None) == INV and untouched()
        assert lib.aln_seqset_candidate_chain_filter(h, C.byref(good), 0, 0, C.byref(summ), None) == INV and untouched()
        assert lib.aln_seqset_candidate_chain_records(h, 0, 1, recs.ctypes.data) == INV and untouched()      # no filter made this list
        # all of it is still there, and an empty range is no refusal
        assert lib.aln_seqset_candidate_chains(h, C.byref(good), n, 0, None, None) == _ffi.OK
        now = type(cand)(ss, n, diags=True)
        assert [x.tolist() for x in (now.index, now.q, now.t, now.shared, now.diag)] == [x.tolist() for x in state]
        kept = cand.chain_filter(0)
        assert len(kept) == n
        assert lib.aln_seqset_candidate_chain_records(h, 0, n + 1, recs.ctypes.data) == INV and untouched()
        assert lib.aln_seqset_candidate_chain_records(h, 0, n, None) == INV and untouched()
        assert lib.aln_seqset_candidate_chain_records(h, n, 0, None) == _ffi.OK
        # a new list has no records again
        ss.seed_join(8, 4)
        assert lib.aln_seqset_candidate_chain_records(h, 0, 1, recs.ctypes.data) == INV and untouched()


# ---------------------------------------------------------------- call history
def test_results_do_not_depend_on_what_the_handle_ran_before():
    seqs = family(11)
    matrix = nucleotide_matrix()
    block = rectangle(0, len(seqs), 0, len(seqs))

    def ask(ss):
        cand = ss.seed_join(8, 4, block=block, max_occ=9)
        recs = cand.chains(max_gap=60, max_skew=4, max_occ=9)
        kept = cand.chain_filter(30, 20, max_gap=60, max_skew=4, max_occ=9)
        return recs.tobytes(), kept.index.tolist(), kept.diag.tolist(), kept.chain.tobytes(), kept.summary

    with SeqSet(seqs, DNA) as ss:
        fresh = ask(ss)
    with SeqSet(seqs, DNA) as ss:
        ss.score(matrix, 11.0, 2.0)
        ss.hits(matrix, 11.0, 2.0, 30.0)
        ss.best(matrix, 11.0, 2.0, 3, block=block, skip_self=True)
        ss.prefilter(3, 4, min_shared=1).hits(matrix, 11.0, 2.0, 30.0)
        ss.word_join(5, 4).score(matrix, 11.0, 2.0)
        big = ss.seed_join(4, 4, block=block)
        big.chains(max_gap=5, max_skew=0, gap_scale=255, max_pair_seeds=50, chunk_anchors=64)
        big.chain_filter(10 ** 6, max_pair_seeds=50, chunk_anchors=64).best(matrix, 11.0, 2.0, 2)
        assert ask(ss) == fresh
        held = ss.hits(matrix, 11.0, 2.0, 30.0)
        held.cigars()
        assert ask(ss) == fresh and ask(ss) == fresh


# ---------------------------------------------------------------- the C99 caller and the command
def test_the_c99_caller():
    exe = native_build.build_seedchain_harness()
    seqs = family(12)
    k, G, B, g, min_score, min_span = 8, 80, 6, 3, 35, 25
    case = os.path.join(ROOT, "tests", "bin", "seedchain_case.txt")
    with open(case, "w") as fh:
        fh.write("%d\n%s\n%s\n%d 4 0 %d %d %d 0 0 %d %d\n" % (len(seqs), " ".join(str(len(s)) for s in seqs), " ".join(str(int(c)) for s in seqs for c in s),
                                                          k, G, B, g, min_score, min_span))
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    os.remove(case)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "guards ok" and all(l.endswith(" 0") for l in lines if l.startswith("rc "))
    (idx, qs, ts, seeds, diag), _summary, _rows = SJ.seed_join(seqs, k, 4)
    want, summary = R.chains(seqs, k, 4, list(zip(qs, ts)), max_gap=G, max_skew=B, gap_scale=g)
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("chain ")] == want
    chunks = len(R.cut([r[6] for r in want], R.CHUNK_ANCHORS))
    assert [l for l in lines if l.startswith("summary ")] == ["summary %d %d %d %d" % (summary["anchors"], summary["with_anchor"], summary["overflowed"], chunks)]
    keep = [c for c, r in enumerate(want) if R.keep(r, min_score, min_span)]
    assert 0 < len(keep) < len(want) and "kept %d" % len(keep) in lines
    assert [l for l in lines if l.startswith("cand ")] == ["cand %d %d %d %d %d" % (idx[c], qs[c], ts[c], seeds[c], diag[c]) for c in keep]
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("rec ")] == [want[c] for c in keep]


def test_the_command_end_to_end(tmp_path):
    rng = np.random.default_rng(13)
    parent = rnd(rng, 220)
    letters = "ACGT"
    reads = []
    for i in range(12):
        lo = int(rng.integers(0, 100))
        s = parent[lo:lo + int(rng.integers(80, 120))].copy() if i < 9 else rnd(rng, 100)
        if i in (3, 7):
            s = DNA.complement_map()[s[::-1]]
        reads.append(s)
    enc = DNA.str_to_vec(letters)
    back = {int(c): ch for c, ch in zip(enc, letters)}
    fa = tmp_path / "reads.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, "".join(back[int(c)] for c in s)) for i, s in enumerate(reads)))
    k, G, B, S, L = 9, 50, 3, 30, 25
    heads = ["r%d" % i for i in range(12)]
    for strands in (False, True):
        paf = tmp_path / ("chains%d.paf" % strands)
        cmd = [sys.executable, "-m", "aligner_amd.allpairs", "-i", str(fa), "--dna", "--kmer", str(k), "--seed-join", "--chain", "--max-gap", str(G), "--max-skew",
               str(B), "--min-chain-score", str(S), "--min-chain-span", str(L), "--chain-paf", str(paf)] + (["--both-strands"] if strands else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        resident = reads + ([DNA.complement_map()[s[::-1]] for s in reads] if strands else [])
        block = (0, 12, 0, 24, 0) if strands else (0, 12, 0, 12, 1)
        (idx, qs, ts, seeds, diag), _s, _r = SJ.seed_join(resident, k, 4, block=block)
        recs, _sum = R.chains(resident, k, 4, list(zip(qs, ts)), max_gap=G, max_skew=B)
        rows, lines = [], []
        for c, r in enumerate(recs):
            if not R.keep(r, S, L) or (strands and not qs[c] < ts[c] % 12):
                continue
            t = ts[c] % 12
            rows.append("%s,%s,%d,%d,%s" % (heads[qs[c]], ("%s,%s" % (heads[t], "-" if ts[c] >= 12 else "+")) if strands else heads[t], seeds[c], diag[c],
                                            ",".join(str(x) for x in r[:6])))
            lines.append(R.paf_line(heads[qs[c]], len(reads[qs[c]]), heads[t], len(reads[t]), r, k, minus=ts[c] >= 12))
        got = [l.split(",") for l in out.stdout.splitlines()]
        cut = 3 if strands else 2
        assert [",".join(g[:cut] + g[cut + 1:]) for g in got] == rows and len(rows) >= (8 if strands else 5)      # (the f column is the fill's business)
        assert paf.read_text().splitlines() == lines
        assert (not strands) or any("\t-\t" in l for l in lines)
