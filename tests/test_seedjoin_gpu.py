"""The positional word index and the seed join on the GPU (aln_seqset_seed_index / _seed_join / _candidate_diags): every list -- pair
numbers, q, t, seeds, diag -- and every summary exact against seedjoin_ref.py.  The band's edges on constructed records, seeds in
their tens of thousands across the compaction's tile edges, the edges of the word (k = 16 with the word 2^32 - 1, k = 7 of 20 codes),
max_occ at its threshold, every block shape, chunks and the cap, both strands, the candidate passes on top, agreement with the word
join where no word repeats, call history, the C99 caller, the refusals and the command.

Sets hold at most a few hundred records of at most about 600 residues."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seedjoin_ref as R                                                        # noqa: E402
import wordjoin_ref as W                                                        # noqa: E402
import strand_cases as K                                                        # noqa: E402
import test_prefilter_gpu as P                                                  # noqa: E402
import test_seqset_gpu as T                                                     # noqa: E402
from aligner_amd import _ffi                                                    # noqa: E402
from aligner_amd import build as native_build                                   # noqa: E402
from aligner_amd.enums import DNA                                               # noqa: E402
from aligner_amd.matrices import nucleotide_matrix                              # noqa: E402
from aligner_amd.seqset import Candidates, SeqSet, both, rectangle, upper      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_MIN = 30.0
TOP = 2 ** 31 - 1
NO = 98                                                                         # a code outside every alphabet here


def blk_tuple(b):
    return (int(b.q_first), int(b.q_count), int(b.t_first), int(b.t_count), int(b.upper))


def as_lists(cand):
    return cand.index.tolist(), cand.q.tolist(), cand.t.tolist(), cand.shared.tolist(), cand.diag.tolist()


def check(ss, seqs, k, a, block=None, **kw):
    """one join held against the reference, entry for entry, summary included; returns (the Candidates, the reference's row totals)"""
    b = upper(0, len(seqs)) if block is None else block
    cand = ss.seed_join(k, a, block=b, **kw)
    want, summary, rows = R.seed_join(seqs, k, a, block=blk_tuple(b), **kw)
    assert len(cand) == len(want[0])
    assert as_lists(cand) == tuple(list(x) for x in want)
    assert cand.summary == summary
    assert cand.diag.dtype == np.int32 and cand.shared.dtype == np.uint32
    return cand, rows


def marker(i):
    """four codes below 20 that no other marker has"""
    return [i // 8000 % 20, i // 400 % 20, i // 20 % 20, i % 20]


def placed(length, items):
    """a record of `length` codes that are no words at k = 4 but for marker i at position p, for every (i, p) of items"""
    s = np.full(length, NO, dtype=np.uint8)
    for i, p in items:
        assert (s[max(p - 1, 0):p + 5] == NO).all() and p + 4 <= length         # markers do not touch: no word spans two of them
        s[p:p + 4] = marker(i)
    return s


def families(a, n_fam, per_fam, seed, length=(60, 300), rate=0.04, k=8):
    """n_fam families of per_fam records -- a random parent and copies with substitutions at `rate`, some with a piece cut out -- and
    the records a join can stumble over"""
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n_fam):
        parent = rng.integers(0, a, rng.integers(length[0], length[1] + 1)).astype(np.uint8)
        for m in range(per_fam):
            s = parent.copy()
            flip = rng.random(len(s)) < rate
            s[flip] = rng.integers(0, a, int(flip.sum())).astype(np.uint8)
            if m % 3 == 2 and len(s) > 3 * k:
                cut = int(rng.integers(k, len(s) - k))
                s = np.concatenate([s[:cut], s[cut + 5:]])                      # a deletion: the seeds behind it sit five diagonals off
            seqs.append(s)
    first = seqs[0]
    seqs.append(np.zeros(0, dtype=np.uint8))                                    # empty
    seqs.append(first[:k - 1].copy())                                           # shorter than k
    seqs.append(first[:k].copy())                                               # one window
    outside = first.copy()
    outside[k - 1::k] = a                                                       # a code >= A inside every window
    seqs.append(outside)
    one_bad = first.copy()
    one_bad[len(one_bad) // 2] = NO                                             # ... inside k windows only
    seqs.append(one_bad)
    seqs.append(np.tile(first[:k + 3], 12))                                     # a tandem repeat: its words at many positions
    seqs.append(np.full(40, a - 1, dtype=np.uint8))                             # the largest word, 40 - k + 1 times
    seqs.append(np.full(k, a - 1, dtype=np.uint8))                              # ... and once
    seqs.append(seqs[1].copy())                                                 # a twin
    seqs.append(np.zeros(0, dtype=np.uint8))
    seqs.append(seqs[2][::-1].copy())
    return seqs


# ---------------------------------------------------------------- the band's edges
def band_records():
    """q and four targets whose seeds with q lie on chosen diagonals (k = 4, A = 20); q is 120 codes long, its markers at 0, 20, ..., 116"""
    q_pos = {0: 0, 1: 20, 2: 40, 3: 60, 4: 80, 5: 100, 6: 116}                  # marker 6 starts q's last window
    q = placed(120, list(q_pos.items()))
    # t1: diagonals 10, 10, 14, 15, 15, 15
    t1 = placed(140, [(0, 10), (1, 30), (2, 54), (3, 75), (4, 95), (5, 115)])
    # t2: equal counts in two windows: diagonals 0, 1 and 30, 31
    t2 = placed(140, [(0, 0), (1, 21), (3, 90), (4, 111)])
    # t3: negative diagonals -15, -14, -14, and q's last window against t's first: -(len_q - k) = -116
    t3 = placed(100, [(1, 5), (2, 26), (3, 46), (6, 0)])
    # t4: q's first window against t's last: len_t - k = 96; and a lone seed on -1
    t4 = placed(100, [(0, 96), (1, 19)])
    return [q, t1, t2, t3, t4]


def test_band_edges():
    seqs = band_records()
    with SeqSet(seqs) as ss:
        assert ss.seed_index(4, 20) == sum(len(ps) for s in seqs for ps in R.positions(s, 4, 20).values()) == 7 + 6 + 4 + 4 + 2
        row = rectangle(0, 1, 1, 4)
        got = {}
        for band in (0, 1, 3, 4, 5, 6, 29, 30, 31, 96, 97, 101, 102, TOP):
            cand, _ = check(ss, seqs, 4, 20, block=row, band=band)
            got[band] = {int(t): (int(s), int(d)) for t, s, d in zip(cand.t, cand.shared, cand.diag)}
        # d0 and d0 + band are in, d0 + band + 1 is out
        assert got[0][1] == (3, 15) and got[3][1] == (4, 14) and got[4][1] == (4, 14) and got[5][1] == (6, 10) and got[6][1] == (6, 10)
        assert got[1][1] == (4, 14)                                              # 14, 15, 15, 15 beats 10, 10
        # two windows with equal counts: the least d0
        assert got[0][2] == (1, 0) and got[1][2] == (2, 0) and got[29][2] == (2, 0) and got[30][2] == (3, 0) and got[31][2] == (4, 0)
        # negative diagonals and the extreme -(len_q - k)
        assert got[0][3] == (2, -14) and got[1][3] == (3, -15) and got[101][3] == (3, -15) and got[102][3] == (4, -116)
        # the extreme len_t - k
        assert got[0][4] == (1, -1) and got[96][4] == (1, -1) and got[97][4] == (2, -1)
        assert got[TOP][4] == (2, -1) and got[TOP][1] == (6, 10) and got[TOP][3] == (4, -116)
        # the same pairs from the other side: the diagonals change sign, the least d0 is the other end
        col = rectangle(1, 4, 0, 1)
        for band in (0, 1, 5, 102, TOP):
            check(ss, seqs, 4, 20, block=col, band=band)
        cand, _ = check(ss, seqs, 4, 20, block=col, band=97)
        assert (int(cand.shared[3]), int(cand.diag[3])) == (2, -96)             # t4 as the query: -(len_q - k) with q's first window
        # min_seeds at the count and one above
        assert check(ss, seqs, 4, 20, block=row, band=4, min_seeds=4)[0].t.tolist() == [1]
        assert check(ss, seqs, 4, 20, block=row, band=4, min_seeds=5)[0].t.tolist() == []
        assert check(ss, seqs, 4, 20, block=row, band=5, min_seeds=6)[0].t.tolist() == [1]


# ---------------------------------------------------------------- multiplicity
@pytest.mark.parametrize("length", [255, 256, 257])
def test_equal_residues_at_k_1(length):
    """Two records of `length` equal residues: length^2 seeds on 2 * length - 1 diagonals.  At 256 that is 65 536 = 256 x 256 seeds, 32
    tiles of the compaction's 2048 entries; the square of both records has four such pairs, about 128 tiles, in one chunk and in a
    chunk per row.  (The carry between the offsets step's trips of 256 tiles starts above 524 288 entries:
    test_more_seeds_than_one_trip_of_the_offsets_step.)"""
    seqs = [np.full(length, 2, dtype=np.uint8), np.full(length, 2, dtype=np.uint8)]
    with SeqSet(seqs) as ss:
        assert ss.seed_index(1, 4) == 2 * length
        one = rectangle(0, 1, 1, 1)
        cand, rows = check(ss, seqs, 1, 4, block=one, band=0)
        assert rows == [length * length] and as_lists(cand) == ([0], [0], [1], [length], [0])
        assert cand.summary == dict(seeds=length * length, pairs_with_seed=1, words_dropped=0, chunks=1)
        cand, _ = check(ss, seqs, 1, 4, block=one, band=TOP)
        assert (int(cand.shared[0]), int(cand.diag[0])) == (length * length, -(length - 1))
        cand, _ = check(ss, seqs, 1, 4, block=one, band=1)
        assert (int(cand.shared[0]), int(cand.diag[0])) == (2 * length - 1, -1)
        # the square with its self pairs: four pairs of length^2 seeds each, in one chunk and in a chunk per row
        sq = rectangle(0, 2, 0, 2)
        whole, _ = check(ss, seqs, 1, 4, block=sq, band=2)
        per_row, _ = check(ss, seqs, 1, 4, block=sq, band=2, chunk_seeds=2 * length * length)
        assert as_lists(per_row) == as_lists(whole) and per_row.summary["chunks"] == 2 and whole.summary["chunks"] == 1
        assert whole.shared.tolist() == [3 * length - 2] * 4 and whole.diag.tolist() == [-1] * 4
        # max_occ: 2 * length occurrences are kept at 2 * length and dropped one below
        assert len(check(ss, seqs, 1, 4, block=sq, max_occ=2 * length)[0]) == 4
        none, _ = check(ss, seqs, 1, 4, block=sq, max_occ=2 * length - 1)
        assert len(none) == 0 and none.summary == dict(seeds=0, pairs_with_seed=0, words_dropped=1, chunks=0)


def test_more_seeds_than_one_trip_of_the_offsets_step():
    """Three records of 730 equal residues at k = 1, the first against the other two: 2 x 532 900 seeds in one chunk, 521 tiles.  The
    second pair's run starts at sorted position 532 900, behind the 256 tiles (524 288 entries) of the offsets step's first trip, so
    its place in the list is the carry of that trip plus what its own trip counts."""
    length = 730
    assert length * length > 256 * 2048 and 2 * length * length <= R.CHUNK_SEEDS
    seqs = [np.full(length, 1, dtype=np.uint8)] * 3
    with SeqSet(seqs) as ss:
        row = rectangle(0, 1, 1, 2)
        cand, rows = check(ss, seqs, 1, 4, block=row, band=1)
        assert rows == [2 * length * length] and cand.summary == dict(seeds=2 * length * length, pairs_with_seed=2, words_dropped=0, chunks=1)
        assert as_lists(cand) == ([0, 1], [0, 0], [1, 2], [2 * length - 1] * 2, [-1, -1])
    # only the pair behind the trip's edge passes (the first target holds its 730 residues at every other position, so no diagonal of
    # its pair has more than half of them): the list's first entry comes from the second trip, behind a carry of 0
    spread = np.full(2 * length, NO, dtype=np.uint8)
    spread[::2] = 1
    other = [seqs[0], spread, seqs[0]]
    with SeqSet(other) as ss:
        cand, rows = check(ss, other, 1, 4, block=rectangle(0, 1, 1, 2), band=0, min_seeds=400)
        assert rows == [2 * length * length] and as_lists(cand) == ([1], [0], [2], [length], [0])


def test_a_homopolymer_against_a_random_record():
    rng = np.random.default_rng(5)
    seqs = [np.zeros(300, dtype=np.uint8), rng.integers(0, 4, 300).astype(np.uint8), rng.integers(0, 4, 77).astype(np.uint8), np.zeros(41, dtype=np.uint8)]
    with SeqSet(seqs) as ss:
        for k in (1, 2, 3):
            for band in (0, 7, 400):
                cand, rows = check(ss, seqs, k, 4, block=rectangle(0, 4, 0, 4), band=band)
        assert max(rows) > 90000                                                # 300 x 300 and 300 x 41 windows of the one word


# ---------------------------------------------------------------- the edges of the word
@pytest.mark.parametrize("k,a,rate", [(16, 4, 0.01), (12, 4, 0.02), (7, 20, 0.03), (8, 4, 0.05)])
def test_words_at_their_edges(k, a, rate):
    """(16, 4): A^k = 2^32, the word field is full and the sort runs as one pass over the whole key; the homopolymer of code 3 is the
    word 2^32 - 1 beside the all-ones key of the windows that are no words."""
    seqs = families(a, 5, 5, 100 * k + a, length=(60, 300), rate=rate, k=k)
    n = len(seqs)
    assert n <= 300 and max(len(s) for s in seqs) <= 600
    with SeqSet(seqs) as ss:
        assert ss.seed_index(k, a) == len(R.occurrences(seqs, k, a))
        total = 0
        for b in (upper(0, n), rectangle(0, n, 0, n), rectangle(3, n - 5, 2, n - 4)):
            for kw in (dict(), dict(band=5, min_seeds=3), dict(band=TOP, min_seeds=2), dict(band=2, min_seeds=4, max_occ=30)):
                cand, _ = check(ss, seqs, k, a, block=b, **kw)
                total += len(cand)
        assert total > 100
        full = ss.seed_join(k, a, block=rectangle(0, n, 0, n))
        have = dict(zip(zip(full.q.tolist(), full.t.tolist()), zip(full.shared.tolist(), full.diag.tolist())))
        homo, once, twin = n - 5, n - 4, n - 3
        assert have[(homo, once)] == (1, -(40 - k)) and have[(once, homo)] == (1, 0) and have[(homo, homo)] == (40 - k + 1, 0)
        assert have[(1, twin)] == have[(twin, 1)] == (len(seqs[1]) - k + 1, 0)
        assert not any(n - 11 in p or n - 10 in p or n - 8 in p for p in have)          # the empty, the short and the one without a word
        if a ** k == 2 ** 32:
            assert R.word(seqs[once], a) == 2 ** 32 - 1


# ---------------------------------------------------------------- max_occ
def test_max_occ_at_its_threshold():
    """marker 1: three occurrences in the set (two in record 0, one in record 1); marker 2: four (records 0, 1 and twice in 2); the
    other markers once or twice"""
    seqs = [placed(60, [(1, 0), (1, 10), (2, 20), (3, 30)]), placed(60, [(1, 5), (2, 15), (3, 40), (4, 50)]), placed(60, [(2, 0), (2, 10), (4, 20)]),
            placed(30, [(5, 3)])]
    with SeqSet(seqs) as ss:
        sq = rectangle(0, 4, 0, 4)
        everything, _ = check(ss, seqs, 4, 20, block=sq, band=TOP)
        assert everything.summary["words_dropped"] == 0
        at3, _ = check(ss, seqs, 4, 20, block=sq, band=TOP, max_occ=3)           # marker 1 has exactly 3: kept; marker 2 has 4: dropped
        assert at3.summary["words_dropped"] == 1
        pairs = dict(zip(zip(at3.q.tolist(), at3.t.tolist()), at3.shared.tolist()))
        assert pairs[(0, 1)] == 3 and pairs[(1, 2)] == 1 and (0, 2) not in pairs and pairs[(2, 2)] == 1
        at2, _ = check(ss, seqs, 4, 20, block=sq, band=TOP, max_occ=2)           # ... and with one less, marker 1 goes too
        assert at2.summary["words_dropped"] == 2
        assert dict(zip(zip(at2.q.tolist(), at2.t.tolist()), at2.shared.tolist()))[(0, 1)] == 1
        at4, _ = check(ss, seqs, 4, 20, block=sq, band=TOP, max_occ=4)
        assert at4.summary["words_dropped"] == 0 and as_lists(at4) == as_lists(everything)
        at1, _ = check(ss, seqs, 4, 20, block=upper(0, 4), band=TOP, max_occ=1)  # only marker 5 is left, and nobody shares it
        assert len(at1) == 0 and at1.summary["words_dropped"] == 4 and at1.summary["seeds"] == 0
        # the count is the whole set's, whatever the block
        assert check(ss, seqs, 4, 20, block=rectangle(3, 1, 3, 1), max_occ=3)[0].summary["words_dropped"] == 1


# ---------------------------------------------------------------- blocks, chunks and the cap
@pytest.fixture(scope="module")
def dna_case():
    k, a = 10, 4
    seqs = families(a, 6, 6, 99, length=(80, 300), rate=0.03, k=k)
    return k, a, seqs


def test_blocks(dna_case):
    k, a, seqs = dna_case
    n = len(seqs)
    with SeqSet(seqs) as ss:
        kept = 0
        for b in (rectangle(0, n, 0, n), upper(0, n), upper(5, n - 11), rectangle(7, 23, 3, n - 9), rectangle(4, 1, 0, n), rectangle(0, n, 7, 1),
                  rectangle(n - 1, 1, n - 1, 1)):
            for kw in (dict(band=5, min_seeds=5), dict(band=0), dict(band=40, min_seeds=20, max_occ=12)):
                kept += len(check(ss, seqs, k, a, block=b, **kw)[0])
        assert kept > 200


def test_chunks_give_the_list_of_one_chunk(dna_case):
    k, a, seqs = dna_case
    n = len(seqs)
    blk = rectangle(2, n - 4, 0, n)
    with SeqSet(seqs) as ss:
        one, rows = check(ss, seqs, k, a, block=blk, band=5, min_seeds=3)
        assert len(one) > 50 and 0 in rows and max(rows) > 100 and one.summary["chunks"] == 1
        for cap in (sum(rows), max(rows), max(rows) + 1, sum(rows[:9]), sum(rows[:9]) + 1, sum(rows) // 3, 1 << 26):
            cand, _ = check(ss, seqs, k, a, block=blk, band=5, min_seeds=3, chunk_seeds=cap)
            assert as_lists(cand) == as_lists(one)
            chunks = sum(1 for f, m in R.cut(rows, cap) if sum(rows[f:f + m]))
            assert cand.summary["chunks"] == chunks
            assert ss.stats()["bytes_down"] == 8 * len(rows) + 4 + 16 * chunks + 16 * len(cand), cap
        assert len(R.cut(rows, max(rows))) > 5


def test_a_row_above_the_cap_changes_nothing(dna_case):
    k, a, seqs = dna_case
    n = len(seqs)
    m = nucleotide_matrix()
    blk = rectangle(2, n - 4, 0, n)
    up = upper(0, n)
    with SeqSet(seqs, DNA) as ss:
        n_bitmap = ss.kmer_index(6, 4)
        n_sorted = ss.word_index(8, 4)
        by_words = ss.word_join(8, 4, min_shared=6, block=up)
        words_before = (by_words.index.tolist(), by_words.shared.tolist())
        earlier, rows = check(ss, seqs, k, a, block=blk, band=5, min_seeds=3)
        held = earlier.hits(m, K.DEL, K.EXT, 200.0)
        assert len(earlier) > 0 and len(held) > 0
        list_before, held_before = as_lists(earlier), P.held_bytes(held)[0]
        count = C.c_uint64(77)
        summ = _ffi.SeedjoinSummary(5, 5, 5, 5)
        spec = _ffi.SeedjoinSpec(k, a, 1, 0, 0, max(rows) - 1, 0, 0)
        assert ss.lib.aln_seqset_seed_join(ss.handle, C.byref(spec), C.byref(blk), C.byref(summ), C.byref(count)) == _ffi.ERR_CAPACITY
        assert count.value == 77 and (summ.seeds, summ.chunks) == (5, 5) and b"max_occ" in ss.lib.aln_last_error()
        # the earlier list with its diagonals and the held hits are what they were
        assert as_lists(Candidates(ss, len(earlier), diags=True)) == list_before and P.held_bytes(held)[0] == held_before
        # the three indexes answer as before: no rebuild, each spec names the index that is there
        spec = _ffi.SeedjoinSpec(k, a, 3, 5, 0, 0, 0, 0)
        assert ss.lib.aln_seqset_seed_join(ss.handle, C.byref(spec), C.byref(blk), None, C.byref(count)) == _ffi.OK      # (the summary is optional)
        assert as_lists(Candidates(ss, int(count.value), diags=True)) == list_before
        wspec = _ffi.WordjoinSpec(8, 4, 6, 0, 0, 0, 0)
        assert ss.lib.aln_seqset_word_join(ss.handle, C.byref(wspec), C.byref(up), C.byref(count)) == _ffi.OK
        again = Candidates(ss, int(count.value))
        assert (again.index.tolist(), again.shared.tolist()) == words_before and again.diag is None
        pspec = _ffi.PrefilterSpec(6, 4, 8, 0, 0, 0, 0)
        assert ss.lib.aln_seqset_prefilter(ss.handle, C.byref(pspec), C.byref(up), C.byref(count)) == _ffi.OK
        again = Candidates(ss, int(count.value))
        assert (again.index.tolist(), again.shared.tolist()) == W.word_join(seqs, 6, 4, 8, 0, blk_tuple(up))[0::3]
        assert n_bitmap.tolist() == [len(W.words(s, 6, 4)) for s in seqs] and n_sorted.tolist() == [len(W.words(s, 8, 4)) for s in seqs]
        assert P.held_bytes(held)[0] == held_before
        spec = _ffi.SeedjoinSpec(k, a, 1, 0, 0, max(rows), 0, 0)                  # a row equal to the cap is taken
        assert ss.lib.aln_seqset_seed_join(ss.handle, C.byref(spec), C.byref(blk), C.byref(summ), C.byref(count)) == _ffi.OK
        want, summary, _ = R.seed_join(seqs, k, a, block=blk_tuple(blk), chunk_seeds=max(rows))
        assert as_lists(Candidates(ss, int(count.value), diags=True)) == tuple(list(x) for x in want) and summ.chunks == summary["chunks"] > 5


# ---------------------------------------------------------------- both strands
def test_a_read_that_is_the_reverse_complement_of_a_piece_of_another():
    k = 12
    rng = np.random.default_rng(12)
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (150, 300, 90, 200, 120)]
    A, B = 1, 3
    recs[B] = K.revcomp(recs[A][50:250])
    n = len(recs)
    resident = recs + [K.revcomp(r) for r in recs]
    with SeqSet.stranded(recs, DNA) as ss:
        assert ss.seed_index(k, 4) == 2 * sum(len(r) - k + 1 for r in recs)
        block = both(rectangle(0, n, 0, n), n)
        cand, _ = check(ss, resident, k, 4, block=block, band=0, min_seeds=20)
        have = dict(zip(zip(cand.q.tolist(), cand.t.tolist()), zip(cand.shared.tolist(), cand.diag.tolist())))
        # the mirror of B is A[50:250]: 200 - k + 1 seeds, the word at 50 + i of A at i of the mirror
        assert have[(A, n + B)] == (200 - k + 1, -50) and (A, B) not in have
        assert have[(B, n + A)] == (200 - k + 1, 50) and (B, A) not in have      # from B's side: A's mirror holds B at 300 - 250 = 50
        assert sorted(p for p in have if p[0] != p[1]) == [(A, n + B), (B, n + A)]
        assert all(have[(i, i)] == (len(recs[i]) - k + 1, 0) for i in range(n))
        # with every seed of the pair counted, (A, B) still does not pass
        loose, _ = check(ss, resident, k, 4, block=block, band=TOP, min_seeds=2)
        assert (A, B) not in set(zip(loose.q.tolist(), loose.t.tolist())) and (A, n + B) in set(zip(loose.q.tolist(), loose.t.tolist()))
        # max_occ counts over all 2n resident records: a word of the shared piece is there twice (in A and in B's mirror), and so is its
        # reverse complement (in B and in A's mirror)
        dropped, _ = check(ss, resident, k, 4, block=block, max_occ=1)
        assert dropped.summary["words_dropped"] >= 2 * (200 - k + 1) and (A, n + B) not in set(zip(dropped.q.tolist(), dropped.t.tolist()))
        assert check(ss, resident, k, 4, block=block, max_occ=2)[0].summary["words_dropped"] < 20


# ---------------------------------------------------------------- the candidate passes on top
@pytest.fixture(scope="module")
def sset():
    with SeqSet(T.make_set()) as s:
        yield s


def test_score_hits_and_best_on_a_seed_join_list(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    seqs = T.make_set()
    n = len(sset)
    blk = upper(0, n)
    f_all, st_all = sset.score(m, d, e, blk, semantics=sem)
    full = sset.hits(m, d, e, F_MIN, blk, semantics=sem)
    full_idx, full_f = full.index.copy(), full.f.copy()
    cand, _ = check(sset, seqs, 3, 20, block=blk, band=3, min_seeds=2)
    assert 0 < len(cand) < sset.pairs(blk)
    f, status = cand.score(m, d, e, semantics=sem)
    assert (T.bits(f) == T.bits(f_all[cand.index.astype(np.int64)])).all() and (status == st_all[cand.index.astype(np.int64)]).all()
    held = cand.hits(m, d, e, F_MIN, semantics=sem)
    rows = np.isin(full_idx, cand.index)
    assert len(held) > 0 and held.index.tolist() == full_idx[rows].tolist() and (T.bits(held.f) == T.bits(full_f[rows])).all()
    # the strings too: every pair of the block held once, then the candidates' held hits against those
    everything = sset.hits(m, d, e, -1e300, blk, semantics=sem)
    where = {int(i): h for h, i in enumerate(everything.index)}
    _digest, _res, all_strs = P.held_bytes(everything)
    held = cand.hits(m, d, e, F_MIN, semantics=sem)
    _digest, _res, strs = P.held_bytes(held)
    for h, i in enumerate(held.index.tolist()):
        assert strs[h][0].tobytes() == all_strs[where[i]][0].tobytes() and strs[h][1].tobytes() == all_strs[where[i]][1].tobytes()
    assert as_lists(Candidates(sset, len(cand), diags=True)) == as_lists(cand)   # the passes leave the list alone
    # best: with min_seeds = 1 the listed pairs are the pairs that share a word, the word join's list
    sq = rectangle(0, n, 0, n)
    by_words = sset.word_join(3, 20, min_shared=1, block=sq)
    want_best = P.held_bytes(by_words.best(m, d, e, 2, skip_self=True, semantics=sem))[0]
    by_seeds, _ = check(sset, seqs, 3, 20, block=sq, band=7)
    assert by_seeds.index.tolist() == by_words.index.tolist()
    best = by_seeds.best(m, d, e, 2, skip_self=True, semantics=sem)
    assert len(best) > 0 and P.held_bytes(best)[0] == want_best
    # ... and what SeqSet.score says of those pairs: per query the two best listed targets, higher f first, then the lower target
    f_sq, st_sq = sset.score(m, d, e, sq, semantics=sem)
    expect = []
    for q in range(n):
        mine = [int(i) for i, qq, tt in zip(by_seeds.index, by_seeds.q, by_seeds.t) if qq == q and tt != q and st_sq[int(i)] == 0]
        mine.sort(key=lambda i: (-float(f_sq[i]), i))
        expect += sorted(mine[:2])
    assert best.index.tolist() == expect and (T.bits(best.f) == T.bits(f_sq[np.array(expect, dtype=np.int64)])).all()


def test_diags_of_the_other_routes_are_refused(sset):
    lib, hnd = sset.lib, sset.handle
    INV = _ffi.ERR_INVALID_ARGUMENT
    diag = np.full(4, 7, dtype=np.int32)
    blk = upper(0, len(sset))
    assert len(sset.prefilter(*P.K3, block=blk, **P.SELECTIVE)) >= 4
    assert lib.aln_seqset_candidate_diags(hnd, 0, 4, diag.ctypes.data) == INV and (diag == 7).all() and b"seed_join" in lib.aln_last_error()
    by_words = sset.word_join(*P.K3, block=blk, **P.SELECTIVE)
    assert by_words.diag is None and by_words.summary is None
    assert lib.aln_seqset_candidate_diags(hnd, 0, 4, diag.ctypes.data) == INV and (diag == 7).all()
    assert lib.aln_seqset_candidate_diags(hnd, 0, 0, None) == INV
    cand = sset.seed_join(3, 20, block=blk)
    assert lib.aln_seqset_candidate_diags(hnd, 1, 4, diag.ctypes.data) == _ffi.OK and diag.tolist() == cand.diag[1:5].tolist()
    diag[:] = 7
    assert lib.aln_seqset_candidate_diags(hnd, len(cand) - 3, 4, diag.ctypes.data) == INV and (diag == 7).all()      # a range beyond the list
    assert lib.aln_seqset_candidate_diags(hnd, len(cand) + 1, 0, diag.ctypes.data) == INV
    assert lib.aln_seqset_candidate_diags(hnd, 0, 4, None) == INV
    assert lib.aln_seqset_candidate_diags(hnd, len(cand), 0, None) == _ffi.OK
    sset.seed_index(3, 20)                                                        # a new index drops the list
    assert lib.aln_seqset_candidate_diags(hnd, 0, 0, None) == INV


# ---------------------------------------------------------------- agreement with the word join
def no_repeat_records(k, a, seed):
    """families in which no record holds a word twice (drawn again until that is so)"""
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(8):
        parent = rng.integers(0, a, rng.integers(60, 121)).astype(np.uint8)
        made = 0
        while made < 5:
            s = parent.copy()
            flip = rng.random(len(s)) < 0.06
            s[flip] = rng.integers(0, a, int(flip.sum())).astype(np.uint8)
            if all(len(ps) == 1 for ps in R.positions(s, k, a).values()):
                seqs.append(s)
                made += 1
            else:
                parent = rng.integers(0, a, len(parent)).astype(np.uint8)
    return seqs


@pytest.mark.parametrize("k,a", [(8, 4), (6, 4), (3, 20), (5, 20)])
def test_seeds_are_shared_words_where_no_word_repeats(k, a):
    seqs = no_repeat_records(k, a, 10 * k + a)
    for s in seqs:                                                                # the premise, from the records themselves
        windows = [tuple(s[i:i + k].tolist()) for i in range(len(s) - k + 1)]
        assert len(set(windows)) == len(windows) and int(s.max()) < a
    n = len(seqs)
    with SeqSet(seqs) as ss:
        for b in (upper(0, n), rectangle(0, n, 0, n)):
            for least in (1, 2, 5, 20):
                by_words = ss.word_join(k, a, min_shared=least, block=b)
                by_seeds, _ = check(ss, seqs, k, a, block=b, band=TOP, min_seeds=least)
                assert len(by_words) > 0 or least > 2
                assert (by_seeds.index.tolist(), by_seeds.q.tolist(), by_seeds.t.tolist(), by_seeds.shared.tolist()) == \
                    (by_words.index.tolist(), by_words.q.tolist(), by_words.t.tolist(), by_words.shared.tolist())


# ---------------------------------------------------------------- call history
def test_no_answer_depends_on_the_calls_before():
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    seqs = T.make_set()
    n = len(seqs)
    blk, sq = upper(0, n), rectangle(0, n, 0, n)

    def others(ss):
        """the other calls, each with fixed arguments: name -> (the call, what it answers as comparable values)"""
        return {
            "kmer_index": lambda: ss.kmer_index(3, 20).tolist(),
            "prefilter": lambda: [x.tolist() for x in (lambda c: (c.index, c.q, c.t, c.shared))(ss.prefilter(3, 20, block=blk, **P.SELECTIVE))],
            "word_index": lambda: ss.word_index(4, 20).tolist(),
            "word_join": lambda: [x.tolist() for x in (lambda c: (c.index, c.q, c.t, c.shared))(ss.word_join(4, 20, min_shared=2, block=blk))],
            "hits": lambda: P.held_bytes(ss.hits(m, d, e, F_MIN, blk, semantics=sem))[0],
            "best": lambda: P.held_bytes(ss.best(m, d, e, 2, block=sq, skip_self=True, semantics=sem))[0],
            "cigars": lambda: (lambda c: (c.words.tolist(), c.offsets.tolist()))(ss.hits(m, d, e, F_MIN, blk, semantics=sem).cigars(extended=True)),
        }

    with SeqSet(seqs) as fresh:
        reference = {name: call() for name, call in others(fresh).items()}
    joins = [dict(k=3, band=3, min_seeds=2, block=blk), dict(k=4, band=0, min_seeds=1, block=sq), dict(k=3, band=TOP, min_seeds=3, max_occ=6, block=sq)]

    def ask(ss, records, j):
        """a seed join (the index rebuilt whenever k changes, and once more explicitly) held against the reference"""
        kw = {key: v for key, v in j.items() if key != "k"}
        if j["k"] == 4:
            assert ss.seed_index(4, 20) == len(R.occurrences(records, 4, 20))
        check(ss, records, j["k"], 20, **kw)

    with SeqSet(seqs) as ss:
        calls = others(ss)
        step = 0
        for name in calls:
            ask(ss, seqs, joins[step % 3]); step += 1                              # before ...
            assert calls[name]() == reference[name], name
            ask(ss, seqs, joins[step % 3]); step += 1                              # ... and after
            assert calls[name]() == reference[name], name                          # and the call itself after a join
        # held hits survive both seed calls
        held = ss.hits(m, d, e, F_MIN, blk, semantics=sem)
        before = P.held_bytes(held)[0]
        ss.seed_index(3, 20)
        ask(ss, seqs, joins[0])
        assert P.held_bytes(held)[0] == before
    # a new set after a destroy: other records, the same answers as a handle that never saw the first set
    other = families(20, 4, 4, 3, length=(50, 200), rate=0.05, k=3)
    with SeqSet(other) as ss:
        bo = upper(0, len(other))
        check(ss, other, 3, 20, block=bo, band=3, min_seeds=2)
        check(ss, other, 5, 20, block=bo, band=0, min_seeds=1)
        check(ss, other, 3, 20, block=rectangle(1, 5, 0, len(other)), band=TOP, min_seeds=4, max_occ=9)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_every_state_intact(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    lib, hnd = sset.lib, sset.handle
    n = len(sset)
    blk = upper(0, n)
    cand = sset.seed_join(3, 20, band=3, min_seeds=2, block=blk)
    held = sset.hits(m, d, e, F_MIN, rectangle(*T.RECT), semantics=sem)
    held_before = P.held_bytes(held)[0]
    INV = _ffi.ERR_INVALID_ARGUMENT
    count, occ = C.c_uint64(77), C.c_uint64(77)
    summ = _ffi.SeedjoinSummary(5, 5, 5, 5)

    def spec(k=3, alphabet=20, min_seeds=1, band=0, max_occ=0, chunk=0, flags=0, reserved=0):
        return _ffi.SeedjoinSpec(k, alphabet, min_seeds, band, max_occ, chunk, flags, reserved)

    def intact():
        return (count.value == 77 and occ.value == 77 and (summ.seeds, summ.pairs_with_seed, summ.words_dropped, summ.chunks) == (5, 5, 5, 5)
                and as_lists(Candidates(sset, len(cand), diags=True)) == as_lists(cand) and P.held_bytes(held)[0] == held_before)

    def join(sp, b=blk, s=summ, c=count):
        return lib.aln_seqset_seed_join(hnd, C.byref(sp) if sp is not None else None, C.byref(b) if b is not None else None,
                                        C.byref(s) if s is not None else None, C.byref(c) if c is not None else None)

    for k, alphabet in ((0, 20), (17, 4), (17, 1), (16, 5), (8, 20), (3, 0), (2, 65537), (1, 0)):
        assert lib.aln_seqset_seed_index(hnd, k, alphabet, C.byref(occ)) == INV and intact()
        assert join(spec(k, alphabet)) == INV and intact()
    for sp in (spec(k=2), spec(alphabet=4), spec(min_seeds=0), spec(band=2 ** 31), spec(band=2 ** 32 - 1), spec(flags=1), spec(reserved=1), spec(chunk=(1 << 26) + 1)):
        assert join(sp) == INV and intact()
    for bb in (_ffi.SeqsetBlock(0, n + 1, 0, n + 1, 1, 0), _ffi.SeqsetBlock(0, 3, 1, 3, 1, 0), _ffi.SeqsetBlock(0, 0, 0, 3, 0, 0), _ffi.SeqsetBlock(0, 3, 0, 3, 0, 1)):
        assert join(spec(), b=bb) == INV and intact()
    assert join(None) == INV and intact()
    assert join(spec(), b=None) == INV and intact()
    assert join(spec(), c=None) == INV and intact()
    widest = spec(min_seeds=2, band=3, chunk=1 << 26)                              # the largest chunk, and the largest band, are taken
    assert join(widest, s=None) == _ffi.OK and count.value == len(cand)
    count.value = 77
    assert join(spec(min_seeds=2, band=TOP)) == _ffi.OK
    count.value, summ.seeds, summ.pairs_with_seed, summ.words_dropped, summ.chunks = 77, 5, 5, 5, 5
    cand = Candidates(sset, len(sset.seed_join(3, 20, band=3, min_seeds=2, block=blk)), diags=True)
    # no seed index at all: a fresh set, even one with the other two indexes of the same (k, A)
    with SeqSet(T.make_set()[:4]) as fresh:
        small = upper(0, 4)
        assert lib.aln_seqset_seed_join(fresh.handle, C.byref(spec()), C.byref(small), C.byref(summ), C.byref(count)) == INV
        fresh.kmer_index(3, 20)
        fresh.word_index(3, 20)
        assert lib.aln_seqset_seed_join(fresh.handle, C.byref(spec()), C.byref(small), C.byref(summ), C.byref(count)) == INV
        assert b"seed index" in lib.aln_last_error()
        assert lib.aln_seqset_word_index(fresh.handle, 9, 4, None) == INV         # the other routes' caps stand
        assert lib.aln_seqset_seed_index(fresh.handle, 3, 20, None) == _ffi.OK     # occurrences is optional
        assert lib.aln_seqset_seed_join(fresh.handle, C.byref(spec()), C.byref(small), None, C.byref(occ)) == _ffi.OK
        occ.value = 77
    assert intact()


# ---------------------------------------------------------------- the C99 caller
def hexf(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def protein_families(seed=5):
    return families(20, 8, 5, seed, length=(60, 160), rate=0.1, k=5)[:40]


def test_through_c(tmp_path):
    """tests/abi_seedjoin.c: the three exports, and the candidate calls on their result, from C99 on buffers of exactly the documented
    sizes, each followed by a guard zone"""
    from aligner_amd.matrices import get_blosum62
    m = get_blosum62()
    seqs = protein_families()
    k, a, min_seeds, band, max_occ, chunk = 4, 20, 3, 4, 4, 400
    tok = [len(seqs)] + [len(s) for s in seqs] + [int(c) for s in seqs for c in s] + [m.shape[0], m.shape[1]]
    tok += [hexf(v) for v in np.asarray(m, dtype=np.float64).ravel()] + [hexf(11.0), hexf(2.0), hexf(F_MIN), 98]
    tok += [k, a, min_seeds, band, max_occ, chunk]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(x) for x in tok) + "\n")
    exe = native_build.build_seedjoin_harness()
    out = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1] for l in lines if l[0] == "rc"] == ["seqset_create", "seed_index", "seed_join", "candidates", "candidate_diags", "candidate_hits", "held_list"]
    assert all(l[2] == "0" for l in lines if l[0] == "rc") and ["guards", "ok"] in lines
    want, summary, rows = R.seed_join(seqs, k, a, min_seeds, band, max_occ, (0, len(seqs), 0, len(seqs), 1), chunk)
    assert [l[1] for l in lines if l[0] == "occurrences"] == [str(len(R.occurrences(seqs, k, a)))]
    assert [l[1:] for l in lines if l[0] == "summary"] == [[str(summary[key]) for key in ("seeds", "pairs_with_seed", "words_dropped", "chunks")]]
    assert summary["chunks"] > 1 and summary["words_dropped"] > 0
    assert [l[1] for l in lines if l[0] == "count"] == [str(len(want[0]))] and len(want[0]) > 20
    assert [l[1:] for l in lines if l[0] == "cand"] == [[str(v) for v in row] for row in zip(*want)]
    with SeqSet(seqs) as ss:
        held = ss.seed_join(k, a, min_seeds=min_seeds, band=band, max_occ=max_occ).hits(m, 11.0, 2.0, F_MIN)
        assert [l[1] for l in lines if l[0] == "held"] == [str(len(held))] and len(held) > 0
        assert [l[1:] for l in lines if l[0] == "hit"] == [[str(int(i)), str(int(q)), str(int(t)), hexf(v)] for i, q, t, v in zip(held.index, held.q, held.t, held.f)]


# ---------------------------------------------------------------- the command
def test_the_command(tmp_path, capsys):
    from aligner_amd import allpairs
    rng = np.random.default_rng(21)
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (150, 300, 90, 200, 120, 160)]
    recs[3] = K.revcomp(recs[1][50:250])                                          # a minus-strand overlap
    recs[5] = np.concatenate([recs[0][40:], rng.integers(0, 4, size=50).astype(np.uint8)])       # a plus-strand overlap: diagonal -40
    n = len(recs)
    fa = tmp_path / "x.fasta"
    letter = {int(DNA.str_to_vec(ch)[0]): ch for ch in "ACGT"}
    assert sorted(letter) == [0, 1, 2, 3]
    fa.write_text("".join(">s%d\n%s\n" % (i, "".join(letter[int(c)] for c in s)) for i, s in enumerate(recs)))
    m = nucleotide_matrix()
    # one strand, K = 14: only this route takes it
    args = ["-i", str(fa), "--dna", "--kmer", "14", "--seed-join", "--min-seeds", "10", "--band", "2"]
    want, _summary, _rows = R.seed_join(recs, 14, 4, 10, 2, 0, (0, n, 0, n, 1))
    assert list(zip(want[1], want[2], want[4])) == [(0, 5, -40)]
    with SeqSet(recs, DNA) as ss:
        f, status = ss.score(m, 11.0, 2.0, None)
        assert allpairs.main(args) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%r,%d,%d" % (q, t, float(f[i]), s, dg) for i, q, t, s, dg in zip(*want)]
    # both strands: the rows of the rectangle's pairs from the record that comes first, the diagonal in the mirror's coordinates
    resident = recs + [K.revcomp(r) for r in recs]
    want, _summary, _rows = R.seed_join(resident, 14, 4, 10, 2, 0, (0, n, 0, 2 * n, 0))
    rows = [(i, q, t, s, dg) for i, q, t, s, dg in zip(*want) if q < t % n]
    assert [(q, t, dg) for _i, q, t, _s, dg in rows] == [(0, 5, -40), (1, n + 3, -50)]
    with SeqSet.stranded(recs, DNA) as ss:
        f, status = ss.score(m, 11.0, 2.0, both(rectangle(0, n, 0, n), n))
        assert allpairs.main(args + ["--both-strands"]) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%s,%r,%d,%d" % (q, t % n, "-" if t >= n else "+", float(f[i]), s, dg) for i, q, t, s, dg in rows]
        # --f-min: the held rows of the candidates
        held = ss.seed_join(14, 4, min_seeds=10, band=2, block=both(rectangle(0, n, 0, n), n)).hits(m, 11.0, 2.0, 100.0)
        assert allpairs.main(args + ["--both-strands", "--f-min", "100.0"]) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%s,%r" % (int(q), int(t) % n, "-" if t >= n else "+", float(v)) for q, t, v in zip(held.q, held.t, held.f) if q < t % n]
        assert len(out) == 2
        # --best-candidates: the rows of the same question asked through the library
        assert allpairs.main(args + ["--both-strands", "--best-candidates", "2", "--paf", str(tmp_path / "x.paf")]) == 0
        out = capsys.readouterr().out.splitlines()
        best = ss.seed_join(14, 4, min_seeds=10, band=2, block=both(rectangle(0, n, 0, n), n)).best(m, 11.0, 2.0, 2, skip_self=True)
        expect = ["s%d,%d,s%d,%s,%r" % (qq, int(best.rank[p]) + 1, int(best.t[p]) % n, "-" if best.t[p] >= n else "+", float(best.f[p]))
                  for qq, pos in best.by_query() for p in pos]
        assert out == expect and len(out) >= 4
        assert len((tmp_path / "x.paf").read_text().splitlines()) == len(out)
    # --max-occ drops what occurs too often: at 1 every word of an overlap is gone, and so is every row
    assert allpairs.main(args + ["--max-occ", "1"]) == 0
    assert capsys.readouterr().out == ""
