"""The sorted word index and its join on the GPU (aln_seqset_word_index / _word_join): equality with the bitmap route of the
prefilter wherever both apply, whole lists compared; protein 5-, 6- and 7-mers (and the full 32-bit word of (8, 16)) against
wordjoin_ref.py; the places where a join can go wrong (short and empty records, codes outside the alphabet, repeated words, one word
in every record, twins, nothing shared, chunks of single rows, a row above the cap); the candidate passes on top; state and refusals;
the C99 caller; the command.  Every comparison is on integers or on bits.

Sets hold 30 .. 300 records of 0 .. 200 residues.  The selection's tile is 2048 entries (aln_select.h): the family sets have more
distinct (word, sequence) entries than one tile, and the one-word set has 90 000 occurrences, 44 tiles."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wordjoin_ref as R                                                        # noqa: E402
import test_prefilter_gpu as P                                                  # noqa: E402
import test_seqset_gpu as T                                                     # noqa: E402
from aligner_amd import _ffi, runtime                                           # noqa: E402
from aligner_amd import build as native_build                                   # noqa: E402
from aligner_amd.seqset import Candidates, SeqSet, rectangle, upper             # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_MIN = 30.0


def blk_tuple(b):
    return (int(b.q_first), int(b.q_count), int(b.t_first), int(b.t_count), int(b.upper))


def as_lists(cand):
    return cand.index.tolist(), cand.q.tolist(), cand.t.tolist(), cand.shared.tolist()


def check_list(cand, want):
    idx, q, t, sh = want
    assert len(cand) == len(idx)
    assert as_lists(cand) == (list(idx), list(q), list(t), list(sh))


def family_set(k, a, n_fam, per_fam, seed, length=(30, 200), rate=0.08):
    """n_fam families of per_fam records: a random parent and copies with substitutions at `rate`, some with a piece cut out; then the
    records a join can stumble over.  Returns (records, names of the special ones by position)."""
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
                s = np.concatenate([s[:cut], s[cut + k:]])
            seqs.append(s)
    first = seqs[0]
    special = {}
    special["empty"] = len(seqs); seqs.append(np.zeros(0, dtype=np.uint8))
    special["short"] = len(seqs); seqs.append(first[:k - 1].copy() if k > 1 else np.zeros(0, dtype=np.uint8))
    special["exact"] = len(seqs); seqs.append(first[:k].copy())                   # one window
    outside = first.copy()
    outside[k - 1::k] = a                                                         # a code >= A inside every window: no word at all
    special["outside"] = len(seqs); seqs.append(outside)
    one_bad = first.copy()
    one_bad[len(one_bad) // 2] = 98                                               # ... inside k windows only
    special["one_bad"] = len(seqs); seqs.append(one_bad)
    special["repeat"] = len(seqs); seqs.append(np.tile(first[:k], 30)[:200])      # the same k words over and over: each counts once
    special["homo"] = len(seqs); seqs.append(np.full(150, first[0], dtype=np.uint8))      # one word, 150 - k + 1 windows
    special["twin_a"] = len(seqs); seqs.append(seqs[1].copy())
    special["twin_b"] = len(seqs); seqs.append(seqs[1].copy())
    special["empty2"] = len(seqs); seqs.append(np.zeros(0, dtype=np.uint8))       # (an empty record that is not the last before others)
    seqs.append(seqs[2][::-1].copy())
    return seqs, special


# ---------------------------------------------------------------- equality with the bitmap route
THRESHOLDS = [(1, 0), (2, 0), (3, 256), (1, 1024), (5, 64)]


def blocks_of(n):
    return [rectangle(0, n, 0, n), upper(0, n), upper(5, n - 11), rectangle(7, 23, 3, n - 9), rectangle(4, 1, 0, n), rectangle(0, n, n - 3, 1)]


@pytest.mark.parametrize("k,a", [(3, 20), (4, 20), (8, 4), (1, 4)])
def test_equal_to_the_bitmap_route(k, a):
    seqs, special = family_set(k, a, 12, 9, 100 * k + a)
    n = len(seqs)
    assert 30 <= n <= 300 and max(len(s) for s in seqs) <= 200
    with SeqSet(seqs) as ss:
        n_bitmap = ss.kmer_index(k, a)
        n_sorted = ss.word_index(k, a)
        assert n_sorted.tolist() == n_bitmap.tolist() == [len(R.words(s, k, a)) for s in seqs]
        assert n_sorted[special["empty"]] == 0 and n_sorted[special["short"]] == 0 and n_sorted[special["exact"]] == 1
        assert n_sorted[special["outside"]] == 0 and n_sorted[special["homo"]] == 1 and n_sorted[special["repeat"]] <= k
        if a ** k > 2048:
            assert int(n_sorted.sum()) > 2048                                   # more than one selection tile of distinct entries
        kept = 0
        for b in blocks_of(n):
            for min_shared, per in THRESHOLDS:
                want = as_lists(ss.prefilter(k, a, min_shared=min_shared, min_per_1024=per, block=b))
                got = ss.word_join(k, a, min_shared=min_shared, min_per_1024=per, block=b)
                check_list(got, want)
                kept += len(got)
        assert kept > 0
        # self pairs of a rectangle are listed; twins share everything
        full = ss.word_join(k, a, min_shared=1, min_per_1024=1024, block=rectangle(0, n, 0, n))
        have = set(zip(full.q.tolist(), full.t.tolist()))
        assert (0, 0) in have and (special["twin_a"], special["twin_b"]) in have and (special["twin_b"], 1) in have
        assert not any(special["empty"] in p or special["outside"] in p for p in have)


# ---------------------------------------------------------------- beyond the bitmap cap
@pytest.mark.parametrize("k,a", [(5, 20), (6, 20), (7, 20), (8, 16)])
def test_beyond_the_bitmap_cap(k, a):
    """(8, 16): A^k = 2^32, the word field is full, and the homopolymer of code 15 is the word 2^32 - 1 beside the all-ones key of
    the windows that are no words."""
    seqs, special = family_set(k, a, 6, 8, 7 * k + a, rate=0.04)
    seqs.append(np.full(40, a - 1, dtype=np.uint8)); seqs.append(np.full(k, a - 1, dtype=np.uint8))     # the largest word, twice
    n = len(seqs)
    with SeqSet(seqs) as ss:
        with pytest.raises(Exception):
            ss.kmer_index(k, a)                                                   # the bitmap route still refuses these
        n_words = ss.word_index(k, a)
        assert n_words.tolist() == [len(R.words(s, k, a)) for s in seqs]
        total = 0
        for b in (upper(0, n), rectangle(3, n - 5, 0, n), rectangle(0, n, 0, n)):
            for min_shared, per in ((1, 0), (2, 128), (4, 512)):
                want = R.word_join(seqs, k, a, min_shared, per, blk_tuple(b))
                check_list(ss.word_join(k, a, min_shared=min_shared, min_per_1024=per, block=b), want)
                total += len(want[0])
        assert total > 100
        pairs = set(zip(*R.word_join(seqs, k, a, 1, 0, (0, n, 0, n, 1))[1:3]))
        assert (n - 2, n - 1) in pairs


# ---------------------------------------------------------------- one word in every record, nothing shared
def test_one_word_carried_by_all_300_records():
    """90 000 occurrences of one word: every pair of the square shares exactly that word.  One thread per occurrence, so the word does
    not sit on one wave; the list is every pair in order."""
    k, a = 4, 20
    seqs = [np.array([3, 1, 4, 1], dtype=np.uint8) for _ in range(300)]
    with SeqSet(seqs) as ss:
        assert ss.word_index(k, a).tolist() == [1] * 300
        cand = ss.word_join(k, a, min_shared=1, min_per_1024=1024, block=rectangle(0, 300, 0, 300))
        assert len(cand) == 90000 and cand.index.tolist() == list(range(90000)) and (cand.shared == 1).all()
        assert (cand.q == np.repeat(np.arange(300), 300)).all() and (cand.t == np.tile(np.arange(300), 300)).all()
        assert ss.stats()["bytes_down"] == 8 * 300 + 12 * 1 + 12 * 90000          # one chunk
        cand = ss.word_join(k, a, block=upper(0, 300))
        assert len(cand) == 44850 and cand.index.tolist() == list(range(44850)) and (cand.shared == 1).all()
        assert len(ss.word_join(k, a, min_shared=2, block=upper(0, 300))) == 0
        # chunks of one row each, and a cut between rows 16 and 17: the same list
        one = ss.word_join(k, a, block=rectangle(0, 300, 0, 300))
        rows = ss.word_join(k, a, block=rectangle(0, 300, 0, 300), chunk_occurrences=300)
        assert ss.stats()["bytes_down"] == 8 * 300 + 12 * 300 + 12 * 90000        # 300 chunks
        assert as_lists(rows) == as_lists(one)
        two = ss.word_join(k, a, block=rectangle(0, 300, 0, 300), chunk_occurrences=17 * 300)
        assert ss.stats()["bytes_down"] == 8 * 300 + 12 * 18 + 12 * 90000         # 17 rows a chunk: 17 chunks of 17 and one of 11
        assert as_lists(two) == as_lists(one)


def test_nothing_shared_is_an_empty_list():
    k, a = 3, 20
    seqs = [np.array([i // 20, i % 20, 7, 98, 98], dtype=np.uint8) for i in range(40)]      # one word each, all different
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    with SeqSet(seqs) as ss:
        assert ss.word_index(k, a).tolist() == [1] * 40
        def outcome(cand):
            """what the candidate calls make of the list: sizes, or the error they raise"""
            try:
                f, status = cand.score(m, d, e, semantics=sem)
                held = cand.hits(m, d, e, F_MIN, semantics=sem)
                return len(cand), len(Candidates(ss, 0)), len(f), len(status), len(held)
            except Exception as ex:                                               # noqa: BLE001
                return type(ex).__name__, str(ex)

        by_join = outcome(ss.word_join(k, a, block=upper(0, 40)))
        by_bitmaps = outcome(ss.prefilter(k, a, min_shared=1, block=upper(0, 40)))
        assert by_join == by_bitmaps and by_join[0] == 0
        # the rectangle lists the self pairs and nothing else
        cand = ss.word_join(k, a, block=rectangle(0, 40, 0, 40))
        assert cand.q.tolist() == cand.t.tolist() == list(range(40))


# ---------------------------------------------------------------- chunks and the cap
@pytest.fixture(scope="module")
def chunk_case():
    k, a = 5, 20
    seqs, special = family_set(k, a, 5, 8, 99, rate=0.05)
    blk = rectangle(2, len(seqs) - 4, 0, len(seqs))
    occ = R.row_occurrences(seqs, k, a, blk_tuple(blk))
    return k, a, seqs, blk, occ


def test_chunks_give_the_list_of_one_chunk(chunk_case):
    k, a, seqs, blk, occ = chunk_case
    want = R.word_join(seqs, k, a, 2, 64, blk_tuple(blk))
    assert len(want[0]) > 50 and 0 in occ and max(occ) > 100
    with SeqSet(seqs) as ss:
        ss.word_index(k, a)
        for cap in (0, sum(occ), max(occ), max(occ) + 1, sum(occ[:9]), sum(occ[:9]) + 1, sum(occ) // 3):
            cand = ss.word_join(k, a, min_shared=2, min_per_1024=64, block=blk, chunk_occurrences=cap)
            check_list(cand, want)
            cut = R.cut(occ, cap if cap else R.CHUNK_OCCURRENCES)
            chunks = sum(1 for f, n in cut if sum(occ[f:f + n]))                  # (a run of rows without an occurrence is no chunk)
            assert ss.stats()["bytes_down"] == 8 * len(occ) + 12 * chunks + 12 * len(cand), cap
        assert R.cut(occ, sum(occ[:9]))[0] == (0, 9 + next(i for i, v in enumerate(occ[9:] + [1]) if v))      # the cut falls after row 8 (and empty rows)
        assert len(R.cut(occ, max(occ))) > 5


def test_a_row_above_the_cap_changes_nothing(chunk_case):
    k, a, seqs, blk, occ = chunk_case
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    with SeqSet(seqs) as ss:
        ss.word_index(k, a)
        earlier = ss.word_join(k, a, min_shared=3, block=upper(0, len(seqs)))
        held = earlier.hits(m, d, e, F_MIN, semantics=sem)
        assert len(earlier) > 0 and len(held) > 0
        list_before, held_before = as_lists(earlier), P.held_bytes(held)[0]
        count = C.c_uint64(77)
        spec = _ffi.WordjoinSpec(k, a, 1, 0, max(occ) - 1, 0, 0)
        assert ss.lib.aln_seqset_word_join(ss.handle, C.byref(spec), C.byref(blk), C.byref(count)) == _ffi.ERR_CAPACITY
        assert count.value == 77 and b"chunk_occurrences" in ss.lib.aln_last_error()
        assert as_lists(Candidates(ss, len(earlier))) == list_before and P.held_bytes(held)[0] == held_before
        # the word index: the join it gives now is the join it gave before (no rebuild: the spec names the built index)
        spec = _ffi.WordjoinSpec(k, a, 3, 0, 0, 0, 0)
        b = upper(0, len(seqs))
        assert ss.lib.aln_seqset_word_join(ss.handle, C.byref(spec), C.byref(b), C.byref(count)) == _ffi.OK
        assert as_lists(Candidates(ss, int(count.value))) == list_before and P.held_bytes(held)[0] == held_before
        spec = _ffi.WordjoinSpec(k, a, 1, 0, max(occ), 0, 0)                       # a row equal to the cap is taken
        assert ss.lib.aln_seqset_word_join(ss.handle, C.byref(spec), C.byref(blk), C.byref(count)) == _ffi.OK
        check_list(Candidates(ss, int(count.value)), R.word_join(seqs, k, a, 1, 0, blk_tuple(blk)))


# ---------------------------------------------------------------- the candidate passes on top, and state
K3 = P.K3
SELECTIVE = P.SELECTIVE


@pytest.fixture(scope="module")
def sset():
    with SeqSet(T.make_set()) as s:
        yield s


def test_hits_and_best_on_top(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    n = len(sset)
    blk = upper(0, n)
    full = sset.hits(m, d, e, F_MIN, blk, semantics=sem)
    full_idx, full_f = full.index.copy(), full.f.copy()
    by_bitmaps = sset.prefilter(*K3, block=blk, **SELECTIVE)
    want_list = as_lists(by_bitmaps)
    want_held = P.held_bytes(by_bitmaps.hits(m, d, e, F_MIN, semantics=sem))[0]
    cand = sset.word_join(*K3, block=blk, **SELECTIVE)
    assert as_lists(cand) == want_list and 0 < len(cand) < sset.pairs(blk)
    held = cand.hits(m, d, e, F_MIN, semantics=sem)
    assert len(held) > 0 and P.held_bytes(held)[0] == want_held
    rows = np.isin(full_idx, cand.index)
    assert held.index.tolist() == full_idx[rows].tolist() and (T.bits(held.f) == T.bits(full_f[rows])).all()     # what SeqSet.hits holds for those pairs
    sq = rectangle(0, n, 0, n)
    want_best = P.held_bytes(sset.prefilter(*K3, block=sq, **SELECTIVE).best(m, d, e, 2, skip_self=True, semantics=sem))[0]
    best = sset.word_join(*K3, block=sq, **SELECTIVE).best(m, d, e, 2, skip_self=True, semantics=sem)
    assert len(best) > 0 and P.held_bytes(best)[0] == want_best


def test_state(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    blk = upper(0, len(sset))
    held = sset.hits(m, d, e, F_MIN, blk, semantics=sem)
    before = P.held_bytes(held)[0]
    # word_index and word_join leave the held pass alone
    sset.word_index(2, 20)
    assert P.held_bytes(held)[0] == before
    cand = sset.word_join(*K3, block=blk, **SELECTIVE)
    listed = as_lists(cand)
    assert P.held_bytes(held)[0] == before and len(cand) > 0
    # a bitmap index after the word index drops the list (as ever) and leaves the word index usable, and the reverse
    sset.kmer_index(*K3)
    idx = np.zeros(1, dtype=np.uint64)
    w = np.zeros(3, dtype=np.uint32)
    assert sset.lib.aln_seqset_candidates(sset.handle, 0, 0, idx.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    count = C.c_uint64(0)
    spec = _ffi.WordjoinSpec(K3[0], K3[1], SELECTIVE["min_shared"], SELECTIVE["min_per_1024"], 0, 0, 0)
    assert sset.lib.aln_seqset_word_join(sset.handle, C.byref(spec), C.byref(blk), C.byref(count)) == _ffi.OK
    assert as_lists(Candidates(sset, int(count.value))) == listed
    sset.word_index(4, 20)
    pspec = _ffi.PrefilterSpec(K3[0], K3[1], SELECTIVE["min_shared"], SELECTIVE["min_per_1024"], 0, 0, 0)
    assert sset.lib.aln_seqset_candidates(sset.handle, 0, 0, idx.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert sset.lib.aln_seqset_prefilter(sset.handle, C.byref(pspec), C.byref(blk), C.byref(count)) == _ffi.OK
    assert as_lists(Candidates(sset, int(count.value))) == listed
    assert P.held_bytes(held)[0] == before
    # the list survives score, hits and best
    sset.score(m, d, e, rectangle(*T.RECT), semantics=sem)
    sset.best(m, d, e, 2, block=rectangle(*T.RECT), semantics=sem)
    assert as_lists(Candidates(sset, len(listed[0]))) == listed


def test_refusals_leave_both_states_intact(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    lib, hnd = sset.lib, sset.handle
    n = len(sset)
    blk = upper(0, n)
    cand = sset.word_join(*K3, block=blk, **SELECTIVE)
    held = sset.hits(m, d, e, F_MIN, rectangle(*T.RECT), semantics=sem)
    held_before = P.held_bytes(held)[0]
    INV = _ffi.ERR_INVALID_ARGUMENT
    count = C.c_uint64(77)
    words = np.full(n, 7, dtype=np.uint32)

    def spec(k=K3[0], alphabet=K3[1], min_shared=1, per=0, chunk=0, flags=0, reserved=0):
        return _ffi.WordjoinSpec(k, alphabet, min_shared, per, chunk, flags, reserved)

    def intact():
        return (count.value == 77 and (words == 7).all() and as_lists(Candidates(sset, len(cand))) == as_lists(cand)
                and P.held_bytes(held)[0] == held_before)

    for k, alphabet in ((0, 20), (9, 4), (8, 20), (8, 17), (3, 0), (2, 65537), (1, 0)):
        assert lib.aln_seqset_word_index(hnd, k, alphabet, words.ctypes.data) == INV and intact()
        assert lib.aln_seqset_word_join(hnd, C.byref(spec(k, alphabet)), C.byref(blk), C.byref(count)) == INV and intact()
    bad_specs = [spec(k=2), spec(alphabet=4), spec(min_shared=0), spec(per=1025), spec(flags=1), spec(reserved=1), spec(chunk=(1 << 26) + 1)]
    for sp in bad_specs:
        assert lib.aln_seqset_word_join(hnd, C.byref(sp), C.byref(blk), C.byref(count)) == INV and intact()
    for bb in (_ffi.SeqsetBlock(0, n + 1, 0, n + 1, 1, 0), _ffi.SeqsetBlock(0, 3, 1, 3, 1, 0), _ffi.SeqsetBlock(0, 0, 0, 3, 0, 0), _ffi.SeqsetBlock(0, 3, 0, 3, 0, 1)):
        assert lib.aln_seqset_word_join(hnd, C.byref(spec()), C.byref(bb), C.byref(count)) == INV and intact()
    assert lib.aln_seqset_word_join(hnd, None, C.byref(blk), C.byref(count)) == INV and intact()
    assert lib.aln_seqset_word_join(hnd, C.byref(spec()), None, C.byref(count)) == INV and intact()
    assert lib.aln_seqset_word_join(hnd, C.byref(spec()), C.byref(blk), None) == INV and intact()
    widest = spec(min_shared=SELECTIVE["min_shared"], per=SELECTIVE["min_per_1024"], chunk=1 << 26)       # the largest chunk is taken
    assert lib.aln_seqset_word_join(hnd, C.byref(widest), C.byref(blk), C.byref(count)) == _ffi.OK and count.value == len(cand)
    count.value = 77
    # no word index at all: a fresh set, even one with a bitmap index of the same (k, A); and the old refusals of the bitmap route stand
    with SeqSet(T.make_set()[:4]) as fresh:
        small = upper(0, 4)
        assert lib.aln_seqset_word_join(fresh.handle, C.byref(spec()), C.byref(small), C.byref(count)) == INV
        fresh.kmer_index(*K3)
        assert lib.aln_seqset_word_join(fresh.handle, C.byref(spec()), C.byref(small), C.byref(count)) == INV
        assert lib.aln_seqset_kmer_index(fresh.handle, 5, 20, None) == INV
        assert lib.aln_seqset_word_index(fresh.handle, 5, 20, None) == _ffi.OK     # n_words is optional
    assert intact()


# ---------------------------------------------------------------- the C99 caller
def hexf(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def protein_families(seed=5):
    """40 records of standard residues in 8 families: related enough to share 5-mers and to align well"""
    seqs, _ = family_set(5, 20, 8, 5, seed, length=(60, 160), rate=0.1)
    return [s for s in seqs[:40]]


def test_through_c(tmp_path):
    """tests/abi_wordjoin.c: the two exports, and the candidate calls on their result, from C99 on buffers of exactly the documented
    sizes, each followed by a guard zone"""
    from aligner_amd.matrices import get_blosum62
    m = get_blosum62()
    seqs = protein_families()
    k, a, min_shared, per, chunk = 5, 20, 2, 32, 2000
    tok = [len(seqs)] + [len(s) for s in seqs] + [int(c) for s in seqs for c in s] + [m.shape[0], m.shape[1]]
    tok += [hexf(v) for v in np.asarray(m, dtype=np.float64).ravel()] + [hexf(11.0), hexf(2.0), hexf(F_MIN), 98]
    tok += [k, a, min_shared, per, chunk]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(x) for x in tok) + "\n")
    exe = native_build.build_wordjoin_harness()
    out = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1] for l in lines if l[0] == "rc"] == ["seqset_create", "word_index", "word_join", "candidates", "candidate_hits", "held_list"]
    assert all(l[2] == "0" for l in lines if l[0] == "rc") and ["guards", "ok"] in lines
    want = R.word_join(seqs, k, a, min_shared, per, (0, len(seqs), 0, len(seqs), 1))
    assert [l[1:] for l in lines if l[0] == "n_words"] == [[str(len(R.words(s, k, a))) for s in seqs]]
    assert [l[1] for l in lines if l[0] == "count"] == [str(len(want[0]))] and len(want[0]) > 20
    assert [l[1:] for l in lines if l[0] == "cand"] == [[str(i), str(q), str(t), str(s)] for i, q, t, s in zip(*want)]
    with SeqSet(seqs) as ss:
        held = ss.word_join(k, a, min_shared=min_shared, min_per_1024=per).hits(m, 11.0, 2.0, F_MIN)
        assert [l[1] for l in lines if l[0] == "held"] == [str(len(held))] and len(held) > 0
        assert [l[1:] for l in lines if l[0] == "hit"] == [[str(int(i)), str(int(q)), str(int(t)), hexf(v)] for i, q, t, v in zip(held.index, held.q, held.t, held.f)]


# ---------------------------------------------------------------- the command
def test_the_command(tmp_path, capsys):
    from aligner_amd import allpairs
    from aligner_amd.enums import Protein
    from aligner_amd.matrices import get_blosum62
    seqs = protein_families()
    letters = Protein.letters
    fa = tmp_path / "x.fasta"
    fa.write_text("".join(">s%d\n%s\n" % (i, "".join(letters[int(c)] for c in s)) for i, s in enumerate(seqs)))
    m = get_blosum62()
    n = len(seqs)
    args = ["-i", str(fa), "--kmer", "5", "--word-join", "--min-shared", "2"]
    idx, q, t, sh = R.word_join(seqs, 5, 20, 2, 0, (0, n, 0, n, 1))
    assert 20 < len(idx) < n * (n - 1) // 2
    with SeqSet(seqs) as ss:
        f, status = ss.score(m, 11.0, 2.0, None)
        full = ss.hits(m, 11.0, 2.0, F_MIN, None)
        rows = [h for h in range(len(full)) if int(full.index[h]) in set(idx)]
        assert allpairs.main(args) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%r,%d" % (x, y, float(f[kk]), s) for kk, x, y, s in zip(idx, q, t, sh)]
        assert allpairs.main(args + ["--f-min", repr(F_MIN)]) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%r" % (int(full.q[h]), int(full.t[h]), float(full.f[h])) for h in rows] and len(out) > 0
        # --min-shared defaults to 1 on this route
        assert allpairs.main(["-i", str(fa), "--kmer", "5", "--word-join", "--f-min", repr(F_MIN)]) == 0
        out1 = capsys.readouterr().out.splitlines()
        ones = set(R.word_join(seqs, 5, 20, 1, 0, (0, n, 0, n, 1))[0])
        assert out1 == ["s%d,s%d,%r" % (int(full.q[h]), int(full.t[h]), float(full.f[h])) for h in range(len(full)) if int(full.index[h]) in ones]
        # --best-candidates: the rows of the same question asked through the library
        assert allpairs.main(args + ["--best-candidates", "2"]) == 0
        out = capsys.readouterr().out.splitlines()
        best = ss.word_join(5, 20, min_shared=2, block=rectangle(0, n, 0, n)).best(m, 11.0, 2.0, 2, skip_self=True)
        want = ["s%d,%d,s%d,%r" % (qq, int(best.rank[p]) + 1, int(best.t[p]), float(best.f[p])) for qq, pos in best.by_query() for p in pos]
        assert out == want and len(out) > 0
    # where both routes apply the command prints the same rows
    both = ["-i", str(fa), "--kmer", "4", "--min-shared", "2", "--min-shared-per-1024", "32", "--f-min", repr(F_MIN)]
    assert allpairs.main(both) == 0
    by_bitmaps = capsys.readouterr().out
    assert allpairs.main(both + ["--word-join"]) == 0
    assert capsys.readouterr().out == by_bitmaps and len(by_bitmaps) > 0
