"""The held store (struct HeldStore, aln_host.hip): a sequence set's held hits and a pair set's held run are fetched through one path
with one contract.  The same pairs are held both ways -- SeqSet.hits over a rectangle, PairSet.from_seqset + run with the one shared
matrix for every pair -- and aln_seqset_held_strings / aln_pairset_strings are called raw, in three layouts: summaries and both
strings are the CPU oracle's, byte for byte the same from both families; the capacity bytes beyond aln_len and both strings of a
failed entry come back as zeros, bytes between the entries' spans are left alone, and a refused fetch leaves its outputs alone.

Eight protein sequences: lengths 1, 2, 63, 64, 65, 300, 301 (the smallest shapes that can be held, the 64-lane strip boundary, and a
300 x 301 pair whose aln_len exceeds the gather's 256-thread stride, so its strided loop runs twice) and one that ends in a code
outside the 24 x 24 matrix, so every pair with it fails.  BLOSUM62, 11 / 2, core local.  The oracle's answers are computed once."""
import ctypes as C

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd.batch import RESULT_DTYPE
from aligner_amd.matrices import get_blosum62
from aligner_amd.pairset import PairSet
from aligner_amd.seqset import SeqSet, rectangle

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 300, 301]
S = len(LENGTHS) + 1
BAD = S - 1
DEL, EXT = 11.0, 2.0
FIELDS = ["f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status"]      # (passes / flags: route diagnostics)
FILL = 0xAB


def make_set():
    """Every sequence holds residue 0 (A: 4 against itself), so every pair of the first seven has a positive cell; the 301 is the 300
    with substitutions and one inserted residue, so that pair's alignment runs over nearly all of both."""
    rng = np.random.default_rng(20261019)
    seqs = []
    for n in LENGTHS[:-1]:
        s = rng.integers(0, 20, n).astype(np.uint8)
        s[0] = 0
        seqs.append(s)
    long_ = seqs[-1].copy()
    mut = rng.random(300) < 0.15
    mut[0] = False
    long_[mut] = rng.integers(0, 20, int(mut.sum()))
    seqs.append(np.concatenate([long_[:150], [7], long_[150:]]).astype(np.uint8))
    bad = rng.integers(0, 20, 40).astype(np.uint8)
    bad[0], bad[-1] = 0, 24
    seqs.append(bad)
    assert [len(s) for s in seqs] == LENGTHS + [40]
    return seqs


_oracle = {}


def oracle(orc):
    """(q, t) -> the oracle's answer, once; the inputs are checked here, on the CPU, before anything is asked of the device."""
    if not _oracle:
        seqs, m = make_set(), get_blosum62()
        for q in range(S):
            for t in range(S):
                o = orc.align(_ffi.CORE_LOCAL, seqs[q], seqs[t], DEL, EXT, m)
                if q == BAD or t == BAD:
                    assert o["status"] == _ffi.ERR_CODE_OUT_OF_RANGE, (q, t)
                else:
                    assert o["status"] == _ffi.OK and o["f"] > 0 and len(o["qa"]) >= 1, (q, t)       # a positive cell: the pair is held
                _oracle[(q, t)] = o
        assert len(_oracle[(5, 6)]["qa"]) > 256 and len(_oracle[(6, 5)]["qa"]) > 256
    return _oracle


class Family:
    """One family's raw fetch: `positions` are this family's own (held positions of a set, pair numbers of a pair set); pair[i] is
    the (q, t) behind position i."""

    def __init__(self, name, fn, handle, count, pair):
        self.name, self.fn, self.handle, self.count, self.pair = name, fn, handle, count, pair

    def caps(self, positions):
        lens = LENGTHS + [40]
        return [lens[self.pair[p][0]] + lens[self.pair[p][1]] + 2 for p in positions]

    def fetch(self, positions, off, size, with_tb=True):
        w = np.ascontiguousarray(positions, dtype=np.uint32)
        res = np.zeros(len(w), dtype=RESULT_DTYPE)
        res.view(np.uint8)[:] = FILL
        tb = np.full(max(size, 1), FILL, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        st = self.fn(self.handle, w.ctypes.data, len(w), res.ctypes.data, tb.ctypes.data if with_tb else None, off.ctypes.data if with_tb else None)
        return st, res, tb


def layouts(caps):
    """name -> (tb_off, bytes): the documented cumulative layout, and the entries' spans in a shuffled order with gaps between them"""
    cum = np.concatenate([[0], np.cumsum([2 * c for c in caps])[:-1]]).astype(np.uint64) if caps else np.zeros(0, dtype=np.uint64)
    order = np.random.default_rng(7).permutation(len(caps))
    off, pos = np.zeros(len(caps), dtype=np.uint64), 3
    for k in order:
        off[k] = pos
        pos += 2 * caps[k] + 5 + int(k) % 3
    return {"cumulative": (cum, int(sum(2 * c for c in caps))), "shuffled": (off, pos)}


def expected_tb(orc_of, fam, positions, off, size):
    """What the caller's buffer must hold: the fill byte wherever no entry's span lies, and per entry 2 * cap bytes: the oracle's strings
    at 0 and at cap, zeros in the rest -- all zeros for a failed entry."""
    want = np.full(max(size, 1), FILL, dtype=np.uint8)
    for k, (p, cap) in enumerate(zip(positions, fam.caps(positions))):
        o, a = orc_of[fam.pair[p]], int(off[k])
        want[a:a + 2 * cap] = 0
        if o["status"] == _ffi.OK:
            want[a:a + len(o["qa"])] = o["qa"]
            want[a + cap:a + cap + len(o["ta"])] = o["ta"]
    return want


def check_results(orc_of, fam, positions, res):
    for k, p in enumerate(positions):
        o, r = orc_of[fam.pair[p]], res[k]
        assert r["status"] == o["status"], (fam.name, p)
        if o["status"] == _ffi.OK:
            assert (r["f"], r["score"], r["aln_len"]) == (o["f"], o["score"], len(o["qa"])), (fam.name, p)
            assert (r["end_y"], r["end_x"], r["start_y"], r["start_x"]) == (*o["end"], *o["start"]), (fam.name, p)


@pytest.fixture(scope="module")
def held(orc):
    """Both families holding the rectangle of all pairs: (oracle answers, the set's family, the pair set's family, set position -> pair
    number)."""
    orc_of = oracle(orc)
    seqs, m = make_set(), get_blosum62()
    block = rectangle(0, S, 0, S)
    with SeqSet(seqs) as ss:
        hits = ss.hits(m, DEL, EXT, float("-inf"), block)
        ok = [(q, t) for q in range(S) for t in range(S) if q != BAD and t != BAD]
        assert [(int(q), int(t)) for q, t in zip(hits.q, hits.t)] == ok          # the failed pairs are no hits
        with PairSet.from_seqset(ss, block) as ps:
            res = ps.run(_ffi.CORE_LOCAL, DEL, EXT, np.broadcast_to(m, (S * S,) + m.shape), np.arange(S * S, dtype=np.uint32))
            all_pairs = [(q, t) for q in range(S) for t in range(S)]
            assert [int(s) for s in res["status"]] == [orc_of[p]["status"] for p in all_pairs]
            lib = ss.lib
            fam_set = Family("seqset", lib.aln_seqset_held_strings, ss.handle, len(hits), ok)
            fam_pair = Family("pairset", lib.aln_pairset_strings, ps.handle, S * S, all_pairs)
            yield orc_of, fam_set, fam_pair, [int(i) for i in hits.index]


def test_both_families_fetch_the_oracles_strings_in_every_layout(held):
    orc_of, fam_set, fam_pair, number = held
    # every held hit in reverse order, one position listed twice; the pair set is asked for the same pairs
    listed = list(range(fam_set.count))[::-1] + [fam_set.count - 2]
    got = {}
    for fam, positions in ((fam_set, listed), (fam_pair, [number[h] for h in listed])):
        for name, (off, size) in layouts(fam.caps(positions)).items():
            st, res, tb = fam.fetch(positions, off, size)
            assert st == _ffi.OK, (fam.name, name)
            check_results(orc_of, fam, positions, res)
            want = expected_tb(orc_of, fam, positions, off, size)
            assert (tb == want).all(), (fam.name, name, np.flatnonzero(tb != want)[:8])
            got[(fam.name, name)] = (res, tb)
        st, res, tb = fam.fetch(positions, [], 16, with_tb=False)
        assert st == _ffi.OK and (tb == FILL).all()
        check_results(orc_of, fam, positions, res)
        got[(fam.name, "null")] = (res, tb)
    for name in ("cumulative", "shuffled", "null"):
        (res_s, tb_s), (res_p, tb_p) = got[("seqset", name)], got[("pairset", name)]
        for fld in FIELDS:
            assert res_s[fld].tobytes() == res_p[fld].tobytes(), (name, fld)
        assert tb_s.tobytes() == tb_p.tobytes(), name


def test_a_failed_entry_of_a_pair_set_reads_zero(held):
    orc_of, _, fam_pair, _ = held
    positions = [BAD * S + 5, 5 * S + 6, 6 * S + BAD, 0]          # failed, the long pair, failed, 1 x 1
    for name, (off, size) in layouts(fam_pair.caps(positions)).items():
        st, res, tb = fam_pair.fetch(positions, off, size)
        assert st == _ffi.OK
        check_results(orc_of, fam_pair, positions, res)
        assert res["status"][0] == res["status"][2] == _ffi.ERR_CODE_OUT_OF_RANGE
        assert (tb == expected_tb(orc_of, fam_pair, positions, off, size)).all(), name


def test_a_short_fetch_after_a_long_one_reads_zero_beyond_its_length(held):
    """The packed span on the device still holds the long pair's strings when the short pair is packed at the same position."""
    orc_of, fam_set, fam_pair, number = held
    long_h, short_h = number.index(5 * S + 6), number.index(0 * S + 1)
    for fam, long_p, short_p in ((fam_set, long_h, short_h), (fam_pair, number[long_h], number[short_h])):
        for name in ("cumulative", "shuffled"):
            for p in (long_p, short_p):
                off, size = layouts(fam.caps([p]))[name]
                st, res, tb = fam.fetch([p], off, size)
                assert st == _ffi.OK
                check_results(orc_of, fam, [p], res)
                assert (tb == expected_tb(orc_of, fam, [p], off, size)).all(), (fam.name, name, p)
            assert int(res["aln_len"][0]) < fam.caps([short_p])[0]          # there are bytes beyond aln_len to speak of


def test_a_position_beyond_the_count_is_refused_and_nothing_is_written(held):
    _, fam_set, fam_pair, _ = held
    for fam in (fam_set, fam_pair):
        positions = [0, fam.count]
        for with_tb in (True, False):
            st, res, tb = fam.fetch(positions, [0, 64], 256, with_tb=with_tb)
            assert st == _ffi.ERR_INVALID_ARGUMENT, fam.name
            assert (res.view(np.uint8) == FILL).all() and (tb == FILL).all(), fam.name
