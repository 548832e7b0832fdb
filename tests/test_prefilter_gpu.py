"""The k-mer prefilter of a resident sequence set on the GPU (aln_seqset_kmer_index / _prefilter / _candidates / _candidate_scores /
_candidate_hits): the index and the sharing kernel against prefilter_ref.py, whole lists compared; the candidate passes against the
unfiltered passes of the same set, bit for bit; state and refusals; the C99 caller; the command.  Every comparison is on integers
or on bits.

The sharing kernel's tile is 16 queries x 256 targets (ALN_PF_QT x ALN_PF_TT, aligner_amd/csrc/aln_prefilter.hip), the selection's
tile 2048 pairs (aln_select.h), its offsets kernel's trip 256 tiles = 524 288 pairs."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prefilter_ref as R                                                       # noqa: E402
import test_seqset_gpu as T                                                     # noqa: E402
from aligner_amd import _ffi, runtime                                           # noqa: E402
from aligner_amd import build as native_build                                   # noqa: E402
from aligner_amd import cluster as cluster_mod                                  # noqa: E402
from aligner_amd.batch import RESULT_DTYPE                                      # noqa: E402
from aligner_amd.seqset import SeqSet, rectangle, upper                         # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QT, TT = 16, 256                 # the sharing kernel's tile


def blk_tuple(b):
    return (int(b.q_first), int(b.q_count), int(b.t_first), int(b.t_count), int(b.upper))


def check_list(cand, want):
    idx, q, t, sh = want
    assert len(cand) == len(idx)
    assert cand.index.tolist() == list(idx) and cand.q.tolist() == list(q) and cand.t.tolist() == list(t) and cand.shared.tolist() == list(sh)


# ---------------------------------------------------------------- the index
def index_set(k, a):
    rng = np.random.default_rng(1000 * k + a)
    seqs = [rng.integers(0, a, n).astype(np.uint8) for n in (0, 1, k - 1, k, k + 1, 255, 256, 257, 1025)]
    every = rng.integers(0, a, 50).astype(np.uint8)
    every[k - 1::k] = a                                   # a code >= A inside every window
    one = rng.integers(0, a, 40).astype(np.uint8)
    one[0] = 98                                           # ... in the first window only
    homo = np.full(30, a - 1, dtype=np.uint8)             # one word
    twin = rng.integers(0, a, 100).astype(np.uint8)
    return seqs + [every, one, homo, twin, twin.copy()]


@pytest.mark.parametrize("k,a", [(2, 4), (3, 5), (4, 20)])
def test_index_and_shared_counts(k, a):
    """(3, 5): 125 bits, a ragged last element; (4, 20): 160 000 bits, the large bitmap, several staged slices in the sharing kernel."""
    seqs = index_set(k, a)
    sets = [R.words(s, k, a) for s in seqs]
    assert len(sets[9]) == 0 and len(sets[11]) == 1 and len(sets[10]) == len(R.words(seqs[10][1:], k, a)) > 0 and sets[12] == sets[13]
    with SeqSet(seqs) as ss:
        n_words = ss.kmer_index(k, a)
        assert n_words.tolist() == [len(w) for w in sets]
        for b in (upper(0, len(seqs)), rectangle(2, 11, 0, 14)):
            cand = ss.prefilter(k, a, block=b)            # thresholds 0: every pair, with its shared count
            assert len(cand) == ss.pairs(b)
            check_list(cand, R.prefilter(seqs, k, a, 0, 0, blk_tuple(b)))
        cand = ss.prefilter(k, a, min_shared=1, min_per_1024=512)
        check_list(cand, R.prefilter(seqs, k, a, 1, 512, (0, len(seqs), 0, len(seqs), 1)))
        assert 0 < len(cand) < ss.pairs()


# ---------------------------------------------------------------- sharing and compaction across tiles
N_TILES = 726
MARKS = ([1, 2, 3, 1], [1, 2, 3], [0, 1, 2, 3], [1, 2, 3, 3])       # words over A = 4, k = 2: 12 23 31 | 12 23 | 01 12 23 | 12 23 33: any two share 2 or 3
TILE_BLOCKS = [(0, N_TILES, 0, N_TILES, 0), (0, N_TILES, 0, N_TILES, 1)] + \
              [(3, qc, 5, tc, 0) for qc in (QT - 1, QT, QT + 1) for tc in (TT - 1, TT, TT + 1)]
EDGE_PAIRS = (2047, 2048, 524287, 524288)


def tiles_case():
    """726 sequences of 'A' (code 0) repeated one to three times, one empty, and marked ones: every sequence of a pair whose number
    sits on a selection-tile edge, on the 256-tile edge or in the last tile of one of the blocks carries a mark."""
    marked = set()
    for b in TILE_BLOCKS:
        pairs = R.block_pairs(b)
        for kk in EDGE_PAIRS + (len(pairs) - 1, len(pairs) - 2):
            if 0 <= kk < len(pairs):
                marked.update(pairs[kk])
    seqs = []
    for i in range(N_TILES):
        seqs.append(np.array(MARKS[i % 4] if i in marked else [0] * (1 + i % 3), dtype=np.uint8))
    seqs[400] = np.zeros(0, dtype=np.uint8)
    assert 400 not in marked
    return seqs


_tiles_ref = {}


def tiles_reference(seqs, b, min_shared, min_per_1024):
    """shared by table lookup: the 16-bit bitmaps of prefilter_ref, ANDed and counted with numpy; the predicate in int64."""
    if "masks" not in _tiles_ref:
        sets = [R.words(s, 2, 4) for s in seqs]
        _tiles_ref["masks"] = np.array([R.bitmap(w, 2, 4)[0] for w in sets], dtype=np.int64)
        _tiles_ref["n"] = np.array([len(w) for w in sets], dtype=np.int64)
        _tiles_ref["pop"] = np.array([bin(v).count("1") for v in range(1 << 16)], dtype=np.int64)
    masks, n, pop = _tiles_ref["masks"], _tiles_ref["n"], _tiles_ref["pop"]
    pairs = np.array(R.block_pairs(b), dtype=np.int64)
    q, t = pairs[:, 0], pairs[:, 1]
    sh = pop[masks[q] & masks[t]]
    keep = (sh >= min_shared) & (sh * 1024 >= min_per_1024 * np.minimum(n[q], n[t]))
    idx = np.flatnonzero(keep)
    return idx, q[idx], t[idx], sh[idx]


@pytest.fixture(scope="module")
def tiles_set():
    seqs = tiles_case()
    with SeqSet(seqs) as ss:
        n_words = ss.kmer_index(2, 4)
        assert n_words.tolist() == [len(R.words(s, 2, 4)) for s in seqs]
        yield ss, seqs


@pytest.mark.parametrize("b", TILE_BLOCKS, ids=lambda b: "%dx%d%s" % (b[1], b[3], "u" if b[4] else ""))
def test_sharing_and_compaction_across_tiles(tiles_set, b):
    ss, seqs = tiles_set
    blk = _ffi.SeqsetBlock(b[0], b[1], b[2], b[3], b[4], 0)
    pairs = ss.pairs(blk)
    for min_shared, per in ((2, 0), (1, 1024)):
        want = tiles_reference(seqs, b, min_shared, per)
        cand = ss.prefilter(2, 4, min_shared=min_shared, min_per_1024=per, block=blk)
        check_list(cand, want)
        assert 0 < len(cand) < pairs
        chunks = 1
        assert ss.stats()["bytes_down"] == 12 * len(cand) + 8 * chunks
        if min_shared == 2:
            have = set(want[0].tolist())
            for kk in EDGE_PAIRS + (pairs - 1,):
                assert kk >= pairs or kk in have, kk                  # candidates on both sides of 2047 | 2048 and 524 287 | 524 288
            assert max(have) // 2048 == (pairs - 1) // 2048         # and in the last tile
    if pairs > 100003:
        cand = ss.prefilter(2, 4, min_shared=2, block=blk, chunk_pairs=100003)          # no multiple of any tile
        check_list(cand, tiles_reference(seqs, b, 2, 0))
        assert ss.stats()["bytes_down"] == 12 * len(cand) + 8 * ((pairs + 100002) // 100003)
    # thresholds 0: every pair of the block, shared exposed for each
    if pairs <= 100003:
        cand = ss.prefilter(2, 4, block=blk, chunk_pairs=1000)
        check_list(cand, tiles_reference(seqs, b, 0, 0))
        assert len(cand) == pairs


# ---------------------------------------------------------------- agreement with the unfiltered pass
K3 = (3, 20)
SELECTIVE = dict(min_shared=2, min_per_1024=16)          # 18 of the upper block's 66 pairs by the reference
F_MIN = 30.0


@pytest.fixture(scope="module")
def sset():
    with SeqSet(T.make_set()) as s:
        yield s


def held_bytes(held):
    """the held list and the raw strings of every held hit"""
    res, strs = held.strings()
    h = hashlib.sha256()
    h.update(held.index.tobytes()); h.update(held.q.tobytes()); h.update(held.t.tobytes()); h.update(held.f.tobytes())
    for name in T.FIELDS:
        h.update(np.ascontiguousarray(res[name]).tobytes())
    for qa, ta in strs:
        h.update(qa.tobytes()); h.update(ta.tobytes())
    return h.hexdigest(), res, strs


@pytest.mark.parametrize("name", T.SCHEMES)
def test_thresholds_zero_equal_the_unfiltered_pass(sset, name):
    sem, m, d, e, kw = T.schemes()[name]
    for blk in (upper(0, len(sset)), rectangle(*T.RECT)):
        f, status = sset.score(m, d, e, blk, semantics=sem, **kw)
        f_min = float(np.median(f[status == 0]))                       # (a threshold some pairs of every scheme meet)
        full = sset.hits(m, d, e, f_min, blk, semantics=sem, **kw)
        want = held_bytes(full)[0]
        cand = sset.prefilter(*K3, block=blk)
        assert len(cand) == sset.pairs(blk) and cand.index.tolist() == list(range(len(cand)))
        cf, cstatus = cand.score(m, d, e, semantics=sem, **kw)
        assert (T.bits(cf) == T.bits(f)).all() and (cstatus == status).all()
        assert (status != 0).any() and (status == 0).any()            # per-pair failures travel
        held = cand.hits(m, d, e, f_min, semantics=sem, **kw)
        assert len(held) == len(full) > 0 and held_bytes(held)[0] == want


@pytest.mark.parametrize("name", T.SCHEMES)
def test_selective_thresholds_hold_the_candidates_rows(sset, name):
    sem, m, d, e, kw = T.schemes()[name]
    seqs = T.make_set()
    n = len(sset)
    blk = upper(0, n)
    want_idx, want_q, want_t, want_sh = R.prefilter(seqs, *K3, SELECTIVE["min_shared"], SELECTIVE["min_per_1024"], blk_tuple(blk))
    assert 0 < len(want_idx) < sset.pairs(blk)
    f, status = sset.score(m, d, e, blk, semantics=sem, **kw)
    ok_f = f[want_idx][status[want_idx] == 0]
    f_min = float(np.median(ok_f))                                     # (a threshold some candidates of every scheme meet)
    full = sset.hits(m, d, e, f_min, blk, semantics=sem, **kw)
    rows = np.flatnonzero(np.isin(full.index, np.array(want_idx, dtype=np.uint64))).astype(np.uint32)
    assert 0 < len(rows)
    full_res, full_strs = full.strings(rows)
    full_rep = full.report(m, keep=rows)
    full_idx, full_f = full.index[rows].copy(), full.f[rows].copy()
    cand = sset.prefilter(*K3, block=blk, **SELECTIVE)
    check_list(cand, (want_idx, want_q, want_t, want_sh))
    cf, cstatus = cand.score(m, d, e, semantics=sem, **kw)
    assert (T.bits(cf) == T.bits(f[cand.index.astype(np.int64)])).all() and (cstatus == status[cand.index.astype(np.int64)]).all()
    held = cand.hits(m, d, e, f_min, semantics=sem, **kw)
    assert held.index.tolist() == full_idx.tolist() and (T.bits(held.f) == T.bits(full_f)).all()
    res, strs = held.strings()
    for name_ in T.FIELDS:
        assert (np.ascontiguousarray(res[name_]).view(np.uint8) == np.ascontiguousarray(full_res[name_]).view(np.uint8)).all(), name_
    assert len(strs) == len(full_strs)
    for (qa, ta), (qb, tb) in zip(strs, full_strs):
        assert qa.tobytes() == qb.tobytes() and ta.tobytes() == tb.tobytes()
    assert held.report(m).tobytes() == full_rep.tobytes()
    # held_cluster on top: the sequences grouped by exactly those hits (the edge list given to the clustering family directly)
    ok = res["status"] == 0
    for mode in ("components", "greedy"):
        got = held.cluster(mode=mode)
        ref = cluster_mod.cluster_edges(n, held.q[ok], held.t[ok], lengths=sset.len.astype(np.uint32), mode=mode)
        assert got.label.tolist() == ref.label.tolist() and got.records.tobytes() == ref.records.tobytes()


def candidate_digest(sset):
    h = hashlib.sha256()
    chunks = []
    for name in T.SCHEMES:
        sem, m, d, e, kw = T.schemes()[name]
        for thresholds in ({}, SELECTIVE):
            cand = sset.prefilter(*K3, block=upper(0, len(sset)), **thresholds)
            f, status = cand.score(m, d, e, semantics=sem, **kw)
            chunks.append((sset.stats()["bytes_down"] - 12 * len(cand)) // 16)
            h.update(cand.index.tobytes()); h.update(f.tobytes()); h.update(status.tobytes())
            h.update(held_bytes(cand.hits(m, d, e, F_MIN, semantics=sem, **kw))[0].encode())
    return h.hexdigest(), chunks


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd.seqset import SeqSet
import test_prefilter_gpu as P
with SeqSet(P.T.make_set()) as s:
    digest, chunks = P.candidate_digest(s)
    print("DIGEST", digest, min(chunks[0::2]))
"""


def test_chunked_list_pass_is_byte_identical(sset):
    """ALN_CHUNK_CELLS = 250 000 (in a child: the other tests must not see it): each of the three pairs among the 512, 513 and 600 long
    sequences exceeds the bound alone, so the pass over the full candidate list runs in three or more list chunks."""
    env = dict(os.environ, ALN_CHUNK_CELLS="250000")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DIGEST" in out.stdout, out.stdout + out.stderr
    tok = out.stdout.split("DIGEST")[1].split()
    digest, chunks = candidate_digest(sset)
    assert tok[0] == digest
    assert int(tok[1]) >= 3 and max(chunks) == 1


def mixed_sources_run():
    """Block and candidate passes taking turns on one set (they share one pass loop, one pair of plans and one set of growing
    buffers), each result beside the same call made first on a set of its own.  A held pass is recorded as its list and the
    summaries and both strings of its first, last and three middle positions, a score pass as its f and statuses.
    -> {"pairs", "candidates", "calls": [[name, n and sha-256 on the fresh set, n and sha-256 in the sequence, bytes_up, bytes_down]]}"""
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    seqs = T.make_set()
    blk = rectangle(*T.RECT)
    calls = [("block best", lambda s, c: s.best(m, d, e, 3, block=blk, semantics=sem)),
             ("candidate best", lambda s, c: c.best(m, d, e, 3, semantics=sem)),
             ("block hits", lambda s, c: s.hits(m, d, e, F_MIN, blk, semantics=sem)),
             ("candidate hits", lambda s, c: c.hits(m, d, e, F_MIN, semantics=sem)),
             ("candidate score", lambda s, c: c.score(m, d, e, semantics=sem)),
             ("block score", lambda s, c: s.score(m, d, e, blk, semantics=sem))]

    def record(out):
        h = hashlib.sha256()
        if isinstance(out, tuple):
            f, status = out
            h.update(f.tobytes()); h.update(status.tobytes())
            return [len(f), h.hexdigest()]
        n = len(out)
        for a in (out.index, out.q, out.t, out.f):
            h.update(a.tobytes())
        res, strs = out.strings(np.array(sorted({0, n // 4, n // 2, 3 * n // 4, n - 1}) if n else [], dtype=np.uint32))
        for name in T.FIELDS:
            h.update(np.ascontiguousarray(res[name]).tobytes())
        for qa, ta in strs:
            h.update(qa.tobytes()); h.update(b"|"); h.update(ta.tobytes()); h.update(b"/")
        return [n, h.hexdigest()]

    fresh = []
    for name, call in calls:
        with SeqSet(seqs) as s:
            fresh.append(record(call(s, s.prefilter(*K3, block=blk, **SELECTIVE))))
    rows = []
    with SeqSet(seqs) as s:
        cand = s.prefilter(*K3, block=blk, **SELECTIVE)
        for (name, call), alone in zip(calls, fresh):
            out = call(s, cand)
            st = s.stats()                                            # (before record fetches strings: a fetch has stats of its own)
            rows.append([name, alone, record(out), st["bytes_up"], st["bytes_down"]])
        return dict(pairs=s.pairs(blk), candidates=len(cand), calls=rows)


MIXED_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_prefilter_gpu as P
print("MIXED", json.dumps(P.mixed_sources_run()))
"""

# bytes_up, bytes_down of the six calls of mixed_sources_run, in its order.  They are the parent commit's: the library built from the
# commit before the two pass loops became one ran mixed_sources_run once (ALN_CHUNK_CELLS = 250 000, the library named by ALN_LIB).
# (Both score passes: 12 bytes per position and 16 per chunk down, so 8 chunks each.)
MIXED_BYTES = [(4244, 472), (3924, 424), (5504, 704), (5016, 624), (2412, 500), (2480, 716)]


def test_block_and_candidate_passes_take_turns_on_one_set():
    """ALN_CHUNK_CELLS = 250 000 in a child, as above, so that every pass runs in several chunks and its plans and buffers are the
    ones the pass before it (over the other kind of source) left behind."""
    env = dict(os.environ, ALN_CHUNK_CELLS="250000")
    code = MIXED_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MIXED" in out.stdout, out.stdout + out.stderr
    got = json.loads(out.stdout.split("MIXED")[1])
    print(got)
    assert 0 < got["candidates"] < got["pairs"] == 49
    assert [r[0] for r in got["calls"]] == ["block best", "candidate best", "block hits", "candidate hits", "candidate score", "block score"]
    for name, alone, mixed, up, down in got["calls"]:
        assert mixed == alone and alone[0] > 0, name
    assert got["calls"][4][1][0] == got["candidates"] and got["calls"][5][1][0] == got["pairs"]
    assert (got["calls"][4][4] - 12 * got["candidates"]) // 16 >= 3 and (got["calls"][5][4] - 12 * got["pairs"]) // 16 >= 3      # chunks
    assert [(r[3], r[4]) for r in got["calls"]] == MIXED_BYTES


# ---------------------------------------------------------------- state
def test_candidate_state_and_held_state_are_separate(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    blk = upper(0, len(sset))
    held = sset.hits(m, d, e, F_MIN, blk, semantics=sem)
    before = held_bytes(held)[0]
    # kmer_index, prefilter and candidates leave the held pass alone
    sset.kmer_index(2, 20)
    assert held_bytes(held)[0] == before
    cand = sset.prefilter(*K3, block=blk, **SELECTIVE)
    again = type(cand)(sset, len(cand))
    assert held_bytes(held)[0] == before and again.index.tolist() == cand.index.tolist()
    listed = cand.index.copy(), cand.shared.copy()
    # the candidate list survives score, hits and best
    sset.score(m, d, e, rectangle(*T.RECT), semantics=sem)
    sset.hits(m, d, e, F_MIN, rectangle(*T.RECT), semantics=sem)
    sset.best(m, d, e, 2, block=rectangle(*T.RECT), semantics=sem)
    again = type(cand)(sset, len(cand))
    assert again.index.tolist() == listed[0].tolist() and again.shared.tolist() == listed[1].tolist()
    got = cand.hits(m, d, e, F_MIN, semantics=sem)
    assert set(got.index.tolist()) <= set(listed[0].tolist()) and len(got) > 0
    # a new index drops it
    sset.kmer_index(*K3)
    idx = np.zeros(1, dtype=np.uint64)
    w = np.zeros(3, dtype=np.uint32)
    assert sset.lib.aln_seqset_candidates(sset.handle, 0, 0, idx.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    f = np.zeros(1)
    p, keep = runtime.make_params(sem, d, e, m, outputs=_ffi.OUT_SCORE)
    assert sset.lib.aln_seqset_candidate_scores(sset.handle, C.byref(p), f.ctypes.data, None) == _ffi.ERR_INVALID_ARGUMENT
    assert held_bytes(got)[0]                                        # the held hits of the candidate pass are still there


def test_refusals_leave_both_states_intact(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    lib, hnd = sset.lib, sset.handle
    n = len(sset)
    blk = upper(0, n)
    cand = sset.prefilter(*K3, block=blk, **SELECTIVE)
    held = sset.hits(m, d, e, F_MIN, rectangle(*T.RECT), semantics=sem)
    held_before = held_bytes(held)[0]
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    count = C.c_uint64(77)
    words = np.full(n, 7, dtype=np.uint32)
    idx = np.full(len(cand) + 1, 5, dtype=np.uint64)
    a, b, c = (np.full(len(cand) + 1, 5, dtype=np.uint32) for _ in range(3))
    f = np.full(len(cand), 1.5)
    status = np.full(len(cand), 9, dtype=np.int32)
    p, keep = runtime.make_params(sem, d, e, m)
    pwm, keep2 = runtime.make_params(_ffi.PWM_LOCAL, d, e, np.ascontiguousarray(m[:, :8]))

    def spec(k=3, alphabet=20, min_shared=0, per=0, chunk=0, flags=0, reserved=0):
        return _ffi.PrefilterSpec(k, alphabet, min_shared, per, chunk, flags, reserved)

    def intact():
        again = type(cand)(sset, len(cand))
        return (count.value == 77 and (words == 7).all() and (idx == 5).all() and (a == 5).all() and (b == 5).all() and (c == 5).all() and (f == 1.5).all()
                and (status == 9).all() and again.index.tolist() == cand.index.tolist() and again.shared.tolist() == cand.shared.tolist()
                and held_bytes(held)[0] == held_before)

    for k, alphabet in ((0, 20), (9, 4), (5, 20), (3, 0), (1, (1 << 18) + 1)):
        assert lib.aln_seqset_kmer_index(hnd, k, alphabet, words.ctypes.data) == INV and intact()
        assert lib.aln_seqset_prefilter(hnd, C.byref(spec(k, alphabet)), C.byref(blk), C.byref(count)) == INV and intact()
    bad_specs = [spec(k=2), spec(alphabet=4), spec(per=1025), spec(flags=1), spec(reserved=1), spec(chunk=(1 << 22) + 1)]
    for sp in bad_specs:
        assert lib.aln_seqset_prefilter(hnd, C.byref(sp), C.byref(blk), C.byref(count)) == INV and intact()
    for bb in (_ffi.SeqsetBlock(0, n + 1, 0, n + 1, 1, 0), _ffi.SeqsetBlock(0, 3, 1, 3, 1, 0), _ffi.SeqsetBlock(0, 0, 0, 3, 0, 0), _ffi.SeqsetBlock(0, 3, 0, 3, 0, 1)):
        assert lib.aln_seqset_prefilter(hnd, C.byref(spec()), C.byref(bb), C.byref(count)) == INV and intact()
    assert lib.aln_seqset_prefilter(hnd, None, C.byref(blk), C.byref(count)) == INV and intact()
    assert lib.aln_seqset_prefilter(hnd, C.byref(spec()), None, C.byref(count)) == INV and intact()
    assert lib.aln_seqset_prefilter(hnd, C.byref(spec()), C.byref(blk), None) == INV and intact()
    assert lib.aln_seqset_candidates(hnd, 1, len(cand), idx.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data) == INV and intact()
    assert lib.aln_seqset_candidates(hnd, len(cand) + 1, 0, idx.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data) == INV and intact()
    assert lib.aln_seqset_candidates(hnd, 0, len(cand), None, a.ctypes.data, b.ctypes.data, c.ctypes.data) == INV and intact()
    assert lib.aln_seqset_candidate_scores(hnd, None, f.ctypes.data, status.ctypes.data) == INV and intact()
    assert lib.aln_seqset_candidate_scores(hnd, C.byref(p), None, status.ctypes.data) == INV and intact()
    assert lib.aln_seqset_candidate_hits(hnd, None, F_MIN, C.byref(count)) == INV and intact()
    assert lib.aln_seqset_candidate_hits(hnd, C.byref(p), F_MIN, None) == INV and intact()
    assert lib.aln_seqset_candidate_scores(hnd, C.byref(pwm), f.ctypes.data, status.ctypes.data) == UNS and intact()
    assert lib.aln_seqset_candidate_hits(hnd, C.byref(pwm), F_MIN, C.byref(count)) == UNS and intact()
    # no index at all, no candidate list at all: a fresh set
    with SeqSet(T.make_set()[:4]) as fresh:
        small = upper(0, 4)
        assert lib.aln_seqset_prefilter(fresh.handle, C.byref(spec()), C.byref(small), C.byref(count)) == INV
        assert lib.aln_seqset_candidates(fresh.handle, 0, 0, idx.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data) == INV
        assert lib.aln_seqset_candidate_hits(fresh.handle, C.byref(p), F_MIN, C.byref(count)) == INV
    assert intact()


# ---------------------------------------------------------------- the C99 caller
def hexf(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(sset, tmp_path):
    """tests/abi_prefilter.c: the five exports called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    seqs = T.make_set()
    tok = [len(seqs)] + [len(s) for s in seqs] + [int(c) for s in seqs for c in s] + [m.shape[0], m.shape[1]]
    tok += [hexf(v) for v in np.asarray(m, dtype=np.float64).ravel()] + [hexf(d), hexf(e), hexf(F_MIN), 98]
    tok += [K3[0], K3[1], SELECTIVE["min_shared"], SELECTIVE["min_per_1024"]]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(x) for x in tok) + "\n")
    exe = native_build.build_prefilter_harness()
    out = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1] for l in lines if l[0] == "rc"] == ["seqset_create", "kmer_index", "prefilter", "candidates", "candidate_scores", "candidate_hits", "held_list"]
    assert all(l[2] == "0" for l in lines if l[0] == "rc") and ["guards", "ok"] in lines
    n_words = sset.kmer_index(*K3)
    cand = sset.prefilter(*K3, **SELECTIVE)
    f, status = cand.score(m, d, e, semantics=sem)
    held = cand.hits(m, d, e, F_MIN, semantics=sem)
    assert [l[1:] for l in lines if l[0] == "n_words"] == [[str(v) for v in n_words.tolist()]]
    assert [l[1] for l in lines if l[0] == "count"] == [str(len(cand))] and [l[1] for l in lines if l[0] == "held"] == [str(len(held))]
    assert [l[1:] for l in lines if l[0] == "cand"] == [[str(int(i)), str(int(q)), str(int(t)), str(int(s))] for i, q, t, s in zip(cand.index, cand.q, cand.t, cand.shared)]
    assert [l[1:] for l in lines if l[0] == "score"] == [[hexf(v), str(int(s))] for v, s in zip(f, status)]
    assert [l[1:] for l in lines if l[0] == "hit"] == [[str(int(i)), str(int(q)), str(int(t)), hexf(v)] for i, q, t, v in zip(held.index, held.q, held.t, held.f)]
    assert len(cand) > 0 and len(held) > 0


# ---------------------------------------------------------------- the command
def test_the_command(sset, tmp_path, capsys):
    from aligner_amd import allpairs
    from aligner_amd.enums import Protein
    from aligner_amd.matrices import get_blosum62
    seqs = [s for s in T.make_set()[3:11]]                # the eight sequences of 7 .. 600 standard residues
    letters = Protein.letters
    fa = tmp_path / "x.fasta"
    fa.write_text("".join(">s%d\n%s\n" % (i, "".join(letters[int(c)] for c in s)) for i, s in enumerate(seqs)))
    m = get_blosum62()
    args = ["-i", str(fa), "--kmer", "3", "--min-shared", "2", "--min-shared-per-1024", "16"]
    idx, q, t, sh = R.prefilter(seqs, 3, 20, 2, 16, (0, len(seqs), 0, len(seqs), 1))
    assert 0 < len(idx) < 28
    with SeqSet(seqs) as ss:
        f, status = ss.score(m, 11.0, 2.0, None)
        full = ss.hits(m, 11.0, 2.0, F_MIN, None)
        rows = [h for h in range(len(full)) if int(full.index[h]) in set(idx)]
        assert allpairs.main(args) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%r,%d" % (a, b, float(f[k]), s) for k, a, b, s in zip(idx, q, t, sh)]
        assert allpairs.main(args + ["--f-min", repr(F_MIN)]) == 0
        out = capsys.readouterr().out.splitlines()
        assert out == ["s%d,s%d,%r" % (int(full.q[h]), int(full.t[h]), float(full.f[h])) for h in rows] and len(out) > 0
        assert allpairs.main(args + ["--f-min", repr(F_MIN), "--cluster", "greedy"]) == 0
        out = capsys.readouterr().out.splitlines()
        ref = cluster_mod.cluster_edges(len(seqs), full.q[rows], full.t[rows], lengths=ss.len.astype(np.uint32), mode="greedy")
        size = dict(zip(ref.records["label"].tolist(), ref.records["size"].tolist()))
        assert out == ["s%d,s%d,%d" % (i, lab, size[lab]) for i, lab in enumerate(ref.label.tolist())]


def test_all_pairs_routes_through_the_prefilter():
    from aligner_amd.matrices import get_blosum62
    from aligner_amd.seqset import all_pairs
    seqs = T.make_set()[3:11]
    m = get_blosum62()
    idx, wq, wt, sh = R.prefilter(seqs, 3, 20, 2, 16, (0, len(seqs), 0, len(seqs), 1))
    fq, ft, ff, fstatus = all_pairs(seqs, m, 11.0, 2.0)
    q, t, f, status = all_pairs(seqs, m, 11.0, 2.0, prefilter=dict(k=3, alphabet_size=20, **SELECTIVE))
    assert q.tolist() == wq and t.tolist() == wt and (T.bits(f) == T.bits(ff[idx])).all() and (status == fstatus[idx]).all()
    f_min = float(np.median(ff[idx]))
    q, t, f, alns = all_pairs(seqs, m, 11.0, 2.0, f_min=f_min, prefilter=dict(k=3, alphabet_size=20, **SELECTIVE))
    keep = [k for k in idx if ff[k] >= f_min]
    assert q.tolist() == fq[keep].tolist() and t.tolist() == ft[keep].tolist() and (T.bits(f) == T.bits(ff[keep])).all() and len(alns) == len(keep) > 0
