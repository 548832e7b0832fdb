"""aln_seqset_candidate_best on the GPU: the k best targets per query among the pairs of a candidate list, against aln_seqset_best
on the same rectangle (a list that holds every pair must give the same held state, bit for bit) and against a numpy restatement of
the rule over the candidates' own f and status (a sparse list).

Two sets.  The dense one is test_best_gpu.py's: eight queries against 4 200 targets of 0 .. 4 residues, prefiltered with both
thresholds 0, so that the list is the whole 8 x 4 200 rectangle: a row spans three pieces of 2048 list positions, and the pieces at
positions 4096 and 8192 and so on hold the end of one row and the beginning of the next.  The sparse one is built here: a family of 60,
80 families of 3, six strangers and three records without a word, prefiltered with k = 3, min_shared 4, 256 / 1024: rows of 60, 3, 1
and 0 candidates; piece 0 ends inside row 35's run of 60, piece 1 holds more than 100 rows."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prefilter_ref as R                                                       # noqa: E402
import select_cases as SC                                                       # noqa: E402
import test_best_gpu as B                                                       # noqa: E402
import test_seqset_gpu as T                                                     # noqa: E402
from aligner_amd import _ffi, runtime                                           # noqa: E402
from aligner_amd import build as native_build                                   # noqa: E402
from aligner_amd import cluster as cluster_mod                                  # noqa: E402
from aligner_amd.enums import Protein                                           # noqa: E402
from aligner_amd.seqset import BestHits, Candidates, SeqSet, best_ranks, rectangle, upper   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 2048
NEG_INF = float("-inf")
DENSE_K = (2, 20)                                  # the index of the dense set: any will do, both thresholds are 0
SPARSE_K = (3, 20)
SPARSE = dict(min_shared=4, min_per_1024=256)
SPARSE_SCHEMES = ("core_local_11_2", "real_valued")      # an integer and a real-valued scheme of test_seqset_gpu.py


# ---------------------------------------------------------------- helpers
def snapshot(held, keep=None):
    """the held list, and the summaries and raw strings of the listed (default: all) held hits, as bytes"""
    res, strs = held.strings(keep)
    return dict(index=held.index.tobytes(), q=held.q.tobytes(), t=held.t.tobytes(), f=held.f.tobytes(), rank=held.rank.tobytes(),
                res=[np.ascontiguousarray(res[n]).tobytes() for n in T.FIELDS], strs=[(a.tobytes(), b.tobytes()) for a, b in strs])


def digest_of(snap):
    h = hashlib.sha256()
    for key in ("index", "q", "t", "f", "rank"):
        h.update(snap[key])
    for r in snap["res"]:
        h.update(r)
    for a, b in snap["strs"]:
        h.update(a); h.update(b)
    return h.hexdigest()


def list_rule(index, q, t, f, status, t_count, k, f_min, skip_self):
    """The numpy restatement over a list: per row (index // t_count) the selectable entries by descending f (-0.0 == +0.0), equal f
    by ascending target, the first min(k, t_count); then all of them in ascending pair order.  -> positions of the list"""
    index, q, t = np.asarray(index).astype(np.int64), np.asarray(q).astype(np.int64), np.asarray(t).astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = (status == 0) & (f == f) & (f >= f_min)
    if skip_self:
        ok &= q != t
    pos = np.flatnonzero(ok)
    row = index[pos] // t_count
    order = pos[np.lexsort((t[pos], -(f[pos] + 0.0), row))]
    rows = index[order] // t_count
    start = np.flatnonzero(np.concatenate([[True], rows[1:] != rows[:-1]])) if len(order) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(order)) - np.repeat(start, np.diff(np.concatenate([start, [len(order)]])))
    return np.sort(order[rank < min(k, t_count)])


def check_against_list(held, cand, f, status, t_count, k, f_min, skip_self):
    want = list_rule(cand.index, cand.q, cand.t, f, status, t_count, k, f_min, skip_self)
    assert isinstance(held, BestHits) and len(held) == len(want), (len(held), len(want))
    assert np.array_equal(held.index, cand.index[want]) and np.array_equal(held.q, cand.q[want]) and np.array_equal(held.t, cand.t[want])
    assert np.array_equal(B.bits(held.f), B.bits(f[want] + 0.0))
    assert np.array_equal(held.rank, best_ranks(cand.q[want], cand.t[want], f[want]))
    return want


# ---------------------------------------------------------------- the dense set: the list is the whole rectangle
@pytest.fixture(scope="module")
def dense():
    with SeqSet(B.set_codes()) as s:
        yield s


def both(sset, blosum62, blk, k, f_min, skip_self=False):
    """(snapshot of Candidates.best, snapshot of SeqSet.best) on a rectangle whose every pair is listed"""
    cand = sset.prefilter(*DENSE_K, block=rectangle(*blk))
    assert len(cand) == blk[1] * blk[3] and np.array_equal(cand.index, np.arange(len(cand), dtype=np.uint64))
    held = cand.best(blosum62, B.DEL, B.EXT, k, f_min=f_min, skip_self=skip_self)
    stats = sset.stats()                               # (before the strings are fetched: they count as bytes too)
    mine = snapshot(held)
    theirs = snapshot(sset.best(blosum62, B.DEL, B.EXT, k, f_min=f_min, block=rectangle(*blk), skip_self=skip_self))
    return mine, theirs, stats


@pytest.mark.parametrize("k", B.KS)
def test_a_list_of_every_pair_equals_best(dense, blosum62, k):
    """8 x 4 200, k in {1, 5, 64} x f_min in {-inf, 12, NaN}: ties on both sides of the position edges 2047 | 2048 and 4095 | 4096
    of row 'AAA' and 'WW', a row with fewer than k selectable entries ('WW': 3 at f_min 12, 40 at -inf), a row with none (the empty
    query).  The whole list, f bit for bit, ranks, summaries and strings."""
    for f_min in B.F_MINS:
        mine, theirs, stats = both(dense, blosum62, B.FULL, k, f_min)
        assert mine == theirs
        n = len(mine["index"]) // 8
        assert (n == 0) == (f_min != f_min)
        if f_min == NEG_INF:
            per_row = np.bincount(np.frombuffer(mine["q"], dtype=np.uint32), minlength=B.NQ)
            assert per_row[B.EMPTY_Q] == 0 and per_row[B.Q_WW] == min(k, 40) and per_row[B.Q_AAA] == k
        # one list chunk: 16 bytes of it, 8 of the total, 16 per kept pair; the selection kernels ran
        assert stats["bytes_down"] == 16 + 8 + 16 * n and stats["fetch_kernel_ms"] > 0 and stats["wall_ms"] > 0


def test_one_row_one_column_and_a_square_with_its_self_pairs(dense, blosum62):
    """1 x 4 200: one row over three pieces.  4 200 x 1: 4 200 rows of one entry, one slot each, two and a bit pieces of 2048 rows.
    70 x 70 with and without skip-self: the list holds the 70 self pairs."""
    for blk in ((B.Q_AAA, 1, B.NQ, B.NT), (B.NQ, B.NT, B.Q_AAA, 1)):
        for k in (1, 64):
            mine, theirs, _ = both(dense, blosum62, blk, k, NEG_INF)
            assert mine == theirs and len(mine["index"]) > 0
    assert len(mine["index"]) // 8 > 2000
    blk = (B.NQ, 70, B.NQ, 70)
    for k in (1, 5, 64):
        for skip in (False, True):
            mine, theirs, _ = both(dense, blosum62, blk, k, NEG_INF, skip)
            assert mine == theirs
            q, t = np.frombuffer(mine["q"], dtype=np.uint32), np.frombuffer(mine["t"], dtype=np.uint32)
            assert (q == t).any() != skip and len(q) > 0


# ---------------------------------------------------------------- the sparse set
def sparse_set():
    rng = np.random.default_rng(20261019)
    seqs = [np.zeros(0, dtype=np.uint8)]                 # row 0: no word, no candidate
    big = rng.integers(0, 20, 24).astype(np.uint8)
    for i in range(60):                                  # one family of 60: rows of 60 candidates, many equal scores
        s = big[: 24 - i % 7].copy()
        if i % 3:
            s[int(rng.integers(0, len(s)))] = rng.integers(0, 20)
        seqs.append(s)
    seqs.append(np.array([3], dtype=np.uint8))           # a row without candidates between the families
    for fam in range(80):                                # 80 families of 3
        anc = rng.integers(0, 20, 14).astype(np.uint8)
        for j in range(3):
            s = anc[: 14 - j].copy()
            if j == 2:
                s[5] = (s[5] + 1) % 20
            seqs.append(s)
    for i in range(6):                                   # strangers: their own candidates only
        seqs.append(rng.integers(0, 20, 12).astype(np.uint8))
    seqs.append(np.array([4, 5], dtype=np.uint8))        # and a last row without candidates
    return seqs


@pytest.fixture(scope="module")
def sparse():
    with SeqSet(sparse_set()) as s:
        yield s


def sparse_candidates(sset):
    n = len(sset)
    return sset.prefilter(*SPARSE_K, block=rectangle(0, n, 0, n), **SPARSE)


def check_the_list_is_not_vacuous(cand, n, k):
    per = np.bincount(cand.q, minlength=n)
    first = np.searchsorted(cand.q, np.arange(n + 1))
    assert per[0] == 0 and per[61] == 0 and per[n - 1] == 0                               # empty rows: front, middle, end
    assert ((per >= 1) & (per < k)).any() and (per > k).any()
    assert max(len(np.unique(cand.q[p:p + PIECE])) for p in range(0, len(cand), PIECE)) >= 100
    assert any(first[r] <= PIECE - 1 and first[r + 1] > PIECE for r in range(n))            # a run crosses 2047 | 2048
    assert (cand.q == cand.t).sum() > 200                                                  # the self pairs are listed


@pytest.mark.parametrize("name", SPARSE_SCHEMES)
def test_sparse_list_equals_the_rule_and_best(sparse, name):
    sem, m, d, e, kw = T.schemes()[name]
    seqs = sparse_set()
    n = len(seqs)
    cand = sparse_candidates(sparse)
    want = R.prefilter(seqs, *SPARSE_K, SPARSE["min_shared"], SPARSE["min_per_1024"], (0, n, 0, n, 0))
    assert cand.index.tolist() == want[0] and cand.q.tolist() == want[1] and cand.t.tolist() == want[2]
    check_the_list_is_not_vacuous(cand, n, 5)
    f, status = cand.score(m, d, e, semantics=sem, **kw)
    assert (status == 0).sum() > 4000 and len(np.unique(f)) < len(f) // 2                   # ties
    if name == "real_valued":
        assert (f != np.round(f)).sum() > 1000
    f_sel = float(np.median(f[status == 0]))
    for k, f_min, skip in ((1, NEG_INF, True), (5, NEG_INF, True), (5, NEG_INF, False), (5, f_sel, True), (64, NEG_INF, False), (64, float("nan"), True)):
        held = cand.best(m, d, e, k, f_min=f_min, skip_self=skip, semantics=sem, **kw)
        check_against_list(held, cand, f, status, n, k, f_min, skip)
        got = {q: pos for q, pos in held.by_query()}
        assert all(np.array_equal(held.rank[pos], np.arange(len(pos))) for pos in got.values())
        assert not ({0, 61, n - 1} & set(got)) and (len(held) == 0) == (f_min != f_min)
    # f bits and strings against SeqSet.best on the same rectangle.  Its rows hold the 64 best of ALL targets: a kept candidate is
    # among them iff it does not come after the row's last entry (or the row is not full)
    k = 5
    held = cand.best(m, d, e, k, skip_self=True, semantics=sem, **kw)
    mine = snapshot(held)
    mine_index, mine_q, mine_f, mine_t = held.index.copy(), held.q.copy(), held.f.copy(), held.t.copy()
    full = sparse.best(m, d, e, 64, skip_self=True, semantics=sem, **kw)
    at = np.searchsorted(full.index, mine_index)
    found = (at < len(full)) & (full.index[np.minimum(at, len(full) - 1)] == mine_index)
    last = {q: pos[-1] for q, pos in full.by_query()}
    for i in range(len(mine_index)):
        p = last[int(mine_q[i])]
        in_front = full.rank[p] < 63 or mine_f[i] > full.f[p] or (mine_f[i] == full.f[p] and mine_t[i] <= full.t[p])
        assert bool(found[i]) == bool(in_front), (i, int(mine_q[i]), int(mine_t[i]))
    assert found.sum() > len(found) // 2
    rows = at[found].astype(np.uint32)
    assert np.array_equal(B.bits(full.f[rows]), B.bits(mine_f[found]))
    res, strs = full.strings(rows)
    sel = np.flatnonzero(found)
    for j, i in enumerate(sel):
        assert (strs[j][0].tobytes(), strs[j][1].tobytes()) == mine["strs"][i]
    for fi, name_ in enumerate(T.FIELDS):
        width = len(mine["res"][fi]) // len(found)
        got_field = np.frombuffer(mine["res"][fi], dtype=np.uint8).reshape(len(found), width)[sel]
        assert got_field.tobytes() == np.ascontiguousarray(res[name_]).tobytes(), name_


# ---------------------------------------------------------------- chunked
def dense_digest(sset, blosum62):
    h, chunks = hashlib.sha256(), None
    cand = sset.prefilter(*DENSE_K, block=rectangle(*B.FULL))
    for k in B.KS:
        for f_min in B.F_MINS[:2]:
            held = cand.best(blosum62, B.DEL, B.EXT, k, f_min=f_min)
            chunks = (sset.stats()["bytes_down"] - 8 - 16 * len(held)) // 16
            h.update(digest_of(snapshot(held)).encode())
    return h.hexdigest(), chunks


def sparse_digest(sset):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    cand = sparse_candidates(sset)
    held = cand.best(m, d, e, 5, skip_self=True, semantics=sem)
    chunks = (sset.stats()["bytes_down"] - 8 - 16 * len(held)) // 16
    return digest_of(snapshot(held)), chunks


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet
import test_search_gpu as S
with SeqSet(S.B.set_codes()) as s:
    print("DENSE", *S.dense_digest(s, get_blosum62()))
with SeqSet(S.sparse_set()) as s:
    print("SPARSE", *S.sparse_digest(s))
"""


def test_chunked_run_is_byte_identical(dense, sparse, blosum62):
    """ALN_CHUNK_CELLS at a fifth of the dense block's cells (in a child: the other tests must not see the variable): 5 list chunks
    of three or four pieces each, none ending on a row or piece edge, so rows are cut by chunk borders and meet their running lists
    again in the next chunk.  The sparse list falls into dozens of chunks of less than a piece under the same bound."""
    cells = B.chunk_cells()
    q, t = B.block_qt(B.FULL)
    counts = SC.chunk_counts(B.set_lengths(), q, t, float(cells))
    assert len(counts) >= 5
    for n, end in zip(counts, np.cumsum(counts)[:-1]):
        assert end % B.NT != 0 and n % PIECE != 0 and n > PIECE, (n, end)
    seqs = sparse_set()
    idx, sq, st, _ = R.prefilter(seqs, *SPARSE_K, SPARSE["min_shared"], SPARSE["min_per_1024"], (0, len(seqs), 0, len(seqs), 0))
    sparse_counts = SC.chunk_counts(np.array([len(s) for s in seqs], dtype=np.int64), np.array(sq), np.array(st), float(cells))
    ends = np.cumsum(sparse_counts)[:-1]
    assert len(sparse_counts) >= 5 and any(sq[e - 1] == sq[e] for e in ends)              # a row is cut by a chunk border
    env = dict(os.environ, ALN_CHUNK_CELLS=str(cells))
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DENSE" in out.stdout and "SPARSE" in out.stdout, out.stdout + out.stderr
    d_tok, s_tok = out.stdout.split("DENSE")[1].split()[:2], out.stdout.split("SPARSE")[1].split()[:2]
    assert int(d_tok[1]) == len(counts) and int(s_tok[1]) == len(sparse_counts)
    mine, chunks = dense_digest(dense, blosum62)
    assert chunks == 1 and d_tok[0] == mine
    mine, chunks = sparse_digest(sparse)
    assert chunks == 1 and s_tok[0] == mine


# ---------------------------------------------------------------- state, on-top calls, refusals
def test_state_on_top_calls_and_refusals(sparse):
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    lib, hnd, n = sparse.lib, sparse.handle, len(sparse)
    cand = sparse_candidates(sparse)
    f, status = cand.score(m, d, e, semantics=sem)
    first = cand.best(m, d, e, 5, skip_self=True, semantics=sem)
    check_against_list(first, cand, f, status, n, 5, NEG_INF, True)
    # the candidate list survives, and a second call with another k reuses it
    again = Candidates(sparse, len(cand))
    assert np.array_equal(again.index, cand.index) and np.array_equal(again.shared, cand.shared)
    second = cand.best(m, d, e, 2, skip_self=True, semantics=sem)
    check_against_list(second, cand, f, status, n, 2, NEG_INF, True)
    assert 0 < len(second) < len(first)
    # held_report and held_cluster on top: what the same pairs give when SeqSet.hits holds them
    rep = second.report(m)
    res, _ = second.strings()
    ok = res["status"] == 0
    assert ok.all() and (rep["columns"] > 0).all() and (rep["identical"] <= rep["columns"]).all()
    for mode in ("components", "greedy"):
        got = second.cluster(mode=mode)
        ref = cluster_mod.cluster_edges(n, second.q[ok], second.t[ok], lengths=sparse.len.astype(np.uint32), mode=mode)
        assert got.label.tolist() == ref.label.tolist() and got.records.tobytes() == ref.records.tobytes()
    kept = second.filter(m, min_identity=0.9)
    assert 0 < len(kept) <= len(second)
    full = sparse.hits(m, d, e, NEG_INF, rectangle(0, n, 0, n), semantics=sem)
    rows = np.searchsorted(full.index, second.index).astype(np.uint32)
    assert np.array_equal(full.index[rows], second.index) and full.report(m, keep=rows).tobytes() == rep.tobytes()
    # refusals: nothing written, the held list of the last good call still served, the candidate list intact
    second = cand.best(m, d, e, 2, skip_self=True, semantics=sem)
    before = snapshot(second)
    count = C.c_uint64(0xABCDEF)
    good, keep = runtime.make_params(sem, d, e, m)
    pwm, keep2 = runtime.make_params(_ffi.PWM_LOCAL, d, e, np.ascontiguousarray(m[:, :8]))
    INV, UNS = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED

    def refused(p, k, flags, want, cnt=count):
        got = lib.aln_seqset_candidate_best(hnd, C.byref(p) if p is not None else None, k, NEG_INF, flags, C.byref(cnt) if cnt is not None else None)
        assert got == want, (got, want, _ffi.last_error())
        assert count.value == 0xABCDEF and snapshot(BestHits(sparse, len(second), sem)) == before
        assert np.array_equal(Candidates(sparse, len(cand)).index, cand.index)

    refused(None, 2, 0, INV)
    refused(good, 2, 0, INV, cnt=None)
    refused(good, 0, 0, INV)
    refused(good, _ffi.SEQSET_BEST_MAX + 1, 0, INV)
    refused(good, 2, 2, INV)
    refused(good, 2, 3, INV)
    refused(pwm, 2, 0, UNS)
    assert lib.aln_seqset_candidate_best(None, C.byref(good), 2, NEG_INF, 0, C.byref(count)) == INV and count.value == 0xABCDEF
    # a NaN f_min selects nothing; an empty candidate list holds nothing, as candidate_hits does on one
    assert len(cand.best(m, d, e, 5, f_min=float("nan"), semantics=sem)) == 0
    empty = sparse.prefilter(*SPARSE_K, block=rectangle(0, n, 0, n), min_shared=1000)
    assert len(empty) == 0
    none = empty.best(m, d, e, 5, semantics=sem)
    assert len(none) == 0 and len(BestHits(sparse, 0, sem)) == 0 and len(empty.hits(m, d, e, NEG_INF, semantics=sem)) == 0
    # a list made on an upper block: a pair of it belongs to both of its sequences
    tri = sparse.prefilter(*SPARSE_K, block=upper(0, n), **SPARSE)
    held = tri.hits(m, d, e, 40.0, semantics=sem)
    kept_before = (len(held), held.index.tobytes())
    assert len(tri) > 0 and lib.aln_seqset_candidate_best(hnd, C.byref(good), 2, NEG_INF, 0, C.byref(count)) == UNS and count.value == 0xABCDEF
    assert b"rectangle" in lib.aln_last_error()
    again = type(held)(sparse, kept_before[0], sem)
    assert again.index.tobytes() == kept_before[1] and len(Candidates(sparse, len(tri))) == len(tri)
    # no candidate list at all: a fresh set, and a set whose index was rebuilt
    with SeqSet(sparse_set()[:8]) as fresh:
        assert lib.aln_seqset_candidate_best(fresh.handle, C.byref(good), 2, NEG_INF, 0, C.byref(count)) == INV
        assert lib.aln_seqset_candidate_hits(fresh.handle, C.byref(good), NEG_INF, C.byref(count)) == INV
    sparse.kmer_index(*SPARSE_K)
    assert lib.aln_seqset_candidate_best(hnd, C.byref(good), 2, NEG_INF, 0, C.byref(count)) == INV and count.value == 0xABCDEF


# ---------------------------------------------------------------- the callers
def hexf(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def test_through_c(sparse, tmp_path):
    """tests/abi_search.c: the export called from C99 on buffers of exactly the documented sizes, each followed by a guard zone"""
    sem, m, d, e, kw = T.schemes()["core_local_11_2"]
    seqs = sparse_set()
    tok = [len(seqs)] + [len(s) for s in seqs] + [int(c) for s in seqs for c in s] + [m.shape[0], m.shape[1]]
    tok += [hexf(v) for v in np.asarray(m, dtype=np.float64).ravel()] + [hexf(d), hexf(e), hexf(20.0), 98]
    tok += [SPARSE_K[0], SPARSE_K[1], SPARSE["min_shared"], SPARSE["min_per_1024"], 4, _ffi.BEST_SKIP_SELF]
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(x) for x in tok) + "\n")
    exe = native_build.build_search_harness()
    out = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1] for l in lines if l[0] == "rc"] == ["seqset_create", "kmer_index", "prefilter", "candidate_best", "held_list", "candidates"]
    assert all(l[2] == "0" for l in lines if l[0] == "rc") and ["guards", "ok"] in lines
    cand = sparse_candidates(sparse)
    held = cand.best(m, d, e, 4, f_min=20.0, skip_self=True, semantics=sem)
    assert [l[1] for l in lines if l[0] in ("count", "count_after")] == [str(len(cand))] * 2 and [l[1] for l in lines if l[0] == "held"] == [str(len(held))]
    assert [l[1:] for l in lines if l[0] == "hit"] == [[str(int(i)), str(int(q)), str(int(t)), hexf(v)] for i, q, t, v in zip(held.index, held.q, held.t, held.f)]
    assert len(held) > 100


def test_the_command(tmp_path, capsys, blosum62):
    """python -m aligner_amd.allpairs --kmer 3 --min-shared-per-1024 256 --best-candidates K [--f-min F]: --best's rows over the
    candidates of the full square, self pairs skipped; against the score pass of the square and the reference prefilter."""
    from aligner_amd import allpairs
    every = sparse_set()
    seqs = every[1:13] + every[62:71] + every[-4:-1]                  # twelve of the family of 60, three families of 3, three strangers
    letters = Protein.letters
    fa = tmp_path / "x.fasta"
    fa.write_text("".join(">s%d\n%s\n" % (i, "".join(letters[int(c)] for c in s)) for i, s in enumerate(seqs)))
    n = len(seqs)
    idx, q, t, _ = (np.array(a, dtype=np.int64) for a in R.prefilter(seqs, 3, 20, 0, 256, (0, n, 0, n, 0)))
    assert n < len(idx) < n * n
    args = ["-i", str(fa), "--kmer", "3", "--min-shared-per-1024", "256", "--best-candidates", "3"]
    with SeqSet(seqs) as ss:
        f, status = ss.score(blosum62, 11.0, 2.0, rectangle(0, n, 0, n))
    for extra, f_min in (([], NEG_INF), (["--f-min", "60.0"], 60.0)):
        assert allpairs.main(args + extra) == 0
        got = capsys.readouterr().out.splitlines()
        pos = list_rule(idx, q, t, f[idx], status[idx], n, 3, f_min, True)
        rank = best_ranks(q[pos], t[pos], f[idx][pos])
        want = ["s%d,%d,s%d,%r" % (q[p], r + 1, t[p], float(f[idx][p])) for r, p in sorted(zip(rank.tolist(), pos.tolist()), key=lambda x: (q[x[1]], x[0]))]
        assert got == want and len(got) > 0
    assert allpairs.main(args + ["--report", "--min-identity", "0.5"]) == 0
    rows = capsys.readouterr().out.splitlines()
    assert 0 < len(rows) <= 3 * n and all(len(r.split(",")) == 11 for r in rows)
    assert allpairs.main(args + ["--cluster", "components"]) == 0
    rows = capsys.readouterr().out.splitlines()
    pos = list_rule(idx, q, t, f[idx], status[idx], n, 3, NEG_INF, True)
    ref = cluster_mod.cluster_edges(n, q[pos].astype(np.uint32), t[pos].astype(np.uint32), lengths=np.array([len(s) for s in seqs], dtype=np.uint32), mode="components")
    size = dict(zip(ref.records["label"].tolist(), ref.records["size"].tolist()))
    assert rows == ["s%d,s%d,%d" % (i, lab, size[lab]) for i, lab in enumerate(ref.label.tolist()) if lab != _ffi.CLUSTER_NONE] and len(rows) > 12
