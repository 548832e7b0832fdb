"""aln_seqset_best on the GPU: the k best targets per query, selected on the device, against a numpy restatement of the rule
(aln_best_rules.h) on inputs whose f and status are known by table lookup, in the manner of test_select_tiles_gpu.py.

The set: eight queries -- 'A', 'AA', 'AAA', '', 'W', 'WW', 'WWWW', 'AW' -- followed by 4 200 targets out of the same eight contents.
Under BLOSUM62 11 / 2 core local a pair's f and status depend on the two contents only (64 oracle calls, once); A x W pairs have no
positive cell and fail; equal scores are everywhere, so the tie rule decides most rows.  A row of the 8 x 4 200 rectangle has three
pieces (2048, 2048, 104).  'AAA' targets begin at 2046, so the best of query 'AAA' straddle the 2047 | 2048 edge; the only 'WW' /
'WWWW' targets sit at 4095, 4096, 4097, so query 'WW' has 3 candidates at f_min = 12 and 40 at -inf; the empty query has none."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from aligner_amd import _ffi, runtime                                             # noqa: E402
from aligner_amd.batch import PairBatch, align_batch                              # noqa: E402
from aligner_amd.enums import Protein                                             # noqa: E402
from aligner_amd.seqset import BestHits, SeqSet, best_ranks, rectangle, upper     # noqa: E402
import select_cases as SC                                                         # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTENTS = ["A", "AA", "AAA", "", "W", "WW", "WWWW", "AW"]          # content ids 0 .. 7; the queries are these, in this order
NQ, NT, PIECE = 8, 4200, 2048
DEL, EXT = 11.0, 2.0
EMPTY_Q, Q_AAA, Q_WW = 3, 2, 5
KS = (1, 5, 64)
F_MINS = (float("-inf"), 12.0, float("nan"))
FIELDS = ["f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status"]


def target_ids():
    """Content id of every target (positions within the block's target range)."""
    ids = np.array([0 if (i * 7) % 3 else 1 for i in range(NT)], dtype=np.int64)       # 'A' and 'AA'
    for a, b in ((2046, 2051), (3000, 3020), (4090, 4095), (4150, 4166)):
        ids[a:b] = 2                                                                  # 'AAA': 46 of them, none before 2046
    ids[[100, 101, 102, 103, 104, 105, 2044, 2045, 2051, 2052, 4098, 4199]] = 4        # 'W'
    ids[[4095, 4096]] = 5                                                              # 'WW' on both sides of 4095 | 4096
    ids[4097] = 6                                                                      # 'WWWW'
    for a, b in ((10, 15), (2040, 2044), (2053, 2057), (4086, 4090), (4099, 4103), (4170, 4174)):
        ids[a:b] = 7                                                                  # 'AW': 25
    ids[4120] = 3                                                                      # the empty target
    return ids


def set_ids():
    return np.concatenate([np.arange(NQ), target_ids()])


def set_codes():
    return [np.asarray(Protein.str_to_vec(CONTENTS[i]), dtype=np.uint8) for i in set_ids()]


def set_lengths():
    return np.array([len(CONTENTS[i]) for i in set_ids()], dtype=np.int64)


FULL = (0, NQ, NQ, NT)                                    # the 8 x 4 200 rectangle
_table = {}


def table(orc, blosum62):
    """Per (query content, target content): the oracle's f, status and strings.  64 calls, once."""
    if not _table:
        codes = [np.asarray(Protein.str_to_vec(s), dtype=np.uint8) for s in CONTENTS]
        n = len(codes)
        f, status, strs = np.zeros((n, n)), np.zeros((n, n), dtype=np.int32), {}
        for a in range(n):
            for b in range(n):
                o = orc.align(orc.CORE_LOCAL, codes[a], codes[b], DEL, EXT, blosum62)
                f[a, b], status[a, b] = (o["f"] if o["status"] == 0 else 0.0), o["status"]
                strs[(a, b)] = (o["qa"].tobytes(), o["ta"].tobytes(), o["end"])
        _table.update(f=f, status=status, strs=strs)
    return _table["f"], _table["status"], _table["strs"]


def block_qt(blk):
    qf, qc, tf, tc = blk
    return np.repeat(np.arange(qf, qf + qc), tc), np.tile(np.arange(tf, tf + tc), qc)


def block_table(orc, blosum62, blk):
    """(q, t, f, status) of every pair of a rectangle, by table lookup."""
    of, ostatus, _ = table(orc, blosum62)
    ids = set_ids()
    q, t = block_qt(blk)
    return q, t, of[ids[q], ids[t]], ostatus[ids[q], ids[t]]


def rule(q, t, f, status, tc, k, f_min, skip_self=False):
    """The numpy restatement: per row of tc pairs the candidates by descending f (-0.0 == +0.0), equal f by ascending target, the
    first k; then all of them in ascending pair order.  -> (pair numbers, f)"""
    with np.errstate(invalid="ignore"):
        ok = (status == 0) & (f == f) & (f >= f_min)
    if skip_self:
        ok &= q != t
    kept = []
    for r in range(len(f) // tc):
        idx = r * tc + np.flatnonzero(ok[r * tc:(r + 1) * tc])
        kept.append(idx[np.lexsort((t[idx], -(f[idx] + 0.0)))][:k])
    kept = np.sort(np.concatenate(kept)) if kept else np.zeros(0, dtype=np.int64)
    return kept.astype(np.int64), f[kept] + 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def sset():
    with SeqSet(set_codes()) as s:
        yield s


def run_best(sset, blosum62, blk, k, f_min, skip_self=False):
    return sset.best(blosum62, DEL, EXT, k, f_min=f_min, block=rectangle(*blk), skip_self=skip_self)


def check_list(held, q, t, want_idx, want_f):
    assert isinstance(held, BestHits)
    assert len(held) == len(want_idx), (len(held), len(want_idx))
    assert np.array_equal(held.index, want_idx.astype(np.uint64))
    assert np.array_equal(bits(held.f), bits(want_f))
    assert np.array_equal(held.q, q[want_idx]) and np.array_equal(held.t, t[want_idx])
    assert np.array_equal(held.rank, best_ranks(q[want_idx], t[want_idx], want_f))


def check_strings(held, orc, blosum62, edges=()):
    """Strings of the hits next to the named pair numbers and of a sample against the oracle."""
    _, _, ostr = table(orc, blosum62)
    ids = set_ids()
    near = []
    for k in edges:
        p = int(np.searchsorted(held.index, k))
        near += [p - 1, p]
    pos = SC.sample_positions(len(held), [p for p in near if 0 <= p < len(held)])
    res, strs = held.strings(pos)
    for j, p in enumerate(pos):
        qa, ta, end = ostr[(ids[held.q[p]], ids[held.t[p]])]
        assert res["status"][j] == 0 and res["f"][j] == held.f[p]
        assert (res["end_y"][j], res["end_x"][j]) == end
        assert strs[j][0].tobytes() == qa and strs[j][1].tobytes() == ta, (int(held.q[p]), int(held.t[p]))


def test_the_table_has_the_cases_the_tests_rest_on(orc, blosum62):
    """On the CPU: ties across both piece edges, a row with fewer than k candidates, an empty row, failing pairs."""
    q, t, f, status = block_table(orc, blosum62, FULL)
    assert (status[EMPTY_Q * NT:(EMPTY_Q + 1) * NT] != 0).all()
    row = slice(Q_WW * NT, (Q_WW + 1) * NT)
    assert ((status[row] == 0) & (f[row] >= 12.0)).sum() == 3 < 5 and (status[row] == 0).sum() == 40 < 64
    assert (status != 0).sum() > 8000 and (status == 0).sum() > 8000                     # A x W fails, in every piece
    row = slice(Q_AAA * NT, (Q_AAA + 1) * NT)
    assert f[row][2047] == f[row][2048] == 12.0 and f[row][:2046].max() < 12.0            # the best of 'AAA' straddle 2047 | 2048
    assert f[Q_WW * NT + 4095] == f[Q_WW * NT + 4096] == 22.0                             # and those of 'WW' 4095 | 4096
    for k in KS:
        idx, _ = rule(q, t, f, status, NT, k, float("-inf"))
        per_row = np.bincount(idx // NT, minlength=NQ)
        assert per_row[EMPTY_Q] == 0 and per_row[Q_WW] == min(k, 40) and per_row[Q_AAA] == k
        if k > 1:
            pieces = {int((i % NT) // PIECE) for i in idx[idx // NT == Q_AAA]}
            assert len(pieces) >= 2                                                      # a row's answer is merged out of several pieces


@pytest.mark.parametrize("k", KS)
def test_full_block_equals_the_rule(sset, orc, blosum62, k):
    q, t, f, status = block_table(orc, blosum62, FULL)
    sf, sstatus = sset.score(blosum62, DEL, EXT, rectangle(*FULL))
    assert np.array_equal(sstatus, status) and np.array_equal(bits(sf[status == 0]), bits(f[status == 0]))
    edges = [r * NT + e for r in range(NQ) for e in (PIECE, 2 * PIECE)]
    for f_min in F_MINS:
        want_idx, want_f = rule(q, t, f, status, NT, k, f_min)
        from_score = rule(q, t, sf, sstatus, NT, k, f_min)
        assert np.array_equal(want_idx, from_score[0]) and np.array_equal(bits(want_f), bits(from_score[1]))
        held = run_best(sset, blosum62, FULL, k, f_min)
        check_list(held, q, t, want_idx, want_f)
        assert (len(held) == 0) == (f_min != f_min)
        if len(held):
            check_strings(held, orc, blosum62, edges)
            got = {qq: pos for qq, pos in held.by_query()}
            assert EMPTY_Q not in got and all(np.array_equal(held.rank[pos], np.arange(len(pos))) for pos in got.values())
            st = sset.stats()
            assert st["fetch_kernel_ms"] > 0 or st["fill_ms"] > 0


def digest(sset, blosum62):
    """Lists, summaries and strings of every (k, f_min) on the full block, hashed; and the chunks the last pass ran."""
    h = hashlib.sha256()
    chunks = None
    for k in KS:
        for f_min in F_MINS[:2]:
            held = run_best(sset, blosum62, FULL, k, f_min)
            st = sset.stats()
            chunks = (st["bytes_down"] - 8 - 16 * len(held)) // 16          # 16 bytes per chunk, 8 for the total, 16 per kept pair
            res, strs = held.strings()
            for a in (held.index, held.q, held.t, held.f, held.rank):
                h.update(np.ascontiguousarray(a).tobytes())
            for name in FIELDS:
                h.update(np.ascontiguousarray(res[name]).tobytes())
            for qa, ta in strs:
                h.update(qa.tobytes()); h.update(ta.tobytes())
    return h.hexdigest(), chunks


def chunk_cells():
    L = set_lengths()
    return int(L[:NQ].sum() * L[NQ:].sum()) // 5 + 31


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd.matrices import get_blosum62
from aligner_amd.seqset import SeqSet
import test_best_gpu as T
with SeqSet(T.set_codes()) as s:
    d, chunks = T.digest(s, get_blosum62())
    print("DIGEST", d)
    print("CHUNKS", chunks)
"""


def test_chunked_run_is_byte_identical(sset, blosum62):
    """ALN_CHUNK_CELLS at a fifth of the block's cells: 5 chunks, none ending on a row or piece edge, so rows are cut in the middle
    and their running lists are merged across chunks -- the only place that happens.  In a child: the other tests must not see the
    variable."""
    q, t = block_qt(FULL)
    counts = SC.chunk_counts(set_lengths(), q, t, float(chunk_cells()))
    assert len(counts) == 5
    for end in np.cumsum(counts)[:-1]:
        assert end % NT not in (0, PIECE, 2 * PIECE), end
    env = dict(os.environ, ALN_CHUNK_CELLS=str(chunk_cells()))
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DIGEST" in out.stdout, out.stdout + out.stderr
    assert int(out.stdout.split("CHUNKS")[1].split()[0]) == len(counts) >= 2
    mine, chunks = digest(sset, blosum62)
    assert chunks == 1
    assert out.stdout.split("DIGEST")[1].split()[0] == mine


def test_one_row_and_one_column(sset, orc, blosum62):
    """1 x 4 200: one row of three pieces.  4 200 x 1: 4 200 rows of one pair, one slot each (more than 16 tiles of 256 rows)."""
    for blk in ((Q_AAA, 1, NQ, NT), (NQ, NT, Q_AAA, 1)):
        q, t, f, status = block_table(orc, blosum62, blk)
        for k in (1, 64):
            want_idx, want_f = rule(q, t, f, status, blk[3], k, float("-inf"))
            held = run_best(sset, blosum62, blk, k, float("-inf"))
            check_list(held, q, t, want_idx, want_f)
        check_strings(held, orc, blosum62)
    assert len(held) == (status == 0).sum() > 2000


EDGE_ROWS = 256 * 256 + 300                 # 258 tiles of 256 rows: the offsets kernel's second trip of 256 tiles begins at row 65 536
EDGE_TARGET, EDGE_F_MIN = 7, 11.0           # against 'AW': 'WWWW' scores 11 (kept, by equality), 'AAA' 4 (below), '' fails


def edge_ids():
    """Content id of every query row of the 65 836 x 1 rectangle: 'WWWW', 'AAA' and '' mixed, except that tile 254 (rows 65 024 ..
    65 279) holds no kept row, tile 255 (.. 65 535) and the last, partial tile (44 rows) only kept rows; tile 256 is mixed again and
    begins with a kept row."""
    i = np.arange(EDGE_ROWS)
    ids = np.where((i * 7) % 3 == 0, 6, np.where(i % 5 == 0, 3, 2))
    ids[254 * 256:255 * 256] = 2
    ids[255 * 256:256 * 256] = 6
    ids[256 * 256:256 * 256 + 2] = (6, 2)
    ids[257 * 256:] = 6
    return ids


def test_one_column_into_the_second_trip_of_tiles(orc, blosum62):
    """65 836 x 1, k = 1: 258 tiles of 256 rows, so the 64-bit tile offsets take their carry into a second trip of 256 tiles (the
    4 200 rows above stay within 17 tiles).  Kept rows lie on both sides of row 65 535 | 65 536."""
    of, ostatus, _ = table(orc, blosum62)
    ids = edge_ids()
    n = EDGE_ROWS
    q, t = np.arange(n), np.full(n, n)
    f, status = of[ids, EDGE_TARGET], ostatus[ids, EDGE_TARGET]
    want_idx, want_f = rule(q, t, f, status, 1, 1, EDGE_F_MIN)
    per_tile = np.bincount(want_idx // 256, minlength=258)
    assert {65535, 65536} <= set(want_idx.tolist()) and 65537 not in want_idx
    assert 0 < per_tile[253] < 256 and per_tile[254] == 0 and per_tile[255] == 256 and 0 < per_tile[256] < 256 and per_tile[257] == 44
    assert (status != 0).sum() > 1000 and ((status == 0) & (f < EDGE_F_MIN)).sum() > 1000 and (want_f == EDGE_F_MIN).all()
    codes = [np.asarray(Protein.str_to_vec(c), dtype=np.uint8) for c in CONTENTS]
    with SeqSet([codes[i] for i in ids] + [codes[EDGE_TARGET]]) as s:
        held = s.best(blosum62, DEL, EXT, 1, f_min=EDGE_F_MIN, block=rectangle(0, n, n, 1))
        check_list(held, q, t, want_idx, want_f)


def test_square_block_and_skip_self(sset, orc, blosum62):
    """The first 70 targets against themselves: with the flag no (i, i) is kept; without it every (i, i) that succeeds is kept, and
    is the first of its row wherever nothing earlier scores as much."""
    blk = (NQ, 70, NQ, 70)
    q, t, f, status = block_table(orc, blosum62, blk)
    for k in (1, 5, 64):
        for skip in (False, True):
            want_idx, want_f = rule(q, t, f, status, 70, k, float("-inf"), skip)
            held = sset.best(blosum62, DEL, EXT, k, block=rectangle(*blk), skip_self=skip)
            check_list(held, q, t, want_idx, want_f)
            diag = held.q == held.t
            if skip:
                assert not diag.any()
            else:
                # (i, i) scores the row's maximum here, so it is the row's first unless an earlier target ties it
                assert (status[q == t] == 0).all()
                tied_before = np.array([(f[i * 70:i * 70 + i][status[i * 70:i * 70 + i] == 0] >= f[i * 70 + i]).any() for i in range(70)])
                firsts = held.q[diag & (held.rank == 0)] - NQ
                assert np.array_equal(firsts, np.flatnonzero(~tied_before)) and 0 < len(firsts) < 70
    check_strings(held, orc, blosum62)


def test_real_valued_scheme(blosum62):
    """f values that are no integers: a 6 x 130 block of random proteins up to 65 long under a non-dyadic matrix, against
    aln_align_batch and the rule."""
    rng = np.random.default_rng(20261018)
    m = blosum62 * 0.37 + 0.013
    d, e = 11.3, 2.1
    anc = rng.integers(0, 20, 65).astype(np.uint8)
    seqs = []
    for i in range(136):
        n = int(rng.integers(1, 66))
        s = anc[:n].copy()
        mut = rng.random(n) < 0.4
        s[mut] = rng.integers(0, 20, int(mut.sum()))
        seqs.append(s)
    blk = (0, 6, 6, 130)
    q, t = block_qt(blk)
    ref = align_batch(PairBatch.from_pairs((seqs[a], seqs[b]) for a, b in zip(q, t)), _ffi.CORE_LOCAL, d, e, m, want_traceback=False).results
    f, status = ref["f"].copy(), ref["status"].copy()
    assert (status == 0).sum() > 700 and (f != np.round(f)).sum() > 700
    with SeqSet(seqs) as s:
        for k, f_min in ((3, float("-inf")), (64, float("-inf")), (64, float(np.median(f)))):
            want_idx, want_f = rule(q, t, f, status, 130, k, f_min)
            held = s.best(m, d, e, k, f_min=f_min, block=rectangle(*blk))
            check_list(held, q, t, want_idx, want_f)
        res, strs = held.strings([0, len(held) - 1])
        assert res["f"][0] == held.f[0] and res["f"][1] == held.f[-1] and len(strs[0][0]) > 0


def test_refusals_and_held_state(sset, orc, blosum62):
    """Refused calls leave count and an earlier held state alone; best replaces hits and hits replaces best."""
    lib = _ffi.load()
    good, keep = runtime.make_params(_ffi.CORE_LOCAL, DEL, EXT, blosum62)
    blk = rectangle(Q_WW, 1, NQ, NT)
    q, t, f, status = block_table(orc, blosum62, (Q_WW, 1, NQ, NT))
    first = run_best(sset, blosum62, (Q_WW, 1, NQ, NT), 5, float("-inf"))
    want_idx, want_f = rule(q, t, f, status, NT, 5, float("-inf"))
    check_list(first, q, t, want_idx, want_f)
    count = C.c_uint64(0xABCDEF)

    def refused(p, b, k, flags, want, cnt=count):
        st = lib.aln_seqset_best(sset.handle, C.byref(p), C.byref(b), k, float("-inf"), flags, C.byref(cnt) if cnt is not None else None)
        assert st == want, (st, want)
        assert count.value == 0xABCDEF
        again = BestHits(sset, len(first), _ffi.CORE_LOCAL)                      # the earlier held list is still served
        assert np.array_equal(again.index, first.index) and np.array_equal(bits(again.f), bits(first.f))

    refused(good, upper(0, 20), 5, 0, _ffi.ERR_UNSUPPORTED)
    pwm, keep2 = runtime.make_params(_ffi.PWM_LOCAL, DEL, EXT, np.ones((4, 30)))
    refused(pwm, blk, 5, 0, _ffi.ERR_UNSUPPORTED)
    refused(good, blk, 0, 0, _ffi.ERR_INVALID_ARGUMENT)
    refused(good, blk, 65, 0, _ffi.ERR_INVALID_ARGUMENT)
    refused(good, blk, 5, 2, _ffi.ERR_INVALID_ARGUMENT)
    refused(good, blk, 5, 3, _ffi.ERR_INVALID_ARGUMENT)
    refused(good, blk, 5, 0, _ffi.ERR_INVALID_ARGUMENT, cnt=None)
    refused(good, _ffi.SeqsetBlock(0, NQ, NQ, NT + 1, 0, 0), 5, 0, _ffi.ERR_INVALID_ARGUMENT)
    refused(good, _ffi.SeqsetBlock(0, NQ, NQ, NT, 0, 1), 5, 0, _ffi.ERR_INVALID_ARGUMENT)
    check_strings(first, orc, blosum62)                                          # held_strings after best, and after the refusals
    # hits replaces best, best replaces hits
    hits = sset.hits(blosum62, DEL, EXT, 22.0, blk)
    assert len(hits) == 3 and np.array_equal(hits.index, [4095, 4096, 4097])
    with pytest.raises(ValueError):
        first.strings([4])                                                       # position 4 of a list of 3
    second = run_best(sset, blosum62, (Q_WW, 1, NQ, NT), 5, float("-inf"))
    check_list(second, q, t, want_idx, want_f)
    assert len(BestHits(sset, 5, _ffi.CORE_LOCAL)) == 5 and np.array_equal(second.index, first.index)


def test_neighbours_on_one_context(sset, orc, blosum62):
    """best, then a score pass on the set and a batch call on the context, then best again: the same list, summaries and strings."""
    def snapshot():
        held = run_best(sset, blosum62, FULL, 5, 12.0)
        res, strs = held.strings()
        return (held.index.tobytes(), held.f.tobytes(), held.rank.tobytes(), [res[n].tobytes() for n in FIELDS], [(a.tobytes(), b.tobytes()) for a, b in strs])

    before = snapshot()
    assert len(before[4]) > 10
    sset.score(blosum62, DEL, EXT, rectangle(0, NQ, NQ, 300))
    codes = set_codes()
    pairs = [(a, NQ + b) for a in (0, 2, 5) for b in (0, 2046, 4095)]
    res = align_batch(PairBatch.from_pairs((codes[a], codes[b]) for a, b in pairs), _ffi.CORE_LOCAL, DEL, EXT, blosum62).results
    of, ostatus, _ = table(orc, blosum62)
    ids = set_ids()
    assert [int(s) for s in res["status"]] == [int(ostatus[ids[a], ids[b]]) for a, b in pairs]
    assert snapshot() == before


def test_command_line_best(tmp_path, capsys, orc, blosum62):
    """python -m aligner_amd.allpairs --best K: per record its K best partners, self pairs skipped, in rank order."""
    from aligner_amd import allpairs
    of, ostatus, _ = table(orc, blosum62)
    recs = [2, 1, 0, 5, 4, 7, 1]                                   # content ids: 'AAA', 'AA', 'A', 'WW', 'W', 'AW', 'AA'
    path = tmp_path / "x.fasta"
    path.write_text("".join(">r%d\n%s\n" % (i, CONTENTS[c]) for i, c in enumerate(recs)))
    assert allpairs.main(["-i", str(path), "--best", "2"]) == 0
    got = capsys.readouterr().out.splitlines()
    want = []
    for i, a in enumerate(recs):
        cand = sorted((-of[a, b], j) for j, b in enumerate(recs) if j != i and ostatus[a, b] == 0)[:2]
        want += ["r%d,%d,r%d,%r" % (i, rank + 1, j, float(-nf)) for rank, (nf, j) in enumerate(cand)]
    assert got == want and len(got) == 14
    with pytest.raises(SystemExit):
        allpairs.main(["-i", str(path), "--best", "2", "--heuristic", "--kd", "1", "--r-squared", "0.5"])
