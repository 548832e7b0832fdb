"""The resident pair set on the GPU (aln_pairset_*): per-pair matrices against the CPU oracle, equivalence with aln_align_batch across
chunks, isolation of a pair from its neighbours, per-pair failures, and heuristic.align_many against single HeuristicAligner calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd.enums import Protein

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_pairs(n, seed, max_len=1500, edges=True):
    rng = np.random.default_rng(seed)
    edge = [1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, max_len] if edges else []
    pairs = []
    for k in range(n):
        nq = edge[k % len(edge)] if k < 2 * len(edge) else int(rng.integers(1, max_len + 1))
        nt = edge[(k // 2) % len(edge)] if k < 2 * len(edge) else int(rng.integers(1, max_len + 1))
        q = rng.integers(0, 24 if k % 5 == 0 else 20, nq).astype(np.uint8)
        t = rng.integers(0, 24 if k % 5 == 0 else 20, nt).astype(np.uint8)
        if k % 2 and min(nq, nt) > 8:                               # a planted homolog
            L = int(rng.integers(4, min(nq, nt)))
            a, b = int(rng.integers(0, nq - L + 1)), int(rng.integers(0, nt - L + 1))
            piece = q[a:a + L].copy()
            mut = rng.random(L) < 0.2
            piece[mut] = rng.integers(0, 20, int(mut.sum()))
            t[b:b + L] = piece
        pairs.append((q, t))
    return pairs


def random_matrices(n, seed, blosum62):
    """One real-valued 24 x 24 matrix per pair: BLOSUM62 rescaled and perturbed (positive diagonal, no dyadic values)."""
    rng = np.random.default_rng(seed)
    return np.array([blosum62 * rng.uniform(0.3, 1.7) + rng.normal(0, 0.6, (24, 24)) for _ in range(n)])


def check_pair(orc, sem, pair, del_, ext, m, summary, strings, counts, where):
    q, t = pair
    ref = orc.align(sem, q, t, del_, ext, m)
    assert summary["status"] == ref["status"], where
    if ref["status"] != 0:
        assert counts.sum() == 0, where
        return
    assert summary["f"] == ref["f"] and summary["score"] == ref["score"], where
    assert (summary["end_y"], summary["end_x"]) == ref["end"] and (summary["start_y"], summary["start_x"]) == ref["start"], where
    assert summary["aln_len"] == len(ref["qa"]), where
    assert strings[0].tobytes() == ref["qa"].tobytes() and strings[1].tobytes() == ref["ta"].tobytes(), where
    assert counts.dtype == np.uint32 and (counts == orc.frequency_matrix(ref["qa"], ref["ta"], 24).astype(np.uint32)).all(), where


@pytest.mark.parametrize("sem,del_,ext", [(_ffi.CORE_LOCAL, 11.0, 2.0), (_ffi.CORE_LOCAL, 4.0, 4.0), (_ffi.CORE_GLOBAL, 11.0, 2.0)])
def test_per_pair_matrices_equal_the_oracle(orc, blosum62, sem, del_, ext):
    from aligner_amd.pairset import PairSet
    n = 272
    pairs = random_pairs(n, 700 + int(del_))
    mats = random_matrices(n, 701, blosum62)
    with PairSet(pairs) as ps:
        active = np.arange(n, dtype=np.uint32)
        res = ps.run(sem, del_, ext, mats, active)
        counts = ps.frequencies(active)
        summ, strs = ps.strings(active)
        st = ps.stats()
    assert summ.tobytes() == res.tobytes()
    assert st["bytes_down"] > 0
    for i in range(n):                                              # every pair, none left out
        check_pair(orc, sem, pairs[i], del_, ext, mats[i], res[i], strs[i], counts[i], i)
    assert (res["status"] == 0).sum() >= n - 16


CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd import _ffi, runtime
from aligner_amd.batch import RESULT_DTYPE, PairBatch
from aligner_amd.matrices import get_blosum62
from aligner_amd.pairset import PairSet
from test_pairset_gpu import random_pairs
pairs = random_pairs(96, 311, max_len=400, edges=False)      # (every chunk holds more than four pairs: the batch call keeps one route)
b = PairBatch.from_pairs(pairs)
m = get_blosum62() * 0.37 + 0.013
lib = _ffi.load()
for sem, d, e in ((_ffi.CORE_LOCAL, 11.3, 2.1), (_ffi.CORE_GLOBAL, 11.3, 2.1)):
    p, keep = runtime.make_params(sem, d, e, m, force_f64=True)
    first, count = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    chunks = lib.aln_plan_chunks(C.byref(p), b.q_len.ctypes.data, b.t_len.ctypes.data, len(b), 1, first.ctypes.data, count.ctypes.data, 64)
    assert chunks >= 3, chunks
    off, total = b.tb_layout()
    want = np.zeros(len(b), dtype=RESULT_DTYPE)
    tb = np.zeros(total, dtype=np.uint8)
    st = lib.aln_align_batch(runtime.context(), C.byref(p), b.seqs.ctypes.data, b.q_off.ctypes.data, b.q_len.ctypes.data, b.t_off.ctypes.data,
                             b.t_len.ctypes.data, len(b), want.ctypes.data, tb.ctypes.data, off.ctypes.data)
    assert st == 0, st
    with PairSet(b) as ps:
        act = np.arange(len(b), dtype=np.uint32)
        got = ps.run(sem, d, e, np.array([m] * len(b)), act)
        summ, strs = ps.strings(act)
    assert got.tobytes() == want.tobytes() and summ.tobytes() == want.tobytes()
    for i in range(len(b)):
        n, o, cap = int(want["aln_len"][i]), int(off[i]), int(b.q_len[i] + b.t_len[i] + 2)
        assert strs[i][0].tobytes() == tb[o:o + n].tobytes() and strs[i][1].tobytes() == tb[o + cap:o + cap + n].tobytes(), i
    print("chunks", chunks)
print("CHILD-OK")
"""


def test_shared_matrix_run_across_chunks_equals_align_batch():
    """Every matrix equal and ALN_CHUNK_CELLS small enough for >= 3 chunks (set in a child: the variable is read per call, but the
    parent's other tests must not see it): summaries and strings byte-equal to aln_align_batch with force_f64."""
    env = dict(os.environ, ALN_CHUNK_CELLS="1000000")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout + out.stderr


def test_a_pair_does_not_depend_on_its_neighbours_and_stale_fetches_fail(blosum62):
    from aligner_amd.pairset import PairSet
    n = 80
    pairs = random_pairs(n, 55, max_len=600)
    mats = random_matrices(n, 56, blosum62)
    lib = _ffi.load()
    with PairSet(pairs) as ps:
        # a fetch before any run
        w = np.zeros(1, dtype=np.uint32)
        buf = np.zeros(24 * 24, dtype=np.uint32)
        assert lib.aln_pairset_frequencies(ps.handle, w.ctypes.data, 1, buf.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        act = np.arange(n, dtype=np.uint32)
        base = ps.run(_ffi.CORE_LOCAL, 11.0, 2.0, mats, act)
        base_counts = ps.frequencies(act)
        base_summ, base_strs = ps.strings(act)
        # other pairs' matrices changed, the order of `active` reversed
        other = random_matrices(n, 57, blosum62)
        keep = np.arange(0, n, 3)
        other[keep] = mats[keep]
        rev = act[::-1].copy()
        res = ps.run(_ffi.CORE_LOCAL, 11.0, 2.0, other[rev], rev)
        counts = ps.frequencies(keep)
        summ, strs = ps.strings(keep)
        for k, i in enumerate(keep):
            assert res[n - 1 - i].tobytes() == base[i].tobytes() == summ[k].tobytes()
            assert counts[k].tobytes() == base_counts[i].tobytes()
            assert strs[k][0].tobytes() == base_strs[i][0].tobytes() and strs[k][1].tobytes() == base_strs[i][1].tobytes()
        # a subset; the second run replaces the held state, and a pair outside it is stale
        sub = np.array([7, 3, 41, 12], dtype=np.uint32)
        res = ps.run(_ffi.CORE_LOCAL, 11.0, 2.0, mats[sub], sub)
        summ, strs = ps.strings(sub[::-1].copy())
        for k, i in enumerate(sub[::-1]):
            assert summ[k].tobytes() == base[i].tobytes() and strs[k][0].tobytes() == base_strs[i][0].tobytes()
        assert res.tobytes() == base[sub].tobytes()
        stale = np.array([3, 5], dtype=np.uint32)
        out = np.full(2 * 24 * 24, 0xdeadbeef, dtype=np.uint32)
        assert lib.aln_pairset_frequencies(ps.handle, stale.ctypes.data, 2, out.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert (out == 0xdeadbeef).all()                            # nothing written
        # invalid runs write nothing and are refused: a duplicate, an index out of range, too large a shape, a matrix in params
        sentinel = np.full(2, 0xab, dtype=np.uint8).tobytes()
        r2 = np.frombuffer(bytearray(sentinel * 48), dtype=np.uint8).copy()
        two = mats[:2].copy()

        def run_raw(active, rows=24, cols=24, matrix=None):
            a = np.array(active, dtype=np.uint32)
            p = _ffi.Params(_ffi.CORE_LOCAL, 0, 11.0, 2.0, matrix, rows, cols, cols, 0, 98, 0, 0, 0, 0)
            return lib.aln_pairset_run(ps.handle, p, two.ctypes.data, a.ctypes.data, len(a), r2.ctypes.data)

        assert run_raw([4, 4]) == _ffi.ERR_INVALID_ARGUMENT
        assert run_raw([4, n]) == _ffi.ERR_INVALID_ARGUMENT
        assert run_raw([4, 5], rows=33, cols=32) == _ffi.ERR_INVALID_ARGUMENT
        assert run_raw([4, 5], matrix=two.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert r2.tobytes() == sentinel * 48
        # ... and leave the held run in place
        summ, _ = ps.strings(sub)
        assert summ.tobytes() == base[sub].tobytes()


def test_per_pair_failures_leave_the_neighbours_exact(orc, blosum62):
    from aligner_amd.pairset import PairSet
    n = 24
    pairs = random_pairs(n, 91, max_len=300, edges=False)
    pairs[3] = (pairs[3][0], np.concatenate([pairs[3][1], np.array([24], np.uint8)]))      # a code outside the matrix
    pairs[8] = (np.zeros(0, np.uint8), pairs[8][1])                                          # empty query
    pairs[15] = (pairs[15][0], np.zeros(0, np.uint8))                                        # empty target
    mats = random_matrices(n, 92, blosum62)
    mats[20] = -np.abs(mats[20]) - 0.25                                                      # no positive cell
    with PairSet(pairs) as ps:
        act = np.arange(n, dtype=np.uint32)
        res = ps.run(_ffi.CORE_LOCAL, 11.0, 2.0, mats, act)
        counts = ps.frequencies(act)
        _, strs = ps.strings(act)
    assert res["status"][3] == _ffi.ERR_CODE_OUT_OF_RANGE and res["status"][8] == _ffi.ERR_EMPTY_SEQUENCE
    assert res["status"][15] == _ffi.ERR_EMPTY_SEQUENCE and res["status"][20] == _ffi.ERR_NO_POSITIVE_CELL
    for i in range(n):
        check_pair(orc, orc.CORE_LOCAL, pairs[i], 11.0, 2.0, mats[i], res[i], strs[i], counts[i], i)
    assert (res["status"] == 0).sum() == n - 4


@pytest.mark.parametrize("how", ["numpy", "native"])
def test_align_many_equals_single_heuristic_aligners(blosum62, how):
    from aligner_amd.heuristic import HeuristicAligner, align_many
    from test_pairset_cpu import recipe_pairs
    pairs, hs = recipe_pairs(64, 808)
    got = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform=how)
    assert len(got) == 64
    for i, (q, t) in enumerate(pairs):
        want = HeuristicAligner.from_seqs(q, t, Protein).perform_alignment(11.0, 2.0, blosum62, hs[i])
        g = got[i]
        assert g.alignment.f == want.alignment.f and g.alignment.coords == want.alignment.coords and g.score == want.score, i
        assert g.alignment.query.tobytes() == want.alignment.query.tobytes(), i
        assert g.alignment.target.tobytes() == want.alignment.target.tobytes(), i
        assert g.matrix.tobytes() == np.ascontiguousarray(want.matrix).tobytes(), i
