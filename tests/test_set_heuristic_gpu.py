"""Heuristic alignment of the pairs of a resident sequence set on the GPU: a pair set that borrows the set's residues against one that
copies them, aln_pairset_loop_begin / loop_step and heuristic.align_set against align_many and single HeuristicAligners, the causes
and their places, the ordered compaction across its tile (2048 entries) and trip (256 tiles) edges, refused calls, lifetimes and
call history.

Not covered on the device: cause 2 (no root) AFTER a run.  The quadratic's linear coefficient is 2 b sum(p * base) / den, and
sum(p * base) is zero by construction of `base`, so whether a root exists depends on r_squared, kd and the frequencies only, never
on the matrix being transformed: a pair without a root has none in loop_begin already.  The cause is decided by aln_loop_rules.h
(tests/test_set_heuristic_cpu.py) and written by the same settle and select kernels that loop_begin's no-root pairs go through."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import set_loop_cases as cases  # noqa: E402

from aligner_amd import _ffi  # noqa: E402
from aligner_amd.enums import DNA, Protein  # noqa: E402
from aligner_amd.errors import ReferencePanic  # noqa: E402
from aligner_amd.simple import Heuristics  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED


def _edge_set():
    """12 sequences: lengths 0, 1, 2, 7, 63, 64, 65, 130, 300, 512, 513 and one holding a code outside the matrix."""
    rng = np.random.default_rng(1201)
    base = rng.integers(0, 20, 513).astype(np.uint8)
    seqs = []
    for n in (0, 1, 2, 7, 63, 64, 65, 130, 300, 512, 513):
        s = rng.integers(0, 20, n).astype(np.uint8)
        if n > 7:                                                    # related sequences: alignments longer than a few columns
            keep = rng.random(n) < 0.6
            s[keep] = base[:n][keep]
        seqs.append(s)
    bad = rng.integers(0, 20, 40).astype(np.uint8)
    bad[17] = 30
    seqs.append(bad)
    return seqs


def _hash(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _strings_hash(strs):
    return _hash(*[x for s in strs for x in s])


BLOCKS = {"upper": ((0, 12, 0, 12, 1), 0, None), "rectangle": ((0, 7, 1, 11, 0), 0, None), "window": ((0, 12, 0, 12, 1), 5, 37)}


def _borrowed_against_copied(blosum62, which):
    from aligner_amd.pairset import PairSet
    from aligner_amd.seqset import SeqSet
    from test_pairset_gpu import random_matrices
    seqs = _edge_set()
    b, first, n = BLOCKS[which]
    qt = cases.block_list(12, b)[first:first + n if n else None]
    assert which != "window" or (qt[0][1] != qt[0][0] + 1 and qt[-1][1] != 11)          # starts and ends inside a row
    pairs = [(seqs[q], seqs[t]) for q, t in qt]
    n = len(pairs)
    mats = random_matrices(n, 77, blosum62)
    rng = np.random.default_rng(5)
    fr = rng.dirichlet(np.ones(24), n)
    kd = rng.choice([-0.2, -0.5, -1.0], n)
    r2 = np.full(n, 576.0)
    act = np.arange(n, dtype=np.uint32)
    out = []
    with SeqSet(seqs) as ss:
        for make in (lambda: PairSet.from_seqset(ss, b, first, n), lambda: PairSet(pairs)):
            with make() as ps:
                up = ps.stats()["bytes_up"]
                res = ps.run(_ffi.CORE_LOCAL, 11.0, 2.0, mats, act)
                summ, strs = ps.strings(act)
                counts = ps.frequencies(act)
                ps.set_heuristics(24, 24, fr, kd, r2)
                st0 = ps.reestimate(act, matrix=blosum62)
                st1 = ps.reestimate(act[res["status"] == 0])
                assert (st0 == 0).all() and (st1 == 0).all()
                res2 = ps.run_stored(_ffi.CORE_LOCAL, 11.0, 2.0, act)
                summ2, strs2 = ps.strings(act)
                store = ps.matrices(act)
                out.append((up, res["status"].tolist(), res2["status"].tolist(),
                            _hash(res, summ, counts, res2, summ2, store), _strings_hash(strs), _strings_hash(strs2)))
                if hasattr(ps, "q"):
                    assert [(int(a), int(c)) for a, c in zip(ps.q, ps.t)] == qt
    assert out[0][0] == 0 and out[1][0] == sum(len(q) + len(t) for q, t in pairs)         # nothing uploaded against sum over pairs
    assert out[0][1:] == out[1][1:]
    st = set(out[0][1])
    assert _ffi.ERR_CODE_OUT_OF_RANGE in st and 0 in st and (which == "window" or _ffi.ERR_EMPTY_SEQUENCE in st)
    return n


@pytest.mark.parametrize("which", sorted(BLOCKS))
def test_borrowed_residues_equal_copied_residues(blosum62, which):
    _borrowed_against_copied(blosum62, which)


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd.matrices import get_blosum62
import test_set_heuristic_gpu as T
print("pairs", T._borrowed_against_copied(get_blosum62(), "upper"))
print("CHILD-OK")
"""


def test_borrowed_residues_across_chunks():
    """ALN_CHUNK_CELLS small enough for several chunks (66 pairs, 1.6e6 cells), set in a child as the existing chunk tests do."""
    env = dict(os.environ, ALN_CHUNK_CELLS="200000")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------- the loop against what we already trust
def _protein_set(n=14, seed=31):
    from test_pairset_cpu import recipe_pairs
    pairs, _ = recipe_pairs(n, seed, lo=60, hi=300)
    seqs = [q for q, _ in pairs]
    for i in range(1, n):                                            # relatives: a mutated stretch of the sequence before
        rng = np.random.default_rng(seed + i)
        L = min(len(seqs[i]), len(seqs[i - 1]), 50)
        piece = seqs[i - 1][:L].copy()
        mut = rng.random(L) < 0.3
        piece[mut] = rng.integers(0, 20, int(mut.sum()))
        seqs[i][-L:] = piece
    return seqs


def _heur_for(seqs, volume):
    def h(q, t):
        fr = np.bincount(seqs[t], minlength=volume).astype(np.float64) / max(len(seqs[t]), 1)
        return Heuristics(kd=[-0.2, -0.5, -1.0][(q + 2 * t) % 3], r_squared=0.0 if (q + t) % 4 == 0 else float(volume * volume), frequencies=fr)
    return h


def _result_bytes(r):
    return (np.float64(r.alignment.f).tobytes() + repr(r.alignment.coords).encode() + np.float64(r.score).tobytes() +
            r.alignment.query.tobytes() + r.alignment.target.tobytes() + np.ascontiguousarray(r.matrix).tobytes())


def _same(a, b):
    if isinstance(b, ReferencePanic):
        return isinstance(a, ReferencePanic) and a.status == b.status and str(a) == str(b)
    return not isinstance(a, Exception) and _result_bytes(a) == _result_bytes(b)


def _many_counted(pairs, del_, ext, matrix, hs, alphabet, transform):
    """align_many on a recording pair set: (results, per pair the number of runs whose active list names it)."""
    from aligner_amd.heuristic import align_many
    from aligner_amd.pairset import PairSet
    runs = np.zeros(len(pairs), dtype=np.int64)

    class Recording(PairSet):
        def run(self, semantics, d, e, matrices, active, **kw):
            runs[np.asarray(active, dtype=np.int64)] += 1
            return PairSet.run(self, semantics, d, e, matrices, active, **kw)

        def run_stored(self, semantics, d, e, active, **kw):
            runs[np.asarray(active, dtype=np.int64)] += 1
            return PairSet.run_stored(self, semantics, d, e, active, **kw)

    return align_many(pairs, del_, ext, matrix, hs, alphabet, transform=transform, errors="return", backend=Recording), runs


def _set_counted(ss, total, del_, ext, matrix, h, **kw):
    """align_set on recording derived pair sets: (yields, per pair the loop_step of its slice at which it came back as finished; 0 for
    a pair that never ran)."""
    from aligner_amd.heuristic import align_set
    from aligner_amd.pairset import PairSet
    steps = np.zeros(total, dtype=np.int64)

    class Recording:
        def __init__(self, seqset, b, first, n):
            self.ps, self.first, self.step = PairSet.from_seqset(seqset, b, first, n), first, 0
            self.q, self.t = self.ps.q, self.ps.t

        def loop_step(self, *a, **k):
            self.step += 1
            out = self.ps.loop_step(*a, **k)
            assert (steps[self.first + out[0].astype(np.int64)] == 0).all()          # a pair finishes once
            steps[self.first + out[0].astype(np.int64)] = self.step
            return out

        def __getattr__(self, name):
            return getattr(self.ps, name)

    return list(align_set(ss, del_, ext, matrix, h, backend=Recording, **kw)), steps


@pytest.mark.parametrize("del_,ext", [(8.0, 8.0), (11.0, 2.0)])
def test_align_set_equals_align_many_and_single_aligners(orc, blosum62, del_, ext):
    from aligner_amd.heuristic import HeuristicAligner
    from aligner_amd.seqset import SeqSet
    seqs = _protein_set()
    h = _heur_for(seqs, 24)
    qt = cases.block_list(14, (0, 14, 0, 14, 1))
    assert len(qt) == 91
    pairs = [(seqs[q], seqs[t]) for q, t in qt]
    hs = [h(q, t) for q, t in qt]
    with SeqSet(seqs) as ss:
        got, steps = _set_counted(ss, 91, del_, ext, blosum62, h, max_pairs=40)          # three slices, cut inside rows
    assert [(g[0], g[1], g[2]) for g in got] == [(k, q, t) for k, (q, t) in enumerate(qt)]
    resident, runs_resident = _many_counted(pairs, del_, ext, blosum62, hs, Protein, "resident")
    native, runs_native = _many_counted(pairs, del_, ext, blosum62, hs, Protein, "native")
    # per-pair iteration counts: the step at which the set's loop hands a pair back is the number of runs align_many gives it
    print("iterations", steps.tolist())
    assert steps.tolist() == runs_resident.tolist() and steps.tolist() == runs_native.tolist()
    assert steps.min() >= 2 and len(set(steps.tolist())) >= 2
    ok = 0
    for k in range(91):
        assert _same(got[k][3], resident[k]) and _same(got[k][3], native[k]), k
        g = got[k][3]
        if isinstance(g, Exception):
            continue
        ok += 1
        # the returned alignment is the oracle's under the returned matrix
        ref = orc.align(orc.CORE_LOCAL, pairs[k][0], pairs[k][1], del_, ext, g.matrix)
        assert ref["status"] == 0 and g.alignment.f == ref["f"] and g.alignment.coords == ref["coords"], k
        assert g.alignment.query.tobytes() == ref["qa"].tobytes() and g.alignment.target.tobytes() == ref["ta"].tobytes(), k
    assert ok >= 85
    for k in range(0, 91, 10):
        want = HeuristicAligner.from_seqs(pairs[k][0], pairs[k][1], Protein).perform_alignment(del_, ext, blosum62, hs[k])
        assert _same(got[k][3], want), k


def test_align_set_on_a_dna_shaped_set(orc):
    from aligner_amd.seqset import SeqSet
    rng = np.random.default_rng(404)
    seqs = [rng.integers(0, 4, int(rng.integers(5, 200))).astype(np.uint8) for _ in range(9)]
    for i in range(1, 9):
        L = min(len(seqs[i]), len(seqs[i - 1]), 30)
        seqs[i][:L] = seqs[i - 1][-L:]
    h = Heuristics(kd=-0.5, r_squared=0.0, frequencies=np.full(4, 0.25))
    b = (0, 4, 3, 6, 0)
    qt = cases.block_list(9, b)
    with SeqSet(seqs, DNA) as ss:
        got, steps = _set_counted(ss, len(qt), 6.0, 1.0, cases.DNA_MATRIX, h, block=b)
    pairs = [(seqs[q], seqs[t]) for q, t in qt]
    want, runs = _many_counted(pairs, 6.0, 1.0, cases.DNA_MATRIX, h, DNA, "resident")
    native, runs_native = _many_counted(pairs, 6.0, 1.0, cases.DNA_MATRIX, h, DNA, "native")
    assert [(g[1], g[2]) for g in got] == qt
    print("iterations", steps.tolist())
    assert steps.tolist() == runs.tolist() and steps.tolist() == runs_native.tolist() and steps.min() >= 2
    assert all(_same(a, b) for a, b in zip(want, native))
    for k in range(len(qt)):
        assert _same(got[k][3], want[k]), k
        ref = orc.align(orc.CORE_LOCAL, seqs[qt[k][0]], seqs[qt[k][1]], 6.0, 1.0, got[k][3].matrix)
        assert got[k][3].alignment.f == ref["f"] and got[k][3].alignment.query.tobytes() == ref["qa"].tobytes(), k


def test_causes_and_their_places(blosum62):
    """An empty sequence, a code outside the matrix, a pair with no positive cell and parameters without a root (loop_begin): the
    panics are align_many's, in its places, and the neighbours' bytes are unchanged."""
    from aligner_amd.heuristic import align_many, align_set
    from aligner_amd.seqset import SeqSet
    seqs = _protein_set(8, 77)
    seqs[2] = np.zeros(0, np.uint8)
    seqs[5] = np.concatenate([seqs[5][:10], np.array([30], np.uint8)])
    seqs[6] = np.full(3, 18, np.uint8)                              # against seqs[7]: nothing scores above zero
    seqs[7] = np.full(4, 5, np.uint8)

    def h(q, t):
        fr = np.bincount(np.minimum(seqs[t], 23), minlength=24).astype(np.float64) / max(len(seqs[t]), 1)
        return Heuristics(kd=-0.5, r_squared=1e-9 if (q, t) in ((0, 1), (3, 4)) else 576.0, frequencies=fr)

    qt = cases.block_list(8, (0, 8, 0, 8, 1))
    pairs = [(seqs[q], seqs[t]) for q, t in qt]
    hs = [h(q, t) for q, t in qt]
    with SeqSet(seqs) as ss:
        got = list(align_set(ss, 11.0, 2.0, blosum62, h))
        clean = {(q, t): r for _, q, t, r in align_set(ss, 11.0, 2.0, blosum62, h, block=(0, 2, 3, 2, 0))}
    want = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="resident", errors="return")
    kinds = set()
    for k, (q, t) in enumerate(qt):
        assert _same(got[k][3], want[k]), (k, q, t)
        if isinstance(want[k], ReferencePanic):
            kinds.add(want[k].status)
    assert kinds >= {-1, _ffi.ERR_EMPTY_SEQUENCE, _ffi.ERR_CODE_OUT_OF_RANGE, _ffi.ERR_NO_POSITIVE_CELL}, kinds
    # the same pairs named through a block without any failing pair: the same bytes
    for (q, t), r in clean.items():
        assert _same(got[qt.index((q, t))][3], r), (q, t)
    with SeqSet(seqs) as ss:
        with pytest.raises(ReferencePanic):
            list(align_set(ss, 11.0, 2.0, blosum62, h, errors="raise"))


# ---------------------------------------------------------------- ordered compaction across tile and trip edges
S_DNA = 805          # 805 x 805 pairs, five in six with a root: more than 2^19 + 1 going, a second trip of the offsets kernel (256
                     # tiles of 2048 entries a trip); the last row (content 6) holds pairs that finish at step 2


@pytest.fixture(scope="module")
def dna_case(orc):
    table = cases.dna_table(orc)
    nc, npar = len(cases.DNA_CONTENTS), len(cases.DNA_PARAMS)
    begin = np.zeros((nc, nc, npar), dtype=bool)
    cause = np.zeros((nc, nc, npar), dtype=np.uint32)
    step = np.zeros((nc, nc, npar), dtype=np.int64)
    status = np.zeros((nc, nc, npar), dtype=np.int32)
    f = np.zeros((nc, nc, npar))
    for (a, b, p), r in table.items():
        begin[a, b, p], cause[a, b, p], step[a, b, p], status[a, b, p], f[a, b, p] = r["begin"], r["cause"], r["step"], r["status"], r["f"]
    # the table is not vacuous: pairs finish at different steps, and every cause the device can show is there
    ok_steps = set(step[(cause == cases.DONE) & ~begin].tolist())
    assert len(ok_steps) >= 2 and begin.any() and (cause[~begin] == cases.FAILED).any() and (cause[~begin] == cases.DONE).any(), ok_steps
    seqs = [np.array(cases.DNA_CONTENTS[cases.dna_content_of(s)], np.uint8) for s in range(S_DNA)]
    k = np.arange(S_DNA * S_DNA, dtype=np.int64)
    q, t = k // S_DNA, k % S_DNA
    par = cases.dna_param_of(q, t)
    cq, ct = cases.dna_content_of(q), cases.dna_content_of(t)
    return dict(seqs=seqs, par=par, begin=begin[cq, ct, par], cause=cause[cq, ct, par], step=step[cq, ct, par], status=status[cq, ct, par],
                f=f[cq, ct, par])


def _window_for(case, first, going):
    """n such that pairs first .. first + n - 1 hold exactly `going` pairs with a root."""
    c = np.cumsum(~case["begin"][first:])
    return int(np.searchsorted(c, going) + 1)


@pytest.mark.parametrize("first,going", [(3, 1), (700, 63), (1500, 64), (31, 65), (5000, 2047), (11, 2048), (100000, 2049), (0, None)])
def test_ordered_compaction_across_tile_and_trip_edges(dna_case, first, going):
    from aligner_amd.pairset import PairSet
    from aligner_amd.seqset import SeqSet
    case = dna_case
    n = S_DNA * S_DNA if going is None else _window_for(case, first, going)
    sl = slice(first, first + n)
    par, begin, cause, step, status, f = (case[x][sl] for x in ("par", "begin", "cause", "step", "status", "f"))
    if going is None:
        going = int((~begin).sum())
        assert going > (1 << 19) + 1
    assert int((~begin).sum()) == going
    tab = cases.DNA_PARAMS
    fr = np.array([p[2] for p in tab])[par]
    kd = np.array([p[0] for p in tab])[par]
    r2 = np.array([p[1] for p in tab])[par]
    lib = _ffi.load()
    with SeqSet(case["seqs"], DNA) as ss, PairSet.from_seqset(ss, (0, S_DNA, 0, S_DNA, 0), first, n) as ps:
        ps.set_heuristics(4, 4, fr, kd, r2)
        st = ps.loop_begin(cases.DNA_MATRIX)
        assert (st == np.where(begin, _ffi.TRANSFORM_NO_ROOT, 0)).all()
        G = np.flatnonzero(~begin).astype(np.uint32)
        best = np.zeros(n)                                          # numpy's copy of the resident best f
        s = 0
        while len(G):
            s += 1
            fin, cz, res, counts = ps.loop_step(_ffi.CORE_LOCAL, cases.DNA_DEL, cases.DNA_EXT, blank=DNA.blank())
            down = ps.stats()["bytes_down"]
            ends = step[G] == s
            want = G[ends]
            assert counts[0] == len(G) and counts[3] == len(G) - len(want), (s, counts)             # it ran exactly the complement
            assert fin.tobytes() == want.tobytes(), s                                                 # ascending going order
            assert (cz == cause[want]).all() and (res["status"] == status[want]).all(), s
            assert counts[1] == int((cause[want] == cases.DONE).sum()) and counts[2] == len(want) - counts[1], (s, counts)
            assert (res["f"][cz == cases.DONE] == f[want][cz == cases.DONE]).all(), s
            assert down == 12 + 56 * len(want), (s, down)                                             # nothing for the pairs that go on
            # the whole step's summaries, fetched before the next step, classify as the rule says against the replayed best
            held = np.zeros(len(G), dtype=res.dtype)
            assert lib.aln_pairset_strings(ps.handle, G.ctypes.data, len(G), held.ctypes.data, None, None) == 0
            assert ((held["status"] != 0) == (ends & (cause[G] == cases.FAILED))).all(), s
            with np.errstate(invalid="ignore"):
                cls = np.where(held["status"] != 0, cases.FAILED, np.where(held["f"] > best[G], 3, cases.DONE)).astype(np.uint32)
            norootnow = ends & (cause[G] == cases.NO_ROOT)          # (none: a pair without a root has none in loop_begin)
            cls[norootnow & (cls == 3)] = cases.NO_ROOT
            assert fin.tobytes() == G[cls != 3].tobytes() and cz.tobytes() == cls[cls != 3].tobytes(), s
            assert res.tobytes() == held[cls != 3].tobytes(), s
            assert counts == (len(G), int((cls == 0).sum()), int(((cls == 1) | (cls == 2)).sum()), int((cls == 3).sum())), (s, counts)
            best[G[cls == 3]] = held["f"][cls == 3]
            if s == 2 and len(G) > 3 * 2048:                                                          # both kinds in the first, a middle, the last tile
                tiles = (len(G) + 2047) // 2048
                mixed = [bool(ends[x * 2048:(x + 1) * 2048].any() and not ends[x * 2048:(x + 1) * 2048].all()) for x in range(tiles)]
                assert mixed[0] and mixed[-1] and any(mixed[tiles // 4:3 * tiles // 4]), (tiles, mixed[0], mixed[-1])      # (the replay's, not the device's)
            if len(G) > (1 << 19):                                                                    # failed pairs on both sides of a tile and the trip edge
                bad = ends & (cause[G] == cases.FAILED)
                for edge in (2048, 1 << 19):
                    assert bad[edge - 64:edge].any() and bad[edge:edge + 64].any(), edge
            G = G[~ends]
        assert s == int(step[~begin].max())
        fin, cz, res, counts = ps.loop_step(_ffi.CORE_LOCAL, cases.DNA_DEL, cases.DNA_EXT, blank=DNA.blank())
        assert counts == (0, 0, 0, 0) and len(fin) == 0


# ---------------------------------------------------------------- refused calls, lifetimes, call history
def _drive(ps, blosum62, fr, kd, r2, between=None, steps=8):
    """The loop on a pair set, hashed: every step's outputs, the finished pairs' strings and matrices."""
    ps.set_heuristics(24, 24, fr, kd, r2)
    h = [_hash(ps.loop_begin(blosum62))]
    for s in range(steps):
        if between:
            between(s)
        fin, cz, res, counts = ps.loop_step(_ffi.CORE_LOCAL, 11.0, 2.0)
        done = fin[cz == 0]
        summ, strs = ps.strings(fin)
        h.append(_hash(fin, cz, res, np.array(counts), summ, ps.matrices(done)) + _strings_hash(strs))
        if counts[3] == 0:
            break
    return h


def test_refused_calls_lifetimes_and_call_history(blosum62):
    from aligner_amd import runtime
    from aligner_amd.pairset import PairSet
    from aligner_amd.seqset import SeqSet
    from test_pairset_gpu import random_pairs
    seqs = _protein_set(9, 5)
    n = 36
    rng = np.random.default_rng(9)
    fr = rng.dirichlet(np.ones(24), n)
    kd = rng.choice([-0.2, -0.5, -1.0], n)
    r2 = np.full(n, 576.0)
    r2[4] = 1e-9
    lib = _ffi.load()
    ctx = runtime.context()
    blk = _ffi.SeqsetBlock(0, 9, 0, 9, 1, 0)
    st = C.c_int(-1)
    with SeqSet(seqs) as ss:
        # creation refused: nothing created
        assert not lib.aln_pairset_create_from_set(None, C.byref(blk), 0, 1, C.byref(st)) and st.value == INVALID
        assert not lib.aln_pairset_create_from_set(ss.handle, None, 0, 1, C.byref(st)) and st.value == INVALID
        bad = _ffi.SeqsetBlock(0, 9, 1, 9, 1, 0)
        assert not lib.aln_pairset_create_from_set(ss.handle, C.byref(bad), 0, 1, C.byref(st)) and st.value == INVALID
        assert not lib.aln_pairset_create_from_set(ss.handle, C.byref(blk), 30, 7, C.byref(st)) and st.value == INVALID
        assert not lib.aln_pairset_create_from_set(ss.handle, C.byref(blk), 37, 0, C.byref(st)) and st.value == INVALID
        with PairSet.from_seqset(ss) as ps:
            base = _drive(ps, blosum62, fr, kd, r2)
        assert len(base) >= 3

        fin, cz = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        res, cnt = np.zeros(n * 48, np.uint8), np.full(4, 99, np.uint32)

        def step(ps, p, outs=None):
            o = outs or (fin.ctypes.data, cz.ctypes.data, res.ctypes.data, cnt.ctypes.data)
            return lib.aln_pairset_loop_step(ps.handle, C.byref(p), *o)

        def params(sem=_ffi.CORE_LOCAL, rows=24, cols=24, matrix=None):
            return _ffi.Params(sem, 0, 11.0, 2.0, matrix, rows, cols, cols, 0, 98, 0, 0, 0, 0)

        b62 = np.ascontiguousarray(blosum62, dtype=np.float64)

        def refused(s):
            if s != 1:
                return
            assert step(ps2, params(rows=20, cols=20)) == INVALID and step(ps2, params(cols=23)) == INVALID
            assert step(ps2, params(matrix=b62.ctypes.data)) == INVALID
            assert step(ps2, params(), (None, cz.ctypes.data, res.ctypes.data, cnt.ctypes.data)) == INVALID
            assert step(ps2, params(), (fin.ctypes.data, cz.ctypes.data, res.ctypes.data, None)) == INVALID
            for sem in (_ffi.LEGACY_GLOBAL, _ffi.LEGACY_LOCAL, _ffi.PWM_LOCAL):
                assert step(ps2, params(sem=sem)) == UNSUPPORTED
            assert (cnt == 99).all() and not fin.any() and not res.any()
            # passes on the set between two steps
            f, stt = ss.score(blosum62, 11.0, 2.0)
            ss.hits(blosum62, 11.0, 2.0, 30.0)
            assert len(f) == 36
        with PairSet.from_seqset(ss) as ps2:
            nb = np.zeros(n, np.int32)
            assert lib.aln_pairset_loop_begin(ps2.handle, b62.ctypes.data, nb.ctypes.data) == INVALID      # no heuristics yet
            assert _drive(ps2, blosum62, fr, kd, r2, between=refused) == base

        # call history: an unrelated batch run and a held pass of another set on the same context between steps
        other = random_pairs(24, 3, max_len=300)
        from test_pairset_resident_gpu import _batch_bytes
        before = _batch_bytes(other, blosum62)
        with SeqSet(_edge_set()[3:11]) as ss2, PairSet.from_seqset(ss) as ps3:
            def history(s):
                assert _batch_bytes(other, blosum62) == before
                ss2.hits(blosum62, 11.0, 2.0, 20.0)
            assert _drive(ps3, blosum62, fr, kd, r2, between=history) == base

    # the set destroyed before its pair set: the residues stay until the pair set goes
    ss = SeqSet(seqs)
    ps4 = PairSet.from_seqset(ss)
    ps5 = PairSet.from_seqset(ss, first=3, n=10)
    ss.close()
    ps5.close()
    assert _drive(ps4, blosum62, fr, kd, r2) == base
    ps4.close()
