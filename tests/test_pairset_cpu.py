"""The resident pair set and the batched heuristic loop, as far as they can be checked without a GPU: the exported symbols and their
bindings, argument validation that needs no device, aln_transform_matrices against transform_matrix and against the pure-Python
restatement of aln_transform_rules.h, and heuristic.align_many's lock-step driver on an oracle-backed pair set."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd.alignment import Alignment
from aligner_amd.enums import Protein
from aligner_amd.errors import AlignerError, ErrorKind, ReferencePanic
from aligner_amd.heuristic import WrongMatrixSpecified, align_many, transform_matrix
from aligner_amd.simple import Heuristics

import pairset_oracle_backend
import transform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["aln_pairset_create", "aln_pairset_run", "aln_pairset_frequencies", "aln_pairset_strings", "aln_pairset_stats",
       "aln_pairset_destroy", "aln_transform_matrices"]


@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def _params(semantics=_ffi.CORE_LOCAL, rows=24, cols=24, matrix=None, heuristics_present=0):
    return _ffi.Params(semantics, heuristics_present, 11.0, 2.0, matrix, rows, cols, cols, 0, 98, 0, 0, 0, 0)


def test_library_exports_the_pairset_symbols_with_the_headers_argument_counts(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aligner_hip.h")).read(), flags=re.S)
    for sym in NEW:
        assert sym in _ffi.EXPORTS and hasattr(lib, sym), sym
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert decl, sym
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert len(getattr(lib, sym).argtypes) == n_args, sym
    assert "#define ALN_PAIRSET_MAX_ENTRIES 1024u" in hdr and _ffi.PAIRSET_MAX_ENTRIES == 1024
    assert lib.aln_abi_version() == 2


def test_pairset_argument_validation_without_a_device(lib):
    st = C.c_int(-1)
    assert not lib.aln_pairset_create(None, None, None, None, None, None, 0, C.byref(st))
    assert st.value == _ffi.ERR_INVALID_ARGUMENT
    res = np.zeros(1, dtype=np.uint8)
    p = _params()
    assert lib.aln_pairset_run(None, None, None, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_run(None, C.byref(p), None, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    for sem in (_ffi.LEGACY_GLOBAL, _ffi.LEGACY_LOCAL, _ffi.PWM_LOCAL):
        p = _params(semantics=sem)
        assert lib.aln_pairset_run(None, C.byref(p), None, None, 0, None) == _ffi.ERR_UNSUPPORTED
    p = _params(semantics=17)
    assert lib.aln_pairset_run(None, C.byref(p), None, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    p = _params(heuristics_present=1)
    assert lib.aln_pairset_run(None, C.byref(p), None, None, 0, None) == _ffi.ERR_UNNECESSARY_ARGUMENT
    which = np.zeros(1, dtype=np.uint32)
    assert lib.aln_pairset_frequencies(None, which.ctypes.data, 1, res.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_strings(None, which.ctypes.data, 1, res.ctypes.data, None, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_stats(None, None, None) == _ffi.ERR_INVALID_ARGUMENT
    lib.aln_pairset_destroy(None)


def test_transform_matrices_argument_validation(lib):
    m = np.zeros((1, 4, 4)); fr = np.zeros((1, 4)); kd = np.zeros(1); r2 = np.zeros(1); out = np.zeros((1, 4, 4)); st = np.zeros(1, np.int32)
    args = [m.ctypes.data, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data, out.ctypes.data, st.ctypes.data]
    assert lib.aln_transform_matrices(0, 4, 4, *([None] * 6)) == _ffi.OK
    for hole in range(6):
        a = list(args)
        a[hole] = None
        assert lib.aln_transform_matrices(1, 4, 4, *a) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices(1, 0, 4, *args) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices(1, 128, 65, *args) == _ffi.ERR_INVALID_ARGUMENT      # 8320 entries > 8192


# ---------------------------------------------------------------- the transform
def _transform_cases(orc, blosum62):
    """(matrix, frequencies, kd, r_squared) inputs: frequency-count matrices of oracle alignments, dense random real matrices, and
    cases aimed at each root branch."""
    rng = np.random.default_rng(20240)
    cases = []
    # frequency counts of oracle alignments (the loop's own inputs), 24 x 24
    for k in range(300):
        n = int(rng.integers(40, 220))
        q = rng.integers(0, 20, n).astype(np.uint8)
        t = np.where(rng.random(n) < 0.3, rng.integers(0, 20, n), q).astype(np.uint8)
        r = orc.align(orc.CORE_LOCAL, q, t, 11.0, 2.0, blosum62)
        assert r["status"] == 0
        counts = orc.frequency_matrix(r["qa"], r["ta"], 24)
        freqs = np.bincount(t, minlength=24).astype(np.float64) / len(t)
        cases.append((counts, freqs, float(rng.choice([-0.2, -0.5, -1.0])), 576.0))
    # BLOSUM62 itself under random frequencies (iteration 0 of the loop)
    for k in range(200):
        freqs = rng.dirichlet(np.ones(24))
        cases.append((blosum62.astype(np.float64), freqs, float(rng.choice([-0.2, -0.5, -1.0, -3.0])), float(rng.choice([576.0, 100.0, 2000.0]))))
    # dense random real matrices of several shapes (sizes below 8, up to 128 and above, odd tails)
    for shape in [(2, 3), (4, 4), (5, 7), (8, 16), (11, 11), (20, 20), (24, 24), (24, 24), (32, 32), (17, 61), (64, 128)]:
        for k in range(120):
            m = rng.normal(0, 10.0 ** rng.integers(-2, 3), shape)
            freqs = rng.dirichlet(np.ones(shape[0]))
            kd = float(rng.normal(0, 1)) if k % 3 else float(rng.choice([0.5, -0.5, 2.0]))
            r2 = float(abs(rng.normal(0, shape[0] * shape[1] * 2)) + 1e-3)
            cases.append((m, freqs, kd, r2))
    # aimed at the branches: r_squared far below b^2 p2 (no root), exactly reachable (both signs), huge (opposite signs)
    for k in range(300):
        shape = (24, 24) if k % 2 else (6, 9)
        m = rng.normal(0, 3, shape)
        freqs = rng.dirichlet(np.ones(shape[0]))
        kd = float(rng.choice([-0.5, 0.7, -2.0]))
        r2 = float(10.0 ** rng.uniform(-6, 6))
        cases.append((m, freqs, kd, r2))
    # a single root: disc == 0 needs a1 == a0 == 0: kd = 0 (b = 0) and r_squared = 0
    for k in range(20):
        m = rng.normal(0, 3, (24, 24))
        cases.append((m, rng.dirichlet(np.ones(24)), 0.0, 0.0))
    # degenerate inputs: zero frequencies (NaN all the way), a zero matrix
    cases.append((rng.normal(0, 1, (24, 24)), np.zeros(24), -0.5, 576.0))
    cases.append((np.zeros((24, 24)), rng.dirichlet(np.ones(24)), -0.5, 576.0))
    return cases


def test_native_transform_equals_transform_matrix_and_the_rules_bit_for_bit(lib, orc, blosum62):
    from aligner_amd.pairset import transform_matrices
    cases = _transform_cases(orc, blosum62)
    assert len(cases) >= 2000
    branches = {"none": 0, "one": 0, "opposite": 0, "distance": 0}
    by_shape = {}
    for idx, c in enumerate(cases):
        by_shape.setdefault(c[0].shape, []).append(idx)
    native = [None] * len(cases)
    for shape, idxs in by_shape.items():
        out, status = transform_matrices(np.array([cases[i][0] for i in idxs]), np.array([cases[i][1] for i in idxs]),
                                         np.array([cases[i][2] for i in idxs]), np.array([cases[i][3] for i in idxs]))
        for k, i in enumerate(idxs):
            native[i] = (int(status[k]), out[k])
    with np.errstate(all="ignore"):
        for idx, (m, freqs, kd, r2) in enumerate(cases):
            try:
                want = transform_matrix(m, kd, r2, freqs)
            except WrongMatrixSpecified:
                want = None
            rows, cols = m.shape
            st_ref, ref, branch = transform_ref.transform([float(x) for x in m.ravel()], rows, cols, [float(x) for x in freqs], kd, r2)
            branches[branch] += 1
            st, got = native[idx]
            if want is None:
                assert st == _ffi.TRANSFORM_NO_ROOT and st_ref == transform_ref.NO_ROOT, idx
                continue
            assert st == 0 and st_ref == 0, idx
            w = np.ascontiguousarray(want, dtype=np.float64)
            assert got.tobytes() == w.tobytes(), idx                                      # bitwise, NaN payloads and signed zeros included
            # (the restatement's NaN comes from math.nan, the hardware's from 0 / 0: the sign of a NaN is not arithmetic)
            r = np.array(ref, dtype=np.float64).reshape(rows, cols)
            nan = np.isnan(w)
            assert (np.isnan(r) == nan).all() and r[~nan].tobytes() == w[~nan].tobytes(), idx
    assert all(v > 0 for v in branches.values()), branches


def test_native_transform_in_place(lib, blosum62):
    rng = np.random.default_rng(5)
    m = np.array([blosum62.astype(np.float64)] * 3)
    fr = rng.dirichlet(np.ones(24), 3)
    kd, r2, st = np.full(3, -0.5), np.full(3, 576.0), np.zeros(3, np.int32)
    want = [transform_matrix(m[k], -0.5, 576.0, fr[k]) for k in range(3)]
    assert lib.aln_transform_matrices(3, 24, 24, m.ctypes.data, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data, m.ctypes.data, st.ctypes.data) == 0
    assert (st == 0).all() and all(m[k].tobytes() == want[k].tobytes() for k in range(3))


# ---------------------------------------------------------------- the lock-step driver
def recipe_pairs(n, seed, lo=60, hi=400):
    """Random and planted-homolog protein pairs of lo .. hi residues with per-pair heuristics: kd in {-0.2, -0.5, -1.0}, r_squared 576."""
    rng = np.random.default_rng(seed)
    pairs, hs = [], []
    for k in range(n):
        nq, nt = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        q = rng.integers(0, 20, nq).astype(np.uint8)
        t = rng.integers(0, 20, nt).astype(np.uint8)
        if k % 3:                                                   # a planted homolog: a mutated stretch of the query inside the target
            L = int(rng.integers(30, min(nq, nt)))
            a, b = int(rng.integers(0, nq - L + 1)), int(rng.integers(0, nt - L + 1))
            piece = q[a:a + L].copy()
            mut = rng.random(L) < rng.uniform(0.05, 0.5)
            piece[mut] = rng.integers(0, 20, int(mut.sum()))
            t[b:b + L] = piece
        freqs = np.bincount(t, minlength=24).astype(np.float64) / len(t)
        pairs.append((q, t))
        hs.append(Heuristics(kd=float(rng.choice([-0.2, -0.5, -1.0])), r_squared=576.0, frequencies=freqs))
    return pairs, hs


def sequential_loop(orc, q, t, del_, ext, matrix, h):
    """The loop of test_heuristic_aligner_loop_matches_oracle_loop for one pair: (result dict, final matrix, iterations), or the
    status / 'wrong-matrix' the reference would panic with."""
    r2 = h.r_squared if abs(h.r_squared) >= np.finfo(np.float64).eps else float(matrix.shape[0] * matrix.shape[1])
    try:
        m = transform_matrix(matrix, h.kd, r2, h.frequencies)
    except WrongMatrixSpecified:
        return "wrong-matrix"
    max_f, iters = 0.0, 0
    while True:
        ref = orc.align(orc.CORE_LOCAL, q, t, del_, ext, m)
        if ref["status"] != 0:
            return ref["status"]
        iters += 1
        if ref["f"] > max_f:
            max_f = ref["f"]
            try:
                m = transform_matrix(Alignment(Protein, ref["qa"], ref["ta"], ref["coords"], ref["f"]).get_frequency_matrix(), h.kd, r2,
                                     h.frequencies)
            except WrongMatrixSpecified:
                return "wrong-matrix"
        else:
            return ref, m, iters


def check_against_sequential(got, want):
    if isinstance(want, tuple):
        ref, m, _iters = want
        assert not isinstance(got, Exception), got
        assert got.alignment.f == ref["f"] and got.alignment.coords == ref["coords"] and got.score == ref["score"]
        assert got.alignment.query.tolist() == ref["qa"].tolist() and got.alignment.target.tolist() == ref["ta"].tolist()
        assert got.matrix.tobytes() == np.ascontiguousarray(m).tobytes()
    else:
        assert isinstance(got, ReferencePanic)
        assert got.status == (-1 if want == "wrong-matrix" else want)


@pytest.mark.parametrize("how", ["numpy", "native"])
def test_lock_step_driver_equals_the_sequential_loop(lib, orc, blosum62, how):
    pairs, hs = recipe_pairs(120, 4242)
    made = []

    def backend(p, device):
        made.append(pairset_oracle_backend.OraclePairSet(p, device))
        return made[-1]

    got = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform=how, backend=backend)
    assert len(got) == len(pairs) and len(made) == 1 and made[0].closed
    counts = []
    for i, (q, t) in enumerate(pairs):
        want = sequential_loop(orc, q, t, 11.0, 2.0, blosum62, hs[i])
        assert isinstance(want, tuple), i
        check_against_sequential(got[i], want)                      # input order: entry i is pair i's
        assert sum(i in run for run in made[0].runs) == want[2]     # a finished pair is not run again
        counts.append(want[2])
    assert len(set(counts)) >= 3, sorted(set(counts))               # pairs finish in different iterations
    assert all(len(a) > len(b) for a, b in zip(made[0].runs, made[0].runs[1:]) if b) or len(made[0].runs) == max(counts)
    assert len(made[0].runs) == max(counts)


def test_lock_step_driver_places_the_panics(lib, orc, blosum62):
    pairs, hs = recipe_pairs(12, 99, lo=60, hi=150)
    pairs[2] = (np.zeros(0, np.uint8), pairs[2][1])                                         # empty query
    pairs[5] = (pairs[5][0], np.concatenate([pairs[5][1][:10], np.array([30], np.uint8)]))  # a code outside the matrix
    hs[7] = Heuristics(kd=-0.5, r_squared=1e-9, frequencies=hs[7].frequencies)             # no real root: WrongMatrixSpecified
    hs[9] = Heuristics(kd=-0.5, r_squared=0.0, frequencies=hs[9].frequencies)              # 0 -> rows * cols
    want = [sequential_loop(orc, q, t, 11.0, 2.0, blosum62, hs[i]) for i, (q, t) in enumerate(pairs)]
    assert want[2] == orc.ERR_EMPTY_SEQUENCE and want[5] == orc.ERR_CODE_OUT_OF_RANGE and want[7] == "wrong-matrix"
    for how in ("numpy", "native"):
        got = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform=how, errors="return",
                         backend=pairset_oracle_backend.OraclePairSet)
        for i in range(len(pairs)):
            check_against_sequential(got[i], want[i])
        with pytest.raises(ReferencePanic) as e:
            align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform=how, backend=pairset_oracle_backend.OraclePairSet)
        assert e.value.status == orc.ERR_EMPTY_SEQUENCE                                     # the first such pair in input order
    # one Heuristics for every pair
    one = align_many(pairs[:2], 11.0, 2.0, blosum62, hs[0], Protein, backend=pairset_oracle_backend.OraclePairSet)
    for i in range(2):
        check_against_sequential(one[i], sequential_loop(orc, pairs[i][0], pairs[i][1], 11.0, 2.0, blosum62, hs[0]))


def test_align_many_argument_errors(blosum62):
    pairs, hs = recipe_pairs(2, 1)
    with pytest.raises(AlignerError) as e:
        align_many(pairs, 11.0, 2.0, blosum62, None, Protein, backend=pairset_oracle_backend.OraclePairSet)
    assert e.value.kind == ErrorKind.MissingArgument
    with pytest.raises(ValueError):
        align_many(pairs, 11.0, 2.0, blosum62, hs[:1], Protein, backend=pairset_oracle_backend.OraclePairSet)
    with pytest.raises(ValueError):
        align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="device", backend=pairset_oracle_backend.OraclePairSet)
    with pytest.raises(ValueError):
        align_many(pairs, 11.0, 2.0, blosum62[:20, :20], hs, Protein, backend=pairset_oracle_backend.OraclePairSet)
    assert align_many([], 11.0, 2.0, blosum62, hs[0], Protein, backend=pairset_oracle_backend.OraclePairSet) == []
