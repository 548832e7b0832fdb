"""The device form of the matrix transform as far as it can be checked without a GPU: the 64-lane split of the numpy-order sum
(aln_transform_rules.h, the text the kernel compiles) replayed lane by lane on the host for every n the pair set allows, the
lock-step driver of heuristic.align_many in "resident" mode on an oracle-backed pair set, and the argument checks of the five new
exports that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from aligner_amd import _ffi
from aligner_amd.enums import Protein
from aligner_amd.errors import ReferencePanic
from aligner_amd.heuristic import WrongMatrixSpecified, align_many, transform_matrix
from aligner_amd.simple import Heuristics

import pairset_oracle_backend
from test_pairset_cpu import check_against_sequential, recipe_pairs, sequential_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 1024

DRIVER = r"""
#include "aln_transform_rules.h"
extern "C" {
// the wave's run of the sum, lane after lane; returns the number of leaves, or -1
int lanes_sum(const double *a, size_t n, double *out)
{
    aln_np_sum_plan pl;
    if (aln_np_sum_plan_make(n, &pl) != 0) return -1;
    double part[64 * ALN_NP_SUM_ROUNDS];
    for (uint32_t r = 0; r < ALN_NP_SUM_ROUNDS; ++r)
        for (uint32_t lane = 0; lane < 64; ++lane) part[r * 64 + lane] = aln_np_sum_lane_partial(&pl, a, lane, r);
    *out = aln_np_sum_combine(&pl, a, part);
    return (int)pl.n_leaves;
}
double rules_sum(const double *a, size_t n) { return aln_np_sum(a, n); }
int leaf_table(size_t n, unsigned *off, unsigned *len)
{
    aln_np_sum_plan pl;
    if (aln_np_sum_plan_make(n, &pl) != 0) return -1;
    for (uint32_t k = 0; k < pl.n_leaves; ++k) { off[k] = pl.off[k]; len[k] = pl.len[k]; }
    return (int)pl.n_leaves;
}
unsigned max_n(void) { return ALN_NP_SUM_MAX_N; }
unsigned max_leaves(void) { return ALN_NP_SUM_MAX_LEAVES; }
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build the transform-rule driver" % cxx)
    tmp = tmp_path_factory.mktemp("transform_rules")
    src, so = os.path.join(str(tmp), "drv.cpp"), os.path.join(str(tmp), "librules.so")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "aligner_amd", "csrc"), src, "-o", so])
    lib = C.CDLL(so)
    lib.lanes_sum.restype = C.c_int
    lib.lanes_sum.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
    lib.rules_sum.restype = C.c_double
    lib.rules_sum.argtypes = [C.c_void_p, C.c_size_t]
    lib.leaf_table.restype = C.c_int
    lib.leaf_table.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    lib.max_n.restype = lib.max_leaves.restype = C.c_uint
    return lib


@pytest.fixture(scope="module")
def lib():
    from aligner_amd import build as native_build
    native_build.build()
    return _ffi.load()


def _sum_inputs():
    """Arrays of MAX_N doubles whose prefixes are summed: magnitudes over sixteen decades with both signs; values that cancel (x, -x
    next to each other, eight apart -- the same running sum -- and a leaf apart); negative zeros; integer counts (the loop's input)."""
    rng = np.random.default_rng(20261017)
    out = []
    a = rng.normal(0, 1, MAX_N) * 10.0 ** rng.integers(-8, 9, MAX_N)
    out.append(a)
    b = rng.normal(0, 1, MAX_N) * 10.0 ** rng.integers(-3, 4, MAX_N)
    b[1::2] = -b[0::2]
    b[5::16] = 1e16
    out.append(b)
    c = rng.normal(0, 1e6, MAX_N)
    c[8:MAX_N:16] = -c[0:MAX_N - 8:16]
    c[72:MAX_N] -= c[0:MAX_N - 72]
    out.append(c)
    d = rng.integers(0, 40, MAX_N).astype(np.float64)
    d[rng.random(MAX_N) < 0.5] = 0.0
    d[::7] = -0.0
    out.append(d)
    out.append(np.full(MAX_N, -0.0))
    return out


def test_lane_sum_equals_the_rules_sum_and_numpy_for_every_n(rules):
    assert rules.max_n() == MAX_N == _ffi.PAIRSET_MAX_ENTRIES
    got = C.c_double()
    leaves_seen = set()
    for a in _sum_inputs():
        for n in range(1, MAX_N + 1):
            x = np.ascontiguousarray(a[:n])
            leaves = rules.lanes_sum(x.ctypes.data, n, C.byref(got))
            assert 1 <= leaves <= rules.max_leaves(), n
            leaves_seen.add(leaves)
            lane = np.float64(got.value).tobytes()
            assert lane == np.float64(rules.rules_sum(x.ctypes.data, n)).tobytes(), n
            assert lane == np.float64(x.sum()).tobytes(), n
    assert {1, 2, 4, 8}.issubset(leaves_seen) and max(leaves_seen) > 8, sorted(leaves_seen)      # two rounds of lanes are exercised
    assert rules.lanes_sum(None, 0, C.byref(got)) == -1 and rules.lanes_sum(None, MAX_N + 1, C.byref(got)) == -1


def test_leaf_table_is_numpys_tree(rules):
    off, ln = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
    assert rules.leaf_table(576, off.ctypes.data, ln.ctypes.data) == 8                  # 24 x 24: eight leaves of 72
    assert ln[:8].tolist() == [72] * 8 and off[:8].tolist() == list(range(0, 576, 72))

    def leaves(o, n):
        if n <= 128:
            return [(o, n)]
        h = n // 2
        h -= h % 8
        return leaves(o, h) + leaves(o + h, n - h)

    for n in list(range(1, 300)) + [511, 512, 513, 1000, 1016, 1023, 1024]:
        k = rules.leaf_table(n, off.ctypes.data, ln.ctypes.data)
        assert list(zip(off[:k].tolist(), ln[:k].tolist())) == leaves(0, n), n


# ---------------------------------------------------------------- the lock-step driver in "resident" mode
class ResidentOraclePairSet(pairset_oracle_backend.OraclePairSet):
    """The four methods of the resident matrices, with transform_matrix on the host."""

    def set_heuristics(self, rows, cols, frequencies, kd, r_squared):
        self.store_shape = (rows, cols)
        self.h = (np.array(frequencies, dtype=np.float64), np.array(kd, dtype=np.float64), np.array(r_squared, dtype=np.float64))
        assert self.h[0].shape == (len(self.pairs), rows) and self.h[1].shape == self.h[2].shape == (len(self.pairs),)
        self.store = {}
        self.calls = []

    def reestimate(self, which, matrix=None):
        assert len(set(which)) == len(which)
        self.calls.append("reestimate")
        src = [np.asarray(matrix, dtype=np.float64)] * len(which) if matrix is not None else self.frequencies(which).astype(np.float64)
        status = np.zeros(len(which), dtype=np.int32)
        for k, i in enumerate(which):
            try:
                self.store[i] = transform_matrix(src[k], self.h[1][i], self.h[2][i], self.h[0][i])
            except WrongMatrixSpecified:
                status[k] = _ffi.TRANSFORM_NO_ROOT
        return status

    def run_stored(self, semantics, del_, ext, active, blank=98, **kw):
        self.calls.append("run_stored")
        return self.run(semantics, del_, ext, np.array([self.store[i] for i in active]), active, blank=blank, **kw)

    def matrices(self, which):
        self.calls.append("matrices")
        return np.array([self.store[i] for i in which]).reshape((len(which),) + tuple(self.store_shape))


def test_resident_driver_equals_the_sequential_loop(lib, orc, blosum62):
    pairs, hs = recipe_pairs(120, 4242)
    made = []

    def backend(p, device):
        made.append(ResidentOraclePairSet(p, device))
        return made[-1]

    got = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="resident", backend=backend)
    assert len(got) == len(pairs) and len(made) == 1 and made[0].closed
    counts = []
    for i, (q, t) in enumerate(pairs):
        want = sequential_loop(orc, q, t, 11.0, 2.0, blosum62, hs[i])
        assert isinstance(want, tuple), i
        check_against_sequential(got[i], want)
        assert sum(i in run for run in made[0].runs) == want[2]     # a finished pair is not run again
        counts.append(want[2])
    assert len(made[0].runs) == max(counts)
    # the parameters went up once, the first matrices came from the shared one, and no run took matrices from the host
    assert made[0].calls[0] == "reestimate" and made[0].calls.count("run_stored") == len(made[0].runs)


def test_resident_driver_places_the_panics(lib, orc, blosum62):
    pairs, hs = recipe_pairs(12, 99, lo=60, hi=150)
    pairs[2] = (np.zeros(0, np.uint8), pairs[2][1])                                         # empty query
    pairs[5] = (pairs[5][0], np.concatenate([pairs[5][1][:10], np.array([30], np.uint8)]))  # a code outside the matrix
    hs[7] = Heuristics(kd=-0.5, r_squared=1e-9, frequencies=hs[7].frequencies)             # no real root: WrongMatrixSpecified
    hs[9] = Heuristics(kd=-0.5, r_squared=0.0, frequencies=hs[9].frequencies)              # 0 -> rows * cols
    want = [sequential_loop(orc, q, t, 11.0, 2.0, blosum62, hs[i]) for i, (q, t) in enumerate(pairs)]
    assert want[2] == orc.ERR_EMPTY_SEQUENCE and want[5] == orc.ERR_CODE_OUT_OF_RANGE and want[7] == "wrong-matrix"
    got = align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="resident", errors="return", backend=ResidentOraclePairSet)
    for i in range(len(pairs)):
        check_against_sequential(got[i], want[i])
    with pytest.raises(ReferencePanic) as e:
        align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="resident", backend=ResidentOraclePairSet)
    assert e.value.status == orc.ERR_EMPTY_SEQUENCE                                         # the first such pair in input order
    with pytest.raises(ValueError):                                                         # the name is "resident"
        align_many(pairs, 11.0, 2.0, blosum62, hs, Protein, transform="device", backend=ResidentOraclePairSet)


# ---------------------------------------------------------------- the exports
NEW = ["aln_pairset_heuristics", "aln_pairset_reestimate", "aln_pairset_run_stored", "aln_pairset_matrices", "aln_transform_matrices_device"]


def test_new_exports_are_bound(lib):
    for sym in NEW:
        assert sym in _ffi.EXPORTS and hasattr(lib, sym) and getattr(lib, sym).argtypes, sym
    assert lib.aln_abi_version() == 2
    from aligner_amd.pairset import PairSet
    for name in ("set_heuristics", "reestimate", "run_stored", "matrices"):
        assert callable(getattr(PairSet, name))


def test_argument_validation_without_a_device(lib):
    buf = np.zeros(64, dtype=np.float64)
    which = np.zeros(1, dtype=np.uint32)
    st = np.zeros(1, dtype=np.int32)
    d = buf.ctypes.data
    assert lib.aln_pairset_heuristics(None, 4, 4, d, d, d) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_reestimate(None, None, which.ctypes.data, 1, st.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_reestimate(None, d, which.ctypes.data, 1, st.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_matrices(None, which.ctypes.data, 1, d) == _ffi.ERR_INVALID_ARGUMENT
    p = _ffi.Params(_ffi.CORE_LOCAL, 0, 11.0, 2.0, None, 4, 4, 4, 0, 98, 0, 0, 0, 0)
    assert lib.aln_pairset_run_stored(None, None, None, 0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_pairset_run_stored(None, C.byref(p), which.ctypes.data, 1, d) == _ffi.ERR_INVALID_ARGUMENT
    for sem in (_ffi.LEGACY_GLOBAL, _ffi.LEGACY_LOCAL, _ffi.PWM_LOCAL):                    # the checks of aln_pairset_run, in its order
        p = _ffi.Params(sem, 0, 11.0, 2.0, None, 4, 4, 4, 0, 98, 0, 0, 0, 0)
        assert lib.aln_pairset_run_stored(None, C.byref(p), None, 0, None) == _ffi.ERR_UNSUPPORTED
    p = _ffi.Params(_ffi.CORE_LOCAL, 1, 11.0, 2.0, None, 4, 4, 4, 0, 98, 0, 0, 0, 0)
    assert lib.aln_pairset_run_stored(None, C.byref(p), None, 0, None) == _ffi.ERR_UNNECESSARY_ARGUMENT
    # the device transform: a null context, and with n == 0 nothing is looked at beyond it
    m = np.zeros((1, 4, 4)); fr = np.zeros((1, 4)); kd = np.zeros(1); r2 = np.zeros(1); out = np.full((1, 4, 4), 7.0)
    args = [m.ctypes.data, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data, out.ctypes.data, st.ctypes.data]
    assert lib.aln_transform_matrices_device(None, 1, 4, 4, *args) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices_device(None, 0, 4, 4, *args) == _ffi.ERR_INVALID_ARGUMENT
    assert (out == 7.0).all()


def test_device_transform_shape_bounds_need_no_device(lib):
    """The shape and null checks come before the device is touched: a context handle that is never dereferenced suffices."""
    m = np.zeros((1, 4, 4)); fr = np.zeros((1, 4)); kd = np.zeros(1); r2 = np.zeros(1); out = np.full((1, 4, 4), 7.0)
    st = np.zeros(1, dtype=np.int32)
    args = [m.ctypes.data, fr.ctypes.data, kd.ctypes.data, r2.ctypes.data, out.ctypes.data, st.ctypes.data]
    fake = C.c_void_p(m.ctypes.data)
    assert lib.aln_transform_matrices_device(fake, 0, 4, 4, *([None] * 6)) == _ffi.OK
    for hole in range(6):
        a = list(args)
        a[hole] = None
        assert lib.aln_transform_matrices_device(fake, 1, 4, 4, *a) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices_device(fake, 1, 0, 4, *args) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices_device(fake, 1, 4, 0, *args) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_transform_matrices_device(fake, 1, 32, 33, *args) == _ffi.ERR_INVALID_ARGUMENT      # 1056 entries > 1024
    assert lib.aln_transform_matrices_device(fake, 1, 65536, 65536, *args) == _ffi.ERR_INVALID_ARGUMENT    # the product in 64 bits
    assert (out == 7.0).all()
