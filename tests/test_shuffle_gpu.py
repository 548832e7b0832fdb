"""Shuffled copies drawn on the device (aln_shuffle_targets / aln_shuffle_scores) and the p-values on top of them: the copies
byte for byte against the restatement in shuffle_ref.py on both sides of the LDS bound, every score against the oracle on the
restated copies, invariance under pair splits, chunking and seeds, calculate_p_values against the host fit, and the errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shuffle_ref  # noqa: E402
from aligner_amd import _ffi, runtime, statistics  # noqa: E402
from aligner_amd.batch import PairBatch, align_batch  # noqa: E402
from aligner_amd.errors import ReferencePanic  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 2048                     # ALN_SHUFFLE_LDS_MAX (aln_device.h)


def _raw_scores(pairs, sem, del_, ext, S, seed, per_pair, max_trim=6, pair_base=0):
    """aln_shuffle_scores through ctypes: (status of the call, f, lengths, per-pair status)."""
    b = pairs if isinstance(pairs, PairBatch) else PairBatch.from_pairs(pairs)
    n = len(b)
    f = np.zeros((n, per_pair)); L = np.zeros((n, per_pair), dtype=np.uint32); st = np.zeros(n, dtype=np.int32)
    p, _keep = runtime.make_params(sem, del_, ext, S, outputs=_ffi.OUT_SCORE)
    spec = _ffi.ShuffleSpec(seed, pair_base, per_pair, max_trim)
    r = _ffi.load().aln_shuffle_scores(runtime.context(), C.byref(p), C.byref(spec), b.seqs.ctypes.data, b.q_off.ctypes.data,
                                       b.q_len.ctypes.data, b.t_off.ctypes.data, b.t_len.ctypes.data, n, f.ctypes.data, L.ctypes.data,
                                       st.ctypes.data)
    return r, f, L, st


def _oracle_f(orc, sem, del_, ext, S, pairs):
    b = PairBatch.from_pairs(pairs)
    ref, _, _ = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, del_, ext, S, n_threads=16, want_traceback=False)
    return np.array([r.f for r in ref]), np.array([r.status for r in ref])


def _sample(per_pair, k, seed=0):
    if per_pair <= k:
        return list(range(per_pair))
    rng = np.random.default_rng(seed)
    return sorted({0, 1, per_pair - 1} | set(rng.choice(per_pair, k - 3, replace=False).tolist()))


# ---------------------------------------------------------------- the copies
LENGTHS = [6, 7, 64, 350, LDS_MAX - 1, LDS_MAX, LDS_MAX + 1, 10000]


def _check_copies(targets, copies, lengths, seed, per_pair, max_trim, pair_base, k):
    for i, t in enumerate(targets):
        assert copies[i].shape == (per_pair, len(t))
        assert lengths[i].tolist() == (len(t) - shuffle_ref.trims(seed, pair_base + i, per_pair, max_trim)).tolist()
        for s in _sample(per_pair, k, seed=i):
            trim, want = shuffle_ref.copy_of(t, seed, pair_base + i, s, max_trim)
            row = copies[i][s]
            assert (row[:len(want)] == want).all(), (len(t), s)
            assert (row[len(want):] == 0).all(), (len(t), s)


def test_copies_every_length_one_call():
    """All lengths in one call (the LDS slot is 2048 bytes: 2049 and 10 000 shuffle in place in global memory), 4 999 copies each."""
    rng = np.random.default_rng(5)
    targets = [rng.integers(0, 24, L).astype(np.uint8) for L in LENGTHS]
    copies, lengths = statistics.shuffle_targets(targets, seed=77, per_pair=4999, max_trim=6)
    _check_copies(targets, copies, lengths, 77, 4999, 6, 0, 24)
    # every copy of the short targets, and the shuffle permutes: no 350-residue copy is its trimmed prefix
    _check_copies(targets[:3], copies[:3], lengths[:3], 77, 4999, 6, 0, 4999)
    assert not any((copies[3][s][:lengths[3][s]] == targets[3][:lengths[3][s]]).all() for s in range(4999))


@pytest.mark.parametrize("L", LENGTHS)
def test_copies_one_length_per_call(L):
    """One target per call: the LDS slot is that target's length (its neighbours 2047 / 2048 / 2049 decide LDS or global)."""
    t = np.random.default_rng(L).integers(0, 24, L).astype(np.uint8)
    per_pair = 300 if L > 400 else 4999
    copies, lengths = statistics.shuffle_targets([t], seed=3, per_pair=per_pair, max_trim=6, pair_base=41)
    _check_copies([t], copies, lengths, 3, per_pair, 6, 41, 32)


# ---------------------------------------------------------------- the scores
def _schemes(S):
    real = S * 1.1 + 0.013             # not a multiple of 2^-k for any k <= 8: the f64 kernels
    return {"core_local_11_2": (_ffi.CORE_LOCAL, 11, 2, S),
            "del_eq_ext": (_ffi.CORE_LOCAL, 4, 4, S),
            "core_global": (_ffi.CORE_GLOBAL, 11, 2, S),
            "real_f64": (_ffi.CORE_LOCAL, 10.7, 1.3, real)}


def _batch(kind):
    rng = np.random.default_rng(17)
    if kind == "one":
        q = rng.integers(0, 20, 180).astype(np.uint8)
        t = np.concatenate([q[20:150], rng.integers(0, 20, 60).astype(np.uint8)])
        return [(q, t)], 4999, 4999
    pairs = []
    for i in range(64):
        if i in (5, 40):              # long pairs: several strips, shared between waves
            nq, nt = 900, 1400
        else:
            nq, nt = rng.integers(20, 400, 2)
        q = rng.integers(0, 20, nq).astype(np.uint8)
        t = rng.integers(0, 20, nt).astype(np.uint8)
        if i % 3 == 0:
            t[: min(nq, nt) // 2] = q[: min(nq, nt) // 2]
        pairs.append((q, t))
    return pairs, 257, 12


@pytest.mark.parametrize("kind", ["one", "mixed"])
@pytest.mark.parametrize("scheme", ["core_local_11_2", "del_eq_ext", "core_global", "real_f64"])
def test_scores_equal_oracle_on_restated_copies(orc, blosum62, kind, scheme):
    sem, d, e, S = _schemes(blosum62)[scheme]
    pairs, per_pair, k = _batch(kind)
    seed = 0xC0FFEE
    r, f, L, st = _raw_scores(pairs, sem, d, e, S, seed, per_pair)
    assert r == 0 and (st == 0).all()
    todo, where = [], []
    for i, (q, t) in enumerate(pairs):
        assert L[i].tolist() == (len(t) - shuffle_ref.trims(seed, i, per_pair, 6)).tolist()
        for s in _sample(per_pair, k, seed=i):
            todo.append((q, shuffle_ref.copy_of(t, seed, i, s, 6)[1]))
            where.append((i, s))
    want, wst = _oracle_f(orc, sem, d, e, S, todo)
    assert (wst == 0).all()
    got = np.array([f[i, s] for i, s in where])
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(where[j], got[j], want[j]) for j in bad[:5]]


def test_copies_routed_elsewhere_upload_the_plans_queue(orc, blosum62):
    """Two copies of a 1000 x 5000 pair take the single-pair route beside a short pair's copies in the batch kernel: the plan's
    own queue goes up over the identity.  The same copies through aln_align_batch show the route (flags bit 1)."""
    rng = np.random.default_rng(8)
    q1 = rng.integers(0, 20, 1000).astype(np.uint8)
    t1 = np.concatenate([q1[100:900], rng.integers(0, 20, 4200).astype(np.uint8)])
    q2, t2 = rng.integers(0, 20, 100).astype(np.uint8), rng.integers(0, 20, 120).astype(np.uint8)
    pairs = [(q2, t2), (q1, t1)]
    seed = 12
    r, f, L, st = _raw_scores(pairs, _ffi.CORE_LOCAL, 11, 2, blosum62, seed, 2)
    assert r == 0 and (st == 0).all()
    todo = [(q, shuffle_ref.copy_of(t, seed, i, s, 6)[1]) for i, (q, t) in enumerate(pairs) for s in range(2)]
    want, _ = _oracle_f(orc, _ffi.CORE_LOCAL, 11, 2, blosum62, todo)
    assert f.ravel().tolist() == want.tolist()
    same = align_batch(PairBatch.from_pairs(todo), _ffi.CORE_LOCAL, 11, 2, blosum62, want_traceback=False)
    assert same.results["f"].tolist() == want.tolist()
    assert [bool(x & _ffi.FLAG_SINGLE) for x in same.results["flags"]] == [False, False, True, True]


# ---------------------------------------------------------------- invariance
def _sixteen():
    rng = np.random.default_rng(23)
    return [(rng.integers(0, 20, rng.integers(50, 300)).astype(np.uint8), rng.integers(0, 20, rng.integers(50, 300)).astype(np.uint8))
            for _ in range(16)]


def test_one_call_equals_one_pair_calls(blosum62):
    pairs = _sixteen()
    r, f, L, st = _raw_scores(pairs, _ffi.CORE_LOCAL, 11, 2, blosum62, 99, 300)
    assert r == 0
    for i in range(16):
        r1, f1, L1, _ = _raw_scores([pairs[i]], _ffi.CORE_LOCAL, 11, 2, blosum62, 99, 300, pair_base=i)
        assert r1 == 0
        assert f1[0].tobytes() == f[i].tobytes() and (L1[0] == L[i]).all(), i


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from aligner_amd import statistics
from aligner_amd.matrices import get_blosum62
from test_shuffle_gpu import _sixteen
f, L, st = statistics.device_shuffled_scores(_sixteen(), 11, 2, get_blosum62(), seed=99, per_pair=300)
np.save(sys.argv[1], f)
"""


def test_small_chunks_give_the_same_bytes(tmp_path, blosum62):
    """ALN_CHUNK_CELLS = 4e6 cuts the 16 pairs (1-9e6 cells each) into many chunks of whole pairs; the scores are the same bytes."""
    f, _, _ = statistics.device_shuffled_scores(_sixteen(), 11, 2, blosum62, seed=99, per_pair=300)
    out = str(tmp_path / "f.npy")
    env = dict(os.environ, ALN_CHUNK_CELLS="4e6")
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.dirname(os.path.abspath(__file__))), out], env=env, check=True,
                   timeout=300)
    assert np.load(out).tobytes() == f.tobytes()


def test_seed_decides_the_copies(blosum62):
    pairs = _sixteen()[:4]
    a = statistics.device_shuffled_scores(pairs, 11, 2, blosum62, seed=5, per_pair=500)
    b = statistics.device_shuffled_scores(pairs, 11, 2, blosum62, seed=5, per_pair=500)
    c = statistics.device_shuffled_scores(pairs, 11, 2, blosum62, seed=6, per_pair=500)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all()
    assert a[0].tobytes() != c[0].tobytes() and (a[1] != c[1]).any()
    ta = statistics.shuffle_targets([t for _, t in pairs], seed=5, per_pair=50)[0]
    tc = statistics.shuffle_targets([t for _, t in pairs], seed=6, per_pair=50)[0]
    assert all((x != y).any() for x, y in zip(ta, tc))


# ---------------------------------------------------------------- p-values
def test_p_values_equal_host_fit_on_restated_copies(orc, blosum62):
    rng = np.random.default_rng(2024)
    q = rng.integers(0, 20, 180).astype(np.uint8)
    t = np.concatenate([q[20:150], rng.integers(0, 20, 60).astype(np.uint8)])       # test_p_value_batch_driver's homolog
    r2 = np.random.default_rng(31)
    pairs = [(q, t), (r2.integers(0, 20, 150).astype(np.uint8), r2.integers(0, 20, 170).astype(np.uint8))]
    seed = 4321
    got = statistics.calculate_p_values(pairs, 11, 2, blosum62, seed=seed)
    for i, (qq, tt) in enumerate(pairs):
        init = orc.align(orc.CORE_LOCAL, qq, tt, 11, 2, blosum62)["f"]
        copies = [shuffle_ref.copy_of(tt, seed, i, s, 6)[1] for s in range(4999)]
        f, _ = _oracle_f(orc, _ffi.CORE_LOCAL, 11, 2, blosum62, [(qq, c) for c in copies])
        scores = np.concatenate([[init], f])
        lengths = np.concatenate([[len(tt)], [len(c) for c in copies]])
        want = statistics.calculate_distribution_params(len(qq), lengths, scores).get_p_value(len(qq), len(tt), init)
        np.testing.assert_array_equal(got[i], want)
    assert 0.0 <= got[0] < 0.05          # a 130-residue exact match is not a chance hit
    # given initial scores are used as they are
    init = np.array([orc.align(orc.CORE_LOCAL, qq, tt, 11, 2, blosum62)["f"] for qq, tt in pairs])
    np.testing.assert_array_equal(statistics.calculate_p_values(pairs, 11, 2, blosum62, initial_scores=init, seed=seed), got)


# ---------------------------------------------------------------- errors
def test_errors(orc, blosum62):
    rng = np.random.default_rng(1)
    pairs = [(rng.integers(0, 20, 80).astype(np.uint8), rng.integers(0, 20, 90).astype(np.uint8)) for _ in range(3)]
    pwm = rng.integers(-2, 3, (4, 30)).astype(np.float64)
    assert _raw_scores(pairs, _ffi.PWM_LOCAL, 5, 5, pwm, 1, 10)[0] == _ffi.ERR_UNSUPPORTED
    short = pairs + [(pairs[0][0], np.array([1, 2, 3, 4, 5], dtype=np.uint8))]
    assert _raw_scores(short, _ffi.CORE_LOCAL, 11, 2, blosum62, 1, 10)[0] == _ffi.ERR_INVALID_ARGUMENT
    assert _raw_scores(short, _ffi.CORE_LOCAL, 11, 2, blosum62, 1, 10, max_trim=5)[0] == 0
    assert _raw_scores(pairs, _ffi.CORE_LOCAL, 11, 2, blosum62, 1, 0)[0] == _ffi.ERR_INVALID_ARGUMENT
    # a code outside the 24 x 24 matrix in pair 1's target flags pair 1 only; an empty query is the reference's panic
    bad = [pairs[0], (pairs[1][0], np.concatenate([pairs[1][1][:40], [30], pairs[1][1][40:]]).astype(np.uint8)), pairs[2],
           (np.zeros(0, dtype=np.uint8), pairs[2][1])]
    r, f, L, st = _raw_scores(bad, _ffi.CORE_LOCAL, 11, 2, blosum62, 1, 64)
    assert r == 0
    assert st.tolist() == [0, _ffi.ERR_CODE_OUT_OF_RANGE, 0, _ffi.ERR_EMPTY_SEQUENCE]
    for i in (0, 2):
        want, _ = _oracle_f(orc, _ffi.CORE_LOCAL, 11, 2, blosum62, [(bad[i][0], shuffle_ref.copy_of(bad[i][1], 1, i, s, 6)[1]) for s in range(64)])
        assert f[i].tolist() == want.tolist()
    with pytest.raises(ReferencePanic) as e:
        statistics.device_shuffled_scores(bad, 11, 2, blosum62, seed=1, per_pair=64)
    assert e.value.status == _ffi.ERR_CODE_OUT_OF_RANGE
    _, _, st2 = statistics.device_shuffled_scores(bad, 11, 2, blosum62, seed=1, per_pair=64, check=False)
    assert st2.tolist() == st.tolist()
