"""The resident sequence set on the GPU (aln_seqset_*): every pair of a block against aln_align_batch on the listed pairs (bit for bit)
and against the CPU oracle, chunked against unchunked, one-by-many and many-by-one blocks, the held hits (list, strings, thresholds),
per-pair failures, refused calls that must leave their outputs alone, held state, and other calls on the same context in between.

One set of 12 protein sequences serves every test: lengths 0, 1, 2, 7, 63, 64, 65, 130, 512, 513, 600 (empty, single cells, the 64-lane
strip boundary, one strip against two) and one sequence that holds a code outside the matrix.  The batch's and the oracle's answers
are computed once per scheme and shared."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from aligner_amd import _ffi, runtime
from aligner_amd.batch import RESULT_DTYPE, PairBatch, align_batch
from aligner_amd.seqset import SeqSet, rectangle, upper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 2, 7, 63, 64, 65, 130, 512, 513, 600]
FIELDS = ["f", "score", "end_y", "end_x", "start_y", "start_x", "aln_len", "status"]      # (passes / flags: route diagnostics)


def make_set():
    """11 random proteins of LENGTHS + one with a code outside a 24 x 24 matrix.  The long ones share mutated segments, so that f
    varies; the 1-residue sequence and the 2-residue sequence score below zero against each other (no positive cell under local)."""
    from aligner_amd.matrices import get_blosum62
    m = get_blosum62()
    rng = np.random.default_rng(20261017)
    anc = rng.integers(0, 20, 700).astype(np.uint8)
    seqs = []
    for n in LENGTHS:
        s = rng.integers(0, 20, n).astype(np.uint8)
        if n >= 63:
            a = int(rng.integers(0, 700 - n + 1))
            piece = anc[a:a + n].copy()
            mut = rng.random(n) < 0.35
            piece[mut] = rng.integers(0, 20, int(mut.sum()))
            keep = rng.random(n) < 0.7
            s[keep] = piece[keep]
        seqs.append(s)
    a = 0
    worst = [b for b in range(20) if m[b, a] < 0 and m[a, b] < 0]
    seqs[1] = np.array([a], dtype=np.uint8)
    seqs[2] = np.array(worst[:2], dtype=np.uint8)
    bad = rng.integers(0, 20, 40).astype(np.uint8)
    bad[17] = 24
    seqs.append(bad)
    return seqs


def schemes():
    from aligner_amd.matrices import get_blosum62
    m = get_blosum62()
    return {
        "core_local_11_2": (_ffi.CORE_LOCAL, m, 11.0, 2.0, {}),            # the row-1 hazard route
        "core_global_4_4": (_ffi.CORE_GLOBAL, m, 4.0, 4.0, {}),
        "legacy_local": (_ffi.LEGACY_LOCAL, m, 11.0, 11.0, {}),
        "real_valued": (_ffi.CORE_LOCAL, m * 0.37 + 0.013, 11.3, 2.1, {}),   # not dyadic: the f64 route
    }


SCHEMES = list(schemes())
RECT = (3, 7, 5, 7)          # queries 3 .. 9, targets 5 .. 11: overlapping ranges that do not start at 0


def upper_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def rect_pairs(qf, qc, tf, tc):
    return [(qf + a, tf + b) for a in range(qc) for b in range(tc)]


_cache = {}


def reference(name, orc):
    """Per scheme, once: aln_align_batch (with strings) over the listed pairs of the upper block and of RECT, and the oracle's f /
    status per (q, t)."""
    if name in _cache:
        return _cache[name]
    sem, m, d, e, kw = schemes()[name]
    seqs = make_set()
    ref = {"oracle": {}}
    for key, pairs in (("upper", upper_pairs(len(seqs))), ("rect", rect_pairs(*RECT))):
        b = PairBatch.from_pairs((seqs[q], seqs[t]) for q, t in pairs)
        ref[key] = (pairs, b, align_batch(b, sem, d, e, m, **kw))
        for q, t in pairs:
            if (q, t) not in ref["oracle"]:
                o = orc.align(sem, seqs[q], seqs[t], d, e, m)
                ref["oracle"][(q, t)] = (o["status"], o["f"])
    _cache[name] = ref
    return ref


@pytest.fixture(scope="module")
def sset():
    with SeqSet(make_set()) as s:
        yield s


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def check_scores(ref, key, f, status):
    pairs, _, want = ref[key]
    assert len(f) == len(pairs) == len(status)
    assert (status == want.results["status"]).all(), (status, want.results["status"])
    assert (bits(f) == bits(want.results["f"])).all()
    for k, (q, t) in enumerate(pairs):
        o_status, o_f = ref["oracle"][(q, t)]
        assert status[k] == o_status, (q, t)
        if o_status == 0:
            assert f[k] == o_f, (q, t)


@pytest.mark.parametrize("name", SCHEMES)
def test_score_equals_batch_and_oracle(sset, orc, name):
    sem, m, d, e, kw = schemes()[name]
    ref = reference(name, orc)
    n = len(sset)
    assert sset.pairs(upper(0, n)) == n * (n - 1) // 2 == 66 and sset.pairs(rectangle(*RECT)) == 49
    f, status = sset.score(m, d, e, upper(0, n), semantics=sem, **kw)
    check_scores(ref, "upper", f, status)
    assert (status != 0).sum() >= 21 and (status == 0).sum() >= 40          # the empty and the out-of-range sequence fail their pairs
    f, status = sset.score(m, d, e, rectangle(*RECT), semantics=sem, **kw)
    check_scores(ref, "rect", f, status)
    st = sset.stats()
    assert st["bytes_down"] >= 12 * 49 and st["fill_ms"] > 0


def digest(sset):
    h = hashlib.sha256()
    for name in SCHEMES:
        sem, m, d, e, kw = schemes()[name]
        for blk in (upper(0, len(sset)), rectangle(*RECT)):
            f, status = sset.score(m, d, e, blk, semantics=sem, **kw)
            h.update(f.tobytes()); h.update(status.tobytes())
            held = sset.hits(m, d, e, 30.0, blk, semantics=sem, **kw)
            res, strs = held.strings()
            h.update(held.index.tobytes()); h.update(held.f.tobytes())
            for name_ in FIELDS:
                h.update(np.ascontiguousarray(res[name_]).tobytes())
            for qa, ta in strs:
                h.update(qa.tobytes()); h.update(ta.tobytes())
    return h.hexdigest()


CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from aligner_amd import _ffi, runtime
from aligner_amd.batch import PairBatch
from aligner_amd.seqset import SeqSet
import test_seqset_gpu as T
seqs = T.make_set()
b = PairBatch.from_pairs((seqs[q], seqs[t]) for q, t in T.upper_pairs(len(seqs)))
sem, m, d, e, kw = T.schemes()["core_local_11_2"]
p, keep = runtime.make_params(sem, d, e, m)
first, count = np.zeros(128, np.uint64), np.zeros(128, np.uint64)
chunks = _ffi.load().aln_plan_chunks(C.byref(p), b.q_len.ctypes.data, b.t_len.ctypes.data, len(b), 1, first.ctypes.data, count.ctypes.data, 128)
assert chunks >= 3, chunks          # each of the three pairs among the 512, 513 and 600 long sequences exceeds the bound alone; the same bounds cut the set's passes
with SeqSet(seqs) as s:
    print("DIGEST", T.digest(s))
"""


def test_chunked_call_is_byte_identical(sset):
    """ALN_CHUNK_CELLS = 250 000: every pair of two of the three long sequences (262 656 .. 307 800 cells) ends a chunk, alone or behind
    the few short pairs in front of it, so chunks end in the middle of a row; set in a child (the variable is read per call, but the
    other tests must not see it).  Scores, hit lists, summaries and strings of every scheme and both blocks hash alike."""
    env = dict(os.environ, ALN_CHUNK_CELLS="250000")
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "DIGEST" in out.stdout, out.stdout + out.stderr
    assert out.stdout.split("DIGEST")[1].split()[0] == digest(sset)


def test_one_by_many_and_many_by_one(sset, orc):
    """Sequence 7 (130 residues) as the only query, then as the only target: a swapped q / t would give the transposed pair, whose
    coordinates and (real-valued matrix, not symmetric after the test's perturbation) f differ."""
    sem, m, d, e, kw = schemes()["core_local_11_2"]
    rng = np.random.default_rng(3)
    m = m + np.triu(rng.integers(-2, 3, m.shape), 1)              # integral, not symmetric
    seqs = make_set()
    for blk, pairs in ((rectangle(7, 1, 3, 8), [(7, t) for t in range(3, 11)]), (rectangle(3, 8, 7, 1), [(q, 7) for q in range(3, 11)])):
        f, status = sset.score(m, d, e, blk, semantics=sem)
        b = PairBatch.from_pairs((seqs[q], seqs[t]) for q, t in pairs)
        want = align_batch(b, sem, d, e, m, want_traceback=False).results
        assert (status == want["status"]).all() and (bits(f) == bits(want["f"])).all()
        for k, (q, t) in enumerate(pairs):
            o = orc.align(sem, seqs[q], seqs[t], d, e, m)
            assert status[k] == o["status"] == 0 and f[k] == o["f"], (q, t)
        held = sset.hits(m, d, e, -1.0, blk, semantics=sem)
        assert list(zip(held.q.tolist(), held.t.tolist())) == pairs
        res, strs = held.strings()
        for k, (q, t) in enumerate(pairs):
            o = orc.align(sem, seqs[q], seqs[t], d, e, m)
            assert (res["end_y"][k], res["end_x"][k]) == o["end"] and strs[k][0].tobytes() == o["qa"].tobytes() and strs[k][1].tobytes() == o["ta"].tobytes()


def check_held(ref, key, held, which):
    """held entries `which` (positions in the held list) against the batch's summaries and strings of the same pairs"""
    pairs, b, want = ref[key]
    res, strs = held.strings(which)
    for k, pos in enumerate(which):
        i = int(held.index[pos])
        assert (int(held.q[pos]), int(held.t[pos])) == pairs[i]
        for name in FIELDS:
            assert res[name][k].tobytes() == want.results[name][i].tobytes(), (name, pairs[i])
        qa, ta = want.aligned(i)
        assert strs[k][0].tobytes() == qa.tobytes() and strs[k][1].tobytes() == ta.tobytes(), pairs[i]


@pytest.mark.parametrize("name", SCHEMES)
def test_hits_list_and_strings(sset, orc, name):
    sem, m, d, e, kw = schemes()[name]
    ref = reference(name, orc)
    for key, blk in (("upper", upper(0, len(sset))), ("rect", rectangle(*RECT))):
        pairs, b, want = ref[key]
        f, status = want.results["f"], want.results["status"]
        ok_f = np.sort(f[status == 0])
        f_min = float(ok_f[len(ok_f) // 2])                       # keeps the upper half of the pairs that succeeded
        expect = np.nonzero((status == 0) & (f >= f_min))[0]
        assert len(expect) > 0
        if ok_f[0] != ok_f[-1]:                                   # (core global: f is 0.0 for every pair, nothing to split)
            assert len(expect) < (status == 0).sum()
        held = sset.hits(m, d, e, f_min, blk, semantics=sem, **kw)
        assert len(held) == len(expect) and (held.index == expect.astype(np.uint64)).all()
        assert (bits(held.f) == bits(f[expect])).all()
        assert [(int(q), int(t)) for q, t in zip(held.q, held.t)] == [pairs[i] for i in expect]
        n = len(held)
        check_held(ref, key, held, np.arange(n, dtype=np.uint32))
        perm = np.random.default_rng(5).permutation(n)[:max(2, n // 2)].astype(np.uint32)
        check_held(ref, key, held, perm)
        check_held(ref, key, held, np.array([n - 1, 0, n - 1], dtype=np.uint32))        # a position listed twice
        alns = held.alignments([0])
        assert alns[0].f == held.f[0]
        # thresholds at the ends
        assert len(sset.hits(m, d, e, float("inf"), blk, semantics=sem, **kw)) == 0
        assert len(sset.hits(m, d, e, float("nan"), blk, semantics=sem, **kw)) == 0
        everything = sset.hits(m, d, e, float("-inf"), blk, semantics=sem, **kw)
        assert (everything.index == np.nonzero(status == 0)[0].astype(np.uint64)).all()


def test_per_pair_failures(sset, orc):
    sem, m, d, e, kw = schemes()["core_local_11_2"]
    ref = reference("core_local_11_2", orc)
    pairs, b, want = ref["upper"]
    n = len(sset)
    f, status = sset.score(m, d, e, upper(0, n), semantics=sem)
    by = {p: k for k, p in enumerate(pairs)}
    for t in range(1, n):
        assert status[by[(0, t)]] == _ffi.ERR_EMPTY_SEQUENCE                              # the empty sequence
    for q in range(1, n - 1):
        assert status[by[(q, n - 1)]] == _ffi.ERR_CODE_OUT_OF_RANGE                       # the code outside the matrix
    assert status[by[(1, 2)]] == _ffi.ERR_NO_POSITIVE_CELL
    assert (status == want.results["status"]).all()
    ok = status == 0
    assert ok.sum() == 66 - 11 - 10 - 1
    for k in np.nonzero(ok)[0]:                                                           # the neighbours are untouched
        assert f[k] == ref["oracle"][pairs[k]][1]
    # without a status array the first failure is the call's status, and f is written all the same
    lib = _ffi.load()
    p, keep = runtime.make_params(sem, d, e, m)
    blk = upper(0, n)
    f2 = np.full(66, -7.0)
    assert lib.aln_seqset_score(sset.handle, C.byref(p), C.byref(blk), f2.ctypes.data, None) == _ffi.ERR_EMPTY_SEQUENCE
    assert (bits(f2) == bits(f)).all()
    blk = rectangle(3, 4, 8, 4)                                                           # its first failure: (3, 11), out of range
    f3 = np.zeros(16)
    assert lib.aln_seqset_score(sset.handle, C.byref(p), C.byref(blk), f3.ctypes.data, None) == _ffi.ERR_CODE_OUT_OF_RANGE
    blk = rectangle(3, 4, 7, 4)                                                           # no failure
    assert lib.aln_seqset_score(sset.handle, C.byref(p), C.byref(blk), f3.ctypes.data, None) == _ffi.OK


def test_refused_calls_leave_their_outputs(sset):
    sem, m, d, e, kw = schemes()["core_local_11_2"]
    lib = _ffi.load()
    n = len(sset)
    f = np.full(200, 0x5A, dtype=np.uint8).view(np.float64).copy()
    status = np.full(50, 0x5A5A5A5A, dtype=np.int32)
    count = C.c_uint64(0xABCDEF)
    f0, s0 = f.tobytes(), status.tobytes()

    def both(p, blk, want):
        assert lib.aln_seqset_score(sset.handle, C.byref(p), C.byref(blk), f.ctypes.data, status.ctypes.data) == want
        assert lib.aln_seqset_hits(sset.handle, C.byref(p), C.byref(blk), 0.0, C.byref(count)) == want
        assert f.tobytes() == f0 and status.tobytes() == s0 and count.value == 0xABCDEF

    good, keep = runtime.make_params(sem, d, e, m)
    for blk in (_ffi.SeqsetBlock(0, n + 1, 0, n + 1, 1, 0),         # a range past n_seqs
                _ffi.SeqsetBlock(n, 1, 0, 1, 0, 0),
                _ffi.SeqsetBlock(0, 2, 8, n, 0, 0),
                _ffi.SeqsetBlock(0, 4, 1, 4, 1, 0),                 # upper with unequal ranges
                _ffi.SeqsetBlock(0, 4, 0, 5, 1, 0),
                _ffi.SeqsetBlock(0, 4, 0, 4, 0, 1),                 # reserved
                _ffi.SeqsetBlock(0, 0, 0, 4, 0, 0),                 # no pairs
                _ffi.SeqsetBlock(3, 1, 3, 1, 1, 0)):
        assert sset.pairs(blk) == 0
        both(good, blk, _ffi.ERR_INVALID_ARGUMENT)
    null_matrix = _ffi.Params(sem, 0, d, e, None, 24, 24, 24, 0, 98, 0, 0, 0, 0)
    both(null_matrix, upper(0, n), _ffi.ERR_INVALID_ARGUMENT)
    pwm, keep2 = runtime.make_params(_ffi.PWM_LOCAL, d, e, np.ones((4, 30)))
    both(pwm, upper(0, n), _ffi.ERR_UNSUPPORTED)
    blk = upper(0, n)
    assert lib.aln_seqset_score(sset.handle, C.byref(good), C.byref(blk), None, status.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
    assert lib.aln_seqset_hits(sset.handle, C.byref(good), C.byref(blk), 0.0, None) == _ffi.ERR_INVALID_ARGUMENT
    assert status.tobytes() == s0
    # a set of 2^32 sequences is refused before anything is read
    st = C.c_int(-1)
    z = np.zeros(4, dtype=np.uint64)
    assert not lib.aln_seqset_create(runtime.context(), z.ctypes.data, z.ctypes.data, z.ctypes.data, 2 ** 32, C.byref(st))
    assert st.value == _ffi.ERR_INVALID_ARGUMENT


def test_held_state(orc):
    sem, m, d, e, kw = schemes()["core_local_11_2"]
    lib = _ffi.load()
    idx = np.full(4, 0x77, dtype=np.uint64); q = np.full(4, 0x77, dtype=np.uint32); t = q.copy(); f = np.full(4, -3.0)
    res = np.full(4 * 48, 0x77, dtype=np.uint8)
    keep = np.zeros(1, dtype=np.uint32)
    off = np.zeros(1, dtype=np.uint64)
    tb = np.full(4096, 0x77, dtype=np.uint8)

    def untouched():
        return (idx == 0x77).all() and (q == 0x77).all() and (t == 0x77).all() and (f == -3.0).all() and (res == 0x77).all() and (tb == 0x77).all()

    def held_list(s, first, n, null=False):
        return lib.aln_seqset_held_list(s.handle, first, n, None if null else idx.ctypes.data, q.ctypes.data, t.ctypes.data, f.ctypes.data)

    def held_strings(s, n=1):
        return lib.aln_seqset_held_strings(s.handle, keep.ctypes.data, n, res.ctypes.data, tb.ctypes.data, off.ctypes.data)

    with SeqSet(make_set()) as s:
        blk = rectangle(7, 2, 9, 2)
        # before any hits
        assert held_list(s, 0, 0) == _ffi.ERR_INVALID_ARGUMENT and held_list(s, 0, 1) == _ffi.ERR_INVALID_ARGUMENT
        assert held_strings(s) == _ffi.ERR_INVALID_ARGUMENT and untouched()
        held = s.hits(m, d, e, -1.0, blk, semantics=sem)
        assert len(held) == 4
        # beyond the count, null pointers
        assert held_list(s, 0, 5) == _ffi.ERR_INVALID_ARGUMENT and held_list(s, 5, 0) == _ffi.ERR_INVALID_ARGUMENT
        assert held_list(s, 1, 2, null=True) == _ffi.ERR_INVALID_ARGUMENT
        keep[0] = 4
        assert held_strings(s) == _ffi.ERR_INVALID_ARGUMENT
        keep[0] = 0
        assert lib.aln_seqset_held_strings(s.handle, None, 1, res.ctypes.data, tb.ctypes.data, off.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_seqset_held_strings(s.handle, keep.ctypes.data, 1, None, tb.ctypes.data, off.ctypes.data) == _ffi.ERR_INVALID_ARGUMENT
        assert lib.aln_seqset_held_strings(s.handle, keep.ctypes.data, 1, res.ctypes.data, tb.ctypes.data, None) == _ffi.ERR_INVALID_ARGUMENT
        assert untouched()
        # the held calls work, strings are optional
        assert held_list(s, 1, 2) == _ffi.OK and (idx[:2] == [1, 2]).all() and (idx[2:] == 0x77).all()
        assert lib.aln_seqset_held_strings(s.handle, keep.ctypes.data, 1, res.ctypes.data, None, None) == _ffi.OK
        assert res[:48].view(RESULT_DTYPE)["f"][0] == held.f[0] and (tb == 0x77).all()
        # bytes of a string's capacity beyond aln_len are zero, by the one-copy layout and by any other
        for base in (0, 8):
            tb[:] = 0x77; off[0] = base
            assert held_strings(s) == _ffi.OK
            n_aln, cap = int(res[:48].view(RESULT_DTYPE)["aln_len"][0]), int(s.len[7] + s.len[9] + 2)
            assert 0 < n_aln < cap and (tb[base + n_aln:base + cap] == 0).all() and (tb[base + cap + n_aln:base + 2 * cap] == 0).all()
            assert (tb[:base] == 0x77).all() and (tb[base + 2 * cap:] == 0x77).all() and (tb[base:base + n_aln] != 0x77).any()
        tb[:] = 0x77; off[0] = 0; res[:] = 0x77
        assert lib.aln_seqset_held_strings(s.handle, keep.ctypes.data, 1, res.ctypes.data, None, None) == _ffi.OK
        # a refused pass leaves them in place, a later score replaces them
        bad = _ffi.SeqsetBlock(0, 4, 0, 4, 0, 1)
        p, keepalive = runtime.make_params(sem, d, e, m)
        assert lib.aln_seqset_score(s.handle, C.byref(p), C.byref(bad), f.ctypes.data, None) == _ffi.ERR_INVALID_ARGUMENT
        assert held_list(s, 0, 4) == _ffi.OK
        s.score(m, d, e, blk, semantics=sem)
        idx[:] = 0x77; q[:] = 0x77; t[:] = 0x77; f[:] = -3.0; res[:] = 0x77
        assert held_list(s, 0, 1) == _ffi.ERR_INVALID_ARGUMENT and held_strings(s) == _ffi.ERR_INVALID_ARGUMENT and untouched()
        with pytest.raises(ValueError):
            held.strings([0])


def test_neighbours_on_one_context(sset, orc):
    """hits, then a batch call and a window scan on the same context, then hits again: the same list, summaries and strings."""
    sem, m, d, e, kw = schemes()["core_local_11_2"]
    ref = reference("core_local_11_2", orc)
    blk = upper(0, len(sset))

    def snapshot():
        held = sset.hits(m, d, e, 40.0, blk, semantics=sem)
        res, strs = held.strings()
        return (held.index.tobytes(), held.f.tobytes(), [res[n].tobytes() for n in FIELDS], [(a.tobytes(), b.tobytes()) for a, b in strs])

    before = snapshot()
    assert len(before[3]) > 0
    pairs, b, want = ref["upper"]
    again = align_batch(b, sem, d, e, m)
    assert again.results.tobytes() == want.results.tobytes()
    lib = _ffi.load()
    rng = np.random.default_rng(9)
    dna = rng.integers(0, 4, 5000).astype(np.uint8)
    pwm = rng.integers(-3, 6, (4, 40)).astype(np.float64)
    st = C.c_int(0)
    scan = lib.aln_scan_create(runtime.context(), dna.ctypes.data, len(dna), C.byref(st))
    assert scan and st.value == 0
    try:
        g = _ffi.ScanGeometry(0, 25, 100, 0, 0)
        nw = lib.aln_scan_windows(scan, C.byref(g))
        fw = np.zeros(nw)
        p, keep = runtime.make_params(_ffi.PWM_LOCAL, 6.0, 2.0, pwm)
        assert lib.aln_scan_score(scan, C.byref(p), C.byref(g), fw.ctypes.data) == _ffi.OK
        o = orc.align_pwm(dna[:100], 6.0, 2.0, pwm)
        assert fw[0] == o["f"]
    finally:
        lib.aln_scan_destroy(scan)
    assert snapshot() == before
