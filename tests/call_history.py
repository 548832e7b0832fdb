"""Helpers of the call-history tests (tests/test_call_history_*.py).  Not a test module (no test_ prefix).

* A fixed, seeded catalogue of small calls, one per user of a pool slot (catalogue()): each entry knows its inputs, the
  environment knobs of its call, how to run itself on the GPU (run), how to get the same answer from the CPU oracle (expected)
  and which kernels must have served it (route, from the flags word).
* schedule(k): a deterministic order of calls in which every ordered pair of entries (a directly followed by b, a = b included)
  occurs exactly once -- an Eulerian circuit of the complete directed graph with loops, k * k + 1 calls.
* The comparison rule of all call-history tests (compare): every field of aln_pair_result except `passes`, both strings up to
  aln_len, D and H where the call asks for them.  Keys that start with "_" are not compared (flags, passes, raw buffers).
* The batches of the tag-wrap tests: three residue sets of identical shapes (wrap_batches) and the 22 000-pair batch that makes
  every one of four fill waves run more than 4 096 multi-strip passes in one launch (pass_batch).
"""
import ctypes as C
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from aligner_amd import _ffi, runtime  # noqa: E402
from aligner_amd.batch import PairBatch, align_batch  # noqa: E402
from aligner_amd.matrices import get_blosum62, nucleotide_matrix  # noqa: E402

FIELDS = ("status", "score", "f", "end_y", "end_x", "start_y", "start_x", "aln_len")
ORC_DTYPE = np.dtype([("f", "<f8"), ("score", "<f8"), ("end_y", "<u4"), ("end_x", "<u4"), ("start_y", "<u4"), ("start_x", "<u4"),
                      ("coords", "<u8", (4,)), ("aln_len", "<u4"), ("status", "<i4")])
assert ORC_DTYPE.itemsize == 72
STRIP_ROWS = 512                    # ALN_STRIP_ROWS (aln_device.h): rows of one strip of the fast batch kernels
CUS = 256                           # compute units of an MI355X: the read-pair entry needs more pairs than 12 per CU
POOL_SLOTS = 4                      # ALN_POOL_SLOTS


# ---------------------------------------------------------------- the schedule
def schedule(k):
    """k * k + 1 entry numbers: an Eulerian circuit of the complete directed graph with loops on k nodes (Hierholzer, the edges
    of every node taken in a fixed rotated order, so that the walk does not run through the catalogue in order)."""
    stride = next(s for s in (5, 7, 3, 1) if np.gcd(s, k) == 1)
    nxt = [[(a + 1 + stride * j) % k for j in range(k)] for a in range(k)]
    for a in range(k):
        assert sorted(nxt[a]) == list(range(k))
    pos = [0] * k
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if pos[a] < k:
            stack.append(nxt[a][pos[a]])
            pos[a] += 1
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return circuit


def transitions(seq):
    return set(zip(seq[:-1], seq[1:]))


# ---------------------------------------------------------------- the comparison rule
def compare(got, want):
    """None when `got` equals `want` in every key of `want` that does not start with "_", else a short description of the first
    difference.  Strings are taken out of the raw buffer got["_tb"] at want["_idx"] once the lengths agree."""
    got = dict(got)
    for key in want:
        if key.startswith("_") or key == "strings":
            continue
        if key not in got:
            return "%s missing" % key
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (key, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(np.atleast_1d(g != w))[0]
            return "%s differs first at %s: got %s, want %s" % (key, bad.tolist(), np.atleast_1d(g)[tuple(bad)], np.atleast_1d(w)[tuple(bad)])
    if "strings" in want:
        if "_idx" in want and "_tb" in got:
            s = np.asarray(got["_tb"])[want["_idx"]]
        elif "strings" in got:
            s = np.asarray(got["strings"])
        else:
            return "strings missing"
        w = np.asarray(want["strings"])
        if s.shape != w.shape or not np.array_equal(s, w):
            bad = int(np.argmax(s != w)) if s.shape == w.shape else -1
            return "strings differ first at byte %d of %d" % (bad, len(w))
    return None


def string_index(q_len, t_len, aln_len):
    """Positions, in the documented cumulative layout of aln_align_batch's tb_buf, of both aligned strings of every pair up to
    its aln_len."""
    cap = q_len.astype(np.int64) + t_len.astype(np.int64) + 2
    off = np.concatenate([[0], np.cumsum(2 * cap)[:-1]])
    parts = []
    for o, c, L in zip(off, cap, aln_len.astype(np.int64)):
        parts.append(np.arange(o, o + L))
        parts.append(np.arange(o + c, o + c + L))
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def batch_expected(orc, b, sem, dele, ext, S, threads=8):
    ref, tb, tb_off = orc.align_batch(sem, b.seqs, b.q_off, b.q_len, b.t_off, b.t_len, dele, ext, S, n_threads=threads)
    r = np.frombuffer(ref, dtype=ORC_DTYPE)
    want = {f: r[f].copy() for f in FIELDS}
    assert (want["status"] == 0).all(), "the catalogue holds valid pairs only"
    want["_idx"] = string_index(b.q_len, b.t_len, want["aln_len"])
    want["strings"] = tb[want["_idx"]]
    return want


def batch_got(res):
    got = {f: res.results[f] for f in FIELDS}
    got["_flags"], got["_passes"], got["_tb"] = res.results["flags"], res.results["passes"], res.tb
    return got


def pair_expected(orc, sem, q, t, dele, ext, S, want_d, want_h):
    ref = orc.align(sem, q, t, dele, ext, S, want_matrices=want_d or want_h)
    assert ref["status"] == 0
    want = dict(status=ref["status"], score=ref["score"], f=ref["f"], end_y=ref["end"][0], end_x=ref["end"][1],
                start_y=ref["start"][0], start_x=ref["start"][1], aln_len=len(ref["qa"]), strings=np.concatenate([ref["qa"], ref["ta"]]))
    if want_d:
        want["D"] = ref["D"]
    if want_h:
        want["H"] = ref["H"]
    return {k: np.asarray(v) for k, v in want.items()}


def pair_got(sem, q, t, dele, ext, S, want_d, want_h, **kw):
    res, qa, ta, D, H = runtime.align_pair(sem, q, t, dele, ext, S, want_directions=want_d, want_h=want_h, **kw)
    got = {f: np.asarray(getattr(res, f)) for f in FIELDS}
    got["strings"] = np.concatenate([qa, ta])
    got["_flags"], got["_passes"] = np.asarray([res.flags]), np.asarray([res.passes])
    if want_d:
        got["D"] = D
    if want_h:
        got["H"] = H
    return got


# ---------------------------------------------------------------- inputs
def _related_pair(rng, n, m, A=20, plant=True):
    q = rng.integers(0, A, n).astype(np.uint8)
    t = rng.integers(0, A, m).astype(np.uint8)
    if plant:
        L = min(n, m) // 2
        a, b = int(rng.integers(0, n - L + 1)), int(rng.integers(0, m - L + 1))
        run = q[a:a + L].copy()
        mut = rng.random(L) < 0.08
        run[mut] = rng.integers(0, A, int(mut.sum()))
        t[b:b + L] = run
    return q, t


def _pairs(seed, shapes, A=20):
    rng = np.random.default_rng(seed)
    return PairBatch.from_pairs([_related_pair(rng, n, m, A, plant=(i % 3 != 2)) for i, (n, m) in enumerate(shapes)])


def _shapes(seed, count, n_range, m_range):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(*n_range)), int(rng.integers(*m_range))) for _ in range(count)]


def _is(flag):
    return lambda got: bool((got["_flags"] & flag).all())


def _not(flag):
    return lambda got: not bool((got["_flags"] & flag).any())


class Entry:
    """One call of the catalogue.  env: the knobs of this call (read with getenv per call by the library)."""

    def __init__(self, name, run, expected, route, env=None, shape=None):
        self.name, self.run, self.expected, self.route, self.env, self.shape = name, run, expected, route, dict(env or {}), dict(shape or {})

    def routed(self, got):
        return all(check(got) for check in self.route)


def _batch_entry(name, b, sem, dele, ext, S, route, env=None, **kw):
    shape = dict(kind="batch", q_len=b.q_len, t_len=b.t_len, semantics=sem, dele=dele, ext=ext, cells=b.cells)
    return Entry(name, lambda: batch_got(align_batch(b, sem, dele, ext, S, **kw)),
                 lambda orc: batch_expected(orc, b, sem, dele, ext, S), route, env, shape)


def _pair_entry(name, q, t, sem, dele, ext, S, route, want_d=False, want_h=False, env=None, **kw):
    shape = dict(kind="pair", N=len(q), M=len(t), semantics=sem, dele=dele, ext=ext)
    return Entry(name, lambda: pair_got(sem, q, t, dele, ext, S, want_d, want_h, **kw),
                 lambda orc: pair_expected(orc, sem, q, t, dele, ext, S, want_d, want_h), route, env, shape)


def _pwm_entry(name, seed, pwm, dele, ext, n_win, width, route):
    from aligner_amd.pwm import align_windows
    rng = np.random.default_rng(seed)
    W = pwm.shape[1]
    chrom = rng.integers(0, 4, 40 * n_win + width).astype(np.uint8)
    motif = np.argmax(pwm, axis=0).astype(np.uint8)
    for p in range(100, len(chrom) - W, 997):                        # windows with a long path and windows with none
        chrom[p:p + W] = np.where(rng.random(W) < 0.1, rng.integers(0, 4, W), motif)
    wins = [chrom[i * 40:i * 40 + width] for i in range(n_win)]

    def run():
        res, alns = align_windows(wins, dele, ext, pwm)
        got = {f: res[f] for f in FIELDS}
        got["numbered"] = np.concatenate([a.numbered for a in alns])
        got["strings"] = np.concatenate([a.query for a in alns])
        got["_flags"], got["_passes"] = res["flags"], res["passes"]
        return got

    def expected(orc):
        refs = [orc.align_pwm(w, dele, ext, pwm) for w in wins]
        assert all(r["status"] == 0 for r in refs)
        want = dict(status=[r["status"] for r in refs], score=[r["score"] for r in refs], f=[r["f"] for r in refs],
                    end_y=[r["end"][0] for r in refs], end_x=[r["end"][1] for r in refs], start_y=[r["start"][0] for r in refs],
                    start_x=[r["start"][1] for r in refs], aln_len=[len(r["numbered"]) for r in refs])
        want = {k: np.asarray(v) for k, v in want.items()}
        want["numbered"] = np.concatenate([r["numbered"] for r in refs])
        want["strings"] = np.concatenate([r["qal"] for r in refs])
        return want

    return Entry(name, run, expected, route, shape=dict(kind="pwm", windows=n_win, width=width, W=W))


def _shuffle_entry(name, seed):
    import shuffle_ref
    rng = np.random.default_rng(seed)
    pairs = [_related_pair(rng, n, m) for n, m in ((90, 70), (60, 110), (120, 100))]
    b = PairBatch.from_pairs(pairs)
    S, per_pair, max_trim, sseed = get_blosum62(), 200, 6, 0xC0FFEE

    def run():
        n = len(b)
        f = np.zeros((n, per_pair)); L = np.zeros((n, per_pair), dtype=np.uint32); st = np.zeros(n, dtype=np.int32)
        p, _keep = runtime.make_params(_ffi.CORE_LOCAL, 11, 2, S, outputs=_ffi.OUT_SCORE)
        spec = _ffi.ShuffleSpec(sseed, 0, per_pair, max_trim)
        r = _ffi.load().aln_shuffle_scores(runtime.context(), C.byref(p), C.byref(spec), b.seqs.ctypes.data, b.q_off.ctypes.data,
                                           b.q_len.ctypes.data, b.t_off.ctypes.data, b.t_len.ctypes.data, n, f.ctypes.data,
                                           L.ctypes.data, st.ctypes.data)
        return dict(call_status=np.asarray(r), f=f, lengths=L, status=st)

    def expected(orc):
        todo = []
        for i, (q, t) in enumerate(pairs):
            for s in range(per_pair):
                todo.append((q, shuffle_ref.copy_of(t, sseed, i, s, max_trim)[1]))
        tb = PairBatch.from_pairs(todo)
        ref, _, _ = orc.align_batch(_ffi.CORE_LOCAL, tb.seqs, tb.q_off, tb.q_len, tb.t_off, tb.t_len, 11, 2, S, n_threads=8, want_traceback=False)
        r = np.frombuffer(ref, dtype=ORC_DTYPE)
        assert (r["status"] == 0).all()
        return dict(call_status=np.asarray(0), f=r["f"].reshape(len(pairs), per_pair).copy(),
                    lengths=tb.t_len.astype(np.uint32).reshape(len(pairs), per_pair), status=np.zeros(len(pairs), np.int32))

    return Entry(name, run, expected, [], shape=dict(kind="shuffle", pairs=len(pairs), per_pair=per_pair))


_scan = threading.local()           # .scan: the calling thread's scan (one handle is one thread's: tests/concurrent_cases.py)


def close_scan():
    """destroys the calling thread's scan of scan_hits_held_list, if it has one"""
    scan = _scan.__dict__.pop("scan", None)
    if scan is not None:
        scan.close()


def _scan_entry(name, seed):
    from aligner_amd.repeats import HeldGpuScan
    from repeats_oracle_backend import OracleScan
    rng = np.random.default_rng(seed)
    n, W, width, step = 20000, 60, 66, 33
    seq = rng.integers(0, 4, n).astype(np.uint8)
    motif = rng.integers(0, 4, W).astype(np.uint8)
    for p in range(300, n - W, 1500):
        seq[p:p + W] = np.where(rng.random(W) < 0.1, rng.integers(0, 4, W), motif)
    pwm = -np.ones((4, W))
    pwm[motif, np.arange(W)] = 2.0
    mean, sd, z_min = 10.0, 4.0, 5.0                                 # hits: f >= 30

    def run():
        if not hasattr(_scan, "scan"):                               # one scan per thread: its private slot is reused as well
            _scan.scan = HeldGpuScan(seq)
        h = _scan.scan.hits(pwm, 3, 1, 0, step, width, mean, sd, z_min)
        alns = h.alignments(np.arange(len(h)))
        return dict(idx=h.idx, f=h.f, numbered=np.concatenate([a.numbered for a in alns] + [np.zeros(0, np.uint32)]),
                    strings=np.concatenate([a.query for a in alns] + [np.zeros(0, np.uint8)]),
                    coords=np.asarray([a.coords for a in alns], dtype=np.int64).reshape(-1, 4))

    def expected(orc):
        idx, alns = OracleScan(seq).select(pwm, 3, 1, 0, step, width, mean, sd, z_min)
        assert len(idx) >= 5
        return dict(idx=idx, f=np.asarray([a.f for a in alns]), numbered=np.concatenate([a.numbered for a in alns]),
                    strings=np.concatenate([a.query for a in alns]),
                    coords=np.asarray([a.coords for a in alns], dtype=np.int64).reshape(-1, 4))

    return Entry(name, run, expected, [], shape=dict(kind="scan", length=n, W=W))


_catalogue = []


def catalogue():
    """The entries, in a fixed order (built once per process)."""
    if _catalogue:
        return _catalogue
    B62, NUC = get_blosum62(), nucleotide_matrix()
    CL, CG, LL = _ffi.CORE_LOCAL, _ffi.CORE_GLOBAL, _ffi.LEGACY_LOCAL
    fast_batch = [_is(_ffi.FLAG_FAST), _not(_ffi.FLAG_SINGLE)]
    e = []
    # more than 16 pairs: a chunk of 16 or fewer sends pairs of 2^18 cells and more to the single-pair route
    e.append(_batch_entry("fast_local_long", _pairs(1, [(3000, 700)] + _shapes(1, 19, (150, 900), (513, 1300))), CL, 11, 2, B62, fast_batch))
    e.append(_batch_entry("fast_local_short", _pairs(2, _shapes(2, 20, (40, 301), (40, 301))), CL, 11, 2, B62, fast_batch))
    e.append(_batch_entry("fast_global", _pairs(3, _shapes(3, 20, (100, 800), (513, 1200))), CG, 11, 2, B62, fast_batch))
    e.append(_batch_entry("read_pairs_duo", _pairs(4, _shapes(4, 12 * CUS + 130, (40, 150), (40, 120)), A=4), CG, 10, 1, NUC, fast_batch))
    e.append(_batch_entry("claim_runs", _pairs(5, _shapes(5, 701, (20, 221), (20, 221)), A=4), CG, 10, 1, NUC, fast_batch, env={"ALN_CLAIM": "3"}))
    e.append(_batch_entry("legacy_local_batch", _pairs(6, _shapes(6, 40, (20, 400), (20, 400))), LL, 4, 4, B62, [_is(_ffi.FLAG_INTEGER), _not(_ffi.FLAG_SINGLE)]))
    rng = np.random.default_rng(7)
    q, t = _related_pair(rng, 1000, 600)
    e.append(_pair_entry("single_local", q, t, CL, 11, 2, B62, [_is(_ffi.FLAG_SINGLE)], want_d=True))
    q, t = _related_pair(rng, 700, 900)
    e.append(_pair_entry("single_global", q, t, CG, 11, 2, B62, [_is(_ffi.FLAG_SINGLE)], env={"ALN_SINGLE_R": "2"}))
    q, t = _related_pair(rng, 300, 600)
    real = np.round(B62 * 0.5 + np.random.default_rng(8).normal(0, 0.05, B62.shape), 3)
    e.append(_pair_entry("wg_real", q, t, CL, 11.5, 2.25, real, [_is(_ffi.FLAG_WORKGROUP), _not(_ffi.FLAG_INTEGER)], want_d=True))
    q, t = _related_pair(rng, 200, 150)
    e.append(_pair_entry("wg_integer_h_d", q, t, CL, 11, 2, B62, [_is(_ffi.FLAG_WORKGROUP)], want_d=True, want_h=True, force_generic=True))
    e.append(_batch_entry("f64_strip_batch", _pairs(9, _shapes(9, 90, (20, 400), (20, 700))), CL, 11.3, 2.1, B62 * 0.37, [_not(_ffi.FLAG_INTEGER)]))
    ipwm = np.random.default_rng(10).integers(-1, 2, (4, 150)).astype(np.float64)
    e.append(_pwm_entry("pwm_fast_windows", 10, ipwm, 3, 1, 120, 200, [_is(_ffi.FLAG_FAST)]))
    rpwm = np.round(np.random.default_rng(11).normal(0, 1, (4, 100)), 2)
    e.append(_pwm_entry("pwm_real_windows", 11, rpwm, 1.5, 0.4, 60, 160, [_not(_ffi.FLAG_INTEGER)]))
    q, t = _related_pair(rng, 77, 140)
    e.append(_pair_entry("force_serial", q, t, CL, 11, 2, B62, [lambda got: bool((got["_passes"] & 0x80).all())], want_d=True, want_h=True, force_serial=True))
    pb = _pairs(12, _shapes(12, 300, (20, 400), (20, 400)))
    e.append(_batch_entry("pipelined_four_slots", pb, CL, 11, 2, B62, fast_batch, env={"ALN_CHUNK_CELLS": str(pb.cells // 7)}))
    e.append(_shuffle_entry("shuffle_scores", 13))
    e.append(_scan_entry("scan_hits_held_list", 14))
    _catalogue.extend(e)
    return _catalogue


def planned_chunks(entry):
    """The number of chunks aln_align_batch cuts a batch entry into, under the entry's knobs (host arithmetic: no GPU)."""
    s = entry.shape
    ql, tl = s["q_len"].astype(np.uint64), s["t_len"].astype(np.uint64)
    p = _ffi.Params(int(s["semantics"]), 0, float(s["dele"]), float(s["ext"]), None, 24, 24, 24, 3, 98, 0, 0, 0, 0)
    with knobs(entry.env):
        return int(_ffi.load().aln_plan_chunks(C.byref(p), ql.ctypes.data, tl.ctypes.data, len(ql), 1, None, None, 0))


class knobs:
    """Sets environment knobs for one call and puts back what was there."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def save_expected(path, wants):
    flat = {}
    for name, want in wants.items():
        for k, v in want.items():
            flat[name + "/" + k] = np.asarray(v)
    np.savez(path, **flat)


def load_expected(path):
    wants = {}
    with np.load(path) as z:
        for key in z.files:
            name, k = key.split("/", 1)
            wants.setdefault(name, {})[k] = z[key]
    return wants


# ---------------------------------------------------------------- the tag-wrap batches
WRAP_SHAPES = [(120, 520), (200, 600), (330, 700), (90, 1100), (250, 1030)]      # multi-strip, each under 2^18 cells


def wrap_batches():
    """Three batches of identical shapes and different residues: a few multi-strip pairs, far fewer than resident waves (their
    strips are shared), each under the 2^18 cells from which a small chunk's pairs go to the single-pair route."""
    assert all(m > STRIP_ROWS and n * m < (1 << 18) for n, m in WRAP_SHAPES)
    return [_pairs(100 + k, WRAP_SHAPES) for k in range(3)]


PASS_PAIRS = 22000


def pass_batch(n_pairs=PASS_PAIRS):
    """22 000 pairs of 8..64 columns and 513..1100 rows (two or three strips: each is one multi-strip pass of the wave that takes
    it, at least), all residues random, a run of the query planted in the target of every third."""
    rng = np.random.default_rng(4096)
    N = rng.integers(8, 65, n_pairs)
    M = rng.integers(513, 1101, n_pairs)
    q_off = np.zeros(n_pairs, np.uint64); t_off = np.zeros(n_pairs, np.uint64)
    pos = np.cumsum(np.stack([N, M], axis=1).ravel())
    q_off[:] = np.concatenate([[0], pos[1:-1:2]]); t_off[:] = pos[0::2]
    seqs = rng.integers(0, 20, int(pos[-1])).astype(np.uint8)
    for i in range(0, n_pairs, 3):
        n, m = int(N[i]), int(M[i])
        at = int(t_off[i]) + (i * 7919) % (m - n + 1)
        run = seqs[int(q_off[i]):int(q_off[i]) + n].copy()
        mut = rng.random(n) < 0.08
        run[mut] = rng.integers(0, 20, int(mut.sum()))
        seqs[at:at + n] = run
    return PairBatch(seqs, q_off, N.astype(np.uint64), t_off, M.astype(np.uint64))


# ---------------------------------------------------------------- the child processes of tests/test_call_history_gpu.py
# python call_history.py MODE expected.npz report.json: runs on the GPU in a context of its own, compares every call with the
# expected answers (computed by the parent from the oracle) and writes what it found; the parent asserts.
WRAP_SEMS = (("core_local", 1), ("core_global", 0))
POOLED_CALLS = 2100                 # > 2 * 1024 + 50 launches on the pooled slot, per semantics
STAGED_RUNS = 1100                  # > 1024 + 50 launches on each staged batch's private slot


def wrap_expected(orc):
    S = get_blosum62()
    return {"%s/%d" % (name, k): batch_expected(orc, b, sem, 11, 2, S) for name, sem in WRAP_SEMS for k, b in enumerate(wrap_batches())}


def pass_expected(orc, sem):
    return batch_expected(orc, pass_batch(), sem, 11, 2, get_blosum62())


def _flat_load(path):
    wants = {}
    with np.load(path) as z:
        for key in z.files:
            name, k = key.rsplit("/", 1)
            wants.setdefault(name, {})[k] = z[key]
    return wants


def flat_save(path, wants):
    np.savez(path, **{name + "/" + k: np.asarray(v) for name, want in wants.items() for k, v in want.items()})


def _child_schedule(wants):
    import time
    cat = catalogue()
    calls = []
    for step, i in enumerate(schedule(len(cat))):
        e = cat[i]
        t0 = time.perf_counter()
        with knobs(e.env):
            got = e.run()
        dt = time.perf_counter() - t0
        calls.append(dict(step=step, entry=e.name, diff=compare(got, wants[e.name]), routed=bool(e.routed(got)), seconds=dt))
    return dict(calls=calls)


def _fast_batch_route(got):
    return bool((got["_flags"] & _ffi.FLAG_FAST).all()) and not bool((got["_flags"] & _ffi.FLAG_SINGLE).any())


def _child_wrap_pooled(wants):
    import time
    S, batches, out = get_blosum62(), wrap_batches(), {}
    for name, sem in WRAP_SEMS:
        bad, t0 = [], time.perf_counter()
        for n in range(POOLED_CALLS):
            k = n % 3
            got = batch_got(align_batch(batches[k], sem, 11, 2, S))
            diff = compare(got, wants["%s/%d" % (name, k)])
            if diff is None and not _fast_batch_route(got):
                diff = "not the fast batch kernel: flags %s" % got["_flags"].tolist()
            if diff is not None:
                bad.append([n, k, diff])
        out[name] = dict(calls=POOLED_CALLS, bad=len(bad), first_bad=bad[:10], seconds=time.perf_counter() - t0)
    return out


def _child_wrap_staged(wants):
    import time
    from aligner_amd.batch import StagedBatch
    S, batches, out = get_blosum62(), wrap_batches(), {}
    for name, sem in WRAP_SEMS:
        staged = [StagedBatch(b, sem, 11, 2, S, outputs=_ffi.OUT_SCORE | _ffi.OUT_TRACEBACK) for b in batches]
        bad, t0 = [], time.perf_counter()
        for n in range(STAGED_RUNS):
            for k, sb in enumerate(staged):
                sb.run()
                got = batch_got(sb.fetch(True))
                diff = compare(got, wants["%s/%d" % (name, k)])
                if diff is None and not _fast_batch_route(got):
                    diff = "not the fast batch kernel: flags %s" % got["_flags"].tolist()
                if diff is not None:
                    bad.append([n, k, diff])
        out[name] = dict(runs_each=STAGED_RUNS, batches=len(staged), bad=len(bad), first_bad=bad[:10], seconds=time.perf_counter() - t0)
        for sb in staged:
            sb.close()
    return out


def _child_passes(wants):
    import time
    S, b, out = get_blosum62(), pass_batch(), {}
    for name, sem in WRAP_SEMS:
        want = wants[name]
        t0 = time.perf_counter()
        got = batch_got(align_batch(b, sem, 11, 2, S))
        dt = time.perf_counter() - t0
        bad = np.zeros(len(b), dtype=bool)
        for f in FIELDS:
            bad |= got[f] != want[f]
        if not bad.any():                                # per pair: both strings (the lengths agree)
            same = got["_tb"][want["_idx"]] == want["strings"]
            ends = np.cumsum(2 * want["aln_len"].astype(np.int64))
            wrong = np.searchsorted(ends, np.nonzero(~same)[0], side="right")
            bad[wrong] = True
        out[name] = dict(pairs=len(b), bad=int(bad.sum()), first_bad=np.nonzero(bad)[0][:10].tolist(), diff=compare(got, want),
                         routed=_fast_batch_route(got), seconds=dt)
    return out


def main(argv):
    import json
    mode, expected, report = argv
    wants = load_expected(expected) if mode == "schedule" else _flat_load(expected)
    run = dict(schedule=_child_schedule, wrap_pooled=_child_wrap_pooled, wrap_staged=_child_wrap_staged, passes=_child_passes)[mode]
    with open(report, "w") as f:
        json.dump(run(wants), f)


if __name__ == "__main__":
    main(sys.argv[1:])
