"""Batch driver behind calculate_p_value -- the reference's only in-tree batch site of the DP path.

Mirror of aligner-core/src/statistics/mod.rs:240-320: the reference spawns THREADS = 10 std::threads, each aligning
SEQUENCES / THREADS shuffled copies of the target against the query with SimpleLocalAligner and keeping only
`alignment.f` (:255-286; thread 5 does one alignment fewer so that, with the initial score, there are exactly 5000
samples).  Here the 4 999 shuffled targets are packed once and scored by ONE score-only batch call on the GPU
(no directions stored, no traceback).  The shuffling stays on the host (`thread_rng` in the reference is unseeded, so
parity for this function is statistical; parity of the scores for given shuffles is bit-exact and tested).

calculate_p_values / device_shuffled_scores are the same batch with the copies drawn on the device (aln_shuffle_scores): the
queries and original targets go up once, every copy is trimmed and shuffled by its own seeded stream (specified bit for bit in
aligner_amd/csrc/aln_shuffle_rules.h, restated in tests/shuffle_ref.py), and only the scores come back -- for many pairs in one
call, so that the chip has enough work.

The extreme-value fit that turns the scores into a p-value (statistics/mod.rs:36-238) is host numerics in the
reference as well; it is restated in numpy below (including the loop-scoped re-binding of k / lambda at :69) and pinned
by tests/test_host_logic.py against an independent scalar restatement (tests/pyref.py).
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from .batch import PairBatch, align_batch
from .errors import AlignerError, ErrorKind

MAXITER = 10000            # statistics/mod.rs:9-13
THREADS = 10
SEQUENCES = 5000
THRESHOLD_GLOBAL = 1e-6
THRESHOLD_LOCAL = 1e-4


def shuffle_and_randomize_sequence(sequence, rng):
    """statistics/mod.rs:309-320: drop 0..6 tail residues, then shuffle."""
    lock = int(rng.integers(0, 7))
    seq = np.array(sequence[:len(sequence) - lock], dtype=np.uint8, copy=True)
    rng.shuffle(seq)
    return seq


def shuffled_scores(query, target, initial_score, del_, ins, matrix, rng=None, device=None):
    """The scores / lengths vectors calculate_p_value builds (statistics/mod.rs:249-292), scored in one GPU batch.

    Returns (scores f64[5000], lengths int[5000], PairBatch of the 4 999 shuffled pairs)."""
    rng = rng or np.random.default_rng()
    query = np.asarray(query, dtype=np.uint8)
    target = np.asarray(target, dtype=np.uint8)
    pairs = []
    for i in range(THREADS):
        limit = SEQUENCES // THREADS
        if i == 5:
            limit = SEQUENCES - (SEQUENCES // THREADS * (THREADS - 1)) - 1      # :264-266
        for _ in range(limit):
            pairs.append((query, shuffle_and_randomize_sequence(target, rng)))
    batch = PairBatch.from_pairs(pairs)
    got = align_batch(batch, _ffi.CORE_LOCAL, del_, ins, matrix, device=device, want_traceback=False)
    bad = got.results["status"] != 0
    if bad.any():
        # the reference unwraps every perform_alignment (:273-277): a panic there is a panic here
        from .runtime import raise_for_status
        raise_for_status(int(got.results["status"][bad][0]), "calculate_p_value")
    scores = np.concatenate([[float(initial_score)], got.results["f"].astype(np.float64)])
    lengths = np.concatenate([[len(target)], batch.t_len.astype(np.int64)])
    return scores, lengths, batch


class DistributionParams:
    """statistics/mod.rs:15-34."""

    def __init__(self, k, lambda_, h):
        self.k, self.lambda_, self.h = k, lambda_, h

    def get_p_value(self, query_length, target_length, score):
        l = np.log(self.k * query_length * target_length) / self.h
        nn = (query_length - l) * (target_length - l)
        return 1.0 - np.exp(-self.k * nn * np.exp(-self.lambda_ * score))


def _nn(query_length, t, k, h):
    l = np.log(k * query_length * t) / h
    return (query_length - l) * (t - l)


def _estimate_k_and_lambda(query_length, t, scores, k, lam, h):
    """statistics/mod.rs:125-188 (Newton iteration on lambda, k from the normalisation)."""
    n = float(len(t))
    nn = _nn(query_length, t, k, h)
    es = np.exp(-lam * scores)
    s = (nn * es).sum()
    ws = (nn * scores * es).sum()
    with np.errstate(all="ignore"):
        for _ in range(MAXITER + 1):
            f = 1.0 / lam - scores.sum() / n + ws / s
            fd = -lam ** -2 - (nn * scores * scores * es).sum() / s + (ws / s) ** 2
            if not np.isfinite(f) or not np.isfinite(fd):
                return k, lam
            new_lam = lam - f / fd
            es = np.exp(-lam * scores)
            s = (nn * es).sum()
            ws = (nn * scores * es).sum()
            new_k = n / s
            if not np.isfinite(new_k) or new_k <= 0:
                return k, lam
            k, lam = new_k, new_lam
            if abs(f) < THRESHOLD_LOCAL:
                return k, lam
            nn = _nn(query_length, t, k, h)
    return k, lam


def _estimate_h(query_length, t, scores, k, lam, h):
    """statistics/mod.rs:190-238."""
    with np.errstate(all="ignore"):
        for _ in range(MAXITER + 1):
            l = np.log(k * query_length * t) / h
            nn = (query_length - l) * (t - l)
            a = 2.0 * l - query_length - t
            b = 1.0 / nn - k * np.exp(-lam * scores)
            c = -l / h
            g = (a * b * c).sum()
            gd = (2.0 * b * c * c - (a * c / nn) ** 2 - 2.0 * a * b * c / h).sum()
            if abs(g) < THRESHOLD_LOCAL:
                return h
            if gd > 0:
                h = h * 2.0 if g > 0 else h / 2.0
            elif g <= 0:
                h /= 2.0
            else:
                h -= g / gd
    return h


def calculate_distribution_params(query_length, target_lengths, scores):
    """statistics/mod.rs:36-123."""
    t_all = np.asarray(target_lengths, dtype=np.float64)
    s_all = np.asarray(scores, dtype=np.float64)
    if len(t_all) != len(s_all):
        raise AlignerError(ErrorKind.ValidationError)
    if len(s_all) == 0:
        raise AlignerError(ErrorKind.ValidationError)
    sd = ((s_all - s_all.mean()) ** 2).mean()          # central_moment(2), named `sd` in the reference
    lam = 1.0 / sd
    h = 1.0
    n = float(len(t_all))
    with np.errstate(all="ignore"):
        nn = query_length * t_all
        k = n / (nn * np.exp(-lam * s_all)).sum()
        ll = n * np.log(lam * k) + (np.log(nn) - lam * s_all - k * nn * np.exp(-lam * s_all)).sum()
        t_act, s_act = t_all.copy(), s_all.copy()
        # statistics/mod.rs:69: `let (k, lambda) = estimate_..(.., k, lambda, h)` SHADOWS inside the loop body, so every
        # iteration restarts the Newton step from the initial moment estimates k0 / lam0 (only h and the active subset
        # carry over), and the fall-through Ok(..) after MAXITER (:122) returns k0 / lam0 with the last h.
        k0, lam0 = k, lam
        for _ in range(MAXITER + 1):
            k, lam = _estimate_k_and_lambda(query_length, t_act, s_act, k0, lam0, h)
            h = _estimate_h(query_length, t_act, s_act, k, lam, h)
            nn = _nn(query_length, t_all, k, h)
            ll_new = n * np.log10(lam * k) + (np.log10(nn) - lam * s_all - k * nn * np.exp(-lam * s_all)).sum()
            if abs(ll_new - ll) / ll < THRESHOLD_GLOBAL:
                return DistributionParams(k, lam, h)
            ll = ll_new
            keep = n * (1.0 - np.exp(-k * nn * np.exp(-lam * s_all))) >= 1.0
            t_act, s_act = t_all[keep], s_all[keep]
    return DistributionParams(k0, lam0, h)


def calculate_p_value(query, target, initial_score, del_, ins, matrix, rng=None, device=None):
    """statistics/mod.rs:240-307."""
    scores, lengths, _ = shuffled_scores(query, target, initial_score, del_, ins, matrix, rng=rng, device=device)
    params = calculate_distribution_params(len(query), lengths, scores)
    return float(params.get_p_value(len(query), len(target), initial_score))


# ---------------------------------------------------------------- copies drawn on the device (aln_shuffle_*)
def _as_pairs(pairs):
    if isinstance(pairs, PairBatch):
        return pairs
    return PairBatch.from_pairs(pairs)


def _spec(seed, per_pair, max_trim, pair_base):
    return _ffi.ShuffleSpec(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair_base) & 0xFFFFFFFFFFFFFFFF, int(per_pair), int(max_trim))


def device_shuffled_scores(pairs, del_, ins, matrix, seed, per_pair=SEQUENCES - 1, max_trim=6, pair_base=0, device=None,
                           semantics=_ffi.CORE_LOCAL, check=True):
    """Scores of every pair's query against per_pair trimmed and shuffled copies of its target, drawn on the device.

    pairs: a PairBatch or (query, target) pairs.  Returns (f float64[n, per_pair], lengths uint32[n, per_pair], status
    int32[n]): copy s of pair i comes from the stream (seed, pair_base + i, s).  A failed pair raises as shuffled_scores does
    (check=False: its status is returned instead and the other pairs are still scored)."""
    from .runtime import context, make_params, raise_for_status
    b = _as_pairs(pairs)
    n = len(b)
    f = np.zeros((n, per_pair), dtype=np.float64)
    lengths = np.zeros((n, per_pair), dtype=np.uint32)
    status = np.zeros(n, dtype=np.int32)
    p, _keep = make_params(semantics, del_, ins, matrix, outputs=_ffi.OUT_SCORE)
    spec = _spec(seed, per_pair, max_trim, pair_base)
    st = _ffi.load().aln_shuffle_scores(context(device), C.byref(p), C.byref(spec), b.seqs.ctypes.data, b.q_off.ctypes.data,
                                        b.q_len.ctypes.data, b.t_off.ctypes.data, b.t_len.ctypes.data, n, f.ctypes.data,
                                        lengths.ctypes.data, status.ctypes.data)
    raise_for_status(st, "aln_shuffle_scores")
    if check and (status != 0).any():
        # the reference unwraps every perform_alignment (statistics/mod.rs:273-277): a panic there is a panic here
        raise_for_status(int(status[status != 0][0]), "aln_shuffle_scores")
    return f, lengths, status


def shuffle_targets(targets, seed, per_pair=SEQUENCES - 1, max_trim=6, pair_base=0, device=None):
    """The copies device_shuffled_scores aligns: for every target a uint8[per_pair, len(target)] array whose row s holds copy s
    in its first lengths[s] bytes (0 behind them), and the lengths.  Returns (copies list, lengths uint32[n, per_pair])."""
    from .runtime import context, raise_for_status
    ts = [np.ascontiguousarray(t, dtype=np.uint8) for t in targets]
    n = len(ts)
    t_len = np.array([len(t) for t in ts], dtype=np.uint64)
    t_off = np.zeros(n, dtype=np.uint64)
    if n > 1:
        t_off[1:] = np.cumsum(t_len)[:-1]
    seqs = np.concatenate(ts) if n else np.zeros(0, dtype=np.uint8)
    out_off = t_off * np.uint64(per_pair)
    out = np.zeros(max(int(t_len.sum()) * per_pair, 1), dtype=np.uint8)
    spec = _spec(seed, per_pair, max_trim, pair_base)
    st = _ffi.load().aln_shuffle_targets(context(device), C.byref(spec), seqs.ctypes.data, t_off.ctypes.data, t_len.ctypes.data, n,
                                         out.ctypes.data, out_off.ctypes.data)
    raise_for_status(st, "aln_shuffle_targets")
    copies = [out[int(out_off[i]):int(out_off[i]) + per_pair * len(ts[i])].reshape(per_pair, len(ts[i])) for i in range(n)]
    lengths = np.array([len(ts[i]) - _trims(seed, pair_base + i, per_pair, max_trim) for i in range(n)],
                       dtype=np.uint32).reshape(n, per_pair)
    return copies, lengths


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _trims(seed, pair, per_pair, max_trim):
    """The first draw of the streams of copies 0 .. per_pair - 1 of `pair` (aln_shuffle_rules.h: aln_shuffle_trim_of), vectorized:
    the trims the device applied, i.e. the lengths aln_shuffle_targets does not return."""
    u = np.uint64
    s = np.arange(per_pair, dtype=np.uint64)
    with np.errstate(over="ignore"):
        state = u(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (u(int(pair) & 0xFFFFFFFFFFFFFFFF) * u(0xD1B54A32D192ED03)) ^ \
            ((s + u(1)) * u(0xABC98388FB8FAC03))
        n = u(int(max_trim) + 1)
        t = u(((1 << 32) - int(n)) % int(n))

        def draw(st):
            z = st + u(0x9E3779B97F4A7C15)
            x = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> u(27))) * u(0x94D049BB133111EB)
            return z, ((x ^ (x >> u(31))) >> u(32)) * n

        state, m = draw(state)
        low = m & u(0xFFFFFFFF)
        redo = low < t
        while redo.any():
            state[redo], m[redo] = draw(state[redo])
            low = m & u(0xFFFFFFFF)
            redo = low < t
    return (m >> u(32)).astype(np.int64)


def calculate_p_values(pairs, del_, ins, matrix, initial_scores=None, seed=None, device=None):
    """calculate_p_value (statistics/mod.rs:240-307) for many pairs in one device call: pair i's scores are
    [initial_i] + the f of its 4 999 copies, its lengths [len(target_i)] + theirs, fitted and evaluated by the same
    calculate_distribution_params / get_p_value.  initial_scores=None: one score-only batch of the pairs themselves (what
    blast_p_value_cmp.rs computes before it calls calculate_p_value); seed=None: one drawn from OS entropy, as the
    reference's unseeded thread_rng.  Returns float64[n]."""
    b = _as_pairs(pairs)
    n = len(b)
    if initial_scores is None:
        got = align_batch(b, _ffi.CORE_LOCAL, del_, ins, matrix, device=device, want_traceback=False)
        bad = got.results["status"] != 0
        if bad.any():
            from .runtime import raise_for_status
            raise_for_status(int(got.results["status"][bad][0]), "calculate_p_values")
        initial_scores = got.results["f"].astype(np.float64)
    initial_scores = np.asarray(initial_scores, dtype=np.float64)
    if len(initial_scores) != n:
        raise AlignerError(ErrorKind.ValidationError)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    f, lengths, _ = device_shuffled_scores(b, del_, ins, matrix, seed, device=device)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        ql, tl = int(b.q_len[i]), int(b.t_len[i])
        scores = np.concatenate([[initial_scores[i]], f[i]])
        lens = np.concatenate([[tl], lengths[i].astype(np.int64)])
        params = calculate_distribution_params(ql, lens, scores)
        out[i] = float(params.get_p_value(ql, tl, initial_scores[i]))
    return out
