"""HeuristicAligner / HeuristicPWMAligner -- the matrix re-estimation loop around the DP path.

Mirror of aligner-core/src/heuristic/mod.rs:9-78 (pairwise) and :80-140 (PWM), with the helper numerics they call:
`transform_matrix` / `get_threshold` (aligner-helpers/src/matrices/mod.rs:8-68).  Each iteration is one hot-path call
with a REAL-VALUED matrix, so it runs on the f64 kernels (|max - x| < f64::EPSILON tie test, no fma contraction).
The loop itself is sequential (each matrix depends on the previous alignment) and stays on the host, as in the reference.

Third-party arithmetic not in the reference tree: roots 0.0.7 `find_roots_quadratic` (Cargo.lock:1781-1782), restated
below from its published algorithm (discriminant test, then the non-cancelling pair of formulas, roots in ascending
order).  No reference test covers this path: parity unpinned beyond source reading.
"""
import numpy as np

from .errors import AlignerError, ErrorKind, ReferencePanic
from .pwm import PWMAligner
from .simple import Heuristics, SimpleLocalAligner


class WrongMatrixSpecified(Exception):
    """`Err(aligner_helpers::Error::WrongMatrixSpecified)` (aligner-helpers/src/lib.rs:11-14)."""


def get_threshold(dim_1):
    """aligner-helpers/src/matrices/mod.rs:8-17."""
    return {20: 22.6, 21: 23.1, 22: 23.6, 23: 24.1, 24: 24.6}.get(dim_1, 0.0)


def find_roots_quadratic(a2, a1, a0):
    """roots 0.0.7: returns () / (x,) / (x_lo, x_hi)."""
    if a2 == 0.0:
        return () if a1 == 0.0 else (-a0 / a1,)
    disc = a1 * a1 - 4.0 * a2 * a0
    if disc < 0.0:
        return ()
    a2x2 = 2.0 * a2
    if disc == 0.0:
        return (-a1 / a2x2,)
    sq = np.sqrt(disc)
    same_sign, diff_sign = (-a1 + sq, -a1 - sq) if a1 < 0.0 else (-a1 - sq, -a1 + sq)
    if abs(same_sign) > abs(a2x2):
        a0x2 = 2.0 * a0
        if abs(diff_sign) > abs(a2x2):
            x1, x2 = a0x2 / same_sign, a0x2 / diff_sign
        else:
            x1, x2 = a0x2 / same_sign, same_sign / a2x2
    else:
        x1, x2 = diff_sign / a2x2, same_sign / a2x2
    return (x1, x2) if x1 < x2 else (x2, x1)


def transform_matrix(matrix, k_d, r_squared, frequencies):
    """aligner-helpers/src/matrices/mod.rs:19-68: rescale `matrix` so that its expectation under p = freq x uniform is k_d
    and its squared norm is r_squared."""
    m = np.asarray(matrix, dtype=np.float64)
    ncols = m.shape[1]
    f = np.full(ncols, 1.0 / ncols)
    p = np.outer(np.asarray(frequencies, dtype=np.float64), f)
    p_squared = (p * p).sum()
    k_0 = (p * m).sum()
    a = (k_d - k_0) / p_squared
    b = k_d / p_squared
    base = m + p * (a - b)
    denominator = (base * base).sum()
    a_coeff = (2.0 * b * (p * base).sum()) / denominator
    b_coeff = (b * b * p_squared - r_squared) / denominator
    roots = find_roots_quadratic(1.0, a_coeff, b_coeff)
    if len(roots) == 0:
        raise WrongMatrixSpecified()
    if len(roots) == 1:
        return p * b + roots[0] * base
    if roots[0] > 0.0 and roots[1] < 0.0:
        return p * b + roots[0] * base
    if roots[0] < 0.0 and roots[1] > 0.0:
        return p * b + roots[1] * base
    m1 = p * b + roots[0] * base
    m2 = p * b + roots[1] * base
    d1 = np.sqrt(((m - m1) ** 2).sum())
    d2 = np.sqrt(((m - m2) ** 2).sum())
    return m1 if d1 < d2 else m2


def _transform_or_panic(matrix, params):
    try:                                                                        # `.unwrap()` at heuristic/mod.rs:53, :71
        return transform_matrix(matrix, params.kd, params.r_squared, params.frequencies)
    except WrongMatrixSpecified:
        raise ReferencePanic(-1, "called `Result::unwrap()` on an `Err` value: WrongMatrixSpecified") from None


class _HeuristicLoop:
    def _loop(self, make_aligner, del_, ext, matrix, params, device):
        transformed = _transform_or_panic(matrix, params)
        max_f = 0.0
        while True:
            result = make_aligner().perform_alignment(del_, ext, transformed, None, device=device)
            if result.alignment.f > max_f:                                      # heuristic/mod.rs:64-72
                max_f = result.alignment.f
                transformed = _transform_or_panic(result.alignment.get_frequency_matrix(), params)
            else:
                result.matrix = transformed                                     # :73-75
                return result


class HeuristicAligner(_HeuristicLoop):
    """heuristic/mod.rs:9-78."""

    def __init__(self, query, target, alphabet):
        self.alphabet, self.query, self.target = alphabet, np.array(query, np.uint8), np.array(target, np.uint8)

    @classmethod
    def from_str_seqs(cls, query, target, alphabet):
        return cls(alphabet.str_to_vec(query), alphabet.str_to_vec(target), alphabet)

    @classmethod
    def from_seqs(cls, query, target, alphabet):
        return cls(query, target, alphabet)

    def perform_alignment(self, del_, ext, matrix, heuristics=None, device=None):
        if heuristics is None:
            raise AlignerError(ErrorKind.MissingArgument)                       # :42-45
        m = np.asarray(matrix, dtype=np.float64)
        params = Heuristics(heuristics.kd, heuristics.r_squared, heuristics.frequencies)
        if abs(params.r_squared - 0.0) < np.finfo(np.float64).eps:              # :47-49
            params.r_squared = float(m.shape[0] * m.shape[1])
        return self._loop(lambda: SimpleLocalAligner.from_seqs(self.query, self.target, self.alphabet), del_, ext, m,
                          params, device)


def _wrong_matrix_panic():
    return ReferencePanic(-1, "called `Result::unwrap()` on an `Err` value: WrongMatrixSpecified")


def _transform_batch(how, matrices, params_list):
    """transform_matrix for a list of (matrix, Heuristics): a list of matrices, a ReferencePanic in the place of a matrix the
    reference would panic on."""
    if how == "numpy":
        out = []
        for m, h in zip(matrices, params_list):
            try:
                out.append(_transform_or_panic(m, h))
            except ReferencePanic as e:
                out.append(e)
        return out
    if how != "native":
        raise ValueError("transform: 'numpy' or 'native'")
    if not len(matrices):
        return []
    from . import _ffi
    from .pairset import transform_matrices
    res, status = transform_matrices(np.asarray(matrices, dtype=np.float64),
                                     np.asarray([np.asarray(h.frequencies, dtype=np.float64) for h in params_list]),
                                     np.asarray([h.kd for h in params_list], dtype=np.float64),
                                     np.asarray([h.r_squared for h in params_list], dtype=np.float64))
    return [res[k] if status[k] == 0 else _wrong_matrix_panic() for k in range(len(status))]


def align_many(pairs, del_, ext, matrix, heuristics, alphabet=None, transform="numpy", device=None, errors="raise", backend=None):
    """HeuristicAligner.from_seqs(q, t, alphabet).perform_alignment(del_, ext, matrix, heuristics) for every (q, t) of `pairs`, in
    lock step on one resident pair set (aligner_amd.pairset.PairSet): every iteration is ONE run over the pairs that are still
    going, each under its own matrix; the pairs whose f did not grow finish and have their strings fetched, the others have their
    frequency matrices counted on the device and transformed on the host.

    heuristics: one Heuristics, or one per pair.  transform: "numpy" (transform_matrix per pair: the single-pair class's bits by
    construction), "native" (aln_transform_matrices, the same order of operations in the library's host code) or "resident" (the
    same order again in a kernel: the parameters go up once, PairSet.reestimate rebuilds the matrices on the device from the held
    strings, run_stored aligns under them, and only the matrices of finished pairs come back).  Returns the
    AlignmentResults in input order, `matrix` being the matrix of the pair's last run.  A pair on which the reference panics
    (empty sequence, code outside the matrix, no positive cell, WrongMatrixSpecified) gives the same ReferencePanic: raised for the
    first such pair (errors="raise") or returned in its place (errors="return").  The matrix must be volume x volume of the
    alphabet (the shape of the frequency matrices) and hold at most 1024 entries.
    backend: a factory (pairs, device) -> object with run / frequencies / strings / close (tests); in "resident" mode with
    set_heuristics / reestimate / run_stored / matrices / strings / close."""
    from . import _ffi
    from . import runtime
    from .alignment import Alignment, AlignmentResult
    from .enums import Protein
    if alphabet is None:
        alphabet = Protein
    if heuristics is None:
        raise AlignerError(ErrorKind.MissingArgument)                           # heuristic/mod.rs:42-45
    if errors not in ("raise", "return"):
        raise ValueError("errors: 'raise' or 'return'")
    if transform not in ("numpy", "native", "resident"):
        raise ValueError("transform: 'numpy', 'native' or 'resident'")
    resident = transform == "resident"
    pairs = [(np.array(q, dtype=np.uint8), np.array(t, dtype=np.uint8)) for q, t in pairs]
    n = len(pairs)
    m = np.asarray(matrix, dtype=np.float64)
    v = alphabet.volume()
    if m.shape != (v, v):
        raise ValueError("align_many: the matrix must be %d x %d (the alphabet's frequency matrix)" % (v, v))
    hs = list(heuristics) if isinstance(heuristics, (list, tuple)) else [heuristics] * n
    if len(hs) != n:
        raise ValueError("heuristics: one, or one per pair")
    if any(h is None for h in hs):
        raise AlignerError(ErrorKind.MissingArgument)
    params = []
    for h in hs:
        r2 = h.r_squared
        if abs(r2 - 0.0) < np.finfo(np.float64).eps:                            # :47-49
            r2 = float(m.shape[0] * m.shape[1])
        params.append(Heuristics(h.kd, r2, h.frequencies))
    out = [None] * n
    if n == 0:
        return out
    if backend is None:
        from .pairset import PairSet
        backend = PairSet
    blank = alphabet.blank()
    active = list(range(n))
    max_f = np.zeros(n, dtype=np.float64)
    if not resident:
        current = dict(zip(active, _transform_batch(transform, [m] * n, params)))
    ps = backend(pairs, device)
    try:
        if resident:                                                            # current[i]: True, the matrix being store entry i
            ps.set_heuristics(m.shape[0], m.shape[1], np.asarray([np.asarray(h.frequencies, dtype=np.float64) for h in params]),
                              np.asarray([h.kd for h in params], dtype=np.float64),
                              np.asarray([h.r_squared for h in params], dtype=np.float64))
            status = ps.reestimate(active, matrix=m)
            current = {i: True if status[k] == 0 else _wrong_matrix_panic() for k, i in enumerate(active)}
        while active:
            going = []
            for i in active:                                                    # `.unwrap()` at heuristic/mod.rs:53, :71
                if isinstance(current[i], ReferencePanic):
                    out[i] = current.pop(i)
                else:
                    going.append(i)
            active = going
            if not active:
                break
            if resident:
                res = ps.run_stored(_ffi.CORE_LOCAL, del_, ext, active, blank=blank)
            else:
                res = ps.run(_ffi.CORE_LOCAL, del_, ext, np.asarray([current[i] for i in active], dtype=np.float64), active, blank=blank)
            done, more = [], []
            for k, i in enumerate(active):
                st = int(res["status"][k])
                if st != _ffi.OK:
                    try:
                        runtime.raise_for_status(st, "aln_pairset_run")
                    except ReferencePanic as e:
                        out[i] = e
                    current.pop(i)
                elif res["f"][k] > max_f[i]:                                    # :64-72
                    max_f[i] = res["f"][k]
                    more.append(i)
                else:
                    done.append(i)
            if done:
                summ, strs = ps.strings(done)
                if resident:
                    for i, mat in zip(done, ps.matrices(done)):
                        current[i] = mat.copy()
                for k, i in enumerate(done):
                    r = summ[k]
                    coords = ((int(r["start_x"]) + 1, int(r["end_x"]) + 1), (int(r["start_y"]) + 1, int(r["end_y"]) + 1))
                    aln = Alignment(alphabet, strs[k][0], strs[k][1], coords, float(r["f"]))
                    out[i] = AlignmentResult(aln, matrix=current.pop(i), score=float(r["score"]),      # :73-75
                                             summary={name: r[name].item() for name in r.dtype.names})
            if more and resident:
                status = ps.reestimate(more)
                for k, i in enumerate(more):
                    if status[k] != 0:
                        current[i] = _wrong_matrix_panic()
            elif more:
                counts = ps.frequencies(more)
                new = _transform_batch(transform, [counts[k].astype(np.float64) for k in range(len(more))], [params[i] for i in more])
                for i, mat in zip(more, new):
                    current[i] = mat
            active = more
    finally:
        ps.close()
    if errors == "raise":
        for r in out:
            if isinstance(r, ReferencePanic):
                raise r
    return out


def align_set(seqset, del_, ext, matrix, heuristics, block=None, max_pairs=1 << 18, errors="return", backend=None):
    """HeuristicAligner for every pair of a block of a resident SeqSet (default: every pair i < j, the request path of the reference):
    a generator of (pair_index, q, t, AlignmentResult | ReferencePanic) in pair order, q and t being sequence numbers of the set
    (sequence q the query), `result.matrix` the matrix of the pair's last run -- what align_many(..., transform="resident") gives for
    the same pairs, bit for bit.

    The block is taken in slices of at most max_pairs consecutive pairs.  A slice is one pair set derived from the set
    (PairSet.from_seqset: the residues are the set's, nothing is uploaded) and driven by PairSet.loop_step: the decision, the
    re-estimation and the going list stay on the device, and per step only the finished pairs come back.  What bounds a slice is its
    per-pair device memory: the store entry and the compact run matrix (8 * v * v bytes each, v the alphabet's volume), the held
    strings (2 * (N + M + 2)), the summary (2 * 48) and the loop's words (36) -- about 10 KiB per pair of 300-residue proteins under a
    24 x 24 matrix, 2.5 GiB for the default slice.

    heuristics: one Heuristics for every pair, or a callable (q, t) -> Heuristics.  r_squared == 0 stands for rows * cols
    (heuristic/mod.rs:47-49), as in align_many.  errors: "return" yields a ReferencePanic in the place of a pair the reference panics
    on; "raise" raises the first one in pair order.  All per-pair work of the host is numpy on arrays.
    backend: a factory (seqset, block, first, n) -> object with q / t / set_heuristics / loop_begin / loop_step / strings / matrices /
    close (tests)."""
    from . import _ffi
    from . import runtime
    from . import seqset as seqset_module
    from .alignment import Alignment, AlignmentResult
    if heuristics is None:
        raise AlignerError(ErrorKind.MissingArgument)                           # heuristic/mod.rs:42-45
    if errors not in ("raise", "return"):
        raise ValueError("errors: 'raise' or 'return'")
    if int(max_pairs) < 1:
        raise ValueError("max_pairs: at least 1")
    alphabet = seqset.alphabet
    m = np.asarray(matrix, dtype=np.float64)
    v = alphabet.volume()
    if m.shape != (v, v):
        raise ValueError("align_set: the matrix must be %d x %d (the alphabet's frequency matrix)" % (v, v))
    b = seqset_module._block(block, len(seqset))
    total = seqset.pairs(b)
    if total == 0:
        raise ValueError("align_set: invalid block (a range beyond the set, unequal ranges of an upper block, or no pairs)")
    if backend is None:
        from .pairset import PairSet
        backend = PairSet.from_seqset
    eps = np.finfo(np.float64).eps
    blank = alphabet.blank()
    for first in range(0, total, int(max_pairs)):
        n = min(int(max_pairs), total - first)
        ps = backend(seqset, b, first, n)
        try:
            sq, st_ = np.asarray(ps.q), np.asarray(ps.t)
            if callable(heuristics):
                hs = [heuristics(int(a), int(c)) for a, c in zip(sq, st_)]
                if any(h is None for h in hs):
                    raise AlignerError(ErrorKind.MissingArgument)
                freq = np.asarray([np.asarray(h.frequencies, dtype=np.float64) for h in hs])
                kd = np.asarray([h.kd for h in hs], dtype=np.float64)
                r2 = np.asarray([h.r_squared for h in hs], dtype=np.float64)
            else:
                freq = np.broadcast_to(np.asarray(heuristics.frequencies, dtype=np.float64), (n, v))
                kd = np.full(n, heuristics.kd, dtype=np.float64)
                r2 = np.full(n, heuristics.r_squared, dtype=np.float64)
            r2 = np.where(np.abs(r2 - 0.0) < eps, float(m.shape[0] * m.shape[1]), r2)      # :47-49
            ps.set_heuristics(v, v, freq, kd, r2)
            out = np.empty(n, dtype=object)
            status = np.asarray(ps.loop_begin(m))
            for i in np.flatnonzero(status != 0):                               # `.unwrap()` at heuristic/mod.rs:53
                out[i] = _wrong_matrix_panic()
            more = int((status == 0).sum())
            while more:
                fin, cause, res, counts = ps.loop_step(_ffi.CORE_LOCAL, del_, ext, blank=blank)
                if counts[0] != more or counts[1] + counts[2] + counts[3] != counts[0] or len(fin) != counts[1] + counts[2]:
                    raise RuntimeError("align_set: a step's counters do not add up")
                more = counts[3]
                done = fin[cause == _ffi.LOOP_CAUSE_DONE]
                for i, r in zip(fin[cause == _ffi.LOOP_CAUSE_FAILED], res[cause == _ffi.LOOP_CAUSE_FAILED]):
                    try:
                        runtime.raise_for_status(int(r["status"]), "aln_pairset_loop_step")
                    except ReferencePanic as e:
                        out[i] = e
                for i in fin[cause == _ffi.LOOP_CAUSE_NO_ROOT]:                  # `.unwrap()` at :71
                    out[i] = _wrong_matrix_panic()
                if len(done):
                    summ, strs = ps.strings(done)
                    mats = ps.matrices(done)
                    for k, i in enumerate(done):
                        r = summ[k]
                        coords = ((int(r["start_x"]) + 1, int(r["end_x"]) + 1), (int(r["start_y"]) + 1, int(r["end_y"]) + 1))
                        aln = Alignment(alphabet, strs[k][0], strs[k][1], coords, float(r["f"]))
                        out[i] = AlignmentResult(aln, matrix=mats[k].copy(), score=float(r["score"]),      # :73-75
                                                 summary={name: r[name].item() for name in r.dtype.names})
        finally:
            ps.close()
        for i in range(n):
            if errors == "raise" and isinstance(out[i], ReferencePanic):
                raise out[i]
            yield first + i, int(sq[i]), int(st_[i]), out[i]


class HeuristicPWMAligner(_HeuristicLoop):
    """heuristic/mod.rs:80-140."""

    def __init__(self, query, alphabet):
        self.alphabet, self.query = alphabet, np.array(query, np.uint8)

    @classmethod
    def from_str_seqs(cls, query, _target, alphabet):
        return cls(alphabet.str_to_vec(query), alphabet)

    @classmethod
    def from_seqs(cls, query, _target, alphabet):
        return cls(query, alphabet)

    def perform_alignment(self, del_, ext, matrix, heuristics=None, device=None):
        if heuristics is None:
            raise AlignerError(ErrorKind.MissingArgument)
        return self._loop(lambda: PWMAligner.from_seqs(self.query, None, self.alphabet), del_, ext,
                          np.asarray(matrix, dtype=np.float64), heuristics, device)
