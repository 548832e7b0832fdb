"""Helpers of the held-hits tests (tests/test_repeats_held_*.py): a CPU scan that offers `hits` computed from the oracle's select
pass, a recorder that also forwards `hits`, the planted chromosomes of the engine cases, and the comparison of two engine runs.
Not a test module (no test_ prefix)."""
import numpy as np

from aligner_amd import repeats as R
from repeats_oracle_backend import OracleScan

_MEMO = {}


class MemoOracleScan(OracleScan):
    """OracleScan whose window alignments are remembered for the process: the engines under comparison align the same windows."""

    def _align(self, w, matrix, del_, ext):
        key = (np.asarray(w).tobytes(), np.asarray(matrix, dtype=np.float64).tobytes(), float(del_), float(ext))
        if key not in _MEMO:
            _MEMO[key] = OracleScan._align(self, w, matrix, del_, ext)
        return _MEMO[key]


class MemoOracleBackend:
    def scan(self, seq):
        return MemoOracleScan(seq)


class FakeHeld:
    """What `hits` returns, on the host: frequencies are summed from the oracle's alignments."""

    def __init__(self, owner, idx, alns, W):
        self.owner, self.idx, self._alns, self.W = owner, np.asarray(idx, dtype=np.int64), alns, W
        self.f = np.array([a.f for a in alns], dtype=np.float64)
        self.generation = owner.generation

    def _check(self):
        assert self.generation == self.owner.generation, "held hits used after a later pass replaced them"

    def frequencies(self, keep):
        self._check()
        out = np.zeros((4, self.W), dtype=np.float64)
        for k in keep:
            out = out + self._alns[int(k)].get_frequency_matrix()
        return out

    def alignments(self, keep):
        self._check()
        self.owner.fetched += len(keep)
        return [self._alns[int(k)] for k in keep]


class HeldOracleScan(MemoOracleScan):
    """The oracle scan with `hits`; like the device, it holds the hits of its last pass only."""

    def __init__(self, seq):
        MemoOracleScan.__init__(self, seq)
        self.generation, self.fetched = 0, 0

    def score(self, *a, **kw):
        self.generation += 1
        return MemoOracleScan.score(self, *a, **kw)

    def hits(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False):
        self.generation += 1
        idx, alns = MemoOracleScan.select(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=reverse)
        return FakeHeld(self, idx, alns, np.asarray(matrix).shape[1])

    def select(self, *a, **kw):
        raise AssertionError("a scan with `hits` is not asked to select")


class HeldOracleBackend:
    def scan(self, seq):
        return HeldOracleScan(seq)


class RecordingHeldBackend:
    """Wraps a backend whose scans offer `hits`; .log gets (kind, first, step, width, reverse, mean, sd, matrix copy, n_hits) per
    pass, a held pass under the kind "select" (what it replaces), and .kept the lists handed to frequencies / alignments."""

    def __init__(self, inner):
        self.inner, self.log, self.kept = inner, [], []

    def scan(self, seq):
        return _RecordingHeldScan(self, self.inner.scan(seq))


class _RecordingHeldScan:
    def __init__(self, owner, inner):
        self.owner, self.inner = owner, inner

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.inner.close()

    def close(self):
        self.inner.close()

    def score(self, matrix, del_, ext, first, step, width, reverse=False):
        f = self.inner.score(matrix, del_, ext, first, step, width, reverse=reverse)
        self.owner.log.append(("score", first, step, width, reverse, None, None, np.array(matrix, dtype=np.float64), len(f)))
        return f

    def hits(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False):
        h = self.inner.hits(matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=reverse)
        self.owner.log.append(("select", first, step, width, reverse, float(mean), float(sd), np.array(matrix, dtype=np.float64),
                               len(h.idx)))
        return _RecordingHeld(self.owner, h)


class _RecordingHeld:
    def __init__(self, owner, inner):
        self.owner, self.inner, self.idx, self.f = owner, inner, inner.idx, inner.f
        if hasattr(inner, "strings"):
            self.strings = self._strings

    def frequencies(self, keep):
        self.owner.kept.append(("frequencies", len(self.idx), len(keep)))
        return self.inner.frequencies(keep)

    def alignments(self, keep):
        self.owner.kept.append(("alignments", len(self.idx), len(keep)))
        return self.inner.alignments(keep)

    def _strings(self, keep):
        self.owner.kept.append(("alignments", len(self.idx), len(keep)))
        return self.inner.strings(keep)


def planted_chromosome(seed, n, rl, flip=False):
    """The chromosome of tests/test_repeats_gpu.py (restated); flip: every third planted copy is written reversed."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, n).astype(np.uint8)
    motif = rng.integers(0, 4, rl + 10).astype(np.uint8)
    for number, p in enumerate(range(500, n - rl - 200, n // 14)):
        m = motif.copy()
        mut = rng.random(len(m)) < 0.1
        m[mut] = rng.integers(0, 4, int(mut.sum()))
        s[p:p + len(m)] = m[::-1] if flip and number % 3 == 2 else m
    raw = bytearray(b"ATCG"[c] for c in s)
    raw[3000:3040] = b"N" * 40
    raw[8000:8007] = b"N" * 7
    return bytes(raw)


# (name, chromosome, options, generator seed): see the issue's list; the properties the tests need are asserted from the oracle run
def engine_cases():
    return [
        ("small", planted_chromosome(1, 12000, 60), R.Options(repeat_length=60, query_offset=10, repeats=3, reverse=True), 101),
        ("default", planted_chromosome(2, 20000, 300), R.Options(repeats=3, reverse=True), 7),
        ("flipped", planted_chromosome(1, 12000, 60, flip=True), R.Options(repeat_length=60, query_offset=10, repeats=2, reverse=True), 101),
    ]


def same_alignment(a, b):
    return (a.numbered.tolist() == b.numbered.tolist() and a.query.tolist() == b.query.tolist() and a.coords == b.coords
            and np.float64(a.f).view(np.uint64) == np.float64(b.f).view(np.uint64) and a.dim == b.dim)


def run_engine(raw, opts, seed, backend):
    return R.perform_calculation_per_sequence(opts, raw, "chr", np.random.default_rng(seed), backend)


def assert_same_engine(a, b, log_a, log_b):
    """Two engine results and pass logs, as _same_engine of tests/test_repeats_gpu.py compares them, plus every task's alignment."""
    assert list(a) == list(b)
    for key in a:
        ta, ma = a[key]
        tb, mb = b[key]
        assert [(t.left_coord, t.right_coord) for t in ta] == [(t.left_coord, t.right_coord) for t in tb], key
        assert [np.float64(t.z).view(np.uint64) for t in ta] == [np.float64(t.z).view(np.uint64) for t in tb], key
        assert np.array_equal(ma, mb), key
        for x, y in zip(ta, tb):
            assert x.alignment is not None and same_alignment(x.alignment, y.alignment), (key, x)
    assert len(log_a) == len(log_b)
    for x, y in zip(log_a, log_b):
        assert x[:5] == y[:5] and x[8] == y[8]
        assert (x[5], x[6]) == (y[5], y[6]) or (np.isnan(x[5]) and np.isnan(y[5]))
        assert np.array_equal(x[7], y[7])


def case_properties(log, result):
    """From a recorded run: (hits per forward cycle, hits of the reverse pass, tasks returned forward / reverse)."""
    fwd = [e[8] for e in log if e[0] == "select" and not e[4]]
    rev = [e[8] for e in log if e[0] == "select" and e[4]]
    return fwd, rev, len(result["direct"][0]), len(result.get("inverse", ([], None))[0])
