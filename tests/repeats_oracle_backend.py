"""Scoring backends for the repeat-search tests: the CPU oracle window by window (orc.align_pwm), and a recorder that logs
what every pass was handed.  Not a test module (no test_ prefix): imported by tests/test_repeats_*.py."""
import numpy as np

from aligner_amd.enums import DNA
from aligner_amd.pwm import PWMAlignment


class OracleBackend:
    def scan(self, seq):
        return OracleScan(seq)


class OracleScan:
    def __init__(self, seq):
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.len = len(self.seq)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        pass

    def _windows(self, first, step, width, reverse):
        s = self.seq[::-1] if reverse else self.seq
        return [(k, s[j:min(j + width, self.len)]) for k, j in enumerate(range(first, self.len, step))]

    def _align(self, w, matrix, del_, ext):
        import oracle
        return oracle.align_pwm(w, del_, ext, matrix)

    def score(self, matrix, del_, ext, first, step, width, reverse=False):
        return np.array([self._align(w, matrix, del_, ext)["f"] for _k, w in self._windows(first, step, width, reverse)],
                        dtype=np.float64)

    def select(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False):
        m = np.asarray(matrix, dtype=np.float64)
        idx, alns = [], []
        with np.errstate(divide="ignore", invalid="ignore"):
            for k, w in self._windows(first, step, width, reverse):
                r = self._align(w, m, del_, ext)
                if (np.float64(r["f"]) - np.float64(mean)) / np.float64(sd) >= z_min:
                    idx.append(k)
                    alns.append(PWMAlignment(DNA, r["numbered"], r["qal"], m.shape[1], r["coords"], r["f"]))
        return np.array(idx, dtype=np.int64), alns


class RecordingBackend:
    """Wraps a backend; .log gets (kind, first, step, width, reverse, mean, sd, matrix copy, n_hits) per pass."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def scan(self, seq):
        return _RecordingScan(self, self.inner.scan(seq))


class _RecordingScan:
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

    def select(self, matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=False):
        idx, alns = self.inner.select(matrix, del_, ext, first, step, width, mean, sd, z_min, reverse=reverse)
        self.owner.log.append(("select", first, step, width, reverse, float(mean), float(sd), np.array(matrix, dtype=np.float64),
                               len(idx)))
        return idx, alns
