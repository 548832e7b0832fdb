"""Pure-Python restatement of the shuffled copies of aln_shuffle_scores / aln_shuffle_targets (aln_shuffle_rules.h), written from
the specification, not from the header: SplitMix64 per copy, Lemire's bounded draw with rejection, the trim as the first draw,
then Fisher-Yates in the order of rand 0.8's SliceRandom::shuffle."""
import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


class Stream:
    def __init__(self, seed, pair, s):
        self.state = (seed ^ ((pair * 0xD1B54A32D192ED03) & M64) ^ (((s + 1) * 0xABC98388FB8FAC03) & M64)) & M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def bounded(self, n):
        assert 1 <= n < (1 << 32)
        m = (self.next() >> 32) * n
        if (m & M32) < n:
            t = ((1 << 32) - n) % n
            while (m & M32) < t:
                m = (self.next() >> 32) * n
        return m >> 32


def copy_of(target, seed, pair, s, max_trim):
    """(trim, copy) of copy s of stream pair `pair` (= pair_base + i)."""
    r = Stream(seed, pair, s)
    trim = r.bounded(max_trim + 1)
    a = list(int(v) for v in target[:len(target) - trim])
    for k in range(len(a) - 1, 0, -1):
        j = r.bounded(k + 1)
        a[k], a[j] = a[j], a[k]
    return trim, np.array(a, dtype=np.uint8)


def trims(seed, pair, per_pair, max_trim):
    return np.array([Stream(seed, pair, s).bounded(max_trim + 1) for s in range(per_pair)], dtype=np.int64)


def copies(target, seed, pair, per_pair, max_trim, sample=None):
    """{s: copy} for s in `sample` (default: every copy)."""
    idx = range(per_pair) if sample is None else sample
    return {s: copy_of(target, seed, pair, s, max_trim)[1] for s in idx}
