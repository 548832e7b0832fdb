"""The k-mer prefilter's rule in Python sets and integers (include/aligner_hip_prefilter.h states it in words); nothing here is taken
from aligner_amd/csrc/aln_prefilter_rules.h, which tests/test_prefilter_rules_cpu.py holds against this file."""

MAX_K = 8
MAX_BITS = 1 << 18


def bits(k, a):
    """A^k, or 0 where (k, A) is refused."""
    if not 1 <= k <= MAX_K or a < 1 or a ** k > MAX_BITS:
        return 0
    return a ** k


def word(window, a):
    """The number of a window (a sequence of k codes), or None if it touches a code >= A."""
    if any(c >= a for c in window):
        return None
    n = 0
    for c in window:
        n = n * a + int(c)
    return n


def words(seq, k, a):
    """K(s): the set of word numbers of s."""
    seq = [int(c) for c in seq]
    out = set()
    for i in range(len(seq) - k + 1):
        w = word(seq[i:i + k], a)
        if w is not None:
            out.add(w)
    return out


def bitmap(ws, k, a):
    """(A^k + 31) // 32 elements of 32 bits: word w is bit w & 31 of element w >> 5."""
    out = [0] * ((a ** k + 31) // 32)
    for w in ws:
        out[w >> 5] |= 1 << (w & 31)
    return out


def candidate(shared, n_q, n_t, min_shared, min_per_1024):
    return shared >= min_shared and shared * 1024 >= min_per_1024 * min(n_q, n_t)


def block_pairs(block):
    """[(q, t)] of a block (q_first, q_count, t_first, t_count, upper) in the block's order."""
    qf, qc, tf, tc, up = block
    if up:
        return [(qf + i, qf + j) for i in range(qc) for j in range(i + 1, qc)]
    return [(qf + i, tf + j) for i in range(qc) for j in range(tc)]


def prefilter(seqs, k, a, min_shared, min_per_1024, block):
    """(index, q, t, shared) lists of the candidates of a block, ascending in pair number."""
    sets = [words(s, k, a) for s in seqs]
    out = ([], [], [], [])
    for idx, (q, t) in enumerate(block_pairs(block)):
        sh = len(sets[q] & sets[t])
        if candidate(sh, len(sets[q]), len(sets[t]), min_shared, min_per_1024):
            for lst, v in zip(out, (idx, q, t, sh)):
                lst.append(v)
    return out
