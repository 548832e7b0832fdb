"""The word join's rule in Python sets and integers (include/aligner_hip_wordjoin.h states it in words); nothing here is taken from
aligner_amd/csrc/aln_wordjoin_rules.h, which tests/test_wordjoin_rules_cpu.py holds against this file.  No bitmaps: K(s) is a set."""

MAX_K = 8
MAX_WORDS = 1 << 32
CHUNK_OCCURRENCES = 1 << 24
MAX_CHUNK_OCCURRENCES = 1 << 26


def n_word_numbers(k, a):
    """A^k, or 0 where (k, A) is refused."""
    if not 1 <= k <= MAX_K or a < 1 or a ** k > MAX_WORDS:
        return 0
    return a ** k


def bits_needed(n):
    """The least b with 2^b >= n."""
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def word(window, a):
    """The number of a window (a sequence of k codes), or None if it touches a code >= A."""
    if any(int(c) >= a for c in window):
        return None
    n = 0
    for c in window:
        n = n * a + int(c)
    return n


def words(seq, k, a):
    """K(s): the set of word numbers of s."""
    seq = [int(c) for c in seq]
    return {w for w in (word(seq[i:i + k], a) for i in range(len(seq) - k + 1)) if w is not None}


def candidate(shared, n_q, n_t, min_shared, min_per_1024):
    return shared >= min_shared and shared * 1024 >= min_per_1024 * min(n_q, n_t)


def block_pairs(block):
    """[(q, t)] of a block (q_first, q_count, t_first, t_count, upper) in the block's order."""
    qf, qc, tf, tc, up = block
    if up:
        return [(qf + i, qf + j) for i in range(qc) for j in range(i + 1, qc)]
    return [(qf + i, tf + j) for i in range(qc) for j in range(tc)]


def word_join(seqs, k, a, min_shared, min_per_1024, block):
    """(index, q, t, shared) lists of the candidates of a block, ascending in pair number; min_shared >= 1."""
    assert min_shared >= 1
    sets = [words(s, k, a) for s in seqs]
    out = ([], [], [], [])
    for idx, (q, t) in enumerate(block_pairs(block)):
        sh = len(sets[q] & sets[t])
        if sh and candidate(sh, len(sets[q]), len(sets[t]), min_shared, min_per_1024):
            for lst, v in zip(out, (idx, q, t, sh)):
                lst.append(v)
    return out


def row_occurrences(seqs, k, a, block):
    """Per query row of the block: the sum over its targets of shared(q, t) -- the occurrences the join expands for that row."""
    sets = [words(s, k, a) for s in seqs]
    qf, qc, tf, tc, up = block
    occ = [0] * qc
    for q, t in block_pairs(block):
        occ[q - qf] += len(sets[q] & sets[t])
    return occ


def cut(occ, cap):
    """[(first row, rows)] of the chunks: the longest runs of whole rows within the cap; None if a single row is above it."""
    out, first = [], 0
    while first < len(occ):
        if occ[first] > cap:
            return None
        n, total = 0, 0
        while first + n < len(occ) and total + occ[first + n] <= cap:
            total += occ[first + n]
            n += 1
        out.append((first, n))
        first += n
    return out
