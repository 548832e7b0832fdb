"""The seed join's rule in Python dictionaries and integers (include/aligner_hip_seedjoin.h states it in words); nothing here is taken
from aligner_amd/csrc/aln_seedjoin_rules.h, which tests/test_seedjoin_rules_cpu.py holds against this file."""
import bisect
from collections import Counter

MAX_K = 16
MAX_WORDS = 1 << 32
MAX_BAND = (1 << 31) - 1
CHUNK_SEEDS = 1 << 24
MAX_CHUNK_SEEDS = 1 << 26
MAX_CHUNK_PAIRS = 1 << 32


def n_word_numbers(k, a):
    """A^k, or 0 where (k, A) is refused."""
    if not 1 <= k <= MAX_K or a < 1 or a ** k > MAX_WORDS:
        return 0
    return a ** k


def word(window, a):
    """The number of a window (a sequence of k codes), or None if it touches a code >= A."""
    n = 0
    for c in window:
        c = int(c)
        if c >= a:
            return None
        n = n * a + c
    return n


def positions(seq, k, a):
    """{word: [pos, ...]} of one record: every window that is a word, positions ascending."""
    seq = [int(c) for c in seq]
    out = {}
    for i in range(len(seq) - k + 1):
        w = word(seq[i:i + k], a)
        if w is not None:
            out.setdefault(w, []).append(i)
    return out


def occurrences(seqs, k, a):
    """[(word, seq, pos)] of the whole set, ascending: the resident list P."""
    return sorted((w, s, p) for s, seq in enumerate(seqs) for w, ps in positions(seq, k, a).items() for p in ps)


def dropped_words(tables, max_occ):
    """The words with more than max_occ occurrences over all records; max_occ == 0 drops nothing."""
    if not max_occ:
        return set()
    total = Counter()
    for t in tables:
        for w, ps in t.items():
            total[w] += len(ps)
    return {w for w, n in total.items() if n > max_occ}


def sort_key(rel_pair, d):
    """(pair number in the chunk) << 32 | (d + 2^31)"""
    assert -(1 << 31) <= d < (1 << 31)
    return rel_pair << 32 | (d + (1 << 31))


def best_window(diags, band):
    """(seeds, diag) of one pair out of the multiset of its seeds' diagonals (not empty): the most seeds with d0 <= d <= d0 + band
    over the diagonals d0 that occur, and the least d0 that reaches it."""
    ds = sorted(diags)
    best, at = 0, None
    for d0 in sorted(set(ds)):
        c = bisect.bisect_right(ds, d0 + band) - bisect.bisect_left(ds, d0)
        if c > best:
            best, at = c, d0
    return best, at


def block_pairs(block):
    """[(q, t)] of a block (q_first, q_count, t_first, t_count, upper) in the block's order."""
    qf, qc, tf, tc, up = block
    if up:
        return [(qf + i, qf + j) for i in range(qc) for j in range(i + 1, qc)]
    return [(qf + i, tf + j) for i in range(qc) for j in range(tc)]


def pair_diagonals(tq, tt, drop):
    """The diagonals pt - pq of every seed of one pair, from the two records' position tables."""
    out = []
    small, big = (tq, tt) if len(tq) <= len(tt) else (tt, tq)
    for w in small:
        if w in big and w not in drop:
            for pq in tq[w]:
                for pt in tt[w]:
                    out.append(pt - pq)
    return out


def row_pairs(block, first, n):
    """pairs of query rows first .. first + n - 1 of a block"""
    qf, qc, tf, tc, up = block
    if up:
        return sum(qc - 1 - r for r in range(first, first + n)) if n < 1000 else \
            (first + n) * (2 * qc - (first + n) - 1) // 2 - first * (2 * qc - first - 1) // 2
    return n * tc


def cut(seeds, cap, block=None):
    """[(first row, rows)] of the chunks: the longest runs of whole rows within the cap whose pairs together are at most 2^32; None if
    a single row is above the cap."""
    out, first = [], 0
    while first < len(seeds):
        if seeds[first] > cap:
            return None
        n, total = 0, 0
        while first + n < len(seeds) and total + seeds[first + n] <= cap and (n == 0 or block is None or row_pairs(block, first, n + 1) <= MAX_CHUNK_PAIRS):
            total += seeds[first + n]
            n += 1
        out.append((first, n))
        first += n
    return out


def seed_join(seqs, k, a, min_seeds=1, band=0, max_occ=0, block=None, chunk_seeds=0):
    """((index, q, t, seeds, diag) lists of the candidates of a block, ascending in pair number; the summary as a dict; the seeds per
    query row).  summary["chunks"] is None where a row is above the cap (the call is ALN_ERR_CAPACITY)."""
    assert min_seeds >= 1 and 0 <= band <= MAX_BAND
    n = len(seqs)
    block = (0, n, 0, n, 1) if block is None else block
    tables = [positions(s, k, a) for s in seqs]
    drop = dropped_words(tables, max_occ)
    out = ([], [], [], [], [])
    rows = [0] * block[1]
    total = with_seed = 0
    for idx, (q, t) in enumerate(block_pairs(block)):
        ds = pair_diagonals(tables[q], tables[t], drop)
        if not ds:
            continue
        total += len(ds)
        with_seed += 1
        rows[q - block[0]] += len(ds)
        seeds, diag = best_window(ds, band)
        if seeds >= min_seeds:
            for lst, v in zip(out, (idx, q, t, seeds, diag)):
                lst.append(v)
    chunks = cut(rows, chunk_seeds if chunk_seeds else CHUNK_SEEDS, block)
    summary = dict(seeds=total, pairs_with_seed=with_seed, words_dropped=len(drop),
                   chunks=None if chunks is None else sum(1 for f, m in chunks if sum(rows[f:f + m])))
    return out, summary, rows
