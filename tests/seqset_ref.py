"""Pure-Python restatement of aligner_amd/csrc/aln_seqset_rules.h: the pair order of a block of the S x S grid of a sequence set.
Written from the rule, not from the header: the upper order is the literal double loop of generate_pairs (aligner-web
dispatcher/handlers.rs:253-264), the closed forms use Python's unbounded integers."""


def block_pairs(n_seqs, q_first, q_count, t_first, t_count, upper, reserved=0):
    if reserved != 0 or upper not in (0, 1):
        return 0
    if q_first + q_count > n_seqs or t_first + t_count > n_seqs:
        return 0
    if upper:
        if q_first != t_first or q_count != t_count:
            return 0
        return q_count * (q_count - 1) // 2
    return q_count * t_count


def generate_pairs(first, n):
    """for (i, rec) in sequences.iter().enumerate() { for ord in sequences[i + 1..] { push((rec, ord)) } }"""
    out = []
    for i in range(n):
        for j in range(i + 1, n):
            out.append((first + i, first + j))
    return out


def rectangle_pairs(q_first, q_count, t_first, t_count):
    return [(q_first + a, t_first + b) for a in range(q_count) for b in range(t_count)]


def row_start(n, r):
    """pairs in front of row r: rows 0 .. r - 1 hold n - 1, n - 2, .. pairs"""
    return sum_first_rows(n, r)


def sum_first_rows(n, r):
    return r * (n - 1) - r * (r - 1) // 2


def upper_unrank(first, n, k):
    """By the closed form with exact integers: the largest r with row_start(r) <= k (math.isqrt, no floating point)."""
    import math
    # rows after r hold (n - 1 - r)(n - r) / 2 ... solve from the end: pairs left from k on
    left = n * (n - 1) // 2 - k                 # >= 1
    m = (1 + math.isqrt(8 * left - 7)) // 2      # the smallest m with m (m + 1) / 2 >= left  <=>  row r = n - 1 - m
    while m * (m + 1) // 2 < left:
        m += 1
    while m > 1 and (m - 1) * m // 2 >= left:
        m -= 1
    r = n - 1 - m
    return first + r, first + r + 1 + (k - row_start(n, r))


def upper_rank(first, n, q, t):
    return row_start(n, q - first) + (t - q - 1)
