"""The rule of aln_seqset_held_report / aln_seqset_held_filter (aligner_amd/csrc/aln_report_rules.h) restated in numpy, and the
constructed cases the CPU and the GPU tests of it share.  Nothing here touches the library under test."""
import numpy as np

SKIP_SEED = 1
BLANK = 98
RECORD = np.dtype([("columns", "<u4"), ("identical", "<u4"), ("positive", "<u4"), ("mismatch", "<u4"), ("q_gap", "<u4"), ("t_gap", "<u4"),
                   ("q_gap_open", "<u4"), ("t_gap_open", "<u4"), ("status", "<i4"), ("reserved", "<u4")])
IDENTICAL, POSITIVE, MISMATCH, Q_GAP, T_GAP, BOTH_BLANK = range(6)


def classes(qa, ta, matrix, blank=BLANK):
    """class of every column of the two aligned strings"""
    x = np.asarray(qa, dtype=np.int64)
    y = np.asarray(ta, dtype=np.int64)
    m = np.asarray(matrix, dtype=np.float64)
    xb, yb = x == blank, y == blank
    both = ~xb & ~yb
    inside = both & (x < m.shape[1]) & (y < m.shape[0])
    pos = np.zeros(len(x), dtype=bool)
    with np.errstate(invalid="ignore"):
        pos[inside] = m[y[inside], x[inside]] >= 0.0            # (a NaN compares false)
    out = np.full(len(x), MISMATCH, dtype=np.int64)
    out[both & pos] = POSITIVE
    out[both & (x == y)] = IDENTICAL
    out[xb & ~yb] = Q_GAP
    out[yb & ~xb] = T_GAP
    out[xb & yb] = BOTH_BLANK
    return out


def report(qa, ta, matrix, flags=0, status=0, blank=BLANK):
    """the record of one held entry with aligned strings qa / ta (their whole aln_len)"""
    r = np.zeros((), dtype=RECORD)
    r["status"] = status
    if status != 0:
        return r
    n = len(qa)
    if (flags & SKIP_SEED) and n:
        n -= 1
    c = classes(qa[:n], ta[:n], matrix, blank)
    r["columns"] = n
    for name, k in (("identical", IDENTICAL), ("positive", POSITIVE), ("mismatch", MISMATCH), ("q_gap", Q_GAP), ("t_gap", T_GAP)):
        r[name] = int((c == k).sum())
    prev = np.concatenate([[-1], c[:-1]]) if n else c
    r["q_gap_open"] = int(((c == Q_GAP) & (prev != Q_GAP)).sum())
    r["t_gap_open"] = int(((c == T_GAP) & (prev != T_GAP)).sum())
    return r


def reports(strings, matrix, flags=0, statuses=None, blank=BLANK):
    out = np.zeros(len(strings), dtype=RECORD)
    for i, (qa, ta) in enumerate(strings):
        out[i] = report(qa, ta, matrix, flags, 0 if statuses is None else int(statuses[i]), blank)
    return out


def keep(rep, q_len, t_len, min_identity=0.0, min_q_cover=0.0, min_t_cover=0.0, min_columns=0):
    """the filter's rule on an array of records: float64 products, each rounded on its own, plain compares (a NaN keeps nothing)"""
    rep = np.asarray(rep, dtype=RECORD)
    cols = rep["columns"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (rep["status"] == 0) & (rep["columns"] >= np.uint32(min_columns))
        ok &= rep["identical"].astype(np.float64) >= np.float64(min_identity) * cols
        ok &= (rep["columns"] - rep["q_gap"]).astype(np.float64) >= np.float64(min_q_cover) * np.asarray(q_len, dtype=np.float64)
        ok &= (rep["columns"] - rep["t_gap"]).astype(np.float64) >= np.float64(min_t_cover) * np.asarray(t_len, dtype=np.float64)
    return ok


# ---------------------------------------------------------------- the constructed cases (Protein codes; BLOSUM62, 11 / 2)
# aln_len of the lengths case.  An aln_len of 1 does not exist: the traceback seeds both strings with the end cell's pair and the walk
# emits at least that cell again (a single W against a single W: aln_len 2), and a pair without a positive cell fails with
# ALN_ERR_NO_POSITIVE_CELL and is never held -- the CPU test shows both with the oracle.  One counted column is LENGTHS[0] with SKIP_SEED.
LENGTHS = [2, 63, 64, 65, 66, 128, 129, 130]
CORE = "ACDEFHIKLMNQRSTVY"                              # no W, no G: the flanks' and the inserts' residues


def _core(rng, n):
    return "".join(rng.choice(list(CORE), n))


def _codes(s):
    from aligner_amd.enums import Protein
    return Protein.str_to_vec(s)


def lengths_case(rng, matrix):
    """[(query, target)]: pair i aligns locally (11 / 2) with aln_len LENGTHS[i], every column an identical one: an exact self-match
    between the flanks WWW (query) and GGG (target), which score -2 against each other and <= 0 ... -4 against the core's residues.
    How the reference's walk ends at such a core's first cell depends on the core (it stops there, or runs on through cells of
    score 0 to the border, emitting blanks), so cores are drawn until the CPU oracle gives the wanted aln_len without a blank."""
    import oracle
    out = []
    for n in LENGTHS:
        for attempt in range(200):
            L = n - (attempt % 3)
            if L < 1:
                continue
            core = _core(rng, L)
            q, t = "WWW" + core + "WWW", "GGG" + core + "GGG"
            o = oracle.align(oracle.CORE_LOCAL, _codes(q), _codes(t), 11, 2, matrix)
            if o["status"] == 0 and len(o["qa"]) == n and (classes(o["qa"], o["ta"], matrix) == IDENTICAL).all():
                out.append((q, t))
                break
        else:
            raise AssertionError("no core gives aln_len %d" % n)
    return out


def seam_case(rng):
    """[(query, target)] x 2.  Pair 0: 60 shared residues, 10 W only the query has, 60 shared residues: target blanks in columns
    60 .. 69, a run that covers columns 63 and 64.  Pair 1: 64 shared residues, 3 W only the target has, 60 shared: query blanks in
    columns 64 .. 66, a run that starts at column 64."""
    a, b = _core(rng, 60), _core(rng, 60)
    c, d = _core(rng, 64), _core(rng, 60)
    return [(a + "W" * 10 + b, a + b), (c + d, c + "WWW" + d)]


def small_set(matrix, seed=20260):
    """(sequences as strings, {name: (q, t) sequence numbers}): the lengths and seam cases interleaved so that every constructed
    pair is (q < t), plus random proteins of 1 .. 150 residues; about 40 sequences"""
    rng = np.random.default_rng(seed)
    seqs, where = [], {}
    for i, (q, t) in enumerate(lengths_case(rng, matrix)):
        where["len%d" % LENGTHS[i]] = (len(seqs), len(seqs) + 1)
        seqs += [q, t]
    for i, (q, t) in enumerate(seam_case(rng)):
        where["seam%d" % i] = (len(seqs), len(seqs) + 1)
        seqs += [q, t]
    letters = list("ARNDCQEGHILKMFPSTWYV")
    for n in [1, 2, 3, 5, 17, 31, 63, 64, 65, 97, 127, 128, 129, 149, 150, 40, 77, 111]:
        seqs.append("".join(rng.choice(letters, n)))
    return seqs, where


TILE_N = 80                                               # 3160 pairs of the upper triangle: tiles 0 and 1 of the selection
TILE_MIX = 0.6                                            # min_identity of the mixed filter


def upper_pair(n, k):
    """(q, t) of pair k of the upper triangle of n sequences, generate_pairs order"""
    q = 0
    while k >= n - 1 - q:
        k -= n - 1 - q
        q += 1
    return q, q + 1 + k


def tile_set(seed=4711):
    """TILE_N random proteins of 12 .. 40 residues; the sequences of held positions 2047 and 2048 (core global with f_min = 0 holds
    every pair of the upper triangle) are copies of one another with one residue changed, so that a min_identity of TILE_MIX keeps
    both while random pairs fall below it"""
    rng = np.random.default_rng(seed)
    letters = list("ARNDCQEGHILKMFPSTWYV")
    seqs = ["".join(rng.choice(letters, int(rng.integers(12, 41)))) for _ in range(TILE_N)]
    (q0, t0), (q1, t1) = upper_pair(TILE_N, 2047), upper_pair(TILE_N, 2048)
    base = "".join(rng.choice(letters, 30))
    for j, s in enumerate(sorted({q0, t0, q1, t1})):
        v = list(base)
        v[3 + 5 * j] = "W" if v[3 + 5 * j] != "W" else "Y"
        seqs[s] = "".join(v)
    return seqs
