"""The rule of a stranded sequence set (include/aligner_hip_strand.h, aligner_amd/csrc/aln_strand_rules.h) restated in plain Python: where
the mirrors lie and what they hold, which strand a hit is on, its coordinates on the original records, where a word of its CIGAR goes --
and the way back, the aligned strings a stranded hit's words stand for, from the original records alone.  The plain plan it builds on is
cigar_ref's."""
import numpy as np

import cigar_ref as R

TILE = 4096
SLACK = 256
PLUS, MINUS = ord("+"), ord("-")
STRAND_KEYS = ("q_rec", "t_rec", "strand", "q_mirror", "t_mirror")


def mirror(rec, table):
    """mirror[j] = table[rec[len - 1 - j]]"""
    rec = [int(c) for c in rec]
    return [int(table[rec[len(rec) - 1 - j]]) for j in range(len(rec))]


def layout(lengths):
    """(off of the 2n records, total of the n, bytes of the residue buffer)"""
    off, at = [], 0
    for n in lengths:
        off.append(at)
        at += int(n)
    return off + [at + o for o in off], at, 2 * at + SLACK


def count_ok(n):
    return 2 * n < 2 ** 32


def tiles(total):
    return (total + TILE - 1) // TILE


def record_at(off, lengths, p):
    """the record that holds residue position p of the packed buffer"""
    for i, (a, n) in enumerate(zip(off, lengths)):
        if a <= p < a + n:
            return i
    raise AssertionError("no record holds %d" % p)


def classify(q_seq, t_seq, n):
    qm, tm = int(q_seq >= n), int(t_seq >= n)
    return (q_seq % n, t_seq % n, MINUS if qm != tm else PLUS, qm, tm)


def flip(length, start, end):
    return length - end, length - start


def record(plain, strand, N, M):
    """the stranded record of a plain one (both tuples in cigar_ref.RECORD_KEYS order)"""
    n_ops, q_start, q_end, t_start, t_end, matches, block, status = plain
    if status != R.OK:
        return plain
    if strand[3]:
        q_start, q_end = flip(N, q_start, q_end)
    if strand[4]:
        t_start, t_end = flip(M, t_start, t_end)
    return (n_ops, q_start, q_end, t_start, t_end, matches, block, status)


def word_pos(r, n_ops, reversed_):
    return n_ops - 1 - r if reversed_ else r


def words(plain_words, strand):
    out = [None] * len(plain_words)
    for r, w in enumerate(plain_words):
        out[word_pos(r, len(plain_words), bool(strand[4]))] = w
    return out


def listed(entries, pairs, lengths, which, n, held, blank, flags):
    """entries: cigar_ref.listed's, per held position; pairs: per held position (q_seq, t_seq) of the 2n; lengths: of the 2n.  Returns
    (records, strand records, offsets, words of all listed hits, summary)."""
    recs, off, _w, summ = R.listed(entries, which, held, blank, flags)
    out_recs, strands, out_words = [], [], []
    for h in which:
        h = int(h)
        plain, w, _p, _o = R.encode(*entries[h], blank, flags)
        s = classify(pairs[h][0], pairs[h][1], n)
        strands.append(s)
        out_recs.append(record(plain, s, int(lengths[pairs[h][0]]), int(lengths[pairs[h][1]])))
        out_words += words(w, s)
    assert [r[0] for r in out_recs] == [r[0] for r in recs]
    return out_recs, strands, off, out_words, summ


def decode(hit_words, rec, strand, originals, table, blank):
    """The two aligned strings (without the seed column) of a stranded hit from its words, its stranded record and strand record and
    the n original records: a mirrored side is aligned as mirror(original), from the start the flip of its coordinates gives back."""
    q = originals[strand[0]]
    t = originals[strand[1]]
    q_start, t_start = rec[1], rec[3]
    if strand[3]:
        q, (q_start, _e) = mirror(q, table), flip(len(q), rec[1], rec[2])
    if strand[4]:
        t, (t_start, _e) = mirror(t, table), flip(len(t), rec[3], rec[4])
    plain = list(hit_words)[::-1] if strand[4] else list(hit_words)
    return R.decode(plain, q, t, q_start, t_start, blank)


def mirrors_numpy(records, table):
    table = np.asarray(table, dtype=np.uint8)
    return [table[np.asarray(r, dtype=np.uint8)[::-1]] for r in records]
