"""The rule of aln_seqset_held_cigar_plan / _fill (include/aligner_hip_cigar.h, aligner_amd/csrc/aln_cigar_rules.h) restated in plain
Python, one column at a time: the op of a column, the runs, the clips, the record, the offsets and the summary -- and the inverse, the two
strings a list of words stands for, which is the round trip the tests use."""
import numpy as np

OK = 0
EXTENDED, CLIPS = 1, 2
M, I, D, S, P, EQ, X = 0, 1, 2, 4, 6, 7, 8
MAX_RUN = (1 << 28) - 1
U32 = 0xFFFFFFFF
RECORD_KEYS = ("n_ops", "q_start", "q_end", "t_start", "t_end", "matches", "block", "status")
SUMMARY_KEYS = ("held", "listed", "total_ops", "failed", "padded", "overflow")


def counted_columns(aln_len):
    """the seed column is never part of a CIGAR"""
    return aln_len - 1 if aln_len > 0 else 0


def op_of(x, y, blank, flags):
    if x == blank and y == blank:
        return P
    if x == blank:
        return D
    if y == blank:
        return I
    if not flags & EXTENDED:
        return M
    return EQ if x == y else X


def word(length, op):
    return (min(length, MAX_RUN) << 4) | op


def encode(query, target, aln_len, status, start_x, start_y, N, blank, flags):
    """(record as a tuple in RECORD_KEYS order, [words], P columns, overflow) of one held entry"""
    assert not flags & ~(EXTENDED | CLIPS)
    if status != OK:
        return (0, 0, 0, 0, 0, 0, 0, status), [], 0, 0
    n = counted_columns(aln_len)
    runs = []                                         # [op, length]
    q_res = t_res = matches = pads = 0
    for j in range(n):                                # (column n, the seed column, is never looked at)
        x, y = int(query[j]), int(target[j])
        op = op_of(x, y, blank, flags)
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
        q_res += x != blank
        t_res += y != blank
        matches += x == y and x != blank
        pads += op == P
    q_end, t_end = min(start_x + q_res, U32), min(start_y + t_res, U32)
    words = [word(length, op) for op, length in runs]
    overflow = 0
    if flags & CLIPS:
        if start_x:
            words.insert(0, word(start_x, S))
        if q_end > N:
            overflow = 1
        elif N - q_end:
            words.append(word(N - q_end, S))
    return (len(words), start_x, q_end, start_y, t_end, matches, n - pads, OK), words, pads, overflow


def offsets(records):
    off, at = [], 0
    for r in records:
        off.append(at)
        at += r[0]
    return off + [at]


def consumed(words):
    """(query residues, target residues) the runs consume; clips consume nothing of the alignment"""
    q = sum(w >> 4 for w in words if w & 15 in (M, I, EQ, X))
    t = sum(w >> 4 for w in words if w & 15 in (M, D, EQ, X))
    return q, t


def decode(words, q_residues, t_residues, q_start, t_start, blank):
    """the two aligned strings without the seed column"""
    qs, ts, q, t = [], [], q_start, t_start
    for w in words:
        n, op = w >> 4, w & 15
        if op == S:
            continue
        assert op in (M, I, D, P, EQ, X), op
        for _ in range(n):
            if op in (M, I, EQ, X):
                qs.append(int(q_residues[q]))
                q += 1
            else:
                qs.append(blank)
            if op in (M, D, EQ, X):
                ts.append(int(t_residues[t]))
                t += 1
            else:
                ts.append(blank)
    return qs, ts


def text(words):
    return "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words)


def listed(entries, which, held, blank, flags):
    """entries: per held position (query string, target string, aln_len, status, start_x, start_y, N).  Returns (records, offsets, words
    of all listed hits, summary dict)."""
    recs, words = [], []
    summ = dict.fromkeys(SUMMARY_KEYS, 0)
    summ["held"], summ["listed"] = held, len(which)
    for h in which:
        rec, w, pads, over = encode(*entries[int(h)], blank, flags)
        recs.append(rec)
        words += w
        summ["failed"] += rec[7] != OK
        summ["padded"] += pads
        summ["overflow"] += over
    off = offsets(recs)
    summ["total_ops"] = off[-1]
    assert len(words) == off[-1]
    return recs, off, words, summ


def entries_of(held, blank=98):
    """per held position (query string, target string, aln_len, status, start_x, start_y, N) from held.strings(), and (summaries,
    strings, sequences).  Asserts on the way that the i-th non-blank of a string is the set's residue start + i -- the start_x /
    start_y convention profile_ref and msa_ref rely on."""
    o = held.owner
    res, strs = held.strings()
    seqs = [o.seqs[int(a):int(a) + int(n)] for a, n in zip(o.off, o.len)]
    entries = []
    for h in range(len(held)):
        qs, ts = strs[h]
        r = res[h]
        q, t = int(held.q[h]), int(held.t[h])
        if int(r["status"]) == OK:
            n = counted_columns(int(r["aln_len"]))
            for string, seq, start in ((qs, seqs[q], int(r["start_x"])), (ts, seqs[t], int(r["start_y"]))):
                own = [int(c) for c in string[:n] if int(c) != blank]
                assert own == [int(c) for c in seq[start:start + len(own)]], "the i-th non-blank of a string is the set's residue start + i"
        entries.append((qs, ts, int(r["aln_len"]), int(r["status"]), int(r["start_x"]), int(r["start_y"]), int(o.len[q])))
    return entries, (res, strs, seqs)


def from_held(held, which=None, flags=0, blank=98):
    """the reference over a HeldHits.  Returns (records, offsets, words, summary, (summaries, strings, sequences))."""
    entries, more = entries_of(held, blank)
    which = list(range(len(held))) if which is None else [int(h) for h in which]
    recs, off, words, summ = listed(entries, which, len(held), blank, flags)
    return recs, off, words, summ, more
