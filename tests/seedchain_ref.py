"""The seed chain's rule in Python sets and integers (include/aligner_hip_seedchain.h states it in words); nothing here is taken from
aligner_amd/csrc/aln_seedchain_rules.h, which tests/test_seedchain_rules_cpu.py holds against this file.

chain_plain is the rule word for word over the SET of anchors, every j against every i.  chain is the same result found faster (the
anchors sorted, the candidates of an i cut out by its pq range, numpy over them) for the pairs of many thousand anchors; the CPU tests
hold the two against each other."""
import bisect

import numpy as np

import seedjoin_ref as SJ

MAX_GAP = (1 << 31) - 1
MAX_SKEW = (1 << 31) - 1
MAX_GAP_SCALE = 255
PAIR_SEEDS = 1 << 16
MAX_PAIR_SEEDS = 1 << 20
CHUNK_ANCHORS = 1 << 24
MAX_CHUNK_ANCHORS = 1 << 26
OVERFLOW = 1
FIELDS = ("score", "anchors", "q_start", "q_end", "t_start", "t_end", "seeds", "flags")
RECORD = np.dtype([("score", "<i4")] + [(name, "<u4") for name in FIELDS[1:]])


def spec_ok(max_gap=1000, max_skew=200, gap_scale=2, max_pair_seeds=0, chunk_anchors=0, flags=0, reserved=(0, 0, 0)):
    """Is a spec's own part in range (k, alphabet and max_occ are the seed index's and the seed join's business)."""
    if not 1 <= max_gap <= MAX_GAP or not 0 <= max_skew <= MAX_SKEW or not 0 <= gap_scale <= MAX_GAP_SCALE:
        return False
    if not 0 <= max_pair_seeds <= MAX_PAIR_SEEDS or not 0 <= chunk_anchors <= MAX_CHUNK_ANCHORS or flags or any(reserved):
        return False
    return (max_pair_seeds or PAIR_SEEDS) <= (chunk_anchors or CHUNK_ANCHORS)


def pair_anchors(tq, tt, drop=()):
    """The set of anchors (pq, pt) of one pair from the two records' position tables (seedjoin_ref.positions)."""
    out = set()
    for w, pqs in tq.items():
        if w in tt and w not in drop:
            out.update((pq, pt) for pq in pqs for pt in tt[w])
    return out


def none_record(a, max_pair_seeds):
    if a > (max_pair_seeds or PAIR_SEEDS):
        return (0, 0, 0, 0, 0, 0, min(a, 0xFFFFFFFF), OVERFLOW)
    return (0,) * 8


def chain_plain(anchors, k, max_gap, max_skew, gap_scale, max_pair_seeds=0):
    """The record of one pair, as a tuple in FIELDS order, from the set of its anchors."""
    anchors = set(anchors)
    a = len(anchors)
    if a == 0 or a > (max_pair_seeds or PAIR_SEEDS):
        return none_record(a, max_pair_seeds)
    f, count, start = {}, {}, {}
    for i in sorted(anchors):                      # (any order that takes an anchor after everything with a smaller pq)
        best = None
        for j in anchors:
            dq, dt = i[0] - j[0], i[1] - j[1]
            if dq <= 0 or dt <= 0 or dq > max_gap or dt > max_gap or abs(dt - dq) > max_skew:
                continue
            v = f[j] + min(dq, dt, k) - ((abs(dt - dq) * gap_scale) >> 4)
            if v > k and (best is None or (v, j) > best):
                best = (v, j)
        if best is None:
            f[i], count[i], start[i] = k, 1, i
        else:
            f[i], count[i], start[i] = best[0], count[best[1]] + 1, start[best[1]]
    assert max(f.values()) <= k << 20
    e = min(anchors, key=lambda x: (-f[x], x))
    return (f[e], count[e], start[e][0], e[0] + k, start[e][1], e[1] + k, a, 0)


def chain(anchors, k, max_gap, max_skew, gap_scale, max_pair_seeds=0):
    """chain_plain's record, for large sets."""
    a = len(set(anchors))
    if a == 0 or a > (max_pair_seeds or PAIR_SEEDS):
        return none_record(a, max_pair_seeds)
    if a <= 64:
        return chain_plain(anchors, k, max_gap, max_skew, gap_scale, max_pair_seeds)
    s = sorted(set(anchors))
    pq = np.array([x[0] for x in s], dtype=np.int64)
    pt = np.array([x[1] for x in s], dtype=np.int64)
    f = np.zeros(a, dtype=np.int64)
    count = np.zeros(a, dtype=np.int64)
    start = np.zeros(a, dtype=np.int64)
    pql = pq.tolist()
    for i in range(a):
        lo, hi = bisect.bisect_left(pql, pql[i] - max_gap, 0, i), bisect.bisect_left(pql, pql[i], 0, i)
        f[i], count[i], start[i] = k, 1, i
        if lo == hi:
            continue
        dq, dt = pq[i] - pq[lo:hi], pt[i] - pt[lo:hi]
        dd = np.abs(dt - dq)
        v = f[lo:hi] + np.minimum(np.minimum(dq, dt), k) - ((dd * gap_scale) >> 4)
        v = np.where((dt > 0) & (dt <= max_gap) & (dd <= max_skew) & (v > k), v, -1)
        j = len(v) - 1 - int(np.argmax(v[::-1]))           # the slice ascends in (pq, pt): of equal v the last is the greatest
        if v[j] > k:
            f[i], count[i], start[i] = v[j], count[lo + j] + 1, start[lo + j]
    assert int(f.max()) <= k << 20
    e = int(np.argmax(f))                                   # the first of equal f: the least (pq, pt)
    b = int(start[e])
    return (int(f[e]), int(count[e]), int(pq[b]), int(pq[e]) + k, int(pt[b]), int(pt[e]) + k, a, 0)


def keep(rec, min_score, min_span=0):
    score, _n, qs, qe, ts, te, _a, flags = rec
    return bool(flags & OVERFLOW) or (score >= min_score and min(qe - qs, te - ts) >= min_span)


def records(recs):
    """A list of record tuples as the structured array the library's records are."""
    out = np.zeros(len(recs), dtype=RECORD)
    for i, r in enumerate(recs):
        out[i] = r
    return out


def chains(seqs, k, a, pairs, max_gap=1000, max_skew=200, gap_scale=2, max_occ=0, max_pair_seeds=0):
    """(the record tuples of the (q, t) in `pairs`, the summary's anchors / with_anchor / overflowed)."""
    tables = [SJ.positions(s, k, a) for s in seqs]
    drop = SJ.dropped_words(tables, max_occ)
    out, total, with_anchor, over = [], 0, 0, 0
    for q, t in pairs:
        anc = pair_anchors(tables[q], tables[t], drop)
        rec = chain(anc, k, max_gap, max_skew, gap_scale, max_pair_seeds)
        out.append(rec)
        with_anchor += bool(anc)
        over += bool(rec[7] & OVERFLOW)
        total += 0 if rec[7] & OVERFLOW else len(anc)
    return out, dict(anchors=total, with_anchor=with_anchor, overflowed=over)


def cut(per_candidate, cap):
    """[(first, n)] of the chunks that hold an anchor: the longest runs of whole candidates within the cap; None if one alone is above
    it."""
    got = SJ.cut(list(per_candidate), cap)
    return None if got is None else [(f, n) for f, n in got if sum(per_candidate[f:f + n])]


def paf_line(q_head, q_len, t_head, t_len, rec, k, minus=False):
    """The approximate PAF line of a kept candidate.  minus: t is a mirror, rec's t coordinates are the mirror's and the line's are the
    original record's: [t_len - t_end, t_len - t_start)."""
    score, n, qs, qe, ts, te = rec[:6]
    if minus:
        ts, te = t_len - te, t_len - ts
    short, long_ = min(qe - qs, te - ts), max(qe - qs, te - ts)
    return "%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcs:i:%d\tcn:i:%d" % (
        q_head, q_len, qs, qe, "-" if minus else "+", t_head, t_len, ts, te, min(n * k, short), long_, score, n)
