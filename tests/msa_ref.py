"""The rule of aln_seqset_held_msa_plan / _fill (include/aligner_hip_msa.h, aligner_amd/csrc/aln_msa_rules.h) restated in plain Python
over arrays of strings, summaries, endpoints and labels: which held hits contribute to which centre (profile_ref.kind_of), how wide the
insert before every centre position is, where every column of a hit lies in its family's matrix, and the rows.  Also the properties a
family alignment has by construction, asserted from this file's own output."""
import numpy as np

import profile_ref as P

NONE = P.NONE
OK = P.OK
SUMMARY_KEYS = ("held", "contributing", "self_pairs", "between_members", "unlisted", "overflow", "bytes", "total_rows")


def counted_columns(aln_len):
    """the seed column is never part of a family alignment"""
    return aln_len - 1 if aln_len > 0 else 0


def walk(center_string, start, aln_len, blank):
    """[(column of the hit, 'r' | 'i', centre position p, k)] of the counted columns: a residue column at p, or the k-th column of the
    insert run before p"""
    out, seen, run = [], 0, 0
    for j in range(counted_columns(aln_len)):
        if center_string[j] != blank:
            out.append((j, "r", start + seen, 0))
            seen += 1
            run = 0
        else:
            out.append((j, "i", start + seen, run))
            run += 1
    return out


def measure(center_string, start, aln_len, blank, len_c, ins):
    """max the hit's runs into ins (len_c + 1 entries); returns its overflow columns"""
    over = 0
    for _j, what, p, k in walk(center_string, start, aln_len, blank):
        if what == "r":
            over += p >= len_c
        elif p > len_c:
            over += 1
        else:
            ins[p] = max(ins[p], k + 1)
    return over


def columns(ins):
    """col[p] for p in 0 .. len_c (col[len_c] is the width)"""
    col, total = [], 0
    for p, w in enumerate(ins):
        total += w
        col.append(p + total)
    return col


def member_row(center_string, member_string, start, aln_len, blank, len_c, ins, col, width):
    row = np.full(width, blank, dtype=np.uint8)
    for j, what, p, k in walk(center_string, start, aln_len, blank):
        if what == "r":
            if p < len_c:
                row[col[p]] = member_string[j]
        elif p <= len_c and k < ins[p]:
            row[col[p] - ins[p] + k] = member_string[j]
    return row


def alignments(q, t, summaries, strings, label, centers, lengths, seqs, blank, kept=None):
    """q, t: the held hits' endpoints; summaries: their records (status, aln_len, start_x, start_y by name); strings: [(aligned query,
    aligned target)]; seqs: the set's sequences; kept: the held positions a filter keeps (None: no filter).  Returns (matrices, row
    lists, records, summary): per centre the (rows + 1) x width uint8 matrix and the held positions of its rows (NONE first),
    [(center, rows, width, inserted)] and the summary dict."""
    centers = [int(c) for c in centers]
    slot = {c: i for i, c in enumerate(centers)}
    summ = dict.fromkeys(SUMMARY_KEYS, 0)
    summ["held"] = len(q)
    keep = None if kept is None else set(int(k) for k in kept)
    mine = [[] for _ in centers]                      # per centre: (held position, centre string, member string, start, aln_len), ascending
    for h in range(len(q)):
        r = summaries[h]
        if int(r["status"]) != OK or (keep is not None and h not in keep):
            continue
        kind, c = P.kind_of(int(q[h]), int(t[h]), label, slot)
        if kind is P.SKIP:
            continue
        if kind != P.COUNTS:
            summ[kind] += 1
            continue
        summ["contributing"] += 1
        qs, ts = strings[h]
        c_is_q = int(q[h]) == c
        cs, ms = (qs, ts) if c_is_q else (ts, qs)
        mine[slot[c]].append((h, cs, ms, int(r["start_x"]) if c_is_q else int(r["start_y"]), int(r["aln_len"])))
    mats, lists, recs = [], [], []
    for i, c in enumerate(centers):
        len_c = int(lengths[c])
        ins = [0] * (len_c + 1)
        for _h, cs, _ms, start, aln_len in mine[i]:
            summ["overflow"] += measure(cs, start, aln_len, blank, len_c, ins)
        col = columns(ins)
        width = col[len_c]
        assert width == len_c + sum(ins)
        m = np.full((len(mine[i]) + 1, width), blank, dtype=np.uint8)
        for p in range(len_c):
            m[0, col[p]] = seqs[c][p]
        for r, (_h, cs, ms, start, aln_len) in enumerate(mine[i]):
            m[r + 1] = member_row(cs, ms, start, aln_len, blank, len_c, ins, col, width)
        mats.append(m)
        lists.append([NONE] + [h for h, *_rest in mine[i]])
        recs.append((c, len(mine[i]), width, width - len_c))
        summ["bytes"] += m.size
        summ["total_rows"] += m.shape[0]
    return mats, lists, recs, summ


def flat(mats, lists):
    """the two output buffers of the fill"""
    out = np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0, dtype=np.uint8)
    return out.astype(np.uint8), np.array([h for l in lists for h in l], dtype=np.uint32)


def check_properties(mats, lists, recs, q, t, summaries, strings, seqs, blank):
    """what a family alignment is, asserted on the reference's own output (for strings that are the set's own: overflow 0, no column
    with a blank on both sides)"""
    for m, rows, (c, n_rows, width, inserted) in zip(mats, lists, recs):
        assert m.shape == (n_rows + 1, width) and inserted == width - len(seqs[c]) and rows[0] == NONE and rows[1:] == sorted(rows[1:])
        assert m[0][m[0] != blank].tolist() == [int(x) for x in seqs[c]], "row 0 without its blanks is the centre"
        assert (m != blank).any(axis=0).all(), "every column has a non-blank somewhere"
        for r, h in enumerate(rows[1:], start=1):
            c_is_q = int(q[h]) == c
            member = int(t[h]) if c_is_q else int(q[h])
            n = counted_columns(int(summaries[h]["aln_len"]))
            cs, ms = (strings[h][0][:n], strings[h][1][:n]) if c_is_q else (strings[h][1][:n], strings[h][0][:n])
            m_start = int(summaries[h]["start_y"]) if c_is_q else int(summaries[h]["start_x"])
            span = int((np.asarray(ms) != blank).sum())
            assert m[r][m[r] != blank].tolist() == [int(x) for x in seqs[member][m_start:m_start + span]], "a row without its blanks is the member's span"
            # the projection of rows 0 and r onto the columns where either is non-blank, between the first and the last column the
            # hit has in the family (row 0 goes on beyond them: the centre's flanks), is the hit's two strings
            c_start = int(summaries[h]["start_x"]) if c_is_q else int(summaries[h]["start_y"])
            col0 = np.flatnonzero(m[0] != blank)
            ends = np.flatnonzero(m[r] != blank).tolist()
            residues = int((np.asarray(cs) != blank).sum())
            if residues:
                ends += [int(col0[c_start]), int(col0[c_start + residues - 1])]
            at = np.arange(width)
            inside = ((m[0] != blank) | (m[r] != blank)) & (at >= min(ends)) & (at <= max(ends)) if ends else np.zeros(width, dtype=bool)
            assert m[0][inside].tolist() == [int(x) for x in cs], "the centre's string"
            assert m[r][inside].tolist() == [int(x) for x in ms], "the member's string"


def from_held(held, labels, centers, blank=98, kept=None):
    """the reference over a HeldHits: strings and summaries from held.strings(), endpoints from the held list"""
    o = held.owner
    res, strs = held.strings()
    seqs = [o.seqs[int(a):int(a) + int(n)] for a, n in zip(o.off, o.len)]
    mats, lists, recs, summ = alignments(held.q, held.t, res, strs, [int(x) for x in labels], centers, o.len, seqs, blank, kept)
    return mats, lists, recs, summ, (res, strs, seqs)
