"""The rule of aln_seqset_held_profiles (include/aligner_hip_profile.h, aligner_amd/csrc/aln_profile_rules.h) restated in plain Python
over arrays of strings, summaries, endpoints and labels: which held hits contribute to which centre, where a column lies on the centre
and which row it is counted in.  With the set's sequences it also asserts the premise of the position rule: every non-blank of a
centre's string is the set's residue at the position the rule assigns."""
import numpy as np

NONE = 0xFFFFFFFF
OK = 0
SKIP_SEED = 1
COUNTS, SELF, BETWEEN, UNLISTED, SKIP = "counts", "self_pairs", "between_members", "unlisted", None
SUMMARY_KEYS = ("held", "contributing", "self_pairs", "between_members", "unlisted", "overflow", "elements")


def counted_columns(aln_len, flags):
    return aln_len - 1 if (flags & SKIP_SEED) and aln_len > 0 else aln_len


def kind_of(q, t, label, centers):
    """(kind, centre) of an OK (and kept) hit"""
    if q == t:
        return SELF, None
    if label[q] != label[t] or label[q] == NONE:
        return SKIP, None
    ends = [v for v in (q, t) if v == label[q]]
    if len(ends) != 1:
        return BETWEEN, None
    return (COUNTS if ends[0] in centers else UNLISTED), ends[0]


def row_of(mc, blank, n_codes):
    if mc < n_codes:
        return mc
    return n_codes if mc == blank else n_codes + 1


def positions(center_string, start, aln_len, flags, blank):
    """[(column, position)] of the counted columns whose centre code is not blank"""
    n = counted_columns(aln_len, flags)
    out, seen = [], 0
    for j in range(n):
        if center_string[j] == blank:
            continue
        seed = not (flags & SKIP_SEED) and j == aln_len - 1
        out.append((j, start + seen - (1 if seed and seen else 0)))
        seen += 1
    return out


def layout(lengths, centers, n_codes):
    offsets, total = [], 0
    for c in centers:
        offsets.append(total)
        total += (n_codes + 2) * int(lengths[c])
    return offsets, total


def profiles(q, t, summaries, strings, label, centers, lengths, n_codes, blank, flags, kept=None, seqs=None):
    """q, t: the held hits' endpoints; summaries: their records (status, aln_len, start_x, start_y by name); strings: [(aligned query,
    aligned target)]; kept: the held positions a filter keeps (None: no filter).  Returns (out, records, summary): the flat uint32
    profiles, [(center, hits, matched, deleted)] and the summary dict."""
    centers = [int(c) for c in centers]
    slot = {c: i for i, c in enumerate(centers)}
    offsets, total = layout(lengths, centers, n_codes)
    out = np.zeros(total, dtype=np.uint32)
    rec = [[c, 0, 0, 0] for c in centers]
    summ = dict.fromkeys(SUMMARY_KEYS, 0)
    summ["held"], summ["elements"] = len(q), total
    keep = None if kept is None else set(int(k) for k in kept)
    for h in range(len(q)):
        r = summaries[h]
        if int(r["status"]) != OK or (keep is not None and h not in keep):
            continue
        kind, c = kind_of(int(q[h]), int(t[h]), label, slot)
        if kind is SKIP:
            continue
        if kind != COUNTS:
            summ[kind] += 1
            continue
        summ["contributing"] += 1
        i = slot[c]
        rec[i][1] += 1
        qs, ts = strings[h]
        c_is_q = int(q[h]) == c
        cs, ms = (qs, ts) if c_is_q else (ts, qs)
        start = int(r["start_x"]) if c_is_q else int(r["start_y"])
        ln = int(lengths[c])
        view = out[offsets[i]:offsets[i] + (n_codes + 2) * ln].reshape(n_codes + 2, ln)
        for j, pos in positions(cs, start, int(r["aln_len"]), flags, blank):
            if pos >= ln:
                summ["overflow"] += 1
                continue
            if seqs is not None:
                assert int(cs[j]) == int(seqs[c][pos]), ("the centre's string does not lie where the rule puts it", h, j, pos)
            row = row_of(int(ms[j]), blank, n_codes)
            view[row, pos] += 1
            rec[i][2] += row < n_codes
            rec[i][3] += row == n_codes
    return out, [tuple(int(x) for x in r) for r in rec], summ


def from_held(held, labels, centers, n_codes, blank=98, skip_seed=True, kept=None, check_premise=True):
    """the reference over a HeldHits: strings and summaries from held.strings(), endpoints from the held list"""
    o = held.owner
    res, strs = held.strings()
    seqs = [o.seqs[int(a):int(a) + int(n)] for a, n in zip(o.off, o.len)]
    return profiles(held.q, held.t, res, strs, [int(x) for x in labels], centers, o.len, n_codes, blank, SKIP_SEED if skip_seed else 0, kept,
                    seqs if check_premise else None)
