"""CIGARs of a sequence set's held hits, run-length encoded on the device (aln_seqset_held_cigar_plan / _fill,
include/aligner_hip_cigar.h).

Per listed hit a handful of 32-bit words `length << 4 | op` in SAM's numbering (the words are BAM's) and a 32-byte record with the
coordinates, the match count and the block length beside them: what a PAF line or a SAM record needs.  The traceback's duplicated seed
column is never part of a CIGAR (aligner_amd/csrc/aln_cigar_rules.h).  HeldHits.cigars (aligner_amd/seqset.py) makes a Cigars; encode
and decode are the same rule and its inverse on the host, in plain numpy.
"""
import numpy as np

from . import _ffi

RECORD_DTYPE = np.dtype([("n_ops", "<u4"), ("q_start", "<u4"), ("q_end", "<u4"), ("t_start", "<u4"), ("t_end", "<u4"), ("matches", "<u4"),
                         ("block", "<u4"), ("status", "<i4")])
assert RECORD_DTYPE.itemsize == 32
CIGAR_RECORD_DTYPE = RECORD_DTYPE
SUMMARY_KEYS = ("held", "listed", "total_ops", "failed", "padded", "overflow")
# aln_strand_record (include/aligner_hip_strand.h): strand is ord("+") or ord("-")
STRAND_DTYPE = np.dtype([("q_rec", "<u4"), ("t_rec", "<u4"), ("strand", "u1"), ("q_mirror", "u1"), ("t_mirror", "u1"), ("reserved", "u1"),
                         ("reserved2", "<u4")])
assert STRAND_DTYPE.itemsize == 16
EXTENDED, CLIPS = _ffi.CIGAR_EXTENDED, _ffi.CIGAR_CLIPS
M, I, D, S, P, EQ, X = 0, 1, 2, 4, 6, 7, 8
OP_CHARS = "MIDNSHP=X"
MAX_RUN = (1 << 28) - 1
CONSUMES_QUERY = (M, I, S, EQ, X)
CONSUMES_TARGET = (M, D, EQ, X)


def summary_dict(s):
    return {k: int(getattr(s, k)) for k in SUMMARY_KEYS}


def text_of(ops):
    """`57M2D3M` of the words."""
    return "".join("%d%s" % (int(w) >> 4, OP_CHARS[int(w) & 15]) for w in ops)


def encode(query_str, target_str, blank=98, flags=0, start_x=0, start_y=0, q_len=None, status=0, skip_seed=True):
    """The rule on the host: (record as a RECORD_DTYPE scalar, words as uint32, P columns, overflow 0 | 1) of the two aligned strings
    as held.strings() returns them.  skip_seed: the strings end with the traceback's seed column, which is left out.  q_len: the
    query's length, for the trailing clip of CLIPS (default: no residues behind the alignment)."""
    if flags & ~(EXTENDED | CLIPS):
        raise ValueError("cigar.encode: unknown flag bits")
    rec = np.zeros((), dtype=RECORD_DTYPE)
    rec["status"] = status
    if status != _ffi.OK:
        return rec, np.zeros(0, dtype=np.uint32), 0, 0
    x = np.asarray(query_str, dtype=np.uint8)
    y = np.asarray(target_str, dtype=np.uint8)
    n = min(len(x), len(y))
    if skip_seed and n:
        n -= 1
    x, y = x[:n], y[:n]
    xb, yb = x == blank, y == blank
    op = np.full(n, M, dtype=np.uint32)
    if flags & EXTENDED:
        op[:] = np.where(x == y, EQ, X)
    op[yb] = I
    op[xb] = D
    op[xb & yb] = P
    first = np.flatnonzero(np.concatenate([[True], op[1:] != op[:-1]])) if n else np.zeros(0, dtype=np.int64)
    length = np.diff(np.concatenate([first, [n]]))
    words = [(int(l) << 4) | int(o) for l, o in zip(length, op[first])]
    q_end, t_end = int(start_x) + int((~xb).sum()), int(start_y) + int((~yb).sum())
    N = q_end if q_len is None else int(q_len)
    overflow = 0
    if flags & CLIPS:
        if start_x:
            words.insert(0, (min(int(start_x), MAX_RUN) << 4) | S)
        if q_end > N:
            overflow = 1
        elif N - q_end:
            words.append((min(N - q_end, MAX_RUN) << 4) | S)
    pads = int((xb & yb).sum())
    rec["n_ops"], rec["q_start"], rec["q_end"], rec["t_start"], rec["t_end"] = len(words), start_x, min(q_end, 0xFFFFFFFF), start_y, min(t_end, 0xFFFFFFFF)
    rec["matches"], rec["block"] = int(((x == y) & ~xb).sum()), n - pads
    return rec, np.array(words, dtype=np.uint32), pads, overflow


def mirror(residues, table):
    """The mirror of a record as a stranded set holds it: table[residues[::-1]]."""
    return np.asarray(table, dtype=np.uint8)[np.asarray(residues, dtype=np.uint8)[::-1]]


def decode(ops, q_residues, t_residues, q_start, t_start, blank=98, reversed_target=False):
    """The two aligned strings (uint8, without the seed column) the words stand for over the two sequences: the inverse of encode.
    Clips stand for residues outside the strings and move nothing; a P column is blank in both.  reversed_target: the words are those
    of a stranded plan's hit on a mirrored target (StrandRecord.t_mirror), which stand in reverse order; the residues and the starts
    are still those of the records that were aligned -- mirror() of an original record, N - q_end and M - t_end of the stranded
    coordinates where a side is mirrored."""
    q_residues = np.asarray(q_residues, dtype=np.uint8)
    t_residues = np.asarray(t_residues, dtype=np.uint8)
    qs, ts, q, t = [], [], int(q_start), int(t_start)
    words = np.asarray(ops, dtype=np.uint32)
    for w in (words[::-1] if reversed_target else words).tolist():
        n, op = w >> 4, w & 15
        if op == S:
            continue
        if op not in (M, I, D, P, EQ, X):
            raise ValueError("cigar.decode: op %d" % op)
        if op in CONSUMES_QUERY:
            if q + n > len(q_residues):
                raise ValueError("cigar.decode: the words consume more than the query has")
            qs.append(q_residues[q:q + n])
            q += n
        else:
            qs.append(np.full(n, blank, dtype=np.uint8))
        if op in CONSUMES_TARGET:
            if t + n > len(t_residues):
                raise ValueError("cigar.decode: the words consume more than the target has")
            ts.append(t_residues[t:t + n])
            t += n
        else:
            ts.append(np.full(n, blank, dtype=np.uint8))
    empty = np.zeros(0, dtype=np.uint8)
    return (np.concatenate(qs) if qs else empty), (np.concatenate(ts) if ts else empty)


class Cigars:
    """.records: RECORD_DTYPE, one per listed hit (n_ops, q_start, q_end, t_start, t_end, matches, block, status); .summary: dict of
    held, listed, total_ops, failed, padded, overflow; .offsets: uint64, len + 1 word offsets; .words: every hit's words, uint32;
    .which: the listed held positions.  Of a stranded plan (HeldHits.cigars(stranded=True)) also .strands (STRAND_DTYPE) and its
    columns .q_rec, .t_rec (the original records) and .strand ("+" / "-" as uint8 codes); None otherwise."""

    def __init__(self, which, records, summary, offsets, words, flags=0, strands=None):
        self.which, self.records, self.summary, self.offsets, self.words, self.flags = which, records, summary, offsets, words, int(flags)
        self.strands = strands
        self.q_rec = None if strands is None else strands["q_rec"]
        self.t_rec = None if strands is None else strands["t_rec"]
        self.strand = None if strands is None else strands["strand"]

    def __len__(self):
        return len(self.records)

    def ops(self, i):
        """The uint32 view of listed hit i's words."""
        return self.words[int(self.offsets[i]):int(self.offsets[i + 1])]

    def text(self, i):
        return text_of(self.ops(i))

    def paf(self, i, q_name, q_len, t_name, t_len, f):
        """Listed hit i as a PAF line (no newline): the 12 standard columns -- the strand it holds, + when it holds none, mapping quality
        255 -- then af:f: and cg:Z:.  Of a stranded plan the names and lengths are those of records q_rec[i] and t_rec[i]."""
        r = self.records[i]
        strand = "+" if self.strand is None else chr(int(self.strand[i]))
        return "\t".join([str(q_name), str(int(q_len)), str(int(r["q_start"])), str(int(r["q_end"])), strand, str(t_name), str(int(t_len)),
                          str(int(r["t_start"])), str(int(r["t_end"])), str(int(r["matches"])), str(int(r["block"])), "255",
                          "af:f:%r" % float(f), "cg:Z:%s" % self.text(i)])
