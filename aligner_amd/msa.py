"""Family alignments of a sequence set, merged on the device (aln_seqset_held_msa_plan / _fill, include/aligner_hip_msa.h).

For every centre -- the representative a clustering names, or any sequence the caller labels a family with -- one matrix of residue
codes: row 0 the centre, one row per held hit between the centre and a member of its family, all in one set of columns, the members'
inserts included (a centre-star alignment; aligner_amd/csrc/aln_msa_rules.h).  HeldHits.msa (aligner_amd/seqset.py) makes a
FamilyAlignments.
"""
import numpy as np

from . import _ffi

RECORD_DTYPE = np.dtype([("center", "<u4"), ("rows", "<u4"), ("width", "<u4"), ("inserted", "<u4")])
assert RECORD_DTYPE.itemsize == 16
SUMMARY_KEYS = ("held", "contributing", "self_pairs", "between_members", "unlisted", "overflow", "bytes", "total_rows")


def summary_dict(s):
    return {k: int(getattr(s, k)) for k in SUMMARY_KEYS}


def layout(records):
    """(byte offsets, row offsets, bytes, total rows) of the families of `records`."""
    rows = records["rows"].astype(np.uint64) + np.uint64(1)
    sizes = rows * records["width"].astype(np.uint64)
    byte_off = np.zeros(len(records), dtype=np.uint64)
    row_off = np.zeros(len(records), dtype=np.uint64)
    if len(records) > 1:
        byte_off[1:] = np.cumsum(sizes)[:-1]
        row_off[1:] = np.cumsum(rows)[:-1]
    return byte_off, row_off, int(sizes.sum()), int(rows.sum())


class FamilyAlignments:
    """.centers: uint32 sequence numbers, ascending; .records: RECORD_DTYPE, one per centre (center, rows, width, inserted); .summary:
    dict of held, contributing, self_pairs, between_members, unlisted, overflow, bytes, total_rows; .rows(i): family i's matrix."""

    def __init__(self, centers, records, summary, out, row_hit, q, t, alphabet, blank):
        self.centers, self.records, self.summary, self.out, self.row_hit = centers, records, summary, out, row_hit
        self.byte_off, self.row_off, _bytes, _rows = layout(records)
        self._q, self._t, self.alphabet, self.blank = q, t, alphabet, int(blank)

    def __len__(self):
        return len(self.centers)

    def rows(self, i):
        """The (rows + 1) x width uint8 view of family i: row 0 the centre, then the contributing hits in ascending held position."""
        a, r, w = int(self.byte_off[i]), int(self.records["rows"][i]) + 1, int(self.records["width"][i])
        return self.out[a:a + r * w].reshape(r, w)

    def hits(self, i):
        """The held positions of rows 1 .. of family i."""
        a = int(self.row_off[i])
        return self.row_hit[a + 1:a + 1 + int(self.records["rows"][i])]

    def members(self, i):
        """The sequence numbers of family i's rows, the centre first."""
        c, h = self.centers[i], self.hits(i).astype(np.int64)
        return np.concatenate([[c], np.where(self._q[h] == c, self._t[h], self._q[h])]).astype(np.uint32)

    def text(self, i):
        """Family i's rows as strings through the alphabet, `-` where a row is blank."""
        m = self.rows(i)
        return ["".join("-" if int(x) == self.blank else ch for x, ch in zip(row, self.alphabet.vec_to_str(row))) for row in m]
