"""Profiles of a sequence set's families, counted on the device (aln_seqset_held_profiles, include/aligner_hip_profile.h).

For every centre -- the representative a clustering names, or any sequence the caller labels a family with -- and every residue
position of it: how often each residue code, a deletion or any other code of the family's members is aligned to it in the held hits
(aligner_amd/csrc/aln_profile_rules.h).  The sequence-against-sequence analogue of PWMAlignment.get_frequency_matrix.
HeldHits.profiles (aligner_amd/seqset.py) makes a Profiles.
"""
import numpy as np

from . import _ffi

RECORD_DTYPE = np.dtype([("center", "<u4"), ("hits", "<u4"), ("matched", "<u4"), ("deleted", "<u4")])
assert RECORD_DTYPE.itemsize == 16
SUMMARY_KEYS = ("held", "contributing", "self_pairs", "between_members", "unlisted", "overflow", "elements")


def summary_dict(s):
    return {k: int(getattr(s, k)) for k in SUMMARY_KEYS}


def default_centers(labels):
    """The labels that have at least one other member: ascending sequence numbers v with labels[v] == v and some w != v with
    labels[w] == v."""
    labels = np.asarray(labels, dtype=np.uint32)
    n = len(labels)
    inside = labels[labels < n].astype(np.int64)
    size = np.bincount(inside, minlength=n) if n else np.zeros(0, dtype=np.int64)
    own = labels == np.arange(n, dtype=np.uint32)
    return np.flatnonzero(own & (size >= 2)).astype(np.uint32)


def layout(lengths, centers, n_codes):
    """(offsets, total): the first element of every centre's profile, and the elements in all."""
    sizes = (int(n_codes) + 2) * np.asarray(lengths, dtype=np.uint64)[np.asarray(centers, dtype=np.int64)] if len(centers) else np.zeros(0, dtype=np.uint64)
    offsets = np.zeros(len(sizes), dtype=np.uint64)
    if len(sizes) > 1:
        offsets[1:] = np.cumsum(sizes)[:-1]
    return offsets, int(sizes.sum())


class Profiles:
    """.centers: uint32 sequence numbers, ascending; .records: RECORD_DTYPE, one per centre (center, hits, matched, deleted);
    .summary: dict of held, contributing, self_pairs, between_members, unlisted, overflow, elements; .counts(i): profile i."""

    def __init__(self, centers, lengths, codes, n_codes, out, records, summary):
        self.centers, self.n_codes, self.records, self.summary = centers, int(n_codes), records, summary
        self.lengths = np.asarray(lengths, dtype=np.uint64)[centers.astype(np.int64)] if len(centers) else np.zeros(0, dtype=np.uint64)
        self.offsets, total = layout(lengths, centers, n_codes)
        self.out = out
        self._codes = codes               # i -> the centre's own residue codes

    def __len__(self):
        return len(self.centers)

    def counts(self, i):
        """The (n_codes + 2) x len view of profile i: rows 0 .. n_codes - 1 the residue codes, row n_codes deletions, row
        n_codes + 1 every other code."""
        a, ln = int(self.offsets[i]), int(self.lengths[i])
        return self.out[a:a + (self.n_codes + 2) * ln].reshape(self.n_codes + 2, ln)

    def frequency(self, i, with_center=True):
        """The residue rows of profile i as float64 (n_codes x len); with_center adds 1 at the centre's own residue of every position
        (a code at or beyond n_codes adds nothing).  Host numpy."""
        f = self.counts(i)[:self.n_codes].astype(np.float64)
        if with_center:
            own = np.asarray(self._codes(i), dtype=np.int64)
            pos = np.flatnonzero(own < self.n_codes)
            f[own[pos], pos] += 1.0
        return f


def labels_of(labels):
    """An array, or a cluster.Clusters, as the uint32 label array."""
    return np.ascontiguousarray(getattr(labels, "label", labels), dtype=np.uint32)


def check_codes(n_codes):
    if not 1 <= int(n_codes) <= _ffi.PROFILE_MAX_CODES:
        raise ValueError("aln_seqset_held_profiles: n_codes must lie in 1 .. %d" % _ffi.PROFILE_MAX_CODES)
    return int(n_codes)
