"""Clusters of an edge list, grouped on the device (aln_cluster_edges / aln_seqset_held_cluster, include/aligner_hip_cluster.h).

Two rules over the same edge list (aligner_amd/csrc/aln_cluster_rules.h): "components" -- single linkage, label = the smallest node of
the connected component -- and "greedy" -- longest-first representatives as CD-HIT users expect them: walking the nodes by length
(longer first, equal lengths by the lower number), a node joins the first representative it shares an edge with, else it becomes a
representative itself.  HeldHits.cluster (aligner_amd/seqset.py) runs them over the held hits of a sequence set.
"""
import ctypes as C

import numpy as np

from . import _ffi
from . import runtime

RECORD_DTYPE = np.dtype([("label", "<u4"), ("size", "<u4"), ("longest", "<u4"), ("edges", "<u4")])
assert RECORD_DTYPE.itemsize == 16
NONE = _ffi.CLUSTER_NONE
MODES = {"components": _ffi.CLUSTER_COMPONENTS, "greedy": _ffi.CLUSTER_GREEDY}


def mode_code(mode):
    """"components" / "greedy" (or the C constant itself) as the C constant."""
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError("cluster mode must be one of %s" % sorted(MODES))
        return MODES[mode]
    return int(mode)


def summary_dict(s):
    return dict(nodes=int(s.nodes), clusters=int(s.clusters), edges=int(s.edges), self_edges=int(s.self_edges), singletons=int(s.singletons),
                rounds=int(s.rounds))


class Clusters:
    """.label: uint32 per node (NONE for a sequence that is not a node); .records: RECORD_DTYPE, one per cluster in ascending label (the
    first `capacity` of them); .summary: dict of nodes, clusters, edges, self_edges, singletons, rounds."""

    def __init__(self, label, records, summary):
        self.label, self.records, self.summary = label, records, summary

    def __len__(self):
        return int(self.summary["clusters"])

    def members(self):
        """The node numbers of every cluster: a list of uint32 arrays in the order of the cluster list, ascending within a cluster.
        Made here from the labels by a stable argsort (the member lists are not part of the C ABI: 4 bytes per node hold them)."""
        nodes = np.flatnonzero(self.label != NONE)
        lab = self.label[nodes]
        order = np.argsort(lab, kind="stable")
        lab, nodes = lab[order], nodes[order].astype(np.uint32)
        cuts = np.flatnonzero(lab[1:] != lab[:-1]) + 1 if len(lab) else np.zeros(0, dtype=np.int64)
        return [part for part in np.split(nodes, cuts) if len(part)]


def cluster_edges(n_nodes, a, b, lengths=None, mode="components", device=None, capacity=None):
    """aln_cluster_edges: the nodes 0 .. n_nodes - 1 grouped by the edges {a[k], b[k]} -- hits of align_batch, of a scan, or from
    anywhere -- on the device.  lengths (uint32 per node; None: all equal) decide the greedy priority and every record's `longest`.
    Returns a Clusters."""
    lib = _ffi.load()
    n = int(n_nodes)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("aln_cluster_edges: a and b are two lists of the same length")
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if lengths.shape != (n,):
            raise ValueError("aln_cluster_edges: one length per node")
    cap = n if capacity is None else int(capacity)
    label = np.zeros(n, dtype=np.uint32)
    rec = np.zeros(cap, dtype=RECORD_DTYPE)
    summ = _ffi.ClusterSummary()
    st = lib.aln_cluster_edges(runtime.context(device), mode_code(mode), n, lengths.ctypes.data if lengths is not None else None,
                               a.ctypes.data if len(a) else None, b.ctypes.data if len(b) else None, len(a), label.ctypes.data if n else None,
                               rec.ctypes.data if cap else None, cap, C.byref(summ))
    runtime.raise_for_status(st, "aln_cluster_edges")
    return Clusters(label, rec[:min(int(summ.clusters), cap)], summary_dict(summ))
