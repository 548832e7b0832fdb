// aln_cluster_rules.h -- grouping the nodes of an edge list (aln_cluster_edges / aln_seqset_held_cluster,
// include/aligner_hip_cluster.h): who comes first, which sequences of a held pass are nodes, and what the two rules mean.  Plain
// integer arithmetic, no HIP, so that the kernels (aln_cluster.hip), the host and a CPU test driver decide all of it the same way.
//
//   nodes       0 .. n_nodes - 1, each with a length (uint32_t; no length array: all lengths equal)
//   edges       unordered pairs {a, b}.  A self edge (a == b) joins nothing and is counted in the summary's self_edges; a pair listed
//               twice, or in both orientations, is one adjacency and is counted as often as it is listed
//   priority    u comes before v iff len[u] > len[v], or the lengths are equal and u < v.  key = len << 32 | ~index: the node with the
//               largest key of a group is the group's first in priority order (an integer max picks it)
//   components  label[v] = the smallest node number of v's connected component
//   greedy      walk the nodes in priority order: v is a representative (label[v] = v) iff no representative before it is adjacent to
//               v, else label[v] = the first representative, in priority order, adjacent to v.  One fixed labelling: it depends on
//               neither the order of the edges nor the launch geometry
//   records     one per cluster in ascending label: label, size, longest (the member first in priority order; the label itself under
//               greedy), edges (listed non-self edges with both ends in the cluster)
//   held nodes  of a held pass over a block of a sequence set: sequence v is a node iff it lies in the block's query range or in its
//               target range (an upper block: its one range); every other sequence is labelled ALN_CLUSTER_NONE and counted nowhere
#pragma once
#include <stdint.h>

#include "../../include/aligner_hip_cluster.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ALN_CLUSTER_HD __host__ __device__
#else
#define ALN_CLUSTER_HD
#endif

// the records' layouts, pinned at compile time (the style of tests/abi_harness.c)
#define ALN_CLUSTER_PIN(name, cond) typedef char aln_cluster_pin_##name[(cond) ? 1 : -1]
ALN_CLUSTER_PIN(record_size, sizeof(aln_cluster_record) == 16);
ALN_CLUSTER_PIN(record_label, __builtin_offsetof(aln_cluster_record, label) == 0);
ALN_CLUSTER_PIN(record_size_at, __builtin_offsetof(aln_cluster_record, size) == 4);
ALN_CLUSTER_PIN(record_longest, __builtin_offsetof(aln_cluster_record, longest) == 8);
ALN_CLUSTER_PIN(record_edges, __builtin_offsetof(aln_cluster_record, edges) == 12);
ALN_CLUSTER_PIN(summary_size, sizeof(aln_cluster_summary) == 48);
ALN_CLUSTER_PIN(summary_nodes, __builtin_offsetof(aln_cluster_summary, nodes) == 0);
ALN_CLUSTER_PIN(summary_clusters, __builtin_offsetof(aln_cluster_summary, clusters) == 8);
ALN_CLUSTER_PIN(summary_edges, __builtin_offsetof(aln_cluster_summary, edges) == 16);
ALN_CLUSTER_PIN(summary_self_edges, __builtin_offsetof(aln_cluster_summary, self_edges) == 24);
ALN_CLUSTER_PIN(summary_singletons, __builtin_offsetof(aln_cluster_summary, singletons) == 32);
ALN_CLUSTER_PIN(summary_rounds, __builtin_offsetof(aln_cluster_summary, rounds) == 40);
ALN_CLUSTER_PIN(summary_reserved, __builtin_offsetof(aln_cluster_summary, reserved) == 44);

#define ALN_CLUSTER_MAX 0xFFFFFFF0ull             // n_nodes and n_edges: every offset of the cluster list fits 32 bits

// does u come before v?  (u != v: a node does not come before itself)
ALN_CLUSTER_HD inline bool aln_cluster_before(uint32_t len_u, uint32_t u, uint32_t len_v, uint32_t v)
{
    return len_u > len_v || (len_u == len_v && u < v);
}

// key(u) > key(v) iff u comes before v
ALN_CLUSTER_HD inline uint64_t aln_cluster_key(uint32_t len, uint32_t index) { return ((uint64_t)len << 32) | (uint64_t)(~index); }
ALN_CLUSTER_HD inline uint32_t aln_cluster_key_index(uint64_t key) { return ~(uint32_t)key; }

// the nodes of a call: the sequences of two ranges (an edge list of its own: 0 .. n_nodes - 1 and an empty second range)
struct aln_cluster_nodes {
    uint64_t q_first, q_count, t_first, t_count;
};

ALN_CLUSTER_HD inline aln_cluster_nodes aln_cluster_nodes_all(uint64_t n_nodes)
{
    aln_cluster_nodes r;
    r.q_first = 0; r.q_count = n_nodes; r.t_first = 0; r.t_count = 0;
    return r;
}

// the held call's: the query range and the target range of the held pass's block (valid: aln_seqset_block_pairs != 0)
ALN_CLUSTER_HD inline aln_cluster_nodes aln_cluster_nodes_of_block(const aln_seqset_block &b)
{
    aln_cluster_nodes r;
    r.q_first = b.q_first; r.q_count = b.q_count; r.t_first = b.t_first; r.t_count = b.t_count;
    return r;
}

ALN_CLUSTER_HD inline bool aln_cluster_is_node(const aln_cluster_nodes &r, uint64_t v)
{
    return (v >= r.q_first && v - r.q_first < r.q_count) || (v >= r.t_first && v - r.t_first < r.t_count);
}

// how many: the two ranges' sizes less what they share
ALN_CLUSTER_HD inline uint64_t aln_cluster_node_count(const aln_cluster_nodes &r)
{
    const uint64_t q_end = r.q_first + r.q_count, t_end = r.t_first + r.t_count;
    const uint64_t lo = r.q_first > r.t_first ? r.q_first : r.t_first;
    const uint64_t hi = q_end < t_end ? q_end : t_end;
    return r.q_count + r.t_count - (hi > lo ? hi - lo : 0u);
}
