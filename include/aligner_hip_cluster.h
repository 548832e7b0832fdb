/*
 * aligner_hip_cluster.h -- the clustering family of the C ABI: grouping the nodes of an edge list, and the sequences of a resident
 * sequence set by its held hits, on the device.  A companion of aligner_hip.h (which it includes): the symbols live in the same
 * libaligner_hip.so, under the same ALN_ABI_VERSION.
 *
 * Why a second header: the project's tests pin the main header's list of functions and records (their number, the mirror lists of
 * the bindings, the C99 callers).  This family was added without moving those yardsticks, so it brings its own header, its own
 * mirror list (_ffi.CLUSTER_EXPORTS) and its own C99 caller (tests/abi_cluster.c); a Rust mirror belongs in a module of its own
 * (cluster.rs) beside lib.rs.  A change that may move the pins can fold the two headers together; nothing else separates them.
 *
 * aligner_amd/csrc/aln_cluster_rules.h is the rule as code.  In words:
 *   nodes       0 .. n_nodes - 1, each with a length (node_len; null: all lengths equal)
 *   edges       unordered pairs {edge_a[k], edge_b[k]}.  A self edge joins nothing and is counted in summary->self_edges.  A pair
 *               listed twice, or in both orientations, is one adjacency, counted as often as it is listed
 *   priority    u comes before v iff len[u] > len[v], or the lengths are equal and u < v
 *   ALN_CLUSTER_COMPONENTS   single linkage: label[v] = the smallest node number of v's connected component
 *   ALN_CLUSTER_GREEDY       longest-first representatives: walking the nodes in priority order, v is a representative
 *               (label[v] = v) iff no representative before it is adjacent to v, else label[v] = the first representative, in
 *               priority order, adjacent to v
 * Both are total rules: one fixed labelling, independent of the order of the edges and of anything the device does in parallel.
 * label (n_nodes words) always comes back in full.  clusters receives the first `capacity` records of the cluster list, which is in
 * ascending label; summary->clusters is the true count also beyond capacity, and the call returns ALN_OK.  summary->rounds: the edge
 * rounds the device ran (components: at most n_nodes + 2, in practice about log2 of the longest path of trees; greedy: at most the
 * longest priority-descending chain of the graph plus one).
 *
 * aln_cluster_edges: any edge list in host arrays.  Up: 8 bytes per edge, 4 per node with lengths.  Down: 4 bytes per node, 16 per
 * written record, the counters.  n_nodes == 0: ALN_OK, everything zero.  ALN_ERR_INVALID_ARGUMENT, nothing written: a null ctx or
 * summary, an unknown mode, a null pointer with a non-zero length, an endpoint >= n_nodes (checked before anything is queued),
 * n_nodes or n_edges above 0xFFFFFFF0.
 *
 * aln_seqset_held_cluster: the sequences of a set grouped by its held hits (of aln_seqset_hits or aln_seqset_best).
 *   nodes       the sequences in the query range or in the target range of the held pass's block; node numbers are sequence numbers,
 *               lengths the sequences' own.  Every other sequence gets ALN_CLUSTER_NONE and is counted nowhere
 *   edges       the held hits with status ALN_OK, joining their q and t.  With a filter: ALL held hits are reported into the set's
 *               buffer as aln_seqset_held_filter does, and an edge is a hit that filter keeps (params and flags as there).  With a
 *               null filter every ALN_OK held hit is an edge, no report pass runs, params and flags are ignored
 * The endpoints of the held hits go up (8 bytes per held hit; with a filter the bit table too); 4 bytes per sequence, 16 per written
 * record and the counters come down.  The held summaries, strings and list are not written: held_list, held_strings, held_report,
 * held_filter and held_significance answer afterwards as before.  stats: ms[2] this call's kernels, ms[3] its wall time, bytes[] as
 * above; ms[0] and ms[1] stay the held pass's.
 * Refused as aln_seqset_held_filter refuses (with a filter); in addition ALN_ERR_INVALID_ARGUMENT for an unknown mode and a null
 * label or summary.  A refused call leaves the held state and the outputs as they were.
 */
#ifndef ALIGNER_HIP_CLUSTER_H
#define ALIGNER_HIP_CLUSTER_H
#include "aligner_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ALN_CLUSTER_COMPONENTS 0u
#define ALN_CLUSTER_GREEDY 1u
#define ALN_CLUSTER_NONE 0xFFFFFFFFu      /* the label of a sequence that is not a node */

typedef struct aln_cluster_record {
    uint32_t label;        /* the smallest member (components), the representative (greedy) */
    uint32_t size;         /* members                                                        */
    uint32_t longest;      /* the member first in priority order (== label under greedy)     */
    uint32_t edges;        /* listed non-self edges with both ends in this cluster           */
} aln_cluster_record;      /* 16 bytes */

typedef struct aln_cluster_summary {
    uint64_t nodes;        /* offset  0                                                      */
    uint64_t clusters;     /* offset  8: the true count, also beyond capacity                */
    uint64_t edges;        /* offset 16: listed edges that are not self edges                */
    uint64_t self_edges;   /* offset 24                                                      */
    uint64_t singletons;   /* offset 32: clusters of one node                                */
    uint32_t rounds;       /* offset 40: edge rounds run on the device                       */
    uint32_t reserved;     /* offset 44: 0                                                   */
} aln_cluster_summary;     /* 48 bytes */

int aln_cluster_edges(aln_ctx *ctx, uint32_t mode, uint64_t n_nodes, const uint32_t *node_len /* optional */,
                      const uint32_t *edge_a, const uint32_t *edge_b, uint64_t n_edges,
                      uint32_t *label /* n_nodes */, aln_cluster_record *clusters /* optional */, uint64_t capacity,
                      aln_cluster_summary *summary);
int aln_seqset_held_cluster(aln_seqset *set, const aln_params *params, uint32_t flags, const aln_hit_filter *filter /* optional */,
                            uint32_t mode, uint32_t *label /* n_seqs */, aln_cluster_record *clusters /* optional */,
                            uint64_t capacity, aln_cluster_summary *summary);

#ifdef __cplusplus
}
#endif
#endif
