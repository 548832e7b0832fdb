// aln_cluster.hip -- device side of aln_cluster_edges / aln_seqset_held_cluster (include/aligner_hip_cluster.h): the nodes of an edge
// list grouped on the device.  aln_cluster_rules.h is the rule; this file is its edge-parallel form.  One thread per edge or per
// node; every round is its own launch and stream order is all that separates rounds (no grid-wide barrier, no cooperative launch,
// no kernel that waits for another workgroup).
//
//   held edges   (held call) hit h keeps its uploaded endpoints iff its summary is ALN_OK and, with a filter, aln_report_keep keeps
//                its report; else both endpoints become ALN_CLUSTER_NONE: a dropped edge, which every kernel below passes over
//   components   hook      edge {a, b} with roots ru != rv (read from `root`, the labels as the last compress left them):
//                          atomicMin(label[max(ru, rv)], min(ru, rv)); sets the changed word.  Reading the roots from a copy makes
//                          a round's outcome -- label[r] = the smallest neighbouring root -- independent of the order of arrival
//                compress  root[v] = the end of v's chain through label (labels fall strictly along it; at most n steps)
//                settle    label[v] = root[v]
//                until a round changes nothing.  Every tree that is not the smallest among its neighbouring trees hooks in each
//                round, so the trees shrink geometrically on anything but adversarial numberings (bound: n rounds, a hook removes
//                a root and none appears)
//   greedy       states undecided / representative / member.  edge round: {a, b}, a before b: a representative and b undecided ->
//                mark[b] = 1; both undecided -> block[b] = 1 (plain stores of the one value).  node round: an undecided node with a
//                mark becomes a member, else without a block a representative; marks and blocks are cleared, the still undecided
//                counted.  Until none is undecided; then one edge pass gives each member the largest key among its adjacent
//                representatives (atomicMax of aln_cluster_key) and a node pass turns keys into labels.  A node is decided only
//                once every neighbour before it is: the fixed point is the sequential walk's result
//   finish       per node atomicAdd(size[label]), atomicMax(key[label]); per edge the counts of the summary (one atomicAdd per
//                workgroup) and atomicAdd(edges[label]) when both ends share a label; singletons counted per workgroup; the cluster
//                list by aln_select.h over the nodes (Keep: label[i] == i) -- ascending label, no atomic appends
//
// Atomics: integer min / max / add only, where the result does not depend on their order.  Every other store is a plain C++ store of a
// thread (vector memory instructions).
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_cluster_rules.h"
#include "aln_report_rules.h"
#include "aln_select.h"

#define ALN_CLUSTER_THREADS 256u
#define CLUSTER_UNDECIDED 0u
#define CLUSTER_REP 1u
#define CLUSTER_MEMBER 2u
#define CLUSTER_OUTSIDE 3u            // not a node

__device__ __forceinline__ uint64_t cluster_index() { return (uint64_t)blockIdx.x * ALN_CLUSTER_THREADS + threadIdx.x; }
__device__ __forceinline__ uint32_t cluster_len(const ClusterArgs &a, uint32_t v) { return a.len ? a.len[v] : 0u; }

// edge k of the list: false for a dropped edge, a self edge or an endpoint beyond the arrays (checked on the host; never indexed)
__device__ __forceinline__ bool cluster_edge(const ClusterArgs &a, uint64_t k, uint32_t *u, uint32_t *v)
{
    if (k >= a.m) return false;
    *u = a.ea[k]; *v = a.eb[k];
    return *u != *v && *u < a.n && *v < a.n;
}

__global__ __launch_bounds__(256) void aln_cluster_held_edges_kernel(const aln_pair_result *res, const aln_hit_report *rep, const HeldEntry *held,
                                                                     aln_hit_filter filter, uint64_t m, uint32_t *ea, uint32_t *eb)
{
    const uint64_t h = cluster_index();
    if (h >= m) return;
    bool keep = res[h].status == ALN_OK;
    if (keep && rep) keep = aln_report_keep(rep[h], filter, held[h].N, held[h].M);
    if (!keep) { ea[h] = ALN_CLUSTER_NONE; eb[h] = ALN_CLUSTER_NONE; }
}

// ---- start: labels, states and the finish's tables
__global__ __launch_bounds__(256) void aln_cluster_init_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    if (v >= a.n) return;
    const bool node = aln_cluster_is_node(a.nodes, v);
    a.label[v] = node ? (uint32_t)v : ALN_CLUSTER_NONE;
    a.aux0[v] = node ? (a.mode == ALN_CLUSTER_GREEDY ? CLUSTER_UNDECIDED : (uint32_t)v) : (a.mode == ALN_CLUSTER_GREEDY ? CLUSTER_OUTSIDE : ALN_CLUSTER_NONE);
    if (a.mode == ALN_CLUSTER_GREEDY) { a.aux1[v] = 0u; a.aux2[v] = 0u; }
    a.key[v] = 0ull;
    a.size[v] = 0u;
    a.cedges[v] = 0u;
}

// ---- components (aux0 = root)
__global__ __launch_bounds__(256) void aln_cluster_hook_kernel(ClusterArgs a)
{
    uint32_t u, v;
    if (!cluster_edge(a, cluster_index(), &u, &v)) return;
    const uint32_t ru = a.aux0[u], rv = a.aux0[v];
    if (ru == rv || ru >= a.n || rv >= a.n) return;
    atomicMin(&a.label[ru > rv ? ru : rv], ru < rv ? ru : rv);
    a.misc[0] = 1u;
}
__global__ __launch_bounds__(256) void aln_cluster_compress_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    if (v >= a.n) return;
    uint32_t r = a.label[v];
    if (r >= a.n) return;                             // not a node
    for (uint64_t step = 0; step < a.n; ++step) {     // (labels fall strictly along a chain: it ends within n steps)
        const uint32_t up = a.label[r];
        if (up == r || up >= a.n) break;
        r = up;
    }
    a.aux0[v] = r;
}
__global__ __launch_bounds__(256) void aln_cluster_settle_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    if (v < a.n) a.label[v] = a.aux0[v];
}

// ---- greedy (aux0 = state, aux1 = mark, aux2 = block)
__device__ __forceinline__ bool cluster_ordered(const ClusterArgs &a, uint64_t k, uint32_t *first, uint32_t *second)
{
    uint32_t u, v;
    if (!cluster_edge(a, k, &u, &v)) return false;
    const bool uv = aln_cluster_before(cluster_len(a, u), u, cluster_len(a, v), v);
    *first = uv ? u : v; *second = uv ? v : u;
    return true;
}
__global__ __launch_bounds__(256) void aln_cluster_greedy_edge_kernel(ClusterArgs a)
{
    uint32_t p, s;
    if (!cluster_ordered(a, cluster_index(), &p, &s)) return;
    if (a.aux0[s] != CLUSTER_UNDECIDED) return;
    const uint32_t sp = a.aux0[p];
    if (sp == CLUSTER_REP) a.aux1[s] = 1u;
    else if (sp == CLUSTER_UNDECIDED) a.aux2[s] = 1u;
}
__global__ __launch_bounds__(256) void aln_cluster_greedy_node_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    bool open = false;
    if (v < a.n && a.aux0[v] == CLUSTER_UNDECIDED) {
        if (a.aux1[v]) a.aux0[v] = CLUSTER_MEMBER;
        else if (!a.aux2[v]) a.aux0[v] = CLUSTER_REP;
        else open = true;
        a.aux1[v] = 0u; a.aux2[v] = 0u;
    }
    const uint32_t c = (uint32_t)__syncthreads_count(open);
    if (threadIdx.x == 0 && c) atomicAdd(&a.misc[0], c);
}
__global__ __launch_bounds__(256) void aln_cluster_greedy_assign_kernel(ClusterArgs a)
{
    uint32_t p, s;
    if (!cluster_ordered(a, cluster_index(), &p, &s)) return;
    if (a.aux0[p] == CLUSTER_REP && a.aux0[s] == CLUSTER_MEMBER)
        atomicMax(reinterpret_cast<unsigned long long *>(&a.key[s]), (unsigned long long)aln_cluster_key(cluster_len(a, p), p));
}
__global__ __launch_bounds__(256) void aln_cluster_greedy_label_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    if (v >= a.n) return;
    const uint32_t st = a.aux0[v];
    if (st == CLUSTER_MEMBER) {
        const uint32_t r = aln_cluster_key_index(a.key[v]);
        a.label[v] = r < a.n ? r : (uint32_t)v;       // (a member has an adjacent representative: its key is set)
    }
    a.key[v] = 0ull;                                   // the finish keys this table by label
}

// ---- finish.  misc: [2..3] edges, [4..5] self edges, [6..7] singletons (64-bit words)
__global__ __launch_bounds__(256) void aln_cluster_tally_nodes_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    if (v >= a.n) return;
    const uint32_t l = a.label[v];
    if (l >= a.n) return;
    atomicAdd(&a.size[l], 1u);
    atomicMax(reinterpret_cast<unsigned long long *>(&a.key[l]), (unsigned long long)aln_cluster_key(cluster_len(a, (uint32_t)v), (uint32_t)v));
}
__global__ __launch_bounds__(256) void aln_cluster_tally_edges_kernel(ClusterArgs a)
{
    const uint64_t k = cluster_index();
    bool self = false, real = false;
    if (k < a.m) {
        const uint32_t u = a.ea[k], v = a.eb[k];
        if (u < a.n && v < a.n) {
            self = u == v;
            real = !self;
            if (real) {
                const uint32_t lu = a.label[u];
                if (lu == a.label[v] && lu < a.n) atomicAdd(&a.cedges[lu], 1u);
            }
        }
    }
    const uint32_t n_real = (uint32_t)__syncthreads_count(real);
    const uint32_t n_self = (uint32_t)__syncthreads_count(self);
    if (threadIdx.x == 0) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(a.misc);
        if (n_real) atomicAdd(&w[1], (unsigned long long)n_real);
        if (n_self) atomicAdd(&w[2], (unsigned long long)n_self);
    }
}
__global__ __launch_bounds__(256) void aln_cluster_singletons_kernel(ClusterArgs a)
{
    const uint64_t v = cluster_index();
    const bool one = v < a.n && a.label[v] == (uint32_t)v && a.size[v] == 1u;
    const uint32_t c = (uint32_t)__syncthreads_count(one);
    if (threadIdx.x == 0 && c) atomicAdd(&reinterpret_cast<unsigned long long *>(a.misc)[3], (unsigned long long)c);
}

// the cluster list (aln_select.h): node i heads a cluster iff it is its own label; cluster o of the list is its record
struct ClusterKeep {
    const uint32_t *label;
    __device__ bool operator()(uint64_t i) const { return label[i] == (uint32_t)i; }
};
struct ClusterEmit {
    const uint32_t *size, *cedges;
    const uint64_t *key;
    uint64_t cap;
    aln_cluster_record *out;
    __device__ void operator()(uint32_t o, uint64_t i) const
    {
        if (o >= cap) return;
        aln_cluster_record r;
        r.label = (uint32_t)i; r.size = size[i]; r.longest = aln_cluster_key_index(key[i]); r.edges = cedges[i];
        out[o] = r;
    }
};

static inline uint32_t cluster_blocks(uint64_t n) { return blocks_of(n, ALN_CLUSTER_THREADS); }
#define CLUSTER_LAUNCH(kernel, count) \
    do { if (count) hipLaunchKernelGGL(kernel, dim3(cluster_blocks(count)), dim3(ALN_CLUSTER_THREADS), 0, s, *a); } while (0)

extern "C" void aln_cluster_launch_held_edges(const aln_pair_result *res, const aln_hit_report *rep, const HeldEntry *held,
                                              const aln_hit_filter *filter, uint64_t m, uint32_t *ea, uint32_t *eb, hipStream_t s)
{
    aln_hit_filter f = {0.0, 0.0, 0.0, 0u, 0u};
    if (filter) f = *filter;
    if (m) hipLaunchKernelGGL(aln_cluster_held_edges_kernel, dim3(cluster_blocks(m)), dim3(ALN_CLUSTER_THREADS), 0, s, res, filter ? rep : nullptr, held, f, m, ea, eb);
}
extern "C" void aln_cluster_launch_init(const ClusterArgs *a, hipStream_t s) { CLUSTER_LAUNCH(aln_cluster_init_kernel, a->n); }
extern "C" void aln_cluster_launch_hook(const ClusterArgs *a, hipStream_t s) { CLUSTER_LAUNCH(aln_cluster_hook_kernel, a->m); }
extern "C" void aln_cluster_launch_compress(const ClusterArgs *a, hipStream_t s)
{
    CLUSTER_LAUNCH(aln_cluster_compress_kernel, a->n);
    CLUSTER_LAUNCH(aln_cluster_settle_kernel, a->n);
}
extern "C" void aln_cluster_launch_greedy_round(const ClusterArgs *a, hipStream_t s)
{
    CLUSTER_LAUNCH(aln_cluster_greedy_edge_kernel, a->m);
    CLUSTER_LAUNCH(aln_cluster_greedy_node_kernel, a->n);
}
extern "C" void aln_cluster_launch_greedy_assign(const ClusterArgs *a, hipStream_t s)
{
    CLUSTER_LAUNCH(aln_cluster_greedy_assign_kernel, a->m);
    CLUSTER_LAUNCH(aln_cluster_greedy_label_kernel, a->n);
}
// tile_count / tile_off: aln_cluster_tiles(n) words each; count[0]: the clusters in all; out: cap records
extern "C" uint64_t aln_cluster_tiles(uint64_t n) { return aln_select_tiles(n); }
extern "C" void aln_cluster_launch_finish(const ClusterArgs *a, uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint64_t cap,
                                          aln_cluster_record *out, hipStream_t s)
{
    CLUSTER_LAUNCH(aln_cluster_tally_nodes_kernel, a->n);
    CLUSTER_LAUNCH(aln_cluster_tally_edges_kernel, a->m);
    CLUSTER_LAUNCH(aln_cluster_singletons_kernel, a->n);
    aln_select_launch(ClusterKeep{a->label}, ClusterEmit{a->size, a->cedges, a->key, cap, out}, a->n, tile_count, tile_off, count, s);
}
