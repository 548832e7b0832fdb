// aln_seqset.hip -- device side of the resident sequence set (aln_seqset_*, include/aligner_hip.h): the kernels that stand between
// S resident sequences and the existing fill / traceback machinery of aln_kernels.hip.
//
//   expand     pairs k0 .. k0 + n - 1 of a block of the S x S grid (aln_seqset_rules.h) -> PairDesc 0 .. n - 1 of a chunk (+ the queue
//              entries 0 .. n - 1): offsets and lengths out of the resident tables, built where they are used.  k is 64-bit (a block
//              may hold more than 2^32 pairs); descriptor and queue entry are chunk-local
//   gather     f and status of every pair of the chunk out of the 48-byte summaries (8 + 4 bytes per pair go back instead of 48), and
//              the first failed pair of the chunk as one word
//   select     status == ALN_OK and f >= f_min per pair, compacted in ascending pair order by the shared two-level prefix sum
//              (aln_select.h; a predicate and an emitter here): the same list every run, no atomic appends
//
// (The held hits' strings are fetched by the held store's gather, aln_pairset.hip.)
// Every store is a plain C++ store or an atomicMax of a thread (vector memory instructions).  The threshold test is a plain IEEE
// compare: a NaN f_min (or f) fails it.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_select.h"
#include "aln_seqset_rules.h"

// ---- descriptor i of the chunk = pair k0 + i of the block (an empty query or target: the reference panics, ALN_ERR_EMPTY_SEQUENCE
// as in chunk_plan)
__global__ __launch_bounds__(256) void aln_seqset_expand_kernel(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t k0,
                                                                aln_seqset_block block, const uint64_t *seq_off, const uint32_t *seq_len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t q, t;
    aln_seqset_unrank(block, k0 + i, &q, &t);
    PairDesc d;
    d.q_off = seq_off[q];
    d.t_off = seq_off[t];
    d.N = seq_len[q];
    d.M = seq_len[t];
    d.dir_off = 0; d.tb_off = 0; d.tag_off = 0; d.h_off = 0;
    d.status = (d.N == 0 || d.M == 0) ? ALN_ERR_EMPTY_SEQUENCE : ALN_OK;
    d.layout = 0;
    descs[i] = d;
    order[i] = (uint32_t)i;
}

// ---- f and status of every pair of the chunk; bad[0] = max over the failed pairs of ((2^40 - 1 - i) << 8 | status): the failed pair
// with the smallest i wins (a chunk holds at most 2^22 pairs)
__global__ __launch_bounds__(256) void aln_seqset_gather_kernel(const aln_pair_result *res, double *f, int32_t *status, uint64_t n,
                                                                unsigned long long *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const aln_pair_result r = res[i];
    f[i] = r.f;
    status[i] = r.status;
    if (r.status != ALN_OK) atomicMax(bad, (unsigned long long)((((1ull << 40) - 1ull - i) << 8) | ((uint32_t)r.status & 0xffu)));
}

__device__ __forceinline__ bool seqset_keep(const aln_pair_result &r, double f_min)
{
    return r.status == ALN_OK && r.f >= f_min;      // IEEE: false for a NaN on either side
}

// ---- selection (aln_select.h): pair k of the chunk is kept by its status and f; kept pair k goes to place o: its number in the block
// and its f (hit_k / hit_f hold n entries: every pair may pass)
struct SeqsetKeep {
    const aln_pair_result *res;
    double f_min;
    __device__ bool operator()(uint64_t k) const { return seqset_keep(res[k], f_min); }
};
struct SeqsetEmit {
    const aln_pair_result *res;
    uint64_t n, k0;
    uint64_t *hit_k;
    double *hit_f;
    __device__ void operator()(uint32_t o, uint64_t k) const { if (o < n) { hit_k[o] = k0 + k; hit_f[o] = res[k].f; } }
};

extern "C" void aln_seqset_launch_expand(PairDesc *descs, uint32_t *order, uint64_t n, uint64_t k0, const aln_seqset_block *block,
                                         const uint64_t *seq_off, const uint32_t *seq_len, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_seqset_expand_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, descs, order, n, k0, *block, seq_off, seq_len);
}

extern "C" void aln_seqset_launch_gather(const aln_pair_result *res, double *f, int32_t *status, uint64_t n, unsigned long long *bad,
                                         hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_seqset_gather_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, res, f, status, n, bad);
}

extern "C" uint64_t aln_seqset_tiles(uint64_t n) { return aln_select_tiles(n); }

// tile_count / tile_off: aln_seqset_tiles(n) words each; hit_k / hit_f: n entries each; count[0]: the chunk's hits
extern "C" void aln_seqset_launch_select(const aln_pair_result *res, uint64_t n, uint64_t k0, double f_min, uint32_t *tile_count,
                                         uint32_t *tile_off, uint32_t *count, uint64_t *hit_k, double *hit_f, hipStream_t s)
{
    aln_select_launch(SeqsetKeep{res, f_min}, SeqsetEmit{res, n, k0, hit_k, hit_f}, n, tile_count, tile_off, count, s);
}
